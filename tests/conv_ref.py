"""float64 references of the perceptual encoders' convolutions, written from the layer definitions — nn.Conv2d(3, 32, 8, 4), nn.Conv2d(32, 64, 4, 2), nn.Conv2d(64, 64, 3, 1),
each followed by ReLU — and not from the kernels, with a per-element error bound for an fp32 evaluation, and the packers of the layouts the kernels read.

Activations are NHWC (n, h, w, c), weights are torch's (co, ci, kh, kw).  Every bound is tr_fused_ref.acc_bound(sum of |term|, K, extra): (K + 2 + extra) 2^-24 times the same
sum over absolute values, K = the products of the sum, extra = the partial slabs of a weight gradient; where a bias is added, one more fp32 operation over |acc| + |b|.
ReLU and the mask are contractions (|relu(a) - relu(b)| <= |a - b|), so the bound carries through them; where the mask is off the bound is 0: the element must be exactly 0."""
import numpy as np

from tr_fused_ref import EPS32, acc_bound


def out_side(side, k, stride):
    return (side - k) // stride + 1


def _corr(X, W, stride, dtype=np.float64, order=1):
    """sum over taps and input channels, no bias: (n, oh, ow, co).  order = -1 walks the taps backwards (another summation order)"""
    n, ih, iw, ci = X.shape
    co, _, kh, kw = W.shape
    oh, ow = out_side(ih, kh, stride), out_side(iw, kw, stride)
    out = np.zeros((n, oh, ow, co), dtype)
    taps = [(a, c) for a in range(kh) for c in range(kw)][::order]
    for a, c in taps:
        out += (X[:, a:a + stride * oh:stride, c:c + stride * ow:stride, :].astype(dtype).reshape(-1, ci) @ W[:, :, a, c].astype(dtype).T).reshape(n, oh, ow, co)
    return out


def fwd(X, W, b, stride, dtype=np.float64, order=1):
    """relu(conv(X, W) + b) -> (out, bound)"""
    K = W.shape[1] * W.shape[2] * W.shape[3]
    acc = _corr(X, W, stride, dtype, order)
    out = np.maximum(acc + np.asarray(b, dtype), 0)
    if dtype != np.float64:
        return out, None
    mag = _corr(np.abs(X), np.abs(W), stride)
    return out, acc_bound(mag, K) + EPS32 * (np.abs(acc) + np.abs(b))


def _scatter(dY, W, stride, side, dtype=np.float64, order=1):
    n, oh, ow, co = dY.shape
    _, ci, kh, kw = W.shape
    dX = np.zeros((n, side, side, ci), dtype)
    taps = [(a, c) for a in range(kh) for c in range(kw)][::order]
    for a, c in taps:
        dX[:, a:a + stride * oh:stride, c:c + stride * ow:stride, :] += (dY.astype(dtype).reshape(-1, co) @ W[:, :, a, c].astype(dtype)).reshape(n, oh, ow, ci)
    return dX


def dgrad(dY, W, stride, side, keep, dtype=np.float64, order=1):
    """the gradient of the layer input (side x side), kept where `keep` (boolean, the ReLU of the layer below) -> (dX, bound).  K = the taps that can reach an input
    pixel x the output channels (the kernels multiply the zero border too)"""
    co, _, kh, kw = W.shape
    K = co * (-(-kh // stride)) * (-(-kw // stride))
    dX = np.where(keep, _scatter(dY, W, stride, side, dtype, order), 0)
    if dtype != np.float64:
        return dX, None
    return dX, np.where(keep, acc_bound(_scatter(np.abs(dY), np.abs(W), stride, side), K), 0.0)


def _wcorr(X, dY, k, stride, dtype=np.float64, order=1):
    n, oh, ow, co = dY.shape
    ci = X.shape[3]
    dW = np.zeros((co, ci, k, k), dtype)
    fr = list(range(n))[::order]
    for a in range(k):
        for c in range(k):
            for f in fr:          # frame by frame: `order` changes the order of the partial sums
                dW[:, :, a, c] += dY[f].astype(dtype).reshape(-1, co).T @ X[f, a:a + stride * oh:stride, c:c + stride * ow:stride, :].astype(dtype).reshape(-1, ci)
    return dW


def wgrad(X, dY, k, stride, slabs, dtype=np.float64, order=1):
    """-> (dW (co, ci, k, k), db (co), bound_w, bound_b); slabs = the partial slabs the device summed"""
    n, oh, ow, co = dY.shape
    K = n * oh * ow
    dW = _wcorr(X, dY, k, stride, dtype, order)
    db = dY.astype(dtype).sum((0, 1, 2))
    if dtype != np.float64:
        return dW, db, None, None
    return dW, db, acc_bound(_wcorr(np.abs(X), np.abs(dY), k, stride), K, slabs), acc_bound(np.abs(dY).sum((0, 1, 2)), K, slabs)


def wgrad_frames(X, dY, k, stride, frames):
    """the contribution of `frames` to dW: what a slab that holds them carries"""
    return _wcorr(X[frames], dY[frames], k, stride)


# ---------------------------------------------------------------------------------------------------- layouts
def pack_fwd(W):
    """[co][(kh, kw, ci)]: the forward weights, and the order of the conv2 / conv3 weight gradients"""
    return np.ascontiguousarray(W.transpose(0, 2, 3, 1)).reshape(W.shape[0], -1)


def pack_c1(W):
    """conv1: [co][(ci, kh, kw)] = torch's own order"""
    return np.ascontiguousarray(W).reshape(W.shape[0], -1)


def pack_dgrad(W, stride):
    """per-parity [class][ci][(a, b, co)], class = (kh % s) s + kw % s, tap (a, b) = (kh // s, kw // s)"""
    co, ci, kh, kw = W.shape
    t = kh // stride
    wd = np.zeros((stride * stride, ci, t, t, co))
    for a in range(kh):
        for c in range(kw):
            wd[(a % stride) * stride + c % stride, :, a // stride, c // stride, :] = W[:, :, a, c].T
    return wd.reshape(stride * stride * ci, -1)


def pack_bits(keep):
    """ReLU bit words of (n, h, w, C) booleans: bit c % 32 of word c // 32, C / 32 words per pixel (2 for 64 channels, 1 for 32), as int32"""
    n, h, w, C = keep.shape
    b = keep.reshape(n, h, w, C // 32, 32).astype(np.uint64)
    return np.ascontiguousarray((b << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32).view(np.int32))


def unpack_bits(words, C):
    """the inverse of pack_bits: words (n, h, w, C / 32) int32 -> (n, h, w, C) booleans"""
    u = np.ascontiguousarray(words).view(np.uint32).astype(np.uint64)
    return ((u[..., None] >> np.arange(32, dtype=np.uint64)) & 1).astype(bool).reshape(words.shape[:3] + (C,))


U8_SCALE = float(np.float32(2.0) / np.float32(255.0))          # ScaleImageTensor + Normalize(0.5, 0.5): x = u (2 / 255) - 1


def shift_frames(u8, shifts, pad):
    """RandomShiftsAug on uint8 NHWC frames: replicate-pad by `pad`, one integer shift (sx, sy) in [0, 2 pad] per frame: out[y][x] = in[clamp(y + sy - pad)][clamp(x + sx - pad)]"""
    n, h, w, _ = u8.shape
    out = np.empty_like(u8)
    for f in range(n):
        ys = np.clip(np.arange(h) + int(shifts[f, 1]) - pad, 0, h - 1)
        xs = np.clip(np.arange(w) + int(shifts[f, 0]) - pad, 0, w - 1)
        out[f] = u8[f][ys][:, xs]
    return out


def u8_values(u8):
    """the exact value x = u (2 / 255) - 1 of a byte, and the value an fp32 fused multiply-add gives (what is then rounded to the storage type)"""
    exact = u8.astype(np.float64) * (2.0 / 255.0) - 1.0
    fma32 = (u8.astype(np.float64) * U8_SCALE - 1.0).astype(np.float32).astype(np.float64)          # u * fp32(2/255) is exact in float64: one rounding, as an fma
    return exact, fma32
