"""Host (no GPU): what tests/test_gpu_conv_kernels.py rests on.

1. tests/conv_ref.py equals torch.nn.functional.conv2d in float64 and its autograd input / weight gradients to 1e-12 (relative to the largest magnitude), at every shape the
   GPU tests use.
2. The reference alone stays inside its bound: an fp32 numpy evaluation that sums the taps (frames, for a weight gradient) in the opposite order differs from the float64 one
   by at most `bound`, element by element.
3. The inputs bite: seven deliberate mistakes, each applied to a copy of the reference, each more than the GPU tests' tolerance off in at least one element at every case
   where the mistake is possible — the evidence that the GPU tests would notice a subtly wrong kernel.  Truncation is measured against conv_inputs.tol16_nearest (half an
   ulp, which the GPU tests assert too): a truncated value is less than one whole ulp from the exact one, so `bound + one ulp` cannot see it by construction.
Also: the inputs are exactly representable in their storage type, the fp16 variants keep every reference accumulator below 65504 and every nonzero input at or above 2^-14,
and the mask values carry every kind in both halves of every packed pair."""
import numpy as np
import pytest
import torch

import conv_inputs as CI
import conv_ref as CR
from plan_ln_inputs import round_t

MAX_SLABS = 512          # no weight-gradient launch of the entries writes more partial slabs: the mistakes are measured against the bound of that many
FD = [pytest.param(*c, id=f"conv{c[0]}-{c[1]}x{c[2]}") for c in CI.FD_CASES]
WG_ALL = sorted(set(CI.WG_CASES) | {(l, CI.WG_PAIR_SIDES[l][k], fr[k]) for l in (3, 2) for fr in CI.WG_PAIR_FRAMES for k in (0, 1)})
WG = [pytest.param(*c, id=f"conv{c[0]}-{c[1]}x{c[2]}") for c in WG_ALL]
C1 = [pytest.param(*c, id=f"{c[0]}x{c[1]}") for c in CI.C1_CASES]
C1_WG = sorted(set(CI.C1_CASES) | {(CI.WG_PAIR_SIDES[1][k], fr[k]) for fr in CI.WG_PAIR_FRAMES for k in (0, 1)})


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _torch_conv(X, W, b, stride, dY):
    """float64 torch: pre-ReLU output, relu output, input gradient and weight / bias gradient of dY"""
    x = _t(X.transpose(0, 3, 1, 2)).requires_grad_(True)
    w = _t(W).requires_grad_(True)
    bb = _t(b).requires_grad_(True)
    y = torch.nn.functional.conv2d(x, w, bb, stride=stride)
    y.backward(_t(dY.transpose(0, 3, 1, 2)))
    return (torch.relu(y).detach().numpy().transpose(0, 2, 3, 1), x.grad.numpy().transpose(0, 2, 3, 1), w.grad.numpy(), bb.grad.numpy())


def _close(a, b, what):
    assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300), (what, float(np.abs(a - b).max()), float(np.abs(b).max()))


def _exceeds(wrong, ref, tol, what):
    over = np.abs(wrong - ref) > tol
    assert over.any(), f"{what}: the mistake stays inside the tolerance everywhere"


def trunc_t(x, dtype):
    """x truncated (toward zero) to the storage type"""
    r = round_t(x, dtype)
    over = np.abs(r) > np.abs(x)
    if dtype == "fp16":
        down = np.nextafter(r.astype(np.float16), np.float16(0)).astype(np.float64)
    else:
        down = ((r.astype(np.float32).view(np.uint32) - np.uint32(0x10000)).view(np.float32)).astype(np.float64)          # one bf16 step toward zero
    return np.where(over, down, r)


# ==================================================================================================== 1. the reference is torch's convolution
@pytest.mark.parametrize("layer,side,frames", FD)
def test_reference_equals_torch_forward_and_data_gradient(layer, side, frames):
    g = CI.LAYERS[layer]
    for dtype in CI.DTYPES16:
        X, dY = CI.acts(layer, side, frames, dtype)
        W, b = CI.weights(layer, dtype)
        out, dx, dw, db = _torch_conv(X, W, b, g["s"], dY)
        _close(CI.fwd_ref(layer, side, frames, dtype)[0], out, "fwd")
        keep = CI.mask_keep(CI.mask_values(layer, side, frames, dtype)[0])
        _close(CI.dgrad_ref(layer, side, frames, dtype, keep)[0], dx * keep, "dgrad")
        _close(CI.dgrad_ref_unmasked(layer, side, frames, dtype)[0], dx, "dgrad unmasked")


@pytest.mark.parametrize("layer,side,frames", WG)
def test_reference_equals_torch_weight_gradient(layer, side, frames):
    g = CI.LAYERS[layer]
    for dtype in CI.DTYPES16:
        X, dY = CI.acts(layer, side, frames, dtype)
        W, b = CI.weights(layer, dtype)
        _, _, dw, db = _torch_conv(X, W, b, g["s"], dY)
        dW, dB, _, _ = CI.wgrad_ref(layer, side, frames, dtype)
        _close(dW, dw, "wgrad")
        _close(dB, db, "bias grad")


@pytest.mark.parametrize("side,frames", C1)
def test_reference_equals_torch_conv1(side, frames):
    pad = CI.c1_pad(side)
    for dtype in CI.DTYPES16:
        Xf, u8, sh, dY = CI.c1_inputs(side, frames, dtype)
        W, b = CI.weights(1, dtype)
        for src in ("f32", "u8", "u8s"):
            x = CI.c1_frames16(side, frames, dtype, src)
            out, _, dw, db = _torch_conv(x, W, b, 4, dY)
            _close(CI.c1_fwd_ref(side, frames, dtype, src)[0], out, "conv1 fwd " + src)
            dW, dB, _, _ = CI.c1_wgrad_ref(side, frames, dtype, src)
            _close(dW, dw, "conv1 wgrad " + src)
            _close(dB, db, "conv1 bias grad " + src)
        # the shifted frames are torch's replicate pad + crop, the folded reference is the convolution of the exact x = u (2/255) - 1
        padded = torch.nn.functional.pad(_t(u8.astype(np.float64)).permute(0, 3, 1, 2), (pad,) * 4, mode="replicate").permute(0, 2, 3, 1).numpy()
        us = CR.shift_frames(u8, sh, pad)
        for f in range(frames):
            assert np.array_equal(us[f], padded[f, sh[f, 1]:sh[f, 1] + side, sh[f, 0]:sh[f, 0] + side])
        _, _, dw, _ = _torch_conv(us.astype(np.float64) * (2.0 / 255.0) - 1.0, W, b, 4, dY)
        _close(CI.c1_wgrad_ref(side, frames, dtype, "u8s", 1)[0], dw, "conv1 folded wgrad")
        exact, fma32 = CR.u8_values(np.arange(256, dtype=np.uint8))
        assert np.abs(fma32 - exact).max() <= 2.0 ** -22          # the rounding of 2/255 to fp32 (255 x 2/255 x 2^-24) and of the result


# ==================================================================================================== 2. the reference stays inside its own bound
@pytest.mark.parametrize("layer,side,frames", FD)
def test_fp32_evaluation_in_another_order_stays_inside_the_bound(layer, side, frames):
    g = CI.LAYERS[layer]
    for dtype in CI.DTYPES16:
        X, dY = CI.acts(layer, side, frames, dtype)
        W, b = CI.weights(layer, dtype)
        ref, bound = CI.fwd_ref(layer, side, frames, dtype)
        got = CR.fwd(X, W, b, g["s"], np.float32, -1)[0].astype(np.float64)
        assert (np.abs(got - ref) <= bound).all(), ("fwd", float((np.abs(got - ref) / bound).max()))
        keep = CI.keep_bits(layer, side, frames)
        ref, bound = CI.dgrad_ref(layer, side, frames, dtype, keep)
        got = CR.dgrad(dY, W, g["s"], side, keep, np.float32, -1)[0].astype(np.float64)
        assert (np.abs(got - ref) <= bound).all(), "dgrad"
        reach = (side - g["k"]) // g["s"] * g["s"] + g["k"]          # rows / columns past `reach` (an odd side under stride 2) get no gradient at all: bound 0 there too
        assert (got[~keep] == 0).all() and (bound[~keep] == 0).all() and (bound[:, :reach, :reach][keep[:, :reach, :reach]] > 0).all() and (ref[:, reach:] == 0).all()


@pytest.mark.parametrize("layer,side,frames", WG)
def test_fp32_weight_gradient_in_another_order_stays_inside_the_bound(layer, side, frames):
    g = CI.LAYERS[layer]
    for dtype in CI.DTYPES16:
        X, dY = CI.acts(layer, side, frames, dtype)
        dW, db, bw, bb = CI.wgrad_ref(layer, side, frames, dtype)
        gW, gb, _, _ = CR.wgrad(X, dY, g["k"], g["s"], 0, np.float32, -1)
        assert (np.abs(gW - dW) <= bw).all() and (np.abs(gb - db) <= bb).all()


@pytest.mark.parametrize("side,frames", C1)
def test_fp32_conv1_in_another_order_stays_inside_the_bound(side, frames):
    for dtype in CI.DTYPES16:
        _, u8, sh, dY = CI.c1_inputs(side, frames, dtype)
        W, b = CI.weights(1, dtype)
        x = CI.c1_frames16(side, frames, dtype, "u8s")
        ref, bound = CI.c1_fwd_ref(side, frames, dtype, "u8s")
        assert (np.abs(CR.fwd(x, W, b, 4, np.float32, -1)[0] - ref) <= bound).all()
        dW, db, bw, bb = CI.c1_wgrad_ref(side, frames, dtype, "u8s")
        gW, gb, _, _ = CR.wgrad(x, dY, 8, 4, 0, np.float32, -1)
        assert (np.abs(gW - dW) <= bw).all() and (np.abs(gb - db) <= bb).all()
        # the fold in fp32: (2/255) (dY * u) - db against the exact-x reference
        dWf, _, bwf, _ = CI.c1_wgrad_ref(side, frames, dtype, "u8s", 1)
        us = CR.shift_frames(u8, sh, CI.c1_pad(side)).astype(np.float32)
        raw, gb32, _, _ = CR.wgrad(us, dY, 8, 4, 0, np.float32, -1)
        fold = raw * np.float32(CR.U8_SCALE) - gb32[:, None, None, None]
        assert (np.abs(fold - dWf) <= bwf).all()


# ==================================================================================================== 3. the inputs bite
def _drop_row_block(X, dY, k, s):
    """the contribution of one slab to dW: frame 0 where there are several frames, else the upper half of the only frame's output rows"""
    if X.shape[0] > 1:
        return CR.wgrad_frames(X, dY, k, s, [0])
    r = dY.shape[1] // 2
    return CR.wgrad_frames(X[:, :(r - 1) * s + k], dY[:, :r], k, s, [0])


@pytest.mark.parametrize("layer,side,frames", FD)
def test_mistakes_exceed_the_tolerance_forward_and_data_gradient(layer, side, frames):
    g = CI.LAYERS[layer]
    k, s = g["k"], g["s"]
    small = int(np.argmin(CI.grade(g["co"])))
    for dtype in CI.DTYPES16:
        X, dY = CI.acts(layer, side, frames, dtype)
        W, b = CI.weights(layer, dtype)
        ref, bound = CI.fwd_ref(layer, side, frames, dtype)
        tol = CI.tol16(ref, bound, dtype)
        # one tap dropped at a border pixel: pixel (0, 0) of frame 0 without tap (0, 0)
        acc = CR._corr(X[:1, :k, :k], W, s)[0, 0, 0]
        wrong = ref.copy()
        wrong[0, 0, 0] = np.maximum(acc - W[:, :, 0, 0] @ X[0, 0, 0] + b, 0)
        _exceeds(wrong, ref, tol, "fwd: tap dropped")
        _exceeds(CR.fwd(X, W.transpose(0, 1, 3, 2), b, s)[0], ref, tol, "fwd: kh and kw swapped")
        b0 = b.copy(); b0[small] = 0.0
        wrong = CR.fwd(X, W, b0, s)[0]
        assert (wrong[..., [c for c in range(g["co"]) if c != small]] == ref[..., [c for c in range(g["co"]) if c != small]]).all()
        _exceeds(wrong, ref, tol, "fwd: bias missing on the smallest-scale channel")
        _exceeds(trunc_t(ref, dtype), ref, CI.tol16_nearest(ref, bound, dtype), "fwd: output truncated")
        assert (np.abs(round_t(ref, dtype) - ref) <= CI.tol16_nearest(ref, bound, dtype)).all()          # ... and rounding to nearest is inside it
        if frames > 1:
            wrong = ref.copy(); wrong[-1, -1] = ref[-2, -1]
            _exceeds(wrong, ref, tol, "fwd: last frame takes its neighbour's border row")
        # ---- data gradient, 16-bit mask values and bit words
        vals, kind = CI.mask_values(layer, side, frames, dtype)
        for keep, what in ((CI.mask_keep(vals), "values"), (CI.keep_bits(layer, side, frames), "bits")):
            ref, bound = CI.dgrad_ref(layer, side, frames, dtype, keep)
            tol = CI.tol16(ref, bound, dtype, keep)
            assert keep[0, 0, 0].any()
            wrong = ref.copy(); wrong[0, 0, 0] = 0.0          # pixel (0, 0) is reached by tap (0, 0) alone
            _exceeds(wrong, ref, tol, f"dgrad {what}: tap dropped")
            _exceeds(CR.dgrad(dY, W.transpose(0, 1, 3, 2), s, side, keep)[0], ref, tol, f"dgrad {what}: kh and kw swapped")
            _exceeds(trunc_t(ref, dtype), ref, CI.tol16_nearest(ref, bound, dtype, keep), f"dgrad {what}: output truncated")
            assert (np.abs(round_t(ref, dtype) - ref) <= CI.tol16_nearest(ref, bound, dtype, keep)).all()
            if frames > 1:
                wrong = ref.copy(); wrong[-1, 0] = ref[-2, 0]
                _exceeds(wrong, ref, tol, f"dgrad {what}: last frame takes its neighbour's border row")
        keep = CI.mask_keep(vals)
        ref, bound = CI.dgrad_ref(layer, side, frames, dtype, keep)
        tol = CI.tol16(ref, bound, dtype, keep)
        for zero, name in ((0, "+0.0"), (1, "-0.0")):
            assert (vals[kind == zero] == 0).all() and (np.signbit(vals[kind == zero]) == bool(zero)).all()
            wrong = CI.dgrad_ref(layer, side, frames, dtype, keep | (kind == zero))[0]
            _exceeds(wrong, ref, tol, f"dgrad: {name} treated as > 0")


@pytest.mark.parametrize("layer,side,frames", WG)
def test_mistakes_exceed_the_tolerance_weight_gradient(layer, side, frames):
    g = CI.LAYERS[layer]
    K = frames * CR.out_side(side, g["k"], g["s"]) ** 2
    for dtype in CI.DTYPES16:
        X, dY = CI.acts(layer, side, frames, dtype)
        dW, db, bw, bb = CI.wgrad_ref(layer, side, frames, dtype)
        tol = CI.wgrad_bound(bw, K, MAX_SLABS)
        _exceeds(dW.transpose(0, 1, 3, 2), dW, tol, "wgrad: kh and kw swapped")
        _exceeds(dW - _drop_row_block(X, dY, g["k"], g["s"]), dW, tol, "wgrad: one slab left out")


@pytest.mark.parametrize("side,frames", C1_WG)
def test_mistakes_exceed_the_tolerance_conv1(side, frames):
    small = int(np.argmin(CI.grade(32)))
    K = frames * CR.out_side(side, 8, 4) ** 2
    for dtype in CI.DTYPES16:
        _, _, _, dY = CI.c1_inputs(side, frames, dtype)
        W, b = CI.weights(1, dtype)
        for src in ("f32", "u8s"):
            x = CI.c1_frames16(side, frames, dtype, src)
            ref, bound = CI.c1_fwd_ref(side, frames, dtype, src)
            tol = CI.tol16(ref, bound, dtype)
            acc = CR._corr(x[:1, :8, :8], W, 4)[0, 0, 0]
            wrong = ref.copy(); wrong[0, 0, 0] = np.maximum(acc - W[:, :, 0, 0] @ x[0, 0, 0] + b, 0)
            _exceeds(wrong, ref, tol, "conv1 fwd: tap dropped")
            _exceeds(CR.fwd(x, W.transpose(0, 1, 3, 2), b, 4)[0], ref, tol, "conv1 fwd: kh and kw swapped")
            b0 = b.copy(); b0[small] = 0.0
            _exceeds(CR.fwd(x, W, b0, 4)[0], ref, tol, "conv1 fwd: bias missing on the smallest-scale channel")
            _exceeds(trunc_t(ref, dtype), ref, CI.tol16_nearest(ref, bound, dtype), "conv1 fwd: output truncated")
            for fold in ((0, 1) if src == "u8s" else (0,)):
                dW, db, bw, bb = CI.c1_wgrad_ref(side, frames, dtype, src, fold)
                tolw = CI.wgrad_bound(bw, K, MAX_SLABS)
                _exceeds(dW.transpose(0, 1, 3, 2), dW, tolw, "conv1 wgrad: kh and kw swapped")
                _exceeds(dW - _drop_row_block(x, dY, 8, 4), dW, tolw, "conv1 wgrad: one slab left out")
        ref, bound = CI.c1_fwd_ref(side, frames, dtype, "u8s")          # a shift ignored (frame 0 carries one) is a mistake the uint8 cases see
        _exceeds(CI.c1_fwd_ref(side, frames, dtype, "u8")[0], ref, CI.tol16(ref, bound, dtype), "conv1 fwd: shifts ignored")


# ==================================================================================================== the inputs themselves
@pytest.mark.parametrize("dtype", CI.DTYPES16)
def test_inputs_are_representable_graded_and_safe_in_fp16(dtype):
    gr = CI.grade(64)
    assert gr.min() == 2.0 ** -6 and gr.max() == 1.0 and (np.maximum(gr[1:] / gr[:-1], gr[:-1] / gr[1:]) >= 10).all() and max(gr[0] / gr[-1], gr[-1] / gr[0]) >= 10
    for layer, side, frames in sorted(set(CI.FD_CASES) | set(WG_ALL)):
        X, dY = CI.acts(layer, side, frames, dtype)
        W, _ = CI.weights(layer, dtype)
        for a in (X, dY, W):
            assert np.array_equal(round_t(a, dtype), a)
            if dtype == "fp16":
                assert np.abs(a[a != 0]).min() >= 2.0 ** -14 and np.abs(a).max() < CI.FP16_MAX
        assert (X == 0).mean() > 0.2          # exact zeros, as a post-ReLU activation has them
        if dtype == "fp16":
            assert np.abs(dY).max() > 64          # the loss scale is in
            if (layer, side, frames) in CI.FD_CASES:
                assert np.abs(CI.fwd_ref(layer, side, frames, dtype)[0]).max() < CI.FP16_MAX
                assert np.abs(CI.dgrad_ref_unmasked(layer, side, frames, dtype)[0]).max() < CI.FP16_MAX
            else:
                assert np.abs(CI.wgrad_ref(layer, side, frames, dtype)[0]).max() < CI.FP16_MAX
    for side, frames in C1_WG:
        Xf, u8, sh, dY = CI.c1_inputs(side, frames, dtype)
        pad = CI.c1_pad(side)
        assert np.array_equal(round_t(dY, dtype), dY) and (frames < 2 or {0, pad, 2 * pad} <= set(sh.reshape(-1).tolist())) and sh.min() >= 0 and sh.max() <= 2 * pad
        if dtype == "fp16":
            assert np.abs(dY[dY != 0]).min() >= 2.0 ** -14 and np.abs(CI.c1_fwd_ref(side, frames, dtype, "f32")[0]).max() < CI.FP16_MAX
            assert np.abs(CI.c1_wgrad_ref(side, frames, dtype, "u8s", 1)[0]).max() < CI.FP16_MAX


@pytest.mark.parametrize("dtype", CI.DTYPES16)
def test_mask_values_carry_every_kind_in_both_halves_of_every_pair(dtype):
    for layer, side, frames in CI.FD_CASES:
        vals, kind = CI.mask_values(layer, side, frames, dtype)
        assert np.array_equal(round_t(vals, dtype), vals) and np.array_equal(np.signbit(round_t(vals, dtype)), np.signbit(vals))          # the subnormals and -0.0 survive the storage type
        sub = CI.SUBNORMAL[dtype]
        assert (vals[kind == 2] == sub).all() and (vals[kind == 3] == -sub).all() and (vals[kind == 4] >= 0.25).all() and (vals[kind == 5] <= -0.25).all()
        per_channel = np.stack([(kind == q).reshape(-1, kind.shape[-1]).any(0) for q in range(6)])
        assert per_channel.all(), "a channel (a half of a packed pair) misses a kind"
        keep = CI.mask_keep(vals)
        assert keep[kind == 2].all() and not keep[kind <= 1].any() and not keep[kind == 3].any()
    words = CR.pack_bits(CI.keep_bits(3, 9, 1))
    assert words.shape == (1, 9, 9, 2) and np.array_equal(CR.unpack_bits(words, 64), CI.keep_bits(3, 9, 1))
    assert CR.pack_bits(CI.keep_bits(2, 20, 1)).shape == (1, 20, 20, 1)
