"""Inputs and case lists shared by tests/test_gpu_conv_kernels.py (GPU) and tests/test_conv_ref_host.py (host), already rounded to the storage type
(plan_ln_inputs.round_t) and built from fixed seeds (hulc_amd.utils.portable_rng).

Graded magnitudes: every element is +-[0.25, 1) times a per-channel power of two.  Output channels walk GRADE = 2^0, 2^-4, 2^0, 2^-5, 2^-1, 2^-6, 2^-2, 2^-6 (neighbours
at least 16 x apart, 2^-6 .. 2^0 over all), input channels alternate 2^0, 2^-4 — so a per-element tolerance bites on the small channels, where a gate relative to the
largest output sees nothing.  The smallest nonzero input is 0.25 * 2^-6 * 2^-4 = 2^-12 >= 2^-14 (normal in fp16)."""
import functools

import numpy as np

import conv_ref as CR
from hulc_amd.utils import portable_rng as prng
from plan_ln_inputs import ULP, frozen, round_t

DTYPES16 = ("bf16", "fp16")
SUBNORMAL = {"bf16": 2.0 ** -133, "fp16": 2.0 ** -24}          # the smallest positive subnormal of the storage type
LOSS_SCALE = 256.0          # the fp16 engine tests' loss scale: the fp16 variant of dY carries it
FP16_MAX = 65504.0
LAYERS = {1: dict(ci=3, co=32, k=8, s=4), 2: dict(ci=32, co=64, k=4, s=2), 3: dict(ci=64, co=64, k=3, s=1)}
GRADE = np.array([0, -4, 0, -5, -1, -6, -2, -6])
GRADE_IN = np.array([0, -4])

# (layer, layer-input side, frames): forward and data gradient.  conv3: 9 = the gripper camera (stacked frames), 23 = the static camera (one band), 31 = two bands per frame;
# conv2: 20 = stacked, even side; 49 = several bands, odd side, parity planes of unequal size; 30 / 33 = even / odd sides in between.  7 frames leave a short last stack
FD_CASES = [(3, side, nf) for side in (9, 23, 31) for nf in (1, 7)] + [(2, side, nf) for side in (20, 49, 30, 33) for nf in (1, 7)]
WG_CASES = [(3, side, 3) for side in (9, 18, 23, 31)] + [(2, side, 3) for side in (20, 49, 57)]          # single weight-gradient launches
WG_PAIR_SIDES = {3: (23, 9), 2: (49, 20), 1: (200, 84)}          # the two cameras' own sides (static, gripper) per layer
WG_PAIR_FRAMES = ((3, 1), (1, 3))
C1_CASES = [(84, 2), (200, 2)]          # conv1: (side, frames)


def grade(n, table=GRADE):
    return 2.0 ** table[np.arange(n) % len(table)]


def _mag(tag, shape, seed):
    """+-[0.25, 1): no element is small by chance"""
    u = prng.uniform01(tag + "m", shape, seed=seed).astype(np.float64)
    s = np.where(prng.uniform01(tag + "s", shape, seed=seed + 1) < 0.5, -1.0, 1.0)
    return s * (0.25 + 0.75 * u)


def dy_scale(dtype):
    return LOSS_SCALE if dtype == "fp16" else 1.0


@functools.lru_cache(maxsize=None)
def weights(layer, dtype):
    """W (co, ci, k, k) rounded to the storage type, b (co) fp32"""
    g = LAYERS[layer]
    W = _mag(f"convW{layer}", (g["co"], g["ci"], g["k"], g["k"]), 21) * grade(g["co"])[:, None, None, None] * grade(g["ci"], GRADE_IN)[None, :, None, None]
    b = (_mag(f"convb{layer}", (g["co"],), 23) * grade(g["co"])).astype(np.float32).astype(np.float64)
    return frozen(round_t(W, dtype), b)


@functools.lru_cache(maxsize=None)
def acts(layer, side, frames, dtype):
    """X (n, side, side, ci): graded per input channel, a quarter of the elements exactly 0 (a post-ReLU activation); dY (n, oh, oh, co): graded per output channel, times
    the loss scale for fp16"""
    g = LAYERS[layer]
    oh = CR.out_side(side, g["k"], g["s"])
    tag = f"conv{layer}_{side}_{frames}"
    X = _mag(tag + "x", (frames, side, side, g["ci"]), 31) * grade(g["ci"], GRADE_IN)
    X = np.where(prng.uniform01(tag + "z", X.shape, seed=33) < 0.25, 0.0, X)
    dY = _mag(tag + "dy", (frames, oh, oh, g["co"]), 35) * grade(g["co"]) * dy_scale(dtype)
    return frozen(round_t(X, dtype), round_t(dY, dtype))


MASK_KINDS = ("+0", "-0", "+sub", "-sub", "+", "-")


@functools.lru_cache(maxsize=None)
def mask_values(layer, side, frames, dtype):
    """the 16-bit mask VALUES of the data-gradient fallback forms: +0.0, -0.0, the smallest positive / negative subnormal of the type, ordinary positives and negatives.
    kind = (c + h + 2 w + n) % 6: over the pixels every channel — so both halves of every packed pair — sees each kind.  -> (values, kind index)"""
    ci = LAYERS[layer]["ci"]
    n, h, w, c = np.meshgrid(np.arange(frames), np.arange(side), np.arange(side), np.arange(ci), indexing="ij")
    kind = (c + h + 2 * w + n) % 6
    sub = SUBNORMAL[dtype]
    ordinary = round_t(np.abs(_mag(f"convmask{layer}_{side}_{frames}", kind.shape, 41)), dtype)
    v = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4], [0.0, -0.0, sub, -sub, ordinary], -ordinary)
    return frozen(v, kind)


def mask_keep(values):
    """what the reference keeps: the value is > 0 (the subnormal passes, both zeros do not)"""
    return values > 0


@functools.lru_cache(maxsize=None)
def keep_bits(layer, side, frames):
    """the boolean ReLU mask of the bit-word forms"""
    ci = LAYERS[layer]["ci"]
    return frozen(prng.uniform01(f"convkeep{layer}_{side}_{frames}", (frames, side, side, ci), seed=43) < 0.5)


# ---------------------------------------------------------------------------------------------------- references (computed once, shared, read-only) and tolerances
@functools.lru_cache(maxsize=None)
def fwd_ref(layer, side, frames, dtype):
    g = LAYERS[layer]
    W, b = weights(layer, dtype)
    return frozen(*CR.fwd(acts(layer, side, frames, dtype)[0], W, b, g["s"]))


@functools.lru_cache(maxsize=None)
def dgrad_ref_unmasked(layer, side, frames, dtype):
    g = LAYERS[layer]
    dY = acts(layer, side, frames, dtype)[1]
    return frozen(*CR.dgrad(dY, weights(layer, dtype)[0], g["s"], side, np.ones((frames, side, side, g["ci"]), bool)))


def dgrad_ref(layer, side, frames, dtype, keep):
    dX, bound = dgrad_ref_unmasked(layer, side, frames, dtype)
    return np.where(keep, dX, 0.0), np.where(keep, bound, 0.0)


@functools.lru_cache(maxsize=None)
def wgrad_ref(layer, side, frames, dtype):
    """(dW, db, bound_w, bound_b) without partial slabs; wgrad_bound adds them"""
    g = LAYERS[layer]
    X, dY = acts(layer, side, frames, dtype)
    return frozen(*CR.wgrad(X, dY, g["k"], g["s"], 0))


def wgrad_bound(bound0, K, slabs):
    """acc_bound is linear in K + 2 + extra: the bound of `slabs` summed slabs from the bound without any"""
    return bound0 * ((K + 2 + slabs) / (K + 2))


def tol16(ref, bound, dtype, keep=None):
    """a 16-bit output: the accumulation bound + one ulp of the storage type (at least its smallest subnormal); where the mask is off: 0 = exact"""
    t = bound + np.maximum(ULP[dtype] * np.abs(ref), SUBNORMAL[dtype])
    return t if keep is None else np.where(keep, t, 0.0)


def tol16_nearest(ref, bound, dtype, keep=None):
    """the same with HALF an ulp: what round-to-nearest of an fp32 accumulator within `bound` of ref guarantees, |rn(a) - ref| <= ulp/2 (|ref| + bound) + bound.  One whole
    ulp cannot tell truncation from rounding (a truncated value is less than one ulp off); half an ulp can"""
    t = bound * (1 + ULP[dtype] / 2) + np.maximum(0.5 * ULP[dtype] * np.abs(ref), SUBNORMAL[dtype])
    return t if keep is None else np.where(keep, t, 0.0)


# ---------------------------------------------------------------------------------------------------- conv1
def c1_pad(side):
    return 10 if side >= 100 else 4


@functools.lru_cache(maxsize=None)
def c1_inputs(side, frames, dtype):
    """conv1: fp32 NCHW frames in (-1, 1) (NOT pre-rounded: the kernels round them to the storage type), uint8 NHWC frames, RandomShiftsAug shifts (sx, sy) that include
    0, pad (no shift) and 2 pad (= +-pad), dY (n, oh, oh, 32)"""
    oh = CR.out_side(side, 8, 4)
    tag = f"conv1_{side}_{frames}"
    Xf = (_mag(tag + "x", (frames, 3, side, side), 51)).astype(np.float32)
    u8 = prng.randint(tag + "u", (frames, side, side, 3), 256, seed=53).astype(np.uint8)
    pad = c1_pad(side)
    sh = np.array([[0, 2 * pad], [2 * pad, pad], [pad, 0], [2 * pad, 2 * pad]], np.int32)[np.arange(frames) % 4]
    dY = round_t(_mag(tag + "dy", (frames, oh, oh, 32), 55) * grade(32) * dy_scale(dtype), dtype)
    return frozen(Xf, u8, sh, dY)


def c1_x16(Xf, dtype):
    """the fp32 NCHW frames as the kernels stage them: rounded to the storage type, NHWC"""
    return round_t(Xf, dtype).transpose(0, 2, 3, 1)


def c1_u8_x16(u8, shifts, pad, dtype):
    """the uint8 frames as the unfolded kernels stage them: shifted, x = fma(u, 2/255, -1) in fp32, rounded to the storage type"""
    return round_t(CR.u8_values(CR.shift_frames(u8, shifts, pad))[1], dtype)


def c1_frames16(side, frames, dtype, src):
    """conv1's input as the kernels stage it (NHWC, 16-bit values): src = "f32" (fp32 NCHW frames), "u8" (uint8 frames, no shift), "u8s" (uint8 frames + shifts)"""
    Xf, u8, sh, _ = c1_inputs(side, frames, dtype)
    pad = c1_pad(side)
    if src == "f32":
        return c1_x16(Xf, dtype)
    return c1_u8_x16(u8, sh if src == "u8s" else np.full((frames, 2), pad, np.int32), pad, dtype)


@functools.lru_cache(maxsize=None)
def c1_fwd_ref(side, frames, dtype, src):
    W, b = weights(1, dtype)
    return frozen(*CR.fwd(c1_frames16(side, frames, dtype, src), W, b, 4))


@functools.lru_cache(maxsize=None)
def c1_wgrad_ref(side, frames, dtype, src, fold=0):
    """(dW (32, 3, 8, 8), db, bound_w, bound_b) without partial slabs.  fold (uint8 only): the kernels multiply dY by the exact byte u and form (2/255) (dY * u) - db per slab:
    the reference takes the exact x = u (2/255) - 1, the bound the magnitudes of both terms and three more operations (scale, subtract, the rounding of 2/255)"""
    _, u8, sh, dY = c1_inputs(side, frames, dtype)
    if not fold:
        return frozen(*CR.wgrad(c1_frames16(side, frames, dtype, src), dY, 8, 4, 0))
    pad = c1_pad(side)
    us = CR.shift_frames(u8, sh if src == "u8s" else np.full((frames, 2), pad, np.int32), pad)
    dW, db, _, bb = CR.wgrad(CR.u8_values(us)[0], dY, 8, 4, 0)
    K = dY.shape[0] * dY.shape[1] * dY.shape[2]
    mag = (2.0 / 255.0) * CR._wcorr(us.astype(np.float64), np.abs(dY), 8, 4) + np.abs(dY).sum((0, 1, 2))[:, None, None, None]
    return frozen(dW, db, CR.acc_bound(mag, K, 3), bb)
