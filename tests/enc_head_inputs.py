"""Inputs, gates and float32-vs-float64 measurements shared by tests/test_gpu_encoder_head.py, tests/test_gpu_logistic_loss.py (GPU) and
tests/test_enc_head_ref_host.py (host, which re-measures every measured gate so that none of them rests on a kernel's output)."""
import functools

import numpy as np
import torch

import enc_head_ref as R

ULP = {"bf16": 2.0 ** -7, "fp16": 2.0 ** -10}          # one unit in the last place of the storage type, relative
TINY = {"bf16": 2.0 ** -133, "fp16": 2.0 ** -24}          # the format's subnormal step: below the normal range rounding is absolute, not relative
ACC = 2e-5          # fp32 accumulation of a dot product, relative to the tensor's largest magnitude (test_gemm_glds_matches_fp64)


def tdt(dtype):
    return torch.bfloat16 if dtype == "bf16" else torch.float16


def round16(x, dtype):
    """x rounded to the 16-bit storage type (round to nearest even, as the device converts), as float64"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(tdt(dtype)).float().numpy().astype(np.float64)


# ==================================================================================================== spatial softmax
SS_NF = 5
SS_SHAPES = [(3, 3), (7, 7), (21, 21), (16, 28), (15, 30), (21, 22)]          # most threads idle | gripper | static (441) | 448 = last register-path size | online path x 2

# fp32 softmax statistics, per shape: 5 x the worst error of the same formulas (enc_head_ref.spatial_softmax_fwd) in numpy float32 against float64 on that shape's own
# ss_inputs, both storage types (ss_measure; test_enc_head_ref_host.py asserts that every gate is 5 x what it measures).
#   (H, W): (coordinates ex, ey: worst absolute error;  1 / sum: worst relative error)
SS_F32 = {(3, 3): (4.1e-7, 3.8e-7),          # measured 4.048e-7, 3.707e-7
          (7, 7): (8.7e-7, 1.15e-6),          # measured 8.662e-7, 1.139e-6
          (21, 21): (7.3e-6, 9.4e-6),          # measured 7.290e-6, 9.359e-6
          (16, 28): (1.15e-5, 1.32e-5),          # measured 1.142e-5, 1.316e-5
          (15, 30): (3.95e-6, 7.25e-6),          # measured 3.907e-6, 7.219e-6
          (21, 22): (4.4e-6, 6.85e-6)}          # measured 4.350e-6, 6.825e-6
SS_GATE = {k: (5 * c, 5 * i) for k, (c, i) in SS_F32.items()}          # (coordinate gate, absolute; 1 / sum gate, relative)


@functools.lru_cache(maxsize=None)
def ss_inputs(H, W, dtype):
    """max(3 randn, 0) maps (Nf, H, W, 64) with: channel 0 all zero, channel 1 one peak of 30, channel 2 all equal and positive, frame 4 not rectified (negative
    values); rounded to the storage type"""
    rng = np.random.default_rng(1000 * H + W)
    f = 3 * rng.standard_normal((SS_NF, H, W, 64))
    f[:4] = np.maximum(f[:4], 0)
    f[..., 0] = 0.0
    f[..., 1] = 0.0
    for n in range(SS_NF):
        f[n, rng.integers(H), rng.integers(W), 1] = 30.0
    f[..., 2] = 2.5
    f = round16(f, dtype)
    f.setflags(write=False)
    return f


def ss_measure(H, W):
    """worst float32-vs-float64 error of the statistics on the (H, W) inputs of both storage types: (coordinates, absolute; 1 / sum, relative)"""
    worst_c = worst_i = 0.0
    for dtype in ("bf16", "fp16"):
        f = ss_inputs(H, W, dtype)
        _, (_, inv, ex, ey) = R.spatial_softmax_fwd(f)
        _, (_, inv32, ex32, ey32) = R.spatial_softmax_fwd(f.astype(np.float32))
        worst_c = max(worst_c, np.abs(ex32 - ex).max(), np.abs(ey32 - ey).max())
        worst_i = max(worst_i, (np.abs(inv32 - inv) / inv).max())
    return float(worst_c), float(worst_i)


# ==================================================================================================== action loss
LL_SHAPES = ((1, 1), (3, 5), (16, 2))
NMIX, NDIM, NCLS, LSMIN, LDH = 10, 6, 10, -7.0, 192          # LDH: the engine's packed head width (3 * 60 + 2 gripper logits, padded to 16)
LL_SECTIONS = ("row_loss", "dlogits", "dmeans", "dlsr", "dgrip")
# distance every tcp-frame action keeps from the branch thresholds -0.999 / 0.999: the device's fp32 frame change is gated at 3e-4 of the float64 one, and 1e-4
# must remain so that the device's action takes the float64 action's branch
LL_ACTION_MARGIN = 5e-4


@functools.lru_cache(maxsize=None)
def ll_inputs(B, S, gripper_control):
    """fp32 heads, actions and robot_obs that take every branch of the loss.  Row r = b * S + t, dimension d: (r + d) % 4 = 0: action at the lower bound (exactly -1
    or within 4e-4 of it), 1: at the upper bound, 2 / 3: inside.  Components alternate between wide ones near the action (delta > 1e-5) and narrow ones far from it
    (the mid-point fallback; some log-scales below log_scale_min).  gripper_control: every second row has a zero tcp orientation, so that its position passes the
    frame change unchanged and keeps its exact +-1."""
    r = np.arange(B * S).reshape(B, S)
    cat = (r[..., None] + np.arange(NDIM)) % 4
    for attempt in range(100):
        rng = np.random.default_rng(1000 * attempt + 10 * B + S)
        edge = np.where(rng.random((B, S, NDIM)) < 0.5, 1.0, rng.uniform(0.9996, 1.0, (B, S, NDIM)))
        a = np.empty((B, S, 7))
        a[..., :NDIM] = np.where(cat == 0, -edge, np.where(cat == 1, edge, rng.uniform(-0.9, 0.9, (B, S, NDIM))))
        a[..., 6] = np.where(r % 2 == 0, -1.0, 1.0)
        ro = rng.uniform(-1, 1, (B, S, 15))
        ro[..., 3:6] = np.where((r % 2 == 0)[..., None], 0.0, ro[..., 3:6])
        a, ro = a.astype(np.float32), ro.astype(np.float32)
        at = R.world_to_tcp(a.astype(np.float64), ro.astype(np.float64)) if gripper_control else a.astype(np.float64)
        # the frame change lands where it lands: take the first draw whose tcp-frame actions all keep LL_ACTION_MARGIN from the two thresholds
        if (np.abs(np.abs(at[..., :NDIM]) - 0.999) > LL_ACTION_MARGIN).all():
            break
    else:
        raise AssertionError("no draw keeps the tcp-frame actions off the thresholds")
    near = (np.arange(NMIX) % 2 == 0) + np.zeros((B, S, NDIM, NMIX), bool)
    off = np.where(near, rng.uniform(-0.5, 0.5, near.shape), rng.choice([-1.0, 1.0], near.shape) * rng.uniform(0.6, 1.2, near.shape))
    means = at[..., :NDIM, None] + off
    inside = (np.abs(at[..., :NDIM]) < 0.999)[..., None]          # by the tcp-frame action: the frame change moves orientations (and rotated positions) off the bounds
    lsr = np.where(inside, np.where(near, rng.uniform(-1.5, 0, near.shape), rng.uniform(-9, -5, near.shape)), rng.uniform(-9, 0, near.shape))
    out = dict(logits=rng.standard_normal(near.shape), means=means, lsr=lsr, grip=rng.standard_normal((B, S, 2)), actions=a, robot_obs=ro)
    out = {k: np.ascontiguousarray(v, np.float32) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


def ll_reference(inp, a_tcp, discrete, dt=np.float64):
    """the loss and its row gradients in dtype dt from the fp32 inputs and the tcp-frame action a_tcp (B, S, 7)"""
    g = inp["grip"].astype(dt) if discrete else None
    return R.logistic_mixture_rows(inp["logits"].astype(dt), inp["means"].astype(dt), inp["lsr"].astype(dt), g, a_tcp.astype(dt), NCLS, LSMIN, 1.0)


def ll_check_branches(ref, a_tcp, min_share=0.05):
    """float32 and float64 must take the same branch everywhere: no delta near its 1e-5 threshold, no action near the two bounds' thresholds; and every branch is
    taken by at least min_share of the components"""
    case, delta = ref["case"], ref["delta"]
    assert not ((case >= 2) & (delta >= 5e-6) & (delta <= 2e-5)).any(), "a component's delta sits at the threshold"
    a = a_tcp[..., :NDIM]
    assert (np.abs(a + 0.999) > 1e-4).all() and (np.abs(a - 0.999) > 1e-4).all(), "an action sits at a bound's threshold"
    if min_share:
        for c in range(4):
            assert (case == c).mean() >= min_share, f"branch {c}: {(case == c).mean():.3f} of the components"


def ll_sections(ref, discrete):
    """the reference as the kernel lays it out: row_loss (B, S, 8) and the four column groups of dheads (unscaled)"""
    B, S = ref["loss"].shape[:2]
    rl = np.zeros((B, S, 8))
    rl[..., :NDIM] = ref["loss"]
    out = dict(dlogits=ref["dlogits"].reshape(B, S, -1), dmeans=ref["dmeans"].reshape(B, S, -1), dlsr=ref["dlsr"].reshape(B, S, -1))
    if discrete:
        rl[..., NDIM] = ref["gloss"]
        out["dgrip"] = ref["dgrip"]
    out["row_loss"] = rl
    return {k: np.asarray(v, np.float64) for k, v in out.items()}


def ll_err(got, ref):
    """per element, relative to |ref| + 1e-3 max|ref| (pure relative error has no meaning at a gradient's zero crossings); the worst over the tensor"""
    return float((np.abs(got - ref) / (np.abs(ref) + 1e-3 * np.abs(ref).max())).max())


def ll_measure(inp, a_tcp, discrete):
    """what fp32 arithmetic alone costs: the reference formulas in numpy float32 against float64 on the same inputs, per section, in ll_err's measure"""
    s64 = ll_sections(ll_reference(inp, a_tcp, discrete), discrete)
    s32 = ll_sections(ll_reference(inp, a_tcp, discrete, np.float32), discrete)
    return {k: ll_err(s32[k], s64[k]) for k in s64}


# 4 x the worst ll_measure over LL_SHAPES x gripper_control x discrete_gripper (test_enc_head_ref_host.py asserts the factor), per section; worst measured values:
LL_F32 = dict(row_loss=2.9e-6, dlogits=8.0e-5, dmeans=4.1e-5, dlsr=9.2e-5, dgrip=1.25e-6)          # measured 2.89e-6, 7.93e-5, 4.05e-5, 9.20e-5, 1.247e-6
LL_GATE = {k: 4 * v for k, v in LL_F32.items()}
