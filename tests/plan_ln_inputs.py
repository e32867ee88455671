"""Inputs, gates and float32-vs-float64 measurements shared by tests/test_gpu_plan_kernels.py, tests/test_gpu_layernorm.py (GPU) and
tests/test_plan_ln_ref_host.py (host, which re-measures every measured gate so that none of them rests on a kernel's output).  Inputs come from
hulc_amd.utils.portable_rng (fixed seeds, built on the host)."""
import functools

import numpy as np
import torch

import hulc_oracle as O
import plan_ln_ref as R
from hulc_amd.utils import portable_rng as prng

ULP = {"bf16": 2.0 ** -7, "fp16": 2.0 ** -10, "fp32": 0.0}          # one unit in the last place of the storage type, relative (fp32: the accumulation bound alone)
ACC = 2e-5          # fp32 accumulation, relative to the tensor's largest magnitude (test_gemm_glds_matches_fp64)
EPS32 = 2.0 ** -24          # unit roundoff of fp32
DTYPES = ("bf16", "fp16", "fp32")


def tdt(dtype):
    return {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[dtype]


def round_t(x, dtype):
    """x rounded to the storage type (round to nearest even, as the device converts), as float64"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(tdt(dtype)).float().numpy().astype(np.float64)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def rel_err(got, ref):
    """per element, relative to |ref| + 1e-3 max|ref| (pure relative error has no meaning at a zero crossing); the worst over the tensor"""
    ref = np.asarray(ref, np.float64)
    return float((np.abs(np.asarray(got, np.float64) - ref) / (np.abs(ref) + 1e-3 * np.abs(ref).max() + 1e-300)).max())


# ==================================================================================================== categorical plan: KL + sample
KL_CASES = [(B, ncat, ncls) for B in (1, 3, 65) for ncat in (32, 3) for ncls in (32, 7, 64)]
KL_W = (0.004, 0.001)          # w_pp, w_pr: the engine's lw * beta * mix / B in order of magnitude
KL_OUT = ("probs", "kl_cat", "dpp", "dpr")


@functools.lru_cache(maxsize=None)
def kl_inputs(B, ncat, ncls):
    """fp32 logits (B, NCAT, NCLS) of both distributions.  Rows (b, cat) alternate between N(0, 1) and N(0, 8^2); row 0 carries a +30 spike on class
    KL_SPIKE % NCLS (pr) and row 1 is all equal (pr)."""
    tag = f"kl{B}_{ncat}_{ncls}"
    scale = np.where(np.arange(B * ncat) % 2 == 0, 1.0, 8.0).reshape(B, ncat, 1)
    pr = prng.normal(tag + "pr", (B, ncat, ncls), seed=11).astype(np.float64) * scale
    pp = prng.normal(tag + "pp", (B, ncat, ncls), seed=12).astype(np.float64) * scale
    pr[0, 0, KL_SPIKE % ncls] += 30.0
    pr[0, 1, :] = 0.75
    return frozen(pr.astype(np.float32), pp.astype(np.float32))


KL_SPIKE = 5


def kl_measure(B, ncat, ncls):
    """rel_err of the reference formulas in float32 against float64 on the case's inputs, per output"""
    pr, pp = kl_inputs(B, ncat, ncls)
    r64 = R.plan_kl(pr.astype(np.float64), pp.astype(np.float64), *KL_W)
    r32 = R.plan_kl(pr, pp, *KL_W)
    return tuple(rel_err(a, b) for a, b in zip(r32, r64))


# measured float32-vs-float64 error per case (probs, kl_cat, dpp, dpr), rounded up by at most a tenth; the gate is 5 x (tests/test_plan_ln_ref_host.py re-measures)
KL_F32 = {
    (1, 32, 32): (4.06e-07, 2.5e-07, 4.23e-06, 6.76e-05),          # measured 4.060e-07, 2.492e-07, 4.228e-06, 6.752e-05
    (1, 32, 7): (3.03e-07, 5.7e-06, 6.32e-05, 0.000263),          # measured 3.030e-07, 5.700e-06, 6.312e-05, 2.620e-04
    (1, 32, 64): (4.75e-07, 3.5e-07, 4.9e-06, 0.000194),          # measured 4.743e-07, 3.499e-07, 4.890e-06, 1.935e-04
    (1, 3, 32): (3.29e-07, 3.82e-07, 9.18e-07, 8.67e-06),          # measured 3.285e-07, 3.817e-07, 9.177e-07, 8.662e-06
    (1, 3, 7): (1.6e-07, 6.54e-08, 1.38e-06, 7.59e-07),          # measured 1.591e-07, 6.540e-08, 1.371e-06, 7.580e-07
    (1, 3, 64): (3.28e-07, 1.31e-07, 2.16e-06, 6.05e-06),          # measured 3.272e-07, 1.300e-07, 2.154e-06, 6.044e-06
    (3, 32, 32): (4.87e-07, 3.8e-07, 7.9e-06, 0.000218),          # measured 4.865e-07, 3.796e-07, 7.899e-06, 2.179e-04
    (3, 32, 7): (4.18e-07, 3.83e-06, 4.61e-05, 0.00023),          # measured 4.177e-07, 3.826e-06, 4.609e-05, 2.291e-04
    (3, 32, 64): (5.19e-07, 5.4e-07, 6.38e-06, 0.000671),          # measured 5.180e-07, 5.396e-07, 6.375e-06, 6.704e-04
    (3, 3, 32): (4.34e-07, 6.45e-08, 3.44e-06, 3e-06),          # measured 4.333e-07, 6.446e-08, 3.432e-06, 2.995e-06
    (3, 3, 7): (1.3e-07, 1.87e-07, 6.7e-07, 0.000446),          # measured 1.294e-07, 1.864e-07, 6.691e-07, 4.459e-04
    (3, 3, 64): (3.63e-07, 9.85e-08, 2.82e-06, 6.46e-06),          # measured 3.627e-07, 9.846e-08, 2.818e-06, 6.456e-06
    (65, 32, 32): (4.79e-07, 1.59e-06, 2.83e-05, 0.000433),          # measured 4.783e-07, 1.586e-06, 2.825e-05, 4.329e-04
    (65, 32, 7): (4.83e-07, 4.6e-06, 8.09e-05, 0.000466),          # measured 4.827e-07, 4.598e-06, 8.089e-05, 4.655e-04
    (65, 32, 64): (5.15e-07, 7.8e-07, 1.18e-05, 0.00107),          # measured 5.142e-07, 7.799e-07, 1.174e-05, 1.063e-03
    (65, 3, 32): (5.27e-07, 5.91e-07, 9.27e-06, 0.000179),          # measured 5.262e-07, 5.904e-07, 9.262e-06, 1.783e-04
    (65, 3, 7): (4.93e-07, 1.49e-06, 1.47e-05, 0.000163),          # measured 4.925e-07, 1.487e-06, 1.468e-05, 1.625e-04
    (65, 3, 64): (4.62e-07, 5.9e-07, 9.57e-06, 0.000242),          # measured 4.618e-07, 5.893e-07, 9.563e-06, 2.419e-04
}
KL_GATE = {k: tuple(5 * x for x in v) for k, v in KL_F32.items()}

# seeds of the sampled draws: chosen so that, in float64, at most 1 % of the rows of every case have their two best Gumbel values closer than KL_GAP (host test)
KL_SEEDS = (3, 77)
KL_GAP = 1e-4


def hash_uniform(seed, n, first=0):
    """the engine's counter-based uniform of elements first .. first + n - 1 (oracle: engine_keep_mask's hash), fp32 arithmetic as on the device"""
    with np.errstate(over="ignore"):
        idx = np.arange(n, dtype=np.uint64) + np.uint64(first)
        z = O._mix64(np.uint64(seed) + (idx + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15))
    h = (z >> np.uint64(32)).astype(np.uint32)
    return (((h >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)).astype(np.float64)


def gumbel_draw(pr, seed):
    """-> (idx (B, NCAT): argmax of logits + Gumbel noise in float64, lowest index on ties; decided (B, NCAT): the best value leads the second best by more than
    KL_GAP * max(1, |best|))"""
    B, ncat, ncls = pr.shape
    u = hash_uniform(seed, pr.size).reshape(pr.shape)
    g = pr.astype(np.float64) - np.log(-np.log(u))
    idx = g.argmax(-1)
    srt = np.sort(g, -1)
    best = srt[..., -1]
    decided = (best - srt[..., -2] > KL_GAP * np.maximum(1.0, np.abs(best))) if ncls > 1 else np.ones_like(best, bool)
    return idx.astype(np.int32), decided


# ==================================================================================================== straight-through backward
ST_CASES = [(rows, ncls) for rows in (1, 96, 2080) for ncls in (32, 7)]


@functools.lru_cache(maxsize=None)
def st_inputs(rows, ncls):
    tag = f"st{rows}_{ncls}"
    probs = R.softmax(2.0 * prng.normal(tag + "l", (rows, ncls), seed=21).astype(np.float64)).astype(np.float32)
    dplan = prng.normal(tag + "d", (rows, ncls), seed=22)
    dpr = 0.01 * prng.normal(tag + "r", (rows, ncls), seed=23)
    dpp = 0.01 * prng.normal(tag + "p", (rows, ncls), seed=24)
    return frozen(probs, dplan.astype(np.float32), dpr.astype(np.float32), dpp.astype(np.float32))


# ==================================================================================================== one-hot gather and scatter
def plan_indices(B, ncat, ncls, pattern, tag=""):
    """pattern 0: uniform; 1: every window on one class (the longest dependent chain of LDS updates); 2: window b on class b % NCLS"""
    if pattern == 0:
        idx = prng.randint(f"idx{B}_{ncat}_{ncls}{tag}", (B, ncat), ncls, seed=31)
    elif pattern == 1:
        idx = np.full((B, ncat), min(3, ncls - 1))
    else:
        idx = np.repeat(np.arange(B)[:, None] % ncls, ncat, 1)
    return np.ascontiguousarray(idx, np.int32)


SC_DC_MIN = 0.5          # the smallest |dC| the scatter inputs hold


@functools.lru_cache(maxsize=None)
def scatter_inputs(B, H, dtype):
    """dC (B, H) of order 1 with mixed signs, |dC| in [0.5, 1.5], rounded to the storage type"""
    tag = f"sc{B}_{H}"
    mag = prng.uniform(tag + "m", (B, H), SC_DC_MIN, 1.5, seed=41).astype(np.float64)
    sign = np.where(prng.uniform01(tag + "s", (B, H), seed=42) < 0.5, -1.0, 1.0)
    dC = round_t(mag * sign, dtype)
    assert np.abs(dC).min() >= SC_DC_MIN
    return frozen(dC)


def scatter_reference(dC, idx, ncls, dw0):
    """-> (sum of the windows' rows alone (H, NCAT * NCLS), gate per element for `dw0 + sum` (dw0 = None: the sum alone): a sum of at most B + 1 fp32 addends,
    |err| <= (B + 1) 2^-24 sum |addends|)"""
    B = dC.shape[0]
    s = R.plan_scatter(dC, idx, ncls)
    mag = R.plan_scatter(np.abs(dC), idx, ncls)
    if dw0 is not None:
        mag = mag + np.abs(dw0)
    return s, (B + 1) * EPS32 * mag


@functools.lru_cache(maxsize=None)
def gather_weight(kin, H, dtype):
    """w_t (KIN, H) in the storage type, every row of a column distinct: element (r, i) takes pattern k = (7 r + 13 i) mod 2048 (7 is odd, so 2048 consecutive
    rows of a column never repeat) of 2048 distinct values: sign = bit 10 of k, magnitude = the (k mod 1024)-th value from 2^-4 up (bf16, eight binades:
    [2^-4, 2^4); fp32 holds the same values) or from 0.5 up (fp16, one binade).  -> float64 values"""
    assert kin <= 2048
    r, i = np.arange(kin)[:, None], np.arange(H)[None, :]
    k = (7 * r + 13 * i) % 2048
    off = (k % 1024).astype(np.int32)
    if dtype == "fp16":
        w = torch.from_numpy((0x3800 + off).astype(np.int16)).view(torch.float16).float().numpy()
    else:
        w = torch.from_numpy((0x3D80 + off).astype(np.int16)).view(torch.bfloat16).float().numpy()
    w = np.where(k >= 1024, -w, w).astype(np.float64)
    assert all(len(np.unique(w[:, c])) == kin for c in (0, H // 2, H - 1))
    return frozen(w)


# ==================================================================================================== continuous plan (mcil)
NK_CASES = [(B, n) for B in (1, 5) for n in (256, 3)]
NK_W = (0.004, 0.001)
NK_OUT = ("plan", "kl_elem", "dpp", "dpr")
NK_V = (-25.0, -5.0, 0.0, 5.0, 25.0)          # var values: both branches of the device's softplus (|x| > 20) and the middle


@functools.lru_cache(maxsize=None)
def nk_inputs(B, n):
    """pr_state, pp_state (B, 2n) fp32 = mean | var, eps (B, n).  var = NK_V[k] + 0.3 N(0, 1) with k = j % 5 for pr and (j // 5 + b) % 5 for pp: every pair of
    regimes meets"""
    tag = f"nk{B}_{n}"
    j, b = np.arange(n)[None, :], np.arange(B)[:, None]
    v = np.array(NK_V)
    v1 = v[(j + 0 * b) % 5] + 0.3 * prng.normal(tag + "v1", (B, n), seed=51)
    v2 = v[(j // 5 + b) % 5] + 0.3 * prng.normal(tag + "v2", (B, n), seed=52)
    pr = np.concatenate([prng.normal(tag + "m1", (B, n), seed=53), v1], -1).astype(np.float32)
    pp = np.concatenate([prng.normal(tag + "m2", (B, n), seed=54), v2], -1).astype(np.float32)
    eps = prng.normal(tag + "e", (B, n), seed=55).astype(np.float32)
    return frozen(pr, pp, eps)


def nk_reference(B, n, dt=np.float64):
    pr, pp, eps = (a.astype(dt) for a in nk_inputs(B, n))
    dpp, dpr = R.kl_normal_grads(pr, pp, *NK_W)
    return R.rsample(pr, eps), R.kl_normal(pr, pp), dpp, dpr


def nk_measure(B, n):
    return tuple(rel_err(a, b) for a, b in zip(nk_reference(B, n, np.float32), nk_reference(B, n)))


# measured float32-vs-float64 rel_err per case (plan, kl_elem, dpp, dpr), rounded up by at most a tenth; gate = 5 x
NK_F32 = {
    (1, 256): (3.04e-07, 2.25e-07, 2.34e-07, 2.21e-07),          # measured 3.038e-07, 2.247e-07, 2.332e-07, 2.202e-07
    (1, 3): (2.37e-08, 1.32e-07, 1.27e-07, 3.16e-07),          # measured 2.369e-08, 1.311e-07, 1.264e-07, 3.154e-07
    (5, 256): (6.1e-07, 2.67e-07, 2.65e-07, 3.17e-07),          # measured 6.097e-07, 2.668e-07, 2.646e-07, 3.163e-07
    (5, 3): (4.38e-08, 2.36e-07, 2.52e-07, 2.52e-07),          # measured 4.374e-08, 2.354e-07, 2.518e-07, 2.518e-07
}
NK_GATE = {k: tuple(5 * x for x in v) for k, v in NK_F32.items()}


@functools.lru_cache(maxsize=None)
def nkb_inputs(B, n):
    """the reparametrised sample's backward: dplan (B, n), dpr_kl (B, 2n) fp32; eps and pr_state are nk_inputs'"""
    dplan = prng.normal(f"rb{B}_{n}", (B, n), seed=56).astype(np.float32)
    dkl = (0.1 * prng.normal(f"rk{B}_{n}", (B, 2 * n), seed=57)).astype(np.float32)
    return frozen(dplan, dkl)


def nkb_reference(B, n, dt=np.float64):
    pr, _, eps = nk_inputs(B, n)
    dplan, dkl = nkb_inputs(B, n)
    return R.rsample_bwd(dplan.astype(dt), eps.astype(dt), pr.astype(dt), dkl.astype(dt))


def nkb_measure(B, n):
    return rel_err(nkb_reference(B, n, np.float32), nkb_reference(B, n))


# measured float32-vs-float64 rel_err of rsample_bwd per case, rounded up by at most a tenth; the fp32 output is gated at 5 x, a 16-bit output at one ulp of the
# storage type + 5 x
NKB_F32 = {
    (1, 256): 1.03e-06,          # measured 1.028e-06
    (1, 3): 4.37e-07,          # measured 4.369e-07
    (5, 256): 1.97e-06,          # measured 1.964e-06
    (5, 3): 1.52e-07,          # measured 1.511e-07
}
NKB_GATE = {k: 5 * v for k, v in NKB_F32.items()}


# ==================================================================================================== LayerNorm
LN_STAT = 2e-5          # the project's gate on mean and rstd, relative per row
LN_ROW_CONST, LN_ROW_CANCEL = 1, 2          # rows of ln_inputs (when rows >= 3): all equal (variance 0) | mean 1e3, spread 1e-2 (cancellation)


@functools.lru_cache(maxsize=None)
def ln_inputs(rows, n):
    """x (rows, n), g, b fp32.  Every row's mean stays away from zero (offset of magnitude >= 1.5 against a spread of 1.5 / sqrt(n)... n = 1 aside, where the mean
    is the value itself), so that the relative gate on the mean has a meaning."""
    tag = f"ln{rows}_{n}"
    off = prng.normal(tag + "o", (rows, 1), seed=62).astype(np.float64)
    off = np.where(off < 0, -1.0, 1.0) * (1.5 + 0.5 * np.abs(off))
    x = prng.normal(tag + "x", (rows, n), seed=61).astype(np.float64) * (1.5 if n > 1 else 0.25) + off
    if rows >= 3:
        x[LN_ROW_CONST] = 2.25
        x[LN_ROW_CANCEL] = 1e3 + 1e-2 * prng.normal(tag + "c", (n,), seed=63)
    g = 1.0 + 0.2 * prng.normal(tag + "g", (n,), seed=64)
    b = 0.2 * prng.normal(tag + "b", (n,), seed=65)
    return frozen(x.astype(np.float32), g.astype(np.float32), b.astype(np.float32))


def ln_cancel_measure(rows, n):
    """relative float32-vs-float64 error of rstd on the cancellation row"""
    x, g, b = ln_inputs(rows, n)
    _, _, r64 = R.ln_fwd(x[LN_ROW_CANCEL].astype(np.float64), g.astype(np.float64), b.astype(np.float64))
    _, _, r32 = R.ln_fwd(x[LN_ROW_CANCEL], g, b)
    return float(abs(r32 - r64) / r64)


# rstd of the cancellation row: worst measured relative float32-vs-float64 error per n over LN_CANCEL_ROWS (n = 1: the row has variance 0), rounded up by at most
# a tenth; gate = 5 x.  x - mean loses the leading 17 bits of x = 1e3 + 1e-2 N(0, 1), so what fp32 keeps of the variance is a few per cent at best.
LN_CANCEL_ROWS = (3, 4, 5, 1027, 15, 16, 17, 33, 45, 48, 51, 64, 99, 192)          # every row count >= 3 the forward and mean tests use
LN_CANCEL_F32 = {
    32: 1.21e-05,          # measured 1.206e-05 (rows 64); all: 2.7e-06 2.7e-06 5.1e-07 8.0e-06 1.0e-08 9.3e-07 4.7e-06 2.0e-06 1.1e-07 1.8e-06 7.4e-06 1.2e-05 8.8e-06 1.1e-06
    64: 1.25e-05,          # measured 1.241e-05 (rows 51); all: 3.6e-07 4.8e-06 2.8e-07 5.8e-06 1.9e-06 1.1e-05 4.4e-06 4.3e-07 7.9e-06 6.4e-06 1.2e-05 5.1e-07 5.6e-07 8.2e-06
    128: 1.64e-05,          # measured 1.636e-05 (rows 15); all: 4.3e-07 1.0e-06 1.7e-07 2.6e-06 1.6e-05 2.3e-07 7.4e-08 9.4e-06 1.1e-06 7.4e-07 1.8e-06 4.1e-06 2.0e-07 2.7e-06
    100: 9.86e-05,          # measured 9.855e-05 (rows 51); all: 2.9e-05 1.3e-05 2.3e-06 8.8e-06 3.5e-06 1.1e-05 3.2e-05 5.1e-08 4.4e-06 6.3e-06 9.9e-05 2.0e-06 1.2e-08 2.0e-05
}
LN_CANCEL_GATE = {k: 5 * v for k, v in LN_CANCEL_F32.items()}


@functools.lru_cache(maxsize=None)
def lnb_inputs(rows, n):
    """x, dy (rows, n), g fp32 and the float64 forward's statistics rounded to fp32"""
    tag = f"lnb{rows}_{n}"
    x = (prng.normal(tag + "x", (rows, n), seed=71).astype(np.float64) * 1.5 + 0.5 * prng.normal(tag + "o", (rows, 1), seed=72)).astype(np.float32)
    dy = prng.normal(tag + "d", (rows, n), seed=73).astype(np.float32)
    g = (1.0 + 0.2 * prng.normal(tag + "g", (n,), seed=74)).astype(np.float32)
    _, mean, rstd = R.ln_fwd(x.astype(np.float64), g.astype(np.float64), np.zeros(n))
    stats = np.stack([mean, rstd], -1).astype(np.float32)
    return frozen(x, dy, g, stats)
