"""Inputs, cases and measured allowances shared by tests/test_gpu_tr_fused.py (GPU) and tests/test_tr_fused_ref_host.py (host, which asserts the input
conditions and re-measures every measured number so that none of them rests on a kernel's output).  Inputs come from hulc_amd.utils.portable_rng (fixed seeds,
built on the host); the backward kernels' inputs (y2, statistics, hff, qkv, Pat, y1) are the float64 forward chain of tests/tr_fused_ref.py with the kernels'
storage roundings, under the engine's own dropout masks (oracle: engine_keep_mask)."""
import functools

import numpy as np

import hulc_oracle as O
import tr_fused_ref as T
from hulc_amd.utils import portable_rng as prng
from plan_ln_inputs import frozen, round_t

DTYPES16 = ("bf16", "fp16")
S_NARROW = (1, 15, 16, 17, 31, 32)          # tr_layer_fwd_kernel<false>: below, at and above the 16-row tile edge, a full window
S_WIDE = (33, 47, 48, 49, 64)          # <true>: second halves of 1, 15, 16, 17 and 32 rows
S_FWD = S_NARROW + S_WIDE
S_ATTN = (1, 2, 15, 16, 17, 31, 32)
BS = (1, 3)
DPS = (0.0, 0.1, 0.5)
SEEDS = dict(att=0x5EED0A77, o=0x5EED000F, h=0x5EED00FF, y=0x5EED0002)          # one per dropout site, as Engine::site_seed gives each its own


def r32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def params(dtype):
    """float64 values of the layer's parameters: weights rounded to the storage type, biases and LayerNorm affine fp32.  Scales: q, k of standard deviation
    ~1 per element (attention rows neither uniform nor one-hot), hidden pre-activations of standard deviation ~1 around biases of +-0.1 (about half active),
    every branch of order 1 next to its residual.  LayerNorm affine with jitter, no bias zero."""
    n = lambda name, shape, std, seed: prng.normal("trf_" + name, shape, std, seed).astype(np.float64)
    P = dict(Wqkv=round_t(n("Wqkv", (3 * T.D, T.D), 0.082, 101), dtype), Wo=round_t(n("Wo", (T.D, T.D), 0.09, 102), dtype),
             W1=round_t(n("W1", (T.FF, T.D), 0.09, 103), dtype), W2=round_t(n("W2", (T.D, T.FF), 0.03, 104), dtype),
             bqkv=r32(n("bqkv", (3 * T.D,), 0.1, 105)), bo=r32(n("bo", (T.D,), 0.1, 106)), b1=r32(n("b1", (T.FF,), 0.1, 107)), b2=r32(n("b2", (T.D,), 0.1, 108)),
             n1g=r32(1.0 + n("n1g", (T.D,), 0.2, 109)), n1b=r32(n("n1b", (T.D,), 0.2, 110)), ln_g=r32(1.0 + n("lng", (T.D,), 0.2, 111)), ln_b=r32(n("lnb", (T.D,), 0.2, 112)),
             n2g=r32(1.0 + n("n2g", (T.D,), 0.2, 113)))
    frozen(*P.values())
    return P


@functools.lru_cache(maxsize=None)
def _windows(tag, nw, rows, std, seed):
    return frozen(r32(prng.normal("trf_" + tag, (nw, rows, T.D), std, seed)))


def per_window(tag, B, rows, std, seed, other=()):
    """(B * rows, 128) fp32 values, window by window from one draw of max(B, 3) windows; the windows listed in `other` take theirs from a second draw"""
    nw = max(B, 3)
    a, b = _windows(f"{tag}_{rows}_{nw}", nw, rows, std, seed), _windows(f"{tag}_{rows}_{nw}_alt", nw, rows, std, seed + 50)
    return np.concatenate([(b if w in other else a)[w] for w in range(B)], 0)


LOW_VAR = 0.02          # spread of the first and last row of window 0: a variance of 4e-4, where the epsilon of the LayerNorm (1e-5) is 1 % of rstd


def xin(B, S, ln_in, other=()):
    """(N, 128) fp32: N(0, 1), or for ln_in a pre-norm sum (spread 1.5 around a row offset of spread 0.7).  Rows 0 and S - 1 of window 0 have the small spread
    LOW_VAR around zero"""
    if not ln_in:
        x = per_window("x", B, S, 1.0, 201, other).copy()
    else:
        x = per_window("xl", B, S, 1.5, 202, other) + np.repeat(per_window("xo", B, 1, 0.7, 203, other)[:, :1], S, 0)
    for r in (0, S - 1):
        x[r] = LOW_VAR * per_window("xs", 1, S, 1.0, 205, other)[r]
    return frozen(r32(x))


def masks(B, S, p):
    if p == 0:
        return None
    N = B * S
    return dict(att=O.engine_keep_mask(SEEDS["att"], (B, T.NH, S, S), p), o=O.engine_keep_mask(SEEDS["o"], (N, T.D), p),
                h=O.engine_keep_mask(SEEDS["h"], (N, T.FF), p), y=O.engine_keep_mask(SEEDS["y"], (N, T.D), p))


def y2_start(B, S, nonzero, other=()):
    """what y2 holds before the launch: zero (the engine's contract) or values of order 1 (pins "adds to")"""
    if not nonzero:
        return np.zeros((B * S, T.D))
    return per_window("y20", B, S, 1.0, 204, other)


@functools.lru_cache(maxsize=None)
def host_forward(dtype, B, S, ln_in, p, other=()):
    """the forward chain with the kernels' storage roundings: the saved tensors the backward kernels start from"""
    r16 = lambda x: round_t(x, dtype)
    c = T.chain_fwd(xin(B, S, ln_in, other), params(dtype), B, S, ln_in, p, masks(B, S, p), r16=r16, r32=r32)
    st2 = r32(T.ln(c["y2"], params(dtype)["n2g"], np.zeros(T.D))[1])
    c["st2"] = st2
    frozen(*c.values())
    return c


def ffn_bwd_dx(B, S, bcast, other=()):
    """the gradient of LayerNorm2's output: (N, 128), or one row per window (B, 128) that the kernel divides by S"""
    return per_window("dxw", B, 1, 1.0, 301, other) if bcast else per_window("dx2", B, S, 1.0, 302, other)


def attn_nparts(B):
    """the attention backward's incoming gradient comes as one array (B = 1) or as four (B = 3), part_stride = N * 128 + 52 floats"""
    return 4 if B == 3 else 1


def attn_bwd_parts(B, S, other=()):
    return np.stack([per_window(f"pt{k}", B, S, 0.5, 310 + k, other) for k in range(attn_nparts(B))])


def param_grad_start(name, nonzero):
    return r32(prng.normal("trf_" + name, (T.D,), 1.0, 401)) if nonzero else np.zeros(T.D)


# ---------------------------------------------------------------------------------------------------- b_b: the one hidden rounding
def bb_host(dtype, B, S, p, exact_dao):
    """b_b (float64) of the attention backward case on the host chain's tensors, with dao rounded to the storage type as the kernel rounds it in LDS, or exact"""
    c, P, mk = host_forward(dtype, B, S, 0, p), params(dtype), masks(B, S, p)
    r16 = lambda x: round_t(x, dtype)
    dy_f = r32(T.ln_bwd(attn_bwd_parts(B, S).sum(0), c["y1"], c["st1"], P["n1g"])[0])
    b_d = r16(T.drop(dy_f, None if mk is None else mk["o"], p))
    return T.b_b(b_d, P["Wo"].T, c["qkv"], c["Pat"], B, S, None if mk is None else mk["att"], p, T.ident if exact_dao else r16)[0]


def bb_measure(dtype, B, S, p):
    """max |b_b(dao rounded) - b_b(dao exact)| over the dq, dk and dv columns"""
    d = np.abs(bb_host(dtype, B, S, p, False) - bb_host(dtype, B, S, p, True))
    return tuple(float(d[:, k * T.D:(k + 1) * T.D].max()) for k in range(3))


# The kernel rounds dao = b_d W_o to 16 bit in LDS and no saved tensor exposes it.  The reference rounds its float64 dao the same way; where the device's fp32 sum
# lands on the other side of a rounding boundary the two differ by one unit in the last place of that element.  Allowance: what rounding EVERY element of dao
# does to b_b, measured per case on the host as max |b_b(dao rounded) - b_b(dao exact)| (dq, dk, dv columns; rounded up by at most a tenth), times 2 for ties
# that round the other way.  tests/test_tr_fused_ref_host.py re-measures.
BB_DAO = {          # (dtype, B, S, dp): dq, dk, dv
    ("bf16", 1, 1, 0.0): (0, 0, 0.0152),
    ("bf16", 1, 1, 0.1): (0, 0, 0.017),
    ("bf16", 1, 1, 0.5): (0, 0, 0.027),
    ("bf16", 1, 2, 0.0): (6.71e-06, 3.47e-05, 0.0147),
    ("bf16", 1, 2, 0.1): (2.96e-05, 0.000101, 0.0163),
    ("bf16", 1, 2, 0.5): (1.87e-05, 0.000102, 0.031),
    ("bf16", 1, 15, 0.0): (0.00207, 0.00125, 0.0016),
    ("bf16", 1, 15, 0.1): (0.00262, 0.00164, 0.00185),
    ("bf16", 1, 15, 0.5): (0.00309, 0.00259, 0.00275),
    ("bf16", 1, 16, 0.0): (0.00285, 0.000821, 0.00177),
    ("bf16", 1, 16, 0.1): (0.00327, 0.00167, 0.00193),
    ("bf16", 1, 16, 0.5): (0.00242, 0.00209, 0.00243),
    ("bf16", 1, 17, 0.0): (0.00307, 0.00113, 0.00202),
    ("bf16", 1, 17, 0.1): (0.00283, 0.00118, 0.00195),
    ("bf16", 1, 17, 0.5): (0.00461, 0.00221, 0.00413),
    ("bf16", 1, 31, 0.0): (0.00288, 0.000911, 0.00184),
    ("bf16", 1, 31, 0.1): (0.00344, 0.00139, 0.00145),
    ("bf16", 1, 31, 0.5): (0.00238, 0.00211, 0.00292),
    ("bf16", 1, 32, 0.0): (0.00178, 0.00119, 0.00117),
    ("bf16", 1, 32, 0.1): (0.00296, 0.000968, 0.00187),
    ("bf16", 1, 32, 0.5): (0.00301, 0.00234, 0.00247),
    ("bf16", 3, 1, 0.0): (0, 0, 0.0309),
    ("bf16", 3, 1, 0.1): (0, 0, 0.0354),
    ("bf16", 3, 1, 0.5): (0, 0, 0.0458),
    ("bf16", 3, 2, 0.0): (0.0028, 0.00275, 0.0235),
    ("bf16", 3, 2, 0.1): (0.00303, 0.00195, 0.0189),
    ("bf16", 3, 2, 0.5): (0.00723, 0.00444, 0.0584),
    ("bf16", 3, 15, 0.0): (0.00566, 0.00253, 0.00413),
    ("bf16", 3, 15, 0.1): (0.00608, 0.00369, 0.00429),
    ("bf16", 3, 15, 0.5): (0.0068, 0.0111, 0.0116),
    ("bf16", 3, 16, 0.0): (0.00532, 0.00264, 0.0042),
    ("bf16", 3, 16, 0.1): (0.00395, 0.00376, 0.00541),
    ("bf16", 3, 16, 0.5): (0.00907, 0.00715, 0.00659),
    ("bf16", 3, 17, 0.0): (0.00418, 0.00304, 0.00439),
    ("bf16", 3, 17, 0.1): (0.00384, 0.00331, 0.00554),
    ("bf16", 3, 17, 0.5): (0.00638, 0.00815, 0.00947),
    ("bf16", 3, 31, 0.0): (0.00501, 0.00277, 0.00363),
    ("bf16", 3, 31, 0.1): (0.00475, 0.00336, 0.00297),
    ("bf16", 3, 31, 0.5): (0.00562, 0.00662, 0.00708),
    ("bf16", 3, 32, 0.0): (0.00335, 0.00269, 0.00347),
    ("bf16", 3, 32, 0.1): (0.00382, 0.0033, 0.00287),
    ("bf16", 3, 32, 0.5): (0.00518, 0.00529, 0.00936),
    ("fp16", 1, 1, 0.0): (0, 0, 0.00241),
    ("fp16", 1, 1, 0.1): (0, 0, 0.0022),
    ("fp16", 1, 1, 0.5): (0, 0, 0.0034),
    ("fp16", 1, 2, 0.0): (7.17e-07, 2.83e-06, 0.00164),
    ("fp16", 1, 2, 0.1): (2.14e-06, 8.41e-06, 0.00196),
    ("fp16", 1, 2, 0.5): (3.85e-06, 1.38e-05, 0.00348),
    ("fp16", 1, 15, 0.0): (0.000308, 0.00017, 0.000355),
    ("fp16", 1, 15, 0.1): (0.000292, 0.000157, 0.000261),
    ("fp16", 1, 15, 0.5): (0.000405, 0.000298, 0.000321),
    ("fp16", 1, 16, 0.0): (0.000228, 0.000157, 0.000243),
    ("fp16", 1, 16, 0.1): (0.000293, 0.00016, 0.000343),
    ("fp16", 1, 16, 0.5): (0.000371, 0.000168, 0.000498),
    ("fp16", 1, 17, 0.0): (0.000331, 0.000123, 0.00023),
    ("fp16", 1, 17, 0.1): (0.000405, 0.000164, 0.000232),
    ("fp16", 1, 17, 0.5): (0.000399, 0.000287, 0.000376),
    ("fp16", 1, 31, 0.0): (0.000377, 0.00038, 0.000177),
    ("fp16", 1, 31, 0.1): (0.000202, 0.000143, 0.000174),
    ("fp16", 1, 31, 0.5): (0.000328, 0.000273, 0.000354),
    ("fp16", 1, 32, 0.0): (0.000223, 0.000111, 0.000166),
    ("fp16", 1, 32, 0.1): (0.00028, 0.000183, 0.000167),
    ("fp16", 1, 32, 0.5): (0.000378, 0.000284, 0.000304),
    ("fp16", 3, 1, 0.0): (0, 0, 0.00733),
    ("fp16", 3, 1, 0.1): (0, 0, 0.00429),
    ("fp16", 3, 1, 0.5): (0, 0, 0.0082),
    ("fp16", 3, 2, 0.0): (0.000385, 0.000208, 0.00249),
    ("fp16", 3, 2, 0.1): (0.000257, 0.000244, 0.00284),
    ("fp16", 3, 2, 0.5): (0.000596, 0.000501, 0.00584),
    ("fp16", 3, 15, 0.0): (0.00078, 0.000434, 0.000643),
    ("fp16", 3, 15, 0.1): (0.000799, 0.00058, 0.00063),
    ("fp16", 3, 15, 0.5): (0.00123, 0.00148, 0.00112),
    ("fp16", 3, 16, 0.0): (0.000828, 0.00047, 0.000519),
    ("fp16", 3, 16, 0.1): (0.000422, 0.000398, 0.000716),
    ("fp16", 3, 16, 0.5): (0.000888, 0.000514, 0.0014),
    ("fp16", 3, 17, 0.0): (0.000577, 0.000371, 0.000431),
    ("fp16", 3, 17, 0.1): (0.000592, 0.000449, 0.000594),
    ("fp16", 3, 17, 0.5): (0.000988, 0.000683, 0.00082),
    ("fp16", 3, 31, 0.0): (0.000567, 0.000497, 0.000399),
    ("fp16", 3, 31, 0.1): (0.000505, 0.000391, 0.000424),
    ("fp16", 3, 31, 0.5): (0.00119, 0.00109, 0.000645),
    ("fp16", 3, 32, 0.0): (0.000479, 0.000321, 0.000326),
    ("fp16", 3, 32, 0.1): (0.000753, 0.000383, 0.000416),
    ("fp16", 3, 32, 0.5): (0.000761, 0.000524, 0.000907),
}


def bb_allowance(dtype, B, S, p):
    """(N, 384): 2 x the recorded measurement of the case, per column third"""
    return np.repeat(2.0 * np.array(BB_DAO[(dtype, B, S, p)]), T.D)[None, :]
