"""Inputs, epilogue cases and the launch-site table shared by tests/test_gpu_gemm_epilogue.py (GPU) and tests/test_gemm_epi_ref_host.py (host).

Operands are asymmetric: a fixed-seed draw (hulc_amd.utils.portable_rng) plus a row-dependent and a column-dependent ramp, so that a transposed or shifted
result shows.  Masks hold positives, negatives, +0.0 and -0.0.  Magnitudes are of order 0.5, so that the longest sum here (K = 6144) stays below 2000 and far
below fp16's 65504 (the host test checks that on the reference)."""
import functools

import numpy as np

import plan_ln_inputs as PI
from hulc_amd.utils import portable_rng as prng

DTYPES = ("bf16", "fp16", "fp32")
DTYPES16 = ("bf16", "fp16")
SEED = 0x5EED1234ABCD
OLD = 7.0          # what every output buffer holds before a launch (plan_ln_gpu_util.sevens): the accumulate cases add to it, gaps and guards must keep it

# HULC_GEMM_RAN_* (hulc_amd/lib.py GEMM_RAN)
RAN_32, RAN_64, RAN_128, RAN_GLDS, RAN_ROUTER, RAN_REG, RAN_KCHUNK, RAN_SPLIT64, RAN_SPLIT128 = range(1, 10)
RAN_DUAL = 12      # 10 and 11: retired launch forms, not reused


@functools.lru_cache(maxsize=None)
def matrix(tag, rows, cols, dtype, scale=0.5):
    """[rows][cols] float64, rounded to the storage type: scale * N(0, 1) + a ramp down the rows (+0.2 over the matrix) and one along the columns (-0.15)"""
    x = scale * prng.normal(f"ge_{tag}_{rows}_{cols}", (rows, cols), seed=61).astype(np.float64)
    x = x + 0.2 * (np.arange(rows)[:, None] / max(rows, 1)) - 0.15 * (np.arange(cols)[None, :] / max(cols, 1))
    return PI.frozen(PI.round_t(x, dtype))


@functools.lru_cache(maxsize=None)
def vector(tag, n):
    """a bias: fp32 values, a ramp plus a draw"""
    x = 0.3 * prng.normal(f"ge_v{tag}_{n}", (n,), seed=62).astype(np.float64) + 0.5 * np.arange(n) / n - 0.2
    return PI.frozen(x.astype(np.float32).astype(np.float64))


@functools.lru_cache(maxsize=None)
def mask_values(tag, n, dtype, tanh):
    """n mask values in the storage type: a draw in (-1, 1) where every 5th element is +0.0 and every 7th is -0.0 (ReLU masks treat both as "not positive")"""
    x = prng.uniform(f"ge_m{tag}_{n}", (n,), -0.95 if tanh else -1.5, 0.95 if tanh else 1.5, seed=63).astype(np.float64)
    x[::5] = 0.0
    x[3::7] = -0.0
    return PI.frozen(PI.round_t(x, dtype))


# ---------------------------------------------------------------------------------------------------- epilogue cases
# name -> the EpiP fields that differ from a bare store.  res: "t" (storage type) or "f32"; mask: 1; out2: (lo fraction, hi fraction) of the output's extent,
# rounded to multiples of 4 (0, 1 = the whole output), "first" = rows [0, rowmod) of the engine's H[0] store, "last" = the last rows (dZ[S-1]).
EPI = {
    "bare16": dict(),
    "bare32": dict(out_f32=1),
    # ---- one field alone
    "alpha": dict(out_f32=1, alpha=1.25),
    "bias": dict(out_f32=1, bias=1),
    "bias2": dict(out_f32=1, bias2=1),
    "bias12_16": dict(bias=1, bias2=1),
    "res16": dict(res="t"),
    "res32": dict(out_f32=1, res="f32"),
    "res16_vs_32": dict(res="f32"),
    "res_late": dict(out_f32=1, res="f32", res_late=1),
    "rowmod": dict(res="t", res_rowmod=6),
    "relu": dict(relu=1),
    "tanh": dict(out_f32=1, relu=2),
    "mask": dict(mask=1),
    "mask_tanh": dict(mask=1, mask_tanh=1),
    "drop": dict(out_f32=1, drop_p=0.3),
    "acc32": dict(out_f32=1, accumulate=1),
    "acc16": dict(accumulate=1),
    "out2_copy": dict(out_f32=1, out2=(0.0, 1.0)),
    "out2_window": dict(out2=(0.3, 0.7), out2_relu=1),
    "out2_mask": dict(out2=(0.5, 1.0), out2_mask=1),
    # ---- pairs
    "res_late_drop": dict(out_f32=1, bias=1, res="f32", res_late=1, drop_p=0.1),          # engine_forward.inc:157 / :161, x + dropout(linear(x))
    "relu_drop": dict(bias=1, relu=1, drop_p=0.1),                                        # engine_forward.inc:159
    "alpha_bias": dict(out_f32=1, alpha=0.75, bias=1),
    "mask_alpha": dict(mask=1, alpha=1.0 / (1.0 - 0.1)),                                  # engine_backward.inc:394
    "rnn_fwd": dict(res="t", relu=1),                                                     # engine_recurrent.inc:107 / :145
    "rnn_fwd_tanh": dict(res="t", relu=2),                                                # engine_recurrent.inc:145 with act = 2, :220
    "rnn_bwd": dict(mask=1, res="t"),                                                     # engine_recurrent.inc:126 / :177
    "rnn_bwd_tanh": dict(mask=1, mask_tanh=1, res="t"),
    "zx0": dict(res="t", res_rowmod=6, out2="first", out2_relu=1),                        # engine_forward.inc:199
    "zx1": dict(bias=1, bias2=1, out2="first", out2_relu=1),                              # engine_forward.inc:203
    "dh_last": dict(out2="last", out2_mask=1),                                            # engine_backward.inc:210 / :276
    "cplan": dict(out_f32=1, bias=1, bias2=1),                                            # engine_forward.inc:182
    "dnext": dict(out_f32=1, res="f32"),                                                  # engine_backward.inc:396 / :432
}
for _k, _v in EPI.items():
    _v.setdefault("name", _k)

TANH_CASES = ("tanh", "rnn_fwd_tanh")


def uses_fast_path(e, dtype):
    """the case can take epi_fast16 (16-bit types) or epi_plain4: alpha == 1 by their definition, no dropout / tanh / late residual"""
    if e.get("alpha", 1.0) != 1.0 or e.get("drop_p", 0) or e.get("relu", 0) == 2 or e.get("mask_tanh", 0):
        return False
    if e.get("out_f32", 0):
        return not any(e.get(k) for k in ("bias", "bias2", "res", "mask", "relu", "out2"))
    return dtype != "fp32" and not e.get("accumulate", 0) and not e.get("res_late", 0)


# ---------------------------------------------------------------------------------------------------- the engine's launch sites
# (site, file:line it mirrors, EPI case with the same flags, shape (M, N, K) as a function of B, S and the dims d).  The host test asks gemm_pick for every site at
# the shipped shapes and requires the pick to be a (kernel family, k-step) the GPU file covers.
def dims(kind):
    mcil = kind in ("mcil", "mcil_gru")
    d = dict(EMB=128, HID=2048, FCH=4096, FF=2048, GOAL=32, PLAN=512 if mcil else 1024, NHEAD=224 if mcil else 192, DE=128 if mcil else 64)
    d["dec_plan"] = 0 if kind == "gcbc" else (d["PLAN"] // 2 if mcil else d["PLAN"])
    return d


SITES = [
    ("tr_in", "engine_forward.inc:154", "bias12_16", lambda B, S, d: (B * S, 3 * d["EMB"], d["EMB"])),
    ("tr_out", "engine_forward.inc:157", "res_late_drop", lambda B, S, d: (B * S, d["EMB"], d["EMB"])),
    ("tr_l1", "engine_forward.inc:159", "relu_drop", lambda B, S, d: (B * S, d["FF"], d["EMB"])),
    ("tr_l2", "engine_forward.inc:161", "res_late_drop", lambda B, S, d: (B * S, d["EMB"], d["FF"])),
    ("pr_fc", "engine_forward.inc:167", "out2_copy", lambda B, S, d: (B, d["FCH"], d["EMB"])),
    ("pr_fs", "engine_forward.inc:168", "bias", lambda B, S, d: (B, d["PLAN"], d["FCH"])),
    ("cplan", "engine_forward.inc:182", "cplan", lambda B, S, d: (B, d["HID"], max(d["dec_plan"], 32))),
    ("cb", "engine_forward.inc:186", "res16_vs_32", lambda B, S, d: (B, d["HID"], d["GOAL"])),
    ("zx0", "engine_forward.inc:199", "zx0", lambda B, S, d: (B * S, d["HID"], d["DE"])),
    ("zx1", "engine_forward.inc:203", "zx1", lambda B, S, d: (B * S, d["HID"], d["HID"])),
    ("heads", "engine_forward.inc:207", "bias", lambda B, S, d: (B * S, d["NHEAD"], d["HID"])),
    ("mlp_fwd", "engine_forward.inc:8", "relu", lambda B, S, d: (B, d["HID"], d["HID"])),
    ("mlp_bwd", "engine_forward.inc:40", "mask", lambda B, S, d: (B, d["HID"], d["HID"])),
    ("rnn_step", "engine_recurrent.inc:107", "rnn_fwd", lambda B, S, d: (B, d["HID"], d["HID"])),
    ("rnn_bptt", "engine_recurrent.inc:126", "rnn_bwd", lambda B, S, d: (B, d["HID"], d["HID"])),
    ("birnn_zx", "engine_recurrent.inc:207", "bias12_16", lambda B, S, d: (B * S, d["HID"], d["EMB"])),
    ("birnn_tanh", "engine_recurrent.inc:220", "rnn_fwd_tanh", lambda B, S, d: (B, d["HID"], d["HID"])),
    ("gru_g", "engine_recurrent.inc:241", "bias", lambda B, S, d: (B, 3 * d["HID"], d["HID"])),
    ("gru_carry", "engine_recurrent.inc:271", "res16", lambda B, S, d: (B, d["HID"], 3 * d["HID"])),
    ("dh1", "engine_backward.inc:210", "dh_last", lambda B, S, d: (B * S, d["HID"], d["NHEAD"])),
    ("dw_hh1", "engine_backward.inc:269", "acc32", lambda B, S, d: (d["HID"], d["HID"], B * S)),
    ("dw_ih0", "engine_backward.inc:294", "acc32", lambda B, S, d: (d["HID"], d["DE"], B * S)),
    ("demb", "engine_backward.inc:298", "acc32", lambda B, S, d: (B * S, d["DE"], d["HID"])),
    ("dplan", "engine_backward.inc:310", "bare32", lambda B, S, d: (B, max(d["dec_plan"], 32), d["HID"])),
    ("dseqf", "engine_backward.inc:335", "out2_copy", lambda B, S, d: (B, d["FCH"], d["PLAN"])),
    ("dxm", "engine_backward.inc:357", "bare32", lambda B, S, d: (B, d["EMB"], d["FCH"])),
    ("tr_dl2", "engine_backward.inc:394", "mask_alpha", lambda B, S, d: (B * S, d["FF"], d["EMB"])),
    ("tr_dl1", "engine_backward.inc:396", "dnext", lambda B, S, d: (B * S, d["EMB"], d["FF"])),
    ("tr_dout", "engine_backward.inc:418", "bare16", lambda B, S, d: (B * S, d["EMB"], d["EMB"])),
    ("tr_din", "engine_backward.inc:432", "dnext", lambda B, S, d: (B * S, d["EMB"], 3 * d["EMB"])),
]
SHIPPED = [(kind, B, S) for kind in ("hulc", "gcbc", "mcil", "mcil_gru") for B, S in ((64, 32), (2, 4), (3, 5))]          # the benchmark's shape and the goldens' sizes

# ---------------------------------------------------------------------------------------------------- GPU cases: (kernel, M, N, K) per kernel
TILE_SHAPES = {1: (45, 38), 2: (70, 67), 3: (130, 133)}          # one tile plus a remainder that is no multiple of 4
TILE_KS = (40, 96, 128, 136, 264)                               # across the BK choices 32 / 64 / 128 and their tails
GLDS_KS = (64, 96, 128, 192, 256, 288)                          # 1 .. 4 ring stages, the ring wrap, the half step before and after it
SKINNY_MS, SKINNY_NS, SKINNY_KS = (1, 16, 17, 33, 64), (16, 48), (128, 160, 512, 1024, 2048)
KCHUNK_SHAPES = ((33, 32, 4096), (64, 16, 6144))
SPLITK_SHAPES = ((64, 64, 1024), (130, 140, 2048))


def expected_ran(kernel, dtype, M, N, K):
    """what the entry must report for a forced kernel"""
    return {1: RAN_32, 2: RAN_64, 3: RAN_128, 4: RAN_GLDS, 5: RAN_ROUTER, 6: RAN_REG, 7: RAN_KCHUNK, 8: RAN_SPLIT128 if (M >= 128 and N >= 128) else RAN_SPLIT64}[kernel]


def covered_picks():
    """(family, k-step) pairs the GPU file's cases run, per type class ("16", "32")"""
    c16 = {(RAN_ROUTER, 0), (RAN_GLDS, 0)}
    for t, fam in ((1, RAN_32), (2, RAN_64), (3, RAN_128)):
        for K in TILE_KS:
            c16.add((fam, 32 if K < 128 else (64 if t == 3 else 128)))
    c32 = {(fam, 32) for fam in (RAN_32, RAN_64, RAN_128)}
    return {"16": c16, "32": c32}
