"""Plain numpy float64 reference of the GEMM core's runtime epilogue (hulc_amd/csrc/gemm.h), written from the order EpiP's comments document, not from the kernels:

    v = acc * alpha;  + bias[col];  + bias2[col];  + res[rrow][col] when not res_late (rrow = row % res_rowmod when res_rowmod > 0);
    relu 1: max(v, 0), 2: tanh(v);  mask: v where mask > 0 else 0, or with mask_tanh v * (1 - mask^2);
    drop_p > 0: 0 where hash_uniform(drop_seed, element offset) < drop_p, else v / (1 - drop_p);  + res when res_late;  accumulate: + the old output;
    second store of the elements whose offset o lies in [out2_lo, out2_hi): out2[o - out2_lo] = max(v, 0) with out2_relu, 0 where out2_mask[o - out2_lo] <= 0.

`product` is the fp64 product with its rigorous fp32 accumulation bound, `epilogue` the steps above with the derived fp32 rounding bound per element:
(number of fp32 operations applied + 1) * 2^-24 * the sum of the magnitudes of the addends (scaled as the value is scaled), in the way of tr_fused_ref.acc_bound.
Element offsets: `offsets` maps (row, col) of the logical [M][N] result to the element offset in the output buffer — leading dimensions larger than N and the
two-level row map leave gaps, and the dropout hash and the out2 window are keyed by the offset, gaps included.  Pinned by tests/test_gemm_epi_ref_host.py."""
import numpy as np

import plan_ln_inputs as PI
import tr_fused_ref as T

EPS32 = T.EPS32


def offsets(M, N, ldc, R1=0, s0=0):
    """element offset of (row, col): row * ldc + col, or with the two-level row map (row // R1) * s0 + (row % R1) * ldc + col"""
    r = np.arange(M, dtype=np.int64)
    base = r * ldc if not s0 else (r // R1) * s0 + (r % R1) * ldc
    return base[:, None] + np.arange(N, dtype=np.int64)[None, :]


def keep_mask(seed, p, off):
    """True where the element survives dropout: not (u < float32(p)) with u = the engine's hash of the element OFFSET"""
    u = PI.hash_uniform(seed, int(off.max()) + 1)
    return ~(u[off].astype(np.float32) < np.float32(p))


def product(A, B, nsplit=1):
    """A [M][K], B [N][K] float64 -> (A B^T, bound): (K + 2 + extra) 2^-24 sum |a||b|; split K adds one rounding per slab"""
    K = A.shape[1]
    return A @ B.T, T.acc_bound(np.abs(A) @ np.abs(B).T, K, nsplit if nsplit > 1 else 0)


def epilogue(acc, f, keep=None):
    """acc [M][N] float64 (the accumulators), f: dict of the job's fields — alpha, bias [N], bias2 [N], res [rows][N], res_rowmod, res_late, relu, mask [M][N] (the
    mask values at the output's elements), mask_tanh, drop_p, accumulate + old [M][N], out2_lo / out2_hi + off [M][N] (element offsets), out2_relu, out2_mask
    (flat, out2_hi - out2_lo values).  keep [M][N] bool: the dropout decisions (required when drop_p > 0).
    -> out [M][N], out2 (flat, NaN where nothing is stored; None without a window), bound [M][N], bound2 (flat like out2)"""
    M, N = acc.shape
    alpha = float(f.get("alpha", 1.0))
    v = acc * alpha
    mag = np.abs(v)
    ops = 1 if alpha != 1.0 else 0
    for k in ("bias", "bias2"):
        if f.get(k) is not None:
            v = v + f[k][None, :]
            mag = mag + np.abs(f[k])[None, :]
            ops += 1
    res = None
    if f.get("res") is not None:
        rows = np.arange(M) % f["res_rowmod"] if f.get("res_rowmod", 0) > 0 else np.arange(M)
        res = f["res"][rows]
    if res is not None and not f.get("res_late", 0):
        v, mag, ops = v + res, mag + np.abs(res), ops + 1
    relu = f.get("relu", 0)
    if relu == 1:
        v = np.maximum(v, 0.0)
    elif relu == 2:
        v = np.tanh(v)          # the device function's own error is the caller's allowance; tanh is 1-Lipschitz, so the incoming bound carries
    if f.get("mask") is not None:
        m = f["mask"]
        if f.get("mask_tanh", 0):
            s = 1.0 - m * m
            # three operations: m * m, 1 - ., the product; the first two round relative to 1 + m^2, not to |1 - m^2| (cancellation as |m| -> 1)
            v, mag, ops = v * s, mag * np.abs(s) + np.abs(v) * (1.0 + m * m), ops + 3
        else:
            v = np.where(m > 0, v, 0.0)
            mag = np.where(m > 0, mag, 0.0)
    p = float(f.get("drop_p", 0.0))
    if p > 0:
        mult = T.mult(p)
        v = np.where(keep, v * mult, 0.0)
        mag = np.where(keep, mag * mult, 0.0)
        ops += 2          # the fp32 rounding of 1 / (1 - p) and the product
    if res is not None and f.get("res_late", 0):
        v, mag, ops = v + res, mag + np.abs(res), ops + 1
    if relu == 2:
        mag = np.maximum(mag, np.abs(v))          # tanh's result, not its argument, is what later operations round
    out, omag, oops = v, mag, ops
    if f.get("accumulate", 0):
        out, omag, oops = v + f["old"], mag + np.abs(f["old"]), ops + 1
    bound = (oops + 1) * EPS32 * omag
    out2 = bound2 = None
    if f.get("out2_hi", 0) > f.get("out2_lo", 0):
        lo, hi = f["out2_lo"], f["out2_hi"]
        out2, bound2 = np.full(hi - lo, np.nan), np.zeros(hi - lo)
        sel = (f["off"] >= lo) & (f["off"] < hi)
        o2 = f["off"][sel] - lo
        w = np.maximum(v[sel], 0.0) if f.get("out2_relu", 0) else v[sel]
        b2 = (ops + 1) * EPS32 * mag[sel]
        if f.get("out2_mask") is not None:
            mk = f["out2_mask"][o2] > 0
            w, b2 = np.where(mk, w, 0.0), np.where(mk, b2, 0.0)
        out2[o2], bound2[o2] = w, b2
    return out, out2, bound, bound2
