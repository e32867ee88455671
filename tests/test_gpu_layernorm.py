"""GPU (-m gpu): the LayerNorm family of csrc/kernels.h alone, through its C-ABI test entries and the launch helpers the engine itself calls
(csrc/plan_ln_launch.h), element by element against float64 (tests/plan_ln_ref.py): layernorm_fwd, layernorm_mean, and the backward as each engine runs it —
layernorm_bwd_fused (bf16, fp16) and layernorm_bwd + dropout_apply + layernorm_param_grad + colsum_final (fp32).  Every output buffer starts at 7.0; the
gaps of strided buffers and the guard rows past the end must still hold 7.0 afterwards, and the gaps of strided inputs hold NaN.

Gates.  Statistics: 2e-5 relative per row, mean and rstd; rstd of the cancellation row (mean 1e3, spread 1e-2): 5 x the float32-vs-float64 error measured per
n (tests/plan_ln_inputs.py LN_CANCEL_F32, re-measured by tests/test_plan_ln_ref_host.py).  Outputs: 2e-5 max|ref| (fp32), + one ulp of the storage type
(16 bit); the cancellation row's outputs are compared with float64 arithmetic on the device's own statistics of that row (its x - mean is exact in fp32, so
the row's error is that of its statistics, gated above).  dg, db: sums of `rows` addends in any order, (rows + 16) 2^-24 sum|addends| per column from the
reference's own addends."""
import numpy as np
import pytest

import hulc_oracle as O
import plan_ln_inputs as I
import plan_ln_ref as R
from plan_ln_gpu_util import GUARD, check16, check32, check_tol, dev, f64, guard_intact, load, ptr, refused, sevens

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NAN = float("nan")


def strided(x, ld, fill=NAN):
    """x (rows, n) on the device in a (rows, ld) fp32 buffer whose gaps hold `fill`"""
    rows, n = x.shape
    t = torch.full((rows, ld), fill, device="cuda", dtype=torch.float32)
    t[:, :n] = dev(x)
    return t


def split_gaps(t, rows, n, what):
    """a (rows + GUARD, ld) output buffer: guard rows and the gap columns intact -> the (rows, n) payload as float64"""
    guard_intact(t, rows, what)
    assert (t[:rows, n:].float() == 7.0).all(), f"{what}: the gap between rows was written"
    return f64(t[:rows, :n])


def stats_check(st, mean, rstd, n, cancel_row, what):
    """mean and rstd 2e-5 relative per row; rstd of the cancellation row at its measured gate"""
    tol_r = I.LN_STAT * rstd
    if cancel_row is not None and n > 1:
        tol_r = tol_r.copy()
        tol_r[cancel_row] = max(I.LN_CANCEL_GATE[n], I.LN_STAT) * rstd[cancel_row]
    check_tol(np.abs(st[:, 0] - mean), I.LN_STAT * np.abs(mean), st[:, 0], mean, what + " mean")
    check_tol(np.abs(st[:, 1] - rstd), tol_r, st[:, 1], rstd, what + " rstd")


def y_reference(x, g, b, st_dev, cancel_row):
    """float64 LayerNorm; the cancellation row from the device's own statistics"""
    y, mean, rstd = R.ln_fwd(x, g, b)
    if cancel_row is not None:
        y[cancel_row] = (x[cancel_row] - st_dev[cancel_row, 0]) * st_dev[cancel_row, 1] * g + b
    return y, mean, rstd


# ==================================================================================================== forward
@pytest.mark.parametrize("dtype", I.DTYPES)
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 1027])
@pytest.mark.parametrize("n", [32, 64, 128, 1, 100])
def test_layernorm_forward_matches_fp64(n, rows, dtype):
    L, lib = load()
    x, g, b = I.ln_inputs(rows, n)
    ldx, ldo, ldf = n + 3, n + 5, n + 2
    x_t, g_t, b_t = strided(x, ldx), dev(g), dev(b)
    x64, g64, b64 = (a.astype(np.float64) for a in (x, g, b))
    cancel = I.LN_ROW_CANCEL if rows >= 3 else None
    st_dev = None
    for absent in (None, "out", "out_f32", "stats"):
        out = None if absent == "out" else sevens((rows, ldo), dtype)
        outf = None if absent == "out_f32" else sevens((rows, ldf))
        stats = None if absent == "stats" else sevens((rows, 2))
        L.check(lib.hulc_k_layernorm_fwd(L.DTYPE[dtype], x_t.data_ptr(), ldx, rows, n, g_t.data_ptr(), b_t.data_ptr(), ptr(out), ldo, ptr(outf), ldf, ptr(stats), None))
        torch.cuda.synchronize()
        what = f"ln_fwd [{dtype}] rows={rows} n={n} without {absent}"
        if stats is not None:
            guard_intact(stats, rows, "stats")
            st = f64(stats[:rows])
            if st_dev is None:
                st_dev = st
            assert (st == st_dev).all(), "the statistics do not depend on which outputs are asked for"
        y, mean, rstd = y_reference(x64, g64, b64, st_dev, cancel)
        if stats is not None:
            stats_check(st, mean, rstd, n, cancel, what)
            if rows >= 3:
                assert st[I.LN_ROW_CONST, 0] == 2.25 and abs(st[I.LN_ROW_CONST, 1] * np.sqrt(1e-5) - 1) <= I.LN_STAT, "the constant row: variance 0"
        if out is not None:
            check16(split_gaps(out, rows, n, "out"), y, dtype, what + " out")
        if outf is not None:
            check32(split_gaps(outf, rows, n, "out_f32"), y, what + " out_f32")


# ==================================================================================================== LayerNorm + mean over S
@pytest.mark.parametrize("dtype", I.DTYPES)
@pytest.mark.parametrize("n", [128, 64])
@pytest.mark.parametrize("S", [1, 15, 16, 17, 33, 64])
@pytest.mark.parametrize("B", [1, 3])
def test_layernorm_mean_matches_fp64(B, S, n, dtype):
    L, lib = load()
    rows = B * S
    x, g, b = I.ln_inputs(rows, n)
    stats, out, yout = sevens((rows, 2)), sevens((B, n), dtype), sevens((rows, n))
    x_t, g_t, b_t = dev(x), dev(g), dev(b)          # named: a temporary's memory is reused by the next allocation
    L.check(lib.hulc_k_layernorm_mean(L.DTYPE[dtype], x_t.data_ptr(), B, S, n, g_t.data_ptr(), b_t.data_ptr(), stats.data_ptr(), out.data_ptr(), yout.data_ptr(), None))
    torch.cuda.synchronize()
    for t, k, m in ((stats, "stats", rows), (out, "out", B), (yout, "yout", rows)):
        guard_intact(t, m, k)
    what = f"ln_mean [{dtype}] B={B} S={S} n={n}"
    cancel = I.LN_ROW_CANCEL if rows >= 3 else None
    st = f64(stats[:rows])
    y, mean, rstd = y_reference(*(a.astype(np.float64) for a in (x, g, b)), st, cancel)
    stats_check(st, mean, rstd, n, cancel, what)
    yd = f64(yout[:rows])
    check32(yd, y, what + " yout")
    check16(f64(out[:B]), yd.reshape(B, S, n).mean(1), dtype, what + " out (mean over S of the device's yout)")


# ==================================================================================================== backward
def lnb_run(lib, L, dtype, rows, n, dy_t, lddy, accumulate=0, want_f=True, want_t=True, drop_p=0.0, seed=0, bcast_rows=0, dy_parts=1, part_stride=0):
    """-> dict(dx_f32, dx_t (rows, n) float64 or None, dg, db (n,), dxf0, dg0, db0: what the accumulating outputs started from)"""
    x, _, g, stats = I.lnb_inputs(rows, n)
    ldx, ldd, ldt = n + 2, n + 3, n + 4
    if dtype == "fp32" and drop_p > 0:
        ldd = ldt = n          # dropout_apply_kernel walks both as one flat array
    tag = f"lnb{rows}_{n}"
    dxf0 = I.prng.normal(tag + "a", (rows, n), seed=75).astype(np.float32)
    dg0 = I.prng.normal(tag + "g0", (n,), seed=76).astype(np.float32)
    db0 = I.prng.normal(tag + "b0", (n,), seed=77).astype(np.float32)
    dxf = dxt = None
    if want_f:
        dxf = sevens((rows, ldd))
        if accumulate:
            dxf[:rows, :n] = dev(dxf0)
    if want_t:
        dxt = sevens((rows, ldt), dtype)
    dg, db = sevens(n), sevens(n)
    dg[:n], db[:n] = dev(dg0), dev(db0)
    scratch = sevens(2 * 64 * n)
    x_t, st_t, g_t = strided(x, ldx), dev(stats), dev(g)          # named: a temporary's memory is reused by the next allocation
    L.check(lib.hulc_k_layernorm_bwd(L.DTYPE[dtype], dy_t.data_ptr(), lddy, x_t.data_ptr(), ldx, st_t.data_ptr(), g_t.data_ptr(), rows, n, ptr(dxf), ldd,
                                     accumulate, ptr(dxt), ldt, dg.data_ptr(), db.data_ptr(), drop_p, seed, bcast_rows, float(max(bcast_rows, 1)), dy_parts, part_stride,
                                     scratch.data_ptr(), None))
    torch.cuda.synchronize()
    guard_intact(dg, n, "dg")
    guard_intact(db, n, "db")
    guard_intact(scratch, 2 * 64 * n, "scratch")
    return dict(dx_f32=split_gaps(dxf, rows, n, "dx_f32") if want_f else None, dx_t=split_gaps(dxt, rows, n, "dx_t") if want_t else None, dg=f64(dg[:n]), db=f64(db[:n]),
                dxf0=dxf0.astype(np.float64), dg0=dg0.astype(np.float64), db0=db0.astype(np.float64))


def lnb_check(o, dy_eff, rows, n, dtype, accumulate, what, keep=None, drop_p=0.0):
    """dy_eff (rows, n) float64: the gradient the launch stands for.  -> worst err/tol of (dx, dg, db)"""
    x, _, g, stats = (a.astype(np.float64) for a in I.lnb_inputs(rows, n))
    dx, ag, ab = R.ln_bwd(dy_eff, x, stats[:, 0], stats[:, 1], g)
    w = [0.0, 0.0, 0.0]
    if o["dx_f32"] is not None:
        ref = dx + o["dxf0"] if accumulate else dx
        w[0] = check32(o["dx_f32"], ref, what + " dx_f32")
    if o["dx_t"] is not None:
        ref = dx if keep is None else np.where(keep, dx / (1.0 - np.float64(np.float32(drop_p))), 0.0)
        w[0] = max(w[0], check16(o["dx_t"], ref, dtype, what + " dx_t"))
        if keep is not None:
            assert (o["dx_t"][~keep] == 0).all(), "dropped elements are exactly zero"
    for k, (got, add, start) in enumerate(((o["dg"], ag, o["dg0"]), (o["db"], ab, o["db0"]))):
        ref = start + add.sum(0)
        gate = (rows + 16) * I.EPS32 * (np.abs(start) + np.abs(add).sum(0))
        w[1 + k] = check_tol(np.abs(got - ref), gate, got, ref, what + (" dg" if k == 0 else " db"))
    return w, (dx, ag, ab)


@pytest.mark.parametrize("dtype", I.DTYPES)
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 17, 1023, 1024, 1027])
@pytest.mark.parametrize("n", [32, 64, 128])
def test_layernorm_backward_matches_fp64(n, rows, dtype):
    """both block shapes of the fused kernel (4 rows up to 1023, 16 from 1024) with a ragged last block in each; the fp32 pair with 1 to 17 row chunks"""
    L, lib = load()
    dy = I.lnb_inputs(rows, n)[1]
    lddy = n + 1
    dy_t = strided(dy, lddy)
    worst = np.zeros(3)
    for accumulate, want_f, want_t in ((0, True, True), (1, True, True), (0, True, False), (0, False, True)):
        o = lnb_run(lib, L, dtype, rows, n, dy_t, lddy, accumulate, want_f, want_t)
        w, _ = lnb_check(o, dy.astype(np.float64), rows, n, dtype, accumulate, f"ln_bwd [{dtype}] rows={rows} n={n} acc={accumulate} f32={want_f} t={want_t}")
        worst = np.maximum(worst, w)
    print(f"ln_bwd [{dtype} rows={rows} n={n}]: worst err/tol dx {worst[0]:.3g} dg {worst[1]:.3g} db {worst[2]:.3g}")


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("rows", [5, 1027])
@pytest.mark.parametrize("n", [32, 64, 128])
def test_layernorm_backward_dropout_mask(n, rows, dtype):
    """drop_p = 0.1 on the 16-bit copy: the keep mask of element row * n + col, dx / (1 - p) where kept, exactly 0 where dropped; dx_f32 stays unmasked"""
    L, lib = load()
    dy = I.lnb_inputs(rows, n)[1]
    seed, p = 0x5EED0000 + rows, 0.1
    keep = O.engine_keep_mask(seed, (rows, n), p)
    assert 0 < (~keep).sum() < keep.size
    o = lnb_run(lib, L, dtype, rows, n, strided(dy, n + 1), n + 1, drop_p=p, seed=seed)
    lnb_check(o, dy.astype(np.float64), rows, n, dtype, 0, f"ln_bwd dropout [{dtype}] rows={rows} n={n}", keep=keep, drop_p=p)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("bc", [7, 16])
@pytest.mark.parametrize("n", [32, 128])
def test_layernorm_backward_broadcast_rows(n, bc, dtype):
    """dy holds one row per window of bc rows, divided by bc (the mean over S in front of it)"""
    L, lib = load()
    rows = 3 * bc
    dyw = I.prng.normal(f"bc{bc}_{n}", (3, n), seed=78).astype(np.float32)
    o = lnb_run(lib, L, dtype, rows, n, strided(dyw, n + 1), n + 1, bcast_rows=bc)
    lnb_check(o, np.repeat(dyw.astype(np.float64), bc, 0) / bc, rows, n, dtype, 0, f"ln_bwd bcast {bc} [{dtype}] n={n}")


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("rows", [5, 1027])
@pytest.mark.parametrize("n", [64, 128])
def test_layernorm_backward_sums_four_partial_gradients(n, rows, dtype):
    L, lib = load()
    lddy = n + 1
    stride = rows * lddy + 13
    parts = I.prng.normal(f"pt{rows}_{n}", (4, rows, n), seed=79).astype(np.float32)
    buf = torch.full((4 * stride,), NAN, device="cuda", dtype=torch.float32)
    for k in range(4):
        buf[k * stride:k * stride + rows * lddy].view(rows, lddy)[:, :n] = dev(parts[k])
    o = lnb_run(lib, L, dtype, rows, n, buf, lddy, dy_parts=4, part_stride=stride)
    lnb_check(o, parts.astype(np.float64).sum(0), rows, n, dtype, 0, f"ln_bwd 4 parts [{dtype}] rows={rows} n={n}")


@pytest.mark.parametrize("rows,n", [(17, 64), (1027, 128)])
def test_layernorm_backward_three_types_agree(rows, n):
    """identical fp32 inputs through the fused kernel of both 16-bit builds and the fp32 pair: within the sum of their gates"""
    L, lib = load()
    dy = I.lnb_inputs(rows, n)[1]
    res = {}
    for dtype in I.DTYPES:
        o = lnb_run(lib, L, dtype, rows, n, strided(dy, n + 1), n + 1)
        _, (dx, ag, ab) = lnb_check(o, dy.astype(np.float64), rows, n, dtype, 0, f"ln_bwd [{dtype}] rows={rows} n={n}")
        res[dtype] = o
    for a, b in (("bf16", "fp16"), ("bf16", "fp32"), ("fp16", "fp32")):
        assert np.abs(res[a]["dx_f32"] - res[b]["dx_f32"]).max() <= 2 * I.ACC * np.abs(dx).max()
        for k, add, start in (("dg", ag, "dg0"), ("db", ab, "db0")):
            gate = (rows + 16) * I.EPS32 * (np.abs(res[a][start]) + np.abs(add).sum(0))
            assert (np.abs(res[a][k] - res[b][k]) <= 2 * gate).all(), (a, b, k)


# ==================================================================================================== argument validation
def test_layernorm_entries_validate_their_arguments():
    """every refusal names its entry, and nothing is launched: the output buffers keep their 7.0"""
    L, lib = load()
    f, h, out = sevens((64, 256)), sevens((64, 256), "bf16"), sevens((64, 256))
    p, o, hp = f.data_ptr(), out.data_ptr(), h.data_ptr()
    BF, F32 = L.DTYPE["bf16"], L.DTYPE["fp32"]

    def fw(dt=BF, x=p, ldx=64, rows=4, n=64, g=p, out_=hp, ldo=64, stats=o):
        return lib.hulc_k_layernorm_fwd(dt, x, ldx, rows, n, g, p, out_, ldo, o, 64, stats, None)
    for rc in (fw(x=None), fw(g=None), fw(n=129), fw(n=0), fw(rows=0), fw(ldx=63), fw(ldo=63), fw(x=p + 2), fw(out_=hp + 1), fw(dt=F32, out_=hp + 2), fw(stats=o + 1), fw(dt=4)):
        refused(lib, rc, "hulc_k_layernorm_fwd")

    def bw(dt=BF, dy=p, stats=p, rows=8, n=64, dxf=o, dxt=hp, dg=o, acc=0, drop_p=0.0, bcast=0, div=1.0, parts=1, stride=0, scratch=o, lddy=64):
        return lib.hulc_k_layernorm_bwd(dt, dy, lddy, p, 64, stats, p, rows, n, dxf, 64, acc, dxt, 64, dg, o, drop_p, 0, bcast, div, parts, stride, scratch, None)
    for rc in (bw(dy=None), bw(stats=None), bw(dg=None), bw(dxf=None, dxt=None), bw(n=129), bw(rows=0), bw(lddy=63), bw(dxf=None, acc=1), bw(drop_p=1.0), bw(drop_p=-0.1),
               bw(dt=F32, dxt=None, bcast=4, div=4.0), bw(dt=F32, dxt=None, parts=2, stride=8 * 64), bw(dt=F32, dxt=None, scratch=None), bw(dt=F32, dxt=None, drop_p=0.1),
               bw(bcast=3, div=3.0), bw(bcast=4, div=0.0), bw(parts=5, stride=8 * 64), bw(parts=2, stride=7 * 64), bw(dxt=hp + 1), bw(dy=p + 2), bw(dt=3)):
        refused(lib, rc, "hulc_k_layernorm_bwd")

    def mn(dt=BF, x=p, B=2, S=4, n=64, out_=hp, yout=o):
        return lib.hulc_k_layernorm_mean(dt, x, B, S, n, p, p, o, out_, yout, None)
    for rc in (mn(x=None), mn(out_=None), mn(yout=None), mn(S=0), mn(B=0), mn(n=129), mn(out_=hp + 1), mn(x=p + 1), mn(dt=8)):
        refused(lib, rc, "hulc_k_layernorm_mean")
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (h == 7.0).all() and (f == 7.0).all(), "a refused call wrote to a buffer"
