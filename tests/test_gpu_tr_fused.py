"""GPU (-m gpu): the three fused transformer layer kernels of csrc/tr_fused.h alone — tr_layer_fwd_kernel (narrow, S <= 32, and the two-half form, 32 < S <= 64),
tr_ffn_bwd_kernel and tr_attn_bwd_kernel — through their C-ABI test entries, launched by the helpers the engine calls, every saved tensor element by element
against the float64 stage references of tests/tr_fused_ref.py.  Each stage is computed from the DEVICE's own tensors in front of it, so rounding never
compounds; ReLU and mask decisions come from device tensors (hff > 0) and the engine's hash (oracle: engine_keep_mask), so no element is excused.  Output
buffers start at 7.0 with guard rows past the end, which must still hold 7.0: a row >= S of the last window's tile lands there.

Gates.  16-bit output of a sum of products: one ulp of the type at |ref| (never less than the spacing of its subnormal numbers) + the rigorous fp32
accumulation bound the reference returns with the sum; fp32 output: the bound alone.  Pat: 2e-6 absolute.  LayerNorm statistics: 2e-5 relative (LN_STAT), the mean also gets the accumulation bound of its own sum (a row's
mean can lie arbitrarily close to zero here).  LayerNorm outputs and input gradients: 2e-5 max|ref| (+ one ulp for 16-bit copies), dg / db: (rows + 16) 2^-24
sum|addends| from the reference's own addends — all as tests/test_gpu_layernorm.py.  b_b: ulp + bound + the measured allowance for the hidden 16-bit rounding
of dao (tests/tr_fused_inputs.py BB_DAO).

Cases: the full cross product of type x S x B x dp x ln_in (forward), x bcast (FFN backward), and type x S x B x dp for the attention backward with nparts
tied to B (1 part for B = 1, 4 parts part_stride = N * 128 + 52 apart for B = 3).  y2 starts non-zero where ln_in = 1, dg / db start non-zero where bcast = 1
(FFN) or B = 3 (attention), zero elsewhere.  620 tests, about 11 s on one MI355X.

Worst err / gate measured over all cases (both types): forward qkv 0.50, Pat 0.15, ao 0.50, y1 0.017, st1 0.006, x1f 0.009, x1t 0.50, hff 0.50, y2 0.0006,
xf_out 0.007, xt_out 0.49, st_out 0.007; FFN backward dg2 0.13, db2 0.11, dt_c 0.50, dt_a 0.50, part 0.007, sum of the partials 0.002; attention backward
dy_f 0.008, dg1 0.16, db1 0.10, b_d 0.50, b_b 0.32, dx 0.006.  (0.5 is the half ulp of round-to-nearest under a gate of one ulp; the fp32 gates are worst-case
bounds, which random rounding errors stay far below.)

Mutations of tr_fused.h shown to fail these tests (bf16 build, each run once): dropout index from the window-local row — forward seed_y, forward seed_o, FFN
backward seed_y (every S, dp > 0, B = 3: at B = 1 local and global rows coincide); attention mask index without the head term (every S, dp > 0); the wide
form attending to its own half's keys only (S >= 33); b2 added by every quarter, the x1 residual added by every quarter, LayerNorm epsilon 1e-6 (every forward
case); 1 / (1 - p) dropped in the FFN backward's P1 (dp > 0); dy2 added to every partial (every FFN case); nparts summing one slab (B = 3, the four-part
cases); bcast without the division (bcast = 1, S >= 15: at S = 1 the divisor is 1); dy_f left out of dx (every attention case); y1 row S written (guard
rows of the last window: every S whose last tile is not full, and the window test).  NOT caught, because it changes nothing: the attention backward's second
16-row tile put under S > 16 — the kernel's comment records wrong dk / dv at S <= 16 for that form, but every case passes with it (see the comment there)."""
import ctypes as C

import numpy as np
import pytest

import plan_ln_inputs as PI
import tr_fused_inputs as I
import tr_fused_ref as T
from plan_ln_gpu_util import check16, check32, check_tol, dev, f64, guard_intact, load, sevens

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WORST = {}          # (kernel, output) -> worst err / gate over the session


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for k in sorted(WORST):
        print(f"worst err/gate  {k[0]:9s} {k[1]:8s} {WORST[k]:.3g}")


def note(kernel, out, w):
    WORST[(kernel, out)] = max(WORST.get((kernel, out), 0.0), w)


TINY = {"bf16": 2.0 ** -133, "fp16": 2.0 ** -24}          # spacing of the type's subnormal numbers: one ulp is never less


def ulp16(ref, dtype):
    """one unit in the last place of the storage type at |ref|"""
    return np.maximum(PI.ULP[dtype] * np.abs(ref), TINY[dtype])


def tol16(ref, bnd, dtype):
    return ulp16(ref, dtype) + bnd


def stats_check(st, ref, x, what):
    """mean: LN_STAT relative + the accumulation bound of the 128-term sum; rstd: LN_STAT relative"""
    w0 = check_tol(np.abs(st[:, 0] - ref[:, 0]), PI.LN_STAT * np.abs(ref[:, 0]) + T.acc_bound(np.abs(x).mean(-1), T.D), st[:, 0], ref[:, 0], what + " mean")
    w1 = check_tol(np.abs(st[:, 1] - ref[:, 1]), PI.LN_STAT * ref[:, 1], st[:, 1], ref[:, 1], what + " rstd")
    return max(w0, w1)


def param_grads_check(kernel, d, names, ag, ab, rows, start, what):
    for name, add, s0 in ((names[0], ag, start[0]), (names[1], ab, start[1])):
        ref = s0 + add.sum(0)
        gate = (rows + 16) * PI.EPS32 * (np.abs(s0) + np.abs(add).sum(0))
        note(kernel, name, check_tol(np.abs(d[name] - ref), gate, d[name], ref, f"{what} {name}"))


def collect(bufs, sizes):
    out = {}
    for k, t in bufs.items():
        guard_intact(t, sizes[k], k)
        out[k] = f64(t[:sizes[k]])
    return out


# ==================================================================================================== forward
W_FWD, F_FWD = ("Wqkv", "Wo", "W1", "W2"), ("bqkv", "bo", "b1", "b2", "n1g", "n1b", "ln_g", "ln_b")


def fwd_run(L, lib, dtype, B, S, ln_in, p, y2_nonzero, other=()):
    """one launch -> dict of every output as float64 (guards checked), plus the inputs x, y2_0"""
    P, N = I.params(dtype), B * S
    x, y20 = I.xin(B, S, ln_in, other), I.y2_start(B, S, y2_nonzero, other)
    par = {k: dev(P[k], dtype) for k in W_FWD}
    par.update({k: dev(P[k]) for k in F_FWD})
    x_t = dev(x)
    sizes = dict(qkv=N, Pat=B * T.NH * S * S, ao=N, y1=N, st1=N, x1t=N, x1f=N, hff=N, y2=N)
    bufs = dict(qkv=sevens((N, 3 * T.D), dtype), Pat=sevens(B * T.NH * S * S), ao=sevens((N, T.D), dtype), y1=sevens((N, T.D)), st1=sevens((N, 2)),
                x1t=sevens((N, T.D), dtype), x1f=sevens((N, T.D)), hff=sevens((N, T.FF), dtype), y2=sevens((N, T.D)))
    bufs["y2"][:N] = dev(y20)
    if ln_in:
        bufs.update(xf_out=sevens((N, T.D)), xt_out=sevens((N, T.D), dtype), st_out=sevens((N, 2)))
        sizes.update(xf_out=N, xt_out=N, st_out=N)
    job = L.HulcTrLayerJob(xin=x_t.data_ptr(), seed_att=I.SEEDS["att"], seed_o=I.SEEDS["o"], seed_h=I.SEEDS["h"], seed_y=I.SEEDS["y"],
                           **{k: t.data_ptr() for k, t in par.items()}, **{k: t.data_ptr() for k, t in bufs.items()})
    L.check(lib.hulc_k_tr_layer_fwd(L.DTYPE[dtype], C.byref(job), B, S, ln_in, p, None))
    torch.cuda.synchronize()
    d = collect(bufs, sizes)
    d["Pat"] = d["Pat"].reshape(B, T.NH, S, S)
    d["x"], d["y2_0"] = x, y20
    return d


def fwd_check(d, dtype, B, S, ln_in, p, what):
    P, mk = I.params(dtype), I.masks(B, S, p) or {}
    x = d["x"]
    if ln_in:
        ref, st = T.ln(x, P["ln_g"], P["ln_b"])
        note("fwd", "st_out", stats_check(d["st_out"], st, x, what + " st_out"))
        note("fwd", "xf_out", check32(d["xf_out"], ref, what + " xf_out"))
        note("fwd", "xt_out", check16(d["xt_out"], ref, dtype, what + " xt_out"))
        x16, xf = d["xt_out"], d["xf_out"]
    else:
        x16, xf = PI.round_t(x, dtype), x
    ref, bnd = T.qkv(x16, P["Wqkv"], P["bqkv"])
    note("fwd", "qkv", check_tol(np.abs(d["qkv"] - ref), tol16(ref, bnd, dtype), d["qkv"], ref, what + " qkv"))
    ref = T.pat(d["qkv"], B, S)
    note("fwd", "Pat", check_tol(np.abs(d["Pat"] - ref), 2e-6, d["Pat"], ref, what + " Pat"))
    ref, bnd = T.ao(d["Pat"], d["qkv"], B, S, mk.get("att"), p)
    note("fwd", "ao", check_tol(np.abs(d["ao"] - ref), tol16(ref, bnd, dtype), d["ao"], ref, what + " ao"))
    ref, bnd = T.y1(xf, d["ao"], P["Wo"], P["bo"], mk.get("o"), p)
    note("fwd", "y1", check_tol(np.abs(d["y1"] - ref), bnd, d["y1"], ref, what + " y1"))
    ref, st = T.ln(d["y1"], P["n1g"], P["n1b"])
    note("fwd", "st1", stats_check(d["st1"], st, d["y1"], what + " st1"))
    note("fwd", "x1f", check32(d["x1f"], ref, what + " x1f"))
    note("fwd", "x1t", check16(d["x1t"], ref, dtype, what + " x1t"))
    ref, bnd = T.hff(d["x1t"], P["W1"], P["b1"], mk.get("h"), p)
    note("fwd", "hff", check_tol(np.abs(d["hff"] - ref), tol16(ref, bnd, dtype), d["hff"], ref, what + " hff"))
    if p > 0:
        assert (d["hff"][~mk["h"]] == 0).all(), "dropped hidden units are exactly zero"
    ref, bnd = T.y2(d["y2_0"], d["x1f"], d["hff"], P["W2"], P["b2"], mk.get("y"), p)
    note("fwd", "y2", check_tol(np.abs(d["y2"] - ref), bnd, d["y2"], ref, what + " y2"))


def same_bits(a, b, names, what):
    for k in names:
        if k in a:
            assert np.array_equal(a[k], b[k]), f"{what}: {k} differs between two identical launches"


FWD_EXACT = ("xf_out", "xt_out", "st_out", "qkv", "Pat", "ao", "y1", "st1", "x1t", "x1f", "hff")


@pytest.mark.parametrize("dtype", I.DTYPES16)
@pytest.mark.parametrize("ln_in", [0, 1])
@pytest.mark.parametrize("p", I.DPS)
@pytest.mark.parametrize("B", I.BS)
@pytest.mark.parametrize("S", I.S_FWD)
def test_layer_forward_matches_fp64(S, B, p, ln_in, dtype):
    L, lib = load()
    what = f"tr_fwd [{dtype}] B={B} S={S} dp={p} ln_in={ln_in}"
    a = fwd_run(L, lib, dtype, B, S, ln_in, p, y2_nonzero=bool(ln_in))
    fwd_check(a, dtype, B, S, ln_in, p, what)
    b = fwd_run(L, lib, dtype, B, S, ln_in, p, y2_nonzero=bool(ln_in))
    same_bits(a, b, FWD_EXACT, what)
    fwd_check(b, dtype, B, S, ln_in, p, what + " (second launch)")


@pytest.mark.parametrize("dtype", I.DTYPES16)
def test_layer_forward_more_workgroups_than_compute_units(dtype):
    """B = 70, S = 5: 280 workgroups"""
    L, lib = load()
    fwd_check(fwd_run(L, lib, dtype, 70, 5, 1, 0.1, True), dtype, 70, 5, 1, 0.1, f"tr_fwd [{dtype}] B=70 S=5")


# ==================================================================================================== FFN backward
def ffn_run(L, lib, dtype, B, S, p, bcast, start_nonzero, other=()):
    P, N = I.params(dtype), B * S
    c = I.host_forward(dtype, B, S, 0, p, other)
    dx = I.ffn_bwd_dx(B, S, bcast, other)
    dg0, db0 = I.param_grad_start("dg2", start_nonzero), I.param_grad_start("db2", start_nonzero)
    ins = dict(dx=dev(dx), y2=dev(c["y2"]), st2=dev(c["st2"]), n2g=dev(P["n2g"]), W2t=dev(P["W2"].T, dtype), W1t=dev(P["W1"].T, dtype), hff=dev(c["hff"], dtype))
    bufs = dict(dg2=sevens(T.D), db2=sevens(T.D), dt_c=sevens((N, T.D), dtype), dt_a=sevens((N, T.FF), dtype), part=sevens(T.NQ * N * T.D))
    bufs["dg2"][:T.D], bufs["db2"][:T.D] = dev(dg0), dev(db0)
    job = L.HulcTrFfnBwdJob(seed_y=I.SEEDS["y"], **{k: t.data_ptr() for k, t in ins.items()}, **{k: t.data_ptr() for k, t in bufs.items()})
    L.check(lib.hulc_k_tr_ffn_bwd(L.DTYPE[dtype], C.byref(job), B, S, bcast, float(S), p, None))
    torch.cuda.synchronize()
    d = collect(bufs, dict(dg2=T.D, db2=T.D, dt_c=N, dt_a=N, part=T.NQ * N * T.D))
    d["part"] = d["part"].reshape(T.NQ, N, T.D)
    d.update(dx=dx, dg0=dg0, db0=db0, c=c)
    return d


def ffn_check(d, dtype, B, S, p, bcast, what):
    P, mk, c = I.params(dtype), I.masks(B, S, p) or {}, d["c"]
    dx = T.bcast_rows(d["dx"], S, float(S)) if bcast else d["dx"]
    dy2, ag, ab = T.ln_bwd(dx, c["y2"], c["st2"], P["n2g"])
    param_grads_check("ffn_bwd", d, ("dg2", "db2"), ag, ab, B * S, (d["dg0"], d["db0"]), what)
    ref = T.drop(dy2, mk.get("y"), p)
    note("ffn_bwd", "dt_c", check16(d["dt_c"], ref, dtype, what + " dt_c"))
    if p > 0:
        assert (d["dt_c"][~mk["y"]] == 0).all(), "dropped elements are exactly zero"
    ref, bnd = T.dt_a(d["dt_c"], P["W2"].T, c["hff"], p)
    note("ffn_bwd", "dt_a", check_tol(np.abs(d["dt_a"] - ref), tol16(ref, bnd, dtype), d["dt_a"], ref, what + " dt_a"))
    ref, bnd = T.parts(d["dt_a"], P["W1"].T, dy2)
    bnd[0] = bnd[0] + PI.ACC * np.abs(dy2).max()          # dy2 itself: the LayerNorm backward in fp32, gated as tests/test_gpu_layernorm.py gates dx_f32
    for q in range(T.NQ):
        note("ffn_bwd", "part", check_tol(np.abs(d["part"][q] - ref[q]), bnd[q], d["part"][q], ref[q], f"{what} part[{q}]"))
    note("ffn_bwd", "sum part", check_tol(np.abs(d["part"].sum(0) - ref.sum(0)), bnd.sum(0), d["part"].sum(0), ref.sum(0), what + " sum of the partials"))


FFN_EXACT = ("dt_c", "dt_a", "part")


@pytest.mark.parametrize("dtype", I.DTYPES16)
@pytest.mark.parametrize("bcast", [0, 1])
@pytest.mark.parametrize("p", I.DPS)
@pytest.mark.parametrize("B", I.BS)
@pytest.mark.parametrize("S", I.S_FWD)
def test_ffn_backward_matches_fp64(S, B, p, bcast, dtype):
    L, lib = load()
    what = f"tr_ffn_bwd [{dtype}] B={B} S={S} dp={p} bcast={bcast}"
    a = ffn_run(L, lib, dtype, B, S, p, bcast, start_nonzero=bool(bcast))
    ffn_check(a, dtype, B, S, p, bcast, what)
    b = ffn_run(L, lib, dtype, B, S, p, bcast, start_nonzero=bool(bcast))
    same_bits(a, b, FFN_EXACT, what)
    ffn_check(b, dtype, B, S, p, bcast, what + " (second launch)")


# ==================================================================================================== attention backward
PART_GAP = 52          # floats between two of the incoming partial arrays (a multiple of 4: the arrays stay 16-byte aligned, as the engine's are)


def attn_run(L, lib, dtype, B, S, p, start_nonzero, other=()):
    P, N = I.params(dtype), B * S
    c = I.host_forward(dtype, B, S, 0, p, other)
    parts = I.attn_bwd_parts(B, S, other)
    nparts, stride = parts.shape[0], N * T.D + PART_GAP
    pbuf = torch.full((nparts * stride,), float("nan"), device="cuda", dtype=torch.float32)
    for k in range(nparts):
        pbuf[k * stride:k * stride + N * T.D] = dev(parts[k]).reshape(-1)
    dg0, db0 = I.param_grad_start("dg1", start_nonzero), I.param_grad_start("db1", start_nonzero)
    ins = dict(parts=pbuf, y1=dev(c["y1"]), st1=dev(c["st1"]), n1g=dev(P["n1g"]), Wot=dev(P["Wo"].T, dtype), Wint=dev(P["Wqkv"].T, dtype), qkv=dev(c["qkv"], dtype),
               Pat=dev(c["Pat"]))
    bufs = dict(dg1=sevens(T.D), db1=sevens(T.D), b_d=sevens((N, T.D), dtype), b_b=sevens((N, 3 * T.D), dtype), dy_f=sevens((N, T.D)), dx=sevens((N, T.D)))
    bufs["dg1"][:T.D], bufs["db1"][:T.D] = dev(dg0), dev(db0)
    job = L.HulcTrAttnBwdJob(seed_o=I.SEEDS["o"], seed_att=I.SEEDS["att"], **{k: t.data_ptr() for k, t in ins.items()}, **{k: t.data_ptr() for k, t in bufs.items()})
    L.check(lib.hulc_k_tr_attn_bwd(L.DTYPE[dtype], C.byref(job), B, S, nparts, stride, p, None))
    torch.cuda.synchronize()
    d = collect(bufs, dict(dg1=T.D, db1=T.D, b_d=N, b_b=N, dy_f=N, dx=N))
    d.update(parts=parts, dg0=dg0, db0=db0, c=c)
    return d


def attn_check(d, dtype, B, S, p, what):
    P, mk, c = I.params(dtype), I.masks(B, S, p) or {}, d["c"]
    r16 = lambda t: PI.round_t(t, dtype)
    dy_f, ag, ab = T.ln_bwd(d["parts"].sum(0), c["y1"], c["st1"], P["n1g"])
    note("attn_bwd", "dy_f", check32(d["dy_f"], dy_f, what + " dy_f"))
    param_grads_check("attn_bwd", d, ("dg1", "db1"), ag, ab, B * S, (d["dg0"], d["db0"]), what)
    # b_d is the 16-bit copy of the device's own dy_f under the mask: one ulp (the division by 1 - p is one more fp32 rounding)
    ref = T.drop(d["dy_f"], mk.get("o"), p)
    note("attn_bwd", "b_d", check_tol(np.abs(d["b_d"] - ref), ulp16(ref, dtype) + 4 * PI.EPS32 * np.abs(ref), d["b_d"], ref, what + " b_d"))
    ref, bnd = T.b_b(d["b_d"], P["Wo"].T, c["qkv"], c["Pat"], B, S, mk.get("att"), p, r16)
    tol = tol16(ref, bnd, dtype) + I.bb_allowance(dtype, B, S, p)
    note("attn_bwd", "b_b", check_tol(np.abs(d["b_b"] - ref), tol, d["b_b"], ref, what + " b_b"))
    ref, bnd = T.dx_attn(d["b_b"], P["Wqkv"].T, d["dy_f"])
    note("attn_bwd", "dx", check_tol(np.abs(d["dx"] - ref), bnd, d["dx"], ref, what + " dx"))


ATTN_EXACT = ("b_d", "b_b", "dy_f", "dx")


@pytest.mark.parametrize("dtype", I.DTYPES16)
@pytest.mark.parametrize("p", I.DPS)
@pytest.mark.parametrize("B", I.BS)
@pytest.mark.parametrize("S", I.S_ATTN)
def test_attention_backward_matches_fp64(S, B, p, dtype):
    L, lib = load()
    what = f"tr_attn_bwd [{dtype}] B={B} S={S} dp={p} nparts={I.attn_nparts(B)}"
    a = attn_run(L, lib, dtype, B, S, p, start_nonzero=B == 3)
    attn_check(a, dtype, B, S, p, what)
    b = attn_run(L, lib, dtype, B, S, p, start_nonzero=B == 3)
    same_bits(a, b, ATTN_EXACT, what)
    attn_check(b, dtype, B, S, p, what + " (second launch)")


# ==================================================================================================== windows do not see each other
@pytest.mark.parametrize("dtype", I.DTYPES16)
@pytest.mark.parametrize("S", [17, 33, 64])
def test_window_one_is_unchanged_by_other_data_in_windows_zero_and_two(S, dtype):
    """B = 3: the outputs of window 1 are bit-identical when windows 0 and 2 carry other data (y2: within twice its gate, its four atomic adds commute only in
    exact arithmetic); the attention backward at S <= 32 only"""
    L, lib = load()
    B, p = 3, 0.1
    w = slice(S, 2 * S)
    a, b = (fwd_run(L, lib, dtype, B, S, 1, p, True, other=o) for o in ((), (0, 2)))
    assert not np.array_equal(a["qkv"][:S], b["qkv"][:S]) and not np.array_equal(a["qkv"][2 * S:], b["qkv"][2 * S:]), "windows 0 and 2 did get other data"
    for k in FWD_EXACT:
        x, y = (t[k][1] if k == "Pat" else t[k][w] for t in (a, b))
        assert np.array_equal(x, y), f"forward {k} of window 1 changed"
    P, mk = I.params(dtype), I.masks(B, S, p)
    bnd = T.y2(a["y2_0"], a["x1f"], a["hff"], P["W2"], P["b2"], mk["y"], p)[1]
    assert (np.abs(a["y2"][w] - b["y2"][w]) <= 2 * bnd[w]).all(), "forward y2 of window 1 changed"
    a, b = (ffn_run(L, lib, dtype, B, S, p, 0, False, other=o) for o in ((), (0, 2)))
    assert not np.array_equal(a["dt_c"][:S], b["dt_c"][:S])
    for k in FFN_EXACT:
        x, y = (t[k][:, w] if k == "part" else t[k][w] for t in (a, b))
        assert np.array_equal(x, y), f"FFN backward {k} of window 1 changed"
    if S <= 32:
        a, b = (attn_run(L, lib, dtype, B, S, p, False, other=o) for o in ((), (0, 2)))
        assert not np.array_equal(a["dx"][:S], b["dx"][:S])
        for k in ATTN_EXACT:
            assert np.array_equal(a[k][w], b[k][w]), f"attention backward {k} of window 1 changed"
