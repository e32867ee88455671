"""GPU (-m gpu): the latent-plan kernels of csrc/kernels.h alone, through their C-ABI test entries, element by element against float64
(tests/plan_ln_ref.py) on the same storage-rounded operands: plan_scatter_grad_lds / _w4, plan_gather_t, plan_kl_sample, st_softmax_bwd, normal_kl_sample,
normal_rsample_bwd.  Every output buffer starts at 7.0 and has guard elements past its end that must still hold 7.0 afterwards.

Gates.  Scatter: a sum of at most B + 1 fp32 addends, |err| <= (B + 1) 2^-24 sum|addends| per element, from the reference's own addends; |dC| >= 0.5 is
at least 100 x the largest gate, so a lost or doubled window misses it by orders of magnitude.  Gather `out`: (NCAT + 2) 2^-24 sum|addends|; `cb`: one ulp of
the storage type + 2e-5 max|ref|; `embg`: bit-exact.  KL / Normal KL outputs: 5 x the float32-vs-float64 error of the same formulas on each case's own inputs
(tests/plan_ln_inputs.py KL_F32 / NK_F32 / NKB_F32, re-measured by tests/test_plan_ln_ref_host.py), in the measure rel_err = |err| / (|ref| + 1e-3 max|ref|).
Straight-through `out`: 2e-5 max|ref|; the 16-bit copies are the correctly rounded device values, bit for bit."""
import numpy as np
import pytest

import plan_ln_inputs as I
import plan_ln_ref as R
from plan_ln_gpu_util import GUARD, check16, check32, check_rel, check_tol, dev, devi, f64, guard_intact, load, ptr, refused, sevens

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

POISON = 12345.0          # what a `store` launch must overwrite


# ==================================================================================================== plan scatter
SC_B = (1, 15, 16, 17, 63, 64, 65, 79, 129)
SC_SHAPES = [(32, 32, 256), (32, 32, 320), (5, 7, 256), (5, 7, 320)]          # (NCAT, NCLS, H); H = 320: the i0 + t < H guard of the last 64-wide tile
SC_KPAD = 5          # KIN = NCAT * NCLS + SC_KPAD: columns past the plan block, guarded


def scatter_run(lib, L, dtype, form, dC_t, idx_t, B, ncat, ncls, H, dw0, store):
    """-> the plan block (H, NCAT * NCLS) as float64; everything outside it must still hold 7.0"""
    P, KIN = ncat * ncls, ncat * ncls + SC_KPAD
    dw = sevens((H, KIN))
    dw[:H, :P] = POISON if store else dev(dw0)
    L.check(lib.hulc_k_plan_scatter_grad(L.DTYPE[dtype], form, dC_t.data_ptr(), idx_t.data_ptr(), B, ncat, ncls, H, KIN, dw.data_ptr(), store, None))
    torch.cuda.synchronize()
    guard_intact(dw, H, "dw rows")
    assert (dw[:H, P:] == 7.0).all(), "dw: columns past the plan block were written"
    return f64(dw[:H, :P])


def scatter_cases(B):
    for (ncat, ncls, H) in SC_SHAPES + ([(32, 32, 2048)] if B == 65 else []):          # + the engine's own size, once per kernel
        for pattern in ((0,) if H == 2048 else (0, 1, 2)):
            yield ncat, ncls, H, pattern


@pytest.mark.parametrize("B", SC_B)
@pytest.mark.parametrize("dtype,form", [("bf16", 0), ("fp16", 0), ("fp32", 0), ("bf16", 1), ("fp16", 1)])
def test_plan_scatter_matches_fp64(dtype, form, B):
    """dw0 + one_hot.T @ dC; form 1 also with store = 1 (the sum alone over a poisoned buffer) and against form 0 on the same inputs"""
    L, lib = load()
    worst = 0.0
    for ncat, ncls, H, pattern in scatter_cases(B):
        dC = I.scatter_inputs(B, H, dtype)
        idx = I.plan_indices(B, ncat, ncls, pattern)
        dw0 = I.prng.uniform(f"dw0_{ncat}_{H}", (H, ncat * ncls), -1.0, 1.0, seed=43).astype(np.float64)
        s, gate = I.scatter_reference(dC, idx, ncls, dw0)
        assert I.SC_DC_MIN >= 100 * gate.max(), "a single window must stand far above the gate"
        dC_t, idx_t = dev(dC, dtype), devi(idx)
        what = f"scatter form {form} B={B} NCAT={ncat} NCLS={ncls} H={H} idx {pattern}"
        got = scatter_run(lib, L, dtype, form, dC_t, idx_t, B, ncat, ncls, H, dw0, 0)
        worst = max(worst, check_tol(np.abs(got - (dw0 + s)), gate, got, dw0 + s, what))
        if form == 1:
            s1, gate1 = I.scatter_reference(dC, idx, ncls, None)
            got1 = scatter_run(lib, L, dtype, 1, dC_t, idx_t, B, ncat, ncls, H, None, 1)
            worst = max(worst, check_tol(np.abs(got1 - s1), gate1, got1, s1, what + " store"))
            got0 = scatter_run(lib, L, dtype, 0, dC_t, idx_t, B, ncat, ncls, H, dw0, 0)
            check_tol(np.abs(got - got0), gate, got, got0, what + " against form 0")
    print(f"scatter [{dtype} form {form} B={B}]: worst err/tol {worst:.3g}")


# ==================================================================================================== plan gather
GA_VARIANTS = [(0, None), (32, (1, 64)), (8, (7, 16)), (32, None), (0, (7, 16))]          # (G of the goal term cb or 0, (S, W) of the embg copy or None)
GA_PAD = 3          # rows between the plan rows and the goal rows of w_t (the engine has its DE embedding rows there)


def gather_once(lib, L, dtype, B, ncat, ncls, H, G, sw, tag):
    P = ncat * ncls
    grow0 = P + GA_PAD
    w = I.gather_weight(P + GA_PAD + 32, H, dtype)
    idx = I.plan_indices(B, max(ncat, 1), ncls, 0, tag)[:, :ncat]
    b1 = I.prng.normal(f"gb1{H}", (H,), seed=44).astype(np.float32)
    b2 = I.prng.normal(f"gb2{H}", (H,), seed=45).astype(np.float32)
    w_t, idx_t, b1_t, b2_t = dev(w, dtype), (devi(idx) if ncat else None), dev(b1), dev(b2)
    assert (f64(w_t) == w).all()
    out = sevens((B, H))
    goal = goal_t = cb = emb_t = embg = None
    S = W = 0
    if G:
        goal = I.round_t(I.prng.normal(f"gg{B}_{G}", (B, G), seed=46), dtype)
        goal_t, cb = dev(goal, dtype), sevens((B, H), dtype)
    if sw:
        S, W = sw
        emb_t = dev(I.prng.normal(f"ge{B}_{S}", (B * S, 128), seed=47), dtype)
        embg = sevens(S * B * W, dtype)
    L.check(lib.hulc_k_plan_gather(L.DTYPE[dtype], w_t.data_ptr(), ptr(idx_t), B, ncat, ncls, H, b1_t.data_ptr(), b2_t.data_ptr(), out.data_ptr(), ptr(emb_t), ptr(embg),
                                   S, W, ptr(goal_t), G, grow0, ptr(cb), None))
    torch.cuda.synchronize()
    what = f"gather [{dtype}] B={B} NCAT={ncat} H={H} G={G} embg={sw}"
    guard_intact(out, B, "out")
    b1d, b2d = b1.astype(np.float64), b2.astype(np.float64)
    ref = R.plan_gather(w, idx.reshape(B, ncat), ncls, b1d, b2d)
    mag = R.plan_gather(np.abs(w), idx.reshape(B, ncat), ncls, np.abs(b1d), np.abs(b2d))
    got = f64(out[:B])
    worst = check_tol(np.abs(got - ref), (ncat + 2) * I.EPS32 * mag, got, ref, what + " out")
    if G:
        guard_intact(cb, B, "cb")
        check16(f64(cb[:B]), ref + goal @ w[grow0:grow0 + G], dtype, what + " cb")
    if sw:
        guard_intact(embg, S * B * W, "embg")
        want = emb_t.view(B, S, 128)[:, :, 128 - W:].permute(1, 0, 2).contiguous().view(-1)          # embg[(t * B + b) * W + c] = emb[(b * S + t) * 128 + 128 - W + c]
        bits = torch.int32 if dtype == "fp32" else torch.int16
        assert torch.equal(embg[:S * B * W].view(bits), want.view(bits)), what + ": embg is not a bit-exact copy"
    return worst


@pytest.mark.parametrize("ncat", [0, 5, 32])
@pytest.mark.parametrize("B", [1, 3, 64, 130])
@pytest.mark.parametrize("dtype", I.DTYPES)
def test_plan_gather_matches_fp64(dtype, B, ncat):
    L, lib = load()
    ncls = 7 if ncat == 5 else 32
    worst = max(gather_once(lib, L, dtype, B, ncat, ncls, 256, G, sw, "") for (G, sw) in GA_VARIANTS)
    if B == 3 and ncat == 32:          # the engine's own size
        worst = max(worst, gather_once(lib, L, dtype, B, 32, 32, 2048, 32, (7, 64), "e"))
    print(f"gather [{dtype} B={B} NCAT={ncat}]: worst err/tol of out {worst:.3g}")


# ==================================================================================================== plan KL + sample
def kl_run(lib, L, case, pp, lscale, idx_in, seed):
    B, ncat, ncls = case
    pr, ppl = I.kl_inputs(*case)
    rows = B * ncat
    o = dict(idx=torch.full((rows + GUARD,), 7, device="cuda", dtype=torch.int32), probs=sevens((rows, ncls)), kl_cat=sevens(rows), dpp=sevens((rows, ncls)), dpr=sevens((rows, ncls)))
    pr_t, pp_t = dev(pr), (dev(ppl) if pp else None)
    idx_t = devi(idx_in) if idx_in is not None else None
    ls_t = dev(np.array([lscale])) if lscale else None
    L.check(lib.hulc_k_plan_kl_sample(pr_t.data_ptr(), ptr(pp_t), B, ncat, ncls, ptr(idx_t), o["idx"].data_ptr(), o["probs"].data_ptr(), o["kl_cat"].data_ptr(), o["dpp"].data_ptr(),
                                      o["dpr"].data_ptr(), I.KL_W[0], I.KL_W[1], seed, ptr(ls_t), None))
    torch.cuda.synchronize()
    for k, t in o.items():
        guard_intact(t, rows, k)
    return o


@pytest.mark.parametrize("lscale", [0.0, 256.0])
@pytest.mark.parametrize("pp", [True, False])
@pytest.mark.parametrize("case", I.KL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_plan_kl_matches_fp64(case, pp, lscale):
    L, lib = load()
    B, ncat, ncls = case
    rows = B * ncat
    idx_in = I.plan_indices(B, ncat, ncls, 0, "kl")
    o = kl_run(lib, L, case, pp, lscale, idx_in, 1)
    assert (o["idx"][:rows].cpu().numpy() == idx_in.reshape(-1)).all(), "an injected sample must come back bit for bit"
    pr, ppl = (a.astype(np.float64) for a in I.kl_inputs(*case))
    p, klc, dpp, dpr = R.plan_kl(pr, ppl, *I.KL_W)
    gate = I.KL_GATE[case]
    what = f"plan_kl {case} pp={pp} lscale={lscale}"
    check_rel(f64(o["probs"][:rows]).reshape(p.shape), p, gate[0], what + " probs")
    if pp:
        s = lscale or 1.0          # the loss scale multiplies the gradients only
        check_rel(f64(o["kl_cat"][:rows]).reshape(klc.shape), klc, gate[1], what + " kl_cat")
        check_rel(f64(o["dpp"][:rows]).reshape(p.shape), s * dpp, gate[2], what + " dpp")
        check_rel(f64(o["dpr"][:rows]).reshape(p.shape), s * dpr, gate[3], what + " dpr")
    else:
        assert all((o[k] == 7.0).all() for k in ("kl_cat", "dpp", "dpr")), "without pp_logits the KL outputs are not written"


@pytest.mark.parametrize("seed", I.KL_SEEDS)
@pytest.mark.parametrize("case", I.KL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_plan_sample_is_the_gumbel_max_of_the_counter_based_uniforms(case, seed):
    L, lib = load()
    B, ncat, ncls = case
    rows = B * ncat
    a = kl_run(lib, L, case, True, 0.0, None, seed)["idx"][:rows].cpu().numpy()
    b = kl_run(lib, L, case, False, 0.0, None, seed)["idx"][:rows].cpu().numpy()
    assert (a == b).all(), "the same seed must give the same draw"
    assert ((a >= 0) & (a < ncls)).all()
    want, decided = I.gumbel_draw(I.kl_inputs(*case)[0], seed)
    want, decided = want.reshape(-1), decided.reshape(-1)
    assert (~decided).mean() <= 0.01
    assert (a[decided] == want[decided]).all(), f"{int((a[decided] != want[decided]).sum())} decided rows differ from the float64 draw"
    assert a[0] == I.KL_SPIKE % ncls, "the spike row selects the spike"


# ==================================================================================================== straight-through backward
@pytest.mark.parametrize("dtype", I.DTYPES)
@pytest.mark.parametrize("rows,ncls", I.ST_CASES)
def test_st_softmax_bwd_matches_fp64(rows, ncls, dtype):
    """out at 2e-5 max|ref|; out_t and dpp_t bit for bit the device's fp32 out / dpp_kl rounded to the storage type (kernels.h as_stored_f32 keeps the
    conversion apart from the multiply-add: fp32 values half way between two fp16 values are where the two roundings part)."""
    L, lib = load()
    probs, dplan, dpr, dpp = I.st_inputs(rows, ncls)
    out, out_t, dpp_t = sevens((rows, ncls)), sevens((rows, ncls), dtype), sevens((rows, ncls), dtype)
    probs_d, dplan_d, dpr_d, dpp_d = dev(probs), dev(dplan), dev(dpr), dev(dpp)          # named: a temporary's memory is reused by the next allocation
    L.check(lib.hulc_k_st_softmax_bwd(L.DTYPE[dtype], probs_d.data_ptr(), dplan_d.data_ptr(), dpr_d.data_ptr(), dpp_d.data_ptr(), rows, ncls, out.data_ptr(),
                                      out_t.data_ptr(), dpp_t.data_ptr(), None))
    torch.cuda.synchronize()
    for t, k in ((out, "out"), (out_t, "out_t"), (dpp_t, "dpp_t")):
        guard_intact(t, rows, k)
    ref = R.st_softmax_bwd(probs.astype(np.float64), dplan.astype(np.float64), dpr.astype(np.float64))
    check32(f64(out[:rows]), ref, f"st_softmax_bwd {rows}x{ncls} out")
    bits = torch.int32 if dtype == "fp32" else torch.int16
    assert torch.equal(out_t[:rows].view(bits), out[:rows].to(I.tdt(dtype)).view(bits)), "out_t must be the correctly rounded device out"
    assert torch.equal(dpp_t[:rows].view(bits), dpp_d.to(I.tdt(dtype)).view(bits)), "dpp_t must be the correctly rounded dpp_kl"
    assert not torch.equal(dpp_t[:rows].float(), dpr_d.to(I.tdt(dtype)).float())


# ==================================================================================================== continuous plan (mcil)
def nk_run(lib, L, dtype, B, n, pp, inject, seed=0, lscale=0.0):
    pr, ppl, eps = I.nk_inputs(B, n)
    o = dict(eps=sevens(B * n), plan_f=sevens(B * n), plan_t=sevens(B * n, dtype), kl=sevens(B * n), dpp=sevens((B, 2 * n)), dpr=sevens((B, 2 * n)))
    pr_t, pp_t, eps_t = dev(pr), (dev(ppl) if pp else None), (dev(eps) if inject else None)
    ls_t = dev(np.array([lscale])) if lscale else None
    L.check(lib.hulc_k_normal_kl_sample(L.DTYPE[dtype], pr_t.data_ptr(), ptr(pp_t), B, n, ptr(eps_t), o["eps"].data_ptr(), o["plan_f"].data_ptr(), o["plan_t"].data_ptr(),
                                        o["kl"].data_ptr(), o["dpp"].data_ptr(), o["dpr"].data_ptr(), I.NK_W[0], I.NK_W[1], seed, ptr(ls_t), None))
    torch.cuda.synchronize()
    for k, t in o.items():
        guard_intact(t, B if k in ("dpp", "dpr") else B * n, k)
    return o


@pytest.mark.parametrize("pp", [True, False])
@pytest.mark.parametrize("dtype", I.DTYPES)
@pytest.mark.parametrize("B,n", I.NK_CASES)
def test_normal_kl_sample_matches_fp64(B, n, dtype, pp):
    L, lib = load()
    lscale = 64.0 if (pp and dtype == "fp16") else 0.0
    o = nk_run(lib, L, dtype, B, n, pp, True, lscale=lscale)
    pr, ppl, eps = I.nk_inputs(B, n)
    plan, kl, dpp, dpr = I.nk_reference(B, n)
    gate = I.NK_GATE[B, n]
    what = f"normal_kl [{dtype}] B={B} n={n}"
    assert (o["eps"][:B * n].cpu().numpy() == eps.reshape(-1)).all(), "an injected eps must come back bit for bit"
    check_rel(f64(o["plan_f"][:B * n]), plan.reshape(-1), gate[0], what + " plan_f")
    bits = torch.int32 if dtype == "fp32" else torch.int16
    assert torch.equal(o["plan_t"][:B * n].view(bits), o["plan_f"][:B * n].to(I.tdt(dtype)).view(bits)), "plan_t must be the correctly rounded plan_f"
    if pp:
        s = lscale or 1.0
        check_rel(f64(o["kl"][:B * n]), kl.reshape(-1), gate[1], what + " kl_elem")
        check_rel(f64(o["dpp"][:B]), s * dpp, gate[2], what + " dpp")
        check_rel(f64(o["dpr"][:B]), s * dpr, gate[3], what + " dpr")
    else:
        assert all((o[k] == 7.0).all() for k in ("kl", "dpp", "dpr")), "without pp_state the KL outputs are not written"


@pytest.mark.parametrize("B,n", I.NK_CASES)
def test_normal_sample_without_injection(B, n):
    """the device's own draw: finite, the same for the same seed, and plan_f = mean + std * eps_out"""
    L, lib = load()
    a = nk_run(lib, L, "fp32", B, n, False, False, seed=991)
    b = nk_run(lib, L, "fp32", B, n, False, False, seed=991)
    e = a["eps"][:B * n]
    assert torch.isfinite(e).all() and torch.equal(e, b["eps"][:B * n]) and torch.equal(a["plan_f"], b["plan_f"])
    if B * n >= 64:
        assert 0.5 < float(e.std()) < 1.5 and abs(float(e.mean())) < 0.5
    pr = I.nk_inputs(B, n)[0].astype(np.float64)
    check_rel(f64(a["plan_f"][:B * n]), R.rsample(pr, f64(e).reshape(B, n)).reshape(-1), I.NK_GATE[B, n][0], f"normal sample B={B} n={n} plan_f")


@pytest.mark.parametrize("dtype", I.DTYPES)
@pytest.mark.parametrize("B,n", I.NK_CASES)
def test_normal_rsample_bwd_matches_fp64(B, n, dtype):
    """out = [dplan | dplan eps sigmoid(var)] + dpr_kl in the storage type.  fp32: rel_err within 5 x the float32-vs-float64 error of the case's own inputs
    (plan_ln_inputs.NKB_F32); 16 bit: per element one ulp of the storage type on top of that same gate."""
    L, lib = load()
    pr, _, eps = I.nk_inputs(B, n)
    dplan, dkl = I.nkb_inputs(B, n)
    out = sevens((B, 2 * n), dtype)
    dplan_d, eps_d, pr_d, dkl_d = dev(dplan), dev(eps), dev(pr), dev(dkl)
    L.check(lib.hulc_k_normal_rsample_bwd(L.DTYPE[dtype], dplan_d.data_ptr(), eps_d.data_ptr(), pr_d.data_ptr(), dkl_d.data_ptr(), B, n, out.data_ptr(), None))
    torch.cuda.synchronize()
    guard_intact(out, B, "out")
    ref, got, gate = I.nkb_reference(B, n), f64(out[:B]), I.NKB_GATE[B, n]
    what = f"normal_rsample_bwd [{dtype}] B={B} n={n}"
    if dtype == "fp32":
        check_rel(got, ref, gate, what)
    else:
        check_tol(np.abs(got - ref), I.ULP[dtype] * np.abs(ref) + gate * (np.abs(ref) + 1e-3 * np.abs(ref).max()), got, ref, what)


# ==================================================================================================== argument validation
def test_plan_entries_validate_their_arguments():
    """every refusal names its entry, and nothing is launched: the output buffers keep their 7.0"""
    L, lib = load()
    B, ncat, ncls, H = 2, 3, 4, 256
    P = ncat * ncls
    f = sevens((64, 256))          # any fp32 buffer
    h = sevens((64, 256), "bf16")
    idx = devi(np.zeros((B, ncat)))
    bad_hi, bad_lo = devi(np.full((B, ncat), ncls)), devi(np.array([[0, 0, 0], [0, -1, 0]]))
    out, outi = sevens((64, 256)), torch.full((64,), 7, device="cuda", dtype=torch.int32)
    BF, F32 = L.DTYPE["bf16"], L.DTYPE["fp32"]
    p, o, oi = f.data_ptr(), out.data_ptr(), outi.data_ptr()

    def kl(pr=p, pp=p, ncls_=ncls, idx_in=None, idx_out=oi, probs=o):
        return lib.hulc_k_plan_kl_sample(pr, pp, B, ncat, ncls_, idx_in, idx_out, probs, o, o, o, 1.0, 1.0, 0, None, None)
    for rc in (kl(pr=None), kl(idx_out=None), kl(ncls_=65), kl(ncls_=0), kl(probs=o + 2), kl(idx_in=bad_hi.data_ptr()), kl(idx_in=bad_lo.data_ptr())):
        refused(lib, rc, "hulc_k_plan_kl_sample")

    def st(dt=BF, probs=p, rows=B, ncls_=ncls, out_t=h.data_ptr()):
        return lib.hulc_k_st_softmax_bwd(dt, probs, p, p, p, rows, ncls_, o, out_t, h.data_ptr(), None)
    for rc in (st(probs=None), st(out_t=None), st(ncls_=65), st(rows=0), st(out_t=h.data_ptr() + 1), st(dt=F32, out_t=h.data_ptr() + 2), st(dt=7)):
        refused(lib, rc, "hulc_k_st_softmax_bwd")

    def ga(dt=BF, w=h.data_ptr(), idx_=idx.data_ptr(), ncat_=ncat, H_=H, emb=None, embg=None, goal=None, cb=None, grow0=P):
        return lib.hulc_k_plan_gather(dt, w, idx_, B, ncat_, ncls, H_, p, p, o, emb, embg, 1, 16, goal, 4, grow0, cb, None)
    for rc in (ga(w=None), ga(idx_=None), ga(H_=300), ga(H_=128), ga(ncat_=65), ga(idx_=bad_hi.data_ptr()), ga(idx_=bad_lo.data_ptr()), ga(emb=h.data_ptr()),
               ga(cb=h.data_ptr()), ga(goal=h.data_ptr(), cb=h.data_ptr(), grow0=P - 1), ga(w=h.data_ptr() + 1), ga(dt=9)):
        refused(lib, rc, "hulc_k_plan_gather")

    def sc(dt=BF, form=1, dC=h.data_ptr(), idx_=idx.data_ptr(), ncls_=ncls, kin=P + 4, dw=o, store=0):
        return lib.hulc_k_plan_scatter_grad(dt, form, dC, idx_, B, ncat, ncls_, H, kin, dw, store, None)
    for rc in (sc(dC=None), sc(dw=None), sc(ncls_=33), sc(form=0, store=1), sc(form=2), sc(dt=F32, form=1), sc(kin=P - 1), sc(idx_=bad_hi.data_ptr()), sc(form=0, idx_=bad_lo.data_ptr()),
               sc(dw=o + 2), sc(store=2)):
        refused(lib, rc, "hulc_k_plan_scatter_grad")

    def nk(dt=BF, pr=p, eps_out=o, B_=B, n=8):
        return lib.hulc_k_normal_kl_sample(dt, pr, p, B_, n, None, eps_out, o, h.data_ptr(), o, o, o, 1.0, 1.0, 0, None, None)
    for rc in (nk(pr=None), nk(eps_out=None), nk(B_=0), nk(n=0), nk(pr=p + 1), nk(dt=5)):
        refused(lib, rc, "hulc_k_normal_kl_sample")
    for rc in (lib.hulc_k_normal_rsample_bwd(BF, None, p, p, p, B, 8, h.data_ptr(), None), lib.hulc_k_normal_rsample_bwd(BF, p, p, p, p, B, 0, h.data_ptr(), None),
               lib.hulc_k_normal_rsample_bwd(BF, p, p, p, p, B, 8, h.data_ptr() + 1, None)):
        refused(lib, rc, "hulc_k_normal_rsample_bwd")
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (outi == 7).all() and (h == 7.0).all() and (f == 7.0).all(), "a refused call wrote to a buffer"


def test_forward_refuses_an_injected_plan_index_out_of_range():
    """hulc_forward_loss reads an injected plan sample back and refuses classes outside [0, 32) before anything is launched with them"""
    from hulc_amd import spec
    from hulc_amd.engine import StepEngine
    from hulc_amd.utils import synthetic
    load()
    dims = spec.ModelDims(kind="hulc", max_window=32, use_clip=True)
    eng = StepEngine(dims, 2, 4, dtype="fp32", dropout_p=0.0, device="cuda:0")
    eng.load_numpy(spec.init_all(dims, seed=7, ln_jitter=True))
    eng.zero_grads()
    mb = next(iter(synthetic.make_batch(2, 2, 4, seed=7).values()))
    d = {k: torch.from_numpy(v).cuda() for k, v in mb.items() if k not in ("use_for_aux", "plan_idx")}
    for bad in (32, -1):
        pidx = np.zeros((2, 32), np.int32)
        pidx[1, 17] = bad
        with pytest.raises(RuntimeError, match="injected plan index"):
            eng.forward_loss(dict(d, plan_idx=torch.from_numpy(pidx).cuda()), False, 0.5, 3.0)
