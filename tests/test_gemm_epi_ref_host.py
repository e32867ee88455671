"""Host (no GPU): pins tests/gemm_epi_ref.py — the float64 reference of the GEMM epilogue that tests/test_gpu_gemm_epilogue.py compares the kernels with — to torch
float64 compositions of the combinations the engine uses, at 1e-12; shows that its derived rounding bound holds for a float32 evaluation of the same steps;
checks that dropout is keyed by the element offset (gaps of a padded leading dimension and of the two-level row map included); and asks the engine's routing
(gemm_pick / gemm_wgrad_nsplit of csrc/gemm.h, through their device-free C entries) for every launch site of the table in tests/gemm_epi_inputs.py at the
shapes the shipped configurations produce: every pick must be a kernel and k-step the GPU file runs."""
import ctypes as C

import numpy as np
import torch

import gemm_epi_inputs as GI
import gemm_epi_ref as G
import plan_ln_inputs as PI
import tr_fused_ref as T

F = torch.nn.functional
TOL = 1e-12


def t64(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))


def close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape and np.abs(a - b).max() <= TOL * max(1.0, np.abs(b).max()), (what, float(np.abs(a - b).max()))


def operands(M, N, K, tag="h"):
    return GI.matrix(tag + "a", M, K, "fp32"), GI.matrix(tag + "b", N, K, "fp32")


def test_residual_plus_dropout_of_linear_under_an_explicit_mask():
    """engine_forward.inc:157 / :161: y = x + dropout(ao Wo^T + bo), the residual late, the mask from the hash of the element offset"""
    M, N, K, p = 21, 12, 40, 0.3
    A, B = operands(M, N, K)
    bias, x = GI.vector("h1", N), GI.matrix("hx", M, N, "fp32")
    off = G.offsets(M, N, N)
    keep = G.keep_mask(GI.SEED, p, off)
    assert 0.5 < keep.mean() < 0.9 and not keep.all()
    out, _, bound, _ = G.epilogue(A @ B.T, dict(bias=bias, res=x, res_late=1, drop_p=p), keep)
    ref = t64(x) + t64(np.where(keep, T.mult(p), 0.0)) * F.linear(t64(A), t64(B), t64(bias))
    close(out, ref.numpy(), "x + dropout(linear)")
    assert (bound > 0).all()


def test_relu_of_linear_and_the_autograd_backward_of_relu_and_tanh_as_masks():
    M, N, K = 13, 20, 24
    A, B = operands(M, N, K, "r")
    bias = GI.vector("h2", N)
    for act, relu in ((torch.relu, 1), (torch.tanh, 2)):
        z = F.linear(t64(A), t64(B), t64(bias)).requires_grad_(True)
        y = act(z)
        out, _, _, _ = G.epilogue(A @ B.T, dict(bias=bias, relu=relu))
        close(out, y.detach().numpy(), f"act {relu}")
        # backward: dz = (dy + dh) * act'(z) expressed through the saved output y, as the recurrent BPTT step does (mask = y, residual = dh, early)
        dy, dh = GI.matrix("hdy", M, N, "fp32"), GI.matrix("hdh", M, N, "fp32")
        y.backward(t64(dy + dh))
        got, _, _, _ = G.epilogue(dy, dict(res=dh, mask=y.detach().numpy(), mask_tanh=int(relu == 2)))
        close(got, z.grad.numpy(), f"backward of act {relu}")


def test_relu_mask_treats_both_zeros_as_not_positive():
    m = np.array([[0.0, -0.0, 1e-30, -1e-30]])
    out, _, _, _ = G.epilogue(np.full((1, 4), 3.0), dict(mask=m))
    assert out.tolist() == [[0.0, 0.0, 3.0, 0.0]]


def test_broadcast_residual_over_time_and_the_second_store():
    """engine_forward.inc:199: Zx0[t * B + b] = embg W^T + Cb[b], H[0] = relu(Zx0[0]) stored a second time; engine_backward.inc:210: dZ[S-1] = dH[S-1] * (H[S-1] > 0)"""
    Bw, S, N, K = 5, 4, 8, 16
    M = Bw * S
    A, B = operands(M, N, K, "z")
    cb = GI.matrix("hcb", Bw, N, "fp32")
    off = G.offsets(M, N, N)
    out, out2, _, _ = G.epilogue(A @ B.T, dict(res=cb, res_rowmod=Bw, out2_lo=0, out2_hi=Bw * N, out2_relu=1, off=off))
    ref = (t64(A) @ t64(B).T).reshape(S, Bw, N) + t64(cb)[None]
    close(out, ref.reshape(M, N).numpy(), "broadcast residual")
    close(out2.reshape(Bw, N), torch.relu(ref[0]).numpy(), "out2 = relu(first rows)")
    h = GI.mask_values("hh", Bw * N, "fp32", False)
    lo = (S - 1) * Bw * N
    out, out2, _, _ = G.epilogue(A @ B.T, dict(out2_lo=lo, out2_hi=lo + Bw * N, out2_mask=h, off=off))
    ref = t64(A) @ t64(B).T
    close(out, ref.numpy(), "plain store")
    close(out2.reshape(Bw, N), (ref[(S - 1) * Bw:] * (t64(h).reshape(Bw, N) > 0)).numpy(), "out2 = masked last step")
    # a window that starts and ends inside the matrix, through a padded leading dimension: the gaps belong to the window's index space
    ldc = N + 3
    off = G.offsets(M, N, ldc)
    lo, hi = 4 * 5, 4 * 31
    _, out2, _, _ = G.epilogue(A @ B.T, dict(out2_lo=lo, out2_hi=hi, off=off))
    flat = np.full(M * ldc, np.nan)
    flat[off.reshape(-1)] = (A @ B.T).reshape(-1)
    assert np.array_equal(np.isnan(out2), np.isnan(flat[lo:hi])) and np.nanmax(np.abs(out2 - flat[lo:hi])) == 0.0


def test_dropout_is_keyed_by_the_element_offset_gaps_included():
    M, N, p = 12, 6, 0.4
    for off in (G.offsets(M, N, N + 2), G.offsets(M, N, 40, R1=4, s0=8)):
        keep = G.keep_mask(GI.SEED, p, off)
        u = PI.hash_uniform(GI.SEED, int(off.max()) + 1)
        assert np.array_equal(keep, ~(u.astype(np.float32) < np.float32(p))[off])
        assert not np.array_equal(keep, G.keep_mask(GI.SEED, p, G.offsets(M, N, N))), "a dense index gives other decisions"
    assert G.offsets(6, 2, 40, R1=4, s0=8)[:, 0].tolist() == [0, 40, 80, 120, 8, 48]


def test_the_derived_bound_holds_for_a_float32_evaluation_of_the_same_steps():
    """every step in float32 (numpy, one rounding per operation as the scalar path has them) stays within the bound the reference returns"""
    M, N, K, p = 33, 20, 64, 0.1
    A, B = operands(M, N, K, "b")
    acc = (A @ B.T).astype(np.float32).astype(np.float64)
    bias, bias2, res = GI.vector("b1", N), GI.vector("b2", N), GI.matrix("bres", M, N, "fp32")
    mk = GI.mask_values("bm", M * N, "fp32", True).reshape(M, N)
    keep = G.keep_mask(GI.SEED, p, G.offsets(M, N, N))
    old = np.full((M, N), GI.OLD)
    f32 = np.float32
    for alpha, late, mt in ((1.0, 0, 0), (0.75, 1, 1), (1.25, 0, 1)):
        f = dict(alpha=alpha, bias=bias, bias2=bias2, res=res, res_late=late, relu=1, mask=mk, mask_tanh=mt, drop_p=p, accumulate=1, old=old)
        ref, _, bound, _ = G.epilogue(acc, f, keep)
        v = acc.astype(f32) * f32(alpha)
        v = v + bias.astype(f32)[None]
        v = v + bias2.astype(f32)[None]
        if not late:
            v = v + res.astype(f32)
        v = np.maximum(v, f32(0))
        m = mk.astype(f32)
        v = v * (f32(1) - m * m) if mt else np.where(m > 0, v, f32(0))
        v = np.where(keep, v * (f32(1) / (f32(1) - f32(p))), f32(0))
        if late:
            v = v + res.astype(f32)
        v = old.astype(f32) + v
        err = np.abs(v.astype(np.float64) - ref)
        assert (err <= bound).all(), (alpha, late, mt, float((err / np.maximum(bound, 1e-300)).max()))
        assert err.max() > 0, "the float32 evaluation does round"


def test_product_bound_counts_one_rounding_per_slab():
    A, B = operands(8, 8, 32, "p")
    r1, b1 = G.product(A, B)
    r4, b4 = G.product(A, B, nsplit=4)
    assert np.array_equal(r1, r4) and np.allclose(b4 / b1, (32 + 2 + 4) / (32 + 2))


def test_fp16_sums_of_the_largest_cases_stay_finite():
    for M, N, K in GI.KCHUNK_SHAPES + GI.SPLITK_SHAPES + ((64, 48, 2048), (500, 128, 2048)):
        A, B = GI.matrix("A", M, K, "fp16"), GI.matrix("B", N, K, "fp16")
        assert (np.abs(A) @ np.abs(B).T).max() + 4 * 2.5 + GI.OLD < 65504 / 4, (M, N, K)


# ---------------------------------------------------------------------------------------------------- routing
def lib():
    from hulc_amd import lib as L
    return L, L.load()


def pick(l, L, dtype, M, N, K, lda=None, ldb=None):
    p, bk = C.c_int32(-1), C.c_int32(-1)
    L.check(l.hulc_k_gemm_pick(L.DTYPE[dtype], M, N, K, lda or K, ldb or K, C.byref(p), C.byref(bk)))
    return p.value, bk.value


def test_every_launch_site_routes_to_a_kernel_the_gpu_file_covers():
    L, l = lib()
    cov = GI.covered_picks()
    seen = set()
    for kind, B, S in GI.SHIPPED:
        d = GI.dims(kind)
        for site, where, epi, shape in GI.SITES:
            assert epi in GI.EPI, (site, epi)
            M, N, K = shape(B, S, d)
            for dtype in GI.DTYPES:
                p = pick(l, L, dtype, M, N, K)
                assert p in cov["32" if dtype == "fp32" else "16"], (site, where, kind, B, S, dtype, (M, N, K), p)
                seen.add((dtype != "fp32", p[0]))
    # the table reaches every family the router has: nothing in the GPU file is there for a kernel no site runs
    assert {f for h, f in seen if h} >= {GI.RAN_64, GI.RAN_GLDS, GI.RAN_ROUTER}, seen
    assert {f for h, f in seen if not h} <= {GI.RAN_32, GI.RAN_64, GI.RAN_128}


def test_routing_rules_at_their_thresholds():
    """gemm_pick: skinny by skinny_ok, 128x128 from 128 workgroups, the LDS-DMA kernel from K = 64 in steps of 32 with 16-byte rows, BK 64 / 128 from K = 128, 64x64
    against 32x32 by workgroup count; gemm_wgrad_nsplit: min(256 / tiles, K / 256, 32) below 128 tiles from K = 512, 16-bit types only"""
    L, l = lib()
    R = GI
    assert pick(l, L, "bf16", 64, 2048, 2048) == (R.RAN_ROUTER, 0)
    assert pick(l, L, "bf16", 64, 2040, 2048)[0] != R.RAN_ROUTER          # N % 16
    assert pick(l, L, "fp32", 64, 2048, 2048) == (R.RAN_32, 32)           # fp32 has no skinny kernel; 1 x 32 tiles of 64 are fewer than 128 workgroups: 32x32
    assert pick(l, L, "bf16", 2048, 2048, 2048) == (R.RAN_GLDS, 0)
    assert pick(l, L, "fp16", 2048, 2048, 2048) == (R.RAN_GLDS, 0)
    assert pick(l, L, "bf16", 2048, 2048, 2048, lda=2052) == (R.RAN_128, 64)          # rows not 16-byte aligned: the register-staged kernel
    assert pick(l, L, "bf16", 2048, 2048, 2056, lda=2056, ldb=2056) == (R.RAN_128, 64)          # K % 32
    assert pick(l, L, "fp32", 2048, 2048, 2048) == (R.RAN_128, 32)
    assert pick(l, L, "bf16", 2047, 2048, 2048) == (R.RAN_GLDS, 0) and pick(l, L, "bf16", 2048, 1920, 2048)[0] == R.RAN_GLDS
    assert pick(l, L, "bf16", 2048, 900, 100, lda=104, ldb=104) == (R.RAN_128, 32)   # 16 x 8 = 128 workgroups, K < 128
    assert pick(l, L, "bf16", 2048, 896, 100, lda=104, ldb=104) == (R.RAN_64, 32)    # 16 x 7 = 112 workgroups of 128: 64x64 (32 x 14)
    assert pick(l, L, "bf16", 2048, 264, 136) == (R.RAN_64, 128)          # 16 x 3 tiles of 128, 32 x 5 = 160 of 64
    assert pick(l, L, "bf16", 520, 136, 136) == (R.RAN_32, 128)           # 9 x 3 = 27 tiles of 64
    assert pick(l, L, "bf16", 40, 40, 72) == (R.RAN_64, 32)               # M, N <= 64: one 64x64 tile
    ns, big = C.c_int32(), C.c_int32()
    for dtype, M, N, K, want in (("bf16", 64, 64, 1024, (4, 0)), ("bf16", 130, 140, 2048, (8, 1)), ("fp32", 64, 64, 1024, (1, 0)), ("bf16", 64, 64, 511, (1, 0)),
                                 ("fp16", 64, 64, 65536, (32, 0)), ("bf16", 2048, 1024, 2048, (1, 1)), ("bf16", 2048, 896, 2048, (2, 1))):
        L.check(l.hulc_k_gemm_wgrad_nsplit(L.DTYPE[dtype], M, N, K, C.byref(ns), C.byref(big)))
        assert (ns.value, big.value) == want, (dtype, M, N, K, ns.value, big.value)
