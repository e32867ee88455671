"""GPU (-m gpu): every GEMM kernel of csrc/gemm.h with the whole runtime epilogue (EpiP), through the C-ABI entries hulc_k_gemm_epi / hulc_k_gemm_dual, which launch
through the launchers the engine calls and report which kernel ran (asserted in every case: nothing falls through to another kernel).

Two comparisons per case, per element, no element excused.  PRODUCT: a launch with a plain fp32 store against gemm_epi_ref.product of the device's own rounded
operands at its accumulation bound (K + 2) 2^-24 sum |a||b|.  EPILOGUE: a second launch of the same kernel with the case's epilogue against
gemm_epi_ref.epilogue applied to the DEVICE's fp32 accumulators of the first launch (the same kernel instance, so the same summation order); mask and dropout
decisions come from the device inputs and the engine's hash of the element OFFSET.  Gate: the reference's derived fp32 bound ((operations + 1) 2^-24 sum
|addends|), plus one ulp of the type (never less than its subnormal spacing) for 16-bit stores, plus TANH_REL |ref| where relu == 2.  Output buffers start at
7.0 (tests/plan_ln_gpu_util.sevens convention) with guard elements; every element outside the result — the gaps of ldc > N and of the two-level row map, the
guards, the part of an out2 buffer outside its window's elements — must still hold 7.0.  Atomic split K (kernel 8) is order-nondeterministic: product bound
plus one rounding per slab over 7 + product.

Bit identity (drop_p = 0, alpha = 1): generic_only = 1 equals generic_only = 0 wherever epi_fast16 / epi_plain4 can run (kernels 4 and 5), and a rerun with an
odd ldc (scalar epi_store, (o & 3) != 0) equals the vector path after de-striding (kernels 2, 4, 5).

Cases: 401 tests, 2224 kernel launches, 3.5 s on one MI355X (bf16, fp16 and fp32; the LDS-DMA and skinny kernels for the 16-bit types).  Every one of the 34
epilogue cases of tests/gemm_epi_inputs.py EPI (each EpiP field alone, the pairs, every row of the launch-site table) runs on each of the kernels 1 .. 7; the
shape tests rotate a few of them over the shapes; no full cross product.

Worst err / gate measured (all types): product — gemm_kernel 32 / 64 / 128: 0.086 / 0.16 / 0.091, glds 0.025, skinny (router and
register form) 0.0074, kchunk 0.0001, dual 0.0003, atomic split K 0.0022; epilogue `out` — gemm_kernel 0.64 / 0.64 / 0.65, glds 0.62, skinny register form
0.58, router 0.53, kchunk, dual 0.50; `out2` — 0.47 .. 0.53.  (0.5 is the half ulp of round-to-nearest under a gate of one ulp; the values above it are
fp32 stores of a single fp32 operation, where one rounding sits under a bound of (1 + 1) 2^-24.)  Device tanhf against float64 tanh: measured 1.39e-7 relative
(2.3 x 2^-24, the rounding of the argument's sum included); the gate allows twice that (TANH_REL below).

Findings on bit identity, scalar epi_store against the vector path (generic_only = 1 against 0 agrees everywhere).  (1) With BOTH biases the vector paths add
bias + bias2 first, the scalar path one after the other: measured, about one element in five of an fp32 store differs in the last bit (941 of 4760 at
(70, 68, 136) fp32, 3511 of 17160 glds bf16; none of a 16-bit store).  (2) fp32 engine, tanh mask: 1 - m * m is contracted into one FMA on one path only:
497 of 4760 elements differ in the last bit.  Neither is a defect — both lie within the derived bound, where the tests gate them — and the arithmetic stays as
it is (the fp32 engine must reproduce the parent's bits); the claim is corrected instead: gemm.h now records the two differences at epi_prefetch4.

Mutations of gemm.h shown to fail these tests (each applied once to a scratch copy, bf16 + fp32 unit, one run; failing tests of the 425 the file had then, the retired grouped and shared-operand launch forms included): dropout index col + r
for o + r in epi_apply4 — 46 (every dropout case on every kernel with a vector path, the padded-ldc / row-map test); res_late ignored in epi_apply4 — 45
(res_late, res_late_drop, and the odd-ldc identity); the residual row (row + 1) % res_rowmod — 30 (rowmod, zx0; run in this in-bounds form: the literal
"without % res_rowmod" reads past the residual buffer, so it moves a load); bias2 skipped in epi_fast16_pre — 16 (bias12_16, zx1 on glds / skinny LDS,
and generic_only identity); mask test >= 0 — 59 (+0.0 and -0.0 of every ReLU mask and out2_mask); 1 - m for 1 - m * m — 30; out2_relu ignored — 76;
accumulate ignored by epi_plain4 (glds acc32, every-tile-once, both identities); alpha applied after the bias (vector paths) — 9 (alpha_bias).
None uncaught."""
import ctypes as C

import numpy as np
import pytest

import gemm_epi_inputs as GI
import gemm_epi_ref as G
import plan_ln_inputs as PI
from plan_ln_gpu_util import check_tol, load

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WORST = {}          # (kernel, output) -> worst err / gate over the session
COUNT = [0]
TANH_SEEN = [0.0]
GUARD = 24          # elements past the end of every output buffer
TINY = {"bf16": 2.0 ** -133, "fp16": 2.0 ** -24}
# device tanhf against float64 tanh over the inputs of the relu == 2 cases, relative to |tanh|: measured worst MEASURED_TANH (printed by every run as "tanh
# measured"); the gate allows twice that: the measurement covers some 10^5 arguments in [-4, 4], a factor of two covers the arguments it did not meet without
# admitting a wrong formula (1 - m^2 in place of tanh', a missing activation or a shifted argument are errors of order 1, seven decades above)
MEASURED_TANH = 1.39e-7          # measured 1.39e-07 = 2.3 x 2^-24 (includes the fp32 rounding of the argument's sum)
TANH_REL = 2.0 * MEASURED_TANH


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print(f"cases launched: {COUNT[0]}; tanh measured: {TANH_SEEN[0]:.3g} (relative to |tanh|)")
    for k in sorted(WORST):
        print(f"worst err/gate  {k[0]:14s} {k[1]:8s} {WORST[k]:.3g}")


def note(kernel, out, w):
    WORST[(kernel, out)] = max(WORST.get((kernel, out), 0.0), w)


def ulp16(ref, dtype):
    return np.maximum(PI.ULP[dtype] * np.abs(ref), TINY[dtype]) if dtype in TINY else 0.0


def ceil4(x):
    return (int(x) + 3) // 4 * 4


def buf(values, dtype):
    """a flat device buffer of the storage type from float64 values"""
    return torch.from_numpy(np.asarray(values, dtype=np.float32)).cuda().to(PI.tdt(dtype)).contiguous()


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


class Prob:
    """one product out = epilogue(A B^T): operands on the device, the output's element offsets, and per launch the buffers of an epilogue case"""

    def __init__(self, dtype, M, N, K, ldc=None, R1=0, s0=0, tag=""):
        self.dtype, self.M, self.N, self.K = dtype, M, N, K
        self.ldc, self.R1, self.s0 = ldc or N, R1, s0
        self.A = GI.matrix("A" + tag, M, K, dtype)
        self.B = GI.matrix("B" + tag, N, K, dtype)
        self.dA, self.dB = buf(self.A, dtype), buf(self.B, dtype)
        self.off = G.offsets(M, N, self.ldc, R1, s0)
        self.extent = ceil4(self.off.max() + 1)
        self.inside = np.zeros(self.extent + GUARD, bool)
        self.inside[self.off.reshape(-1)] = True
        self.keep = []          # device tensors of the launches in flight

    def scatter(self, logical, fill=GI.OLD, n=None):
        flat = np.full(self.extent if n is None else n, fill)
        flat[self.off.reshape(-1)] = np.asarray(logical).reshape(-1)
        return flat

    def job(self, L, e, generic_only=0, nsplit=1, wfrag=0, z_stride=0, atomic=0):
        """-> (ctypes job, ctx: the output buffers and the reference's fields)"""
        dtype, M, N = self.dtype, self.M, self.N
        f32 = bool(e.get("out_f32", 0))
        slabs = nsplit if z_stride else 1
        out = torch.full((self.extent + GUARD + (slabs - 1) * z_stride,), GI.OLD, device="cuda", dtype=torch.float32 if f32 else PI.tdt(dtype))
        j = L.HulcGemmEpiJob(A=self.dA.data_ptr(), B=self.dB.data_ptr(), M=M, N=N, K=self.K, lda=self.K, ldb=self.K, ldc=self.ldc, out_R1=self.R1, out_s0=self.s0,
                             nsplit=nsplit, wfrag=wfrag, out=out.data_ptr(), out_f32=int(f32), accumulate=e.get("accumulate", 0), atomic=atomic, z_stride=z_stride,
                             res_f32=0, res_late=e.get("res_late", 0), res_rowmod=e.get("res_rowmod", 0), mask_tanh=e.get("mask_tanh", 0), relu=e.get("relu", 0),
                             alpha=e.get("alpha", 1.0), drop_p=e.get("drop_p", 0.0), drop_seed=GI.SEED, out2_relu=e.get("out2_relu", 0), generic_only=generic_only)
        f = dict(alpha=float(np.float32(e.get("alpha", 1.0))), res_late=j.res_late, res_rowmod=j.res_rowmod, mask_tanh=j.mask_tanh, relu=j.relu, drop_p=e.get("drop_p", 0.0),
                 accumulate=j.accumulate, off=self.off)
        ctx = dict(out=out, f=f, f32=f32, keep=None, out2=None, e=e)
        hold = [out]
        for k in ("bias", "bias2"):
            if e.get(k):
                f[k] = GI.vector(k, N)
                t = buf(f[k], "fp32")
                setattr(j, k, t.data_ptr())
                hold.append(t)
        if e.get("res"):
            rt = "fp32" if e["res"] == "f32" else dtype
            rows = e.get("res_rowmod", 0) or M
            f["res"] = GI.matrix("res", rows, N, rt)
            t = buf(f["res"], rt)
            j.res, j.res_f32, j.res_ld = t.data_ptr(), int(e["res"] == "f32"), N
            hold.append(t)
        if e.get("mask"):
            f["mask"] = GI.mask_values("m", M * N, dtype, bool(e.get("mask_tanh", 0))).reshape(M, N)
            t = buf(self.scatter(f["mask"]), dtype)
            j.mask = t.data_ptr()
            hold.append(t)
        if e.get("drop_p", 0) > 0:
            ctx["keep"] = G.keep_mask(GI.SEED, e["drop_p"], self.off)
        if j.accumulate:
            f["old"] = np.full((M, N), GI.OLD)
        if e.get("out2"):
            nrows = min(e.get("res_rowmod", 0) or 5, M)
            if e["out2"] == "first":
                lo, hi = 0, ceil4(self.off[nrows - 1, N - 1] + 1)
            elif e["out2"] == "last":
                lo, hi = int(self.off[M - nrows, 0]) // 4 * 4, self.extent
            else:
                lo, hi = int(e["out2"][0] * self.extent) // 4 * 4, ceil4(e["out2"][1] * self.extent)
            hi = min(hi, self.extent)
            o2 = torch.full((hi - lo + GUARD,), GI.OLD, device="cuda", dtype=PI.tdt(dtype))
            j.out2, j.out2_lo, j.out2_hi = o2.data_ptr(), lo, hi
            f["out2_lo"], f["out2_hi"], f["out2_relu"] = lo, hi, j.out2_relu
            ctx["out2"] = o2
            hold.append(o2)
            if e.get("out2_mask"):
                m2 = GI.mask_values("m2", M * N, dtype, False).reshape(M, N)
                f["out2_mask"] = self.scatter(m2, 1.0)[lo:hi]
                t = buf(f["out2_mask"], dtype)
                j.out2_mask = t.data_ptr()
                hold.append(t)
        self.keep.append(hold)
        return j, ctx

    def read(self, ctx, what, slab=0, z_stride=0):
        """-> the logical [M][N] result as float64; everything outside it must still hold 7.0"""
        flat = host(ctx["out"])
        if z_stride == 0:
            assert (flat[~self.inside] == GI.OLD).all(), f"{what}: elements outside the result (gaps of the row map or guards) were written"
        return flat[slab * z_stride:][self.off]

    def read2(self, ctx, what):
        """-> out2 flat over its window (float64), the window's logical selection"""
        f = ctx["f"]
        flat = host(ctx["out2"])
        n = f["out2_hi"] - f["out2_lo"]
        assert (flat[n:] == GI.OLD).all(), f"{what}: out2 written past its window"
        return flat[:n]


def launch(L, lib, dtype, kernel, j, want, what):
    ran = C.c_int32(-1)
    L.check(lib.hulc_k_gemm_epi(L.DTYPE[dtype], C.byref(j), kernel, C.byref(ran), None))
    torch.cuda.synchronize()
    COUNT[0] += 1
    assert ran.value == want, f"{what}: kernel {kernel} ran {ran.value}, expected {want}"


def check_product(p, acc, kname, what, nsplit=1, old=0.0, ops=(None, None)):
    """acc against the fp64 product of the device's own operands (ops: other operands than the problem's); old: what the output held before an accumulating or
    atomic launch — each of its nsplit additions rounds relative to at most old + sum |a||b|"""
    A, B = (p.A if ops[0] is None else ops[0]), (p.B if ops[1] is None else ops[1])
    r, bnd = G.product(A, B, nsplit) if A.shape[1] else (np.zeros((p.M, p.N)), np.zeros((p.M, p.N)))
    if old:
        r, bnd = r + old, bnd + (nsplit + 1) * PI.EPS32 * (old + np.abs(A) @ np.abs(B).T)
    note(kname, "product", check_tol(np.abs(acc - r), bnd, acc, r, what + " product"))


def check_epilogue(p, ctx, acc, kname, what):
    """the epilogue launch `ctx` against the reference applied to the device accumulators `acc`"""
    e, dtype = ctx["e"], p.dtype
    ref, ref2, bnd, bnd2 = G.epilogue(acc, ctx["f"], ctx["keep"])
    got = p.read(ctx, what)
    tol = bnd + (0.0 if ctx["f32"] else ulp16(ref, dtype))
    if e.get("relu", 0) == 2:
        pure = np.tanh(acc * ctx["f"]["alpha"] + (ctx["f"]["res"][np.arange(p.M) % (e.get("res_rowmod", 0) or p.M)] if "res" in ctx["f"] else 0.0))
        if ctx["f32"] or dtype == "fp32":
            rel = np.abs(got - ref) / np.maximum(np.abs(pure), 1e-30)
            TANH_SEEN[0] = max(TANH_SEEN[0], float(rel.max()))
        tol = tol + TANH_REL * np.abs(pure)
    note(kname, "out", check_tol(np.abs(got - ref), tol, got, ref, what + " out"))
    if e.get("drop_p", 0) > 0:
        dropped = ~ctx["keep"]
        res_late = ctx["f"]["res"] if e.get("res_late", 0) else 0.0
        assert dropped.any() and (np.abs(got - (res_late + (GI.OLD if e.get("accumulate", 0) else 0.0)))[dropped] <= tol[dropped]).all()
    if ref2 is not None:
        got2 = p.read2(ctx, what)
        hole = np.isnan(ref2)
        assert (got2[hole] == GI.OLD).all(), f"{what}: out2 written at offsets that belong to no element"
        assert not hole.all(), f"{what}: the out2 window is empty"
        r2 = np.where(hole, GI.OLD, ref2)
        note(kname, "out2", check_tol(np.abs(got2 - r2), np.where(hole, 0.0, bnd2 + ulp16(r2, dtype if dtype in TINY else "fp32")), got2, r2, what + " out2"))
    return got


KNAME = {1: "gemm32", 2: "gemm64", 3: "gemm128", 4: "glds", 5: "skinny_router", 6: "skinny_reg", 7: "kchunk", 8: "splitk"}


def both(L, lib, dtype, kernel, M, N, K, epis, ldc=None, R1=0, s0=0, wfrag=0, want=None, generic_only=0):
    """the product launch, then one epilogue launch per case of `epis`, each checked.  -> {case: logical output}"""
    p = Prob(dtype, M, N, K, ldc, R1, s0)
    want = want or GI.expected_ran(kernel, dtype, M, N, K)
    what = f"{KNAME.get(kernel, 'pick')} [{dtype}] {M}x{N}x{K} ldc={p.ldc}" + (f" map({R1},{s0})" if s0 else "") + (" wfrag" if wfrag else "")
    j, ctx = p.job(L, GI.EPI["bare32"], wfrag=wfrag)
    launch(L, lib, dtype, kernel, j, want, what)
    acc = p.read(ctx, what)
    kname = KNAME.get(kernel, "pick")
    check_product(p, acc, kname, what)
    outs = {}
    for name in epis:
        e = GI.EPI[name]
        j, ctx = p.job(L, e, generic_only=generic_only, wfrag=wfrag)
        launch(L, lib, dtype, kernel, j, want, f"{what} {name}")
        outs[name] = check_epilogue(p, ctx, acc, kname, f"{what} {name}")
    return outs


ROTATE = ("res_late_drop", "zx0", "rnn_bwd_tanh", "acc16", "out2_window", "relu_drop", "dh_last", "mask_alpha")


def types_of(kernel):
    return GI.DTYPES if kernel in (0, 1, 2, 3, 8) else GI.DTYPES16          # the LDS-DMA and skinny kernels exist for the 16-bit types only


# ==================================================================================================== shapes
@pytest.mark.parametrize("dtype", GI.DTYPES)
@pytest.mark.parametrize("K", GI.TILE_KS)
@pytest.mark.parametrize("kernel", [1, 2, 3])
def test_tile_kernels_at_ragged_shapes(kernel, K, dtype):
    """gemm_kernel 32x32 / 64x64 / 128x128: one tile plus a remainder that is no multiple of 4, K across the BK choices and their tails"""
    L, lib = load()
    M, N = GI.TILE_SHAPES[kernel]
    i = GI.TILE_KS.index(K) + kernel
    both(L, lib, dtype, kernel, M, N, K, ("bare16", ROTATE[i % len(ROTATE)], ROTATE[(i + 3) % len(ROTATE)]))


@pytest.mark.parametrize("dtype", GI.DTYPES)
@pytest.mark.parametrize("kernel", [1, 2, 3])
def test_tile_kernels_n_multiple_of_four_but_odd_leading_dimension(kernel, dtype):
    L, lib = load()
    M, N = GI.TILE_SHAPES[kernel]
    both(L, lib, dtype, kernel, M, N // 4 * 4, 136, ("bare16", "res_late_drop", "zx1", "rnn_bwd", "rnn_bwd_tanh", "cplan"), ldc=N // 4 * 4 + 3)


@pytest.mark.parametrize("dtype", GI.DTYPES16)
@pytest.mark.parametrize("K", GI.GLDS_KS)
def test_glds_ring_stages(K, dtype):
    """gemm_glds_kernel (130, 132): 1 .. 4 ring stages, the ring wrap, the half step before and after it"""
    L, lib = load()
    i = GI.GLDS_KS.index(K)
    both(L, lib, dtype, 4, 130, 132, K, ("bare16", "acc32", ROTATE[i % len(ROTATE)], ROTATE[(i + 5) % len(ROTATE)]))


@pytest.mark.parametrize("dtype", GI.DTYPES16)
def test_glds_every_tile_exactly_once(dtype):
    """(643, 384, 64): 18 tiles — no multiple of 8, tiles_m no multiple of 4; accumulate from 7.0, so a tile computed twice shows as well as one left out"""
    L, lib = load()
    both(L, lib, dtype, 4, 643, 384, 64, ("acc32", "acc16", "bare16"))


@pytest.mark.parametrize("dtype", GI.DTYPES16)
@pytest.mark.parametrize("K", GI.SKINNY_KS)
@pytest.mark.parametrize("N", GI.SKINNY_NS)
@pytest.mark.parametrize("M", GI.SKINNY_MS)
@pytest.mark.parametrize("kernel", [5, 6])
def test_skinny_shapes(kernel, M, N, K, dtype):
    """the production skinny router (LDS-DMA forms where they apply) and the register-fragment kernel"""
    L, lib = load()
    i = GI.SKINNY_MS.index(M) + GI.SKINNY_KS.index(K) + N // 16
    both(L, lib, dtype, kernel, M, N, K, ("bare16", ("rnn_fwd", "rnn_bwd", "zx1", "res_late_drop", "acc16")[i % 5]))


@pytest.mark.parametrize("dtype", GI.DTYPES16)
@pytest.mark.parametrize("kernel", [5, 6])
def test_skinny_many_rows(kernel, dtype):
    L, lib = load()
    both(L, lib, dtype, kernel, 500, 128, 2048, ("bare16", "zx0", "acc32"))


@pytest.mark.parametrize("dtype", GI.DTYPES16)
@pytest.mark.parametrize("wfrag", [0, 1])
@pytest.mark.parametrize("shape", GI.KCHUNK_SHAPES)
def test_kchunk_row_major_and_fragment_ordered_weights(shape, wfrag, dtype):
    L, lib = load()
    both(L, lib, dtype, 7, *shape, ("bare16", "res16", "rnn_bwd_tanh"), wfrag=wfrag)


@pytest.mark.parametrize("dtype", GI.DTYPES)
@pytest.mark.parametrize("ns", ["rule", 2, 32])
@pytest.mark.parametrize("shape", GI.SPLITK_SHAPES)
def test_split_k_atomic(shape, ns, dtype):
    """kernel 8: 7 + product within the product bound plus one rounding per slab"""
    L, lib = load()
    M, N, K = shape
    if ns == "rule":
        n, big = C.c_int32(), C.c_int32()
        L.check(lib.hulc_k_gemm_wgrad_nsplit(L.DTYPE["bf16"], M, N, K, C.byref(n), C.byref(big)))
        ns = n.value
        assert ns == {1024: 4, 2048: 8}[K]
    p = Prob(dtype, M, N, K, ldc=N + 4)
    what = f"splitk [{dtype}] {M}x{N}x{K} nsplit={ns}"
    j, ctx = p.job(L, GI.EPI["bare32"], nsplit=ns, atomic=1)
    launch(L, lib, dtype, 8, j, GI.expected_ran(8, dtype, M, N, K), what)
    check_product(p, p.read(ctx, what), "splitk", what, nsplit=ns, old=GI.OLD)


@pytest.mark.parametrize("dtype", GI.DTYPES)
def test_split_k_slabs(dtype):
    """kernel 2 with nsplit = 3 and z_stride: slab s holds the product over its own K range (the range launch_gemm derives: ceil(K / nsplit) rounded up to BK)"""
    L, lib = load()
    M, N, K, ns = 70, 67, 264, 3
    p = Prob(dtype, M, N, K)
    zs = p.extent + 8
    j, ctx = p.job(L, GI.EPI["bare32"], nsplit=ns, z_stride=zs)
    what = f"slabs [{dtype}] {M}x{N}x{K}"
    launch(L, lib, dtype, 2, j, GI.RAN_64, what)
    bk = 32 if dtype == "fp32" else 128
    ks = ((K + ns - 1) // ns + bk - 1) // bk * bk
    for s in range(ns):
        a, b = p.A[:, s * ks:(s + 1) * ks], p.B[:, s * ks:(s + 1) * ks]
        check_product(p, p.read(ctx, what, s, zs), "gemm64", f"{what} slab {s}", ops=(a, b))
    flat = host(ctx["out"])
    for s in range(ns):
        seg = flat[s * zs:(s + 1) * zs] if s < ns - 1 else flat[s * zs:]
        inside = np.zeros(seg.size, bool)
        inside[p.off.reshape(-1)] = True
        assert (seg[~inside] == GI.OLD).all(), f"{what}: slab {s} wrote outside its result"


@pytest.mark.parametrize("dtype", GI.DTYPES)
@pytest.mark.parametrize("kernel", [0, 2])
def test_dropout_through_a_padded_leading_dimension_and_the_two_level_row_map(kernel, dtype):
    """the hash is keyed by the element offset: ldc > N, and dense_out_map(B, EMB, S * EMB) — row r = t * B + b lands at b * S * EMB + t * EMB"""
    L, lib = load()
    Bw, S, N = 5, 4, 38
    want = GI.RAN_64
    both(L, lib, dtype, kernel, Bw * S, N, 136, ("drop", "res_late_drop", "relu_drop"), ldc=N + 6, want=want)
    both(L, lib, dtype, kernel, Bw * S, N, 136, ("drop", "res_late_drop", "acc32", "out2_window"), ldc=S * 40, R1=Bw, s0=40, want=want)


# ==================================================================================================== every epilogue case on every kernel
EPI_SHAPES = {1: (45, 38, 136), 2: (70, 67, 136), 3: (130, 133, 136), 4: (130, 132, 96), 5: (33, 48, 512), 6: (17, 48, 160), 7: (33, 32, 4096)}
EPI_GROUPS = [sorted(GI.EPI)[i::4] for i in range(4)]


@pytest.mark.parametrize("kernel,group,dtype", [(k, g, d) for k in sorted(EPI_SHAPES) for g in range(4) for d in types_of(k)])
def test_every_epilogue_case(kernel, group, dtype):
    """every row of the launch-site table, each EpiP field alone and the pairs (tests/gemm_epi_inputs.py EPI), on each kernel"""
    L, lib = load()
    both(L, lib, dtype, kernel, *EPI_SHAPES[kernel], EPI_GROUPS[group])


# ==================================================================================================== bit identity
def identical(a, b, what, bad):
    """records a difference instead of stopping at the first: the assertion at the end of the test names every case that differs"""
    if not np.array_equal(a, b):
        bad.append(f"{what}: {int((a != b).sum())} of {a.size} elements differ, first at {np.argwhere(a != b)[0].tolist()}: {a[a != b][0]!r} vs {b[a != b][0]!r}")


def no_drop(name):
    e = dict(GI.EPI[name])
    e["drop_p"] = 0.0
    return e


@pytest.mark.parametrize("dtype", GI.DTYPES16)
@pytest.mark.parametrize("kernel,shape", [(4, (130, 132, 96)), (5, (33, 48, 512)), (5, (64, 48, 2048))])
def test_generic_only_equals_the_compact_paths_bit_for_bit(kernel, shape, dtype):
    """epi_fast16 and epi_plain4 claim the arithmetic and order of the generic vector path: the same launch with generic_only = 1 gives the same bits"""
    L, lib = load()
    names = [n for n in sorted(GI.EPI) if GI.uses_fast_path(GI.EPI[n], dtype)]
    assert len(names) >= 12
    p = Prob(dtype, *shape)
    want = GI.expected_ran(kernel, dtype, *shape)
    bad = []
    for name in names:
        got = []
        for g in (0, 1):
            j, ctx = p.job(L, GI.EPI[name], generic_only=g)
            launch(L, lib, dtype, kernel, j, want, name)
            got.append((p.read(ctx, name), p.read2(ctx, name) if ctx["out2"] is not None else np.zeros(0)))
        identical(got[0][0], got[1][0], f"{KNAME[kernel]} [{dtype}] {name} out, generic_only 0 vs 1", bad)
        identical(got[0][1], got[1][1], f"{KNAME[kernel]} [{dtype}] {name} out2, generic_only 0 vs 1", bad)
    assert not bad, "\n".join(bad)


ODD_LDC = [(2, (70, 68, 136)), (4, (130, 132, 96)), (5, (33, 48, 512))]


def two_biases(name):
    return bool(GI.EPI[name].get("bias") and GI.EPI[name].get("bias2"))


@pytest.mark.parametrize("kernel,shape,dtype", [(k, s, d) for k, s in ODD_LDC for d in types_of(k)])
def test_odd_leading_dimension_equals_the_vector_path_bit_for_bit(kernel, shape, dtype):
    """an odd ldc sends every lane through the scalar epi_store ((o & 3) != 0); with alpha == 1 and no dropout the de-strided result equals the vector path's.
    Two exceptions, both recorded in gemm.h at epi_prefetch4 and compared at the derived bound by test_tile_kernels_n_multiple_of_four_but_odd_leading_dimension
    (zx1, cplan, rnn_bwd_tanh) instead: the cases with BOTH biases — the vector paths add bias + bias2 first and then the sum to the accumulator, the scalar path adds
    them one after the other — and, for fp32 only, the tanh mask: 1 - m * m is contracted into one FMA on one path and not on the other (measured: 497 of 4760
    elements differ in the last bit at (70, 68, 136); with a 16-bit mask m * m is exact in fp32 and the paths agree)."""
    L, lib = load()
    M, N, K = shape
    names = [n for n in sorted(GI.EPI) if GI.EPI[n].get("alpha", 1.0) == 1.0 and not GI.EPI[n].get("out2") and not two_biases(n)
             and not (dtype == "fp32" and GI.EPI[n].get("mask_tanh"))]
    pv, ps = Prob(dtype, M, N, K), Prob(dtype, M, N, K, ldc=N + 5)
    want = GI.expected_ran(kernel, dtype, M, N, K)
    bad = []
    for name in names:
        e = no_drop(name)
        got = []
        for p in (pv, ps):
            j, ctx = p.job(L, e)
            launch(L, lib, dtype, kernel, j, want, name)
            got.append(p.read(ctx, name))
        identical(got[0], got[1], f"{KNAME[kernel]} [{dtype}] {name}: ldc = N (vector) vs ldc = N + 5 (scalar)", bad)
    assert not bad, "\n".join(bad)


# ==================================================================================================== dual
def dual(L, lib, dtype, probs, epis, what):
    """one hulc_k_gemm_dual launch over the two `probs` with the epilogue cases `epis` -> the contexts"""
    jobs, ctxs = (L.HulcGemmEpiJob * 2)(), []
    for i, (p, name) in enumerate(zip(probs, epis)):
        jobs[i], ctx = p.job(L, GI.EPI[name])
        ctxs.append(ctx)
    ran = C.c_int32(-1)
    L.check(lib.hulc_k_gemm_dual(L.DTYPE[dtype], jobs, C.byref(ran), None))
    torch.cuda.synchronize()
    COUNT[0] += 1
    assert ran.value == GI.RAN_DUAL, (what, ran.value)
    return ctxs


@pytest.mark.parametrize("dtype", GI.DTYPES16)
@pytest.mark.parametrize("epis", [("rnn_fwd", "rnn_bwd"), ("rnn_fwd_tanh", "rnn_bwd_tanh"), ("rnn_bwd", "rnn_fwd")])
@pytest.mark.parametrize("M,N", [(33, 32), (64, 48)])
def test_dual_launch_with_two_different_epilogues(M, N, epis, dtype):
    """skinny_lds_kernel<2, 4, 16, true>: the forward step's ReLU / tanh with residual beside the backward step's mask with residual (engine_recurrent.inc:147 / :177)"""
    L, lib = load()
    probs = [Prob(dtype, M, N, 2048, tag=f"d{i}") for i in range(2)]
    what = f"dual [{dtype}] {M}x{N}x2048 {epis}"
    accs = [p.read(c, what) for p, c in zip(probs, dual(L, lib, dtype, probs, ["bare32"] * 2, what))]
    ctxs = dual(L, lib, dtype, probs, epis, what)
    for i, (p, c, a) in enumerate(zip(probs, ctxs, accs)):
        check_product(p, a, "dual", f"{what} problem {i}")
        check_epilogue(p, c, a, "dual", f"{what} problem {i} {epis[i]}")


def test_routed_kernel_is_reported():
    """kernel 0 launches what gemm_pick chooses and says so"""
    L, lib = load()
    for dtype, M, N, K, want in (("bf16", 33, 48, 512, GI.RAN_ROUTER), ("fp32", 33, 48, 512, GI.RAN_64), ("bf16", 2048, 1024, 64, GI.RAN_GLDS), ("fp16", 520, 136, 136, GI.RAN_32),
                                 ("bf16", 2048, 900, 104, GI.RAN_128)):
        both(L, lib, dtype, 0, M, N, K, ("bias12_16",), want=want)
