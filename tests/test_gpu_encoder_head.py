"""GPU (-m gpu): the kernels of the 16-bit encoder head alone, in both 16-bit types, element by element against float64 (tests/enc_head_ref.py) on the
same 16-bit-rounded operands: spatial_softmax_fwd64 / bwd64 (csrc/kernels.h) and enc_tail_fwd / enc_tail_bwd (csrc/enc_tail.h) through their C-ABI test
entries.  Every stage of a multi-stage kernel is checked from the device's own output of the stage before it, every output buffer starts at 7.0 and has
guard rows past Nf that must still hold 7.0 afterwards.

Gates.  16-bit output: |got - ref| <= u |ref| + a, u = one unit in the last place of the storage type (2^-7 bf16, 2^-10 fp16), a = 2e-5 max|ref| (fp32
accumulation, the bound of test_gemm_glds_matches_fp64).  fp32 output of a dot product: 2e-5 max|ref|.  Softmax statistics: maximum bit-exact, coordinates
absolute and 1 / sum relative at 5 x the float32-vs-float64 error measured on each shape's own inputs (tests/enc_head_inputs.py SS_F32 / SS_GATE: from
2.05e-6 / 1.9e-6 at 3x3 to 5.75e-5 / 6.6e-5 at 16x28; re-measured by tests/test_enc_head_ref_host.py).  LayerNorm statistics: 2e-5 relative per row, mean and rstd."""
import functools

import numpy as np
import pytest

import enc_head_ref as R
from enc_head_inputs import ACC, SS_GATE, SS_NF, SS_SHAPES, TINY, ULP, round16, ss_inputs, tdt
import hulc_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 3          # rows past Nf in every output buffer


def _lib():
    from hulc_amd import lib as L
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    return L, L.load()


def h16(x, dtype):
    """x rounded to the 16-bit storage type, on the device"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda().to(tdt(dtype)).contiguous()


def f32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def f64(t):
    return t.float().cpu().numpy().astype(np.float64)


def sevens(shape, td=torch.float32):
    return torch.full(shape, 7.0, device="cuda", dtype=td)


def ptr(t):
    return None if t is None else t.data_ptr()


def check16(got, ref, dtype, what):
    """a 16-bit output, per element: one ulp of the storage type + the fp32 accumulation bound"""
    ref = np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    tol = ULP[dtype] * np.abs(ref) + ACC * np.abs(ref).max()
    k = np.unravel_index(np.argmax(err - tol), err.shape)
    print(f"{what} [{dtype}]: worst err/tol = {float((err / tol).max()):.3f} (max|ref| {float(np.abs(ref).max()):.4g})")
    assert (err <= tol).all(), f"{what}: element {k}: got {got[k]!r} ref {ref[k]!r} tol {tol[k]:.3g} ({int((err > tol).sum())} elements off)"


def check32(got, ref, what, scale=1.0):
    """an fp32 output of a dot product: 2e-5 max|ref| (times `scale`)"""
    ref = np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    tol = ACC * scale * np.abs(ref).max()
    print(f"{what}: worst err/tol = {float(err.max() / tol):.3f} (max|ref| {float(np.abs(ref).max()):.4g})")
    k = np.unravel_index(np.argmax(err), err.shape)
    assert err.max() <= tol, f"{what}: element {k}: got {got[k]!r} ref {ref[k]!r} tol {tol:.3g}"


def guard_intact(t, Nf, what):
    assert (t[Nf:].float() == 7.0).all(), f"{what}: rows past Nf were written"


# ==================================================================================================== spatial softmax
def ss_forward(lib, L, dtype, ft, H, W):
    out = sevens((SS_NF + GUARD, 128), tdt(dtype))
    stats = sevens((SS_NF + GUARD, 64, 4))
    L.check(lib.hulc_k_spatial_softmax64(L.DTYPE[dtype], ft.data_ptr(), H, W, SS_NF, out.data_ptr(), stats.data_ptr(), None, None, None))
    torch.cuda.synchronize()
    guard_intact(out, SS_NF, "out")
    guard_intact(stats, SS_NF, "stats")
    return out, stats


def ss_backward(lib, L, dtype, ft, H, W, stats_t, dout_t):
    df = sevens((SS_NF + GUARD, H, W, 64), tdt(dtype))
    L.check(lib.hulc_k_spatial_softmax64(L.DTYPE[dtype], ft.data_ptr(), H, W, SS_NF, None, stats_t.data_ptr(), dout_t.data_ptr(), df.data_ptr(), None))
    torch.cuda.synchronize()
    guard_intact(df, SS_NF, "df")
    return f64(df[:SS_NF])


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("H,W", SS_SHAPES)
def test_spatial_softmax_forward(H, W, dtype):
    L, lib = _lib()
    f = ss_inputs(H, W, dtype)
    ft = h16(f, dtype)
    ref_out, (M, inv, ex, ey) = R.spatial_softmax_fwd(f)
    out, stats = ss_forward(lib, L, dtype, ft, H, W)
    st = stats[:SS_NF].cpu().numpy()
    assert (st[..., 0] == M.astype(np.float32)).all(), "the maximum must be bit-exact"
    ec = max(np.abs(st[..., 2] - ex).max(), np.abs(st[..., 3] - ey).max())
    ei = (np.abs(st[..., 1] - inv) / inv).max()
    gate_c, gate_i = SS_GATE[H, W]
    print(f"stats [{dtype} {H}x{W}]: coordinates {ec:.3g} (gate {gate_c:.3g}), 1/sum {ei:.3g} (gate {gate_i:.3g})")
    assert ec <= gate_c and ei <= gate_i
    # the constructed channels: uniform softmax of an all-zero / all-equal channel sits at the centre, 1/sum = 1/(H W)
    assert np.abs(st[:, [0, 2], 2:4]).max() <= gate_c and (np.abs(st[:, [0, 2], 1] * (H * W) - 1) <= gate_i).all()
    check16(f64(out[:SS_NF]), ref_out, dtype, f"out {H}x{W}")


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("H,W", SS_SHAPES)
def test_spatial_softmax_backward(H, W, dtype):
    """df from float64 statistics (handed to the kernel as fp32) against float64; closed entries (f <= 0) exactly zero."""
    L, lib = _lib()
    f = ss_inputs(H, W, dtype)
    ft = h16(f, dtype)
    _, st64 = R.spatial_softmax_fwd(f)
    dout = np.random.default_rng(H + W).standard_normal((SS_NF, 128)).astype(np.float32)
    stats_t = f32(np.stack(st64, -1))
    df = ss_backward(lib, L, dtype, ft, H, W, stats_t, f32(dout))
    ref = R.spatial_softmax_bwd(f, st64, dout.astype(np.float64))
    assert (f <= 0).any() and (df[f <= 0] == 0).all(), "entries with f <= 0 must be exactly zero"
    check16(df, ref, dtype, f"df {H}x{W}")


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("H,W", [(21, 21), (7, 7)])
def test_spatial_softmax_forward_then_backward(H, W, dtype):
    """The engine's sequence: the backward reads the statistics the forward left on the device; reference from those same statistics."""
    L, lib = _lib()
    f = ss_inputs(H, W, dtype)
    ft = h16(f, dtype)
    _, stats = ss_forward(lib, L, dtype, ft, H, W)
    dout = np.random.default_rng(H).standard_normal((SS_NF, 128)).astype(np.float32)
    df = ss_backward(lib, L, dtype, ft, H, W, stats, f32(dout))
    st = f64(stats[:SS_NF])
    ref = R.spatial_softmax_bwd(f, tuple(st[..., i] for i in range(4)), dout.astype(np.float64))
    assert (df[f <= 0] == 0).all()
    check16(df, ref, dtype, f"df after forward {H}x{W}")


def test_spatial_softmax_entry_validates():
    L, lib = _lib()
    t = sevens((4, 4))
    p = t.data_ptr()
    assert lib.hulc_k_spatial_softmax64(1, p, 1, 4, 1, p, p, None, None, None) == 1          # H < 2: the coordinate step 2 / (H - 1) does not exist
    assert lib.hulc_k_spatial_softmax64(1, p, 2, 2, 0, p, p, None, None, None) == 1
    assert lib.hulc_k_spatial_softmax64(1, p, 2, 2, 1, None, p, None, None, None) == 1          # forward without out
    assert lib.hulc_k_spatial_softmax64(1, p, 2, 2, 1, None, p, p, None, None) == 1          # backward without df
    assert lib.hulc_k_spatial_softmax64(0, p, 2, 2, 1, p, p, None, None, None) == 1          # fp32 is not a 16-bit type
    assert b"hulc_k_spatial_softmax64" in lib.hulc_last_error()
    torch.cuda.synchronize()
    assert (t == 7.0).all()


# ==================================================================================================== dense tail
TAIL_NF = [1, 15, 16, 17, 37]          # one ragged tile | one row short of a tile | exactly one | one row over | three tiles, the last with 5 rows


@functools.lru_cache(maxsize=None)
def tail_weights(dtype):
    """per camera (0 static, 1 gripper): W1, W2 rounded to the storage type (float64 values), fp32 biases and LayerNorm parameters"""
    rng = np.random.default_rng(77)
    cams = []
    for k in range(2):
        W1 = round16(0.09 * rng.standard_normal((512, 128)), dtype)
        W2 = round16(0.05 * rng.standard_normal((64, 512)), dtype)
        b1, b2 = (0.1 * rng.standard_normal(512)).astype(np.float32), (0.1 * rng.standard_normal(64)).astype(np.float32)
        lng, lnb = (1 + 0.1 * rng.standard_normal(64)).astype(np.float32), (0.1 * rng.standard_normal(64)).astype(np.float32)
        cams.append(dict(W1=W1, W2=W2, b1=b1, b2=b2, lng=lng, lnb=lnb))
    return cams


def tail_x(Nf, dtype):
    """static camera: spatial-softmax coordinates in [-1, 1]; gripper camera: a ReLU output"""
    rng = np.random.default_rng(Nf)
    return [round16(rng.uniform(-1, 1, (Nf, 128)), dtype), round16(np.maximum(rng.standard_normal((Nf, 128)), 0), dtype)]


def run_tail_fwd(lib, L, dtype, Nf, xs, pos=None, S=1, drop_p=0.0, seed=0, null_pos=False):
    W = tail_weights(dtype)
    keep, jobs, outs = [], [], []
    for k in range(2):
        c = W[k]
        dev = dict(x=h16(xs[k], dtype), W1=h16(c["W1"], dtype), W2=h16(c["W2"], dtype), b1=f32(c["b1"]), b2=f32(c["b2"]), lng=f32(c["lng"]), lnb=f32(c["lnb"]),
                   f1=sevens((Nf + GUARD, 512), tdt(dtype)), f2=sevens((Nf + GUARD, 64)), lnst=sevens((Nf + GUARD, 2)))
        keep.append(dev)
        jobs.append(L.HulcEncTailJob(*[dev[n].data_ptr() for n in ("x", "W1", "W2", "b1", "b2", "lng", "lnb", "f1", "f2", "lnst")], 64 * k))
        outs.append(dev)
    emb = sevens((Nf + GUARD, 128), tdt(dtype))
    x0 = dict(xf=sevens((Nf + GUARD, 128)), xt=sevens((Nf + GUARD, 128), tdt(dtype)), z0=sevens((Nf + GUARD, 128)), z1=sevens((Nf + GUARD, 128)))
    pos_t = None if pos is None or null_pos else f32(pos)
    import ctypes as C
    L.check(lib.hulc_k_enc_tail_fwd(L.DTYPE[dtype], Nf, 128, C.byref(jobs[0]), C.byref(jobs[1]), emb.data_ptr(), ptr(pos_t), S, drop_p, seed,
                                    x0["xf"].data_ptr(), x0["xt"].data_ptr(), x0["z0"].data_ptr(), x0["z1"].data_ptr(), None))
    torch.cuda.synchronize()
    guard_intact(emb, Nf, "emb")
    for k in range(2):
        for n in ("f1", "f2", "lnst"):
            guard_intact(outs[k][n], Nf, f"camera {k} {n}")
    for n, t in x0.items():
        guard_intact(t, Nf, n)
    return outs, emb, x0


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("Nf", TAIL_NF)
def test_enc_tail_forward(Nf, dtype):
    """f1 from x; f2 from the device's f1; emb and the LayerNorm statistics (mean and rstd, each 2e-5 relative per row) from the device's f2."""
    L, lib = _lib()
    xs = tail_x(Nf, dtype)
    outs, emb, x0 = run_tail_fwd(lib, L, dtype, Nf, xs)
    W = tail_weights(dtype)
    for k in range(2):
        c = W[k]
        f1 = f64(outs[k]["f1"][:Nf])
        check16(f1, R.tail_fc1(xs[k], c["W1"], c["b1"].astype(np.float64)), dtype, f"camera {k} f1")
        f2 = f64(outs[k]["f2"][:Nf])
        check32(f2, R.tail_fc2(f1, c["W2"], c["b2"].astype(np.float64)), f"camera {k} f2")
        y, mean, rstd = R.tail_ln(f2, c["lng"].astype(np.float64), c["lnb"].astype(np.float64))
        check16(f64(emb[:Nf, 64 * k:64 * k + 64]), y, dtype, f"camera {k} emb")
        st = f64(outs[k]["lnst"][:Nf])
        print(f"camera {k} lnst [{dtype}]: worst relative error mean {float((np.abs(st[:, 0] - mean) / np.abs(mean)).max()):.3g}, rstd {float((np.abs(st[:, 1] - rstd) / rstd).max()):.3g}")
        assert (np.abs(st[:, 1] - rstd) <= ACC * rstd).all(), "rstd"
        assert (np.abs(st[:, 0] - mean) <= ACC * np.abs(mean)).all(), "mean"
    for t in x0.values():          # pos == NULL: the transformer-input buffers are not touched
        assert (t.float() == 7.0).all()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("drop_p", [0.0, 0.1])
def test_enc_tail_forward_x0(drop_p, dtype):
    """The transformer input of the same launch: xf = dropout(emb + pos[row % S]) from the device's emb with the engine's exact keep mask, xt within one ulp of the
    device's xf (below fp16's normal range, where a sum emb + pos may land, its absolute step 2^-24 instead), both FFN accumulators exactly zero; without pos none of the four buffers is written."""
    L, lib = _lib()
    Nf, S, seed = 35, 5, 0x1234567
    xs = tail_x(Nf, dtype)
    pos = np.random.default_rng(3).standard_normal((S, 128)).astype(np.float32)
    outs, emb, x0 = run_tail_fwd(lib, L, dtype, Nf, xs, pos, S, drop_p, seed)
    keep = O.engine_keep_mask(seed, (Nf, 128), drop_p)
    if drop_p > 0:
        assert 0.05 < 1 - keep.mean() < 0.15
    ref = R.tail_x0(f64(emb[:Nf]), pos.astype(np.float64), S, keep, drop_p)
    xf = f64(x0["xf"][:Nf])
    assert ((xf == 0) == ~keep).all() or drop_p == 0, "the keep mask must be the engine's, element for element"
    check32(xf, ref, "xf")
    xt = f64(x0["xt"][:Nf])
    assert (np.abs(xt - xf) <= ULP[dtype] * np.abs(xf) + TINY[dtype]).all(), "xt is the 16-bit rounding of xf"
    assert (x0["z0"][:Nf] == 0).all() and (x0["z1"][:Nf] == 0).all()
    # the tail's own outputs do not depend on the x0 path
    outs_b, emb_b, x0_b = run_tail_fwd(lib, L, dtype, Nf, xs, pos, S, drop_p, seed, null_pos=True)
    assert torch.equal(emb_b, emb) and all(torch.equal(outs_b[k][n], outs[k][n]) for k in range(2) for n in ("f1", "f2", "lnst"))
    for n, t in x0_b.items():
        assert (t.float() == 7.0).all(), f"{n} written without pos"


def tail_saved(Nf, dtype):
    """the saved tensors of a float64 forward, rounded as the kernel stores them (f1 16 bit, f2 / lnst fp32), with -0.0 planted in f1 and in the gripper's x"""
    rng = np.random.default_rng(100 + Nf)
    W = tail_weights(dtype)
    xs = tail_x(Nf, dtype)
    saved = []
    for k in range(2):
        c = W[k]
        f1 = R.tail_fc1(xs[k], c["W1"], c["b1"].astype(np.float64))
        f2 = R.tail_fc2(f1, c["W2"], c["b2"].astype(np.float64)).astype(np.float32)
        _, mean, rstd = R.tail_ln(f2.astype(np.float64), c["lng"].astype(np.float64), c["lnb"].astype(np.float64))
        f1 = np.where(rng.random(f1.shape) < 0.05, -0.0, f1)
        xm = np.where(rng.random(xs[k].shape) < 0.05, -0.0, xs[k])
        saved.append(dict(f1=f1, f2=f2, lnst=np.stack([mean, rstd], -1).astype(np.float32), xmask=xm))
    return saved


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("Nf,swap", [(n, False) for n in TAIL_NF] + [(17, True)])
def test_enc_tail_backward(Nf, swap, dtype):
    """d_f2 from demb; d_f1 from the device's d_f2 (zero wherever f1 is +0 or -0); dx from the device's d_f1: fp32 and unmasked for the static camera, 16 bit and
    masked by the fc7 output (again +0 and -0 alike) for the gripper camera.  dlng / dlnb start non-zero and are added to: 2e-5 max|ref| times the Nf rows summed.
    swap: the gripper camera as job 0 and the static one as job 1 — a job's result must not depend on its place in the launch."""
    import ctypes as C
    L, lib = _lib()
    W, saved = tail_weights(dtype), tail_saved(Nf, dtype)
    rng = np.random.default_rng(200 + Nf)
    demb = rng.standard_normal((Nf + GUARD, 128)).astype(np.float32)
    demb_t = f32(demb)
    devs, jobs = [], []
    for k in range(2):
        c, s = W[k], saved[k]
        pre = rng.standard_normal((2, 64)).astype(np.float32) + 3.0
        f1_t = h16(s["f1"], dtype)
        xm_t = h16(s["xmask"], dtype)
        neg0 = 0x8000
        assert (f1_t.view(torch.int16).cpu().numpy().astype(np.uint16) == neg0).mean() > 0.03, "-0.0 must reach the device as a bit pattern"
        dev = dict(f2=f32(s["f2"]), lnst=f32(s["lnst"]), lng=f32(c["lng"]), f1=f1_t, W2t=h16(c["W2"].T, dtype), W1t=h16(c["W1"].T, dtype),
                   xmask=xm_t if k == 1 else None, dlng=f32(pre[0]), dlnb=f32(pre[1]), d_f2=sevens((Nf + GUARD, 64), tdt(dtype)),
                   d_f1=sevens((Nf + GUARD, 512), tdt(dtype)), dx_f32=sevens((Nf + GUARD, 128)) if k == 0 else None,
                   dx_t=sevens((Nf + GUARD, 128), tdt(dtype)) if k == 1 else None, pre=pre)
        devs.append(dev)
        jobs.append(L.HulcEncTailBwdJob(*[ptr(dev[n]) for n in ("f2", "lnst", "lng", "f1", "W2t", "W1t", "xmask", "dlng", "dlnb", "d_f2", "d_f1", "dx_f32", "dx_t")], 64 * k))
    order = (1, 0) if swap else (0, 1)
    L.check(lib.hulc_k_enc_tail_bwd(L.DTYPE[dtype], Nf, 128, C.byref(jobs[order[0]]), C.byref(jobs[order[1]]), demb_t.data_ptr(), None))
    torch.cuda.synchronize()
    for k in range(2):
        c, s, dev = W[k], saved[k], devs[k]
        for n in ("d_f2", "d_f1", "dx_f32", "dx_t"):
            if dev[n] is not None:
                guard_intact(dev[n], Nf, f"camera {k} {n}")
        f2, mean, rstd = s["f2"].astype(np.float64), s["lnst"][:, 0].astype(np.float64), s["lnst"][:, 1].astype(np.float64)
        ref_d2, ref_dg, ref_db = R.tail_ln_bwd(demb[:Nf, 64 * k:64 * k + 64].astype(np.float64), f2, mean, rstd, c["lng"].astype(np.float64))
        d_f2 = f64(dev["d_f2"][:Nf])
        check16(d_f2, ref_d2, dtype, f"camera {k} d_f2")
        check32(f64(dev["dlng"]), dev["pre"][0] + ref_dg, f"camera {k} dlng", scale=Nf)
        check32(f64(dev["dlnb"]), dev["pre"][1] + ref_db, f"camera {k} dlnb", scale=Nf)
        f1 = f64(dev["f1"])
        d_f1 = f64(dev["d_f1"][:Nf])
        assert (d_f1[f1 <= 0] == 0).all(), "d_f1 must be zero where f1 is +0 or -0"
        check16(d_f1, R.tail_fc2_bwd(d_f2, c["W2"], f1), dtype, f"camera {k} d_f1")
        if k == 0:
            check32(f64(dev["dx_f32"][:Nf]), R.tail_fc1_bwd(d_f1, c["W1"]), "static dx_f32")
        else:
            xm = f64(dev["xmask"])
            dx = f64(dev["dx_t"][:Nf])
            assert (dx[xm <= 0] == 0).all(), "dx_t must be zero where the fc7 output is +0 or -0"
            check16(dx, R.tail_fc1_bwd(d_f1, c["W1"], xm), dtype, "gripper dx_t")


def test_enc_tail_entries_validate():
    import ctypes as C
    L, lib = _lib()
    t = sevens((64, 128))
    p = t.data_ptr()
    job = L.HulcEncTailJob(p, p, p, p, p, p, p, p, p, p, 0)
    bad = L.HulcEncTailJob(p, p, p, p, p, p, p, p, None, p, 0)
    far = L.HulcEncTailJob(p, p, p, p, p, p, p, p, p, p, 65)
    args = (p, None, 1, 0.0, 0, None, None, None, None, None)
    assert lib.hulc_k_enc_tail_fwd(1, 0, 128, C.byref(job), C.byref(job), *args) == 1          # Nf < 1
    assert lib.hulc_k_enc_tail_fwd(1, 1, 128, C.byref(job), None, *args) == 1          # one job missing
    assert lib.hulc_k_enc_tail_fwd(1, 1, 128, C.byref(job), C.byref(bad), *args) == 1          # null f2
    assert lib.hulc_k_enc_tail_fwd(1, 1, 128, C.byref(job), C.byref(far), *args) == 1          # col0 + 64 > ldemb
    assert lib.hulc_k_enc_tail_fwd(0, 1, 128, C.byref(job), C.byref(job), *args) == 1          # fp32
    assert lib.hulc_k_enc_tail_fwd(1, 1, 128, C.byref(job), C.byref(job), p, p, 5, 0.1, 0, None, p, p, p, None) == 1          # pos without xf
    bj = L.HulcEncTailBwdJob(p, p, p, p, p, p, None, p, p, p, p, p, None, 0)
    both = L.HulcEncTailBwdJob(p, p, p, p, p, p, None, p, p, p, p, p, p, 0)
    assert lib.hulc_k_enc_tail_bwd(1, 1, 128, C.byref(bj), C.byref(both), p, None) == 1          # dx_f32 and dx_t
    assert lib.hulc_k_enc_tail_bwd(1, 1, 128, C.byref(bj), C.byref(bj), None, None) == 1          # no demb
    assert lib.hulc_k_enc_tail_bwd(2, -3, 128, C.byref(bj), C.byref(bj), p, None) == 1
    assert b"hulc_k_enc_tail_bwd" in lib.hulc_last_error()
    torch.cuda.synchronize()
    assert (t == 7.0).all()
