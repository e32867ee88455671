"""GPU (-m gpu): one encoder stage for BOTH cameras as one launch (conv_reg.h launch_conv_reg_jobs through hulc_k_conv_pair) — conv2 / conv3 forward and
the conv3 / conv2 data gradients in the production ReLU-bitmask forms, and the conv3 / conv2 / conv1 weight gradients (conv_wgrad.h launch_conv_wgrad_pair,
conv1_wgrad.h launch_conv1_wgrad_jobs).  Job A has the static camera's maps (49 -> 23, 23 -> 21; conv1 200 -> 49), job B the gripper camera's (20 -> 9, 9 -> 7; 84 -> 20); the
weights differ per job; frame counts are small, unequal and odd; the workgroup split is given explicitly, and the entry gives every job a zeroed claim counter of
its own, so the weight-gradient kernels (the ones that claim) walk their items by dynamic claiming inside the two-job launch.

Every output (and the ReLU bit words conv2's forward emits) must be bit-identical to two single-job launches of the same entry and within the existing
per-kernel gate max|err| / max|ref| < 6e-3 of the fp64 reference (test_gpu_kernels.py test_conv_reg_fwd / test_conv_reg_dgrad3).  Job B's output lies
directly behind job A's in ONE allocation with a sentinel page between them, everything prefilled with a sentinel.

Weight gradients: each job's dW and db within max|err| / max|ref| < 1e-4 of fp64 (the gate of test_conv_wgrad_tr), and no value of one job's gradient
moves by more than that when the OTHER job's inputs are replaced by zeros (slab assignment differs between runs, so not bitwise).

The engine-level case runs a B=2, S=3 bf16 step: forward tensors identical across two runs, every encoder gradient tensor within the bounds the 512-frame
test holds a bf16 step to (test_gpu_fullsize.py: rel-L2 < 0.2 per tensor, cosine > 0.995) of the fp32 engine's — the reordered backward with the gripper
camera's own gradient buffers."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FWD2, FWD3, DGRAD2, DGRAD3, WGRAD1, WGRAD2, WGRAD3 = 2, 3, 12, 13, 21, 22, 23
# stage -> (CI, KH, S, side of the larger map [static, gripper])
GEO = {FWD2: (32, 4, 2, (49, 20)), FWD3: (64, 3, 1, (23, 9)), DGRAD2: (32, 4, 2, (49, 20)), DGRAD3: (64, 3, 1, (23, 9)), WGRAD2: (32, 4, 2, (49, 20)), WGRAD3: (64, 3, 1, (23, 9)), WGRAD1: (3, 8, 4, (200, 84))}
PAGE = 2048          # sentinel page between the two jobs' outputs: 4 KB of bf16 / 8 KB of bit words
SENT = 7.0


def _lib():
    from hulc_amd import lib as L
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    return L, L.load()


def bf(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda().to(torch.bfloat16).contiguous()


def f64(t):
    return t.float().cpu().numpy().astype(np.float64)


def _fwd_ref(X, W, b, S):
    n, ih, _, _ = X.shape
    co, _, kh, _ = W.shape
    oh = (ih - kh) // S + 1
    out = np.zeros((n, oh, oh, co))
    for a in range(kh):
        for c in range(kh):
            out += np.einsum("nhwc,dc->nhwd", X[:, a:a + S * oh:S, c:c + S * oh:S, :], W[:, :, a, c])
    return np.maximum(out + b, 0)


def _dgrad_ref(dY, W, S, IH):
    n, oh, _, _ = dY.shape
    _, ci, kh, _ = W.shape
    dX = np.zeros((n, IH, IH, ci))
    for a in range(kh):
        for c in range(kh):
            dX[:, a:a + S * oh:S, c:c + S * oh:S, :] += np.einsum("nhwd,dc->nhwc", dY, W[:, :, a, c])
    return dX


@functools.lru_cache(maxsize=None)
def _job(stage, cam, nf):
    """Operands (device) and the fp64 reference of one camera's job; computed once per (stage, camera, frames) and never modified."""
    CI, KH, S, sides = GEO[stage]
    IH = sides[cam]
    OH = (IH - KH) // S + 1
    rng = np.random.default_rng(1000 * stage + 100 * cam + nf)
    fwd = stage in (FWD2, FWD3)
    ramp_axis = (slice(None), None, None, None) if fwd else (None, slice(None), None, None)
    ramp = np.arange(64 if fwd else CI)[ramp_axis] * 0.01
    Wb = f64(bf((rng.standard_normal((64, CI, KH, KH)) + ramp) * 0.1))          # asymmetric in the channel index; differs per job (seed)
    d = dict(IH=IH, OH=OH, nf=nf, CI=CI)
    if fwd:
        d["x"] = bf(rng.standard_normal((nf, IH, IH, CI)))
        b = rng.standard_normal(64).astype(np.float32)
        d["bias"] = torch.from_numpy(b).cuda()
        d["w"] = bf(Wb.transpose(0, 2, 3, 1).reshape(64, -1))
        d["ref"] = _fwd_ref(f64(d["x"]), Wb, b, S)
        d["out_shape"] = (nf, OH, OH, 64)
        d["in_side"], d["out_side"] = IH, OH
    else:
        d["x"] = bf(rng.standard_normal((nf, OH, OH, 64)) * (np.arange(64) % 5 + 1))          # dY
        TA = KH // S
        wd = np.zeros((S * S, CI, TA, TA, 64))
        for kh in range(KH):
            for kw in range(KH):
                wd[(kh % S) * S + kw % S, :, kh // S, kw // S, :] = Wb[:, :, kh, kw].T
        d["w"] = bf(wd.reshape(S * S * CI, -1))
        maskv = rng.standard_normal((nf, IH, IH, CI))
        bits = (maskv > 0).reshape(nf, IH, IH, CI // 32, 32).astype(np.int64)                     # bit c%32 of word c/32 = (channel c > 0)
        words = (bits << np.arange(32)).sum(-1).astype(np.uint32).view(np.int32)
        d["maskbits"] = torch.from_numpy(np.ascontiguousarray(words)).cuda()
        d["bias"] = None
        d["ref"] = _dgrad_ref(f64(d["x"]), Wb, S, IH) * (maskv > 0)
        d["out_shape"] = (nf, IH, IH, CI)
        d["in_side"], d["out_side"] = OH, IH
    return d


def _cjob(L, d, out, bits):
    j = L.HulcConvJob()
    j.input = d["x"].data_ptr(); j.w = d["w"].data_ptr(); j.bias = d["bias"].data_ptr() if d["bias"] is not None else None
    j.out = out.data_ptr(); j.bits = bits.data_ptr() if bits is not None else None
    j.frames, j.in_side, j.out_side = d["nf"], d["in_side"], d["out_side"]
    return j


def _views(flat, shapes):
    """[A | sentinel page | B] views of one allocation."""
    na = int(np.prod(shapes[0]))
    nb = int(np.prod(shapes[1]))
    return flat[:na].view(shapes[0]), flat[na:na + PAGE], flat[na + PAGE:na + PAGE + nb].view(shapes[1])


@pytest.mark.parametrize("wgs", [(3, 2), (1, 1)])
@pytest.mark.parametrize("frames", [(7, 5), (1, 3), (3, 1)])
@pytest.mark.parametrize("stage", [FWD2, FWD3, DGRAD3, DGRAD2])
def test_two_camera_launch_equals_two_single_launches_and_fp64(stage, frames, wgs):
    L, lib = _lib()
    jobs = [_job(stage, 0, frames[0]), _job(stage, 1, frames[1])]
    shapes = [j["out_shape"] for j in jobs]
    total = sum(int(np.prod(s)) for s in shapes) + PAGE
    emits_bits = stage == FWD2                     # conv2's forward also writes the ReLU bit words of its output (2 per pixel)
    bshapes = [s[:3] + (2,) for s in shapes]
    btotal = sum(int(np.prod(s)) for s in bshapes) + PAGE

    def buffers():
        flat = torch.full((total,), SENT, device="cuda", dtype=torch.bfloat16)      # every output must be overwritten, nothing else
        bflat = torch.full((btotal,), -1, device="cuda", dtype=torch.int32) if emits_bits else None
        return flat, bflat

    def io(k, flat, bflat):
        o = _views(flat, shapes)[0 if k == 0 else 2]
        if emits_bits:
            return o, _views(bflat, bshapes)[0 if k == 0 else 2]
        return o, (jobs[k]["maskbits"] if stage in (DGRAD2, DGRAD3) else None)

    flat, bflat = buffers()
    ja, jb = (_cjob(L, jobs[k], *io(k, flat, bflat)) for k in range(2))
    L.check(lib.hulc_k_conv_pair(stage, C.byref(ja), C.byref(jb), wgs[0], wgs[1], None))
    torch.cuda.synchronize()
    # the same two jobs as single-job launches of the same entry, each on the workgroups it had in the pair
    sflat, sbflat = buffers()
    for k in range(2):
        js = _cjob(L, jobs[k], *io(k, sflat, sbflat))
        L.check(lib.hulc_k_conv_pair(stage, C.byref(js), None, wgs[k], 0, None))
    torch.cuda.synchronize()
    assert torch.equal(flat.view(torch.int16), sflat.view(torch.int16))              # outputs and the sentinel page, bit for bit
    outs = _views(flat, shapes)
    assert bool((outs[1] == SENT).all()), "a job wrote into the page between the two outputs"
    for k, o in ((0, outs[0]), (1, outs[2])):
        ref = jobs[k]["ref"]
        err = np.abs(f64(o) - ref).reshape(ref.shape[0], -1).max(1) / np.abs(ref).max()
        print(f"[camera merge stage {stage} frames {frames} wgs {wgs}] job {'AB'[k]} worst frame error {err.max():.2e}")
        assert err.max() < 6e-3, (k, err.max(), int(err.argmax()))                  # bf16 output rounding; a pixel left at the sentinel is an O(1) error
    if emits_bits:
        assert torch.equal(bflat, sbflat)
        bv = _views(bflat, bshapes)
        assert bool((bv[1] == -1).all())
        sh = torch.arange(32, device="cuda")
        for o, w in ((outs[0], bv[0]), (outs[2], bv[2])):
            got = (((w.to(torch.int64) & 0xFFFFFFFF)[..., None] >> sh) & 1).reshape(o.shape).bool()
            assert torch.equal(got, o > 0)


def _wgrad_ref(X, dY, KH, S):
    n, oh, _, co = dY.shape
    out = np.zeros((co, KH, KH, X.shape[3]))
    for kh in range(KH):
        for kw in range(KH):
            out[:, kh, kw, :] = np.einsum("nhwc,nhwd->cd", dY, X[:, kh:kh + S * oh:S, kw:kw + S * oh:S, :])
    return out.reshape(co, -1)


@functools.lru_cache(maxsize=None)
def _wjob(stage, cam, nf):
    CI, KH, S, sides = GEO[stage]
    IH = sides[cam]
    OH = (IH - KH) // S + 1
    rng = np.random.default_rng(2000 * stage + 100 * cam + nf)
    if stage == WGRAD1:      # conv1: fp32 NCHW frames (the kernel rounds them to bf16), 32 output channels, dW in (c, kh, kw) order
        X = torch.from_numpy(rng.standard_normal((nf, 3, IH, IH)).astype(np.float32)).cuda()
        dY = bf(rng.standard_normal((nf, OH, OH, 32)) * (np.arange(32) % 5 + 1))
        ref = _wgrad_ref(f64(X.to(torch.bfloat16)).transpose(0, 2, 3, 1), f64(dY), KH, S).reshape(32, KH, KH, 3).transpose(0, 3, 1, 2).reshape(32, -1)
        return dict(X=X, dY=dY, nf=nf, IH=IH, OH=OH, K=192, CO=32, ref=ref, bref=f64(dY).sum((0, 1, 2)))
    X = bf(rng.standard_normal((nf, IH, IH, CI)))
    dY = bf(rng.standard_normal((nf, OH, OH, 64)) * (np.arange(64) % 5 + 1))
    return dict(X=X, dY=dY, nf=nf, IH=IH, OH=OH, K=KH * KH * CI, CO=64, ref=_wgrad_ref(f64(X), f64(dY), KH, S), bref=f64(dY).sum((0, 1, 2)))


@pytest.mark.parametrize("wgs", [(3, 2), (1, 1)])
@pytest.mark.parametrize("frames", [(7, 5), (1, 3), (3, 1)])
@pytest.mark.parametrize("stage", [WGRAD3, WGRAD2, WGRAD1])
def test_two_camera_weight_gradient_against_fp64_and_independent_of_the_other_job(stage, frames, wgs):
    L, lib = _lib()
    jobs = [_wjob(stage, 0, frames[0]), _wjob(stage, 1, frames[1])]

    def run(zero=None):
        outs = []
        cj = []
        for k, d in enumerate(jobs):
            X, dY = (torch.zeros_like(d["X"]), torch.zeros_like(d["dY"])) if zero == k else (d["X"], d["dY"])
            dw = torch.full((d["CO"], d["K"]), SENT, device="cuda")                     # overwritten by the entry
            db = torch.full((d["CO"],), SENT, device="cuda")
            j = L.HulcConvJob()
            j.input = X.data_ptr(); j.w = dY.data_ptr(); j.bias = None; j.out = dw.data_ptr(); j.bits = db.data_ptr()
            j.frames, j.in_side, j.out_side = d["nf"], d["IH"], d["OH"]
            cj.append(j); outs.append((dw, db, X, dY))
        L.check(lib.hulc_k_conv_pair(stage, C.byref(cj[0]), C.byref(cj[1]), wgs[0], wgs[1], None))
        torch.cuda.synchronize()
        return [(f64(dw), f64(db)) for dw, db, _, _ in outs]

    full = run()
    for k, d in enumerate(jobs):
        dw, db = full[k]
        e_w = np.abs(dw - d["ref"]).max() / np.abs(d["ref"]).max()
        e_b = np.abs(db - d["bref"]).max() / np.abs(d["bref"]).max()
        print(f"[camera merge wgrad stage {stage} frames {frames} wgs {wgs}] job {'AB'[k]} dW {e_w:.2e} db {e_b:.2e}")
        assert e_w < 1e-4, (k, e_w)
        assert e_b < 1e-4, (k, e_b)
    for other in (0, 1):                                   # the OTHER job's inputs as zeros: this job's gradient stays, the zeroed job's is zero
        k = 1 - other
        part = run(zero=other)
        assert np.abs(part[k][0] - full[k][0]).max() / np.abs(jobs[k]["ref"]).max() < 1e-4, (stage, frames, wgs, k)
        assert np.abs(part[k][1] - full[k][1]).max() / np.abs(jobs[k]["bref"]).max() < 1e-4, (stage, frames, wgs, k)
        assert not part[other][0].any() and not part[other][1].any()


ENC_FWD = (("emb", 128), ("s_a1", 49 * 49 * 32), ("s_a2", 23 * 23 * 64), ("s_a3", 21 * 21 * 64), ("g_a1", 20 * 20 * 32), ("g_a2", 9 * 9 * 64), ("g_a3", 7 * 7 * 64))


def test_bf16_step_is_repeatable_and_its_encoder_gradients_follow_the_fp32_engine():
    from hulc_amd import spec
    from hulc_amd.engine import StepEngine
    from hulc_amd.utils import synthetic
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    Bt, St = 2, 3
    dims = spec.ModelDims(kind="hulc", max_window=32, use_clip=False)
    P = spec.init_all(dims, seed=21, ln_jitter=True)
    mb = synthetic.make_batch(Bt, 0, St, seed=21, edge_frac=0.05, aux_mask="all")["vis"]
    mb["plan_idx"] = np.random.default_rng(5).integers(0, 32, (Bt, 32)).astype(np.int32)          # injected categorical sample: both engines take the same plan
    dev_mb = {k: torch.from_numpy(v.astype(np.int32) if k == "plan_idx" else v).cuda() for k, v in mb.items()}
    res = {}
    for dtype in ("fp32", "bf16"):
        eng = StepEngine(dims, Bt, St, dtype=dtype, device="cuda:0", dropout_p=0.0, seed=3)
        eng.load_numpy(P)
        runs = []
        for _ in range(2 if dtype == "bf16" else 1):
            eng.zero_grads()
            eng.forward_loss(dev_mb, False, 1.0, 3.0, step=0)
            eng.backward()
            torch.cuda.synchronize()
            fwd = {n: eng.get_tensor(n, Bt * St * k).copy() for n, k in ENC_FWD}
            runs.append((fwd, {n: t.detach().cpu().numpy().astype(np.float64) for n, t in eng.views(eng.flat_grads).items() if n.startswith("perceptual_encoder.")}))
        eng.close()
        res[dtype] = runs
    (f0, g0), (f1, g1) = res["bf16"]
    for n, k in ENC_FWD:
        assert f0[n].size == Bt * St * k and np.abs(f0[n]).max() > 0, n
        assert np.array_equal(f0[n], f1[n]), n                                      # the forward is deterministic: the same bits in both runs
    gref = res["fp32"][0][1]
    assert len(gref) >= 20
    # the static encoder's conv3 bias gradient cancels exactly per (frame, channel) (softmax Jacobian): rounding noise in either engine (test_gpu_fullsize.py)
    cancels = "perceptual_encoder.rgb_static_encoder.conv_model.4.bias"
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    for g in (g0, g1):
        errs = sorted(((rel(g[n], gref[n]), n) for n in gref if n != cancels and np.linalg.norm(gref[n]) > 1e-6), reverse=True)
        print("[camera merge, B=2 S=3 bf16 vs fp32] worst encoder gradient tensors:", [(round(e, 4), n.split("perceptual_encoder.")[1]) for e, n in errs[:6]])
        assert errs[0][0] < 2e-1, errs[:4]
        a = np.concatenate([g[n].reshape(-1) for n in gref if n != cancels])
        b = np.concatenate([gref[n].reshape(-1) for n in gref if n != cancels])
        assert float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b))) > 0.995


def test_conv1_weight_gradient_entry_form_does_not_reach_the_engines_routing():
    """The uint8 form of conv1's weight gradient is an argument of the launcher (conv1_wgrad.h conv1_wgrad_plan), not library state: a bf16 engine's backward at
    B = 2, S = 2 from uint8 frames in reproducible mode, then hulc_k_conv1_wgrad_u8 with form = 1 on 3 frames of 84 x 84, then the same backward again — the conv1
    weight and bias gradients of both cameras must have the same bits before and after the entry ran the other form."""
    from bench import synth_batch
    from hulc_amd import spec
    from hulc_amd.engine import StepEngine
    L, lib = _lib()
    Bt, St = 2, 2
    dims = spec.ModelDims(kind="hulc", max_window=32, use_clip=False)
    eng = StepEngine(dims, Bt, St, dtype="bf16", device="cuda:0", dropout_p=0.0, seed=3)
    eng.load_numpy(spec.init_all(dims, seed=21, ln_jitter=True))
    eng.set_option("reproducible", 1)
    mb = synth_batch(Bt, St, torch.device("cuda:0"), 11, False, "u8")

    def conv1_grads():
        eng.zero_grads()
        eng.forward_loss(mb, False, 1.0, 3.0, step=0)
        eng.backward()
        torch.cuda.synchronize()
        return {n: t.detach().cpu().numpy().copy() for n, t in eng.views(eng.flat_grads).items() if n.startswith("perceptual_encoder.") and ".conv_model.0." in n}

    before = conv1_grads()
    assert len(before) == 4 and all(np.abs(g).max() > 0 for g in before.values()), sorted(before)
    Nf, IH, pad = 3, 84, 4
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randint(0, 256, (Nf, IH, IH, 3), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
    sh = torch.randint(0, 2 * pad + 1, (Nf, 2), device="cuda", generator=g, dtype=torch.int32)
    dY = torch.randn(Nf, 20, 20, 32, device="cuda", generator=g).to(torch.bfloat16)
    gw = torch.zeros(32, 192, device="cuda"); gb = torch.zeros(32, device="cuda")
    L.check(lib.hulc_k_conv1_wgrad_u8(x.data_ptr(), sh.data_ptr(), pad, dY.data_ptr(), gw.data_ptr(), gb.data_ptr(), Nf, IH, 1, 1, None))
    torch.cuda.synchronize()
    assert float(gw.abs().max()) > 0
    after = conv1_grads()
    eng.close()
    for n in before:
        assert np.array_equal(before[n].view(np.uint32), after[n].view(np.uint32)), n
