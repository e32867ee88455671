"""GPU (-m gpu): the BC-Z and MIA language auxiliary losses on the engine (csrc/aux_heads.h, hulc_aux_*), against the fixtures of the unmodified reference
(tools/gen_golden_aux.py) and against torch restatements written here.  Gates are the project's own: fp32 loss 1e-3 of the reference and every gradient
tensor 1e-3 rel-L2 of its float64 gradients (5e-3 for the conv sums) as test_gpu_parity.py; 16-bit loss 5e-3 and gradient cosine > 0.99 as test_gpu_shapes.py;
the paired pass 2e-5 as test_paired_pass_equals_two_modality_passes."""
import ctypes as C
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from aux_golden_util import AUX_CASES, BL, BV, S, case_batch, load_aux_case  # noqa: E402
from golden_util import adam_close, check_grads64, grad_entries, load_case, rel_l2, sample_idx  # noqa: E402
from hulc_amd import spec  # noqa: E402

CLIP_BETA = 3.0
HEADS = ("bc_z_lang_decoder.", "mia_lang_discriminator.", "proj_vis_lang.")


def _engine(dims, B, S_, dtype, **kw):
    from hulc_amd.engine import StepEngine
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible — the product path has no CPU fallback")
    return StepEngine(dims, B, S_, dtype=dtype, dropout_p=0.0, **kw)


def to_dev(mb):
    out = {}
    for k, v in mb.items():
        if k == "use_for_aux":
            out["aux_rows"] = np.nonzero(v)[0].astype(np.int32)
        elif k == "plan_idx":
            out[k] = torch.from_numpy(v.astype(np.int32)).cuda()
        else:
            out[k] = torch.from_numpy(v).cuda()
    return out


def total_of(dims, per, nmod, bcz_beta=1.0, mia_beta=1.0):
    """train/total_loss as the reference adds it up (hulc.py:491-537): modality means, then the auxiliary losses times their betas."""
    tot = sum(l["total_mod"] for l in per.values()) / nmod
    for l in per.values():
        tot += (CLIP_BETA * l["clip"] if dims.use_clip else 0.0) + bcz_beta * l.get("bc_z", 0.0) + mia_beta * l.get("mia", 0.0)
    return tot


def run_step(eng, batch, step=0):
    eng.zero_grads()
    per = {}
    for sc, mb in batch.items():
        per[sc] = eng.forward_loss(to_dev(mb), "lang" in sc, 1.0 / len(batch), CLIP_BETA, step=step)
        eng.backward()
    return total_of(eng.dims, per, len(batch)), per


def grads_np(eng):
    return {n: t.detach().cpu().numpy() for n, t in eng.views(eng.flat_grads).items()}


def check_logged(dims, per, fx, tol):
    l = per["lang"]
    for key, got in (("log/train/pred_lang", l.get("bc_z")), ("log/train/lang_contrastive", l.get("mia"))):
        if key in fx.files:
            ref = float(fx[key])
            print(f"   {key}: engine {got:.6f} reference {ref:.6f}")
            assert abs(got - ref) <= tol * abs(ref), (key, got, ref)          # a reference value of 0 (no flagged row) must be met exactly
    if dims.use_clip:
        assert abs(CLIP_BETA * l["clip"] - float(fx["log/train/lang_clip_loss"])) <= tol * abs(float(fx["log/train/lang_clip_loss"]))


# ---------------------------------------------------------------------------------------------------------------- fixture parity, fp32
@pytest.mark.parametrize("name", list(AUX_CASES))
def test_fp32_step_matches_the_reference(name):
    dims, P, batch, fx = load_aux_case(name)
    eng = _engine(dims, BL, S, "fp32")
    eng.load_numpy(P)
    tot, per = run_step(eng, batch)
    ref = float(fx["loss_total"])
    print(f"[{name}] total: engine {tot:.6f} reference {ref:.6f}")
    assert abs(tot - ref) <= 1e-3 * abs(ref), (tot, ref)
    check_logged(dims, per, fx, 1e-3)
    assert per["lang"]["aux_rows"] == int(batch["lang"]["use_for_aux"].sum())
    Gg = grads_np(eng)
    w64, wn64 = check_grads64(Gg, fx, label=name)          # every tensor, heads included: 1e-3 (5e-3 for the conv sums) against the float64 reference
    print(f"[{name}] grads vs fp64 reference: worst {w64[0]:.2e} ({w64[1]}) conv sums {wn64[0]:.2e} ({wn64[1]})")
    for key in fx.files:
        if key.startswith("gradnone/"):
            assert not np.any(Gg[key[len("gradnone/"):]])
    if not batch["lang"]["use_for_aux"].any():               # no flagged row: nothing launched, loss slots 0, head gradients exactly zero (the reference's are zero tensors)
        assert per["lang"]["mia"] == 0.0 and per["lang"]["bc_z"] == 0.0 and per["lang"]["clip"] == 0.0
        for n in Gg:
            if n.startswith(HEADS) or n == "logit_scale":
                assert not np.any(Gg[n]), n
                assert "gradnorm/" + n in fx.files and float(fx["gradnorm/" + n]) == 0.0, n
    eng.adam_step()
    pv = eng.views(eng.flat_params)
    for key in fx.files:
        if key.startswith("adam1/"):
            n = key[len("adam1/"):]
            flat = pv[n].detach().cpu().numpy().reshape(-1)
            got = flat if flat.size <= 4096 else flat[sample_idx(n, flat.size)]
            assert adam_close(got, fx[key], grad_entries(fx, n)), n
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- fixture parity, 16-bit engines
def _head_cosine(Gg, fx, scale):
    a, b = [], []
    for key in fx.files:
        if key.startswith("gradnorm64/") and key[len("gradnorm64/"):].startswith(HEADS):
            n = key[len("gradnorm64/"):]
            g = Gg[n].reshape(-1).astype(np.float64) / scale
            if "grad64/" + n in fx.files:
                a.append(g); b.append(fx["grad64/" + n].reshape(-1).astype(np.float64))
            else:
                a.append(g[sample_idx(n, g.size)]); b.append(fx["gradsamp64/" + n].astype(np.float64))
    a, b = np.concatenate(a), np.concatenate(b)
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["aux_mia_hulc", "aux_all_hulc"])
def test_16bit_step_close_to_the_reference(name, dtype):
    """The 16-bit gates of test_gpu_shapes.py: the step's loss within 5e-3 of the reference, the head tensors' gradients at cosine > 0.99 against the
    float64 reference.  fp16: the gradient buffer holds gradients x the loss scale, which must cancel.  The fixtures' scaled heads have gradients of norm
    10 - 30 whose fp16 intermediates overflow at GradScaler's initial 65536 — what the scaler answers with skipped steps and a smaller scale; the test
    starts at the scale 256 it would settle near.  The two auxiliary slots are printed next to the reference's values.  The image gain of the fixtures is
    a cancellation that 16-bit operands resolve to their mantissa only (aux_golden_util.SCALES): the cases use the smallest gain that keeps the
    generator's assertions."""
    dims, P, batch, fx = load_aux_case(name)
    eng = _engine(dims, BL, S, dtype)
    if dtype == "fp16":
        eng.scaler_enable(init_scale=256.0)
    eng.load_numpy(P)
    tot, per = run_step(eng, batch)
    eng.flush_grads()
    ref = float(fx["loss_total"])
    scale = eng.scaler_state()["scale"] if dtype == "fp16" else 1.0
    Gg = grads_np(eng)
    cos = _head_cosine(Gg, fx, scale)
    print(f"[{name} {dtype}] total: engine {tot:.6f} reference {ref:.6f}; head-gradient cosine {cos:.5f}; loss scale {scale}")
    for key, k in (("log/train/pred_lang", "bc_z"), ("log/train/lang_contrastive", "mia")):
        if key in fx.files:
            print(f"   {key}: engine {per['lang'][k]:.6f} reference {float(fx[key]):.6f}")
    for n in Gg:
        if n.startswith(HEADS) and "gradnorm64/" + n in fx.files:
            r = np.linalg.norm(Gg[n].astype(np.float64)) / scale / float(fx["gradnorm64/" + n])
            print(f"   {n}: |g| / |g_ref| = {r:.4f}")
    assert abs(tot - ref) <= 5e-3 * abs(ref), (tot, ref)
    if dtype == "fp16":
        assert scale == 256.0
    assert cos > 0.99, cos
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- torch restatements
def _t(P, n):
    return torch.from_numpy(np.asarray(P[n], np.float64)).requires_grad_(True)


def _lin(x, W, b):
    return x @ W.T + b


def bcz_restated(P, sf, lang):
    """mean(1 - cos(mlp(seq_feat[rows]), lang[rows])), plain quotient; returns loss, {head name: tensor}, the seq_feat leaf."""
    names = [f"bc_z_lang_decoder.mlp.{i}.{k}" for i in (0, 2) for k in ("weight", "bias")]
    T = {n: _t(P, n) for n in names}
    sf = torch.from_numpy(sf.astype(np.float64)).requires_grad_(True)
    tg = torch.from_numpy(lang.astype(np.float64))
    pred = _lin(torch.relu(_lin(sf, T[names[0]], T[names[1]])), T[names[2]], T[names[3]])
    cos = (pred * tg).sum(-1) / (torch.linalg.norm(pred, dim=1) * torch.linalg.norm(tg, dim=1))
    return (1 - cos).mean(), T, sf


def mia_restated(P, sf, goal, shift=1):
    """BCE with logits over D([img | txt]) (label 1) and D([img | roll(txt, shift)]) (label 0); returns loss, {name: tensor}, the seq_feat and goal leaves."""
    names = [f"proj_vis_lang.{m}.{i}.{k}" for m in ("mlp_im", "mlp_lang") for i in (0, 2) for k in ("weight", "bias")]
    names += [f"mia_lang_discriminator.mlp.{i}.{k}" for i in (0, 3) for k in ("weight", "bias")]
    T = {n: _t(P, n) for n in names}
    sf = torch.from_numpy(sf.astype(np.float64)).requires_grad_(True)
    g = torch.from_numpy(goal.astype(np.float64)).requires_grad_(True)
    mlp = lambda x, p, a, b: _lin(torch.relu(_lin(x, T[f"{p}.{a}.weight"], T[f"{p}.{a}.bias"])), T[f"{p}.{b}.weight"], T[f"{p}.{b}.bias"])
    img, txt = mlp(sf, "proj_vis_lang.mlp_im", 0, 2), mlp(g, "proj_vis_lang.mlp_lang", 0, 2)
    D = lambda a, b: mlp(torch.cat([a, b], -1), "mia_lang_discriminator.mlp", 0, 3)
    neg = txt if shift == 0 else torch.roll(txt, shifts=shift, dims=0)
    z = torch.cat([D(img, txt), D(img, neg)], 0)
    y = torch.cat([torch.ones(len(sf), 1), torch.zeros(len(sf), 1)], 0).double()
    return torch.nn.functional.binary_cross_entropy_with_logits(z, y), T, sf, g


def _lang_only_runs(eng, mb, weights):
    """One lang batch, the same plan sample, one run per (bc_z weight, mia weight): returns [(losses, grads)]."""
    out = []
    for wb, wm in weights:
        eng.set_aux_weights(wb, wm)
        eng.zero_grads()
        l = eng.forward_loss(mb, True, 1.0, CLIP_BETA, step=0)
        eng.backward()
        out.append((l, grads_np(eng)))
    return out


def _upstream_gate(name, d, ref, noise):
    gate = max(1e-4 * np.linalg.norm(ref), 10.0 * noise)
    err = np.linalg.norm(d - ref)
    print(f"   {name}: |d - ref| {err:.3e}  |ref| {np.linalg.norm(ref):.3e}  run-to-run noise of two weight-0 runs {noise:.3e}  gate {gate:.3e}")
    assert np.linalg.norm(ref) > 0, name
    assert err <= gate, (name, err, gate)


def test_bcz_partial_mask_matches_torch_where_the_reference_raises():
    """Mask [F,T,T,T]: the reference's BC-Z indexes seq_feat by the mask twice and raises; the engine selects the rows once.  Loss slot, head gradients and
    the gradient that flows back into seq_feat (read off plan_recognition.fc.bias = sum_rows dL/dseq_feat) against torch autograd on the engine's own
    seq_feat.  The upstream gate's second term is the run-to-run noise of the fp32 engine's atomics, measured here between two weight-0 runs."""
    c = dict(AUX_CASES["aux_bcz_hulc"], mask="some", seed=7)
    dims = spec.ModelDims(kind="hulc", use_clip=True, use_bc_z=True)
    P = spec.init_all(dims, seed=c["seed"], ln_jitter=True)
    lang = case_batch(c)["lang"]
    rows = np.nonzero(lang["use_for_aux"])[0]
    assert list(lang["use_for_aux"]) == [False, True, True, True]
    eng = _engine(dims, BL, S, "fp32")
    eng.load_numpy(P)
    mb = to_dev(lang)
    (l0, g0), (l0b, g0b), (l1, g1) = _lang_only_runs(eng, mb, [(0.0, 1.0), (0.0, 1.0), (1.0, 1.0)])
    sf = eng.get_tensor("seq_feat", BL * 4096).reshape(BL, 4096)[rows]
    loss, T, sfl = bcz_restated(P, sf, lang["lang"][rows])
    loss.backward()
    print(f"[bcz partial] loss slot {l1['bc_z']:.7f} torch {float(loss):.7f}")
    assert abs(l1["bc_z"] - float(loss)) <= 1e-5 and l0["bc_z"] == l1["bc_z"] and l1["aux_rows"] == 3
    for n, t in T.items():
        e = rel_l2(g1[n], t.grad.numpy())
        print(f"   {n}: rel-L2 {e:.2e}")
        assert e <= 1e-4, (n, e)
        assert not np.any(g0[n]), n                                      # weight 0: the head's gradients are zeros
    key = "plan_recognition.fc.bias"
    _upstream_gate(key, (g1[key] - g0[key]).astype(np.float64), sfl.grad.numpy().sum(0), float(np.linalg.norm(g0b[key].astype(np.float64) - g0[key])))
    eng.close()


@pytest.mark.parametrize("name,n_rows", [("aux_mia_noclip_gcbc", 3), ("aux_mia_hulc", 3), ("aux_mia_noclip_gcbc", 1)])
def test_mia_matches_torch_roll_direction_and_one_row(name, n_rows):
    """The fixtures' scaled parameters on a lang-only batch, MIA weight 0 against weight 1.  The engine's loss is the roll(+1) restatement's and misses
    roll(-1) by more than 10x the gate; the discriminator's and the projection's gradients against autograd; the upstream gradients through
    plan_recognition.fc.bias (= sum_rows dL/dseq_feat) and language_goal.ln.bias (= sum_rows dL/dgoal).  Without the CLIP loss the weight-0 run leaves all of
    these at zero; with it (aux_mia_hulc: the MIA kernel ADDS to the CLIP kernel's dimg / dtxt) the difference of the two runs is the MIA share and is gated
    like the upstream gradients.  n_rows = 1: the roll is the identity, the same pair is scored with label 1 and label 0."""
    dims, P, batch, fx = load_aux_case(name)
    lang = dict(batch["lang"])
    if n_rows == 1:
        lang["use_for_aux"] = np.array([False, False, True, False])
    rows = np.nonzero(lang["use_for_aux"])[0]
    assert len(rows) == n_rows
    eng = _engine(dims, BL, S, "fp32")
    eng.load_numpy(P)
    mb = to_dev(lang)
    (l0, g0), (l0b, g0b), (l1, g1) = _lang_only_runs(eng, mb, [(1.0, 0.0), (1.0, 0.0), (1.0, 1.0)])
    sf = eng.get_tensor("seq_feat", BL * 4096).reshape(BL, 4096)[rows]
    goal = eng.get_tensor("goal", BL * 32).reshape(BL, 32)[rows]
    loss, T, sfl, gl = mia_restated(P, sf, goal, 1)
    loss.backward()
    got, ref = l1["mia"], float(loss)
    gate = 1e-3 * abs(ref)
    print(f"[mia {name} n={n_rows}] loss slot {got:.7f} torch roll(+1) {ref:.7f}")
    assert abs(got - ref) <= 1e-5 * max(1.0, abs(ref)) and l0["mia"] == l1["mia"] and l1["aux_rows"] == n_rows
    if n_rows == 3:
        minus = float(mia_restated(P, sf, goal, -1)[0])
        print(f"   roll(-1) {minus:.7f}: engine misses it by {abs(got - minus):.3e} (gate {gate:.3e}); fixture meta roll(+1) {float(fx['meta/mia_roll_plus']):.7f} "
              f"roll(-1) {float(fx['meta/mia_roll_minus']):.7f} no roll {float(fx['meta/mia_no_roll']):.7f}")
        assert abs(got - minus) > 10 * gate
        assert abs(got - float(fx["log/train/lang_contrastive"])) <= gate
    else:
        assert abs(ref - math.log(2.0)) > 1e-3          # not the degenerate value either
    noise = lambda n: float(np.linalg.norm(g0b[n].astype(np.float64) - g0[n]))
    for n, t in T.items():
        d = (g1[n] - g0[n]).astype(np.float64)
        if n.startswith("mia_lang_discriminator.") or not dims.use_clip:
            e = rel_l2(d, t.grad.numpy())
            print(f"   {n}: rel-L2 {e:.2e}")
            assert e <= 1e-4, (n, e)
            assert not np.any(g0[n]), n                                  # weight 0: zeros
        else:
            _upstream_gate(n, d.reshape(-1), t.grad.numpy().reshape(-1), noise(n))
    for key, ref_up in (("plan_recognition.fc.bias", sfl.grad.numpy().sum(0)), ("language_goal.ln.bias", gl.grad.numpy().sum(0))):
        _upstream_gate(key, (g1[key] - g0[key]).astype(np.float64), ref_up, noise(key))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- paired pass
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_paired_pass_equals_two_modality_passes_with_heads(dtype):
    """hulc_forward_loss_pair with both heads: the aux rows land on the lang half (row indices + Bv, lang rows numbered from Bv)."""
    dims, P, batch0, fx = load_aux_case("aux_all_hulc")
    lang = dict(batch0["lang"])
    lang["use_for_aux"] = np.array([True, False, True, True])
    vis = case_batch(dict(AUX_CASES["aux_all_hulc"]))["vis"]
    # equal window counts: the vis half is the lang windows' frames under the vis modality's plan sample
    vis4 = {k: np.concatenate([vis[k], vis[k]], 0) for k in vis}
    batch = {"vis": vis4, "lang": lang}
    eng = _engine(dims, 2 * BL, S, dtype)
    eng.load_numpy(P)
    tot1, per1 = run_step(eng, batch)
    eng.flush_grads()
    g1 = grads_np(eng)
    eng.zero_grads()
    pv, pl = eng.forward_loss_pair(to_dev(batch["vis"]), to_dev(batch["lang"]), 0.5, CLIP_BETA, step=0)
    eng.backward()
    eng.flush_grads()
    g2 = grads_np(eng)
    tol = 2e-5 if dtype == "fp32" else 5e-3
    for k in ("total_mod", "kl", "action"):
        assert abs(pv[k] - per1["vis"][k]) <= tol * max(1.0, abs(per1["vis"][k])), (k, pv[k], per1["vis"][k])
    for k in ("total_mod", "kl", "action", "clip", "bc_z", "mia"):
        print(f"   [{dtype}] lang {k}: pair {pl[k]:.6f} single {per1['lang'][k]:.6f}")
        assert abs(pl[k] - per1["lang"][k]) <= tol * max(1.0, abs(per1["lang"][k])), (k, pl[k], per1["lang"][k])
    assert pl["aux_rows"] == 3 and "mia" not in pv
    if dtype == "fp32":
        errs = {n: rel_l2(g2[n], g1[n]) for n in g1 if np.linalg.norm(g1[n]) > 1e-6}
        worst = max((e, n) for n, e in errs.items())
        print(f"   paired vs single gradients: worst {worst[0]:.2e} ({worst[1]})")
        assert worst[0] <= 2e-5, worst
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- heads off, error paths, buckets
def test_heads_off_is_the_parent_step_and_the_error_paths():
    from hulc_amd import lib as L
    dims, P, batch, fx = load_case("hulc_tiny")
    eng = _engine(dims, 2, 4, "fp32")
    eng.load_numpy(P)
    assert not eng.aux_heads

    def step():
        eng.zero_grads()
        per = {}
        for sc, mb in batch.items():
            per[sc] = eng.forward_loss(to_dev(mb), "lang" in sc, 0.5, CLIP_BETA, step=0)
            eng.backward()
        return per, grads_np(eng)

    per_a, g_a = step()
    assert "mia" not in per_a["lang"]
    assert eng.aux_losses() == dict(bc_z=0.0, mia=0.0, aux_rows=0)          # heads off: zeros, documented in include/hulc_hip.h
    per_b, g_b = step()
    # the lang modality's forward is deterministic in the fp32 engine: a context that never enables the heads computes what it computed before, bit for bit
    tot = sum(l["total_mod"] for l in per_a.values()) / 2 + CLIP_BETA * per_a["lang"]["clip"]
    assert abs(tot - float(fx["loss_total"])) <= 1e-3 * abs(float(fx["loss_total"]))
    for sc in per_a:
        assert per_a[sc] == per_b[sc]
    for n in ("proj_vis_lang.mlp_im.0.weight", "proj_vis_lang.mlp_lang.2.weight", "logit_scale", "action_decoder.mean_fc.weight"):
        assert np.array_equal(g_a[n], g_b[n]), n
    check_grads64(g_a, fx, label="heads off")
    # enable after bind
    with pytest.raises(RuntimeError, match="after hulc_bind_params"):
        L.check(eng.lib.hulc_aux_heads_enable(eng.ctx, 1, 1))
    eng.close()
    # enable on mcil
    m = _engine(spec.ModelDims(kind="mcil", use_clip=False), 2, 4, "fp32")
    with pytest.raises(RuntimeError, match="MCIL"):
        L.check(m.lib.hulc_aux_heads_enable(m.ctx, 0, 1))
    m.close()
    # heads enabled, nothing run yet: zeros; a table without the head tensors does not bind
    d2 = spec.ModelDims(kind="hulc", use_clip=True, use_mia=True)
    e2 = _engine(d2, 2, 4, "fp32")
    assert e2.aux_losses() == dict(bc_z=0.0, mia=0.0, aux_rows=0)
    e2.close()
    e3 = _engine(spec.ModelDims(kind="hulc", use_clip=True), 2, 4, "fp32")
    L.check(e3.lib.hulc_aux_heads_enable(e3.ctx, 1, 0))
    with pytest.raises(RuntimeError, match="missing from the table"):
        e3.bind()
    e3.close()


def test_comm_buckets_partition_the_buffer_with_heads_bound():
    dims = spec.ModelDims(kind="hulc", use_clip=True, use_bc_z=True, use_mia=True)
    eng = _engine(dims, 2, 4, "bf16")
    eng.bind()
    b = sorted(x for x in eng.comm_buckets() if x[1] > x[0])
    assert b[0][0] == 0 and b[-1][1] == eng.numel and all(b[i][1] == b[i + 1][0] for i in range(len(b) - 1)), b
    first = eng.comm_buckets()[0]          # issued first: [action_decoder.lo, numel) — the heads' gradients are final before the decoder backward
    for n, (off, shape) in eng.layout.items():
        if n.startswith(HEADS) or n == "logit_scale":
            assert first[0] <= off < first[1], n
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- module
def _ref_batch(batch):
    rb = {}
    for sc, mb in batch.items():
        d = dict(rgb_obs=dict(rgb_static=torch.from_numpy(mb["rgb_static"]), rgb_gripper=torch.from_numpy(mb["rgb_gripper"])), depth_obs={},
                 robot_obs=torch.zeros(mb["actions"].shape[:2] + (8,)), actions=torch.from_numpy(mb["actions"]),
                 state_info=dict(robot_obs=torch.from_numpy(mb["robot_obs"])), idx=torch.arange(mb["actions"].shape[0]))
        if "lang" in mb:
            d["lang"] = torch.from_numpy(mb["lang"])
            d["use_for_aux_lang_loss"] = torch.from_numpy(mb["use_for_aux"])
        if mb.get("plan_idx") is not None:
            d["plan_idx"] = torch.from_numpy(mb["plan_idx"].astype(np.int32))
        rb[sc] = d
    return rb


def test_module_logs_the_reference_names_and_values():
    """Hulc(...) with both losses: validation_step against val_aux_hulc, training_step against aux_all_hulc, strict state_dict round trip."""
    from hulc_amd.hulc import Hulc
    bcz = dict(_target_="hulc.models.auxiliary_loss_networks.bc_z_lang_decoder.BCZLangDecoder", in_features=4096, lang_dim=384)
    mia = dict(_target_="hulc.models.auxiliary_loss_networks.mia_lang_discriminator.MIALangDiscriminator", in_features=32, lang_dim=32, dropout_p=0.0)
    m = Hulc(precision="fp32", max_batch_size=BL, max_seq_len=S, use_clip_auxiliary_loss=True, use_bc_z_auxiliary_loss=True, bc_z_lang_decoder=bcz,
             use_mia_auxiliary_loss=True, mia_lang_discriminator=mia)
    # validation
    dims, P, batch, fx = load_aux_case("val_aux_hulc")
    assert dims == m.dims
    m.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()}, strict=True)
    m.eval()
    noise = {sc: {k: fx[f"{k}_{sc}"] for k in ("plan_idx_pp", "plan_idx_pr", "u_mix_pp", "u_act_pp", "u_mix_pr", "u_act_pr")} for sc in batch}
    m.validation_step(_ref_batch(batch), 0, noise=noise)
    for key in ("val/lang_pred_loss", "val/lang_contrastive_loss", "val/val_pred_clip_loss"):
        print(f"   {key}: module {m.logged[key]:.6f} reference {float(fx[key]):.6f}")
        assert abs(m.logged[key] - float(fx[key])) <= 1e-3 * abs(float(fx[key])), key
    assert abs(m.logged["val_act/lang_act_loss_pp"] - float(fx["action_loss_pp_lang"])) <= 1e-3 * abs(float(fx["action_loss_pp_lang"]))
    # training
    dims, P, batch, fx = load_aux_case("aux_all_hulc")
    sd = {k: torch.from_numpy(v) for k, v in P.items()}
    m.load_state_dict(sd, strict=True)
    out = m.state_dict()
    assert set(P) <= set(out) and all(np.array_equal(out[k].cpu().numpy().reshape(P[k].shape), P[k]) for k in P)
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if not k.startswith("mia_lang_discriminator.")}, strict=True)
    total = float(m.training_step(_ref_batch(batch), 0))          # eval mode (dropout off), the recorded plan sample: the fixture's step
    for key in ("train/pred_lang", "train/lang_contrastive", "train/lang_clip_loss", "train/total_loss"):
        print(f"   {key}: module {m.logged[key]:.6f} reference {float(fx['log/' + key]):.6f}")
        assert abs(m.logged[key] - float(fx["log/" + key])) <= 1e-3 * abs(float(fx["log/" + key])), key
    assert abs(total - float(fx["loss_total"])) <= 1e-3 * abs(float(fx["loss_total"]))
    m.engine.close()
