"""GPU (-m gpu): the deterministic action decoder on the engine (csrc/det_head.h, hulc_decoder_select) against the fixtures of the unmodified reference
(tools/gen_golden_det.py).  Gates are the project's own: fp32 loss 1e-3 of the reference, every gradient tensor 1e-3 rel-L2 of its float64 gradients (5e-3
for the conv sums) and adam_close as test_gpu_parity.py; 16-bit loss 5e-3 and gradient cosine > 0.99 as test_gpu_shapes.py; the paired pass 2e-5; the
rollout's actions 2e-3 as test_gpu_val.py / test_gpu_rollout_envs.py."""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from det_golden_util import BL, BV, DET_CASES, GOLDEN, ROLLOUT_DET, S, VAL_DET_CASES, case_batch, case_dims, case_params, load_det_case, rollout_frames  # noqa: E402
from golden_util import adam_close, check_grads64, grad_entries, load_case, rel_l2, sample_idx  # noqa: E402
from hulc_amd import spec  # noqa: E402

CLIP_BETA = 3.0
HEAD = "action_decoder.actions.0."


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


def run_step(eng, batch, step=0):
    eng.zero_grads()
    per = {}
    for sc, mb in batch.items():
        per[sc] = eng.forward_loss(to_dev(mb), "lang" in sc, 1.0 / len(batch), CLIP_BETA, step=step)
        eng.backward()
    tot = sum(l["total_mod"] for l in per.values()) / len(batch) + sum(CLIP_BETA * l["clip"] for l in per.values())
    return tot, per


def ref_style_batch(batch, dev="cuda"):
    """the reference's batch layout (rgb_obs / state_info dicts), with the recorded plan sample"""
    out = {}
    for sc, mb in batch.items():
        d = dict(rgb_obs=dict(rgb_static=torch.from_numpy(mb["rgb_static"]).to(dev), rgb_gripper=torch.from_numpy(mb["rgb_gripper"]).to(dev)),
                 depth_obs={}, robot_obs=torch.zeros(mb["actions"].shape[:2] + (8,), device=dev), actions=torch.from_numpy(mb["actions"]).to(dev),
                 state_info=dict(robot_obs=torch.from_numpy(mb["robot_obs"]).to(dev)), idx=torch.arange(mb["actions"].shape[0], device=dev),
                 plan_idx=torch.from_numpy(mb["plan_idx"].astype(np.int32)).to(dev))
        if "lang" in mb:
            d["lang"] = torch.from_numpy(mb["lang"]).to(dev)
            d["use_for_aux_lang_loss"] = torch.from_numpy(mb["use_for_aux"]).to(dev)
        out[sc] = d
    return out


def grads_np(eng):
    return {n: t.detach().cpu().numpy() for n, t in eng.views(eng.flat_grads).items()}


# ---------------------------------------------------------------------------------------------------------------- fixture parity, fp32
@pytest.mark.parametrize("name", list(DET_CASES))
def test_fp32_step_matches_the_reference(name):
    dims, P, batch, fx = load_det_case(name)
    eng = _engine(dims, BL, S, "fp32")
    eng.load_numpy(P)
    tot, per = run_step(eng, batch)
    ref = float(fx["loss_total"])
    print(f"[{name}] total: engine {tot:.6f} reference {ref:.6f}")
    assert abs(tot - ref) <= 1e-3 * abs(ref), (tot, ref)
    for sc in batch:
        r = float(fx[f"log/train/action_loss_{sc}"])
        print(f"   action_loss_{sc}: engine {per[sc]['action']:.6f} reference {r:.6f}")
        assert abs(per[sc]["action"] - r) <= 1e-3 * abs(r), (sc, per[sc]["action"], r)
    Gg = grads_np(eng)
    assert set(Gg) == {k[len("gradnorm64/"):] for k in fx.files if k.startswith("gradnorm64/")}
    w64, wn64 = check_grads64(Gg, fx, label=name)
    print(f"[{name}] grads vs fp64 reference: worst {w64[0]:.2e} ({w64[1]}) conv sums {wn64[0]:.2e} ({wn64[1]})")
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
def _cosine(Gg, fx, scale):
    a, b = [], []
    for key in fx.files:
        if key.startswith("gradnorm64/"):
            n = key[len("gradnorm64/"):]
            g = Gg[n].reshape(-1).astype(np.float64) / scale
            if "grad64/" + n in fx.files:
                a.append(g); b.append(fx["grad64/" + n].reshape(-1).astype(np.float64))
            else:
                a.append(g[sample_idx(n, g.size)]); b.append(fx["gradsamp64/" + n].astype(np.float64))
    a, b = np.concatenate(a), np.concatenate(b)
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(DET_CASES))
def test_16bit_step_close_to_the_reference(name, dtype):
    """fp16: the gradient buffer holds gradients x the loss scale, which must cancel.  The fixtures' head weight is 8 x the default (det_golden_util.HEAD_SCALE),
    so the gradients entering the decoder are 8 x larger and the fp16 backward of the language goal encoder (language_goal.mlp.*, upstream of the decoder)
    overflows at GradScaler's initial 65536 and still at 8192 (finite from 1024 down, measured) — what the scaler answers with skipped steps and a smaller
    scale; like test_gpu_aux_losses.py the test starts at 256 and checks that the scale stays there."""
    dims, P, batch, fx = load_det_case(name)
    eng = _engine(dims, BL, S, dtype)
    if dtype == "fp16":
        eng.scaler_enable(init_scale=256.0)
    eng.load_numpy(P)
    tot, per = run_step(eng, batch)
    eng.flush_grads()
    ref = float(fx["loss_total"])
    scale = eng.scaler_state()["scale"] if dtype == "fp16" else 1.0
    Gg = grads_np(eng)
    assert all(np.isfinite(g).all() for g in Gg.values())
    cos = _cosine(Gg, fx, scale)
    print(f"[{name} {dtype}] total: engine {tot:.6f} reference {ref:.6f}; gradient cosine {cos:.5f}; loss scale {scale}")
    for n in (HEAD + "weight", HEAD + "bias"):
        print(f"   {n}: |g| / |g_ref| = {np.linalg.norm(Gg[n].astype(np.float64)) / scale / float(fx['gradnorm64/' + n]):.4f}")
    assert abs(tot - ref) <= 5e-3 * abs(ref), (tot, ref)
    if dtype == "fp16":
        assert scale == 256.0
    assert cos > 0.99, cos
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- paired pass, split backward
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_paired_pass_equals_two_modality_passes(dtype):
    """hulc_forward_loss_pair needs equal window counts: the lang windows of det_huber_hulc next to its vis windows twice over."""
    dims, P, batch0, fx = load_det_case("det_huber_hulc")
    vis = batch0["vis"]
    batch = {"vis": {k: np.concatenate([vis[k], vis[k]], 0) for k in vis}, "lang": batch0["lang"]}
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
    for got, sc in ((pv, "vis"), (pl, "lang")):
        for k in ("total_mod", "kl", "action", "clip"):
            print(f"   [{dtype}] {sc} {k}: pair {got[k]:.6f} single {per1[sc][k]:.6f}")
            assert abs(got[k] - per1[sc][k]) <= tol * max(1.0, abs(per1[sc][k])), (sc, k, got[k], per1[sc][k])
    if dtype == "fp32":
        errs = {n: rel_l2(g2[n], g1[n]) for n in g1 if np.linalg.norm(g1[n]) > 1e-6}
        worst = max((e, n) for n, e in errs.items())
        print(f"   paired vs single gradients: worst {worst[0]:.2e} ({worst[1]}); head weight {errs[HEAD + 'weight']:.2e}")
        assert worst[0] <= 2e-5, worst
    else:
        a, b = np.concatenate([g.reshape(-1) for g in g1.values()]).astype(np.float64), np.concatenate([g.reshape(-1) for g in g2.values()]).astype(np.float64)
        assert float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b))) > 0.999
    eng.close()


def test_backward_parts_and_second_backward_accumulate():
    """hulc_backward_part(0) + (1) give the gradients of hulc_backward; a second modality's backward ADDS to the head's gradients (plain accumulate targets)."""
    dims, P, batch, fx = load_det_case("det_mse_hulc")
    eng = _engine(dims, BL, S, "fp32")
    eng.load_numpy(P)
    eng.zero_grads()
    eng.forward_loss(to_dev(batch["vis"]), False, 0.5, CLIP_BETA, step=0)
    eng.backward()
    g_vis = grads_np(eng)
    eng.zero_grads()
    eng.forward_loss(to_dev(batch["vis"]), False, 0.5, CLIP_BETA, step=0)
    eng.backward(0)
    eng.backward(1)
    g_parts = grads_np(eng)
    for n in (HEAD + "weight", HEAD + "bias", "action_decoder.rnn.weight_hh_l1"):
        assert np.array_equal(g_parts[n], g_vis[n]), n
    eng.forward_loss(to_dev(batch["lang"]), True, 0.5, CLIP_BETA, step=0)
    eng.backward()
    g_both = grads_np(eng)
    eng.zero_grads()
    eng.forward_loss(to_dev(batch["lang"]), True, 0.5, CLIP_BETA, step=0)
    eng.backward()
    g_lang = grads_np(eng)
    for n in (HEAD + "weight", HEAD + "bias"):
        assert np.linalg.norm(g_lang[n]) > 0
        assert rel_l2(g_both[n], g_vis[n].astype(np.float64) + g_lang[n]) <= 1e-6, n
    eng.close()


def test_grad_clip_norms_and_bucket_plan_cover_the_head():
    """gradient-norm logging counts the head's tensors; the data-parallel bucket plan partitions the buffer with them in the decoder's bucket"""
    dims, P, batch, fx = load_det_case("det_huber_hulc")
    eng = _engine(dims, BL, S, "fp32")
    eng.load_numpy(P)
    eng.set_grad_clip("norm", 1e9, track=True)
    run_step(eng, batch)
    Gg = grads_np(eng)
    eng.adam_step()
    norms = eng.grad_norms(per_tensor=True)
    total = float(np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in Gg.values())))
    assert abs(norms["total"] - total) <= 1e-4 * total, (norms["total"], total)
    for n in (HEAD + "weight", HEAD + "bias"):
        got = float(norms["per_tensor"][n])
        assert abs(got - np.linalg.norm(Gg[n].astype(np.float64))) <= 1e-4 * got and got > 0, n
    buckets = eng.comm_buckets()
    spans = sorted(b for b in buckets if b[1] > b[0])
    assert spans[0][0] == 0 and spans[-1][1] == eng.numel and all(a[1] == b[0] for a, b in zip(spans, spans[1:])), buckets
    for n in (HEAD + "weight", HEAD + "bias"):          # the decoder's bucket is issued first
        assert buckets[0][0] <= eng.layout[n][0] < buckets[0][1], (n, buckets[0])
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- validation
def test_validate_matches_the_reference():
    name = "val_det_hulc"
    dims, P, batch, fx = load_det_case(name)
    for sc, mb in batch.items():
        B = mb["actions"].shape[0]
        eng = _engine(dims, B, S, "fp32")
        eng.load_numpy(P)
        d = {k: torch.from_numpy(np.ascontiguousarray(mb[k], np.float32)).cuda() for k in ("rgb_static", "rgb_gripper", "actions", "robot_obs", "lang") if k in mb}
        noise = dict(plan_idx_pp=fx[f"plan_idx_pp_{sc}"], plan_idx_pr=fx[f"plan_idx_pr_{sc}"], u_mix_pp=np.zeros((B, S, 6, 10), np.float32))      # the noise is accepted and ignored
        o = eng.validate(d, "lang" in sc, noise, want_pred=True)
        eng.close()
        for k in ("action_loss_pp", "action_loss_pr", "kl_loss"):
            ref = float(fx[f"{k}_{sc}"])
            print(f"   [{sc}] {k}: engine {o[k]:.6f} reference {ref:.6f}")
            assert abs(o[k] - ref) <= 1e-3 * abs(ref) + 1e-6, (sc, k, o[k], ref)
        for k in ("mae_pp", "mae_pr"):
            assert np.abs(o[k] - fx[f"{k}_{sc}"].mean(0)).max() <= 2e-3, (sc, k, o[k], fx[f"{k}_{sc}"].mean(0))
        for k in ("gripper_sr_pp", "gripper_sr_pr"):
            assert abs(o[k] - float(fx[f"{k}_{sc}"])) <= 1e-6, (sc, k)
        for k in ("pred_pp", "pred_pr"):
            assert np.abs(o[k].cpu().numpy() - fx[f"{k}_{sc}"]).max() <= 2e-3, (sc, k)


# ---------------------------------------------------------------------------------------------------------------- rollout: module, engine, batched policy
def _det_model(c, max_batch, criterion="HuberLoss"):
    from hulc_amd import config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = config.compose(os.path.join(root, "conf"), "config", ["model=hulc", "model/action_decoder=deterministic", f"model.action_decoder.criterion={criterion}",
                                                                "trainer.precision=fp32", f"datamodule.batch_size={max_batch}"])
    m = config.instantiate(cfg.model, device="cuda:0", max_seq_len=4)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in case_params(c).items()})
    m.eval()
    return m


def test_module_rollout_and_batched_policy_match_the_reference():
    """Hulc.reset / step with the composed deterministic config reproduce the reference rollout across one replan (2e-3); BatchedPolicy(model, 3) rows equal
    the fixture within the same gate, whatever noise they are handed."""
    from hulc_amd import BatchedPolicy
    c = ROLLOUT_DET
    fx = np.load(os.path.join(GOLDEN, c["name"] + ".npz"))
    nsteps, rf = c["nsteps"], c["replan_freq"]
    frames = rollout_frames(c)
    m = _det_model(c, 3)
    assert m.dims.decoder == "deterministic" and m.dims.criterion == "HuberLoss"
    m.replan_freq = rf
    m.lang_embeddings = {"do the task": frames["lang"]["lang"][0:1]}
    goals = {"lang": "do the task", "vis": dict(rgb_obs=dict(rgb_static=torch.from_numpy(frames["vis"]["rgb_static"][:, nsteps:nsteps + 1]),
                                                              rgb_gripper=torch.from_numpy(frames["vis"]["rgb_gripper"][:, nsteps:nsteps + 1])))}

    def b1_obs(mode, t):
        mb = frames[mode]
        return dict(rgb_obs=dict(rgb_static=torch.from_numpy(mb["rgb_static"][:, t:t + 1]), rgb_gripper=torch.from_numpy(mb["rgb_gripper"][:, t:t + 1])),
                    depth_obs={}, robot_obs=torch.zeros(1, 1, 8), robot_obs_raw=torch.from_numpy(mb["robot_obs"][:, t:t + 1]))

    single = {}
    for mode in ("vis", "lang"):
        m.reset()
        for t in range(nsteps):
            a = m.step(b1_obs(mode, t), goals[mode], noise=dict(plan_idx=fx[f"plan_idx_{mode}"][t][0], u_mix=np.full((6, 10), 0.5, np.float32)))
            assert a.shape == (1, 1, 7)
            single[(mode, t)] = a.numpy()[0, 0]
            err = np.abs(single[(mode, t)] - fx[f"actions_{mode}"][0, t]).max()
            print(f"   step {mode} {t}: max |action - reference| {err:.2e}")
            assert err <= 2e-3, (mode, t, err)
    m.reset()
    pol = BatchedPolicy(m, 3)
    prog = {0: [("lang", t) for t in range(nsteps)], 1: [("vis", t) for t in range(nsteps)], 2: [None] + [("lang", t) for t in range(nsteps)]}
    for k in range(nsteps + 1):
        live = [(e, *prog[e][k]) for e in (1, 0, 2) if k < len(prog[e]) and prog[e][k] is not None]
        cat = lambda key: torch.from_numpy(np.stack([frames[mo][key][0, t][None] for _, mo, t in live]))
        obs = dict(rgb_obs=dict(rgb_static=cat("rgb_static"), rgb_gripper=cat("rgb_gripper")), robot_obs_raw=cat("robot_obs"))
        noise = dict(plan_idx=np.stack([fx[f"plan_idx_{mo}"][t][0] for _, mo, t in live]))
        a = pol.step(obs, [goals[mo] for _, mo, _ in live], env_ids=[e for e, _, _ in live], noise=noise)
        assert tuple(a.shape) == (len(live), 1, 7)
        for r, (e, mo, t) in enumerate(live):
            assert np.abs(a.numpy()[r, 0] - fx[f"actions_{mo}"][0, t]).max() <= 2e-3, (k, e, mo, t)
            assert np.abs(a.numpy()[r, 0] - single[(mo, t)]).max() <= 2e-3, (k, e, mo, t)
    m.engine.close()


def test_module_training_and_validation_steps_log_the_reference_names():
    """training_step / validation_step of the composed config: the reference's metric names, the fixture's values"""
    c = DET_CASES["det_huber_hulc"]
    dims, P, batch, fx = load_det_case("det_huber_hulc")
    m = _det_model(c, BL)
    loss = m.training_step(ref_style_batch(batch), 0)
    ref = float(fx["loss_total"])
    assert abs(float(loss) - ref) <= 1e-3 * abs(ref), (float(loss), ref)
    for k in ("train/kl_loss", "train/action_loss", "train/total_loss", "train/lang_clip_loss", "train/action_loss_vis", "train/action_loss_lang"):
        assert abs(m.logged[k] - float(fx["log/" + k])) <= 1e-3 * max(1.0, abs(float(fx["log/" + k]))), k
    p = dict(m.named_parameters())[HEAD + "weight"]
    assert p.grad is not None and float(p.grad.abs().sum()) > 0
    # load_state_dict is strict against the reference's key set of this configuration (tests/golden/state_manifest_det.json)
    from det_golden_util import load_manifest
    man = load_manifest()["hulc_det_w32"]["state_dict"]
    sd = {k: (torch.from_numpy(P[k]) if e["param"] else torch.tensor(e["value"], dtype=torch.float32).reshape(e["shape"])) for k, e in man.items()}
    assert set(m.state_dict()) == set(sd)
    m.load_state_dict(sd, strict=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict({**sd, "action_decoder.mean_fc.weight": torch.zeros(60, 2048)}, strict=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != HEAD + "bias"}, strict=True)
    rb = {sc: {k: v for k, v in d.items() if k != "plan_idx"} for sc, d in ref_style_batch(batch).items()}
    m.validation_step(rb, 0)
    for sc in batch:
        for k in (f"val_act/{sc}_act_loss_pp", f"val_kl/{sc}_kl_loss", f"val_total_mae/{sc}_total_mae_pp", f"val_grip/{sc}_grip_sr_pr"):
            assert k in m.logged and np.isfinite(m.logged[k]), k
    m.engine.close()


# ---------------------------------------------------------------------------------------------------------------- selector rules, the untouched default
def test_decoder_select_rules():
    from hulc_amd import lib as L
    lib = L.load()
    last = lambda: lib.hulc_last_error().decode("utf-8", "replace")
    for kind in ("gcbc", "mcil", "mcil_gru"):
        cfg = L.HulcConfig(kind=L.KIND[kind], dtype=L.DTYPE["fp32"], max_batch=2, max_seq=4, max_window=32, use_clip=0, kl_beta=0.01, kl_balancing_mix=0.8, dropout_p=0.0,
                           num_classes=10, gripper_alpha=1.0, log_scale_min=-7.0, seed=1)
        ctx = C.c_void_p()
        L.check(lib.hulc_ctx_create(C.byref(cfg), C.byref(ctx)))
        assert lib.hulc_decoder_select(ctx, 1, 0) != 0 and "hulc_decoder_select" in last(), kind
        L.check(lib.hulc_ctx_destroy(ctx))
    cfg = L.HulcConfig(kind=L.KIND["hulc"], dtype=L.DTYPE["fp32"], max_batch=2, max_seq=4, max_window=32, use_clip=1, kl_beta=0.01, kl_balancing_mix=0.8, dropout_p=0.0,
                       num_classes=10, gripper_alpha=1.0, log_scale_min=-7.0, seed=1)
    ctx = C.c_void_p()
    L.check(lib.hulc_ctx_create(C.byref(cfg), C.byref(ctx)))
    before = lib.hulc_workspace_bytes(ctx)
    assert lib.hulc_decoder_select(ctx, 2, 0) != 0 and lib.hulc_decoder_select(ctx, 1, 2) != 0      # unknown decoder, unknown criterion: nothing selected yet
    L.check(lib.hulc_decoder_select(ctx, 1, 1))
    assert lib.hulc_workspace_bytes(ctx) < before, "the packed-head buffers are released"
    assert lib.hulc_decoder_select(ctx, 1, 1) != 0 and "already" in last()
    L.check(lib.hulc_ctx_destroy(ctx))
    # after the bind: refused; a logistic table bound to a deterministic context: the head's tensors are missing
    dims = spec.ModelDims(kind="hulc", use_clip=True)
    eng = _engine(dims, 2, 4, "fp32")
    eng.load_numpy(spec.init_all(dims, seed=1))
    assert lib.hulc_decoder_select(eng.ctx, 1, 0) != 0 and "after hulc_bind_params" in last()
    eng.close()
    eng = _engine(dims, 2, 4, "fp32")
    L.check(lib.hulc_decoder_select(eng.ctx, 1, 0))
    with pytest.raises(RuntimeError, match="required parameter name is missing"):
        eng.bind()
    eng.close()


def test_default_context_keeps_the_parent_commits_forward_bits():
    """A context that never calls hulc_decoder_select: the fp32 forward of hulc_tiny gives, bit for bit, the losses and the packed heads recorded from the commit
    before the deterministic decoder (tests/golden/hulc_tiny_fwd_bits.npz)."""
    dims, P, batch, fx = load_case("hulc_tiny")
    bits = np.load(os.path.join(GOLDEN, "hulc_tiny_fwd_bits.npz"))
    eng = _engine(dims, 2, 4, "fp32")
    eng.load_numpy(P)
    eng.zero_grads()
    for sc, mb in batch.items():
        l = eng.forward_loss(to_dev(mb), "lang" in sc, 0.5, CLIP_BETA, step=0)
        got = np.array([l["total_mod"], l["kl"], l["action"], l["clip"]], np.float32).view(np.uint32)
        heads = eng.get_tensor("heads", 4 * 2 * 192).astype(np.float32).view(np.uint32)
        assert np.array_equal(got, bits[f"losses_{sc}"]), (sc, got, bits[f"losses_{sc}"])
        assert np.array_equal(heads, bits[f"heads_{sc}"]), sc
        eng.backward()
    eng.close()
