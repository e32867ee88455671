"""GPU (-m gpu): the feed-forward action decoder body (action_decoder.rnn_model=mlp_decoder; hulc_decoder_body_select) on the engine against the fixtures of the
unmodified reference (tools/gen_golden_mlp.py) and, stage by stage, against tests/mlp_decoder_ref.py applied to each stage's own device inputs.  Gates are
the project's own, as in tests/test_gpu_det_decoder.py: fp32 loss 1e-3 of the reference, every gradient tensor 1e-3 rel-L2 of its float64 gradients (5e-3 for
the conv sums) and adam_close; 16-bit loss 5e-3 and gradient cosine > 0.99; the paired pass 2e-5 (fp32) / 5e-3 (16 bit); actions 2e-3; the stage bounds are
those tests/gemm_epi_ref.py derives."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import mlp_decoder_ref as R  # noqa: E402
import plan_ln_inputs as PI  # noqa: E402
from golden_util import adam_close, check_grads64, grad_entries, load_case, rel_l2, sample_idx  # noqa: E402
from mlp_golden_util import (BL, BODY, BV, GOLDEN, MLP_CASES, ROLLOUT_MLP, ROUTES, S, case_dims, case_params, load_manifest, load_mlp_case, rollout_frames, route)  # noqa: E402
from plan_ln_gpu_util import check_tol  # noqa: E402
from hulc_amd import spec  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP_BETA = 3.0
AD = "action_decoder."
MLP = "model.action_decoder.rnn_model=mlp_decoder"


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
@pytest.mark.parametrize("name", list(MLP_CASES))
def test_fp32_step_matches_the_reference(name):
    dims, P, batch, fx = load_mlp_case(name)
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
    with_grad = {k[len("gradnorm64/"):] for k in fx.files if k.startswith("gradnorm64/")}
    assert set(BODY) <= with_grad <= set(Gg)
    for n in set(Gg) - with_grad:          # gcbc: the plan networks take no part in the step (gradnone/ in the fixture); their gradients stay zero
        assert f"gradnone/{n}" in fx.files and not np.any(Gg[n]), n
    w64, wn64 = check_grads64(Gg, fx, label=name)
    print(f"[{name}] grads vs fp64 reference: worst {w64[0]:.2e} ({w64[1]}) conv sums {wn64[0]:.2e} ({wn64[1]})")
    for n in BODY:
        assert np.linalg.norm(Gg[n]) > 0, n
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
@pytest.mark.parametrize("name", list(MLP_CASES))
def test_16bit_step_close_to_the_reference(name, dtype):
    """fp16: the gradient buffer holds gradients x the loss scale, which must cancel (started at 256 as tests/test_gpu_det_decoder.py does; it must stay there)"""
    dims, P, batch, fx = load_mlp_case(name)
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
    for n in BODY:
        print(f"   {n}: |g| / |g_ref| = {np.linalg.norm(Gg[n].astype(np.float64)) / scale / float(fx['gradnorm64/' + n]):.4f}")
    assert abs(tot - ref) <= 5e-3 * abs(ref), (tot, ref)
    if dtype == "fp16":
        assert scale == 256.0
    assert cos > 0.99, cos
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- paired pass, split backward, lazy zeroing
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_paired_pass_equals_two_modality_passes(dtype):
    """hulc_forward_loss_pair needs equal window counts: the lang windows of mlp_hulc next to its vis windows twice over."""
    dims, P, batch0, fx = load_mlp_case("mlp_hulc")
    vis = batch0["vis"]
    batch = {"vis": {k: np.concatenate([vis[k], vis[k]], 0) for k in vis}, "lang": batch0["lang"]}
    eng = _engine(dims, 2 * BL, S, dtype)
    if dtype == "fp16":
        eng.scaler_enable(init_scale=256.0)
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
        print(f"   paired vs single gradients: worst {worst[0]:.2e} ({worst[1]}); body {max(errs[n] for n in BODY):.2e}")
        assert worst[0] <= 2e-5, worst
    else:
        assert all(np.isfinite(g).all() for g in g2.values())
        a, b = np.concatenate([g.reshape(-1) for g in g1.values()]).astype(np.float64), np.concatenate([g.reshape(-1) for g in g2.values()]).astype(np.float64)
        assert float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b))) > 0.999
    eng.close()


def test_backward_parts_and_second_backward_accumulate():
    """hulc_backward_part(0) + (1) give the gradients of hulc_backward; a second modality's backward ADDS to the body's gradients (1e-6)."""
    dims, P, batch, fx = load_mlp_case("mlp_hulc")
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
    for n in BODY:
        assert np.array_equal(g_parts[n], g_vis[n]), n
    eng.forward_loss(to_dev(batch["lang"]), True, 0.5, CLIP_BETA, step=0)
    eng.backward()
    g_both = grads_np(eng)
    eng.zero_grads()
    eng.forward_loss(to_dev(batch["lang"]), True, 0.5, CLIP_BETA, step=0)
    eng.backward()
    g_lang = grads_np(eng)
    for n in BODY:
        assert np.linalg.norm(g_lang[n]) > 0
        assert rel_l2(g_both[n], g_vis[n].astype(np.float64) + g_lang[n]) <= 1e-6, n
    eng.close()


@pytest.mark.parametrize("kind,dtype", [("hulc", "bf16"), ("gcbc", "fp16")])
def test_lazy_zero_grads_equals_the_plain_memset(kind, dtype):
    """lazy_zero_grads 0 and 1, the buffer NaN-poisoned behind hulc_zero_grads.  "Identical" is asserted bit for bit where two runs of the SAME setting are
    identical: at B S = 128 the two 2048 x 2048 weight gradients of the body (the tensors lazy zeroing skips) go through the accumulate-only transpose + GEMM
    path without split K (asserted: no atomics).  This test DEPARTS from bit identity for every other tensor, because fp32 atomic adds land in a different order
    on every run, with either setting: the body's three bias gradients (column sums of dy / da1 / da0, M = 128 fp32 adds in any order) are held to twice
    tests/mlp_decoder_ref.py's stage_bgrad bound, (M + 1) 2^-24 sum |dY| per element and run; rnn.0.weight (plan scatter + two products) and the tensors
    outside the body keep the 5e-3 rel-L2 of tests/test_gpu_lazyzero.py.  A tensor that was never zeroed is NaN whatever the gate."""
    sys.path.insert(0, ROOT)
    from bench import synth_batch
    from hulc_amd import lib as L
    B, S_ = 16, 8
    ns, big = C.c_int32(-1), C.c_int32(-1)
    L.check(L.load().hulc_k_gemm_wgrad_nsplit(L.DTYPE[dtype], 2048, 2048, B * S_, C.byref(ns), C.byref(big)))
    assert ns.value == 1, ns.value
    dims = spec.ModelDims(kind=kind, max_window=32, use_clip=False, decoder_body="mlp")
    eng = _engine(dims, B, S_, dtype, seed=1)
    if dtype == "fp16":
        eng.scaler_enable(init_scale=256.0)
    eng.load_numpy(spec.init_all(dims, seed=0, ln_jitter=True))
    dev = torch.device("cuda:0")
    mb = synth_batch(B, S_, dev, 1, False)
    g = torch.Generator(device=dev); g.manual_seed(5)
    mb["plan_idx"] = torch.randint(0, 32, (B, 32), device=dev, generator=g, dtype=torch.int32)

    def run(poison):
        eng.zero_grads()
        if poison:
            eng.flat_grads.fill_(float("nan"))          # what zero_grads did not zero is now NaN ...
            eng.zero_grads()                              # ... and what it did zero is zeroed again
        eng.forward_loss(mb, False, 1.0, 0.0, step=0)
        eng.backward()
        torch.cuda.synchronize()
        return eng.flat_grads.clone()

    eng.set_option("lazy_zero_grads", 0)
    ref = run(False)
    eng.set_option("lazy_zero_grads", 1)
    runs = (run(True), run(False))
    M = B * S_
    bias_tol = {bn: 2 * R.stage_bgrad(eng.get_tensor(dn, M * 2048).astype(np.float64).reshape(M, 2048))[1]
                for bn, dn in ((BODY[5], "dec_dy"), (BODY[3], "dec_da1"), (BODY[1], "dec_da0"))}
    for got in runs:
        assert torch.isfinite(got).all(), "a lazily zeroed gradient tensor was added to (or never zeroed)"
        for name, (off, shape) in eng.layout.items():
            n = int(np.prod(shape)) if len(shape) else 1
            a, b = got[off:off + n].double(), ref[off:off + n].double()
            if name in (BODY[2], BODY[4]):
                assert float(b.abs().max()) > 0 and torch.equal(got[off:off + n], ref[off:off + n]), name
            elif name in bias_tol:
                d = (a - b).abs().cpu().numpy()
                print(f"   [{kind} {dtype}] {name}: max |lazy - memset| {d.max():.3e}, smallest bound {bias_tol[name].min():.3e}")
                assert float(b.abs().max()) > 0 and (d <= bias_tol[name]).all(), name
            elif float(b.abs().max()) == 0.0:
                assert float(a.abs().max()) == 0.0, name
            else:
                assert float((a - b).norm() / b.norm()) < 5e-3, name
    eng.close()


def test_grad_clip_norms_and_bucket_plan_cover_the_body():
    dims, P, batch, fx = load_mlp_case("mlp_gcbc")
    eng = _engine(dims, BL, S, "fp32")
    eng.load_numpy(P)
    eng.set_grad_clip("norm", 1e9, track=True)
    run_step(eng, batch)
    Gg = grads_np(eng)
    eng.adam_step()
    norms = eng.grad_norms(per_tensor=True)
    total = float(np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in Gg.values())))
    assert abs(norms["total"] - total) <= 1e-4 * total, (norms["total"], total)
    assert set(norms["per_tensor"]) == set(Gg) and not any("weight_hh" in n for n in Gg)
    for n in BODY:
        got = float(norms["per_tensor"][n])
        assert abs(got - np.linalg.norm(Gg[n].astype(np.float64))) <= 1e-4 * got and got > 0, n
    buckets = eng.comm_buckets()
    spans = sorted(b for b in buckets if b[1] > b[0])
    assert spans[0][0] == 0 and spans[-1][1] == eng.numel and all(a[1] == b[0] for a, b in zip(spans, spans[1:])), buckets
    for n in BODY:          # the decoder's bucket is issued first
        assert buckets[0][0] <= eng.layout[n][0] < buckets[0][1], (n, buckets[0])
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- validation
def test_validate_matches_the_reference():
    name = "val_mlp_hulc"
    dims, P, batch, fx = load_mlp_case(name)
    keys = ("plan_idx_pp", "plan_idx_pr", "u_mix_pp", "u_act_pp", "u_mix_pr", "u_act_pr")
    for sc, mb in batch.items():
        B = mb["actions"].shape[0]
        eng = _engine(dims, B, S, "fp32")
        eng.load_numpy(P)
        d = {k: torch.from_numpy(np.ascontiguousarray(mb[k], np.float32)).cuda() for k in ("rgb_static", "rgb_gripper", "actions", "robot_obs", "lang") if k in mb}
        o = eng.validate(d, "lang" in sc, {k: fx[f"{k}_{sc}"] for k in keys}, want_pred=True)
        eng.close()
        for k in ("action_loss_pp", "action_loss_pr", "kl_loss"):
            ref = float(fx[f"{k}_{sc}"])
            print(f"   [{sc}] {k}: engine {o[k]:.6f} reference {ref:.6f}")
            assert abs(o[k] - ref) <= 1e-3 * abs(ref) + 1e-6, (sc, k, o[k], ref)
        for k in ("mae_pp", "mae_pr"):
            assert np.abs(o[k] - fx[f"{k}_{sc}"].mean(0)).max() <= 2e-3, (sc, k, o[k], fx[f"{k}_{sc}"].mean(0))
        for k in ("gripper_sr_pp", "gripper_sr_pr"):
            assert abs(o[k] - float(fx[f"{k}_{sc}"])) <= 1e-6, (sc, k)


# ---------------------------------------------------------------------------------------------------------------- module: training, validation, rollout, batched policy
def _mlp_model(c, max_batch, precision="fp32"):
    from hulc_amd import config
    cfg = config.compose(os.path.join(ROOT, "conf"), "config", [f"model={c['kind']}", MLP, f"trainer.precision={precision}", f"datamodule.batch_size={max_batch}"])
    m = config.instantiate(cfg.model, device="cuda:0", max_seq_len=4)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in case_params(c).items()})
    m.eval()
    return m


@pytest.mark.parametrize("name", list(MLP_CASES))
def test_module_training_and_validation_steps(name):
    c = MLP_CASES[name]
    dims, P, batch, fx = load_mlp_case(name)
    m = _mlp_model(c, BL)
    assert m.dims.decoder_body == "mlp" and m.dims.kind == c["kind"]
    loss = m.training_step(ref_style_batch(batch), 0)
    ref = float(fx["loss_total"])
    assert abs(float(loss) - ref) <= 1e-3 * abs(ref), (float(loss), ref)
    for k in ("train/action_loss", "train/total_loss", "train/action_loss_vis", "train/action_loss_lang"):
        assert abs(m.logged[k] - float(fx["log/" + k])) <= 1e-3 * max(1.0, abs(float(fx["log/" + k]))), k
    for n in BODY:
        p = dict(m.named_parameters())[n]
        assert p.grad is not None and float(p.grad.abs().sum()) > 0, n
    # load_state_dict is strict against the reference's key set of this configuration (tests/golden/state_manifest_mlp.json)
    man = load_manifest()[name]["state_dict"]
    sd = {k: (torch.from_numpy(P[k]) if e["param"] else torch.tensor(e["value"], dtype=torch.float32).reshape(e["shape"])) for k, e in man.items()}
    assert set(m.state_dict()) == set(sd)
    m.load_state_dict(sd, strict=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict({**sd, AD + "rnn.weight_hh_l0": torch.zeros(2048, 2048)}, strict=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != BODY[5]}, strict=True)
    rb = {sc: {k: v for k, v in d.items() if k != "plan_idx"} for sc, d in ref_style_batch(batch).items()}
    m.validation_step(rb, 0)
    for sc in batch:
        k = f"val_act/{sc}_act_loss_pp" if c["kind"] == "hulc" else f"val_act/{sc}_act_loss"          # GCBC.validation_step has one pass (gcbc.py:226-246)
        assert k in m.logged and np.isfinite(m.logged[k]), k
    m.engine.close()


def test_checkpoint_records_the_body_and_a_mismatched_resume_is_refused(tmp_path):
    """a short fit with the composed option descends and checkpoints; the checkpoint's hyper_parameters hold the body; Trainer.fit(ckpt_path=...) of the other
    body is refused with both bodies named, in both directions (a checkpoint without the field counts as the recurrence)"""
    from hulc_amd import config
    from hulc_amd.trainer import ModelCheckpoint, SyntheticDataModule, Trainer, get_last_checkpoint

    def build(*ov):
        cfg = config.compose(os.path.join(ROOT, "conf"), "config", ["model=gcbc", "trainer.precision=bf16", "datamodule.batch_size=2", *ov])
        return config.instantiate(cfg.model, device="cuda:0", max_seq_len=4)

    one = list(SyntheticDataModule(batch_size=2, max_window_size=4, modalities=["vis", "lang"], steps_per_epoch=1, seed=3).train_dataloader(0))

    class Fixed:
        def train_dataloader(self, rank=0):
            for _ in range(6):
                yield one[0]

        def val_dataloader(self, rank=0):
            yield one[0]

    m = build(MLP)
    tr = Trainer(max_epochs=1, log_dir=str(tmp_path), callbacks=[ModelCheckpoint()], log_every=1)
    losses = [h["loss"] for h in tr.fit(m, Fixed())]
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    ck = get_last_checkpoint(str(tmp_path))
    sd = torch.load(ck, map_location="cpu", weights_only=False)
    assert sd["hyper_parameters"]["decoder_body"] == "mlp" and BODY[4] in sd["state_dict"] and AD + "rnn.weight_hh_l1" not in sd["state_dict"]
    m.engine.close()
    m2 = build()
    with pytest.raises(RuntimeError, match=r"'mlp' decoder body.*builds 'rnn'"):
        Trainer(max_epochs=2, log_dir=str(tmp_path / "a"), log_every=1).fit(m2, Fixed(), ckpt_path=ck)
    m2.engine.close()
    old = str(tmp_path / "old.ckpt")
    del sd["hyper_parameters"]["decoder_body"]
    torch.save(sd, old)
    m3 = build(MLP)
    with pytest.raises(RuntimeError, match=r"'rnn' decoder body.*builds 'mlp'"):
        Trainer(max_epochs=2, log_dir=str(tmp_path / "b"), log_every=1).fit(m3, Fixed(), ckpt_path=old)
    Trainer(max_epochs=2, log_dir=str(tmp_path / "c"), log_every=1, limit_val_batches=0).fit(m3, Fixed(), ckpt_path=ck)          # the matching body resumes
    m3.engine.close()


def test_module_rollout_and_batched_policy_match_the_reference():
    """Hulc.reset / step with the composed mlp_decoder config reproduce the reference rollout across one replan (2e-3); BatchedPolicy(model, 3) rows with
    out-of-step environments equal the fixture and the B = 1 path within the same gate; a repeated step (same observation, plan, goal and noise) returns the
    same action — nothing is carried from step to step."""
    from hulc_amd import BatchedPolicy
    c = ROLLOUT_MLP
    fx = np.load(os.path.join(GOLDEN, c["name"] + ".npz"))
    nsteps, rf = c["nsteps"], c["replan_freq"]
    frames = rollout_frames(c)
    m = _mlp_model(c, 3)
    m.replan_freq = rf
    m.lang_embeddings = {"do the task": frames["lang"]["lang"][0:1]}
    goals = {"lang": "do the task", "vis": dict(rgb_obs=dict(rgb_static=torch.from_numpy(frames["vis"]["rgb_static"][:, nsteps:nsteps + 1]),
                                                              rgb_gripper=torch.from_numpy(frames["vis"]["rgb_gripper"][:, nsteps:nsteps + 1])))}

    def b1_obs(mode, t):
        mb = frames[mode]
        return dict(rgb_obs=dict(rgb_static=torch.from_numpy(mb["rgb_static"][:, t:t + 1]), rgb_gripper=torch.from_numpy(mb["rgb_gripper"][:, t:t + 1])),
                    depth_obs={}, robot_obs=torch.zeros(1, 1, 8), robot_obs_raw=torch.from_numpy(mb["robot_obs"][:, t:t + 1]))

    def nz(mode, t):
        return dict(plan_idx=fx[f"plan_idx_{mode}"][t][0], u_mix=fx[f"u_mix_{mode}"][t][0, 0], u_act=fx[f"u_act_{mode}"][t][0, 0])

    single = {}
    for mode in ("vis", "lang"):
        m.reset()
        for t in range(nsteps):
            a = m.step(b1_obs(mode, t), goals[mode], noise=nz(mode, t))
            assert a.shape == (1, 1, 7)
            single[(mode, t)] = a.numpy()[0, 0]
            err = np.abs(single[(mode, t)] - fx[f"actions_{mode}"][0, t]).max()
            print(f"   step {mode} {t}: max |action - reference| {err:.2e}")
            assert err <= 2e-3, (mode, t, err)
    # no state leaks: step 0 twice (the second call is no replan step: same plan, same goal; the recurrent body would continue from the first call's state)
    m.reset()
    a0 = m.step(b1_obs("lang", 0), goals["lang"], noise=nz("lang", 0)).numpy()
    a1 = m.step(b1_obs("lang", 0), goals["lang"], noise=nz("lang", 0)).numpy()
    assert np.array_equal(a0, a1) and np.array_equal(a0[0, 0], single[("lang", 0)])
    m.reset()
    pol = BatchedPolicy(m, 3)
    prog = {0: [("lang", t) for t in range(nsteps)], 1: [("vis", t) for t in range(nsteps)], 2: [None] + [("lang", t) for t in range(nsteps)]}
    for k in range(nsteps + 1):
        live = [(e, *prog[e][k]) for e in (1, 0, 2) if k < len(prog[e]) and prog[e][k] is not None]
        cat = lambda key: torch.from_numpy(np.stack([frames[mo][key][0, t][None] for _, mo, t in live]))
        obs = dict(rgb_obs=dict(rgb_static=cat("rgb_static"), rgb_gripper=cat("rgb_gripper")), robot_obs_raw=cat("robot_obs"))
        noise = dict(plan_idx=np.stack([fx[f"plan_idx_{mo}"][t][0] for _, mo, t in live]), u_mix=np.stack([fx[f"u_mix_{mo}"][t][0, 0] for _, mo, t in live]),
                     u_act=np.stack([fx[f"u_act_{mo}"][t][0, 0] for _, mo, t in live]))
        a = pol.step(obs, [goals[mo] for _, mo, _ in live], env_ids=[e for e, _, _ in live], noise=noise)
        assert tuple(a.shape) == (len(live), 1, 7)
        for r, (e, mo, t) in enumerate(live):
            assert np.abs(a.numpy()[r, 0] - fx[f"actions_{mo}"][0, t]).max() <= 2e-3, (k, e, mo, t)
            assert np.abs(a.numpy()[r, 0] - single[(mo, t)]).max() <= 2e-3, (k, e, mo, t)
    m.engine.close()


def test_batched_rollout_16bit_equals_the_b1_path():
    """the 16-bit hulc_rollout_envs_act of this body runs the recurrence-free row kernels (rollout_step.h; no per-slot hidden buffers; more rows and the stages
    themselves: tests/test_gpu_mlp_rollout_rows.py): three slots stepped together give the B = 1 rollout's (dec_fwd) actions of the same frames, plans and noise (2e-3 x the action range is far below a flipped mixture component: the noise pins it)."""
    c = ROLLOUT_MLP
    frames = rollout_frames(c)
    dims, P = case_dims(c), case_params(c)
    eng = _engine(dims, 3, 2, "bf16")
    eng.load_numpy(P)
    mb = frames["lang"]
    u_mix = np.full((3, 6, 10), 0.999, np.float32)
    for r in range(3):
        for d in range(6):
            u_mix[r, d, (r + 3 * d) % 10] = 0.0          # a Gumbel gap of ~13.9 in favour of one component: rounding cannot change the choice
    u_act = np.linspace(0.2, 0.8, 18, dtype=np.float32).reshape(3, 6)
    plan = np.stack([(np.arange(32) * (r + 1)) % 32 for r in range(3)]).astype(np.int32)
    obs = lambda rows: dict(rgb_static=torch.from_numpy(np.stack([mb["rgb_static"][0, t] for t in rows])[:, None]).cuda(),
                            rgb_gripper=torch.from_numpy(np.stack([mb["rgb_gripper"][0, t] for t in rows])[:, None]).cuda(),
                            robot_obs_raw=torch.from_numpy(np.stack([mb["robot_obs"][0, t] for t in rows])[:, None]).cuda())
    lang = torch.from_numpy(np.repeat(mb["lang"][0:1], 3, 0)).cuda()
    b1 = []
    for r in range(3):
        eng.rollout_reset()
        eng.rollout_plan(obs([r]), lang[0:1], plan_idx=plan[r])
        b1.append(eng.rollout_act(obs([r]), u_mix=u_mix[r], u_act=u_act[r]))
    eng.rollout_envs_init(3)
    eng.rollout_envs_plan(obs([0, 1, 2]), lang, env_ids=[2, 0, 1], plan=plan)
    a = eng.rollout_envs_act(obs([0, 1, 2]), env_ids=[2, 0, 1], u_mix=u_mix, u_act=u_act)
    a2 = eng.rollout_envs_act(obs([0, 1, 2]), env_ids=[2, 0, 1], u_mix=u_mix, u_act=u_act)
    assert np.array_equal(a, a2), "a second step with the same inputs: no state"
    eng.rollout_envs_reset([0], clear_hidden=True)
    with pytest.raises(RuntimeError, match="no plan"):
        eng.rollout_envs_act(obs([1]), env_ids=[0], u_mix=u_mix[:1], u_act=u_act[:1])
    # gate: the five 16-bit tensors between the frames and the heads (emb, a0, a1, y, and the time-invariant term) each round to half a bf16 ulp (2^-9 relative),
    # and the two paths run them at different row counts: 5 x 2^-9 of the action range 4.  A wrong slot, plan or noise row is no rounding: the rows differ by far more
    gate = 5 * 2.0 ** -9 * 4
    b1 = np.stack([np.asarray(x).reshape(7) for x in b1])
    assert min(np.abs(b1[i, :6] - b1[j, :6]).max() for i in range(3) for j in range(i)) > 4 * gate
    for r in range(3):
        err = np.abs(np.asarray(a)[r].reshape(-1) - b1[r]).max()
        print(f"   row {r}: max |batched - B=1| {err:.2e} (gate {gate:.2e})")
        assert err <= gate, (r, err)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- the entry's rules, the untouched default
def _ctx(L, lib, kind, use_clip=0):
    cfg = L.HulcConfig(kind=L.KIND[kind], dtype=L.DTYPE["fp32"], max_batch=2, max_seq=4, max_window=32, use_clip=use_clip, kl_beta=0.01, kl_balancing_mix=0.8, dropout_p=0.0,
                       num_classes=10, gripper_alpha=1.0, log_scale_min=-7.0, seed=1)
    ctx = C.c_void_p()
    L.check(lib.hulc_ctx_create(C.byref(cfg), C.byref(ctx)))
    return ctx


def test_body_select_rules():
    from hulc_amd import lib as L
    lib = L.load()
    last = lambda: lib.hulc_last_error().decode("utf-8", "replace")
    for kind in ("mcil", "mcil_gru"):
        ctx = _ctx(L, lib, kind)
        assert lib.hulc_decoder_body_select(ctx, L.BODY["mlp"]) != 0 and "MCIL" in last(), kind
        L.check(lib.hulc_ctx_destroy(ctx))
    for kind in ("hulc", "gcbc"):
        ctx = _ctx(L, lib, kind, 1)
        before = lib.hulc_workspace_bytes(ctx)
        assert lib.hulc_decoder_body_select(ctx, 2) != 0 and "unknown body" in last()          # nothing selected yet
        L.check(lib.hulc_decoder_body_select(ctx, L.BODY["mlp"]))
        assert lib.hulc_workspace_bytes(ctx) < before, "the recurrence's buffers are released"
        assert lib.hulc_decoder_body_select(ctx, L.BODY["mlp"]) != 0 and "already" in last()
        assert lib.hulc_decoder_select(ctx, L.DECODER["deterministic"], 0) != 0, "mlp, then deterministic"
        assert ("feed-forward" if kind == "hulc" else "HULC_KIND_GCBC") in last()          # gcbc has no deterministic decoder at all: that refusal comes first
        L.check(lib.hulc_ctx_destroy(ctx))
    ctx = _ctx(L, lib, "hulc", 1)
    L.check(lib.hulc_decoder_select(ctx, L.DECODER["deterministic"], 0))
    assert lib.hulc_decoder_body_select(ctx, L.BODY["mlp"]) != 0 and "deterministic" in last(), "deterministic, then mlp"
    L.check(lib.hulc_ctx_destroy(ctx))
    # HULC_BODY_RNN: accepted, changes nothing — the recurrent table binds and steps; after the bind every call is refused
    dims = spec.ModelDims(kind="hulc", use_clip=True)
    eng = _engine(dims, 2, 4, "fp32")
    before = lib.hulc_workspace_bytes(eng.ctx)
    L.check(lib.hulc_decoder_body_select(eng.ctx, L.BODY["rnn"]))
    assert lib.hulc_workspace_bytes(eng.ctx) == before
    eng.load_numpy(spec.init_all(dims, seed=1))
    assert lib.hulc_decoder_body_select(eng.ctx, L.BODY["mlp"]) != 0 and "after hulc_bind_params" in last()
    eng.close()
    # a recurrent table bound to an mlp context: the body's tensors are missing — and the other way round
    eng = _engine(dims, 2, 4, "fp32")
    L.check(lib.hulc_decoder_body_select(eng.ctx, L.BODY["mlp"]))
    with pytest.raises(RuntimeError, match="required parameter name is missing"):
        eng.bind()
    eng.close()
    # the engine wrapper selects the body itself for an mlp table: a second selection of the same context is refused
    eng = _engine(spec.ModelDims(kind="gcbc", use_clip=True, decoder_body="mlp"), 2, 4, "fp32")
    assert lib.hulc_decoder_body_select(eng.ctx, L.BODY["rnn"]) != 0 and "already" in last()
    eng.close()


def test_default_context_keeps_the_parent_commits_forward_bits():
    """A context that never calls hulc_decoder_body_select: the fp32 forward of hulc_tiny gives, bit for bit, the losses and the packed heads recorded before
    either selector existed (tests/golden/hulc_tiny_fwd_bits.npz)."""
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
    with pytest.raises(RuntimeError, match="unknown tensor"):
        eng.get_tensor("dec_a0", 16)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- stage-level float64 at the routed shapes
STAGE_SHAPES = [(40, 8, ("64", 128)), (64, 16, ("glds", 0))]          # B, S, the route of M x 2048 x 2048 (tests/mlp_golden_util.py ROUTES)
assert all((B * S_,) + want in ROUTES for B, S_, want in STAGE_SHAPES)
ROWS = 7          # every 7th row: coprime to every tile and fragment height, so every row position of a tile and every tile is met


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,S_,want", STAGE_SHAPES)
def test_stages_against_float64_of_their_own_device_inputs(B, S_, want, dtype):
    """One training step at B S = 320 / 1024; dec_a0 / dec_a1 / dec_y and their gradients are read back and every stage — forward, data gradient, weight
    gradient, bias gradient — is compared with float64 applied to THAT stage's device inputs, so only one product's rounding enters each comparison.  Per-element
    bound: tests/gemm_epi_ref.py's for the operand and output types ((K + 2) 2^-24 sum |a||b| + the epilogue's + one ulp of a 16-bit output).  ReLU decisions
    must agree exactly wherever the float64 pre-activation is further from zero than its bound; masked gradient elements must be exactly zero."""
    sys.path.insert(0, ROOT)
    from bench import synth_batch
    from hulc_amd import lib as L
    M, H = B * S_, 2048
    assert route(dtype, M) == want, (M, route(dtype, M))
    dims = spec.ModelDims(kind="hulc", max_window=32, use_clip=False, decoder_body="mlp")
    P = spec.init_all(dims, seed=4, ln_jitter=True)
    eng = _engine(dims, B, S_, dtype, seed=1)
    if dtype == "fp16":
        eng.scaler_enable(init_scale=256.0)
    eng.load_numpy(P)
    dev = torch.device("cuda:0")
    mb = synth_batch(B, S_, dev, 3, False)
    g = torch.Generator(device=dev); g.manual_seed(7)
    mb["plan_idx"] = torch.randint(0, 32, (B, 32), device=dev, generator=g, dtype=torch.int32)
    eng.zero_grads()
    eng.forward_loss(mb, False, 1.0, 0.0, step=0)
    eng.backward()
    eng.flush_grads()
    T = {k: eng.get_tensor(k, M * H).astype(np.float64).reshape(M, H) for k in ("dec_a0", "dec_a1", "dec_y", "dec_dy", "dec_da1", "dec_da0")}
    emb = eng.get_tensor("emb", M * 128).astype(np.float64).reshape(B, S_, 128)
    cb = eng.get_tensor("dec_cb", B * H).astype(np.float64).reshape(B, H)
    Gg = grads_np(eng)
    eng.close()
    assert all(np.isfinite(v).all() for v in T.values())
    W = {n: PI.round_t(P[n], dtype) for n in BODY if n.endswith("weight")}          # the engine's 16-bit shadow of the fp32 parameters
    bias = {n: P[n].astype(np.float64) for n in BODY if n.endswith("bias")}
    embg = emb[..., 64:].transpose(1, 0, 2).reshape(M, 64)          # time-major rows r = t B + b
    rows = np.arange(0, M, ROWS)
    kp = dims.dec_plan

    def fwd(what, X, Wn, bn, got, act, res=None):
        ref, tol, pre, ptol = R.stage_fwd(X[rows], Wn if isinstance(Wn, np.ndarray) else W[Wn], bias[bn] if res is None else None, dtype, act, res=res, res_rowmod=0)
        check_tol(np.abs(got[rows] - ref), tol, got[rows], ref, f"{what} [{dtype} M={M}]")
        if act:
            sure = np.abs(pre) > ptol
            frac = float((got[rows] > 0).mean())
            assert 0.2 < frac < 0.8 and sure.mean() > 0.99, (what, frac, sure.mean())
            assert np.array_equal((got[rows] > 0)[sure], (pre > 0)[sure]), f"{what}: a ReLU decision differs away from zero"

    # layer 0: the K = 64 product over the gripper half of emb + the time-invariant term (bias, plan columns, goal columns) as the broadcast residual
    fwd("a0", embg, np.ascontiguousarray(W[BODY[0]][:, kp:kp + 64]), None, T["dec_a0"], True, res=cb[rows % B])
    fwd("a1", T["dec_a0"], BODY[2], BODY[3], T["dec_a1"], True)
    fwd("y", T["dec_a1"], BODY[4], BODY[5], T["dec_y"], False)

    def dgrad(what, dY, Wn, mask, got):
        ref, tol = R.stage_dgrad(dY[rows], W[Wn].T.copy(), mask[rows], dtype)
        check_tol(np.abs(got[rows] - ref), tol, got[rows], ref, f"{what} [{dtype} M={M}]")
        assert (got[mask <= 0] == 0).all() and (got[rows] != 0).mean() > 0.2, f"{what}: the ReLU mask"

    dgrad("da1", T["dec_dy"], BODY[4], T["dec_a1"], T["dec_da1"])
    dgrad("da0", T["dec_da1"], BODY[2], T["dec_a0"], T["dec_da0"])

    ns, big = C.c_int32(-1), C.c_int32(-1)
    L.check(L.load().hulc_k_gemm_wgrad_nsplit(L.DTYPE[dtype], H, H, M, C.byref(ns), C.byref(big)))
    wrows = np.arange(0, H, ROWS)

    def wgrad(what, dY, X, got, nsplit):
        ref, tol = R.stage_wgrad(dY[:, wrows], X, nsplit)
        check_tol(np.abs(got[wrows] - ref), tol, got[wrows], ref, f"{what} [{dtype} M={M}]")
        assert np.abs(ref).max() > 0

    def bgrad(what, dY, got):
        ref, tol = R.stage_bgrad(dY)
        check_tol(np.abs(got - ref), tol, got, ref, f"{what} [{dtype} M={M}]")

    wgrad("dW2", T["dec_dy"], T["dec_a1"], Gg[BODY[4]].astype(np.float64), max(ns.value, 1))
    bgrad("db2", T["dec_dy"], Gg[BODY[5]].astype(np.float64))
    wgrad("dW1", T["dec_da1"], T["dec_a0"], Gg[BODY[2]].astype(np.float64), max(ns.value, 1))
    bgrad("db1", T["dec_da1"], Gg[BODY[3]].astype(np.float64))
    wgrad("dW0[:, emb]", T["dec_da0"], embg, Gg[BODY[0]].astype(np.float64)[:, kp:kp + 64], 2)          # accumulates into the zeroed gradient: one more rounding
    bgrad("db0", T["dec_da0"], Gg[BODY[1]].astype(np.float64))
