"""Generate tests/golden/mlp_{hulc,gcbc}.npz, val_mlp_hulc.npz, rollout_mlp_hulc.npz and state_manifest_mlp.json: the UNMODIFIED reference with
action_decoder.rnn_model=mlp_decoder (hulc/models/decoders/utils/rnn.py: Linear-ReLU-Linear-ReLU-Linear in place of the recurrence), on CPU, eval mode, with
the recorded plan sample.  No file of the reference is edited or copied.

Run in the build container only:  python tools/gen_golden_mlp.py [case ...]
Format as tools/gen_golden_det.py: inputs and parameters by name (tests/mlp_golden_util.py regenerates them), the reference's losses and logged values,
per-parameter gradients (full up to 4096 elements, else norm + 64 samples), parameters after one Adam step, the float64 run's gradients (grad64/), the
parameter table in named_parameters order — and the decoder's inputs of the float64 run (emb64_<scope>, goal64_<scope>, a_tcp_<scope>), from which
tests/mlp_decoder_ref.py restates the action loss and the decoder's gradients.

The generator asserts that between 20 % and 80 % of the reference's own a0 and a1 are positive in every case and scope (mlp_golden_util.RELU_POS); a seed that
fails this is replaced by the next one.
"""
from __future__ import annotations

import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
warnings.filterwarnings("ignore")

import ref_harness  # noqa: E402
from gen_golden import FULL_MAX, sample_idx, to_ref_batch  # noqa: E402
from gen_golden_val import RandRecorder, load_params  # noqa: E402
from gen_golden_aux import record_grads  # noqa: E402
from mlp_golden_util import (BL, BV, MLP_CASES, RELU_POS, ROLLOUT_MLP, S, VAL_MLP_CASES, case_batch, case_params, rollout_frames)  # noqa: E402


def build(c, double=False):
    """conf/model/{hulc,gcbc}.yaml with model.action_decoder.rnn_model=mlp_decoder, resolved."""
    ref_harness.install_stubs()
    cfg = ref_harness.model_cfg(c["kind"], max_window=32, use_clip=True)
    ad = dict(cfg["action_decoder"])
    ad["rnn_model"] = "mlp_decoder"
    cfg["action_decoder"] = ref_harness.to_cfg(ad)
    if c["kind"] == "hulc":
        from hulc.models.hulc import Hulc as Cls
    else:
        from hulc.models.gcbc import GCBC as Cls
    m = Cls(**cfg).eval()
    assert isinstance(m.action_decoder.rnn, torch.nn.Sequential) and len(m.action_decoder.rnn) == 5
    return m.double() if double else m


def run_case(name, c, outdir):
    batch = case_batch(c)
    rb = to_ref_batch(batch)
    P = case_params(c)
    model = build(c)
    names = [n for n, _ in model.named_parameters()]
    assert set(names) == set(P.keys()), set(names) ^ set(P.keys())
    load_params(model, P)
    scope_order = list(batch.keys())
    rec, calls = {}, {"i": 0}
    frac = {}

    def hook_loss(m, store, tag):
        orig = m.action_decoder.loss

        def loss_hook(latent_plan, perceptual_emb, latent_goal, actions, robot_obs):
            sc = scope_order[calls["i"] % len(scope_order)]
            calls["i"] += 1
            if latent_plan.shape[-1] > 0 and tag == "":
                store[f"plan_idx_{sc}"] = latent_plan.detach().reshape(latent_plan.shape[0], 32, 32).argmax(-1).numpy()
            if tag == "64":
                store[f"emb64_{sc}"] = perceptual_emb.detach().numpy().astype(np.float64)
                store[f"goal64_{sc}"] = latent_goal.detach().numpy().astype(np.float64)
            return orig(latent_plan, perceptual_emb, latent_goal, actions, robot_obs)

        m.action_decoder.loss = loss_hook

    hook_loss(model, rec, "")
    acalls = {1: 0, 3: 0}

    def relu_hook(idx):
        def h(module, inp, out):
            sc = scope_order[acalls[idx] % len(scope_order)]
            acalls[idx] += 1
            frac[(sc, idx)] = float((out > 0).float().mean())
        return h

    model.action_decoder.rnn[1].register_forward_hook(relu_hook(1))
    model.action_decoder.rnn[3].register_forward_hook(relu_hook(3))
    torch.manual_seed(1234 + c["seed"])
    opt = torch.optim.Adam(model.parameters(), lr=2e-4)
    loss = model.training_step(rb, 0)
    for (sc, idx), f in sorted(frac.items()):
        print(f"[{name}/{sc}] a{idx // 2}: {100 * f:.1f} % positive")
        assert RELU_POS[0] <= f <= RELU_POS[1], (name, sc, idx, f, "take the next seed")
        rec[f"relu_pos_a{idx // 2}_{sc}"] = np.float64(f)
    opt.zero_grad()
    loss.backward()
    from hulc.models.decoders.utils.gripper_control import world_to_tcp_frame
    for sc in scope_order:
        rec[f"a_tcp_{sc}"] = world_to_tcp_frame(rb[sc]["actions"], rb[sc]["state_info"]["robot_obs"]).numpy()
    fx = {"loss_total": np.float32(loss.item())}
    for k, v in model.logged.items():
        fx["log/" + k] = np.float32(v)
    fx.update(rec)
    record_grads(model, fx)
    opt.step()
    for n, p in model.named_parameters():
        flat = p.detach().numpy().reshape(-1)
        fx[f"adam1/{n}"] = flat.copy() if flat.size <= FULL_MAX else flat[sample_idx(n, flat.size)]

    # ---- float64 run of the same unmodified reference with the recorded plan sample (as tools/gen_golden.py)
    import torch.distributions as D
    model64 = build(c, double=True)
    with torch.no_grad():
        for n, p in model64.named_parameters():
            p.copy_(torch.from_numpy(P[n]).reshape(p.shape).double())
    calls["i"] = 0
    hook_loss(model64, fx, "64")
    it = {"i": 0}
    orig_rs = D.Independent.rsample

    def rs(self, sample_shape=torch.Size()):
        sc = scope_order[it["i"] % len(scope_order)]
        it["i"] += 1
        probs = self.base_dist.probs
        onehot = torch.nn.functional.one_hot(torch.from_numpy(fx[f"plan_idx_{sc}"]).long(), probs.shape[-1]).to(probs.dtype)
        return onehot + probs - probs.detach()

    def cast(x, key=""):          # actions / robot_obs stay fp32: world_to_tcp_frame is an fp32 island by construction (gripper_control.py:17-20)
        if isinstance(x, dict):
            return {k: cast(v, k) for k, v in x.items()}
        if key in ("actions", "state_info", "robot_obs"):
            return x
        return x.double() if torch.is_tensor(x) and x.is_floating_point() else x

    D.Independent.rsample = rs
    try:
        loss64 = model64.training_step(cast(rb), 0)
        loss64.backward()
    finally:
        D.Independent.rsample = orig_rs
    fx["loss_total_fp64"] = np.float64(loss64.item())
    for k, v in model64.logged.items():
        fx["log64/" + k] = np.float64(v)
    record_grads(model64, fx, tag64=True)
    fx["meta/param_names"] = np.array(names)
    fx["meta/param_shapes"] = np.array(json.dumps([list(p.shape) for _, p in model.named_parameters()]))
    fx["meta/shape"] = np.array([BV, BL, S, c["seed"]], np.int64)
    print(f"[{name}] loss {loss.item():.6f} (fp64 {loss64.item():.6f}) " + " ".join(f"{k}={v:.6f}" for k, v in model.logged.items() if "action" in k))
    np.savez_compressed(os.path.join(outdir, name + ".npz"), **fx)


def run_val(name, c, outdir):
    """lmp_val of both modalities (hulc.py:301-388) with the four uniform draws of LogisticDecoderRNN._sample recorded (as tools/gen_golden_val.py)."""
    batch = case_batch(c)
    rb = to_ref_batch(batch)
    model = build(c)
    load_params(model, case_params(c))
    fx = {"meta/shape": np.array([BV, BL, S, c["seed"]], np.int64)}
    torch.manual_seed(4321 + c["seed"])
    with torch.no_grad():
        for sc, db in rb.items():
            emb = model.perceptual_encoder(db["rgb_obs"], db["depth_obs"], db["robot_obs"])
            goal = model.language_goal(db["lang"]) if "lang" in sc else model.visual_goal(emb[:, -1])
            with RandRecorder() as rr:
                (plan_pp, loss_pp, plan_pr, loss_pr, kl, mae_pp, mae_pr, sr_pp, sr_pr, seq_feat) = model.lmp_val(emb, goal, db["actions"], db["state_info"]["robot_obs"])
            assert len(rr.draws) == 4, len(rr.draws)
            B = emb.shape[0]
            fx[f"plan_idx_pp_{sc}"] = plan_pp.reshape(B, 32, 32).argmax(-1).numpy().astype(np.int32)
            fx[f"plan_idx_pr_{sc}"] = plan_pr.reshape(B, 32, 32).argmax(-1).numpy().astype(np.int32)
            fx[f"u_mix_pp_{sc}"], fx[f"u_act_pp_{sc}"], fx[f"u_mix_pr_{sc}"], fx[f"u_act_pr_{sc}"] = rr.draws
            for k, v in (("action_loss_pp", loss_pp), ("action_loss_pr", loss_pr), ("kl_loss", kl), ("gripper_sr_pp", sr_pp), ("gripper_sr_pr", sr_pr)):
                fx[f"{k}_{sc}"] = np.float32(v.item())
            fx[f"mae_pp_{sc}"] = mae_pp.numpy()
            fx[f"mae_pr_{sc}"] = mae_pr.numpy()
            print(f"[{name}/{sc}] loss_pp {loss_pp.item():.6f} loss_pr {loss_pr.item():.6f} kl {kl.item():.6f} sr {sr_pp.item():.3f}/{sr_pr.item():.3f}")
    np.savez_compressed(os.path.join(outdir, name + ".npz"), **fx)


def run_rollout(c, outdir):
    """reset / step (hulc.py:843-957) across one replan: a vision-goal rollout, then a language-goal rollout with the same weights; the two uniform draws of
    every step are recorded."""
    nsteps, rf = c["nsteps"], c["replan_freq"]
    model = build(c)
    load_params(model, case_params(c))
    model.replan_freq = rf
    frames = rollout_frames(c)
    vis, lang = frames["vis"], frames["lang"]
    fx = {"meta": np.array([nsteps, rf, c["seed"]], np.int64)}
    model.lang_embeddings = {"do the task": lang["lang"][0:1].reshape(1, 1, 384)}
    torch.manual_seed(99 + c["seed"])
    for mode, mb in (("vis", vis), ("lang", lang)):
        model.reset()
        if mode == "vis":
            goal = dict(rgb_obs=dict(rgb_static=torch.from_numpy(mb["rgb_static"][:, nsteps:nsteps + 1]), rgb_gripper=torch.from_numpy(mb["rgb_gripper"][:, nsteps:nsteps + 1])),
                        depth_obs={}, robot_obs=torch.zeros(1, 1, 8))
        else:
            goal = "do the task"
        acts, plans, umix, uact = [], [], [], []
        for t in range(nsteps):
            obs = dict(rgb_obs=dict(rgb_static=torch.from_numpy(mb["rgb_static"][:, t:t + 1]), rgb_gripper=torch.from_numpy(mb["rgb_gripper"][:, t:t + 1])),
                       depth_obs={}, robot_obs=torch.zeros(1, 1, 8), robot_obs_raw=torch.from_numpy(mb["robot_obs"][:, t:t + 1]))
            with RandRecorder() as rr:
                a = model.step(obs, goal)
            assert len(rr.draws) == 2
            assert model.action_decoder.hidden_state is None, "mlp_decoder returns h_n = None: act() keeps no state"
            umix.append(rr.draws[0]); uact.append(rr.draws[1])
            plans.append(model.plan.reshape(1, 32, 32).argmax(-1).numpy().astype(np.int32))
            acts.append(a.detach().numpy().copy())
        fx[f"actions_{mode}"] = np.concatenate(acts, 1)          # (1, nsteps, 7)
        fx[f"plan_idx_{mode}"] = np.stack(plans, 0)              # (nsteps, 1, 32): the plan in force at each step
        fx[f"u_mix_{mode}"] = np.stack(umix, 0)
        fx[f"u_act_{mode}"] = np.stack(uact, 0)
        print(f"[{c['name']}/{mode}] actions[0] {fx[f'actions_{mode}'][0, 0].round(3)}")
    np.savez_compressed(os.path.join(outdir, c["name"] + ".npz"), **fx)


def run_manifest(outdir):
    out = {}
    for name, c in MLP_CASES.items():
        model = build(c)
        params = {n for n, _ in model.named_parameters()}
        entries = {}
        for k, v in model.state_dict().items():
            e = dict(shape=list(v.shape), dtype=str(v.dtype).replace("torch.", ""), param=k in params)
            if k not in params and v.numel() <= 512:
                e["value"] = v.detach().reshape(-1).tolist()
            entries[k] = e
        out[name] = dict(kind=c["kind"], state_dict=entries, order=[n for n, _ in model.named_parameters()], n_params=sum(int(p.numel()) for p in model.parameters()))
    json.dump(out, open(os.path.join(outdir, "state_manifest_mlp.json"), "w"), indent=0, sort_keys=True)
    print("state_manifest_mlp.json:", {k: len(v["state_dict"]) for k, v in out.items()}, "keys")


if __name__ == "__main__":
    out = os.path.join(ROOT, "tests", "golden")
    only = sys.argv[1:]
    for name, c in MLP_CASES.items():
        if not only or name in only:
            run_case(name, c, out)
    for name, c in VAL_MLP_CASES.items():
        if not only or name in only:
            run_val(name, c, out)
    if not only or ROLLOUT_MLP["name"] in only:
        run_rollout(ROLLOUT_MLP, out)
    if not only or "manifest" in only:
        run_manifest(out)
