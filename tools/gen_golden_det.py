"""Generate tests/golden/det_*.npz, val_det_hulc.npz, rollout_det_hulc.npz and state_manifest_det.json: the UNMODIFIED reference with
model/action_decoder=deterministic (hulc.models.decoders.deterministic_decoder.DeterministicDecoder), on CPU, eval mode, with the recorded plan sample.

The reference module cannot be instantiated as it stands: its constructor does eval(rnn_model) and never imports rnn_decoder (a NameError).  The name is
bound in the imported module's namespace at run time (bind_rnn_decoder below) — no file of the reference is edited or copied.

Run in the build container only:  python tools/gen_golden_det.py [case ...]
Format as tools/gen_golden_aux.py: inputs and parameters by name (tests/det_golden_util.py regenerates them), the reference's losses and logged values,
per-parameter gradients (full up to 4096 elements, else norm + 64 samples), parameters after one Adam step, the float64 run's gradients (grad64/), the
parameter table, and the decoder's last hidden states (dec_h1_<scope>, what tests/det_head_ref.py restates the loss from).
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
from gen_golden_val import load_params  # noqa: E402
from gen_golden_aux import record_grads  # noqa: E402
from det_golden_util import (BL, BV, DET_CASES, HEAD_SCALE, ROLLOUT_DET, S, SCALE_LADDER, VAL_DET_CASES, case_batch, case_dims, case_params,  # noqa: E402
                             rollout_frames)


def bind_rnn_decoder():
    ref_harness.install_stubs()
    import hulc.models.decoders.deterministic_decoder as DD
    from hulc.models.decoders.utils.rnn import rnn_decoder
    DD.rnn_decoder = rnn_decoder


def build(c, double=False):
    """conf/model/hulc.yaml with model/action_decoder=deterministic, resolved (conf/model/action_decoder/deterministic.yaml)."""
    bind_rnn_decoder()
    cfg = ref_harness.model_cfg("hulc", max_window=32, use_clip=True)
    cfg["action_decoder"] = ref_harness.to_cfg(dict(
        _target_="hulc.models.decoders.deterministic_decoder.DeterministicDecoder", hidden_size=2048, out_features=7, policy_rnn_dropout_p=0.0,
        perceptual_features=None, latent_goal_features=32, plan_features=None, criterion=c["criterion"], num_layers=2, rnn_model="rnn_decoder",
        perceptual_emb_slice=[64, 128], gripper_control=True))
    from hulc.models.hulc import Hulc
    m = Hulc(**cfg).eval()
    return m.double() if double else m


def residual_counts(c, scale):
    """(#|d| > 1.2, #|d| < 0.8) of the training residuals tanh(head) - actions of the reference at this head scale."""
    batch = case_batch(c)
    rb = to_ref_batch(batch)
    model = build(c)
    load_params(model, case_params(c, scale))
    ds = []
    orig = model.action_decoder.forward

    def fwd(*a, **k):
        out = orig(*a, **k)
        ds.append(out[0].detach())
        return out

    model.action_decoder.forward = fwd
    torch.manual_seed(1234 + c["seed"])
    with torch.no_grad():
        model.training_step(rb, 0)
    d = torch.cat([(p - db["actions"]).reshape(-1) for p, db in zip(ds, rb.values())]).abs().numpy()
    return int((d > 1.2).sum()), int((d < 0.8).sum()), d.size


def check_scale():
    c = DET_CASES["det_huber_hulc"]
    chosen = None
    for f in SCALE_LADDER:
        hi, lo, n = residual_counts(c, f)
        print(f"[scale {f:g}] {hi} of {n} residuals above 1.2, {lo} below 0.8")
        if chosen is None and hi >= 10 and lo >= 10:
            chosen = f
    assert chosen == HEAD_SCALE, f"det_golden_util.HEAD_SCALE must be {chosen} (the smallest factor of the ladder with 10 residuals on each side)"


def run_case(name, c, outdir):
    batch = case_batch(c)
    rb = to_ref_batch(batch)
    P = case_params(c)
    model = build(c)
    names = [n for n, _ in model.named_parameters()]
    assert set(names) == set(P.keys()), set(names) ^ set(P.keys())
    load_params(model, P)
    scope_order = list(batch.keys())
    rec, calls, hcalls = {}, {"i": 0}, {"i": 0}
    orig_loss = model.action_decoder.loss

    def loss_hook(latent_plan, perceptual_emb, latent_goal, actions, robot_obs):
        sc = scope_order[calls["i"] % len(scope_order)]
        calls["i"] += 1
        rec[f"plan_idx_{sc}"] = latent_plan.detach().reshape(latent_plan.shape[0], 32, 32).argmax(-1).numpy()
        return orig_loss(latent_plan, perceptual_emb, latent_goal, actions, robot_obs)

    def rnn_hook(module, inp, out):
        sc = scope_order[hcalls["i"] % len(scope_order)]
        hcalls["i"] += 1
        rec[f"dec_h1_{sc}"] = out[0].detach().numpy().astype(np.float32)          # (B, S, 2048)

    model.action_decoder.loss = loss_hook
    model.action_decoder.rnn.register_forward_hook(rnn_hook)
    torch.manual_seed(1234 + c["seed"])
    opt = torch.optim.Adam(model.parameters(), lr=2e-4)
    loss = model.training_step(rb, 0)
    opt.zero_grad()
    loss.backward()
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
    crit64 = model64.action_decoder.criterion      # the fp32 actions meet fp64 predictions: widen the target (exact) so that the criterion's backward sees one dtype
    crit64.register_forward_pre_hook(lambda mod, args: (args[0], args[1].to(args[0].dtype)))
    it = {"i": 0}
    orig_rs = D.Independent.rsample

    def rs(self, sample_shape=torch.Size()):
        sc = scope_order[it["i"] % len(scope_order)]
        it["i"] += 1
        probs = self.base_dist.probs
        onehot = torch.nn.functional.one_hot(torch.from_numpy(fx[f"plan_idx_{sc}"]).long(), probs.shape[-1]).to(probs.dtype)
        return onehot + probs - probs.detach()

    def cast(x, key=""):
        if isinstance(x, dict):
            return {k: cast(v, k) for k, v in x.items()}
        if key in ("actions", "state_info", "robot_obs"):      # fp32 data either way; the (discarded) tcp-frame transform of loss() builds fp32 rotation matrices
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
    fx["meta/head_scale"] = np.float64(HEAD_SCALE)
    print(f"[{name}] loss {loss.item():.6f} (fp64 {loss64.item():.6f}) " + " ".join(f"{k}={v:.6f}" for k, v in model.logged.items() if "action" in k))
    np.savez_compressed(os.path.join(outdir, name + ".npz"), **fx)


def run_val(name, c, outdir):
    """lmp_val of both modalities (hulc.py:301-388): DeterministicDecoder.loss_and_act = the criterion in the tcp frame, predictions in the world frame."""
    batch = case_batch(c)
    rb = to_ref_batch(batch)
    model = build(c)
    load_params(model, case_params(c))
    fx = {"meta/shape": np.array([BV, BL, S, c["seed"]], np.int64), "meta/head_scale": np.float64(HEAD_SCALE)}
    torch.manual_seed(4321 + c["seed"])
    with torch.no_grad():
        for sc, db in rb.items():
            emb = model.perceptual_encoder(db["rgb_obs"], db["depth_obs"], db["robot_obs"])
            goal = model.language_goal(db["lang"]) if "lang" in sc else model.visual_goal(emb[:, -1])
            (plan_pp, loss_pp, plan_pr, loss_pr, kl, mae_pp, mae_pr, sr_pp, sr_pr, seq_feat) = model.lmp_val(emb, goal, db["actions"], db["state_info"]["robot_obs"])
            B = emb.shape[0]
            fx[f"plan_idx_pp_{sc}"] = plan_pp.reshape(B, 32, 32).argmax(-1).numpy().astype(np.int32)
            fx[f"plan_idx_pr_{sc}"] = plan_pr.reshape(B, 32, 32).argmax(-1).numpy().astype(np.int32)
            for k, v in (("action_loss_pp", loss_pp), ("action_loss_pr", loss_pr), ("kl_loss", kl), ("gripper_sr_pp", sr_pp), ("gripper_sr_pr", sr_pr)):
                fx[f"{k}_{sc}"] = np.float32(v.item())
            fx[f"mae_pp_{sc}"] = mae_pp.numpy()
            fx[f"mae_pr_{sc}"] = mae_pr.numpy()
            for tag, plan in (("pp", plan_pp), ("pr", plan_pr)):      # the world-frame predictions of both passes (deterministic: a second call returns them again)
                _, act = model.action_decoder.loss_and_act(plan, emb, goal, db["actions"], db["state_info"]["robot_obs"])
                fx[f"pred_{tag}_{sc}"] = act.numpy().astype(np.float32)
            print(f"[{name}/{sc}] loss_pp {loss_pp.item():.6f} loss_pr {loss_pr.item():.6f} kl {kl.item():.6f} sr {sr_pp.item():.3f}/{sr_pr.item():.3f}")
    np.savez_compressed(os.path.join(outdir, name + ".npz"), **fx)


def run_rollout(c, outdir):
    """reset / step (hulc.py:843-957) across one replan: a vision-goal rollout, then a language-goal rollout with the same weights."""
    nsteps, rf = c["nsteps"], c["replan_freq"]
    model = build(c)
    load_params(model, case_params(c))
    model.replan_freq = rf
    frames = rollout_frames(c)
    vis, lang = frames["vis"], frames["lang"]
    fx = {"meta": np.array([nsteps, rf, c["seed"]], np.int64), "meta/head_scale": np.float64(HEAD_SCALE)}
    model.lang_embeddings = {"do the task": lang["lang"][0:1].reshape(1, 1, 384)}
    torch.manual_seed(99 + c["seed"])
    for mode, mb in (("vis", vis), ("lang", lang)):
        model.reset()
        if mode == "vis":
            goal = dict(rgb_obs=dict(rgb_static=torch.from_numpy(mb["rgb_static"][:, nsteps:nsteps + 1]), rgb_gripper=torch.from_numpy(mb["rgb_gripper"][:, nsteps:nsteps + 1])),
                        depth_obs={}, robot_obs=torch.zeros(1, 1, 8))
        else:
            goal = "do the task"
        acts, plans = [], []
        for t in range(nsteps):
            obs = dict(rgb_obs=dict(rgb_static=torch.from_numpy(mb["rgb_static"][:, t:t + 1]), rgb_gripper=torch.from_numpy(mb["rgb_gripper"][:, t:t + 1])),
                       depth_obs={}, robot_obs=torch.zeros(1, 1, 8), robot_obs_raw=torch.from_numpy(mb["robot_obs"][:, t:t + 1]))
            a = model.step(obs, goal)
            plans.append(model.plan.reshape(1, 32, 32).argmax(-1).numpy().astype(np.int32))
            acts.append(a.detach().numpy().copy())
        fx[f"actions_{mode}"] = np.concatenate(acts, 1)          # (1, nsteps, 7)
        fx[f"plan_idx_{mode}"] = np.stack(plans, 0)              # (nsteps, 1, 32): the plan in force at each step
        print(f"[{c['name']}/{mode}] actions[0] {fx[f'actions_{mode}'][0, 0].round(3)}")
    np.savez_compressed(os.path.join(outdir, c["name"] + ".npz"), **fx)


def run_manifest(outdir):
    model = build(DET_CASES["det_huber_hulc"])
    params = {n for n, _ in model.named_parameters()}
    entries = {}
    for k, v in model.state_dict().items():
        e = dict(shape=list(v.shape), dtype=str(v.dtype).replace("torch.", ""), param=k in params)
        if k not in params and v.numel() <= 512:
            e["value"] = v.detach().reshape(-1).tolist()
        entries[k] = e
    out = {"hulc_det_w32": dict(kind="hulc", state_dict=entries, n_params=sum(int(p.numel()) for p in model.parameters()))}
    json.dump(out, open(os.path.join(outdir, "state_manifest_det.json"), "w"), indent=0, sort_keys=True)
    print("state_manifest_det.json:", len(entries), "keys")


if __name__ == "__main__":
    out = os.path.join(ROOT, "tests", "golden")
    only = sys.argv[1:]
    if not only:
        check_scale()
    for name, c in DET_CASES.items():
        if not only or name in only:
            run_case(name, c, out)
    for name, c in VAL_DET_CASES.items():
        if not only or name in only:
            run_val(name, c, out)
    if not only or ROLLOUT_DET["name"] in only:
        run_rollout(ROLLOUT_DET, out)
    if not only or "manifest" in only:
        run_manifest(out)
