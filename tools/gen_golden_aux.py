"""Generate tests/golden/aux_*.npz and val_aux_*.npz: the UNMODIFIED reference with the BC-Z / MIA language auxiliary losses switched on
(model.use_bc_z_auxiliary_loss / model.use_mia_auxiliary_loss), on CPU, eval mode, with the recorded plan sample.

Run in the build container only:  python tools/gen_golden_aux.py [case ...]
Format as tools/gen_golden.py: inputs and parameters by name (tests/aux_golden_util.py regenerates them), the reference's losses and logged values,
per-parameter gradients (full up to 4096 elements, else norm + 64 samples), parameters after one Adam step, and the float64 run's gradients (grad64/).
meta/ entries: the reference's parameter table and — from this file's own torch restatement of the MIA
loss on the reference's seq_feat / latent goal — the loss with roll(+1) (= the reference), roll(-1) and no roll.
"""
from __future__ import annotations

import json
import math
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
from aux_golden_util import AUX_CASES, BL, BV, IM0, S, VAL_AUX_CASES, case_batch, case_params  # noqa: E402

LOSS_GATE = 1e-3          # the tests' gate on a loss value, relative to the reference's value
LN2 = math.log(2.0)


def build(c, double=False):
    m = ref_harness.build_reference(c["kind"], max_window=32, use_clip=c["clip"], use_bc_z=c["bcz"], use_mia=c["mia"]).eval()
    return m.double() if double else m


def mia_restatement(P, seq_feat, goal, rows, shift):
    """BCE-with-logits of the discriminator on [img | txt] and [img | roll(txt, shift)] — this file's own statement of the loss, for the roll check."""
    t = lambda n: torch.from_numpy(P[n]).double()
    sf, g = torch.from_numpy(seq_feat).double()[rows], torch.from_numpy(goal).double()[rows]
    lin = lambda x, n: x @ t(n + ".weight").T + t(n + ".bias")
    img = lin(torch.relu(lin(sf, "proj_vis_lang.mlp_im.0")), "proj_vis_lang.mlp_im.2")
    txt = lin(torch.relu(lin(g, "proj_vis_lang.mlp_lang.0")), "proj_vis_lang.mlp_lang.2")
    D = lambda a, b: lin(torch.relu(lin(torch.cat([a, b], -1), "mia_lang_discriminator.mlp.0")), "mia_lang_discriminator.mlp.3")
    neg = txt if shift == 0 else torch.roll(txt, shifts=shift, dims=0)
    z = torch.cat([D(img, txt), D(img, neg)], 0)
    y = torch.cat([torch.ones(len(rows), 1), torch.zeros(len(rows), 1)], 0).double()
    return float(torch.nn.functional.binary_cross_entropy_with_logits(z, y))


def centred_bias(c, rb, mask):
    """param overrides of a MIA case (aux_golden_util.SCALES, the case's gain): the first image-projection bias, moved so that the gain on its weight amplifies
    only the rows' differences: b' = b - (gain - 1) W mean(seq_feat[rows]) with W, b the regenerated default tensors and seq_feat the reference's own."""
    if not c["mia"]:
        return {}
    P = case_params(c)
    model = build(c)
    load_params(model, P)
    with torch.no_grad():
        db = rb["lang"]
        emb = model.perceptual_encoder(db["rgb_obs"], db["depth_obs"], db["robot_obs"])
        sf = model.plan_recognition(emb)[1].numpy()
    rows = np.nonzero(mask)[0] if mask.any() else np.arange(len(mask))
    W = P[IM0 + ".weight"].astype(np.float64) / c["gain"]
    b = P[IM0 + ".bias"].astype(np.float64) - (c["gain"] - 1.0) * (W @ sf[rows].astype(np.float64).mean(0))
    return {IM0 + ".bias": b.astype(np.float32)}


def record_grads(model, fx, tag64=False):
    for n, p in model.named_parameters():
        if p.grad is None:
            if not tag64:
                fx[f"gradnone/{n}"] = np.int32(1)
            continue
        g = p.grad.detach().numpy()
        sfx = "64" if tag64 else ""
        fx[f"gradnorm{sfx}/{n}"] = np.float64(np.sqrt((g.astype(np.float64) ** 2).sum()))
        if g.size <= FULL_MAX:
            fx[f"grad{sfx}/{n}"] = g.astype(np.float32)
        else:
            fx[f"gradsamp{sfx}/{n}"] = g.reshape(-1)[sample_idx(n, g.size)].astype(np.float32)


def run_case(name, c, outdir):
    batch = case_batch(c)
    mask = batch["lang"]["use_for_aux"]
    if c["mask"] == "some":
        assert mask.sum() >= 3 and (~mask[:-1]).any(), mask          # >= 3 flagged rows, an unflagged row that is not the last
    rb = to_ref_batch(batch)
    over = centred_bias(c, rb, mask)
    P = case_params(c, over)
    model = build(c)
    names = [n for n, _ in model.named_parameters()]
    assert set(names) == set(P.keys()), set(names) ^ set(P.keys())
    load_params(model, P)
    scope_order = list(batch.keys())
    rec, calls, pcalls = {}, {"i": 0}, {"i": 0}
    orig_loss = model.action_decoder.loss

    def loss_hook(latent_plan, perceptual_emb, latent_goal, actions, robot_obs):
        sc = scope_order[calls["i"] % len(scope_order)]
        calls["i"] += 1
        if latent_plan.shape[-1] > 0:
            rec[f"plan_idx_{sc}"] = latent_plan.detach().reshape(latent_plan.shape[0], 32, 32).argmax(-1).numpy()
        rec[f"goal_{sc}"] = latent_goal.detach().numpy().astype(np.float32)
        return orig_loss(latent_plan, perceptual_emb, latent_goal, actions, robot_obs)

    def pr_hook(module, inp, out):
        sc = scope_order[pcalls["i"] % len(scope_order)]
        pcalls["i"] += 1
        rec[f"seq_feat_{sc}"] = out[1].detach().numpy().astype(np.float32)

    model.action_decoder.loss = loss_hook
    model.plan_recognition.register_forward_hook(pr_hook)
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

    for n, v in over.items():
        fx["param/" + n] = v
    fx["meta/param_names"] = np.array(names)
    fx["meta/param_shapes"] = np.array(json.dumps([list(p.shape) for _, p in model.named_parameters()]))
    fx["meta/shape"] = np.array([BV, BL, S, c["seed"]], np.int64)
    fx["meta/mask"] = mask
    if c["mia"] and mask.any():
        rows = np.nonzero(mask)[0]
        ref = float(fx["log/train/lang_contrastive"])          # beta = 1
        plus, minus, none = (mia_restatement(P, rec["seq_feat_lang"], rec["goal_lang"], rows, s) for s in (1, -1, 0))
        print(f"[{name}] MIA: reference {ref:.6f}; restated roll(+1) {plus:.6f} roll(-1) {minus:.6f} no roll {none:.6f}")
        assert abs(plus - ref) <= LOSS_GATE * abs(ref), (plus, ref)
        assert abs(ref - LN2) > 0.05, ref
        assert abs(minus - ref) > 10 * LOSS_GATE * abs(ref) and abs(none - ref) > 10 * LOSS_GATE * abs(ref), (ref, minus, none)
        fx["meta/mia_roll_plus"], fx["meta/mia_roll_minus"], fx["meta/mia_no_roll"] = np.float64(plus), np.float64(minus), np.float64(none)
    print(f"[{name}] loss {loss.item():.6f} (fp64 {loss64.item():.6f}) " + " ".join(f"{k}={v:.6f}" for k, v in model.logged.items() if "lang" in k))
    np.savez_compressed(os.path.join(outdir, name + ".npz"), **fx)


def run_val(name, c, outdir):
    """The lang modality of Hulc.validation_step (hulc.py:770-813) with both heads; the vis modality carries no auxiliary loss."""
    batch = case_batch(c)
    rb = to_ref_batch(batch)
    over = centred_bias(c, rb, batch["lang"]["use_for_aux"])
    P = case_params(c, over)
    model = build(c)
    load_params(model, P)
    fx = {"meta/shape": np.array([BV, BL, S, c["seed"]], np.int64), "meta/mask": batch["lang"]["use_for_aux"],
          "meta/param_names": np.array([n for n, _ in model.named_parameters()]),
          "meta/param_shapes": np.array(json.dumps([list(p.shape) for _, p in model.named_parameters()]))}
    for n, v in over.items():
        fx["param/" + n] = v
    torch.manual_seed(4321 + c["seed"])
    with torch.no_grad():
        for sc, db in rb.items():
            emb = model.perceptual_encoder(db["rgb_obs"], db["depth_obs"], db["robot_obs"])
            goal = model.language_goal(db["lang"]) if "lang" in sc else model.visual_goal(emb[:, -1])
            with RandRecorder() as rr:
                (plan_pp, loss_pp, plan_pr, loss_pr, kl, mae_pp, mae_pr, sr_pp, sr_pr, seq_feat) = model.lmp_val(emb, goal, db["actions"], db["state_info"]["robot_obs"])
            B = emb.shape[0]
            fx[f"plan_idx_pp_{sc}"] = plan_pp.reshape(B, 32, 32).argmax(-1).numpy().astype(np.int32)
            fx[f"plan_idx_pr_{sc}"] = plan_pr.reshape(B, 32, 32).argmax(-1).numpy().astype(np.int32)
            fx[f"u_mix_pp_{sc}"], fx[f"u_act_pp_{sc}"], fx[f"u_mix_pr_{sc}"], fx[f"u_act_pr_{sc}"] = rr.draws
            fx[f"action_loss_pp_{sc}"] = np.float32(loss_pp.item())
            fx[f"kl_loss_{sc}"] = np.float32(kl.item())
            if "lang" in sc:
                m = db["use_for_aux_lang_loss"]
                fx["val/lang_pred_loss"] = np.float32(model.bc_z_auxiliary_loss(seq_feat, db["lang"], m).item())
                fx["val/val_pred_clip_loss"] = np.float32(model.clip_auxiliary_loss(seq_feat, goal, m).item())
                fx["val/lang_contrastive_loss"] = np.float32(model.mia_auxiliary_loss(seq_feat, goal, m).item())
    print(f"[{name}] " + " ".join(f"{k}={float(v):.6f}" for k, v in fx.items() if k.startswith("val/")))
    assert abs(float(fx["val/lang_contrastive_loss"]) - LN2) > 0.05
    np.savez_compressed(os.path.join(outdir, name + ".npz"), **fx)


if __name__ == "__main__":
    out = os.path.join(ROOT, "tests", "golden")
    only = sys.argv[1:]
    for name, c in AUX_CASES.items():
        if not only or name in only:
            run_case(name, c, out)
    for name, c in VAL_AUX_CASES.items():
        if not only or name in only:
            run_val(name, c, out)
