"""Generate tests/golden/clip_rows72.npz by running the UNMODIFIED reference on CPU: the one fixture with more than 64 rows flagged by
use_for_aux_lang_loss (hulc, 1 vis + 72 lang windows of 2 frames, CLIP loss, seed 41; every lang row except b % 12 == 5 is flagged: 66 rows).

Run in the build container only:  python tools/gen_golden_rows.py
Like tools/gen_golden.py, but it records no stage activations (they would make the file 2.7 MB): the losses, the logged values, the plan sample the
reference drew, the fp32 gradient entries and the parameters after one Adam step, and the gradient entries of a float64 evaluation with the same plan
sample.  The case and the flag rule live in tests/aux_rows_util.py, which the tests read too.
"""
from __future__ import annotations

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
from aux_rows_util import ROWS_CASE, rows_case_inputs  # noqa: E402
from gen_golden import FULL_MAX, sample_idx, to_ref_batch  # noqa: E402


def load_params(model, P, double=False):
    with torch.no_grad():
        for n, p in model.named_parameters():
            t = torch.from_numpy(P[n]).reshape(p.shape)
            p.copy_(t.double() if double else t)


def main(outdir):
    c = ROWS_CASE
    dims, P, batch = rows_case_inputs(c)
    assert int(batch["lang"]["use_for_aux"].sum()) == 66 and batch["lang"]["use_for_aux"].shape == (72,)
    model = ref_harness.build_reference(c["kind"], max_window=32, use_clip=c["use_clip"]).eval()
    assert set(n for n, _ in model.named_parameters()) == set(P)
    load_params(model, P)
    scope_order = list(batch)
    rec, calls = {}, {"i": 0}
    orig_loss = model.action_decoder.loss

    def loss_hook(latent_plan, perceptual_emb, latent_goal, actions, robot_obs):      # the plan the reference samples
        sc = scope_order[calls["i"]]
        calls["i"] += 1
        rec[f"plan_idx_{sc}"] = latent_plan.detach().reshape(latent_plan.shape[0], 32, 32).argmax(-1).numpy()
        return orig_loss(latent_plan, perceptual_emb, latent_goal, actions, robot_obs)

    model.action_decoder.loss = loss_hook
    torch.manual_seed(1234 + c["seed"])
    opt = torch.optim.Adam(model.parameters(), lr=2e-4)
    rb = to_ref_batch(batch)
    loss = model.training_step(rb, 0)
    opt.zero_grad()
    loss.backward()
    fx = {"loss_total": np.float32(loss.item())}
    for k, v in model.logged.items():
        fx["log/" + k] = np.float32(v)
    fx.update(rec)
    for n, p in model.named_parameters():
        if p.grad is None:
            fx[f"gradnone/{n}"] = np.int32(1)
            continue
        g = p.grad.detach().numpy()
        fx[f"gradnorm/{n}"] = np.float64(np.sqrt((g.astype(np.float64) ** 2).sum()))
        if g.size <= FULL_MAX:
            fx[f"grad/{n}"] = g.copy()
        else:
            fx[f"gradsamp/{n}"] = g.reshape(-1)[sample_idx(n, g.size)]
    opt.step()
    for n, p in model.named_parameters():
        flat = p.detach().numpy().reshape(-1)
        fx[f"adam1/{n}"] = flat.copy() if flat.size <= FULL_MAX else flat[sample_idx(n, flat.size)]
    fx["meta"] = np.array([c["Bv"], c["Bl"], c["S"], int(c["use_clip"]), c["seed"]], np.int64)

    # float64 evaluation of the same unmodified reference with the recorded plan sample (tools/gen_golden.py: grad64/ gradsamp64/ gradnorm64/)
    import torch.distributions as D
    model64 = ref_harness.build_reference(c["kind"], max_window=32, use_clip=c["use_clip"]).eval().double()
    load_params(model64, P, double=True)
    it = {"i": 0}
    orig_rs = D.Independent.rsample

    def rs(self, sample_shape=torch.Size()):
        sc = scope_order[it["i"] % len(scope_order)]
        it["i"] += 1
        probs = self.base_dist.probs
        onehot = torch.nn.functional.one_hot(torch.from_numpy(fx[f"plan_idx_{sc}"]).long(), probs.shape[-1]).to(probs.dtype)
        return onehot + probs - probs.detach()

    def cast(x, key=""):          # actions / robot_obs stay fp32, as in tools/gen_golden.py
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
    for n, p in model64.named_parameters():
        if p.grad is None:
            continue
        g = p.grad.detach().numpy()
        fx[f"gradnorm64/{n}"] = np.float64(np.sqrt((g ** 2).sum()))
        if g.size <= FULL_MAX:
            fx[f"grad64/{n}"] = g.astype(np.float32)
        else:
            fx[f"gradsamp64/{n}"] = g.reshape(-1)[sample_idx(n, g.size)].astype(np.float32)
    path = os.path.join(outdir, c["name"] + ".npz")
    np.savez_compressed(path, **fx)
    print(f"[{c['name']}] fp32 loss {loss.item():.8f} fp64 loss {loss64.item():.8f}; {os.path.getsize(path)} bytes")

    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import hulc_oracle as O
    for sc in scope_order:
        batch[sc]["plan_idx"] = fx[f"plan_idx_{sc}"]
    losses, _ = O.training_step(P, dims, batch)
    print(f"[{c['name']}] oracle loss {float(losses['total']):.8f} clip {float(losses['clip']):.8f}")


if __name__ == "__main__":
    out = os.path.join(ROOT, "tests", "golden")
    os.makedirs(out, exist_ok=True)
    main(out)
