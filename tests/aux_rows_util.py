"""Helpers of the tests of the language auxiliary losses on more than 64 flagged rows (tests/test_gpu_aux_rows.py, tests/test_aux_rows_host.py):
the case of the one reference fixture (tests/golden/clip_rows72.npz, written by tools/gen_golden_rows.py = the unmodified reference), the flag rule it
shares with the generator, float64 numpy restatements of the three loss kernels, and the torch restatements of the MIA / BC-Z heads (as in
tests/test_gpu_aux_losses.py, copied so that no test module depends on another)."""
import os

import numpy as np

from hulc_amd import spec
from hulc_amd.utils import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP_BETA = 3.0
# the fixture's case: hulc, 1 vis window, 72 lang windows of 2 frames, CLIP loss, seed 41
ROWS_CASE = dict(name="clip_rows72", kind="hulc", Bv=1, Bl=72, S=2, use_clip=True, seed=41, edge_frac=0.05)


def flag_rule(B):
    """use_for_aux_lang_loss of the > 64-row cases: every row except b % 12 == 5 (72 rows -> 66 flagged, not contiguous)."""
    return (np.arange(B) % 12) != 5


def rows_case_inputs(c=ROWS_CASE):
    dims = spec.ModelDims(kind=c["kind"], max_window=32, use_clip=c["use_clip"])
    P = spec.init_all(dims, seed=c["seed"], ln_jitter=True)
    batch = synthetic.make_batch(c["Bv"], c["Bl"], c["S"], seed=c["seed"], edge_frac=c["edge_frac"], aux_mask="all")
    batch["lang"]["use_for_aux"] = flag_rule(c["Bl"])
    return dims, P, batch


def load_rows_case():
    dims, P, batch = rows_case_inputs()
    fx = np.load(os.path.join(ROOT, "tests", "golden", ROWS_CASE["name"] + ".npz"))
    for sc in batch:
        if f"plan_idx_{sc}" in fx.files:
            batch[sc]["plan_idx"] = fx[f"plan_idx_{sc}"]
    return dims, P, batch, fx


# ---------------------------------------------------------------------------------------------------------------- float64 restatements of the kernels
def clip_loss64(img, txt, logit_scale, w):
    """hulc.py:679-695 in float64 on the given fp32 inputs: loss, dimg, dtxt (times w), d logit_scale (times w)."""
    img, txt = np.asarray(img, np.float64), np.asarray(txt, np.float64)
    n = img.shape[0]
    ni, nt = np.linalg.norm(img, axis=1, keepdims=True), np.linalg.norm(txt, axis=1, keepdims=True)
    a, b = img / ni, txt / nt
    s = np.exp(np.float64(logit_scale))
    cos = a @ b.T
    L = s * cos

    def lse(x, axis):
        m = x.max(axis, keepdims=True)
        return m + np.log(np.exp(x - m).sum(axis, keepdims=True))

    rl, cl = lse(L, 1), lse(L, 0)
    d = np.diag(L)
    loss = ((rl[:, 0] - d).sum() + (cl[0] - d).sum()) / (2 * n)
    g = ((np.exp(L - rl) - np.eye(n)) + (np.exp(L - cl) - np.eye(n))) / (2 * n)
    da, db = s * g @ b, s * g.T @ a
    dimg = w * (da - a * (a * da).sum(1, keepdims=True)) / ni
    dtxt = w * (db - b * (b * db).sum(1, keepdims=True)) / nt
    return loss, dimg, dtxt, w * (g * cos).sum() * s


def mia_head64(img, txt, W0, b0, W1, b1, w, shift=1):
    """BCE with logits of D([img | txt]) (label 1) and D([img | roll(txt, shift)]) (label 0), D = W1 relu(W0 x + b0) + b1, in float64:
    loss (unweighted), dimg, dtxt, dW0, db0, dW1, db1 (times w)."""
    img, txt, W0, b0, W1, b1 = (np.asarray(x, np.float64) for x in (img, txt, W0, b0, W1, b1))
    n = img.shape[0]
    neg = np.roll(txt, shift, 0)
    x = np.concatenate([np.concatenate([img, txt], 1), np.concatenate([img, neg], 1)], 0)
    y = np.concatenate([np.ones(n), np.zeros(n)])
    h = x @ W0.T + b0
    r = np.maximum(h, 0)
    z = r @ W1.reshape(-1) + b1.reshape(())
    loss = (np.maximum(z, 0) - z * y + np.log1p(np.exp(-np.abs(z)))).mean()
    dz = w * (1 / (1 + np.exp(-z)) - y) / (2 * n)
    dh = (dz[:, None] * W1.reshape(1, -1)) * (h > 0)
    dx = dh @ W0
    dimg = dx[:n, :32] + dx[n:, :32]
    dtxt = dx[:n, 32:] + np.roll(dx[n:, 32:], -shift, 0)
    return loss, dimg, dtxt, dh.T @ x, dh.sum(0), (dz[:, None] * r).sum(0).reshape(W1.shape), np.array([dz.sum()])


def cosine_dist64(pred, tgt, w):
    p, t = np.asarray(pred, np.float64), np.asarray(tgt, np.float64)
    n = p.shape[0]
    pt, np_, nt = (p * t).sum(1, keepdims=True), np.linalg.norm(p, axis=1, keepdims=True), np.linalg.norm(t, axis=1, keepdims=True)
    loss = (1 - pt / (np_ * nt)).mean()
    return loss, -(w / n) * (t / (np_ * nt) - pt * p / (np_ ** 3 * nt))


def kernel_rows(n, seed):
    """(n, 32) img / txt rows for the kernel-level tests: row norms spread over 0.1 .. 10 and one near-duplicate pair (rows 1 and n - 2)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(2):
        x = rng.standard_normal((n, 32))
        x *= (10.0 ** rng.uniform(-1, 1, (n, 1))) / np.linalg.norm(x, axis=1, keepdims=True)
        x[n - 2] = x[1] * (1 + 1e-3) + 1e-4 * rng.standard_normal(32) * np.linalg.norm(x[1])
        out.append(x.astype(np.float32))
    return out


# ---------------------------------------------------------------------------------------------------------------- engine helpers
def to_dev(mb):
    import torch
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
    """zero_grads, then one forward + backward per modality; returns train/total_loss as the reference adds it up (hulc.py:491-537) and the loss dicts."""
    eng.zero_grads()
    per = {}
    for sc, mb in batch.items():
        per[sc] = eng.forward_loss(to_dev(mb), "lang" in sc, 1.0 / len(batch), CLIP_BETA, step=step)
        eng.backward()
    tot = sum(l["total_mod"] for l in per.values()) / len(batch)
    for l in per.values():
        tot += (CLIP_BETA * l["clip"] if eng.dims.use_clip else 0.0) + l.get("bc_z", 0.0) + l.get("mia", 0.0)
    return tot, per


def grads_np(eng):
    return {n: t.detach().cpu().numpy() for n, t in eng.views(eng.flat_grads).items()}


# ---------------------------------------------------------------------------------------------------------------- torch restatements of the heads
def _t(P, n):
    import torch
    return torch.from_numpy(np.asarray(P[n], np.float64)).requires_grad_(True)


def _lin(x, W, b):
    return x @ W.T + b


def bcz_restated(P, sf, lang):
    """mean(1 - cos(mlp(seq_feat[rows]), lang[rows])), plain quotient; returns loss, {head name: tensor}, the seq_feat leaf."""
    import torch
    names = [f"bc_z_lang_decoder.mlp.{i}.{k}" for i in (0, 2) for k in ("weight", "bias")]
    T = {n: _t(P, n) for n in names}
    sf = torch.from_numpy(sf.astype(np.float64)).requires_grad_(True)
    tg = torch.from_numpy(lang.astype(np.float64))
    pred = _lin(torch.relu(_lin(sf, T[names[0]], T[names[1]])), T[names[2]], T[names[3]])
    cos = (pred * tg).sum(-1) / (torch.linalg.norm(pred, dim=1) * torch.linalg.norm(tg, dim=1))
    return (1 - cos).mean(), T, sf


def mia_restated(P, sf, goal, shift=1):
    """BCE with logits over D([img | txt]) (label 1) and D([img | roll(txt, shift)]) (label 0); returns loss, {name: tensor}, the seq_feat and goal leaves."""
    import torch
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
