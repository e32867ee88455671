"""CPU: the host side of the language auxiliary losses on more than 64 flagged rows — the C-ABI declares and exports the three per-kernel entries, and
the numpy oracle reproduces the one reference fixture with 66 flagged rows (tests/golden/clip_rows72.npz, tools/gen_golden_rows.py), which pins the
yardstick the GPU tests of tests/test_gpu_aux_rows.py use."""
import ctypes as C
import os
import re

import numpy as np

import hulc_oracle as O
from aux_rows_util import CLIP_BETA, ROOT, clip_loss64, cosine_dist64, flag_rule, load_rows_case, mia_head64

ENTRIES = ("hulc_k_clip_loss", "hulc_k_clip_loss_fp32", "hulc_k_mia_head", "hulc_k_cosine_dist")


def test_header_declares_and_library_exports_the_kernel_entries():
    from hulc_amd import lib as L
    hdr = open(os.path.join(ROOT, "include", "hulc_hip.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in L.EXPORTS, name
    lib = C.CDLL(L.LIB_PATH)          # the symbols resolve without a device
    for name in ENTRIES:
        assert getattr(lib, name) is not None


def test_oracle_reproduces_the_fixture_with_66_flagged_rows():
    dims, P, batch, fx = load_rows_case()
    mask = batch["lang"]["use_for_aux"]
    assert mask.shape == (72,) and int(mask.sum()) == 66 and np.array_equal(mask, flag_rule(72)) and not mask[5] and mask[6]
    assert list(fx["meta"]) == [1, 72, 2, 1, 41]
    assert not any(k.startswith(("emb_", "seq_feat_", "goal_", "pr_logits_", "means_")) for k in fx.files)          # no stage activations: the file stays small
    losses, _ = O.training_step(P, dims, batch, want_grads=False)
    ref = float(fx["loss_total"])
    print(f"[clip_rows72] oracle {float(losses['total']):.6f} reference fp32 {ref:.6f} fp64 {float(fx['loss_total_fp64']):.6f}")
    assert abs(float(losses["total"]) - ref) <= 2e-5 * abs(ref)                                  # the gates of tests/test_oracle_golden.py
    assert abs(float(losses["total"]) - float(fx["loss_total_fp64"])) <= 2e-5 * abs(ref)
    assert abs(float(losses["clip"]) - float(fx["log/train/lang_clip_loss"])) < 3e-5
    for sc in batch:
        assert abs(float(losses[f"action_{sc}"]) - float(fx[f"log/train/action_loss_{sc}"])) < 3e-5
        assert abs(float(losses[f"kl_{sc}"]) - float(fx[f"log/train/kl_loss_scaled_{sc}"])) < 1e-6


def test_float64_restatements_agree_with_autograd():
    """The restatements the kernel-level GPU tests compare against, checked here against torch autograd in float64."""
    import torch
    rng = np.random.default_rng(0)
    n = 7
    img, txt = rng.standard_normal((n, 32)), rng.standard_normal((n, 32))
    ti, tt, ls = torch.tensor(img, requires_grad=True), torch.tensor(txt, requires_grad=True), torch.tensor(1.3, dtype=torch.float64, requires_grad=True)
    a, b = ti / ti.norm(dim=1, keepdim=True), tt / tt.norm(dim=1, keepdim=True)
    lg = ls.exp() * a @ b.T
    lab = torch.arange(n)
    loss = (torch.nn.functional.cross_entropy(lg, lab) + torch.nn.functional.cross_entropy(lg.T, lab)) / 2
    (CLIP_BETA * loss).backward()
    got = clip_loss64(img, txt, 1.3, CLIP_BETA)
    for g, r in zip(got, (loss.item(), ti.grad.numpy(), tt.grad.numpy(), ls.grad.item())):
        assert np.allclose(g, r, rtol=1e-10, atol=1e-12)
    W0, b0, W1, b1 = rng.standard_normal((512, 64)) / 8, rng.standard_normal(512) / 10, rng.standard_normal((1, 512)) / 16, np.array([0.05])
    T = [torch.tensor(x, requires_grad=True) for x in (img, txt, W0, b0, W1, b1)]
    D = lambda x: torch.relu(x @ T[2].T + T[3]) @ T[4].T + T[5]
    z = torch.cat([D(torch.cat([T[0], T[1]], 1)), D(torch.cat([T[0], torch.roll(T[1], 1, 0)], 1))], 0)
    y = torch.cat([torch.ones(n, 1), torch.zeros(n, 1)], 0).double()
    loss = torch.nn.functional.binary_cross_entropy_with_logits(z, y)
    (2.0 * loss).backward()
    got = mia_head64(img, txt, W0, b0, W1, b1, 2.0)
    assert np.allclose(got[0], loss.item(), rtol=1e-12)
    for g, t in zip(got[1:], T):
        assert np.allclose(g, t.grad.numpy().reshape(g.shape), rtol=1e-9, atol=1e-12)
    p, t = rng.standard_normal((n, 384)), rng.standard_normal((n, 384))
    tp = torch.tensor(p, requires_grad=True)
    loss = (1 - torch.nn.functional.cosine_similarity(tp, torch.tensor(t), dim=1, eps=0.0)).mean()
    (2.0 * loss).backward()
    got = cosine_dist64(p, t, 2.0)
    assert np.allclose(got[0], loss.item(), rtol=1e-12) and np.allclose(got[1], tp.grad.numpy(), rtol=1e-9, atol=1e-14)
