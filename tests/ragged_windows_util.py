"""Shared helpers of the ragged-encoder-pass tests (hulc_batch::window_len_host): the batch builders, step runner and comparisons of
tests/test_gpu_store_windows.py restated (_padded_index, _modality, _step, _engine, _same_loss), plus the numpy statement of the three row kernels.
Nothing here needs a device at import time."""
import numpy as np
import torch

DET = dict(fused_transformer=0)      # bf16 step comparisons: see tests/test_gpu_store_windows.py (the fused transformer's fp32 atomics make identical runs differ)
B1 = 4                               # windows of the small case


def t(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a) if dt is None else np.ascontiguousarray(a, dt)).cuda()


def stores(F, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (F, 200, 200, 3), dtype=np.uint8), rng.integers(0, 256, (F, 84, 84, 3), dtype=np.uint8), rng


def plan(lens, S, F):
    """The contract's host arithmetic, written out here (the test of frame_store.ragged_plan compares against literals, not against this)."""
    L = np.clip(np.asarray(lens, np.int64), 1, min(S, F)).astype(np.int32)
    off = np.zeros(len(L) + 1, np.int32)
    off[1:] = np.cumsum(L)
    return L, off, int(off[-1])


def compact_tables(starts, L, off, S, F, sh_s, sh_g, off_base=0):
    """window_compact_kernel in numpy: (frame [N'], shift_static [N'][2], shift_gripper [N'][2])."""
    n = int(L.sum())
    frame, o_s, o_g = np.zeros(n, np.int64), np.zeros((n, 2), np.int32), np.zeros((n, 2), np.int32)
    for b in range(len(L)):
        s0 = min(max(int(starts[b]), 0), F - int(L[b]))
        for u in range(int(L[b])):
            r = int(off[b]) - off_base + u
            frame[r], o_s[r], o_g[r] = s0 + u, sh_s[b * S + u], sh_g[b * S + u]
    return frame, o_s, o_g


def expand_rows(src, L, off, S):
    """rows_expand_kernel in numpy: [B*S][n] from [N'][n]."""
    idx = np.concatenate([off[b] + np.minimum(np.arange(S), L[b] - 1) for b in range(len(L))])
    return src[idx]


def reduce_rows(src, L, off, S, dtype=np.float32):
    """rows_reduce_kernel in numpy: [N'][n] from [B*S][n], the duplicates' rows added to the last real row in ascending t, accumulated in `dtype`."""
    out = np.zeros((int(off[-1]), src.shape[1]), dtype)
    for b in range(len(L)):
        rows = src[b * S:(b + 1) * S].astype(dtype)
        out[off[b]:off[b] + L[b] - 1] = rows[:L[b] - 1]
        acc = rows[L[b] - 1].copy()
        for u in range(L[b], S):
            acc = (acc + rows[u]).astype(dtype)
        out[off[b] + L[b] - 1] = acc
    return out


def modality(dims_batch, store_s, store_g, starts, lens, S, rng, lang=None, shifts=True):
    """(padded, ragged) store batches of one modality: the same store, starts, lens, shifts, actions and plan draw; the ragged one adds the host lens."""
    B = len(starts)
    pad = dict(actions=t(dims_batch["actions"], np.float32), robot_obs=t(dims_batch["robot_obs"], np.float32), plan_idx=t(dims_batch["plan_idx"], np.int32),
               pad_static=10, pad_gripper=4, rgb_static=t(store_s), rgb_gripper=t(store_g), window_start=t(starts), window_len=t(lens, np.int32))
    if lang is not None:
        pad.update(lang=t(lang, np.float32), aux_rows=np.arange(B, dtype=np.int32))
    if shifts:
        pad.update(shift_static=t(rng.integers(0, 21, (B * S, 2)).astype(np.int32)), shift_gripper=t(rng.integers(0, 9, (B * S, 2)).astype(np.int32)))
    return pad, dict(pad, window_len_host=np.asarray(lens, np.int32).copy())


def step(eng, mb, mb_lang=None):
    eng.zero_grads()
    if mb_lang is None:
        l = eng.forward_loss(mb, False, 1.0, 3.0, step=0)
    else:
        lv, ll = eng.forward_loss_pair(mb, mb_lang, 0.5, 3.0, step=0)
        l = {**{"vis_" + k: v for k, v in lv.items()}, **{"lang_" + k: v for k, v in ll.items()}}
    frames = eng.encoder_frames()
    eng.backward()
    torch.cuda.synchronize()
    return l, eng.flat_grads.clone(), frames


def engine(dims, P, B, S, dtype, **options):
    from hulc_amd.engine import StepEngine
    eng = StepEngine(dims, B, S, dtype=dtype, device="cuda:0", dropout_p=0.0, seed=1)
    for k, v in options.items():
        eng.set_option(k, v)
    eng.load_numpy(P)
    return eng


def same_loss(a, b, dtype):
    if dtype == "fp32":
        return all(a[k] == b[k] for k in a)
    return all(abs(a[k] - b[k]) <= 1e-5 * abs(a[k]) + 1e-7 for k in a)


def small_case(seed, lens=None):
    """hulc_tiny, B = 4, S = 4, F = 17, lens [1, S, S-1, 2]; starts: out of range, 0, ending on the store's last frame, an overlapping one.  N' = 10."""
    from golden_util import load_case
    from hulc_amd.utils import synthetic
    dims, P, _, _ = load_case("hulc_tiny")
    S = 4
    batch = synthetic.make_batch(B1, B1, S, seed=seed, edge_frac=0.05, aux_mask="all")
    rng0 = np.random.default_rng(seed + 100)
    for sc in batch:
        batch[sc]["plan_idx"] = rng0.integers(0, 32, (B1, 32)).astype(np.int32)
    F = 3 * S + 5
    store_s, store_g, rng = stores(F, seed)
    lens = np.array([1, S, S - 1, 2], np.int32) if lens is None else np.asarray(lens, np.int32)
    starts = np.array([F + 100, 0, F - (S - 1), 5], np.int64)
    return dims, P, batch, S, F, store_s, store_g, rng, starts, lens


def encoder_split(eng):
    """([(name, offset, numel)] of the perceptual_encoder.* tensors, boolean mask of their elements in the flat gradient)."""
    enc = [(n, off, int(np.prod(shape))) for n, (off, shape) in eng.layout.items() if n.startswith("perceptual_encoder.")]
    mask = torch.zeros(eng.flat_grads.numel(), dtype=torch.bool, device=eng.flat_grads.device)
    for _, off, k in enc:
        mask[off:off + k] = True
    return enc, mask


def rel(a, b):
    """|a - b| / |b| in float64."""
    return ((a.double() - b.double()).norm() / b.double().norm()).item()
