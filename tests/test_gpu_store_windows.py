"""GPU, through the C-ABI: variable-length windows gathered from the HBM-resident frame store and padded on the device (hulc_batch::window_len,
hulc_store_gather, FrameStore.sample_windows, CalvinStoreDataModule).  The reference pads a window of min_window_size..max_window_size frames to the
maximum by repeating its last frame after the image transform (vision.yaml / lang.yaml: pad true); its dataset code (calvin_agent) is not part of
the reference tree, so every expectation here is a plain numpy / torch materialisation of the rule written in the test itself:
batch frame (b, t) = store frame clamp(start_b, 0, F - L_b) + min(t, L_b - 1), shift (b, t) = shift[b S + min(t, L_b - 1)]."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import store_windows_util as U  # noqa: E402
from golden_util import load_case  # noqa: E402
from hulc_amd.engine import StepEngine  # noqa: E402
from hulc_amd.utils import synthetic  # noqa: E402


def t(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a) if dt is None else np.ascontiguousarray(a, dt)).cuda()


def _stores(F, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (F, 200, 200, 3), dtype=np.uint8), rng.integers(0, 256, (F, 84, 84, 3), dtype=np.uint8), rng


def _padded_index(starts, lens, S, F):
    """(B,S) store indices and (B*S,) effective batch-frame indices of padded windows — the rule of include/hulc_hip.h, in numpy."""
    L = np.clip(lens, 1, S).astype(np.int64)
    s0 = np.clip(starts, 0, F - L)
    tt = np.minimum(np.arange(S)[None, :], L[:, None] - 1)
    return s0[:, None] + tt, (np.arange(len(L))[:, None] * S + tt).reshape(-1)


def _modality(dims_batch, store_s, store_g, starts, lens, S, rng, lang=None, shifts=True):
    """(materialised batch, store + window_len batch) of one modality with the same actions / robot_obs / plan draw."""
    F, B = store_s.shape[0], len(starts)
    idx, eff = _padded_index(starts, lens, S, F)
    common = dict(actions=t(dims_batch["actions"], np.float32), robot_obs=t(dims_batch["robot_obs"], np.float32), plan_idx=t(dims_batch["plan_idx"], np.int32),
                  pad_static=10, pad_gripper=4)
    if lang is not None:
        common.update(lang=t(lang, np.float32), aux_rows=np.arange(B, dtype=np.int32))
    mat = dict(common, rgb_static=t(store_s[idx.reshape(-1)].reshape(B, S, 200, 200, 3)), rgb_gripper=t(store_g[idx.reshape(-1)].reshape(B, S, 84, 84, 3)))
    sto = dict(common, rgb_static=t(store_s), rgb_gripper=t(store_g), window_start=t(starts), window_len=t(lens, np.int32))
    if shifts:
        sh_s = rng.integers(0, 21, (B * S, 2)).astype(np.int32)
        sh_g = rng.integers(0, 9, (B * S, 2)).astype(np.int32)
        mat.update(shift_static=t(sh_s[eff]), shift_gripper=t(sh_g[eff]))          # the effective shifts: a padded frame is an exact duplicate
        sto.update(shift_static=t(sh_s), shift_gripper=t(sh_g))                    # entries with t >= L are ignored by the kernels
    return mat, sto


def _step(eng, mb, mb_lang=None):
    eng.zero_grads()
    if mb_lang is None:
        l = eng.forward_loss(mb, False, 1.0, 3.0, step=0)
    else:
        lv, ll = eng.forward_loss_pair(mb, mb_lang, 0.5, 3.0, step=0)
        l = {**{"vis_" + k: v for k, v in lv.items()}, **{"lang_" + k: v for k, v in ll.items()}}
    eng.backward()
    torch.cuda.synchronize()
    return l, eng.flat_grads.clone()


def _engine(dims, P, B, S, dtype, **options):
    eng = StepEngine(dims, B, S, dtype=dtype, device="cuda:0", dropout_p=0.0, seed=1)
    for k, v in options.items():
        eng.set_option(k, v)
    eng.load_numpy(P)
    return eng


# The bf16 step comparisons run with the plan-recognition transformer's UNFUSED kernels.  Measured with batches that do not use the store at all (the
# same materialised step evaluated ten times, B=4): with the fused transformer the KL loss differs from run to run by up to 3e-5 relative (the bound
# taken over from the existing store test, 1e-5 |a| + 1e-7, is then missed by identical inputs), and the whole gradient takes one of a few discrete
# values — relative distances 4e-5 .. 8e-5 at S=4, 8e-6 at S=32 (1.4e-4 on the gripper camera's conv1 weights) against 4e-10 / 2e-9 between runs that
# land on the same value — so a noise estimate from ONE pair of runs is ~0 or ~1e-4 by chance and `3 x noise + 1e-5` fails for identical inputs about
# one time in four.  With fused_transformer=0 the losses are bit-identical from run to run and every pair of gradients is within 5e-10 (S=4) / 2e-9
# (S=32): the bounds stay as they are and are effectively their floors.  Everything this file is about — conv1's uint8 forward and weight gradient,
# the fp32 engine's ingest — runs the production kernels either way; the encoder embedding is compared under the default options.
DET = dict(fused_transformer=0)


def _same_loss(a, b, dtype):
    if dtype == "fp32":
        return all(a[k] == b[k] for k in a)
    return all(abs(a[k] - b[k]) <= 1e-5 * abs(a[k]) + 1e-7 for k in a)            # the existing store test's bound (bf16: fp32 atomics in the transformer)


def _grads_agree(g0, g1, g0_again, dtype, what):
    if dtype == "fp32":
        assert torch.equal(g0, g1), what
        return
    noise = ((g0 - g0_again).double().norm() / g0.double().norm()).item()          # the materialised step twice = the backward's own run-to-run noise
    rel = ((g0 - g1).double().norm() / g0.double().norm()).item()
    print(f"[store windows {what}] rel {rel:.3e} noise {noise:.3e}")
    assert rel <= 3.0 * noise + 1e-5, (what, rel, noise)


B1 = 4      # windows of the small cases: lens [1, S, S-1, 2], starts: out of range, 0, start + L == F (start + S > F), an overlapping one


def _small_case(seed):
    dims, P, _, _ = load_case("hulc_tiny")
    S = 4
    batch = synthetic.make_batch(B1, B1, S, seed=seed, edge_frac=0.05, aux_mask="all")
    rng0 = np.random.default_rng(seed + 100)
    for sc in batch:
        batch[sc]["plan_idx"] = rng0.integers(0, 32, (B1, 32)).astype(np.int32)
    F = 3 * S + 5
    store_s, store_g, rng = _stores(F, seed)
    lens = np.array(([1, S, S - 1, 2] * B1)[:B1], np.int32)
    starts = np.array([F + 100, 0, F - (S - 1), 5], np.int64)
    assert starts[2] + lens[2] == F and starts[2] + S > F
    return dims, P, batch, S, F, store_s, store_g, rng, starts, lens


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_padded_store_windows_equal_the_materialised_batch(dtype):
    """The step on window_start + window_len == the step on the batch materialised here with index s0 + min(t, L-1) and the effective shifts: fp32 bit for
    bit; bf16 the loss to the existing store test's bound, the gradients to 3 x the materialised step's own run-to-run noise + 1e-5 (see DET).  hulc_validate
    and the paired vis + lang pass (different lens per modality) agree the same way."""
    dims, P, batch, S, F, store_s, store_g, rng, starts, lens = _small_case(21)
    mat, sto = _modality(batch["vis"], store_s, store_g, starts, lens, S, rng)
    # the paired pass: the lang modality has its own lens and starts
    lens_l = np.array([S, 2, 1, S - 1], np.int32)
    starts_l = np.array([F - S, F - 2, -7, 3], np.int64)
    lang = rng.standard_normal((B1, 384)).astype(np.float32)
    mat_l, sto_l = _modality(batch["lang"], store_s, store_g, starts_l, lens_l, S, rng, lang=lang / np.linalg.norm(lang, axis=-1, keepdims=True))
    eng = _engine(dims, P, 2 * B1, S, dtype, **(DET if dtype == "bf16" else {}))
    (l0, g0), (l1, g1), (_, g2) = _step(eng, mat), _step(eng, sto), _step(eng, mat)
    assert _same_loss(l0, l1, dtype), (l0, l1)
    _grads_agree(g0, g1, g2, dtype, "single")
    (p0, h0), (p1, h1), (_, h2) = _step(eng, mat, mat_l), _step(eng, sto, sto_l), _step(eng, mat, mat_l)
    assert _same_loss(p0, p1, dtype), (p0, p1)
    _grads_agree(h0, h1, h2, dtype, "pair")
    # validation reads the store the same way (no shifts: the validation transforms)
    strip = lambda d: {k: v for k, v in d.items() if not k.startswith("shift") and k != "plan_idx"}
    va, vb = eng.validate(strip(mat), False, None), eng.validate(strip(sto), False, None)
    assert abs(va["action_loss_pp"] - vb["action_loss_pp"]) <= (0.0 if dtype == "fp32" else 1e-5 * abs(va["action_loss_pp"]))
    assert torch.equal(va["sampled_plan_idx_pp"], vb["sampled_plan_idx_pp"])
    if dtype == "fp32":
        assert np.array_equal(va["mae_pp"], vb["mae_pp"]) and va["kl_loss"] == vb["kl_loss"]
    eng.close()


def test_full_length_and_absent_window_len_are_the_plain_store_batch():
    """window_len = [S] * B and no window_len at all: bit-identical loss (bf16, see DET, and fp32) and fp32 gradients of the plain store batch — in the
    single pass and in the paired vis + lang pass (fixed windows of both modalities gathered from the store, each modality with its own starts), where the
    plain store batches also agree with the materialised pair as in test_padded_store_windows_equal_the_materialised_batch."""
    dims, P, batch, S, F, store_s, store_g, rng, starts, _ = _small_case(22)
    full = np.full(B1, S, np.int32)
    mat, sto = _modality(batch["vis"], store_s, store_g, starts, full, S, rng)
    plain = {k: v for k, v in sto.items() if k != "window_len"}
    lang = rng.standard_normal((B1, 384)).astype(np.float32)
    mat_l, sto_l = _modality(batch["lang"], store_s, store_g, np.array([F - S, 1, -7, F + 3], np.int64), full, S, rng, lang=lang / np.linalg.norm(lang, axis=-1, keepdims=True))
    plain_l = {k: v for k, v in sto_l.items() if k != "window_len"}
    for dtype in ("fp32", "bf16"):
        eng = _engine(dims, P, 2 * B1, S, dtype, **(DET if dtype == "bf16" else {}))
        for a, b in (((plain,), (sto,)), ((plain, plain_l), (sto, sto_l))):
            la, ga = _step(eng, *a)
            lb, gb = _step(eng, *b)
            assert all(la[k] == lb[k] for k in la), (dtype, len(a), la, lb)
            if dtype == "fp32":
                assert torch.equal(ga, gb)
        # the paired pass on fixed store windows against the same windows materialised
        (l0, g0), (l1, g1), (_, g2) = _step(eng, mat, mat_l), _step(eng, plain, plain_l), _step(eng, mat, mat_l)
        assert _same_loss(l0, l1, dtype), (dtype, l0, l1)
        _grads_agree(g0, g1, g2, dtype, "pair, fixed windows")
        eng.close()


def test_bf16_padded_windows_at_more_than_one_frame_per_workgroup():
    """bf16, B=4, S=32 (128 frames per camera: the 16-bit conv1 kernels loop over several frames per workgroup), lens {20, 27, 32, 1}: the encoder
    embedding of store + lens == the materialised padded batch bit for bit (deterministic forward); the conv1 weight-gradient slices agree to the
    noise criterion of the small case."""
    dims, P, _, _ = load_case("hulc_tiny")
    B, S, F = 4, 32, 150
    batch = synthetic.make_batch(B, 0, S, seed=23, edge_frac=0.05, aux_mask="all")
    batch["vis"]["plan_idx"] = np.random.default_rng(5).integers(0, 32, (B, 32)).astype(np.int32)
    store_s, store_g, rng = _stores(F, 23)
    lens = np.array([20, 27, 32, 1], np.int32)
    starts = np.array([0, F - 27, 40, F + 3], np.int64)                            # the second ends at the store's last frame, the last is clamped to it
    mat, sto = _modality(batch["vis"], store_s, store_g, starts, lens, S, rng)
    eng = _engine(dims, P, B, S, "bf16")
    emb = []
    for mb in (mat, sto, mat):
        _step(eng, mb)
        emb.append(eng.get_tensor("emb", B * S * 512).copy())
    eng.close()
    assert emb[0].size >= B * S * 64 and np.array_equal(emb[0], emb[1]) and np.array_equal(emb[0], emb[2])
    assert np.abs(emb[0]).max() > 0
    eng = _engine(dims, P, B, S, "bf16", **DET)
    grads = [_step(eng, mb)[1] for mb in (mat, sto, mat)]
    n_checked = 0
    for name, (off, shape) in eng.layout.items():
        if "conv_model.0.weight" in name:
            k = int(np.prod(shape))
            _grads_agree(grads[0][off:off + k], grads[1][off:off + k], grads[2][off:off + k], "bf16", name)
            n_checked += 1
    assert n_checked == 2                                                          # the static and the gripper camera's first layer
    _grads_agree(grads[0], grads[1], grads[2], "bf16", "whole gradient")
    eng.close()


@pytest.mark.parametrize("absolute", [False, True])
def test_store_gather_equals_numpy(absolute):
    """hulc_store_gather against numpy: F=37, B=5, S=8, lens {1, 3, 8, 8, 5}, one clamped start; relative actions pad dims 0..5 with zeros and repeat
    the gripper, absolute actions repeat all seven; robot_obs repeats; lang rows by index.  Copies and zeros only: exact."""
    dims, P, _, _ = load_case("hulc_tiny")
    F, B, S, A = 37, 5, 8, 6
    rng = np.random.default_rng(31)
    act, ro, lang = (rng.standard_normal(s).astype(np.float32) for s in ((F, 7), (F, 15), (A, 384)))
    lens = np.array([1, 3, 8, 8, 5], np.int32)
    starts = np.array([36, 10, F + 50, 0, 32], np.int64)                           # F + 50 is clamped to F - 8; 32 + 5 == F
    rows = np.array([5, 0, 3, 3, 1], np.int32)
    idx, _ = _padded_index(starts, lens, S, F)
    want_a, want_r = act[idx].copy(), ro[idx]
    if not absolute:
        pad = np.arange(S)[None, :] >= lens[:, None]
        want_a[pad, :6] = 0.0
    eng = StepEngine(dims, B, S, dtype="fp32", device="cuda:0", dropout_p=0.0, seed=1)
    a, r, l = eng.store_gather(t(act), t(ro), t(starts), S, window_len=t(lens), lang=t(lang), lang_row=t(rows), absolute=absolute)
    a2, r2, l2 = eng.store_gather(t(act), t(ro), t(starts[[1, 3]]), S)             # no lens, no lang table: plain windows
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), want_a) and np.array_equal(r.cpu().numpy(), want_r) and np.array_equal(l.cpu().numpy(), lang[rows])
    plain = starts[[1, 3]][:, None] + np.arange(S)[None, :]
    assert l2 is None and np.array_equal(a2.cpu().numpy(), act[plain]) and np.array_equal(r2.cpu().numpy(), ro[plain])
    with pytest.raises(ValueError):
        eng.store_gather(t(act), t(ro), t(starts), S, window_len=torch.from_numpy(lens))       # a host tensor
    with pytest.raises(ValueError):
        eng.store_gather(t(act), t(ro[:-1]), t(starts), S)
    eng.close()


def test_frame_store_batch_gathers_through_the_engine():
    """FrameStore.batch(lens=...) = window_len in the dict, starts clamped once, tables gathered by hulc_store_gather with the padding rules."""
    from hulc_amd.utils.frame_store import FrameStore
    dims, P, _, _ = load_case("hulc_tiny")
    F, S = 37, 8
    rng = np.random.default_rng(33)
    act, ro, lang = (rng.standard_normal(s).astype(np.float32) for s in ((F, 7), (F, 15), (3, 384)))
    z = lambda h: torch.zeros(F, h, h, 3, dtype=torch.uint8)
    eng = StepEngine(dims, 4, S, dtype="fp32", device="cuda:0", dropout_p=0.0, seed=1)
    st = FrameStore(z(8), z(4), episode_ends=[20, F], device="cuda:0", actions=torch.from_numpy(act), robot_obs=torch.from_numpy(ro),
                    lang=torch.from_numpy(lang), lang_segments=[(1, 12), (21, 30), (30, 36)]).attach(eng)
    starts, lens = torch.tensor([35, 0, 14, -2]), torch.tensor([5, 8, 6, 1], dtype=torch.int32)
    d = st.batch(starts, S, lens=lens, lang_rows=torch.tensor([2, 0, 1, 1], dtype=torch.int32), shifts=True)
    torch.cuda.synchronize()
    assert d["window_start"].tolist() == [32, 0, 14, 0] and d["window_len"].tolist() == [5, 8, 6, 1] and d["window_len"].dtype == torch.int32
    idx, _ = _padded_index(np.array([32, 0, 14, 0]), lens.numpy(), S, F)
    want = act[idx].copy()
    want[np.arange(S)[None, :] >= lens.numpy()[:, None], :6] = 0.0
    assert np.array_equal(d["actions"].cpu().numpy(), want) and np.array_equal(d["state_info"]["robot_obs"].cpu().numpy(), ro[idx])
    assert np.array_equal(d["lang"].cpu().numpy(), lang[[2, 0, 1, 1]]) and d["shift_static"].shape == (4 * S, 2)
    ms, mg = st.materialise(d["window_start"], S, lens=d["window_len"])
    assert ms.shape == (4, S, 8, 8, 3) and mg.shape == (4, S, 4, 4, 3)
    eng.close()


def test_window_len_argument_errors():
    dims, P, batch, S, F, store_s, store_g, rng, starts, lens = _small_case(24)
    mat, sto = _modality(batch["vis"], store_s, store_g, starts, lens, S, rng)
    eng = _engine(dims, P, B1, S, "fp32")
    with pytest.raises(RuntimeError, match="window_start"):                        # reported by the library before any launch
        eng.forward_loss(dict(mat, window_len=t(lens)), False, 1.0, 3.0)
    with pytest.raises(RuntimeError, match="window_start"):
        eng.validate({k: v for k, v in dict(mat, window_len=t(lens)).items() if not k.startswith("shift") and k != "plan_idx"}, False, None)
    with pytest.raises(ValueError):                                                # a host tensor
        eng.forward_loss(dict(sto, window_len=torch.from_numpy(lens)), False, 1.0, 3.0)
    with pytest.raises(ValueError):                                                # not int32
        eng.forward_loss(dict(sto, window_len=t(lens.astype(np.int64))), False, 1.0, 3.0)
    with pytest.raises(ValueError):                                                # not (B,)
        eng.forward_loss(dict(sto, window_len=t(lens[:-1])), False, 1.0, 3.0)
    l = eng.forward_loss(dict(sto, rgb_static=t(store_s[:2]), rgb_gripper=t(store_g[:2]), window_len=t(np.ones(B1, np.int32))), False, 1.0, 3.0)
    assert np.isfinite(l["total_mod"])                                             # a store shorter than S is fine with short windows
    eng.close()


def test_fit_on_a_calvin_directory_end_to_end(tmp_path):
    """datamodule=calvin_store through the CLI's own composition: a dataset directory written here (two training episodes of 40 and 25 frames, one
    validation episode of 30, annotated segments, embeddings.npy) -> FrameStore -> Trainer.fit for one epoch, fp32."""
    from hulc_amd import config
    from hulc_amd.trainer import Trainer
    from hulc_amd.training import CONF_DIR, make_datamodule, trainer_kwargs
    root = U.write_dataset(tmp_path / "data", seed=3)
    cfg = config.compose(CONF_DIR, "config", ["datamodule=calvin_store", f"datamodule.root_data_dir={root}", "datamodule.batch_size=2", "datamodule.min_window_size=5",
                                              "datamodule.max_window_size=8", "trainer.precision=fp32", "trainer.max_epochs=1", "model.max_batch_size=4",
                                              "model.val_instructions={open_drawer: [open the drawer], push_block: [push the block]}", f"log_dir={tmp_path / 'run'}"])
    dm = make_datamodule(cfg, "cuda:0")
    dm.record_windows = True
    assert dm.steps_per_epoch == ((40 - 5 + 1) + (25 - 5 + 1)) // 2
    model = config.instantiate(cfg.model, device="cuda:0", max_seq_len=cfg.datamodule.max_window_size)
    tr = Trainer(**trainer_kwargs(cfg), log_every=1)
    hist = tr.fit(model, dm)
    assert tr.global_step == dm.steps_per_epoch == len(hist)
    assert all(np.isfinite(h["loss"]) for h in hist)
    assert all(np.isfinite(v) for h in hist for k, v in h.items() if k.startswith("train/"))
    val = tr.val_history[-1]
    assert any(k.startswith("val_act/") for k in val) and all(np.isfinite(v) for v in val.values())
    assert any(k.startswith("lang_gt/") for k in val)                              # on_fit_start found the annotations through train_datasets / val_datasets
    eps = {"train": np.array([40, 65]), "val": np.array([30])}
    segs = {"train": np.array(U.TRAIN_SEGMENTS), "val": np.array(U.VAL_SEGMENTS)}
    assert {w["split"] for w in dm.window_log} == {"train", "val"} and {w["modality"] for w in dm.window_log} == {"vis", "lang"}
    for w in dm.window_log:
        s, l = w["starts"], w["lens"]
        assert l.min() >= 5 and l.max() <= 8 and s.min() >= 0
        if w["modality"] == "vis":
            e = eps[w["split"]]
            assert np.array_equal(np.searchsorted(e, s, side="right"), np.searchsorted(e, s + l - 1, side="right")) and np.all(s + l <= e[-1])
        else:                                                                      # store index == frame id here (one rank, episodes back to back from 0)
            sg = segs[w["split"]]
            assert all(np.any((sg[:, 0] <= a) & (a + n - 1 <= sg[:, 1])) for a, n in zip(s, l))
    model.engine.close()
