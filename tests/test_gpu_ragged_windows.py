"""GPU, through the C-ABI: the ragged encoder pass (hulc_batch::window_len_host) — the perceptual encoders run on the N' real frames of variable-length
padded windows, their rows are expanded to the (B,S,128) embedding, and the embedding gradient is reduced to compact rows before the encoder backward.
Every step test compares against the PADDED pass of the same store batch (window_len), which tests/test_gpu_store_windows.py holds to the materialised
batch.  The small case: hulc_tiny, B = 4, S = 4, a store of 17 frames, lens [1, S, S-1, 2] (N' = 10: not a multiple of the tail's 16 rows per
workgroup); the 16-bit case: B = 4, S = 32, lens {20, 27, 32, 1}.

The measured values of the bounds below are recorded in profiles/ragged_windows.txt."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ragged_windows_util as R  # noqa: E402
import store_windows_util as U  # noqa: E402
from golden_util import load_case  # noqa: E402
from hulc_amd import lib as L  # noqa: E402
from hulc_amd.hulc import Hulc  # noqa: E402
from hulc_amd.utils import synthetic  # noqa: E402
from hulc_amd.utils.frame_store import FrameStore, ragged_plan  # noqa: E402

t = R.t
ENC_CAP = 1e-4      # fp32: rel-L2 of every perceptual_encoder.* gradient, ragged vs padded — a tenth of the 1e-3 gate that holds the fp32 engine to fp64


# ------------------------------------------------------------------------------------------------------------------ the three row kernels
def _kernel_case(name):
    if name == "small":
        B, S, F = 4, 4, 17
        return B, S, F, np.array([1, S, S - 1, 2], np.int32), np.array([F + 100, 0, F - (S - 1), 5], np.int64)
    B, S, F = 64, 32, 16384
    rng = np.random.default_rng(3)
    return B, S, F, rng.integers(20, 33, B).astype(np.int32), rng.integers(-50, F + 50, B).astype(np.int64)


@pytest.mark.parametrize("case", ["small", "big"])
def test_window_compact_and_rows_expand_equal_numpy(case):
    """Integers and copies: exact.  The second launch builds the tables of a paired pass's second batch (off_base = the first batch's N')."""
    B, S, F, lens, starts = _kernel_case(case)
    Lc, off, n = R.plan(lens, S, F)
    rng = np.random.default_rng(7)
    sh_s, sh_g = rng.integers(0, 21, (B * S, 2)).astype(np.int32), rng.integers(0, 9, (B * S, 2)).astype(np.int32)
    lib = L.load()
    d_len, d_off, d_st, d_ss, d_sg = t(Lc), t(off), t(starts), t(sh_s), t(sh_g)      # (held: a temporary's memory is reused by the next allocation)
    frame = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    o_s, o_g = torch.full((n, 2), -1, dtype=torch.int32, device="cuda"), torch.full((n, 2), -1, dtype=torch.int32, device="cuda")
    L.check(lib.hulc_k_window_compact(d_st.data_ptr(), d_len.data_ptr(), d_off.data_ptr(), 0, B, S, F, d_ss.data_ptr(), d_sg.data_ptr(), frame.data_ptr(),
                                      o_s.data_ptr(), o_g.data_ptr(), None))
    torch.cuda.synchronize()
    wf, ws, wg = R.compact_tables(starts, Lc, off, S, F, sh_s, sh_g)
    assert np.array_equal(frame.cpu().numpy(), wf) and np.array_equal(o_s.cpu().numpy(), ws) and np.array_equal(o_g.cpu().numpy(), wg)
    assert wf.min() >= 0 and wf.max() < F
    # the second half of the windows as a batch of its own behind the first half, without shifts
    h = B // 2
    n2 = int(off[B] - off[h])
    frame2 = torch.full((n2,), -1, dtype=torch.int64, device="cuda")
    L.check(lib.hulc_k_window_compact(d_st[h:].data_ptr(), d_len[h:].data_ptr(), d_off[h:].data_ptr(), int(off[h]), B - h, S, F, None, None, frame2.data_ptr(), None, None, None))
    torch.cuda.synchronize()
    assert np.array_equal(frame2.cpu().numpy(), wf[off[h]:])
    for eb, dt in ((2, np.uint16), (4, np.float32)):
        src = rng.integers(0, 60000, (n, 128)).astype(dt) if eb == 2 else rng.standard_normal((n, 128)).astype(dt)
        dst = torch.from_numpy(np.zeros((B * S, 128), dt).view(np.int16 if eb == 2 else np.float32)).cuda()
        d_src = torch.from_numpy(src.view(np.int16 if eb == 2 else np.float32)).cuda()
        L.check(lib.hulc_k_rows_expand(eb, d_src.data_ptr(), d_len.data_ptr(), d_off.data_ptr(), B, S, 128, dst.data_ptr(), None))
        torch.cuda.synchronize()
        assert np.array_equal(dst.cpu().numpy().view(dt), R.expand_rows(src, Lc, off, S)), eb
    assert lib.hulc_k_rows_expand(3, d_src.data_ptr(), d_len.data_ptr(), d_off.data_ptr(), B, S, 128, dst.data_ptr(), None) != 0      # refused before any launch


@pytest.mark.parametrize("case", ["small", "big"])
def test_rows_reduce_is_the_stated_fp32_sum(case):
    """Bit-exact against numpy float32 accumulation in ascending t; within fp32 rounding of S terms of the float64 sum; twice the same bits."""
    B, S, F, lens, _ = _kernel_case(case)
    Lc, off, n = R.plan(lens, S, F)
    rng = np.random.default_rng(11)
    src = (rng.standard_normal((B * S, 128)) * np.exp(rng.uniform(-3, 3, (B * S, 1)))).astype(np.float32)
    lib = L.load()
    d_src, d_len, d_off = t(src), t(Lc), t(off)
    outs = []
    for _ in range(2):
        dst = torch.full((n, 128), float("nan"), dtype=torch.float32, device="cuda")
        L.check(lib.hulc_k_rows_reduce(d_src.data_ptr(), d_len.data_ptr(), d_off.data_ptr(), B, S, 128, dst.data_ptr(), None))
        torch.cuda.synchronize()
        outs.append(dst.cpu().numpy())
    want32, want64 = R.reduce_rows(src, Lc, off, S, np.float32), R.reduce_rows(src, Lc, off, S, np.float64)
    assert np.array_equal(outs[0].view(np.uint32), want32.view(np.uint32)) and np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    # a sum of k <= S fp32 terms added one by one: |error| <= (k - 1) eps sum |terms| (eps = 2^-24), bounded here with k = S for every row
    mag = R.reduce_rows(np.abs(src), Lc, off, S, np.float64)
    assert np.all(np.abs(outs[0].astype(np.float64) - want64) <= (S - 1) * 2.0 ** -24 * mag + 1e-45)


# ------------------------------------------------------------------------------------------------------------------ step level
def _emb(eng, B, S):
    return eng.get_tensor("emb", B * S * 512).copy()


def _check_fp32_grads(eng, g_pad, g_rag, what):
    """fp32: non-encoder tensors equal bit for bit (finished before the encoder backward, from an identical forward); every perceptual_encoder.* tensor within ENC_CAP."""
    enc, mask = R.encoder_split(eng)
    assert len(enc) >= 20 and torch.equal(g_pad[~mask], g_rag[~mask]), what
    worst = max((R.rel(g_rag[off:off + k], g_pad[off:off + k]), n) for n, off, k in enc if g_pad[off:off + k].abs().max() > 0)
    print(f"[ragged {what}] fp32 worst encoder tensor rel-L2 {worst[0]:.3e} ({worst[1]})")
    assert worst[0] <= ENC_CAP, (what, worst)
    return worst[0]


def _check_16bit_grads(ref, mask, g_pad, g_rag, g_pad_again, what):
    """16-bit: against the fp32 engine's padded encoder gradient R: e_rag <= 1.1 e_pad + 3 noise + 1e-5."""
    r = ref[mask]
    e_pad, e_rag = R.rel(g_pad[mask], r), R.rel(g_rag[mask], r)
    noise = ((g_pad[mask].double() - g_pad_again[mask].double()).norm() / r.double().norm()).item()
    print(f"[ragged {what}] bf16 e_pad {e_pad:.4e} e_rag {e_rag:.4e} noise {noise:.3e}")
    assert e_rag <= 1.1 * e_pad + 3.0 * noise + 1e-5, (what, e_pad, e_rag, noise)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_ragged_single_pass_against_the_padded_pass(dtype):
    """The path ran (encoder_frames), the forward is bit-identical (emb under the default options; losses), the backward agrees (fp32: criteria of
    _check_fp32_grads; bf16: _check_16bit_grads against the fp32 engine's padded gradient), and hulc_validate agrees."""
    dims, P, batch, S, F, store_s, store_g, rng, starts, lens = R.small_case(31)
    pad, rag = R.modality(batch["vis"], store_s, store_g, starts, lens, S, rng)
    n_real = ragged_plan(lens, S, F)[2]
    assert n_real == 10
    ref = None
    if dtype == "bf16":
        e32 = R.engine(dims, P, R.B1, S, "fp32")
        ref = R.step(e32, pad)[1]
        e32.close()
    eng = R.engine(dims, P, R.B1, S, dtype)
    # ---- forward under the default options: the embedding
    (l0, _, f0), e0 = R.step(eng, pad), _emb(eng, R.B1, S)
    (l1, _, f1), e1 = R.step(eng, rag), _emb(eng, R.B1, S)
    assert f0 == R.B1 * S and f1 == n_real                                         # the padded pass encodes B S frames, the ragged one N'
    assert np.abs(e0).max() > 0 and np.array_equal(e0.view(np.uint32), e1.view(np.uint32))
    if dtype == "fp32":
        assert R.same_loss(l0, l1, dtype), (l0, l1)
    # ---- losses and gradients (bf16: transformer unfused, see DET)
    if dtype == "bf16":
        eng.set_option("fused_transformer", 0)
    (l0, g0, _), (l1, g1, _), (_, g2, _) = R.step(eng, pad), R.step(eng, rag), R.step(eng, pad)
    assert R.same_loss(l0, l1, dtype), (l0, l1)
    if dtype == "fp32":
        _check_fp32_grads(eng, g0, g1, "single")
        assert torch.equal(g0, g2)
    else:
        _check_16bit_grads(ref, R.encoder_split(eng)[1], g0, g1, g2, "single small")
    # ---- validation (no shifts: the validation transforms)
    strip = lambda d: {k: v for k, v in d.items() if not k.startswith("shift") and k != "plan_idx"}
    va, vb = eng.validate(strip(pad), False, None), eng.validate(strip(rag), False, None)
    assert eng.encoder_frames() == n_real
    if dtype == "fp32":
        assert va["action_loss_pp"] == vb["action_loss_pp"] and va["kl_loss"] == vb["kl_loss"] and np.array_equal(va["mae_pp"], vb["mae_pp"])
        assert torch.equal(va["sampled_plan_idx_pp"], vb["sampled_plan_idx_pp"]) and torch.equal(va["sampled_plan_idx_pr"], vb["sampled_plan_idx_pr"])
    else:
        for k in ("action_loss_pp", "action_loss_pr", "kl_loss"):
            assert abs(va[k] - vb[k]) <= 1e-5 * abs(va[k]), (k, va[k], vb[k])
    eng.close()


def test_full_lens_are_the_padded_pass_bit_for_bit():
    """L_b = S for every window: N' = B S, no sum has more than one term — the whole fp32 gradient is equal."""
    dims, P, batch, S, F, store_s, store_g, rng, starts, _ = R.small_case(32)
    pad, rag = R.modality(batch["vis"], store_s, store_g, starts, np.full(R.B1, S + 3, np.int32), S, rng)      # beyond S: clamped
    eng = R.engine(dims, P, R.B1, S, "fp32")
    (l0, g0, f0), (l1, g1, f1) = R.step(eng, pad), R.step(eng, rag)
    assert f0 == f1 == R.B1 * S and l0 == l1 and torch.equal(g0, g1)
    eng.close()


def test_bf16_ragged_windows_at_more_than_one_frame_per_workgroup():
    """The 16-bit case: B = 4, S = 32, lens {20, 27, 32, 1} (N' = 80; the 16-bit conv1 kernels loop over several frames per workgroup)."""
    dims, P, _, _ = load_case("hulc_tiny")
    B, S, F = 4, 32, 150
    batch = synthetic.make_batch(B, 0, S, seed=33, edge_frac=0.05, aux_mask="all")
    batch["vis"]["plan_idx"] = np.random.default_rng(5).integers(0, 32, (B, 32)).astype(np.int32)
    store_s, store_g, rng = R.stores(F, 33)
    lens, starts = np.array([20, 27, 32, 1], np.int32), np.array([0, F - 27, 40, F + 3], np.int64)
    pad, rag = R.modality(batch["vis"], store_s, store_g, starts, lens, S, rng)
    e32 = R.engine(dims, P, B, S, "fp32")
    ref = R.step(e32, pad)[1]
    e32.close()
    eng = R.engine(dims, P, B, S, "bf16")
    (_, _, f0), e0 = R.step(eng, pad), _emb(eng, B, S)
    (_, _, f1), e1 = R.step(eng, rag), _emb(eng, B, S)
    assert f0 == B * S and f1 == 80 and np.abs(e0).max() > 0 and np.array_equal(e0.view(np.uint32), e1.view(np.uint32))
    eng.set_option("fused_transformer", 0)
    (l0, g0, _), (l1, g1, _), (_, g2, _) = R.step(eng, pad), R.step(eng, rag), R.step(eng, pad)
    assert R.same_loss(l0, l1, "bf16"), (l0, l1)
    _check_16bit_grads(ref, R.encoder_split(eng)[1], g0, g1, g2, "single S=32")
    eng.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_ragged_paired_pass(dtype):
    """vis lens [1, S, S-1, 2], lang lens [S, 2, 1, S-1]: the conv1 stages split the N'_vis + N'_lang frames at N'_vis, not in the middle."""
    dims, P, batch, S, F, store_s, store_g, rng, starts, lens = R.small_case(34)
    lens_l, starts_l = np.array([S, 2, 1, S - 1], np.int32), np.array([F - S, F - 2, -7, 3], np.int64)
    lang = rng.standard_normal((R.B1, 384)).astype(np.float32)
    pad, rag = R.modality(batch["vis"], store_s, store_g, starts, lens, S, rng)
    pad_l, rag_l = R.modality(batch["lang"], store_s, store_g, starts_l, lens_l, S, rng, lang=lang / np.linalg.norm(lang, axis=-1, keepdims=True))
    n_v, n_l = ragged_plan(lens, S, F)[2], ragged_plan(lens_l, S, F)[2]
    assert (n_v, n_l) == (10, 10) and lens.tolist() != lens_l.tolist()
    ref = None
    if dtype == "bf16":
        e32 = R.engine(dims, P, 2 * R.B1, S, "fp32")
        ref = R.step(e32, pad, pad_l)[1]
        e32.close()
    eng = R.engine(dims, P, 2 * R.B1, S, dtype)
    (_, _, f0), e0 = R.step(eng, pad, pad_l), _emb(eng, 2 * R.B1, S)
    (_, _, f1), e1 = R.step(eng, rag, rag_l), _emb(eng, 2 * R.B1, S)
    assert f0 == 2 * R.B1 * S and f1 == n_v + n_l
    assert np.abs(e0).max() > 0 and np.array_equal(e0.view(np.uint32), e1.view(np.uint32))
    if dtype == "bf16":
        eng.set_option("fused_transformer", 0)
    (l0, g0, _), (l1, g1, _), (_, g2, _) = R.step(eng, pad, pad_l), R.step(eng, rag, rag_l), R.step(eng, pad, pad_l)
    assert R.same_loss(l0, l1, dtype), (l0, l1)
    if dtype == "fp32":
        _check_fp32_grads(eng, g0, g1, "pair")
    else:
        _check_16bit_grads(ref, R.encoder_split(eng)[1], g0, g1, g2, "pair small")
    # one ragged and one padded batch: refused with a message, and the context goes on working
    for a, b in ((rag, pad_l), (pad, rag_l)):
        with pytest.raises(RuntimeError, match="both modalities or for neither"):
            eng.forward_loss_pair(a, b, 0.5, 3.0, step=0)
    l2, g3, f2 = R.step(eng, rag, rag_l)
    assert f2 == n_v + n_l and R.same_loss(l1, l2, dtype)
    if dtype == "fp32":
        assert torch.equal(g1, g3)                                                 # the ragged backward is deterministic: fixed order, no atomics
    eng.close()


def test_ragged_edges():
    """All lens 1 (N' = B, S-fold sums), B = 1, window_len_host without window_start, and the workspace of a context that never uses the feature."""
    dims, P, batch, S, F, store_s, store_g, rng, starts, _ = R.small_case(35)
    pad, rag = R.modality(batch["vis"], store_s, store_g, starts, np.ones(R.B1, np.int32), S, rng)
    eng = R.engine(dims, P, R.B1, S, "fp32")
    ws_fresh = eng.workspace_bytes()
    (l0, g0, f0), e0 = R.step(eng, pad), _emb(eng, R.B1, S)
    ws_padded = eng.workspace_bytes()
    (l1, g1, f1), e1 = R.step(eng, rag), _emb(eng, R.B1, S)
    assert f0 == R.B1 * S and f1 == R.B1 and l0 == l1 and np.array_equal(e0.view(np.uint32), e1.view(np.uint32))
    _check_fp32_grads(eng, g0, g1, "all lens 1")
    # the compact buffers are allocated on first use: a context that never passes window_len_host holds what it held before the feature existed
    # (its own lazy buffers — the uint8 ingest's, window_len's tables — and nothing else), a ragged one the three compact buffers more
    assert ws_fresh <= ws_padded < eng.workspace_bytes()
    other = R.engine(dims, P, R.B1, S, "fp32")
    R.step(other, pad)
    assert other.workspace_bytes() == ws_padded
    other.close()
    # B = 1: one window of 3 real frames
    pad1, rag1 = R.modality({k: batch["vis"][k][:1] for k in ("actions", "robot_obs", "plan_idx")}, store_s, store_g, np.array([5], np.int64), np.array([3], np.int32), S, rng)
    (l0, g0, f0), (l1, g1, f1) = R.step(eng, pad1), R.step(eng, rag1)
    assert f0 == S and f1 == 3 and l0 == l1
    _check_fp32_grads(eng, g0, g1, "B = 1")
    # without the frame store: reported by the library before any launch (forward and validate), the counter of the last pass untouched
    mat = {k: v for k, v in rag.items() if k not in ("window_start", "window_len")}
    mat.update(rgb_static=t(store_s[:R.B1 * S].reshape(R.B1, S, 200, 200, 3)), rgb_gripper=t(store_g[:R.B1 * S].reshape(R.B1, S, 84, 84, 3)))
    with pytest.raises(RuntimeError, match="window_len_host.*window_start"):
        eng.forward_loss(mat, False, 1.0, 3.0)
    with pytest.raises(RuntimeError, match="window_len_host.*window_start"):
        eng.validate({k: v for k, v in mat.items() if not k.startswith("shift") and k != "plan_idx"}, False, None)
    assert eng.encoder_frames() == 3
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ two-tier store, module level
ENDS = [9, 17]


def _tier_store(frames, eng, **tiers):
    return FrameStore(frames["s"], frames["g"], episode_ends=ENDS, device="cuda:0", actions=frames["actions"], robot_obs=frames["robot_obs"], **tiers).attach(eng)


def test_ragged_step_on_a_two_tier_store():
    """The small store cut in two (resident_frames 10 -> R = 9): windows of both tiers; batch(ragged=True, staged=handle) == the all-resident ragged step."""
    dims, P, _, _ = load_case("hulc_tiny")
    S, F = 4, 17
    store_s, store_g, rng = R.stores(F, 36)
    act = rng.uniform(-1, 1, (F, 7)).astype(np.float32)
    frames = dict(s=torch.from_numpy(store_s), g=torch.from_numpy(store_g), actions=torch.from_numpy(act),
                  robot_obs=torch.from_numpy((rng.standard_normal((F, 15)) * 0.3).astype(np.float32)))
    starts, lens = np.array([0, 5, 9, 14], np.int64), np.array([1, S, S - 1, 2], np.int32)      # two resident windows, two of the host tier
    eng = R.engine(dims, P, R.B1, S, "fp32")
    res, tie = _tier_store(frames, eng), _tier_store(frames, eng, resident_frames=10, stage_slots=4, stage_slot_frames=S)
    assert tie.R == 9

    def mb(store, staged=None):
        g = torch.Generator(device="cuda:0")
        g.manual_seed(5)
        d = store.batch(None if staged is not None else torch.as_tensor(starts), S, lens=None if staged is not None else torch.as_tensor(lens), shifts=True, generator=g,
                        staged=staged, ragged=True)
        d["plan_idx"] = torch.from_numpy(np.random.default_rng(1).integers(0, 32, (R.B1, 32)).astype(np.int32)).cuda()
        assert d["window_len_host"].tolist() == lens.tolist()
        return Hulc._modality_batch(d, False, torch.device("cuda:0"))

    m_res, m_tie = mb(res), mb(tie, staged=tie.stage(starts, S, lens))
    assert m_tie["window_start"].tolist() == [0, 5, 9, 13] and eng.store_stage_stats()["copies"] == 4      # two windows x two cameras, their real frames only
    (l0, g0, f0), (l1, g1, f1) = R.step(eng, m_res), R.step(eng, m_tie)
    assert f0 == f1 == 10 and l0 == l1
    _, mask = R.encoder_split(eng)
    assert torch.equal(g0[mask], g1[mask]) and torch.equal(g0, g1)
    assert m_tie["staged"].done
    eng.close()


def test_module_training_step_and_datamodule_fit(tmp_path):
    """Hulc.training_step on {"vis": store.batch(..., ragged=True), "lang": ...} logs the padded dicts' train/* values (fp32: the forward is bit-identical),
    on the store of the tiny CALVIN directory; CalvinStoreDataModule(ragged_encoders=True) runs a two-step fit on it."""
    from hulc_amd import config
    from hulc_amd.trainer import Trainer
    from hulc_amd.training import CONF_DIR, make_datamodule, trainer_kwargs
    root = U.write_dataset(tmp_path / "data", seed=3)
    cfg = config.compose(CONF_DIR, "config", ["datamodule=calvin_store", f"datamodule.root_data_dir={root}", "datamodule.batch_size=2", "datamodule.min_window_size=5",
                                              "datamodule.max_window_size=8", "datamodule.ragged_encoders=true", "trainer.precision=fp32", "trainer.max_epochs=1", "model.max_batch_size=4",
                                              "model.val_instructions={open_drawer: [open the drawer], push_block: [push the block]}", f"log_dir={tmp_path / 'run'}"])
    dm = make_datamodule(cfg, "cuda:0")
    assert dm.ragged_encoders
    model = config.instantiate(cfg.model, device="cuda:0", max_seq_len=cfg.datamodule.max_window_size)
    dm.attach(model.engine)
    st, S = dm.stores["train"], 8
    (sv, lv, _), (sl, ll, rows, aux, _) = st.sample_windows(2, 5, S, np.random.default_rng(2), return_host=True), st.sample_lang_windows(2, 5, S, np.random.default_rng(3), return_host=True)

    def batches(ragged):
        g = torch.Generator(device="cuda:0")
        g.manual_seed(9)
        b = {"vis": st.batch(sv, S, lens=lv, shifts=True, generator=g, ragged=ragged), "lang": st.batch(sl, S, lens=ll, lang_rows=rows, use_for_aux=aux, shifts=True, generator=g, ragged=ragged)}
        for i, sc in enumerate(b):
            b[sc]["plan_idx"] = torch.from_numpy(np.random.default_rng(10 + i).integers(0, 32, (2, 32)).astype(np.int32)).cuda()
        return b

    logs, frames = [], []
    for ragged in (False, True):
        model.logged.clear()
        model.global_step = 0
        model.training_step(batches(ragged), 0)
        torch.cuda.synchronize()
        logs.append({k: v for k, v in model.logged.items() if k.startswith("train/")})
        frames.append(model.engine.encoder_frames())
    print(f"[ragged module] padded {logs[0]} ragged {logs[1]} frames {frames}")
    assert frames == [2 * 2 * S, int(lv.sum().item() + ll.sum().item())] and frames[1] < frames[0]
    assert logs[0] and logs[0].keys() == logs[1].keys() and all(logs[0][k] == logs[1][k] for k in logs[0])
    model.global_step = 0
    dm.record_windows = True
    tr = Trainer(**trainer_kwargs(cfg), log_every=1, limit_train_batches=2)
    hist = tr.fit(model, dm)
    assert tr.global_step == 2 == len(hist) and all(np.isfinite(h["loss"]) for h in hist)
    last = dm.window_log[-1]                                                       # the last encoder pass of the fit: the validation batch's lang modality
    assert last["split"] == "val" and last["modality"] == "lang" and model.engine.encoder_frames() == int(last["lens"].sum())
    model.engine.close()
