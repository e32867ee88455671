"""GPU: the two-tier frame store (FrameStore(resident_frames=...), hulc_store_stage / hulc_store_stage_join / hulc_store_stage_stats,
CalvinStoreDataModule(resident_gb=...)).  A tiered store keeps the episodes up to its cut in HBM and the others in pinned host memory; host-tier windows
are copied into staging slots behind the resident frames and `window_start` names the slot.  The step cannot tell the difference, so every case
compares against the SAME windows drawn from an all-resident store of the same frames, with the comparison tests/test_gpu_store_windows.py uses
between store and materialised batch: fp32 bit for bit; bf16 (transformer unfused, see DET there: a repeated identical run is then bit-equal in
the losses) the losses to 1e-5 relative, the gradients to 3 x the resident step's own run-to-run difference + 1e-5.

Full-size frames, S = 8, a store of three episodes of 24, 20 and 28 frames (F = 72, about 10 MB)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import store_windows_util as U  # noqa: E402
from golden_util import load_case  # noqa: E402
from hulc_amd import lib as L  # noqa: E402
from hulc_amd.engine import StepEngine  # noqa: E402
from hulc_amd.hulc import Hulc  # noqa: E402
from hulc_amd.utils.frame_store import FrameStore  # noqa: E402

ENDS = [24, 44, 72]
F, S, A = 72, 8, 5
DET = dict(fused_transformer=0)


@pytest.fixture(scope="module")
def frames():
    """The frames and tables of the store, made once and never written."""
    rng = np.random.default_rng(41)
    lang = rng.standard_normal((A, 384)).astype(np.float32)
    act = rng.uniform(-1, 1, (F, 7)).astype(np.float32)
    act[:, 6] = np.where(rng.random(F) < 0.5, -1.0, 1.0)
    return dict(s=torch.from_numpy(rng.integers(0, 256, (F, 200, 200, 3), dtype=np.uint8)), g=torch.from_numpy(rng.integers(0, 256, (F, 84, 84, 3), dtype=np.uint8)),
                actions=torch.from_numpy(act), robot_obs=torch.from_numpy((rng.standard_normal((F, 15)) * 0.3).astype(np.float32)),
                lang=torch.from_numpy(lang / np.linalg.norm(lang, axis=-1, keepdims=True)))


def _store(fr, eng, **tiers):
    return FrameStore(fr["s"], fr["g"], episode_ends=ENDS, device="cuda:0", actions=fr["actions"], robot_obs=fr["robot_obs"], lang=fr["lang"], **tiers).attach(eng)


def _engine(dtype, max_batch, **options):
    dims, P, _, _ = load_case("hulc_tiny")
    eng = StepEngine(dims, max_batch, S, dtype=dtype, device="cuda:0", dropout_p=0.0, seed=1)
    for k, v in options.items():
        eng.set_option(k, v)
    eng.load_numpy(P)
    return eng


def _mb(store, starts, lens, rows=None, seed=0, staged=None, shifts=True):
    """One modality's engine inputs from a store: the same starts / lens / shift draws / plan injection for whichever store is asked."""
    g = torch.Generator(device="cuda:0")
    g.manual_seed(1000 + seed)
    B = len(starts)
    d = store.batch(None if staged is not None else torch.as_tensor(starts), S, lens=None if staged is not None else torch.as_tensor(lens, dtype=torch.int32),
                    lang_rows=None if rows is None else torch.as_tensor(rows, dtype=torch.int32), shifts=shifts, generator=g, staged=staged)
    d["plan_idx"] = torch.from_numpy(np.random.default_rng(seed).integers(0, 32, (B, 32)).astype(np.int32)).cuda()
    return Hulc._modality_batch(d, rows is not None, torch.device("cuda:0"))


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


def _same_loss(a, b, dtype):
    if dtype == "fp32":
        return all(a[k] == b[k] for k in a)
    return all(abs(a[k] - b[k]) <= 1e-5 * abs(a[k]) + 1e-7 for k in a)


def _grads_agree(g0, g1, g0_again, dtype, what):
    if dtype == "fp32":
        assert torch.equal(g0, g1), what
        return
    noise = ((g0 - g0_again).double().norm() / g0.double().norm()).item()
    rel = ((g0 - g1).double().norm() / g0.double().norm()).item()
    print(f"[store tiers {what}] rel {rel:.3e} noise {noise:.3e}")
    assert rel <= 3.0 * noise + 1e-5, (what, rel, noise)


# vis: resident full window, host window of 5, host window that ends on the store's last frame, host window of one frame
VIS = (np.array([0, 30, 64, 50], np.int64), np.array([8, 5, 8, 1], np.int32))
# lang: resident window of 3, host full window, ONE frame that is the store's last, resident full window
LANG = (np.array([10, 44, 71, 2], np.int64), np.array([3, 8, 1, 8], np.int32), np.array([4, 0, 2, 2], np.int32))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_mixed_tier_pair_step_equals_the_resident_store(frames, dtype):
    """Cut after episode 0 (resident_frames 30 -> R = 24); every modality mixes resident and host-tier windows of different lengths."""
    eng = _engine(dtype, 8, **(DET if dtype == "bf16" else {}))
    res, tie = _store(frames, eng), _store(frames, eng, resident_frames=30, stage_slots=8, stage_slot_frames=S)
    assert tie.R == 24 and tie.rgb_static.shape[0] == 24 + 8 * S and tie.host_static.is_pinned() and tie.host_static.shape[0] == F - 24
    rv, rl = _mb(res, *VIS, seed=1), _mb(res, *LANG, seed=2)
    tv, tl = _mb(tie, *VIS, seed=1), _mb(tie, *LANG, seed=2)
    assert tv["window_start"].tolist() == [0, 24, 32, 40] and tl["window_start"].tolist() == [10, 48, 56, 2]       # slots 0..2, then 3..4
    assert torch.equal(tv["actions"], rv["actions"]) and torch.equal(tl["robot_obs"], rl["robot_obs"]) and torch.equal(tl["lang"], rl["lang"])      # tables: original starts
    assert eng.store_stage_stats() == dict(calls=2, copies=10, bytes=(5 + 8 + 1 + 8 + 1) * (120000 + 21168))      # only the L real frames
    (l0, g0), (l1, g1), (_, g2) = _step(eng, rv, rl), _step(eng, tv, tl), _step(eng, rv, rl)
    print(f"[store tiers pair {dtype}] resident {l0} tiered {l1}")
    assert _same_loss(l0, l1, dtype), (l0, l1)
    _grads_agree(g0, g1, g2, dtype, f"pair {dtype}")
    assert tv["staged"].done and tl["staged"].done                                 # the backward marked both handles
    torch.cuda.synchronize()
    # what the slots hold: the frames of the host-tier windows, nothing else moved
    assert torch.equal(tie.rgb_static[24:24 + 5].cpu(), frames["s"][30:35]) and torch.equal(tie.rgb_gripper[32:40].cpu(), frames["g"][64:72])
    assert torch.equal(tie.rgb_static[:24].cpu(), frames["s"][:24])
    eng.close()


def test_everything_staged_and_everything_resident(frames):
    """resident_frames = 0: every window goes through a slot; resident_frames = F: a tiered store without a host tier stages nothing."""
    eng = _engine("fp32", 4)
    res = _store(frames, eng)
    none = _store(frames, eng, resident_frames=0, stage_slots=4, stage_slot_frames=S)
    whole = _store(frames, eng, resident_frames=F, stage_slots=4, stage_slot_frames=S)
    assert none.R == 0 and none.rgb_static.shape[0] == 4 * S and whole.R == F and whole.host_static is None
    l0, g0 = _step(eng, _mb(res, *VIS, seed=3))
    assert eng.store_stage_stats()["calls"] == 0
    mb = _mb(whole, *VIS, seed=3)
    assert mb["window_start"].tolist() == VIS[0].tolist() and mb["staged"].ticket == 0
    l1, g1 = _step(eng, mb)
    assert eng.store_stage_stats() == dict(calls=0, copies=0, bytes=0)
    mb = _mb(none, *VIS, seed=3)
    assert mb["window_start"].tolist() == [0, 8, 16, 24]
    l2, g2 = _step(eng, mb)
    assert eng.store_stage_stats() == dict(calls=1, copies=8, bytes=(8 + 5 + 8 + 1) * (120000 + 21168))
    assert l0 == l1 == l2 and torch.equal(g0, g1) and torch.equal(g0, g2)
    eng.close()


def test_four_optimizer_steps_with_lookahead_on_a_ring_of_two_batches(frames):
    """Stage batch n + 1, then run batch n — the datamodule's order — on a ring of exactly two batches (2 x (2 + 2) slots), every window host-tier so
    that steps 2 and 3 overwrite the slots steps 0 and 1 read.  Per-step losses and the final parameters equal the same four steps on the resident store."""
    rng = np.random.default_rng(7)
    host_starts = np.concatenate([np.arange(24, 44 - 4), np.arange(44, 72 - 4)])
    steps = [dict(vs=rng.choice(host_starts, 2), vl=rng.integers(1, 5, 2).astype(np.int32), ls=rng.choice(host_starts, 2), ll=rng.integers(1, 5, 2).astype(np.int32),
                  rows=rng.integers(0, A, 2).astype(np.int32)) for _ in range(4)]
    steps[1]["vl"][0], steps[2]["ll"][1] = 8, 8                                    # full windows too (30..37 and 64..71)
    steps[1]["vs"][0], steps[2]["ls"][1] = 30, 64

    def run(tiers):
        eng = _engine("fp32", 4)
        st = _store(frames, eng, **tiers)
        stage = lambda w: (st.stage(w["vs"], S, w["vl"]), st.stage(w["ls"], S, w["ll"])) if st.tiered else (None, None)
        losses, ahead = [], stage(steps[0])
        for n, w in enumerate(steps):
            cur, ahead = ahead, (stage(steps[n + 1]) if n + 1 < len(steps) else None)
            mv = _mb(st, w["vs"], w["vl"], seed=10 + n, staged=cur[0]) if st.tiered else _mb(st, w["vs"], w["vl"], seed=10 + n)
            ml = _mb(st, w["ls"], w["ll"], rows=w["rows"], seed=20 + n, staged=cur[1]) if st.tiered else _mb(st, w["ls"], w["ll"], rows=w["rows"], seed=20 + n)
            eng.zero_grads()
            lv, ll = eng.forward_loss_pair(mv, ml, 0.5, 3.0, step=n)
            eng.backward()
            eng.adam_step(lr=1e-3)
            losses.append((lv, ll))
        torch.cuda.synchronize()
        out = losses, eng.flat_params.clone(), (eng.store_stage_stats(), eng.get_option("persistent_rnn_fallbacks"))
        eng.close()
        return out

    l_res, p_res, _ = run({})
    l_tie, p_tie, (stats, fallbacks) = run(dict(resident_frames=24, stage_slots=8, stage_slot_frames=S))
    print(f"[store tiers lookahead] losses resident {[a['total_mod'] for a, _ in l_res]} tiered {[a['total_mod'] for a, _ in l_tie]} stats {stats}")
    assert stats["calls"] == 8 and stats["copies"] == 2 * 16 and fallbacks == 0
    assert l_res == l_tie
    assert torch.equal(p_res, p_tie)


def test_validation_step_on_a_tiered_store(frames):
    m = Hulc(precision="fp32", max_batch_size=4, max_seq_len=S, use_clip_auxiliary_loss=False)
    res, tie = _store(frames, m.engine), _store(frames, m.engine, resident_frames=50, stage_slots=8, stage_slot_frames=S)
    assert tie.R == 44

    def val(st):
        tt = torch.as_tensor
        b = {"vis": st.batch(tt(VIS[0]), S, lens=tt(VIS[1])), "lang": st.batch(tt(LANG[0]), S, lens=tt(LANG[1]), lang_rows=tt(LANG[2]))}
        m.logged.clear()
        out = m.validation_step(b, 0)
        return out, dict(m.logged), b

    o0, g0, _ = val(res)
    o1, g1, b1 = val(tie)
    print(f"[store tiers validation] resident {g0} tiered {g1}")
    assert g0 and g0 == g1
    assert all(torch.equal(o0[k], o1[k]) for k in o0 if k.startswith("sampled_plan"))
    assert b1["vis"]["staged"].done and b1["lang"]["staged"].done and b1["vis"]["window_start"].tolist() == [0, 30, 44, 52]
    assert m.engine.store_stage_stats()["calls"] == 2
    m.engine.close()


def test_stage_error_paths_leave_nothing_enqueued():
    eng = _engine("fp32", 2)
    dst = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    pinned = torch.arange(4096, dtype=torch.int32).to(torch.uint8).pin_memory()
    pageable = np.zeros(4096, np.uint8)
    host_dst = torch.zeros(4096, dtype=torch.uint8).pin_memory()
    big = torch.zeros(1 << 26, dtype=torch.uint8, device="cuda:0")                 # larger than any block the 4 KiB pinned tensor can sit in
    ok = (pinned.data_ptr(), dst.data_ptr(), 4096)
    t0 = eng.store_stage([ok])
    eng.store_stage_join(t0)
    torch.cuda.synchronize()
    assert t0 >= 1 and torch.equal(dst.cpu(), pinned)
    before = eng.store_stage_stats()
    assert before == dict(calls=1, copies=1, bytes=4096)
    arr = lambda cs: (L.HulcStageCopy * len(cs))(*[L.HulcStageCopy(src=s, dst=d, bytes=b) for s, d, b in cs])
    bad = [[ok, (pageable.ctypes.data, dst.data_ptr(), 4096)],                     # a pageable source (after a good copy: nothing of the call is enqueued)
           [(pinned.data_ptr(), host_dst.data_ptr(), 4096)],                       # a destination in host memory
           [(pinned.data_ptr(), dst.data_ptr(), 0)], [(pinned.data_ptr(), dst.data_ptr(), -16)],
           [(None, dst.data_ptr(), 16)], [(pinned.data_ptr(), None, 16)],
           [(pinned.data_ptr(), big.data_ptr(), big.numel())],                     # a source that runs past the end of its pinned buffer
           [(big.data_ptr(), big.data_ptr(), 1 << 40)]]                            # device ranges larger than any allocation (the allocator's segment counts)
    dst.zero_()
    for cs in bad:
        assert eng.lib.hulc_store_stage(eng.ctx, arr(cs), len(cs)) < 0, cs
        assert L.load().hulc_last_error()
    assert eng.lib.hulc_store_stage(eng.ctx, arr([ok]), 0) < 0                     # n = 0
    assert eng.lib.hulc_store_stage(eng.ctx, None, 1) < 0
    with pytest.raises(RuntimeError, match="hulc_store_stage"):
        eng.store_stage([(pinned.data_ptr(), dst.data_ptr(), 0)])
    torch.cuda.synchronize()
    assert eng.store_stage_stats() == before and not dst.any()                     # counters unchanged, nothing was copied
    # tickets: only the last HULC_STAGE_TICKETS - 1 can be joined
    assert eng.lib.hulc_store_stage_join(eng.ctx, 0) != 0 and eng.lib.hulc_store_stage_join(eng.ctx, t0 + 1) != 0      # never issued
    with open(os.path.join(ROOT, "include", "hulc_hip.h")) as f:
        ring = int(re.search(r"#define\s+HULC_STAGE_TICKETS\s+(\d+)", f.read()).group(1))
    assert eng.get_option("stage_tickets") == ring                                 # the library was compiled with the header's ring
    tickets = [eng.store_stage([(pinned.data_ptr(), dst.data_ptr(), 64)]) for _ in range(ring)]
    assert tickets == list(range(t0 + 1, t0 + 1 + ring))
    assert eng.lib.hulc_store_stage_join(eng.ctx, t0) != 0                         # older than the event ring
    assert eng.lib.hulc_store_stage_join(eng.ctx, tickets[0]) != 0                 # its pair is the next to be reused
    eng.store_stage_join(tickets[1])
    eng.store_stage_join(tickets[-1])
    torch.cuda.synchronize()
    assert eng.store_stage_stats() == dict(calls=1 + ring, copies=1 + ring, bytes=4096 + 64 * ring)
    eng.close()


def test_calvin_datamodule_with_a_host_tier_trains_like_the_resident_one(tmp_path):
    """The tiny CALVIN directory of the store-window tests; resident_gb = 75 frames: validation (30 frames) resident, training gets 45 -> its cut falls
    after episode 0 (40 frames) and episode 1 (25 frames) lives on the host.  One epoch, fp32: the windows drawn and every step's loss equal the run
    with resident_gb = None, no persistent recurrence fell back, and host-tier windows were in fact staged."""
    from hulc_amd import config
    from hulc_amd.trainer import Trainer
    from hulc_amd.training import CONF_DIR, make_datamodule, trainer_kwargs
    from hulc_amd.utils.calvin_store import FRAME_BYTES
    root = U.write_dataset(tmp_path / "data", seed=3)

    def fit(resident_gb, tag):
        cfg = config.compose(CONF_DIR, "config", ["datamodule=calvin_store", f"datamodule.root_data_dir={root}", "datamodule.batch_size=2", "datamodule.min_window_size=5",
                                                  "datamodule.max_window_size=8", f"datamodule.resident_gb={resident_gb}", "trainer.precision=fp32", "trainer.max_epochs=1",
                                                  "model.max_batch_size=4", "model.val_instructions={open_drawer: [open the drawer], push_block: [push the block]}",
                                                  f"log_dir={tmp_path / tag}"])
        dm = make_datamodule(cfg, "cuda:0")
        dm.record_windows = True
        model = config.instantiate(cfg.model, device="cuda:0", max_seq_len=cfg.datamodule.max_window_size)
        tr = Trainer(**trainer_kwargs(cfg), log_every=1)
        hist = tr.fit(model, dm)
        out = dict(dm=dm, losses=[h["loss"] for h in hist], val=dict(tr.val_history[-1]), stats=model.engine.store_stage_stats(),
                   fallbacks=model.engine.get_option("persistent_rnn_fallbacks"))
        model.engine.close()
        return out

    a = fit("null", "resident")
    b = fit((75 * FRAME_BYTES + 1) / 2 ** 30, "tiered")
    st = b["dm"].stores
    assert not a["dm"].stores["train"].tiered and a["stats"]["calls"] == 0
    assert st["train"].tiered and st["train"].R == 40 and st["train"].host_static.shape[0] == 25 and st["train"].ring.n_slots == 2 * 2 * 2 and st["train"].ring.slot_frames == 8
    assert st["val"].R == 30 and st["val"].host_static is None
    assert len(a["dm"].window_log) == len(b["dm"].window_log) > 0
    for wa, wb in zip(a["dm"].window_log, b["dm"].window_log):
        assert wa["split"] == wb["split"] and wa["modality"] == wb["modality"] and np.array_equal(wa["starts"], wb["starts"]) and np.array_equal(wa["lens"], wb["lens"])
    print(f"[store tiers datamodule] losses resident {a['losses'][:4]}.. tiered {b['losses'][:4]}.. staged {b['stats']}")
    assert len(a["losses"]) == b["dm"].steps_per_epoch and a["losses"] == b["losses"]
    assert a["val"] == b["val"]
    n_host = sum(int((w["starts"] >= 40).sum()) for w in b["dm"].window_log if w["split"] == "train")
    assert n_host > 0 and b["stats"]["copies"] == 2 * n_host and b["fallbacks"] == 0 and a["fallbacks"] == 0
