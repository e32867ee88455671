"""CPU (-m "not gpu"): the host-side planning of the two-tier frame store — the resident cut (plan_tiers), the staging ring (SlotRing: round-robin
hand-out, rewritten starts, the recycle guard) and the datamodule's budget split (split_budget).  Nothing here touches a device: the copies themselves
(hulc_store_stage) are covered by tests/test_gpu_store_tiers.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hulc_amd.utils.calvin_store import FRAME_BYTES, split_budget  # noqa: E402
from hulc_amd.utils.frame_store import FrameStore, SlotRing, plan_tiers  # noqa: E402

ENDS = [24, 44, 72]      # three episodes of 24, 20 and 28 frames


def test_plan_tiers_cuts_on_episode_boundaries():
    assert [plan_tiers(ENDS, b) for b in (0, 1, 23)] == [0, 0, 0]                  # below the first episode: nothing resident
    assert [plan_tiers(ENDS, b) for b in (72, 73, 10 ** 9)] == [72, 72, 72]        # at or above F: nothing on the host
    assert [plan_tiers(ENDS, b) for b in (24, 25, 43)] == [24, 24, 24]             # inside episode 1: its start
    assert [plan_tiers(ENDS, b) for b in (44, 60, 71)] == [44, 44, 44]             # inside episode 2: its start
    assert plan_tiers([5], 4) == 0 and plan_tiers([5], 5) == 5
    with pytest.raises(ValueError):
        plan_tiers([10, 10], 5)
    with pytest.raises(ValueError):
        plan_tiers([], 5)


def test_slot_ring_hands_out_round_robin_and_rewrites_starts():
    R, SF = 24, 8
    ring = SlotRing(R, 4, SF)
    starts, lens = np.array([3, 30, 16, 64, 24]), np.array([8, 5, 1, 8, 7])
    h = ring.plan(starts, lens)
    assert h.slots == [0, 1, 2] and not h.done
    assert h.frame_starts.tolist() == [3, R + 0 * SF, 16, R + 1 * SF, R + 2 * SF]  # resident windows keep their starts, the others name their slot
    assert h.table_starts.tolist() == starts.tolist()                              # the tables are gathered with the original starts
    assert h.copies == [(30, 0, 5), (64, 1, 8), (24, 2, 7)]                        # (source frame, slot, frames): only the L real frames
    assert starts.tolist() == [3, 30, 16, 64, 24]                                  # the caller's array is not written
    h.mark_enqueued()
    h2 = ring.plan(np.array([50, 2, 44]), np.array([8, 8, 2]))                     # continues at slot 3 and wraps
    assert h2.slots == [3, 0] and h2.frame_starts.tolist() == [R + 3 * SF, 2, R + 0 * SF] and h2.copies == [(50, 3, 8), (44, 0, 2)]
    h3 = ring.plan(np.array([0, 10]), np.array([8, 8]))                            # all resident: no slot, nothing to wait for
    assert h3.slots == [] and h3.copies == [] and h3.done and h3.ticket == 0 and h3.frame_starts.tolist() == [0, 10]
    assert ring.next == 1


def test_slot_ring_budget_and_slot_size_are_checked_before_anything_changes():
    ring = SlotRing(24, 2, 8)
    with pytest.raises(ValueError, match="slots"):
        ring.plan(np.array([24, 30, 50]), np.array([4, 4, 4]))                     # three host-tier windows, two slots
    with pytest.raises(ValueError, match="slot"):
        ring.plan(np.array([24]), np.array([9]))                                   # longer than a slot
    assert ring.next == 0 and ring.owner == [None, None]
    assert ring.plan(np.array([24, 30]), np.array([8, 8])).slots == [0, 1]
    with pytest.raises(ValueError):
        SlotRing(24, 2, 0)
    with pytest.raises(ValueError):
        SlotRing(24, -1, -1)


def test_recycle_guard_raises_for_an_unconsumed_generation():
    ring = SlotRing(24, 4, 8)
    a = ring.plan(np.array([30, 40]), np.array([8, 8]))                            # slots 0, 1
    b = ring.plan(np.array([50, 60]), np.array([8, 8]))                            # slots 2, 3: the batch staged ahead
    with pytest.raises(RuntimeError, match="slot 0"):
        ring.plan(np.array([25]), np.array([4]))                                   # would overwrite batch a, which no step has read yet
    assert ring.next == 0 and ring.owner[0] is a                                   # the failed call changed nothing
    a.mark_enqueued()                                                              # what StepEngine.backward / validate do
    c = ring.plan(np.array([25, 26]), np.array([4, 4]))
    assert c.slots == [0, 1]
    with pytest.raises(RuntimeError, match="slot 2"):
        ring.plan(np.array([27]), np.array([4]))
    b.release()                                                                    # a batch that is never run
    assert ring.plan(np.array([27]), np.array([4])).slots == [2]


def test_budget_split_validation_first_training_gets_the_rest():
    gb = lambda frames: (frames * FRAME_BYTES + 1) / 2 ** 30
    assert FRAME_BYTES == 141168 and FRAME_BYTES % 16 == 0 and 120000 % 16 == 0 and 21168 % 16 == 0
    assert split_budget(gb(1000), 30, 65) == (30, 65)                              # everything fits
    assert split_budget(gb(30 + 40), 30, 65) == (30, 40)                           # validation first, training gets the rest
    assert split_budget(gb(30 + 64), 30, 65) == (30, 64)
    assert split_budget(gb(30 + 65), 30, 65) == (30, 65)
    assert split_budget(gb(30), 30, 65) == (30, 0)
    assert split_budget(gb(20), 30, 65) == (20, 0)                                 # validation itself does not fit
    assert split_budget(0.0, 30, 65) == (0, 0)
    assert split_budget(1.0, 30, 2000, frame_bytes=2 ** 20) == (30, 1024 - 30)     # GiB
    assert split_budget((70 * FRAME_BYTES - 1) / 2 ** 30, 30, 65) == (30, 39)      # a byte short of 70 frames


def test_tiered_store_arguments_and_default_are_checked_on_the_host():
    import torch
    z = lambda h: torch.zeros(72, h, h, 3, dtype=torch.uint8)
    plain = FrameStore(z(2), z(2), episode_ends=ENDS, device="cpu")
    assert not plain.tiered and plain.ring is None and plain.R == 72 and plain.rgb_static.shape[0] == 72 and plain.host_static is None
    with pytest.raises(ValueError):
        plain.stage(np.array([0]), 8)                                              # staging belongs to a tiered store
    with pytest.raises(ValueError):
        FrameStore(z(2), z(2), episode_ends=ENDS, device="cpu", stage_slots=2, stage_slot_frames=8)      # a ring without a budget
    with pytest.raises(ValueError):
        FrameStore(z(2), z(2), episode_ends=ENDS, device="cpu", resident_frames=30)                      # frames on the host, no ring
    whole = FrameStore(z(2), z(2), episode_ends=ENDS, device="cpu", resident_frames=100)                 # R == F: no host tier, no ring needed
    assert whole.tiered and whole.R == 72 and whole.host_static is None and whole.rgb_static.shape[0] == 72
    rng = np.random.default_rng(0)
    s, g = (torch.from_numpy(rng.integers(0, 256, (72, h, h, 3), dtype=np.uint8)) for h in (2, 3))
    st = FrameStore(s, g, episode_ends=ENDS, device="cpu", resident_frames=30, stage_slots=4, stage_slot_frames=8)
    assert st.R == 24 and st.rgb_static.shape[0] == 24 + 32 and st.rgb_gripper.shape[0] == 24 + 32 and st.host_static.shape[0] == 48
    assert torch.equal(st.rgb_static[:24], s[:24]) and torch.equal(st.host_static, s[24:]) and torch.equal(st.host_gripper, g[24:])
    with pytest.raises(ValueError, match="engine"):
        st.stage(np.array([30]), 8, np.array([8]))                                 # a host-tier window and no engine to copy it
    assert st.ring.next == 0 and st.ring.owner == [None] * 4                       # ... reserved nothing

    class Recorder:                                                                # stands in for StepEngine.store_stage / store_stage_join
        def __init__(self):
            self.calls, self.joined = [], []

        def store_stage(self, copies):
            self.calls.append(list(copies))
            return len(self.calls)

        def store_stage_join(self, ticket):
            self.joined.append(ticket)

    rec = Recorder()
    st.attach(rec)
    with pytest.raises(ValueError, match="slots"):
        st.stage(np.full(5, 30), 8, np.full(5, 8))                                 # more host-tier windows than slots: before any copy
    assert rec.calls == []
    h = st.stage(np.array([0, 5]), 8, np.array([8, 3]))                            # resident windows cost nothing
    assert h.ticket == 0 and h.done and h.frame_starts.tolist() == [0, 5] and h.lens.tolist() == [8, 3] and h.lens.dtype == np.int32 and rec.calls == []
    h = st.stage(torch.tensor([70, 2, 44]), 8, torch.tensor([8, 8, 3], dtype=torch.int32))      # 70 + 8 > F: clamped to 64 like batch() clamps
    assert h.ticket == 1 and len(rec.calls) == 1 and h.table_starts.tolist() == [64, 2, 44] and h.frame_starts.tolist() == [24, 2, 32]
    fs, fg = 2 * 2 * 3, 3 * 3 * 3                                                  # bytes per frame of the two (tiny) cameras
    want = [(st.host_static.data_ptr() + (64 - 24) * fs, st.rgb_static.data_ptr() + 24 * fs, 8 * fs),
            (st.host_static.data_ptr() + (44 - 24) * fs, st.rgb_static.data_ptr() + 32 * fs, 3 * fs),      # only the L = 3 real frames
            (st.host_gripper.data_ptr() + (64 - 24) * fg, st.rgb_gripper.data_ptr() + 24 * fg, 8 * fg),
            (st.host_gripper.data_ptr() + (44 - 24) * fg, st.rgb_gripper.data_ptr() + 32 * fg, 3 * fg)]
    assert rec.calls[0] == want                                                    # one call, one copy per camera and host-tier window
    with pytest.raises(ValueError, match="resident cut"):
        st.stage(np.array([20]), 8, np.array([8]))                                 # not inside one episode
    d = st.batch(None, 8, actions=torch.zeros(3, 8, 7), robot_obs=torch.zeros(3, 8, 15), staged=h)
    assert rec.joined == [1] and d["staged"] is h and d["window_start"].tolist() == [24, 2, 32] and d["window_len"].tolist() == [8, 8, 3]
    assert d["rgb_obs"]["rgb_static"] is st.rgb_static and "staged" not in plain.batch(torch.tensor([0]), 8, actions=torch.zeros(1, 8, 7), robot_obs=torch.zeros(1, 8, 15))
    st.batch(None, 8, actions=torch.zeros(3, 8, 7), robot_obs=torch.zeros(3, 8, 15), staged=h)
    assert rec.joined == [1]                                                       # joined once
    # filled episode by episode
    st2 = FrameStore.allocate(72, (2, 2, 3), (3, 3, 3), episode_ends=ENDS, device="cpu", resident_frames=50, stage_slots=2, stage_slot_frames=8)
    for a, b in zip([0] + ENDS[:-1], ENDS):
        st2.write_frames(a, s[a:b].numpy(), g[a:b].numpy())
    assert st2.R == 44 and torch.equal(st2.rgb_static[:44], s[:44]) and torch.equal(st2.host_gripper, g[44:])
    with pytest.raises(ValueError):
        st2.write_frames(70, s[:5], g[:5])
    # the samplers hand back the host arrays they drew
    a, l, (ha, hl) = st.sample_windows(6, 3, 8, np.random.default_rng(1), return_host=True)
    a2, l2 = st.sample_windows(6, 3, 8, np.random.default_rng(1))
    assert np.array_equal(a.numpy(), ha) and np.array_equal(l.numpy(), hl) and torch.equal(a, a2) and torch.equal(l, l2) and hl.dtype == np.int32


class _HostEngine:
    """Stands in for the StepEngine on the CPU: counts the staging calls and gathers zero tables."""

    def __init__(self):
        self.tickets = 0

    def store_stage(self, copies):
        self.tickets += 1
        return self.tickets

    def store_stage_join(self, ticket):
        pass

    def store_gather(self, actions, robot_obs, starts, S, window_len=None, lang=None, lang_row=None, absolute=False):
        import torch
        B = int(starts.shape[0])
        return torch.zeros(B, S, 7), torch.zeros(B, S, 15), None if lang is None else torch.zeros(B, 384)


def _run(batch):
    """What StepEngine.backward / validate do for the batches they ran."""
    for d in batch.values():
        d["staged"].mark_enqueued()


def test_a_loader_cut_short_leaves_no_slot_reserved(tmp_path):
    """limit_train_batches / limit_val_batches: the trainer fetches one batch more than it runs and drops the loader.  Neither that batch nor the one
    staged ahead may keep its slots: the next epoch wraps onto them.  Everything on the host (resident_gb = 0), so every window takes a slot and a
    batch of 2 x 2 windows fills half of the ring of 8."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import store_windows_util as U
    from hulc_amd.utils.calvin_store import CalvinStoreDataModule
    root = U.write_dataset(tmp_path / "data", seed=3, small_frames=True)
    dm = CalvinStoreDataModule(root, batch_size=2, min_window_size=5, max_window_size=8, device="cpu", resident_gb=0.0, rank=0, world=1, val_batches=2)
    dm.attach(_HostEngine())
    for split in ("train", "val"):
        assert dm.stores[split].tiered and dm.stores[split].R == 0 and dm.stores[split].ring.n_slots == 8
    for loader in (dm.train_dataloader, dm.val_dataloader):
        for epoch in range(2):                                                     # two epochs of ONE batch each, as Trainer.fit takes them
            it = loader()
            _run(next(it))
            dropped = next(it)                                                     # fetched, then the loop breaks on its limit
            assert not any(d["staged"].done for d in dropped.values())
            it.close()                                                             # what dropping the generator does
            assert all(d["staged"].done for d in dropped.values())
        ring = dm.stores["train" if loader == dm.train_dataloader else "val"].ring
        assert all(h is None or h.done for h in ring.owner)
        n = 0
        for batch in loader():                                                     # and a whole epoch afterwards
            _run(batch)
            n += 1
        assert n == (dm.steps_per_epoch if loader == dm.train_dataloader else 2)
    # a batch that is neither run nor released still trips the guard: the cleanup is the loader's, not a hole in the ring
    it = dm.train_dataloader()
    next(it)                                                                       # batch 0 yielded, batch 1 staged ahead: the ring is full
    with pytest.raises(RuntimeError, match="slot"):
        next(it)                                                                   # batch 2 would take the slots of batch 0, which was never run


def test_the_engine_keeps_no_finished_handle_pending():
    """StepEngine._staged_read: handles of all-resident batches (done from the start) and released ones do not pile up when no backward follows."""
    import types
    from hulc_amd.engine import StepEngine
    ring = SlotRing(24, 4, 8)
    eng = types.SimpleNamespace(_staged_pending=[])
    for _ in range(100):
        StepEngine._staged_read(eng, dict(staged=ring.plan(np.array([0, 8]), np.array([8, 8]))))       # resident windows only
    assert eng._staged_pending == []
    for _ in range(100):                                                           # forward-only on host-tier windows, each given up afterwards
        h = ring.plan(np.array([30, 50]), np.array([8, 8]))
        StepEngine._staged_read(eng, dict(staged=h))
        StepEngine._staged_read(eng, dict(staged=h))                               # the same batch read twice is pending once
        assert eng._staged_pending == [h]
        h.release()
    assert len(eng._staged_pending) == 1
    StepEngine._staged_read(eng, dict(rgb_static=None))
    StepEngine._staged_done(eng)
    assert eng._staged_pending == []
