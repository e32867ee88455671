"""CPU (-m "not gpu"): the window rules of the frame store's samplers (hulc_amd/utils/frame_store.py; restated from calvin_agent's datasets:
min_window_size .. max_window_size frames, inside one episode / one annotated segment) as properties over many draws, and the host side of
CalvinStoreDataModule (steps_per_epoch per rank).  FrameStore(device="cpu") serves the samplers only; nothing here computes on a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import store_windows_util as U  # noqa: E402
from hulc_amd.utils.frame_store import FrameStore  # noqa: E402

MINW, MAXW, AUXW, DRAWS = 5, 8, 3, 2000
ENDS = [40, 65]                                            # the 40- and the 25-frame episode back to back
SEGMENTS = [(3, 20), (42, 55), (22, 39), (57, 62)]         # inclusive; the last holds 6 frames: 2 valid starts < AUXW


@pytest.fixture(scope="module")
def store():
    z = lambda h: torch.zeros(ENDS[-1], h, h, 3, dtype=torch.uint8)
    return FrameStore(z(2), z(2), episode_ends=ENDS, device="cpu", lang=torch.zeros(len(SEGMENTS), 384), lang_segments=SEGMENTS,
                      aux_lang_loss_window=AUXW)


@pytest.fixture(scope="module")
def draws(store):
    s, l = store.sample_windows(DRAWS, MINW, MAXW, np.random.default_rng(0))
    return s.numpy(), l.numpy()


def test_vis_windows_lie_inside_one_episode_and_within_bounds(store, draws):
    s, l = draws
    assert s.dtype == np.int64 and l.dtype == np.int32 and s.shape == l.shape == (DRAWS,)
    assert l.min() >= MINW and l.max() <= MAXW
    ep_of = lambda i: np.searchsorted(np.asarray(ENDS), i, side="right")
    assert np.all(s >= 0) and np.all(s + l <= ENDS[-1])
    assert np.array_equal(ep_of(s), ep_of(s + l - 1))
    assert set(np.unique(l)) == set(range(MINW, MAXW + 1))                      # every length occurs
    pop = store.valid_starts(MINW)
    assert set(np.unique(s)) <= set(pop.tolist()) and len(pop) == (40 - MINW + 1) + (25 - MINW + 1)


def test_a_start_with_six_frames_left_only_gets_lens_five_and_six(store):
    class Fixed:                                                                # a generator whose start draw always picks population entry k
        def __init__(self, k, seed):
            self.k, self.g, self.first = k, np.random.default_rng(seed), True

        def integers(self, lo, hi, size=None):
            if self.first:
                self.first = False
                return np.full(size, self.k, np.int64)
            return self.g.integers(lo, hi, size=size)
    pop = store.valid_starts(MINW)
    for start in (34, 59):                                                      # 40 - 34 = 65 - 59 = 6 frames left
        k = int(np.nonzero(pop == start)[0][0])
        s, l = store.sample_windows(DRAWS, MINW, MAXW, Fixed(k, start))
        assert np.all(s.numpy() == start)
        assert set(np.unique(l.numpy())) == {5, 6}
    assert np.array_equal(store.frames_left(np.array([0, 34, 39, 40, 59, 64])), [40, 6, 1, 25, 6, 1])


def test_lang_windows_stay_inside_their_segment_with_the_right_row_and_aux_flag(store):
    s, l, rows, aux = (x.numpy() for x in store.sample_lang_windows(DRAWS, MINW, MAXW, np.random.default_rng(1)))
    assert l.dtype == np.int32 and rows.dtype == np.int32 and aux.dtype == bool
    seg = np.asarray(SEGMENTS)
    a, e = seg[rows, 0], seg[rows, 1]                                           # default rows: segment i -> table row i
    assert np.all(s >= a) and np.all(s + l - 1 <= e)
    assert np.all(s <= e - MINW + 1) and l.min() >= MINW and l.max() <= MAXW
    assert set(np.unique(rows)) == set(range(len(SEGMENTS)))
    assert set(np.unique(l)) == set(range(MINW, MAXW + 1))
    last_valid = e - MINW + 1
    want = s > last_valid - AUXW                                                # among the last AUXW valid starts of the segment
    assert np.array_equal(aux, want) and aux.any() and not aux.all()
    assert np.all(aux[rows == 3])                                               # a segment with fewer valid starts than the window: all flagged
    for i, (a_i, e_i) in enumerate(SEGMENTS):                                   # exactly min(AUXW, valid starts) distinct flagged starts per segment
        assert len(np.unique(s[(rows == i) & aux])) == min(AUXW, e_i - MINW + 2 - a_i)


def test_lang_rows_map_segments_to_table_rows():
    z = lambda h: torch.zeros(65, h, h, 3, dtype=torch.uint8)
    st = FrameStore(z(2), z(2), episode_ends=ENDS, device="cpu", lang=torch.zeros(9, 384), lang_segments=SEGMENTS[:2], lang_rows=[7, 5])
    s, l, rows, aux = (x.numpy() for x in st.sample_lang_windows(200, MINW, MAXW, np.random.default_rng(2)))
    assert set(np.unique(rows)) == {5, 7}
    assert np.all(s[rows == 7] <= 20 - MINW + 1) and np.all(s[rows == 5] >= 42)
    with pytest.raises(ValueError):
        FrameStore(z(2), z(2), episode_ends=ENDS, device="cpu", lang=torch.zeros(2, 384), lang_segments=[(3, 70)])


def test_valid_start_populations_are_cached(store):
    assert store.valid_starts(MINW) is store.valid_starts(MINW)
    assert store.valid_lang_starts(MINW) is store.valid_lang_starts(MINW)
    assert store.valid_starts(MINW) is not store.valid_starts(MAXW)
    with pytest.raises(ValueError):
        store.sample_windows(4, 41, 41)                                         # no episode holds 41 frames
    with pytest.raises(ValueError):
        store.sample_windows(4, 6, 5)


def test_batch_without_an_engine_refuses_variable_length_windows(store):
    st = FrameStore(store.rgb_static, store.rgb_gripper, episode_ends=ENDS, device="cpu", actions=torch.zeros(65, 7), robot_obs=torch.zeros(65, 15))
    s, l = st.sample_windows(4, MINW, MAXW, np.random.default_rng(3))
    with pytest.raises(ValueError):                                             # the padding rules live in hulc_store_gather: no torch fall-back
        st.batch(s, MAXW, lens=l)
    d = st.batch(torch.tensor([0, 64, -3, 30]), MAXW)                           # fixed windows: starts clamped once, for frames and tables alike
    assert d["window_start"].tolist() == [0, 65 - MAXW, 0, 30] and "window_len" not in d


def test_datamodule_steps_per_epoch_is_the_same_on_every_rank(tmp_path):
    from hulc_amd.utils.calvin_store import CalvinStoreDataModule
    root = U.write_dataset(tmp_path / "data", small_frames=True)
    kw = dict(root_data_dir=root, batch_size=2, min_window_size=MINW, max_window_size=MAXW, device="cpu")
    dms = [CalvinStoreDataModule(rank=r, world=2, **kw) for r in (0, 1)]
    valid = (40 - MINW + 1) + (25 - MINW + 1)
    assert dms[0].steps_per_epoch == dms[1].steps_per_epoch == valid // (2 * 2)
    assert CalvinStoreDataModule(rank=0, world=1, **kw).steps_per_epoch == valid // 2
    assert dms[0].stores["train"].F == 40 and dms[1].stores["train"].F == 25   # rank r keeps the episodes with index % world == r
    assert dms[0].stores["train"].lang_rows.tolist() == [0, 2] and dms[1].stores["train"].lang_rows.tolist() == [1]
    assert dms[1].stores["train"].lang_segments.tolist() == [[2, 15]]           # frame ids 42..55 of the episode that starts at 40
    assert dms[0].stores["val"].F == dms[1].stores["val"].F == 30               # fewer episodes than ranks: kept whole
    ds = dms[0].train_datasets["lang"]
    assert os.path.exists(os.path.join(ds.abs_datasets_dir, ds.lang_folder, "auto_lang_ann.npy")) and len(ds.lang_lookup) == 3
    with pytest.raises(RuntimeError):                                           # no engine attached: no batches
        next(iter(dms[0].train_dataloader()))
    with pytest.raises(FileNotFoundError):
        CalvinStoreDataModule(root_data_dir=str(tmp_path / "nope"), device="cpu", rank=0, world=1)


def test_calvin_store_conf_composes():
    from hulc_amd import config
    from hulc_amd.training import CONF_DIR
    cfg = config.compose(CONF_DIR, "config", ["datamodule=calvin_store", "datamodule.root_data_dir=/data/task_D_D"])
    assert cfg.datamodule._target_ == "hulc_amd.utils.calvin_store.CalvinStoreDataModule"
    assert (cfg.datamodule.min_window_size, cfg.datamodule.max_window_size, cfg.datamodule.aux_lang_loss_window) == (20, 32, 8)
    assert cfg.datamodule.root_data_dir == "/data/task_D_D" and cfg.datamodule.lang_folder == "lang_annotations"
