"""Host side of the ragged encoder pass (hulc_batch::window_len_host): the plan arithmetic, the C-ABI field, and the way the host lens travel from
FrameStore.batch / CalvinStoreDataModule through Hulc._modality_batch into the engine's batch struct.  No device needed."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import store_windows_util as U  # noqa: E402
from hulc_amd import lib  # noqa: E402
from hulc_amd.engine import StepEngine  # noqa: E402
from hulc_amd.hulc import Hulc  # noqa: E402
from hulc_amd.utils import frame_store  # noqa: E402
from hulc_amd.utils.frame_store import FrameStore  # noqa: E402


@pytest.mark.parametrize("lens, S, F, want_L, want_off", [
    ([1, 4, 3, 2], 4, 17, [1, 4, 3, 2], [0, 1, 5, 8, 10]),                          # the small case of the GPU tests: N' = 10
    ([4, 4, 4], 4, 17, [4, 4, 4], [0, 4, 8, 12]),                                   # all full: N' = B S
    ([1, 1, 1, 1, 1], 32, 100, [1, 1, 1, 1, 1], [0, 1, 2, 3, 4, 5]),                # all ones: N' = B
    ([40, 0, -3, 33, 32], 32, 100, [32, 1, 1, 32, 32], [0, 32, 33, 34, 66, 98]),    # beyond S and below 1 are clamped
    ([8, 2, 5], 8, 3, [3, 2, 3], [0, 3, 5, 8]),                                     # a store shorter than S bounds L too
])
def test_ragged_plan_literals(lens, S, F, want_L, want_off):
    for given in (lens, np.asarray(lens, np.int32), torch.tensor(lens, dtype=torch.int32)):
        L, off, n = frame_store.ragged_plan(given, S, F)
        assert L.dtype == np.int32 and off.dtype == np.int32
        assert L.tolist() == want_L and off.tolist() == want_off and n == want_off[-1]
    with pytest.raises(ValueError):
        frame_store.ragged_plan(lens, 0, F)
    with pytest.raises(ValueError):
        frame_store.ragged_plan(lens, S, 0)


def test_batch_struct_has_the_host_field_where_the_header_puts_it(tmp_path):
    names = [f[0] for f in lib.HulcBatch._fields_]
    assert names[-2:] == ["window_len", "window_len_host"]
    src = tmp_path / "field.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hulc_hip.h"\nint main(void) {'
                   'printf("%zu %zu %zu\\n", sizeof(hulc_batch), offsetof(hulc_batch, window_len), offsetof(hulc_batch, window_len_host)); return 0; }\n')
    exe = tmp_path / "field"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, o_len, o_host = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert ctypes.sizeof(lib.HulcBatch) == size and lib.HulcBatch.window_len.offset == o_len and lib.HulcBatch.window_len_host.offset == o_host == o_len + 8


def test_library_exports_the_row_kernel_entries():
    l = lib.load()
    for name in ("hulc_k_window_compact", "hulc_k_rows_expand", "hulc_k_rows_reduce"):
        assert name in lib.EXPORTS and getattr(l, name) is not None


def _cpu_store(F=37):
    z = lambda h: torch.zeros(F, h, h, 3, dtype=torch.uint8)
    return FrameStore(z(8), z(4), episode_ends=[20, F], device="cpu")


def test_frame_store_batch_ragged_puts_host_lens_into_the_dict():
    st, S = _cpu_store(), 8
    starts = torch.tensor([35, 0, 14, -2])
    act, ro = torch.zeros(4, S, 7), torch.zeros(4, S, 15)
    for lens in (torch.tensor([5, 8, 60, 0], dtype=torch.int32), np.array([5, 8, 60, 0], np.int64)):
        d = st.batch(starts, S, actions=act, robot_obs=ro, lens=lens, ragged=True)
        h = d["window_len_host"]
        assert isinstance(h, np.ndarray) and h.dtype == np.int32 and h.tolist() == [5, 8, 8, 1]                # clamped as the device lens are
        assert d["window_len"].tolist() == [5, 8, 8, 1] and d["window_start"].tolist() == [32, 0, 14, 0]
    assert "window_len_host" not in st.batch(starts, S, actions=act, robot_obs=ro, lens=torch.tensor([5, 8, 6, 1], dtype=torch.int32))      # the default stays padded
    with pytest.raises(ValueError, match="lens"):
        st.batch(starts, S, actions=act, robot_obs=ro, ragged=True)
    # Hulc._modality_batch hands the array on as it is: it stays on the host
    d = st.batch(starts, S, actions=act, robot_obs=ro, lens=torch.tensor([5, 8, 6, 1], dtype=torch.int32), ragged=True)
    mb = Hulc._modality_batch(d, False, torch.device("cpu"))
    assert mb["window_len_host"] is d["window_len_host"]
    assert "window_len_host" not in Hulc._modality_batch({k: v for k, v in d.items() if k != "window_len_host"}, False, torch.device("cpu"))


def test_step_engine_takes_host_lens_and_refuses_device_tensors():
    B, S, F = 3, 4, 9
    u8 = lambda h: torch.zeros(F, h, h, 3, dtype=torch.uint8)
    mb = dict(rgb_static=u8(8), rgb_gripper=u8(4), actions=torch.zeros(B, S, 7))
    kept = []
    ptr = lambda x: (kept.append(x.contiguous()), kept[-1].data_ptr())[1]
    for given in (np.array([1, 4, 2], np.int32), np.array([1, 4, 2], np.int64), torch.tensor([1, 4, 2], dtype=torch.int32), torch.tensor([1, 4, 2])):
        h = StepEngine._host_lens(dict(mb, window_len_host=given))
        assert h.dtype == torch.int32 and h.device.type == "cpu" and h.is_contiguous() and h.tolist() == [1, 4, 2]
    assert StepEngine._host_lens(mb) is None
    with pytest.raises(ValueError, match="host"):
        StepEngine._ingest_fields(dict(mb, window_len_host=torch.empty(B, dtype=torch.int32, device="meta")), ptr)      # any device but the CPU
    with pytest.raises(ValueError):
        StepEngine._ingest_fields(dict(mb, window_len_host=np.array([1, 4], np.int32)), ptr)                              # not (B,)
    with pytest.raises(ValueError):                                                                                       # fp32 frames: no store to index
        StepEngine._ingest_fields(dict(mb, rgb_static=torch.zeros(B, S, 3, 8, 8), window_len_host=np.array([1, 4, 2], np.int32)), ptr)


def test_datamodule_passes_the_key_through(tmp_path):
    """CalvinStoreDataModule(ragged_encoders=True): every batch carries the host lens of its own draw (clamped like the device lens), the padded default none;
    the windows drawn are the same.  The table gathers need an engine, so they are stood in for by fixed tensors here."""
    from hulc_amd.utils.calvin_store import CalvinStoreDataModule
    root = U.write_dataset(tmp_path / "data", seed=3, small_frames=True)

    class Gather:      # what FrameStore.batch needs of an attached engine on an all-resident store
        def store_gather(self, actions, robot_obs, starts, S, window_len=None, lang=None, lang_row=None, absolute=False):
            B = starts.shape[0]
            return torch.zeros(B, S, 7), torch.zeros(B, S, 15), (None if lang is None else lang[lang_row.to(torch.int64)])

    logs = {}
    for ragged in (False, True):
        dm = CalvinStoreDataModule(str(root), batch_size=3, min_window_size=5, max_window_size=8, device="cpu", seed=1, rank=0, world=1, ragged_encoders=ragged).attach(Gather())
        dm.record_windows = True
        batches = [b for _, b in zip(range(2), dm.train_dataloader())] + list(dm.val_dataloader())
        logs[ragged] = dm.window_log
        for b in batches:
            for m in ("vis", "lang"):
                if not ragged:
                    assert "window_len_host" not in b[m]
                    continue
                h = b[m]["window_len_host"]
                assert isinstance(h, np.ndarray) and h.dtype == np.int32 and h.tolist() == b[m]["window_len"].tolist()
                assert Hulc._modality_batch(b[m], m == "lang", torch.device("cpu"))["window_len_host"] is h
    assert len(logs[True]) == len(logs[False]) > 0
    assert all(np.array_equal(a["starts"], b["starts"]) and np.array_equal(a["lens"], b["lens"]) for a, b in zip(logs[False], logs[True]))


def test_conf_default_is_off():
    from hulc_amd import config
    from hulc_amd.training import CONF_DIR
    cfg = config.compose(CONF_DIR, "config", ["datamodule=calvin_store", "datamodule.root_data_dir=/nowhere"])
    assert cfg.datamodule.ragged_encoders is False
