"""CALVIN dataset directory -> HBM-resident frame stores -> `Trainer.fit`.

Reads `<root_data_dir>/training` and `<root_data_dir>/validation` in the layout of the reference's dataset/README.md:50-119 — one
`episode_%07d.npz` per time step (`rgb_static`, `rgb_gripper`, `rel_actions`, `robot_obs`), `ep_start_end_ids.npy` (inclusive ends) and
`<lang_folder>/auto_lang_ann.npy` (`language.emb`, `info.indx`) — uploads every split ONCE into a `FrameStore` with its per-frame and language
tables, and yields the reference's `{"vis": ..., "lang": ...}` batches of variable-length windows padded to `max_window_size`
(conf/datamodule/datasets/vision_dataset/vision.yaml, lang_dataset/lang.yaml: min_window_size 20, max_window_size 32, pad true,
aux_lang_loss_window 8).  Per step nothing crosses PCIe but the window indices: frames are gathered inside conv1 (hulc_batch::window_start /
window_len), actions / robot_obs / language rows by hulc_store_gather.

The reference's own dataset classes live in calvin_agent, which is not part of the reference tree: the window rules are the ones restated in
hulc_amd/utils/frame_store.py.  Depth / tactile / proprio observation spaces and the shared-memory dataset variants are not covered.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .frame_store import FrameStore


class _LangDatasetInfo:
    """What Hulc.on_fit_start reads from `datamodule.train_datasets["lang"]` / `val_datasets["lang"]` (hulc.py:697-737): where the annotations lie
    and `lang_lookup`, batch `idx` -> annotation index.  The lang batches carry the annotation index itself as `idx`, so the lookup is the identity."""

    def __init__(self, abs_datasets_dir: str, lang_folder: str, n_annotations: int):
        self.abs_datasets_dir, self.lang_folder = abs_datasets_dir, lang_folder
        self.lang_lookup = np.arange(n_annotations, dtype=np.int64)


def load_split(split_dir: str, lang_folder: str, rank: int = 0, world: int = 1):
    """One split of a CALVIN dataset directory as host arrays: the frames of this rank's episodes (episode index % world == rank; every
    episode if the split has fewer episodes than ranks) back to back.
    -> dict(rgb_static (F,200,200,3) u8, rgb_gripper (F,84,84,3) u8, actions (F,7), robot_obs (F,15), episode_ends (exclusive store indices),
    episode_lens of EVERY episode of the split, lang (A,384) or None, lang_segments (store indices, inclusive) + lang_rows of this rank's segments)."""
    ep = np.asarray(np.load(os.path.join(split_dir, "ep_start_end_ids.npy")), np.int64).reshape(-1, 2)
    if ep.size == 0:
        raise ValueError(f"{split_dir}/ep_start_end_ids.npy lists no episode")
    # a split with fewer episodes than ranks (a tiny validation split) is kept whole on every rank
    mine = [i for i in range(len(ep)) if i % max(1, world) == rank] if len(ep) >= world else list(range(len(ep)))
    cols: Dict[str, List[np.ndarray]] = {k: [] for k in ("rgb_static", "rgb_gripper", "rel_actions", "robot_obs")}
    store_index: Dict[int, int] = {}
    ends = []
    for i in mine:
        for fid in range(int(ep[i, 0]), int(ep[i, 1]) + 1):
            with np.load(os.path.join(split_dir, f"episode_{fid:07d}.npz")) as z:
                for k in cols:
                    cols[k].append(np.asarray(z[k]))
            store_index[fid] = len(store_index)
        ends.append(len(store_index))
    out = dict(rgb_static=np.stack(cols["rgb_static"]).astype(np.uint8, copy=False), rgb_gripper=np.stack(cols["rgb_gripper"]).astype(np.uint8, copy=False),
               actions=np.stack(cols["rel_actions"]).astype(np.float32), robot_obs=np.stack(cols["robot_obs"]).astype(np.float32),
               episode_ends=np.asarray(ends, np.int64), episode_lens=ep[:, 1] - ep[:, 0] + 1, lang=None, lang_segments=np.zeros((0, 2), np.int64),
               lang_rows=np.zeros((0,), np.int64), n_annotations=0)
    ann_path = os.path.join(split_dir, lang_folder, "auto_lang_ann.npy")
    if os.path.exists(ann_path):
        ann = np.load(ann_path, allow_pickle=True).item()
        emb = np.asarray(ann["language"]["emb"], np.float32)
        indx = np.asarray(ann["info"]["indx"], np.int64).reshape(-1, 2)
        out["lang"] = emb.reshape(len(indx), -1)
        out["n_annotations"] = len(indx)
        keep = [j for j, (a, e) in enumerate(indx) if int(a) in store_index and int(e) in store_index]      # segments of this rank's episodes
        out["lang_segments"] = np.asarray([(store_index[int(indx[j, 0])], store_index[int(indx[j, 1])]) for j in keep], np.int64).reshape(-1, 2)
        out["lang_rows"] = np.asarray(keep, np.int64)
    return out


class CalvinStoreDataModule:
    """conf/datamodule/calvin_store.yaml.  Training: `steps_per_epoch` batches per epoch of `batch_size` windows per modality with RandomShiftsAug
    shifts; validation: the same without shifts, from a fixed seed.  Data parallel: rank r keeps the episodes with index % world == r, and
    `steps_per_epoch` = valid vis starts of the WHOLE split // (batch_size x world), the same count on every rank."""

    def __init__(self, root_data_dir: str, batch_size: int = 32, min_window_size: int = 20, max_window_size: int = 32, lang_folder: str = "lang_annotations",
                 aux_lang_loss_window: int = 8, modalities: Sequence[str] = ("vis", "lang"), pad_static: int = 10, pad_gripper: int = 4, val_batches: int = 1,
                 device: str = "cuda:0", seed: int = 0, rank: Optional[int] = None, world: Optional[int] = None, training_dir: str = "training",
                 validation_dir: str = "validation", **_unused):
        if not root_data_dir or not os.path.isdir(str(root_data_dir)):
            raise FileNotFoundError(f"datamodule.root_data_dir={root_data_dir!r} is not a directory")
        if rank is None or world is None:
            from .. import parallel
            rank, world = parallel.rank(), parallel.world_size()
        self.rank, self.world = int(rank), max(1, int(world))
        self.batch_size, self.S, self.min_window = int(batch_size), int(max_window_size), int(min_window_size)
        if not 1 <= self.min_window <= self.S:
            raise ValueError(f"need 1 <= min_window_size <= max_window_size (got {min_window_size}, {max_window_size})")
        self.modalities = list(modalities)
        self.device, self.seed, self.val_batches = torch.device(device), int(seed), int(val_batches)
        self.lang_folder = str(lang_folder)
        self.stores: Dict[str, FrameStore] = {}
        self.train_datasets, self.val_datasets = {}, {}
        for split, sub, info in (("train", training_dir, self.train_datasets), ("val", validation_dir, self.val_datasets)):
            d = os.path.join(str(root_data_dir), sub)
            h = load_split(d, self.lang_folder, self.rank, self.world)
            t = torch.from_numpy
            self.stores[split] = FrameStore(t(h["rgb_static"]), t(h["rgb_gripper"]), episode_ends=h["episode_ends"], device=self.device, actions=t(h["actions"]),
                                            robot_obs=t(h["robot_obs"]), pad_static=pad_static, pad_gripper=pad_gripper,
                                            lang=None if h["lang"] is None else t(h["lang"]), lang_segments=h["lang_segments"],
                                            aux_lang_loss_window=aux_lang_loss_window, lang_rows=h["lang_rows"])
            if h["lang"] is not None:
                info["lang"] = _LangDatasetInfo(d, self.lang_folder, h["n_annotations"])
            if split == "train":      # from the WHOLE split, so that every rank takes the same number of optimizer steps
                self.steps_per_epoch = int(np.maximum(h["episode_lens"] - self.min_window + 1, 0).sum()) // (self.batch_size * self.world)
        if any("lang" in m for m in self.modalities) and "lang" not in self.train_datasets:
            raise FileNotFoundError(f"modalities {self.modalities} need {training_dir}/{self.lang_folder}/auto_lang_ann.npy")
        self.engine = None
        self.window_log: List[Dict] = []      # with record_windows: (split, modality, starts, lens) of every batch drawn (tests)
        self.record_windows = False

    def attach(self, engine) -> "CalvinStoreDataModule":
        """The StepEngine whose stream the table gathers run on (Hulc.engine); Trainer.fit attaches the module's."""
        self.engine = engine
        for s in self.stores.values():
            s.attach(engine)
        return self

    def _batch(self, split: str, rng: np.random.Generator, tg: Optional[torch.Generator]):
        st, out = self.stores[split], {}
        if self.engine is None:
            raise RuntimeError("CalvinStoreDataModule: attach(engine) before drawing batches (Trainer.fit attaches the module's engine)")
        for m in self.modalities:
            if "lang" in m:
                starts, lens, rows, aux = st.sample_lang_windows(self.batch_size, self.min_window, self.S, rng)
                d = st.batch(starts, self.S, lens=lens, lang_rows=rows, use_for_aux=aux, shifts=tg is not None, generator=tg)
                d["idx"] = rows.to(torch.int64)          # annotation index: lang_lookup is the identity
            else:
                starts, lens = st.sample_windows(self.batch_size, self.min_window, self.S, rng)
                d = st.batch(starts, self.S, lens=lens, shifts=tg is not None, generator=tg)
            if self.record_windows:
                self.window_log.append(dict(split=split, modality=m, starts=starts.cpu().numpy(), lens=lens.cpu().numpy()))
            out[m] = d
        return out

    def train_dataloader(self, rank: Optional[int] = None):
        self._epoch = getattr(self, "_epoch", -1) + 1
        rng = np.random.default_rng([self.seed, self.rank, self._epoch])
        tg = torch.Generator(device=self.device)
        tg.manual_seed(self.seed * 1000003 + 7919 * self.rank + self._epoch)
        for _ in range(self.steps_per_epoch):
            yield self._batch("train", rng, tg)

    def val_dataloader(self, rank: Optional[int] = None):
        rng = np.random.default_rng([self.seed, self.rank, 0x5eed])      # fixed: the same validation windows after every epoch
        for _ in range(self.val_batches):
            yield self._batch("val", rng, None)
