"""CALVIN dataset directory -> HBM-resident frame stores -> `Trainer.fit`.

Reads `<root_data_dir>/training` and `<root_data_dir>/validation` in the layout of the reference's dataset/README.md:50-119 — one
`episode_%07d.npz` per time step (`rgb_static`, `rgb_gripper`, `rel_actions`, `robot_obs`), `ep_start_end_ids.npy` (inclusive ends) and
`<lang_folder>/auto_lang_ann.npy` (`language.emb`, `info.indx`) — uploads every split ONCE, episode by episode, into a `FrameStore` with its per-frame and
language tables (`resident_gb`: a split larger than the budget keeps its remaining episodes in pinned host memory, staged one step ahead), and yields the reference's `{"vis": ..., "lang": ...}` batches of variable-length windows padded to `max_window_size`
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

from .frame_store import FrameStore, ragged_plan


class _LangDatasetInfo:
    """What Hulc.on_fit_start reads from `datamodule.train_datasets["lang"]` / `val_datasets["lang"]` (hulc.py:697-737): where the annotations lie
    and `lang_lookup`, batch `idx` -> annotation index.  The lang batches carry the annotation index itself as `idx`, so the lookup is the identity."""

    def __init__(self, abs_datasets_dir: str, lang_folder: str, n_annotations: int):
        self.abs_datasets_dir, self.lang_folder = abs_datasets_dir, lang_folder
        self.lang_lookup = np.arange(n_annotations, dtype=np.int64)


FRAME_BYTES = 200 * 200 * 3 + 84 * 84 * 3      # one frame of both cameras as uint8: 120 000 + 21 168 bytes


def split_budget(resident_gb: float, val_frames: int, train_frames: int, frame_bytes: int = FRAME_BYTES):
    """`resident_gb` (GiB of device memory for resident frames) over the two splits -> (resident_frames of the validation store, of the training
    store): validation is resident first, training gets the rest.  The stores cut these budgets down to an episode boundary (plan_tiers).  The
    staging ring of a split that does not fit comes on top: 2 x batch_size x modalities x max_window_size frames, 0.58 GB at the defaults."""
    left = int(float(resident_gb) * 2 ** 30) // int(frame_bytes)
    val = min(int(val_frames), left)
    return val, min(int(train_frames), left - val)


def split_episodes(split_dir: str, rank: int = 0, world: int = 1):
    """(ep (E,2) inclusive frame ids of every episode of the split, the indices of this rank's episodes, their exclusive end indices in the store)."""
    ep = np.asarray(np.load(os.path.join(split_dir, "ep_start_end_ids.npy")), np.int64).reshape(-1, 2)
    if ep.size == 0:
        raise ValueError(f"{split_dir}/ep_start_end_ids.npy lists no episode")
    # a split with fewer episodes than ranks (a tiny validation split) is kept whole on every rank
    mine = [i for i in range(len(ep)) if i % max(1, world) == rank] if len(ep) >= world else list(range(len(ep)))
    return ep, mine, np.cumsum([int(ep[i, 1] - ep[i, 0] + 1) for i in mine]).astype(np.int64)


def load_split(split_dir: str, lang_folder: str, rank: int = 0, world: int = 1, make_store=None):
    """One split of a CALVIN dataset directory as host arrays: the frames of this rank's episodes (episode index % world == rank; every
    episode if the split has fewer episodes than ranks) back to back.
    -> dict(rgb_static (F,200,200,3) u8, rgb_gripper (F,84,84,3) u8, actions (F,7), robot_obs (F,15), episode_ends (exclusive store indices),
    episode_lens of EVERY episode of the split, lang (A,384) or None, lang_segments (store indices, inclusive) + lang_rows of this rank's segments).
    make_store(F, episode_ends, static_shape, gripper_shape) -> an object with write_frames(first, rgb_static, rgb_gripper): the frames are then
    written into it ONE EPISODE at a time instead of being stacked on the host (never two copies of the split, never a whole-split upload); the
    dict carries it as `store` and its rgb_static / rgb_gripper are None."""
    ep, mine, ends = split_episodes(split_dir, rank, world)
    cols: Dict[str, List[np.ndarray]] = {k: [] for k in ("rgb_static", "rgb_gripper", "rel_actions", "robot_obs")}
    store_index: Dict[int, int] = {}
    store = None
    for i in mine:
        first = len(store_index)
        for fid in range(int(ep[i, 0]), int(ep[i, 1]) + 1):
            with np.load(os.path.join(split_dir, f"episode_{fid:07d}.npz")) as z:
                for k in cols:
                    cols[k].append(np.asarray(z[k]))
            store_index[fid] = len(store_index)
        if make_store is not None:
            if store is None:
                store = make_store(int(ends[-1]), ends, cols["rgb_static"][0].shape, cols["rgb_gripper"][0].shape)
            store.write_frames(first, np.stack(cols["rgb_static"]).astype(np.uint8, copy=False), np.stack(cols["rgb_gripper"]).astype(np.uint8, copy=False))
            cols["rgb_static"], cols["rgb_gripper"] = [], []
    frames = (lambda k: np.stack(cols[k]).astype(np.uint8, copy=False)) if make_store is None else (lambda k: None)
    out = dict(rgb_static=frames("rgb_static"), rgb_gripper=frames("rgb_gripper"), store=store,
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
    `steps_per_epoch` = valid vis starts of the WHOLE split // (batch_size x world), the same count on every rank.
    resident_gb (None: every split wholly on the device): GiB of device memory for the resident frames of both splits (split_budget) — validation resident
    first, training gets the rest; the episodes beyond a store's cut live in pinned host memory and their windows are staged into a ring of
    2 x batch_size x len(modalities) slots of max_window_size frames.  train_dataloader stages batch n + 1 before it yields batch n, so the copies
    wait only for step n - 1 and run under step n.  The windows drawn are the same as without a budget (same seed, same rng stream).
    ragged_encoders (default false): the batches carry `window_len_host`, so the perceptual encoders run on the real frames of the windows only
    (INTEGRATION.md 4f); the windows drawn and everything else in the batch are the same."""

    def __init__(self, root_data_dir: str, batch_size: int = 32, min_window_size: int = 20, max_window_size: int = 32, lang_folder: str = "lang_annotations",
                 aux_lang_loss_window: int = 8, modalities: Sequence[str] = ("vis", "lang"), pad_static: int = 10, pad_gripper: int = 4, val_batches: int = 1,
                 device: str = "cuda:0", seed: int = 0, rank: Optional[int] = None, world: Optional[int] = None, training_dir: str = "training",
                 validation_dir: str = "validation", resident_gb: Optional[float] = None, ragged_encoders: bool = False, **_unused):
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
        self.resident_gb = None if resident_gb is None else float(resident_gb)
        self.ragged_encoders = bool(ragged_encoders)      # every batch carries the host lens of its draw as window_len_host: the ragged encoder pass
        stage_slots = 2 * self.batch_size * len(self.modalities)      # two batches: the one the step reads and the one staged ahead
        budget = {"train": None, "val": None}
        if self.resident_gb is not None:
            if self.resident_gb < 0:
                raise ValueError(f"datamodule.resident_gb={resident_gb}: expected a size in GiB or null")
            n = {sub: int(split_episodes(os.path.join(str(root_data_dir), sub), self.rank, self.world)[2][-1]) for sub in (validation_dir, training_dir)}
            budget["val"], budget["train"] = split_budget(self.resident_gb, n[validation_dir], n[training_dir])
        for split, sub, info in (("train", training_dir, self.train_datasets), ("val", validation_dir, self.val_datasets)):
            d = os.path.join(str(root_data_dir), sub)

            def make_store(F, ends, shape_s, shape_g, resident=budget[split]):
                tiers = {}
                if resident is not None:       # a split that fits whole needs no ring
                    tiers = dict(resident_frames=resident, stage_slots=stage_slots if resident < F else 0, stage_slot_frames=self.S if resident < F else 0)
                return FrameStore.allocate(F, shape_s, shape_g, episode_ends=ends, device=self.device, pad_static=pad_static, pad_gripper=pad_gripper, **tiers)

            h = load_split(d, self.lang_folder, self.rank, self.world, make_store=make_store)
            t = torch.from_numpy
            st = self.stores[split] = h["store"].set_tables(t(h["actions"]), t(h["robot_obs"]))
            st.set_lang(None if h["lang"] is None else t(h["lang"]), h["lang_segments"], h["lang_rows"], aux_lang_loss_window)
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
        return self._assemble(split, self._draw(split, rng), tg)

    def _draw(self, split: str, rng: np.random.Generator):
        """The windows of one batch, per modality, and — on a tiered store — their staging started (FrameStore.stage: the copies of the host-tier
        windows are enqueued behind whatever the engine's stream holds NOW).  The host copies of the draw serve the log and the staging: nothing is
        read back from the device."""
        st, drawn = self.stores[split], {}
        if self.engine is None:
            raise RuntimeError("CalvinStoreDataModule: attach(engine) before drawing batches (Trainer.fit attaches the module's engine)")
        for m in self.modalities:
            if "lang" in m:
                starts, lens, rows, aux, (hs, hl) = st.sample_lang_windows(self.batch_size, self.min_window, self.S, rng, return_host=True)
            else:
                (starts, lens, (hs, hl)), rows, aux = st.sample_windows(self.batch_size, self.min_window, self.S, rng, return_host=True), None, None
            if self.record_windows:
                self.window_log.append(dict(split=split, modality=m, starts=hs.copy(), lens=hl.copy()))
            drawn[m] = dict(starts=starts, lens=lens, host_lens=hl, rows=rows, aux=aux, staged=st.stage(hs, self.S, hl) if st.tiered else None)
        return drawn

    def _assemble(self, split: str, drawn: Dict, tg: Optional[torch.Generator]):
        st, out = self.stores[split], {}
        for m, w in drawn.items():
            if w["rows"] is not None:
                d = st.batch(w["starts"], self.S, lens=w["lens"], lang_rows=w["rows"], use_for_aux=w["aux"], shifts=tg is not None, generator=tg, staged=w["staged"])
                d["idx"] = w["rows"].to(torch.int64)          # annotation index: lang_lookup is the identity
            else:
                d = st.batch(w["starts"], self.S, lens=w["lens"], shifts=tg is not None, generator=tg, staged=w["staged"])
            if self.ragged_encoders:      # the host array of the draw, clamped as batch() clamps the device lens: no read-back
                d["window_len_host"] = ragged_plan(w["host_lens"], self.S, st.F)[0]
            out[m] = d
        return out

    def train_dataloader(self, rank: Optional[int] = None):
        self._epoch = getattr(self, "_epoch", -1) + 1
        rng = np.random.default_rng([self.seed, self.rank, self._epoch])
        tg = torch.Generator(device=self.device)
        tg.manual_seed(self.seed * 1000003 + 7919 * self.rank + self._epoch)
        if not self.stores["train"].tiered:
            for _ in range(self.steps_per_epoch):
                yield self._batch("train", rng, tg)
            return
        # lookahead 1: batch n + 1 is drawn and its host-tier windows staged BEFORE batch n is assembled and yielded — the copies wait for step n - 1
        # (enqueued by now) and run under step n; the join of batch n + 1 is enqueued only when that batch is assembled, after step n.  The two
        # random streams (window draws: rng; shifts: tg) are separate, so each sees the order it sees without the lookahead
        cur = None
        ahead = self._draw("train", rng) if self.steps_per_epoch > 0 else None
        try:
            for i in range(self.steps_per_epoch):
                cur, ahead = ahead, None
                if i + 1 < self.steps_per_epoch:
                    ahead = self._draw("train", rng)
                yield self._assemble("train", cur, tg)
        finally:
            # an epoch cut short (limit_train_batches: Trainer.fit fetches one batch more than it runs): neither the batch staged ahead nor the one
            # yielded last may ever be run, and their slots must not stay reserved into the next epoch.  Releasing a batch that WAS run changes
            # nothing, and a reader that is already enqueued stays protected by the stream wait inside hulc_store_stage
            self._release(cur, ahead)

    @staticmethod
    def _release(*drawn) -> None:
        for d in drawn:
            for w in (d or {}).values():
                if w["staged"] is not None:
                    w["staged"].release()

    def val_dataloader(self, rank: Optional[int] = None):
        """On a tiered validation store every batch is staged and joined on the spot: no lookahead, the copies are not hidden under a step."""
        rng = np.random.default_rng([self.seed, self.rank, 0x5eed])      # fixed: the same validation windows after every epoch
        cur = None
        try:
            for _ in range(self.val_batches):
                cur = self._draw("val", rng)
                yield self._assemble("val", cur, None)
        finally:                               # limit_val_batches: a batch fetched and dropped is never marked by validate
            self._release(cur)
