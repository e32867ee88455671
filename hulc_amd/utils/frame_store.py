"""HBM-resident frame store: the MI355X-first replacement for the reference's host-side shared-memory frame cache.

The reference keeps the CALVIN episodes' frames in host shared memory (README.md:85-86: ~20 minutes to fill; dataset/README.md:55-56) and every step
converts uint8 -> fp32, applies the transforms on the CPU and copies a (B,S,3,H,W) fp32 batch to the GPU.  A MI355X holds 288 GB: the uint8 frames of a
training split live ON the device (`FrameStore`), a batch is B window starts, and conv1 gathers the windows by index (include/hulc_hip.h:
hulc_batch::window_start; scale / normalise / RandomShiftsAug run inside conv1's load path as for any uint8 batch).  Per step nothing but the indices,
the (B,S,7) actions and (B,S,15) robot_obs cross PCIe — or nothing at all if those live on the device too (`actions` / `robot_obs` arguments).

    store = FrameStore(rgb_static_u8, rgb_gripper_u8, episode_ends=[...], device="cuda:0")       # (F,200,200,3), (F,84,84,3) uint8, once
    starts = store.sample_starts(B, S, generator)                                                 # (B,) int64: every window inside ONE episode
    batch = {"vis": store.batch(starts, S, actions, robot_obs, shifts=True, generator=g)}         # reference-shaped dict for Hulc.training_step

Variable-length windows (the reference's datasets: min_window_size..max_window_size frames, padded to the maximum — vision.yaml / lang.yaml):

    starts, lens = store.sample_windows(B, 20, 32, generator)                                     # a window of lens[b] real frames inside one episode
    batch = {"vis": store.batch(starts, 32, lens=lens, shifts=True, engine=module.engine)}        # hulc_batch::window_len + hulc_store_gather

The window rules are restated from calvin_agent (whose source is not part of the reference tree): a start is valid if at least `min_window` frames
remain in its episode (lang: its annotated segment), the length is uniform in [min_window, min(max_window, frames remaining)], the window is padded
to max_window by repeating its last frame (relative actions: zeros, gripper repeated).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch


class FrameStore:
    def __init__(self, rgb_static: torch.Tensor, rgb_gripper: torch.Tensor, episode_ends: Optional[Sequence[int]] = None, device="cuda:0",
                 actions: Optional[torch.Tensor] = None, robot_obs: Optional[torch.Tensor] = None, pad_static: int = 10, pad_gripper: int = 4,
                 lang: Optional[torch.Tensor] = None, lang_segments: Optional[Sequence] = None, aux_lang_loss_window: int = 8,
                 lang_rows: Optional[Sequence[int]] = None):
        """rgb_static (F,H,W,3) / rgb_gripper (F,h,w,3): uint8, the frames of all episodes back to back; episode_ends: exclusive end index of every
        episode (ascending, last == F; default: one episode).  actions (F,7) / robot_obs (F,15): optional per-frame fp32 tables kept on the device too.
        lang (A,384): optional language table; lang_segments: (start_i, end_i) store indices, INCLUSIVE ends, of the annotated segments; lang_rows: the
        table row of each segment (default: segment i -> row i)."""
        if rgb_static.dtype != torch.uint8 or rgb_gripper.dtype != torch.uint8 or rgb_static.dim() != 4 or rgb_gripper.dim() != 4:
            raise ValueError("FrameStore expects uint8 (F,H,W,3) tensors")
        if rgb_static.shape[0] != rgb_gripper.shape[0] or rgb_static.shape[-1] != 3 or rgb_gripper.shape[-1] != 3:
            raise ValueError("both cameras must hold the same F frames, channels last")
        self.device = torch.device(device)
        self.rgb_static = rgb_static.to(self.device).contiguous()
        self.rgb_gripper = rgb_gripper.to(self.device).contiguous()
        self.F = int(rgb_static.shape[0])
        ends = np.asarray([self.F] if episode_ends is None else list(episode_ends), np.int64)
        if ends.size == 0 or ends[-1] != self.F or np.any(np.diff(np.concatenate([[0], ends])) <= 0):
            raise ValueError("episode_ends must be ascending exclusive end indices whose last entry is F")
        self.episode_ends = ends
        self.episode_starts = np.concatenate([[0], ends[:-1]])
        self.actions = None if actions is None else actions.to(self.device, torch.float32).contiguous()
        self.robot_obs = None if robot_obs is None else robot_obs.to(self.device, torch.float32).contiguous()
        self.pad_static, self.pad_gripper = int(pad_static), int(pad_gripper)
        self.lang = None if lang is None else lang.to(self.device, torch.float32).reshape(-1, 384).contiguous()
        seg = np.zeros((0, 2), np.int64) if lang_segments is None else np.asarray(list(lang_segments), np.int64).reshape(-1, 2)
        if seg.size and (np.any(seg[:, 0] < 0) or np.any(seg[:, 1] >= self.F) or np.any(seg[:, 1] < seg[:, 0])):
            raise ValueError("lang_segments must be (start, end) store indices with 0 <= start <= end < F (inclusive ends)")
        self.lang_segments = seg
        self.lang_rows = np.arange(len(seg), dtype=np.int64) if lang_rows is None else np.asarray(list(lang_rows), np.int64)
        if len(self.lang_rows) != len(seg) or (len(seg) and self.lang is not None and (self.lang_rows.min() < 0 or self.lang_rows.max() >= self.lang.shape[0])):
            raise ValueError("lang_rows must name one row of the lang table per segment")
        self.aux_lang_loss_window = int(aux_lang_loss_window)
        self.engine = None                         # StepEngine whose stream the table gathers run on (attach(); hulc_store_gather)
        self._valid: Dict[int, np.ndarray] = {}    # window size -> valid-start population, built once
        self._valid_lang: Dict[int, tuple] = {}

    def attach(self, engine) -> "FrameStore":
        """The StepEngine that gathers actions / robot_obs / lang from the store's tables (hulc_store_gather, on the engine's stream)."""
        self.engine = engine
        return self

    def bytes(self) -> int:
        return self.rgb_static.numel() + self.rgb_gripper.numel()

    def valid_starts(self, S: int) -> np.ndarray:
        """Every start index with at least S frames left in ITS episode (host array; the sampling population, hulc's disk datasets index the same way).
        Built once per window size and cached: treat the array as read-only."""
        S = int(S)
        pop = self._valid.get(S)
        if pop is None:
            parts = [np.arange(a, b - S + 1, dtype=np.int64) for a, b in zip(self.episode_starts, self.episode_ends) if b - a >= S]
            pop = self._valid[S] = np.concatenate(parts) if parts else np.zeros((0,), np.int64)
        return pop

    def frames_left(self, starts: np.ndarray) -> np.ndarray:
        """Frames from each start to the end of its episode (the start's own frame included)."""
        starts = np.asarray(starts, np.int64)
        return self.episode_ends[np.searchsorted(self.episode_ends, starts, side="right")] - starts

    def sample_windows(self, B: int, min_window: int, max_window: int, generator: Optional[np.random.Generator] = None):
        """B variable-length windows: a start with at least `min_window` frames left in its episode, and a length uniform in
        [min_window, min(max_window, frames left)] -> (starts (B,) int64, lens (B,) int32), both on the store's device."""
        if not 1 <= int(min_window) <= int(max_window):
            raise ValueError(f"need 1 <= min_window <= max_window (got {min_window}, {max_window})")
        pop = self.valid_starts(min_window)
        if pop.size == 0:
            raise ValueError(f"no episode of the store holds {min_window} frames")
        g = generator or np.random.default_rng()
        starts = pop[g.integers(0, pop.size, size=B)]
        hi = np.minimum(int(max_window), self.frames_left(starts))
        lens = g.integers(int(min_window), hi + 1)
        return torch.from_numpy(starts).to(self.device), torch.from_numpy(lens.astype(np.int32)).to(self.device)

    def valid_lang_starts(self, min_window: int):
        """(starts, segment index, aux flag) of every lang start: s in [start_i, end_i - min_window + 1] for segment i; aux = s is among the last
        `aux_lang_loss_window` valid starts of its segment.  Built once per window size and cached."""
        m = int(min_window)
        hit = self._valid_lang.get(m)
        if hit is None:
            st, sg, ax = [], [], []
            for i, (a, e) in enumerate(self.lang_segments):
                s = np.arange(a, e - m + 2, dtype=np.int64)
                st.append(s); sg.append(np.full(s.shape, i, np.int64)); ax.append(s > e - m + 1 - self.aux_lang_loss_window)
            cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros((0,), dt)
            hit = self._valid_lang[m] = (cat(st, np.int64), cat(sg, np.int64), cat(ax, bool))
        return hit

    def sample_lang_windows(self, B: int, min_window: int, max_window: int, generator: Optional[np.random.Generator] = None):
        """B language windows, each inside ONE annotated segment (start_i, end_i): length uniform in [min_window, min(max_window, end_i - s + 1)].
        -> (starts int64, lens int32, lang table rows int32, use_for_aux_lang_loss bool), on the store's device."""
        if not 1 <= int(min_window) <= int(max_window):
            raise ValueError(f"need 1 <= min_window <= max_window (got {min_window}, {max_window})")
        st, sg, ax = self.valid_lang_starts(min_window)
        if st.size == 0:
            raise ValueError(f"no annotated segment of the store holds {min_window} frames")
        g = generator or np.random.default_rng()
        pick = g.integers(0, st.size, size=B)
        starts, seg = st[pick], sg[pick]
        hi = np.minimum(int(max_window), self.lang_segments[seg, 1] - starts + 1)
        lens = g.integers(int(min_window), hi + 1)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        return dev(starts), dev(lens.astype(np.int32)), dev(self.lang_rows[seg].astype(np.int32)), dev(ax[pick])

    def sample_starts(self, B: int, S: int, generator: Optional[np.random.Generator] = None) -> torch.Tensor:
        """B window starts drawn uniformly from valid_starts(S) -> (B,) int64 on the device."""
        pop = self.valid_starts(S)
        if pop.size == 0:
            raise ValueError(f"no episode of the store holds {S} frames")
        g = generator or np.random.default_rng()
        return torch.from_numpy(pop[g.integers(0, pop.size, size=B)]).to(self.device)

    def batch(self, starts: torch.Tensor, S: int, actions: Optional[torch.Tensor] = None, robot_obs: Optional[torch.Tensor] = None, shifts: bool = False,
              generator: Optional[torch.Generator] = None, lang: Optional[torch.Tensor] = None, use_for_aux: Optional[torch.Tensor] = None,
              lens: Optional[torch.Tensor] = None, lang_rows: Optional[torch.Tensor] = None, absolute: bool = False, engine=None) -> Dict:
        """The reference-shaped batch dict of one modality (hulc/models/hulc.py:395-414) for `Hulc.training_step` / `validation_step`: the stores stand in
        for rgb_obs, `window_start` names the windows.  actions / robot_obs: (B,S,7) / (B,S,15) tensors, or None to gather them from the store's own
        per-frame tables.  shifts=True draws the per-frame RandomShiftsAug offsets (transforms.py:8-29) on the device.
        lens (B,) int32: variable-length windows padded to S (`window_len`).  lang_rows (B,) int32: rows of the store's lang table (instead of `lang`).
        absolute: the actions table holds absolute targets, padding repeats all seven dims.
        With an engine (argument, or attach()) the tables are gathered by hulc_store_gather — required for `lens`, whose padding rules live there;
        without one, fixed windows are gathered by torch indexing.  The starts are clamped ONCE here, so frames and tables always name the same rows."""
        starts = starts.to(self.device, torch.int64)
        B = int(starts.shape[0])
        engine = engine if engine is not None else self.engine
        if lens is not None:
            lens = lens.to(self.device, torch.int32).clamp(1, min(int(S), self.F))
            starts = torch.minimum(starts.clamp(min=0), self.F - lens.to(torch.int64))
        else:
            if self.F < S:
                raise ValueError(f"the store holds {self.F} frames, fewer than one window of {S}")
            starts = starts.clamp(0, self.F - S)
        if lang is None and lang_rows is not None:
            if self.lang is None:
                raise ValueError("lang_rows needs a store built with its lang table")
            lang_rows = lang_rows.to(self.device, torch.int32)
        if actions is None or robot_obs is None or (lang is None and lang_rows is not None):
            if (actions is None or robot_obs is None) and (self.actions is None or self.robot_obs is None):
                raise ValueError("pass actions / robot_obs or build the store with its per-frame tables")
            if engine is not None and self.actions is not None and self.robot_obs is not None:
                a, r, l = engine.store_gather(self.actions, self.robot_obs, starts, S, window_len=lens, lang=self.lang if lang is None and lang_rows is not None else None,
                                              lang_row=lang_rows if lang is None else None, absolute=absolute)
                lang = l if lang is None else lang
            elif lens is not None:
                raise ValueError("variable-length windows gather the store's tables through hulc_store_gather: pass engine= or attach() one")
            else:
                idx = starts[:, None] + torch.arange(S, device=self.device)[None, :]
                a, r = self.actions[idx], self.robot_obs[idx]
                if lang is None and lang_rows is not None:
                    lang = self.lang[lang_rows.to(torch.int64)]
            actions = a if actions is None else actions
            robot_obs = r if robot_obs is None else robot_obs
        d = dict(rgb_obs=dict(rgb_static=self.rgb_static, rgb_gripper=self.rgb_gripper), window_start=starts, depth_obs={},
                 actions=actions.to(self.device, torch.float32), state_info=dict(robot_obs=robot_obs.to(self.device, torch.float32)),
                 robot_obs=torch.zeros(B, S, 8, device=self.device), idx=torch.arange(B, device=self.device),
                 pad_static=self.pad_static, pad_gripper=self.pad_gripper)
        if lens is not None:
            d["window_len"] = lens
        if shifts:
            d["shift_static"] = torch.randint(0, 2 * self.pad_static + 1, (B * S, 2), device=self.device, generator=generator, dtype=torch.int32)
            d["shift_gripper"] = torch.randint(0, 2 * self.pad_gripper + 1, (B * S, 2), device=self.device, generator=generator, dtype=torch.int32)
        if lang is not None:
            d["lang"] = lang.to(self.device, torch.float32)
            d["use_for_aux_lang_loss"] = (torch.ones(B, dtype=torch.bool, device=self.device) if use_for_aux is None else use_for_aux.to(self.device))
        return d

    def materialise(self, starts: torch.Tensor, S: int, lens: Optional[torch.Tensor] = None):
        """The same windows as (B,S,H,W,3) uint8 tensors (tests; the path the store exists to avoid).  lens: padded by repeating the last real frame."""
        t = torch.arange(S, device=self.device)[None, :]
        if lens is not None:
            t = torch.minimum(t, lens.to(self.device, torch.int64)[:, None] - 1)
        idx = (starts.to(self.device, torch.int64)[:, None] + t).reshape(-1)
        B = int(starts.shape[0])
        return (self.rgb_static[idx].reshape(B, S, *self.rgb_static.shape[1:]).contiguous(), self.rgb_gripper[idx].reshape(B, S, *self.rgb_gripper.shape[1:]).contiguous())
