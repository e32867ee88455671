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

A split larger than HBM: `resident_frames=` keeps as many whole episodes resident as fit, the others stay in pinned host memory and the host-tier windows of
the NEXT batch are copied by the copy engines into a ring of staging slots at the tail of the same device allocation (`stage` / `batch(staged=)`).

The window rules are restated from calvin_agent (whose source is not part of the reference tree): a start is valid if at least `min_window` frames
remain in its episode (lang: its annotated segment), the length is uniform in [min_window, min(max_window, frames remaining)], the window is padded
to max_window by repeating its last frame (relative actions: zeros, gripper repeated).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch


def plan_tiers(episode_ends: Sequence[int], resident_frames: int) -> int:
    """The resident cut R of a two-tier store: the largest episode boundary <= resident_frames — 0 (nothing resident) below the first episode's
    length, F (nothing on the host) at or above F.  Frames [0, R) stay in HBM, [R, F) in pinned host memory; windows never cross an episode, so
    every window lies wholly in one tier.  Plain host arithmetic."""
    ends = np.asarray(list(episode_ends), np.int64)
    if ends.size == 0 or np.any(np.diff(np.concatenate([[0], ends])) <= 0):
        raise ValueError("episode_ends must be ascending exclusive end indices")
    fit = ends[ends <= int(resident_frames)]
    return int(fit[-1]) if fit.size else 0


def ragged_plan(lens, S: int, store_frames: int):
    """The host arithmetic of the ragged encoder pass (include/hulc_hip.h hulc_batch::window_len_host), restated: -> (L, offsets, n_real) with
    L[b] = clamp(lens[b], 1, min(S, store_frames)) (B,) int32, offsets[b] = sum of L[:b] (B + 1,) int32 and n_real = offsets[B] = N', the number of
    frames the perceptual encoders run on.  Compact frame offsets[b] + t (t < L[b]) is frame t of window b; batch row (b, t) reads compact row
    offsets[b] + min(t, L[b] - 1).  Plain host arithmetic."""
    if int(S) < 1 or int(store_frames) < 1:
        raise ValueError(f"ragged_plan needs S >= 1 and store_frames >= 1 (got {S}, {store_frames})")
    ln = np.asarray(lens.detach().cpu().numpy() if torch.is_tensor(lens) else lens).astype(np.int64).reshape(-1)
    L = np.clip(ln, 1, min(int(S), int(store_frames))).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(L, dtype=np.int64)]).astype(np.int32)
    return L, offsets, int(offsets[-1])


class StagedWindows:
    """What `FrameStore.stage` hands back for one batch of windows: `frame_starts` (B,) int64, the starts to put into `window_start` — resident windows
    keep theirs, host-tier windows name their staging slot —, `table_starts` the original ones for the per-frame tables, `lens`, the `ticket` of the
    copies (0: every window was resident) and the `slots` taken.  The slots stay reserved until the engine has ENQUEUED the last reader of the batch
    (`mark_enqueued`, called by StepEngine.backward / validate) or the batch is given up (`release`)."""

    def __init__(self, frame_starts: np.ndarray, table_starts: np.ndarray, lens: Optional[np.ndarray], slots: Sequence[int], copies: Sequence[tuple]):
        self.frame_starts, self.table_starts, self.lens = frame_starts, table_starts, lens
        self.slots, self.copies = list(slots), list(copies)      # copies: (source store frame, slot, frames) per host-tier window
        self.ticket = 0
        self.done = len(self.slots) == 0
        self.joined = False

    def mark_enqueued(self) -> None:
        self.done = True

    def release(self) -> None:
        self.done = True


class SlotRing:
    """The staging ring of a two-tier store, host bookkeeping only: `n_slots` slots of `slot_frames` frames behind the R resident frames, handed out
    round-robin.  Slot j = device frames [R + j slot_frames, R + (j + 1) slot_frames).  A slot whose last batch has not been marked or released is
    never handed out again: `plan` raises instead of overwriting frames a step may still read."""

    def __init__(self, R: int, n_slots: int, slot_frames: int):
        if n_slots < 0 or slot_frames < 0 or (n_slots > 0) != (slot_frames > 0):
            raise ValueError(f"a staging ring needs stage_slots and stage_slot_frames both > 0 or both 0 (got {n_slots}, {slot_frames})")
        self.R, self.n_slots, self.slot_frames = int(R), int(n_slots), int(slot_frames)
        self.next = 0
        self.owner: list = [None] * self.n_slots

    def slot_base(self, j: int) -> int:
        return self.R + int(j) * self.slot_frames

    def plan(self, starts: np.ndarray, lens: np.ndarray) -> StagedWindows:
        """starts / lens (B,): clamped window starts and real lengths.  Windows with start >= R take the next slots of the ring.  Nothing is changed
        when the call fails: ValueError if it needs more slots than the ring has or a window longer than a slot, RuntimeError if a slot it would
        take still belongs to a batch the engine has not finished enqueuing."""
        starts, lens = np.asarray(starts, np.int64), np.asarray(lens, np.int64)
        host = np.nonzero(starts >= self.R)[0]
        if host.size > self.n_slots:
            raise ValueError(f"{host.size} host-tier windows in one call, the staging ring has {self.n_slots} slots")
        if host.size and int(lens[host].max()) > self.slot_frames:
            raise ValueError(f"a window of {int(lens[host].max())} frames does not fit a staging slot of {self.slot_frames}")
        take = [(self.next + i) % self.n_slots for i in range(host.size)]
        for j in take:
            if self.owner[j] is not None and not self.owner[j].done:
                raise RuntimeError(f"staging slot {j} still belongs to a batch whose backward / validate has not been enqueued: run it, or release() its "
                                   "handle, before staging further ahead (stage_slots bounds the lookahead)")
        frame_starts = starts.copy()
        copies = []
        for b, j in zip(host, take):
            frame_starts[b] = self.slot_base(j)
            copies.append((int(starts[b]), j, int(lens[b])))
        h = StagedWindows(frame_starts, starts.copy(), None, take, copies)
        for j in take:
            self.owner[j] = h
        if take:
            self.next = (take[-1] + 1) % self.n_slots
        return h


class FrameStore:
    def __init__(self, rgb_static: torch.Tensor, rgb_gripper: torch.Tensor, episode_ends: Optional[Sequence[int]] = None, device="cuda:0",
                 actions: Optional[torch.Tensor] = None, robot_obs: Optional[torch.Tensor] = None, pad_static: int = 10, pad_gripper: int = 4,
                 lang: Optional[torch.Tensor] = None, lang_segments: Optional[Sequence] = None, aux_lang_loss_window: int = 8,
                 lang_rows: Optional[Sequence[int]] = None, resident_frames: Optional[int] = None, stage_slots: int = 0, stage_slot_frames: int = 0):
        """rgb_static (F,H,W,3) / rgb_gripper (F,h,w,3): uint8, the frames of all episodes back to back; episode_ends: exclusive end index of every
        episode (ascending, last == F; default: one episode).  actions (F,7) / robot_obs (F,15): optional per-frame fp32 tables kept on the device too.
        lang (A,384): optional language table; lang_segments: (start_i, end_i) store indices, INCLUSIVE ends, of the annotated segments; lang_rows: the
        table row of each segment (default: segment i -> row i).
        resident_frames (None: the whole store lives on the device): a budget of device frames — the episodes up to the cut R = plan_tiers(...) stay
        resident, frames [R, F) go to pinned host memory, and the device tensors end in `stage_slots` staging slots of `stage_slot_frames` frames.
        `FrameStore.allocate` builds the same store with its tiers allocated but empty, to be filled with `write_frames`."""
        if rgb_static.dtype != torch.uint8 or rgb_gripper.dtype != torch.uint8 or rgb_static.dim() != 4 or rgb_gripper.dim() != 4:
            raise ValueError("FrameStore expects uint8 (F,H,W,3) tensors")
        if rgb_static.shape[0] != rgb_gripper.shape[0] or rgb_static.shape[-1] != 3 or rgb_gripper.shape[-1] != 3:
            raise ValueError("both cameras must hold the same F frames, channels last")
        self._build(int(rgb_static.shape[0]), tuple(rgb_static.shape[1:]), tuple(rgb_gripper.shape[1:]), (rgb_static, rgb_gripper), episode_ends, device, actions,
                    robot_obs, pad_static, pad_gripper, lang, lang_segments, aux_lang_loss_window, lang_rows, resident_frames, stage_slots, stage_slot_frames)

    @classmethod
    def allocate(cls, frames: int, static_shape: Sequence[int] = (200, 200, 3), gripper_shape: Sequence[int] = (84, 84, 3),
                 episode_ends: Optional[Sequence[int]] = None, device="cuda:0", actions: Optional[torch.Tensor] = None, robot_obs: Optional[torch.Tensor] = None,
                 pad_static: int = 10, pad_gripper: int = 4, lang: Optional[torch.Tensor] = None, lang_segments: Optional[Sequence] = None,
                 aux_lang_loss_window: int = 8, lang_rows: Optional[Sequence[int]] = None, resident_frames: Optional[int] = None, stage_slots: int = 0,
                 stage_slot_frames: int = 0) -> "FrameStore":
        """A store of `frames` frames whose tiers are allocated but not filled (`write_frames` fills them, episode by episode: no second copy of the
        split on the host, no pageable copy of the host tier).  Keyword arguments as the constructor's."""
        shape_s, shape_g = tuple(int(x) for x in static_shape), tuple(int(x) for x in gripper_shape)
        if len(shape_s) != 3 or len(shape_g) != 3 or shape_s[-1] != 3 or shape_g[-1] != 3 or int(frames) < 1:
            raise ValueError("FrameStore.allocate expects frames >= 1 and (H,W,3) frame shapes")
        st = cls.__new__(cls)
        st._build(int(frames), shape_s, shape_g, None, episode_ends, device, actions, robot_obs, pad_static, pad_gripper, lang, lang_segments, aux_lang_loss_window,
                  lang_rows, resident_frames, stage_slots, stage_slot_frames)
        return st

    def _build(self, frames: int, shape_s: tuple, shape_g: tuple, fill, episode_ends, device, actions, robot_obs, pad_static, pad_gripper, lang, lang_segments,
               aux_lang_loss_window, lang_rows, resident_frames, stage_slots, stage_slot_frames):
        """The one construction path: `frames` frames of the two frame shapes; fill = (rgb_static, rgb_gripper) to write into the tiers, or None."""
        self.device = torch.device(device)
        self.F = int(frames)
        ends = np.asarray([self.F] if episode_ends is None else list(episode_ends), np.int64)
        if ends.size == 0 or ends[-1] != self.F or np.any(np.diff(np.concatenate([[0], ends])) <= 0):
            raise ValueError("episode_ends must be ascending exclusive end indices whose last entry is F")
        self.episode_ends = ends
        self.episode_starts = np.concatenate([[0], ends[:-1]])
        self.tiered = resident_frames is not None
        self.host_static = self.host_gripper = None      # the host tier: frames [R, F) in pinned memory (tiered stores with R < F)
        if not self.tiered:
            if stage_slots or stage_slot_frames:
                raise ValueError("stage_slots / stage_slot_frames belong to a tiered store: pass resident_frames")
            self.R, self.ring = self.F, None
            if fill is not None:
                self.rgb_static = fill[0].to(self.device).contiguous()
                self.rgb_gripper = fill[1].to(self.device).contiguous()
            else:
                self.rgb_static = torch.empty((self.F,) + shape_s, dtype=torch.uint8, device=self.device)
                self.rgb_gripper = torch.empty((self.F,) + shape_g, dtype=torch.uint8, device=self.device)
        else:
            if int(resident_frames) < 0:
                raise ValueError("resident_frames must be >= 0")
            self.R = plan_tiers(ends, int(resident_frames))
            self.ring = SlotRing(self.R, stage_slots, stage_slot_frames)
            if self.R < self.F and self.ring.n_slots == 0:
                raise ValueError(f"{self.F - self.R} frames of the store lie on the host: a tiered store needs stage_slots and stage_slot_frames")
            n_dev = self.R + self.ring.n_slots * self.ring.slot_frames
            self.rgb_static = torch.zeros((n_dev,) + shape_s, dtype=torch.uint8, device=self.device)       # zeros: a slot that was never written is defined memory
            self.rgb_gripper = torch.zeros((n_dev,) + shape_g, dtype=torch.uint8, device=self.device)
            if self.R < self.F:      # allocated pinned and filled in place: never a pageable copy first
                pin = self.device.type == "cuda"
                self.host_static = torch.empty((self.F - self.R,) + shape_s, dtype=torch.uint8, pin_memory=pin)
                self.host_gripper = torch.empty((self.F - self.R,) + shape_g, dtype=torch.uint8, pin_memory=pin)
            if fill is not None:
                self.write_frames(0, *fill)
        self.actions = None if actions is None else actions.to(self.device, torch.float32).contiguous()
        self.robot_obs = None if robot_obs is None else robot_obs.to(self.device, torch.float32).contiguous()
        self.pad_static, self.pad_gripper = int(pad_static), int(pad_gripper)
        self.aux_lang_loss_window = int(aux_lang_loss_window)
        self.set_lang(lang, lang_segments, lang_rows)
        self.engine = None                         # StepEngine whose stream the table gathers run on (attach(); hulc_store_gather)
        self._valid: Dict[int, np.ndarray] = {}    # window size -> valid-start population, built once
        self._valid_lang: Dict[int, tuple] = {}

    def write_frames(self, first: int, rgb_static, rgb_gripper) -> None:
        """Fill store frames [first, first + n) of both cameras from (n,H,W,3) uint8 host tensors / arrays — each part goes straight to its tier."""
        s, g = (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, np.uint8)) for x in (rgb_static, rgb_gripper))
        n, first = int(s.shape[0]), int(first)
        if g.shape[0] != n or first < 0 or first + n > self.F or tuple(s.shape[1:]) != tuple(self.rgb_static.shape[1:]) or tuple(g.shape[1:]) != tuple(self.rgb_gripper.shape[1:]):
            raise ValueError(f"write_frames: frames [{first}, {first + n}) of shapes {tuple(s.shape)}, {tuple(g.shape)} do not fit the store")
        k = min(max(self.R - first, 0), n)             # the first k frames are resident
        if k:
            self.rgb_static[first:first + k].copy_(s[:k])
            self.rgb_gripper[first:first + k].copy_(g[:k])
        if k < n:
            self.host_static[first + k - self.R:first + n - self.R].copy_(s[k:])
            self.host_gripper[first + k - self.R:first + n - self.R].copy_(g[k:])

    def set_tables(self, actions=None, robot_obs=None) -> "FrameStore":
        """The per-frame tables of a store built with `allocate` (they stay whole on the device: 88 bytes per frame)."""
        self.actions = None if actions is None else torch.as_tensor(actions).to(self.device, torch.float32).contiguous()
        self.robot_obs = None if robot_obs is None else torch.as_tensor(robot_obs).to(self.device, torch.float32).contiguous()
        return self

    def set_lang(self, lang=None, lang_segments=None, lang_rows=None, aux_lang_loss_window: Optional[int] = None) -> "FrameStore":
        """The language table and annotated segments of a store built with `allocate` (arguments as the constructor's)."""
        self.lang = None if lang is None else torch.as_tensor(lang).to(self.device, torch.float32).reshape(-1, 384).contiguous()
        seg = np.zeros((0, 2), np.int64) if lang_segments is None else np.asarray(list(lang_segments), np.int64).reshape(-1, 2)
        if seg.size and (np.any(seg[:, 0] < 0) or np.any(seg[:, 1] >= self.F) or np.any(seg[:, 1] < seg[:, 0])):
            raise ValueError("lang_segments must be (start, end) store indices with 0 <= start <= end < F (inclusive ends)")
        self.lang_segments = seg
        self.lang_rows = np.arange(len(seg), dtype=np.int64) if lang_rows is None else np.asarray(list(lang_rows), np.int64)
        if len(self.lang_rows) != len(seg) or (len(seg) and self.lang is not None and (self.lang_rows.min() < 0 or self.lang_rows.max() >= self.lang.shape[0])):
            raise ValueError("lang_rows must name one row of the lang table per segment")
        if aux_lang_loss_window is not None:
            self.aux_lang_loss_window = int(aux_lang_loss_window)
        self._valid_lang = {}
        return self

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

    def sample_windows(self, B: int, min_window: int, max_window: int, generator: Optional[np.random.Generator] = None, return_host: bool = False):
        """B variable-length windows: a start with at least `min_window` frames left in its episode, and a length uniform in
        [min_window, min(max_window, frames left)] -> (starts (B,) int64, lens (B,) int32), both on the store's device.
        return_host: a third element (starts int64, lens int32) — the host arrays the draw produced, for `stage` and for logs (no read-back)."""
        if not 1 <= int(min_window) <= int(max_window):
            raise ValueError(f"need 1 <= min_window <= max_window (got {min_window}, {max_window})")
        pop = self.valid_starts(min_window)
        if pop.size == 0:
            raise ValueError(f"no episode of the store holds {min_window} frames")
        g = generator or np.random.default_rng()
        starts = pop[g.integers(0, pop.size, size=B)]
        hi = np.minimum(int(max_window), self.frames_left(starts))
        lens = g.integers(int(min_window), hi + 1).astype(np.int32)
        out = (torch.from_numpy(starts).to(self.device), torch.from_numpy(lens).to(self.device))
        return out + ((starts, lens),) if return_host else out

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

    def sample_lang_windows(self, B: int, min_window: int, max_window: int, generator: Optional[np.random.Generator] = None, return_host: bool = False):
        """B language windows, each inside ONE annotated segment (start_i, end_i): length uniform in [min_window, min(max_window, end_i - s + 1)].
        -> (starts int64, lens int32, lang table rows int32, use_for_aux_lang_loss bool), on the store's device.
        return_host: a fifth element (starts int64, lens int32), the host arrays of the draw."""
        if not 1 <= int(min_window) <= int(max_window):
            raise ValueError(f"need 1 <= min_window <= max_window (got {min_window}, {max_window})")
        st, sg, ax = self.valid_lang_starts(min_window)
        if st.size == 0:
            raise ValueError(f"no annotated segment of the store holds {min_window} frames")
        g = generator or np.random.default_rng()
        pick = g.integers(0, st.size, size=B)
        starts, seg = st[pick], sg[pick]
        hi = np.minimum(int(max_window), self.lang_segments[seg, 1] - starts + 1)
        lens = g.integers(int(min_window), hi + 1).astype(np.int32)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        out = (dev(starts), dev(lens), dev(self.lang_rows[seg].astype(np.int32)), dev(ax[pick]))
        return out + ((starts, lens),) if return_host else out

    def sample_starts(self, B: int, S: int, generator: Optional[np.random.Generator] = None) -> torch.Tensor:
        """B window starts drawn uniformly from valid_starts(S) -> (B,) int64 on the device."""
        pop = self.valid_starts(S)
        if pop.size == 0:
            raise ValueError(f"no episode of the store holds {S} frames")
        g = generator or np.random.default_rng()
        return torch.from_numpy(pop[g.integers(0, pop.size, size=B)]).to(self.device)

    def stage(self, starts, S: int, lens=None, engine=None) -> StagedWindows:
        """Tiered stores: reserve staging slots for the host-tier windows of one batch and start their copies — ONE hulc_store_stage call on the
        engine's copy stream, which first waits for what the engine's stream holds so far (the slots' previous readers), so call it one step ahead:
        stage batch n + 1, then run batch n.  Only the L real frames of a window are copied (window_len handles the padding); resident windows cost
        nothing.  starts / lens must be known on the host: numpy arrays and CPU tensors are taken as they are, a device tensor costs one .cpu()
        (a synchronisation — `sample_windows(return_host=True)` avoids it).  The starts are clamped as `batch` clamps them.
        Raises ValueError (before any copy) if the call needs more slots than the ring has, RuntimeError if it would recycle slots of a batch whose
        backward / validate has not been enqueued (StagedWindows.mark_enqueued / release)."""
        if not self.tiered:
            raise ValueError("stage() belongs to a tiered store (resident_frames=...)")
        host = lambda x, dt: np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x).astype(dt).reshape(-1)
        st = host(starts, np.int64)
        if lens is not None:
            ln = np.clip(host(lens, np.int64), 1, min(int(S), self.F))
            if ln.shape != st.shape:
                raise ValueError("stage: lens must be (B,) like starts")
        else:
            if self.F < S:
                raise ValueError(f"the store holds {self.F} frames, fewer than one window of {S}")
            ln = np.full(st.shape, int(S), np.int64)
        st = np.minimum(np.maximum(st, 0), self.F - ln)
        if np.any((st < self.R) & (st + ln > self.R)):
            raise ValueError("stage: a window crosses the resident cut — windows must lie inside one episode")
        engine = engine if engine is not None else self.engine
        if engine is None and np.any(st >= self.R):
            raise ValueError("host-tier windows are staged by hulc_store_stage: pass engine= or attach() one")
        h = self.ring.plan(st, ln)
        h.lens = None if lens is None else ln.astype(np.int32)
        if h.copies:
            try:
                copies = []
                for dev, hostt in ((self.rgb_static, self.host_static), (self.rgb_gripper, self.host_gripper)):
                    fb = dev[0].numel()
                    for src, j, L in h.copies:      # bounds: R <= src, src + L <= F (clamped above); L <= slot_frames (SlotRing.plan)
                        copies.append((hostt.data_ptr() + (src - self.R) * fb, dev.data_ptr() + self.ring.slot_base(j) * fb, L * fb))
                h.ticket = engine.store_stage(copies)
            except Exception:
                h.release()
                raise
        return h

    def batch(self, starts: Optional[torch.Tensor], S: int, actions: Optional[torch.Tensor] = None, robot_obs: Optional[torch.Tensor] = None, shifts: bool = False,
              generator: Optional[torch.Generator] = None, lang: Optional[torch.Tensor] = None, use_for_aux: Optional[torch.Tensor] = None,
              lens: Optional[torch.Tensor] = None, lang_rows: Optional[torch.Tensor] = None, absolute: bool = False, engine=None,
              staged: Optional[StagedWindows] = None, ragged: bool = False) -> Dict:
        """The reference-shaped batch dict of one modality (hulc/models/hulc.py:395-414) for `Hulc.training_step` / `validation_step`: the stores stand in
        for rgb_obs, `window_start` names the windows.  actions / robot_obs: (B,S,7) / (B,S,15) tensors, or None to gather them from the store's own
        per-frame tables.  shifts=True draws the per-frame RandomShiftsAug offsets (transforms.py:8-29) on the device.
        lens (B,) int32: variable-length windows padded to S (`window_len`).  lang_rows (B,) int32: rows of the store's lang table (instead of `lang`).
        absolute: the actions table holds absolute targets, padding repeats all seven dims.
        ragged=True (needs lens): the clamped lens also go into the dict on the HOST, as `window_len_host` (B,) int32 numpy — the engine then runs the
        perceptual encoders on the real frames of the windows only (hulc_batch::window_len_host; `ragged_plan` restates its arithmetic).  lens given as
        a numpy array or CPU tensor are taken as they are; a device tensor costs one .cpu() (a synchronisation — `sample_windows(return_host=True)`
        hands out the host arrays of its draw).  Works with `staged=`: staging rewrites only the starts.
        With an engine (argument, or attach()) the tables are gathered by hulc_store_gather — required for `lens`, whose padding rules live there;
        without one, fixed windows are gathered by torch indexing.  The starts are clamped ONCE here, so frames and tables always name the same rows.
        Tiered stores: `staged` = the handle `stage` returned for these windows (starts / lens are then taken from it); without one the windows are
        staged now — correct, but the copies are not overlapped with a step.  The engine's stream joins the handle's ticket, `window_start` holds the
        starts rewritten to the staging slots, the tables are gathered with the original starts, and the dict carries the handle as `staged`."""
        engine = engine if engine is not None else self.engine
        table_starts = None
        lens_host = None
        if ragged and not self.tiered:
            if lens is None:
                raise ValueError("ragged=True needs lens (the windows' real frame counts)")
            lens_host = np.asarray(lens.detach().cpu().numpy() if torch.is_tensor(lens) else lens).astype(np.int64).reshape(-1)
            lens_host = np.clip(lens_host, 1, min(int(S), self.F)).astype(np.int32)
        if lens is not None and not torch.is_tensor(lens):
            lens = torch.from_numpy(np.ascontiguousarray(lens, np.int32))
        if self.tiered:
            if staged is None:
                staged = self.stage(starts, S, lens, engine=engine)
            if staged.ticket and not staged.joined:
                engine.store_stage_join(staged.ticket)
                staged.joined = True
            starts = torch.from_numpy(staged.frame_starts).to(self.device)
            table_starts = torch.from_numpy(staged.table_starts).to(self.device)
            lens = None if staged.lens is None else torch.from_numpy(staged.lens).to(self.device)
            if ragged:
                if staged.lens is None:
                    raise ValueError("ragged=True needs lens (the windows' real frame counts)")
                lens_host = staged.lens.astype(np.int32)      # clamped by stage()
        elif staged is not None:
            raise ValueError("staged= belongs to a tiered store (resident_frames=...)")
        starts = starts.to(self.device, torch.int64)
        B = int(starts.shape[0])
        if not self.tiered:                        # (a tiered store's starts / lens were clamped on the host by stage())
            if lens is not None:
                lens = lens.to(self.device, torch.int32).clamp(1, min(int(S), self.F))
                starts = torch.minimum(starts.clamp(min=0), self.F - lens.to(torch.int64))
            else:
                if self.F < S:
                    raise ValueError(f"the store holds {self.F} frames, fewer than one window of {S}")
                starts = starts.clamp(0, self.F - S)
        if table_starts is None:
            table_starts = starts
        if lang is None and lang_rows is not None:
            if self.lang is None:
                raise ValueError("lang_rows needs a store built with its lang table")
            lang_rows = lang_rows.to(self.device, torch.int32)
        if actions is None or robot_obs is None or (lang is None and lang_rows is not None):
            if (actions is None or robot_obs is None) and (self.actions is None or self.robot_obs is None):
                raise ValueError("pass actions / robot_obs or build the store with its per-frame tables")
            if engine is not None and self.actions is not None and self.robot_obs is not None:
                a, r, l = engine.store_gather(self.actions, self.robot_obs, table_starts, S, window_len=lens, lang=self.lang if lang is None and lang_rows is not None else None,
                                              lang_row=lang_rows if lang is None else None, absolute=absolute)
                lang = l if lang is None else lang
            elif lens is not None:
                raise ValueError("variable-length windows gather the store's tables through hulc_store_gather: pass engine= or attach() one")
            else:
                idx = table_starts[:, None] + torch.arange(S, device=self.device)[None, :]
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
        if lens_host is not None:
            d["window_len_host"] = lens_host
        if staged is not None:
            d["staged"] = staged
        if shifts:
            d["shift_static"] = torch.randint(0, 2 * self.pad_static + 1, (B * S, 2), device=self.device, generator=generator, dtype=torch.int32)
            d["shift_gripper"] = torch.randint(0, 2 * self.pad_gripper + 1, (B * S, 2), device=self.device, generator=generator, dtype=torch.int32)
        if lang is not None:
            d["lang"] = lang.to(self.device, torch.float32)
            d["use_for_aux_lang_loss"] = (torch.ones(B, dtype=torch.bool, device=self.device) if use_for_aux is None else use_for_aux.to(self.device))
        return d

    def materialise(self, starts: torch.Tensor, S: int, lens: Optional[torch.Tensor] = None):
        """The same windows as (B,S,H,W,3) uint8 tensors (tests; the path the store exists to avoid).  lens: padded by repeating the last real frame."""
        if self.tiered:
            raise ValueError("materialise reads store frames by index: a tiered store keeps only part of them on the device")
        t = torch.arange(S, device=self.device)[None, :]
        if lens is not None:
            t = torch.minimum(t, lens.to(self.device, torch.int64)[:, None] - 1)
        idx = (starts.to(self.device, torch.int64)[:, None] + t).reshape(-1)
        B = int(starts.shape[0])
        return (self.rgb_static[idx].reshape(B, S, *self.rgb_static.shape[1:]).contiguous(), self.rgb_gripper[idx].reshape(B, S, *self.rgb_gripper.shape[1:]).contiguous())
