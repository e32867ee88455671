"""StepEngine — thin Python owner of one libhulc_hip context + the flat fp32 parameter/gradient/Adam buffers.

torch is plumbing here (device memory, streams, torch.distributed); every FLOP of the step runs in the HIP library.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import lib as L
from . import spec


class StepEngine:
    def __init__(self, dims: spec.ModelDims, max_batch: int, max_seq: int, dtype: str = "bf16", device: str = "cuda:0",
                 kl_beta: float = 0.01, kl_balancing_mix: float = 0.8, dropout_p: float = 0.1, num_classes: int = 10,
                 gripper_alpha: float = 1.0, log_scale_min: float = -7.0, seed: int = 42, layout_pad: int = 64):
        self.lib = L.load()
        if not torch.cuda.is_available():
            raise RuntimeError("hulc_amd.StepEngine needs a HIP device (torch.cuda.is_available() is False); no CPU fallback")
        self.dims = dims
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.dtype = dtype
        self.layout, self.numel = spec.layout(dims, layout_pad)      # layout_pad 4: the tightly packed table a C caller may bind (tests)
        dev = self.device
        self.flat_params = torch.zeros(self.numel, dtype=torch.float32, device=dev)
        self.flat_grads = torch.zeros(self.numel, dtype=torch.float32, device=dev)
        self.adam_m = torch.zeros(self.numel, dtype=torch.float32, device=dev)
        self.adam_v = torch.zeros(self.numel, dtype=torch.float32, device=dev)
        cfg = L.HulcConfig(kind=L.KIND["mcil_gru" if (dims.kind == "mcil" and dims.rnn_type == "gru") else dims.kind], dtype=L.DTYPE[dtype], max_batch=max_batch, max_seq=max_seq,
                           max_window=dims.max_window, use_clip=int(dims.use_clip), kl_beta=kl_beta,
                           kl_balancing_mix=kl_balancing_mix, dropout_p=dropout_p, num_classes=num_classes,
                           gripper_alpha=gripper_alpha, log_scale_min=log_scale_min, seed=seed)
        self.cfg = cfg
        self.ctx = C.c_void_p()
        L.check(self.lib.hulc_ctx_create(C.byref(cfg), C.byref(self.ctx)))
        L.check(self.lib.hulc_set_stream(self.ctx, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        self.aux_heads = bool(dims.use_bc_z or dims.use_mia)
        if self.aux_heads:      # before the bind: the heads' tensors are then required by name (include/hulc_hip.h: hulc_aux_heads_enable)
            L.check(self.lib.hulc_aux_heads_enable(self.ctx, int(dims.use_bc_z), int(dims.use_mia)))
        if dims.decoder == "deterministic":      # before the bind as well: action_decoder.actions.0.* replaces the mixture heads (hulc_decoder_select)
            L.check(self.lib.hulc_decoder_select(self.ctx, L.DECODER["deterministic"], L.CRITERION[dims.criterion]))
        if dims.decoder_body == "mlp":      # before the bind: action_decoder.rnn.{0,2,4}.* replace the recurrence's eight tensors (hulc_decoder_body_select)
            L.check(self.lib.hulc_decoder_body_select(self.ctx, L.BODY["mlp"]))
        names = list(self.layout.keys())
        self._names = (C.c_char_p * len(names))(*[n.encode() for n in names])
        self._offs = (C.c_int64 * len(names))(*[self.layout[n][0] for n in names])
        self._nums = (C.c_int64 * len(names))(*[int(np.prod(self.layout[n][1])) if len(self.layout[n][1]) else 1 for n in names])
        self._bound = False
        self._keep = []
        self._staged_pending = []      # StagedWindows handles of forwards whose backward has not been enqueued yet (_staged_read)
        self.adam_t = 0

    # ---- parameters -------------------------------------------------------------------------------------------
    def views(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        out = {}
        for n, (off, shape) in self.layout.items():
            k = int(np.prod(shape)) if len(shape) else 1
            out[n] = flat[off:off + k].view(*shape) if len(shape) else flat[off:off + 1].view(())
        return out

    def bind(self):
        L.check(self.lib.hulc_bind_params(self.ctx, self.flat_params.data_ptr(), self.flat_grads.data_ptr(), self.adam_m.data_ptr(),
                                          self.adam_v.data_ptr(), self.numel, len(self.layout), self._names, self._offs, self._nums))
        self._bound = True
        self.flat_ema = None      # a new bind switches the averaged weights off (hulc_ema_enable)

    def load_numpy(self, params: Dict[str, np.ndarray]):
        v = self.views(self.flat_params)
        for n, t in v.items():
            t.copy_(torch.from_numpy(np.asarray(params[n], np.float32)).reshape(t.shape))
        if self._bound:
            self.prepare_weights()
        else:
            self.bind()

    def prepare_weights(self):
        L.check(self.lib.hulc_prepare_weights(self.ctx))

    def zero_grads(self):
        """hulc_zero_grads.  16-bit engines (option lazy_zero_grads, default 1): the large store-first Linear weight gradients keep the previous
        step's values until the next backward writes them / the library reads them (include/hulc_hip.h); call `flush_grads()` before reading
        `flat_grads` yourself between zero_grads() and the end of the next backward."""
        L.check(self.lib.hulc_zero_grads(self.ctx))

    def flush_grads(self):
        """hulc_flush_grads: zero whatever zero_grads() left marked stale (no-op otherwise)."""
        L.check(self.lib.hulc_flush_grads(self.ctx))

    # ---- step pieces ------------------------------------------------------------------------------------------
    @staticmethod
    def _ingest_fields(mb: Dict, ptr) -> Dict:
        """uint8 (B,S,H,W,C) frames select the fused ingest path (include/hulc_hip.h: frames_u8); optional per-frame RandomShiftsAug
        shifts `shift_static` / `shift_gripper` (B*S,2) int32 in [0, 2*pad] with pads `pad_static` (10) / `pad_gripper` (4).
        `window_start` (B,) int64 selects the FRAME STORE form (hulc_batch::window_start): rgb_static / rgb_gripper are then the device-resident
        stores (F,H,W,3) uint8 and window b = store frames [window_start[b], window_start[b] + S) — nothing is materialised per step.
        `window_len` (B,) int32 on the device next to it: window b holds that many real frames and is padded to S by repeating its last one
        (hulc_batch::window_len).
        `window_len_host` (B,) int32 numpy array or CPU tensor, valid only with window_start: the same lengths on the HOST select the ragged encoder
        pass (hulc_batch::window_len_host) — the perceptual encoders run on the real frames only; `window_len` is then ignored by the library.  It
        stays on the host: a device tensor is a ValueError."""
        wlh = StepEngine._host_lens(mb)
        rel = {}
        if mb.get("actions_absolute"):        # RelativeActions (transforms.py:32-56) applied on the device
            rel = dict(actions_absolute=1, max_rel_pos=float(mb.get("max_rel_pos", 0.02)), max_rel_orn=float(mb.get("max_rel_orn", 0.05)))
        if mb["rgb_static"].dtype != torch.uint8:
            if mb.get("window_len") is not None or wlh is not None:
                raise ValueError("window_len / window_len_host need the frame store form: uint8 stores and window_start")
            return rel
        if mb["rgb_gripper"].dtype != torch.uint8 or mb["rgb_static"].shape[-1] != 3 or mb["rgb_gripper"].shape[-1] != 3:
            raise ValueError("uint8 ingest expects both cameras as uint8 (B,S,H,W,3) tensors")
        f = dict(rel, frames_u8=1, pad_static=int(mb.get("pad_static", 10)), pad_gripper=int(mb.get("pad_gripper", 4)))
        for k in ("shift_static", "shift_gripper"):
            if mb.get(k) is not None:
                f[k] = ptr(mb[k].to(torch.int32))
        if mb.get("window_start") is not None:
            if mb["rgb_static"].dim() != 4 or mb["rgb_gripper"].dim() != 4 or mb["rgb_static"].shape[0] != mb["rgb_gripper"].shape[0]:
                raise ValueError("frame store: rgb_static / rgb_gripper must be (F,H,W,3) uint8 stores of the same F next to window_start (B,)")
            ws = mb["window_start"]
            if not ws.is_cuda:
                raise ValueError("frame store: window_start must live on the device")
            f["window_start"] = ptr(ws.to(torch.int64))
            f["store_frames"] = int(mb["rgb_static"].shape[0])
        if mb.get("window_len") is not None:      # without window_start the library reports the error (hulc_last_error)
            wl = mb["window_len"]
            if not torch.is_tensor(wl) or not wl.is_cuda or wl.dtype != torch.int32 or wl.dim() != 1 or wl.shape[0] != mb["actions"].shape[0]:
                raise ValueError("frame store: window_len must be a (B,) int32 tensor on the device")
            f["window_len"] = ptr(wl)
        if wlh is not None:      # without window_start the library reports the error (hulc_last_error)
            f["window_len_host"] = ptr(wlh)
        return f

    @staticmethod
    def _host_lens(mb: Dict) -> Optional[torch.Tensor]:
        """The batch's `window_len_host` as a contiguous (B,) int32 CPU tensor, or None; raises for a device tensor or a wrong shape."""
        wl = mb.get("window_len_host")
        if wl is None:
            return None
        if torch.is_tensor(wl):
            if wl.device.type != "cpu":
                raise ValueError(f"window_len_host must stay on the host (numpy array or CPU tensor), got a tensor on {wl.device}")
            wl = wl.to(torch.int32)
        else:
            wl = torch.from_numpy(np.ascontiguousarray(wl, np.int32))
        if wl.dim() != 1 or wl.shape[0] != mb["actions"].shape[0]:
            raise ValueError("window_len_host must be a (B,) int32 array")
        return wl.contiguous()

    def _batch_struct(self, mb: Dict, is_lang: bool, step: int, keep: list):
        B, S = mb["actions"].shape[:2]

        def ptr(t):
            t = t.contiguous()
            keep.append(t)
            return t.data_ptr()

        b = L.HulcBatch(B=B, S=S, is_lang=int(is_lang), rgb_static=ptr(mb["rgb_static"]), rgb_gripper=ptr(mb["rgb_gripper"]),
                        actions=ptr(mb["actions"]), robot_obs=ptr(mb["robot_obs"]), lang=ptr(mb["lang"]) if is_lang else None,
                        plan_idx=ptr(mb["plan_idx"]) if mb.get("plan_idx") is not None else None, aux_rows=None, n_aux=0, step=step,
                        **self._ingest_fields(mb, ptr))
        self._staged_read(mb)
        if mb.get("plan_eps") is not None:          # mcil: injected N(0,1) draw of the reparametrised plan sample
            b.plan_eps = ptr(mb["plan_eps"].to(torch.float32))
        if is_lang and mb.get("aux_rows") is not None and len(mb["aux_rows"]) > 0:
            rows = np.ascontiguousarray(mb["aux_rows"], np.int32)
            keep.append(rows)
            b.aux_rows = rows.ctypes.data
            b.n_aux = len(rows)
        return b

    def forward_loss_pair(self, mb_vis: Dict, mb_lang: Dict, loss_weight: float, clip_weight: float, step: int = 0, sync_losses: bool = True):
        """Both modalities of a step as ONE pass over 2B windows (hulc_forward_loss_pair; needs equal B and S).  Returns the two loss
        dicts (vis, lang), or the (8,) device tensor [vis x4, lang x4] with sync_losses=False.  One backward() follows for the pair."""
        keep = []
        bv = self._batch_struct(mb_vis, False, step, keep)
        bl = self._batch_struct(mb_lang, True, step, keep)
        self._keep = keep
        if sync_losses:
            out = (C.c_float * 8)()
            L.check(self.lib.hulc_forward_loss_pair(self.ctx, C.byref(bv), C.byref(bl), loss_weight, clip_weight, out, 1))
            return (dict(total_mod=out[0], kl=out[1], action=out[2], clip=out[3]), self._with_aux(dict(total_mod=out[4], kl=out[5], action=out[6], clip=out[7]), True))
        if not hasattr(self, "_loss_dev8"):
            self._loss_dev8 = torch.zeros(8, dtype=torch.float32, device=self.device)
        L.check(self.lib.hulc_forward_loss_pair(self.ctx, C.byref(bv), C.byref(bl), loss_weight, clip_weight, self._loss_dev8.data_ptr(), 0))
        self._loss_dev = self._loss_dev8[4:]
        return self._loss_dev8

    def forward_loss(self, mb: Dict, is_lang: bool, loss_weight: float, clip_weight: float, step: int = 0,
                     sync_losses: bool = True):
        """mb: device tensors rgb_static (B,S,3,200,200) f32, rgb_gripper, actions, robot_obs(15), [lang], [plan_idx int32],
        [aux_rows: host int32 numpy]."""
        keep = []
        b = self._batch_struct(mb, is_lang, step, keep)
        self._keep = keep
        if sync_losses:
            out = (C.c_float * 4)()
            L.check(self.lib.hulc_forward_loss(self.ctx, C.byref(b), loss_weight, clip_weight, out, 1))
            return self._with_aux(dict(total_mod=out[0], kl=out[1], action=out[2], clip=out[3]), is_lang)
        if not hasattr(self, "_loss_dev"):
            self._loss_dev = torch.zeros(4, dtype=torch.float32, device=self.device)
        L.check(self.lib.hulc_forward_loss(self.ctx, C.byref(b), loss_weight, clip_weight, self._loss_dev.data_ptr(), 0))
        return self._loss_dev

    # ---- BC-Z / MIA language auxiliary heads (include/hulc_hip.h: hulc_aux_*; dims.use_bc_z / dims.use_mia) -------------------------------
    def set_aux_weights(self, bc_z_weight: float = 1.0, mia_weight: float = 1.0) -> None:
        """hulc_aux_weights_set: the factors multiplied into the two losses' gradients by every following forward (default 1 each)."""
        L.check(self.lib.hulc_aux_weights_set(self.ctx, float(bc_z_weight), float(mia_weight)))

    def aux_losses(self) -> Dict:
        """hulc_aux_losses_get: {"bc_z", "mia", "aux_rows"} of the last forward_loss / forward_loss_pair / validate, unweighted; a head that did
        not run (not enabled, no flagged row, no forward yet) reads 0.  Synchronises the stream."""
        out = (C.c_float * 4)()
        L.check(self.lib.hulc_aux_losses_get(self.ctx, out))
        return dict(bc_z=out[0], mia=out[1], aux_rows=int(out[2]))

    def _with_aux(self, losses: Dict, is_lang: bool) -> Dict:
        if self.aux_heads and is_lang:
            losses.update(self.aux_losses())
        return losses

    def store_gather(self, actions: torch.Tensor, robot_obs: torch.Tensor, window_start: torch.Tensor, S: int, window_len: Optional[torch.Tensor] = None,
                     lang: Optional[torch.Tensor] = None, lang_row: Optional[torch.Tensor] = None, absolute: bool = False):
        """hulc_store_gather: the non-image half of a frame-store batch from the per-frame tables actions (F,7) / robot_obs (F,15) and, optionally, the
        language table lang (A,384) with one row index per window — all fp32 / int on the device.  Same window arithmetic and padding as the frames
        (window_len); padded relative actions are zero in dims 0..5 and repeat the gripper, `absolute` repeats all seven.  One asynchronous launch on
        the context's stream.  Returns (actions (B,S,7), robot_obs (B,S,15), lang (B,384) or None)."""
        def dev(t, dtype, shape_tail, name):
            if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype or tuple(t.shape[1:]) != shape_tail or not t.is_contiguous():
                raise ValueError(f"store_gather: {name} must be a contiguous {dtype} device tensor of shape (n,{','.join(map(str, shape_tail))})")
            return t
        actions, robot_obs = dev(actions, torch.float32, (7,), "actions"), dev(robot_obs, torch.float32, (15,), "robot_obs")
        if actions.shape[0] != robot_obs.shape[0] or actions.shape[0] < 1:
            raise ValueError("store_gather: actions and robot_obs must hold the same F >= 1 rows")
        ws = dev(window_start, torch.int64, (), "window_start")
        B = int(ws.shape[0])
        wl = None if window_len is None else dev(window_len, torch.int32, (), "window_len")
        if wl is not None and wl.shape[0] != B:
            raise ValueError("store_gather: window_len must be (B,)")
        lang_out = None
        if lang is not None:
            lang = dev(lang, torch.float32, (384,), "lang")
            if lang_row is None:
                raise ValueError("store_gather: a lang table needs lang_row (B,)")
            lang_row = dev(lang_row, torch.int32, (), "lang_row")
            if lang_row.shape[0] != B:
                raise ValueError("store_gather: lang_row must be (B,)")
            lang_out = torch.empty(B, 384, dtype=torch.float32, device=self.device)
        a_out = torch.empty(B, int(S), 7, dtype=torch.float32, device=self.device)
        r_out = torch.empty(B, int(S), 15, dtype=torch.float32, device=self.device)
        t = L.HulcStoreTables(actions=actions.data_ptr(), robot_obs=robot_obs.data_ptr(), lang=None if lang is None else lang.data_ptr(),
                              store_frames=int(actions.shape[0]), lang_rows=0 if lang is None else int(lang.shape[0]), absolute=int(bool(absolute)))
        L.check(self.lib.hulc_store_gather(self.ctx, C.byref(t), ws.data_ptr(), None if wl is None else wl.data_ptr(), None if lang is None else lang_row.data_ptr(),
                                           B, int(S), a_out.data_ptr(), r_out.data_ptr(), None if lang_out is None else lang_out.data_ptr()))
        return a_out, r_out, lang_out

    # ---- host tier of a two-tier frame store (include/hulc_hip.h: hulc_store_stage; hulc_amd/utils/frame_store.py) ---------------------------
    def store_stage(self, copies) -> int:
        """hulc_store_stage: `copies` = [(src pointer, dst pointer, bytes)] — src pinned host or device memory, dst device memory — as ONE call on the
        context's copy stream, which first waits for everything enqueued on the engine's stream so far.  Returns the ticket (> 0) for store_stage_join.
        The caller keeps the buffers alive until the ticket has been joined and its readers have run."""
        n = len(copies)
        arr = (L.HulcStageCopy * max(n, 1))(*[L.HulcStageCopy(src=int(s), dst=int(d), bytes=int(b)) for s, d, b in copies])
        ticket = int(self.lib.hulc_store_stage(self.ctx, arr, n))
        if ticket <= 0:
            L.check(1)
        return ticket

    def store_stage_join(self, ticket: int) -> None:
        """hulc_store_stage_join: the engine's stream waits for that ticket's copies (no host synchronisation)."""
        L.check(self.lib.hulc_store_stage_join(self.ctx, int(ticket)))

    def store_stage_stats(self) -> Dict:
        """{"calls", "copies", "bytes"} staged by this context so far."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        L.check(self.lib.hulc_store_stage_stats(self.ctx, C.byref(a), C.byref(b), C.byref(c)))
        return dict(calls=a.value, copies=b.value, bytes=c.value)

    def _staged_read(self, mb: Dict) -> None:
        """A batch that reads staging slots (FrameStore.batch: `staged`): its handle is marked once the LAST reader of the slots has been enqueued —
        the backward that follows this forward (conv1's weight gradient re-reads the frames), or the validate itself."""
        h = mb.get("staged")
        if h is None or h.done:      # all-resident batches hold no slot: nothing to wait for
            return
        # forward-only use (no backward ever marks): handles given up with release() drop out here, the others are bounded by the ring, whose guard
        # raises once their slots would be needed again
        self._staged_pending = [p for p in self._staged_pending if not p.done and p is not h]
        self._staged_pending.append(h)

    def _staged_done(self) -> None:
        for h in self._staged_pending:
            h.mark_enqueued()
        self._staged_pending = []

    # ------------------------------------------------------------------ validation / rollout (forward only)
    @staticmethod
    def _dev_or_host_ptr(x, keep, dtype):
        """Noise arrays may be torch (device/host) tensors or numpy arrays; returns a raw pointer and keeps the buffer alive."""
        if x is None:
            return None
        if torch.is_tensor(x):
            t = x.to(dtype=torch.int32 if dtype == np.int32 else torch.float32).contiguous()
            keep.append(t)
            return t.data_ptr()
        a = np.ascontiguousarray(x, dtype)
        keep.append(a)
        return a.ctypes.data

    def validate(self, mb: Dict, is_lang: bool, noise: Optional[Dict] = None, want_pred: bool = False) -> Dict:
        """One modality of Hulc.validation_step (hulc.py:770-797 -> lmp_val :301-388), eval mode.  noise (optional, parity):
        plan_idx_pp / plan_idx_pr (B,32) int, u_mix_pp / u_mix_pr (B,S,6,10), u_act_pp / u_act_pr (B,S,6) uniform [0,1) draws."""
        B, S = mb["actions"].shape[:2]
        keep = []

        def ptr(t):
            t = t.contiguous()
            keep.append(t)
            return t.data_ptr()

        b = L.HulcBatch(B=B, S=S, is_lang=int(is_lang), rgb_static=ptr(mb["rgb_static"]), rgb_gripper=ptr(mb["rgb_gripper"]),
                        actions=ptr(mb["actions"]), robot_obs=ptr(mb["robot_obs"]), lang=ptr(mb["lang"]) if is_lang else None,
                        plan_idx=None, aux_rows=None, n_aux=0, step=int(mb.get("step", 0)), **self._ingest_fields(mb, ptr))
        noise = dict(noise or {})
        mcil = self.dims.kind == "mcil"
        if mcil:       # continuous plans travel as (B,256) fp32 in the plan slots (include/hulc_hip.h: hulc_val_noise)
            noise["plan_idx_pp"], noise["plan_idx_pr"] = noise.get("plan_pp"), noise.get("plan_pr")
        nz = L.HulcValNoise(**{k: self._dev_or_host_ptr(noise.get(k), keep, np.int32 if (k.startswith("plan") and not mcil) else np.float32)
                               for k in ("plan_idx_pp", "plan_idx_pr", "u_mix_pp", "u_act_pp", "u_mix_pr", "u_act_pr")})
        if is_lang and mb.get("aux_rows") is not None and len(mb["aux_rows"]) > 0:      # rows of the CLIP validation loss (hulc.py:804-808)
            rows = np.ascontiguousarray(mb["aux_rows"], np.int32)
            keep.append(rows)
            b.aux_rows = rows.ctypes.data
            b.n_aux = len(rows)
        out = (C.c_float * 18)()
        ppp = torch.zeros(B, 256 if mcil else 32, dtype=torch.float32 if mcil else torch.int32, device=self.device)
        ppr = torch.zeros(B, 256 if mcil else 32, dtype=torch.float32 if mcil else torch.int32, device=self.device)
        pred_pp = torch.zeros(B, S, 7, device=self.device) if want_pred else None
        pred_pr = torch.zeros(B, S, 7, device=self.device) if want_pred else None
        L.check(self.lib.hulc_validate(self.ctx, C.byref(b), C.byref(nz), out, ppp.data_ptr(), ppr.data_ptr(),
                                       pred_pp.data_ptr() if want_pred else None, pred_pr.data_ptr() if want_pred else None))
        if mb.get("staged") is not None:
            mb["staged"].mark_enqueued()
        o = list(out)
        res = dict(action_loss_pp=o[0], action_loss_pr=o[1], kl_loss=o[2], gripper_sr_pp=o[3], gripper_sr_pr=o[4],
                   mae_pp=np.array(o[5:11], np.float32), mae_pr=np.array(o[11:17], np.float32), sampled_plan_idx_pp=ppp, sampled_plan_idx_pr=ppr, val_pred_clip_loss=o[17])
        if self.aux_heads and is_lang:      # val/lang_pred_loss, val/lang_contrastive_loss (hulc.py:798-813)
            a = self.aux_losses()
            res.update(lang_pred_loss=a["bc_z"], lang_contrastive_loss=a["mia"], aux_rows=a["aux_rows"])
        if mcil:
            res.update(sampled_plan_pp=ppp, sampled_plan_pr=ppr)
        if want_pred:
            res.update(pred_pp=pred_pp, pred_pr=pred_pr)
        return res

    def clip_gt_encode(self, lang_emb, slot: int) -> None:
        """encoded_lang_{train,val} of Hulc.on_validation_epoch_start (hulc.py:967-974) kept on the device: slot 0 = training instructions,
        1 = validation instructions.  lang_emb: (m,384) fp32, numpy or tensor."""
        keep = []
        if isinstance(lang_emb, torch.Tensor):
            lang_emb = lang_emb.to(dtype=torch.float32).contiguous()
        p = self._dev_or_host_ptr(lang_emb, keep, np.float32)
        m = int(lang_emb.shape[0])
        if lang_emb.ndim != 2 or lang_emb.shape[1] != 384:
            raise ValueError(f"lang_emb must be (m,384), got {tuple(lang_emb.shape)}")
        L.check(self.lib.hulc_clip_gt_encode(self.ctx, p, m, int(slot)))

    def clip_gt_scores(self, slot: int) -> np.ndarray:
        """logits_per_image (n,m) of Hulc._clip_groundtruth_loss (hulc.py:1024-1029) for the masked rows of the last lang `validate`."""
        n, m = C.c_int32(0), C.c_int32(0)
        L.check(self.lib.hulc_clip_gt_scores(self.ctx, int(slot), None, 0, C.byref(n), C.byref(m)))       # shape query
        out = np.empty((n.value, m.value), np.float32)
        L.check(self.lib.hulc_clip_gt_scores(self.ctx, int(slot), out.ctypes.data, out.size, C.byref(n), C.byref(m)))
        return out

    def rollout_reset(self):
        L.check(self.lib.hulc_rollout_reset(self.ctx))

    def _obs(self, obs, keep):
        def ptr(t):
            t = t.to(device=self.device, dtype=torch.float32).contiguous()
            keep.append(t)
            return t.data_ptr()
        return L.HulcRolloutObs(rgb_static=ptr(obs["rgb_static"]), rgb_gripper=ptr(obs["rgb_gripper"]),
                                robot_obs_raw=ptr(obs["robot_obs_raw"]) if obs.get("robot_obs_raw") is not None else None)

    def rollout_plan(self, obs: Dict, goal, plan_idx=None):
        """goal: dict(rgb_static, rgb_gripper) (1,1,3,H,W) for a visual goal or a (384,) language embedding tensor.  Returns the plan (32,) int32."""
        keep = []
        o = self._obs(obs, keep)
        gs = gg = gl = None
        if isinstance(goal, dict):
            gs = goal["rgb_static"].to(device=self.device, dtype=torch.float32).contiguous(); keep.append(gs)
            gg = goal["rgb_gripper"].to(device=self.device, dtype=torch.float32).contiguous(); keep.append(gg)
        else:
            gl = torch.as_tensor(goal).to(device=self.device, dtype=torch.float32).reshape(-1).contiguous(); keep.append(gl)
        mcil = self.dims.kind == "mcil"      # continuous (256,) fp32 plan instead of (32,) int32 category indices
        out = torch.zeros(256 if mcil else 32, dtype=torch.float32 if mcil else torch.int32, device=self.device)
        L.check(self.lib.hulc_rollout_plan(self.ctx, C.byref(o), gs.data_ptr() if gs is not None else None, gg.data_ptr() if gg is not None else None,
                                           gl.data_ptr() if gl is not None else None, self._dev_or_host_ptr(plan_idx, keep, np.float32 if mcil else np.int32), out.data_ptr()))
        return out

    def rollout_act(self, obs: Dict, u_mix=None, u_act=None) -> np.ndarray:
        keep = []
        o = self._obs(obs, keep)
        out = (C.c_float * 7)()
        L.check(self.lib.hulc_rollout_act(self.ctx, C.byref(o), self._dev_or_host_ptr(u_mix, keep, np.float32),
                                          self._dev_or_host_ptr(u_act, keep, np.float32), out))
        return np.array(list(out), np.float32)

    def rollout_get_goal(self) -> np.ndarray:
        """The (32,) fp32 latent goal the last rollout_plan encoded (second return value of get_pp_plan_vision / get_pp_plan_lang)."""
        out = np.empty(32, np.float32)
        L.check(self.lib.hulc_rollout_get_goal(self.ctx, out.ctypes.data))
        return out

    def rollout_set_state(self, plan, latent_goal) -> None:
        """Install a caller-held plan ((32,) int32 indices; (256,) fp32 for mcil; None for gcbc) and (32,) latent goal for the next rollout_act calls."""
        g = np.ascontiguousarray(np.asarray(latent_goal, np.float32).reshape(-1))
        if g.size != 32:
            raise ValueError("latent_goal must have 32 elements")
        p = None
        if plan is not None:
            mcil = self.dims.kind == "mcil"
            p = np.ascontiguousarray(np.asarray(plan, np.float32 if mcil else np.int32).reshape(-1))
            if p.size != (256 if mcil else 32):
                raise ValueError("plan must have %d elements" % (256 if mcil else 32))
        L.check(self.lib.hulc_rollout_set_state(self.ctx, p.ctypes.data if p is not None else None, g.ctypes.data))

    # ------------------------------------------------------------------ batched multi-environment rollout (hulc_rollout_envs_*)
    def _envs_obs(self, obs: Dict, env_ids, keep, need_robot: bool):
        """obs: rgb_static (n,[1,]3,200,200), rgb_gripper (n,[1,]3,84,84), robot_obs_raw (n,[1,]15); env_ids: the slot of every row (None = 0..n-1)."""
        def dev(t, tail):
            t = torch.as_tensor(t)
            t = t.to(device=self.device, dtype=torch.float32).reshape((int(t.shape[0]),) + tail).contiguous()
            keep.append(t)
            return t
        rs, rg = dev(obs["rgb_static"], (3, 200, 200)), dev(obs["rgb_gripper"], (3, 84, 84))
        n = int(rs.shape[0])
        if rg.shape[0] != n:
            raise ValueError("rgb_static and rgb_gripper disagree on the number of rows")
        ro = None
        if need_robot:
            ro = dev(obs["robot_obs_raw"], (15,))
            if ro.shape[0] != n:
                raise ValueError("robot_obs_raw must have one row per environment")
        o = L.HulcRolloutEnvsObs(n=n, slots=self._slots_ptr(env_ids, n, keep), rgb_static=rs.data_ptr(), rgb_gripper=rg.data_ptr(),
                                 robot_obs_raw=ro.data_ptr() if ro is not None else None)
        return o, n

    @staticmethod
    def _slots_ptr(env_ids, n, keep):
        if env_ids is None:
            return None
        s = np.ascontiguousarray(np.asarray(env_ids, np.int32).reshape(-1))
        if n is not None and s.size != n:
            raise ValueError(f"{s.size} env ids for {n} rows")
        keep.append(s)
        return s.ctypes.data

    def _plan_shape(self):
        mcil = self.dims.kind == "mcil"
        return (256 if mcil else 32), (torch.float32 if mcil else torch.int32), (np.float32 if mcil else np.int32)

    def rollout_envs_init(self, max_envs: int) -> None:
        """Give the context `max_envs` (<= max_batch, <= 64) independent policy slots; clears every slot; may be called again."""
        L.check(self.lib.hulc_rollout_envs_init(self.ctx, int(max_envs)))

    def rollout_envs_reset(self, env_ids=None, clear_hidden: bool = False) -> None:
        """Drop plan and goal of the slots `env_ids` (None = all); hulc / mcil also zero their hidden states, gcbc only with clear_hidden."""
        keep = []
        n = 0 if env_ids is None else len(env_ids)
        L.check(self.lib.hulc_rollout_envs_reset(self.ctx, n, self._slots_ptr(env_ids, None, keep), int(bool(clear_hidden))))

    def rollout_envs_plan(self, obs: Dict, goal, env_ids=None, plan=None, want_goal: bool = False):
        """goal: dict(rgb_static (n,[1,]3,200,200), rgb_gripper) for visual goals or an (n,384) language-embedding tensor — one kind per call.
        plan: optional injected (n,32) int / (n,256) fp32 (mcil) plans.  Returns the stored plans as a device tensor (None for gcbc), with want_goal the
        pair (plans, (n,32) fp32 latent goals as numpy)."""
        keep = []
        o, n = self._envs_obs(obs, env_ids, keep, False)
        gs = gg = gl = None
        if isinstance(goal, dict):
            gs = torch.as_tensor(goal["rgb_static"]).to(device=self.device, dtype=torch.float32).reshape(-1, 3, 200, 200).contiguous()
            gg = torch.as_tensor(goal["rgb_gripper"]).to(device=self.device, dtype=torch.float32).reshape(-1, 3, 84, 84).contiguous()
            if gs.shape[0] != n or gg.shape[0] != n:
                raise ValueError("one goal image pair per row")
        else:
            gl = torch.as_tensor(goal).to(device=self.device, dtype=torch.float32).reshape(-1, 384).contiguous()
            if gl.shape[0] != n:
                raise ValueError("one (384,) language embedding per row")
        width, tdt, ndt = self._plan_shape()
        if plan is not None and int(np.prod(plan.shape)) != n * width:
            raise ValueError(f"plan must be ({n},{width})")
        out = torch.zeros(n, width, dtype=tdt, device=self.device) if self.dims.kind != "gcbc" else None
        lg = np.empty((n, 32), np.float32) if want_goal else None
        L.check(self.lib.hulc_rollout_envs_plan(self.ctx, C.byref(o), gs.data_ptr() if gs is not None else None, gg.data_ptr() if gg is not None else None,
                                                gl.data_ptr() if gl is not None else None, self._dev_or_host_ptr(plan, keep, ndt),
                                                out.data_ptr() if out is not None else None, lg.ctypes.data if want_goal else None))
        return (out, lg) if want_goal else out

    def rollout_envs_act(self, obs: Dict, env_ids=None, u_mix=None, u_act=None) -> np.ndarray:
        """One decoder step for the n rows of `obs` on their slots' plans, goals and hidden states.  Returns the (n,7) world-frame actions."""
        keep = []
        o, n = self._envs_obs(obs, env_ids, keep, True)
        D = 7 if self.dims.kind == "mcil" else 6
        if u_mix is not None and int(np.prod(u_mix.shape)) != n * D * 10:
            raise ValueError(f"u_mix must be ({n},{D},10)")
        if u_act is not None and int(np.prod(u_act.shape)) != n * D:
            raise ValueError(f"u_act must be ({n},{D})")
        out = np.empty((n, 7), np.float32)
        L.check(self.lib.hulc_rollout_envs_act(self.ctx, C.byref(o), self._dev_or_host_ptr(u_mix, keep, np.float32),
                                               self._dev_or_host_ptr(u_act, keep, np.float32), out.ctypes.data))
        return out

    def rollout_envs_get_state(self, env_ids):
        """(plans, latent goals) of the slots `env_ids` as numpy: (n,32) int32 | (n,256) fp32 | None (gcbc), (n,32) fp32."""
        keep = []
        n = len(env_ids)
        width, _, ndt = self._plan_shape()
        plan = np.empty((n, width), ndt) if self.dims.kind != "gcbc" else None
        goal = np.empty((n, 32), np.float32)
        L.check(self.lib.hulc_rollout_envs_get_state(self.ctx, n, self._slots_ptr(env_ids, n, keep), plan.ctypes.data if plan is not None else None, goal.ctypes.data))
        return plan, goal

    def rollout_envs_set_state(self, env_ids, plan, latent_goal) -> None:
        """Install caller-held plans ((n,32) int | (n,256) fp32 for mcil | None for gcbc) and (n,32) latent goals; the hidden states are not touched."""
        keep = []
        n = len(env_ids)
        width, _, ndt = self._plan_shape()
        g = np.ascontiguousarray(np.asarray(latent_goal, np.float32).reshape(-1))
        if g.size != n * 32:
            raise ValueError(f"latent_goal must be ({n},32)")
        p = None
        if plan is not None:
            p = np.ascontiguousarray(np.asarray(plan.cpu() if torch.is_tensor(plan) else plan, ndt).reshape(-1))
            if p.size != n * width:
                raise ValueError(f"plan must be ({n},{width})")
        L.check(self.lib.hulc_rollout_envs_set_state(self.ctx, n, self._slots_ptr(env_ids, n, keep), p.ctypes.data if p is not None else None, g.ctypes.data))

    def set_kl_beta(self, kl_beta: float):
        L.check(self.lib.hulc_set_kl_beta(self.ctx, float(kl_beta)))

    def set_dropout(self, p: float):
        L.check(self.lib.hulc_set_dropout(self.ctx, float(p)))

    def set_option(self, name: str, value: int):
        """Runtime options of the context (include/hulc_hip.h: hulc_set_option), e.g. ``persistent_rnn`` = 0 when processes share one GPU."""
        L.check(self.lib.hulc_set_option(self.ctx, name.encode(), int(value)))

    def timers_enable(self, on: bool = True, only: str = ""):
        L.check(self.lib.hulc_timers_enable(self.ctx, int(on), only.encode()))

    def timers_read(self, reset: bool = True) -> dict:
        import json
        buf = C.create_string_buffer(1 << 16)
        L.check(self.lib.hulc_timers_read(self.ctx, buf, len(buf), int(reset)))
        return json.loads(buf.value.decode())

    def backward(self, part: int = -1):
        """part -1: whole backward; 0: everything but the perceptual encoders; 1: the encoders (must follow 0)."""
        if part < 0:
            L.check(self.lib.hulc_backward(self.ctx))
        else:
            L.check(self.lib.hulc_backward_part(self.ctx, part))
        if part != 0:                  # the encoders' backward (conv1's weight gradient) is the last reader of a batch's frames
            self._staged_done()

    @property
    def encoder_numel(self) -> int:
        """Flat-buffer elements [0, encoder_numel) belong to perceptual_encoder.*; the rest is final after backward(part=0)."""
        return min(off for n, (off, _) in self.layout.items() if not n.startswith("perceptual_encoder."))

    def adam_step(self, lr=2e-4, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0):
        self.adam_t += 1
        self._check_step(self.lib.hulc_adam_step(self.ctx, lr, b1, b2, eps, self.adam_t, grad_scale))

    def _check_step(self, rc: int) -> None:
        """L.check for the optimizer entries: a call refused because the averaged weights are swapped in was no step, `adam_t` does not count it."""
        if rc and self.flat_ema is not None and self.ema_swapped:
            self.adam_t -= 1
        L.check(rc)

    def optimizer_step(self, kind="adam", lr=2e-4, b1=0.9, b2=0.999, eps=1e-8, weight_decay=0.0, momentum=0.0, dampening=0.0, nesterov=False, grad_scale=1.0):
        """hulc_optimizer_step: torch.optim.Adam / AdamW / SGD (conf/model/optimizer/*.yaml) over the flat buffers; `adam_t` counts the calls."""
        self.adam_t += 1
        o = L.HulcOptim(kind=L.OPTIM[kind], lr=lr, beta1=b1, beta2=b2, eps=eps, weight_decay=weight_decay, momentum=momentum, dampening=dampening,
                        nesterov=int(bool(nesterov)), step=self.adam_t, grad_scale=grad_scale)
        self._check_step(self.lib.hulc_optimizer_step(self.ctx, C.byref(o)))

    # ---- data-parallel gradient all-reduce owned by the library (RCCL over xGMI, include/hulc_hip.h: hulc_comm_*) ---------------
    @staticmethod
    def comm_unique_id() -> bytes:
        """rank 0: the 128-byte ncclUniqueId every rank must pass to comm_init (distribute it with any store / torch.distributed)."""
        buf = C.create_string_buffer(128)
        L.check(L.load().hulc_comm_unique_id(buf, 128))
        return buf.raw

    def comm_prepare(self):
        """Phase 1 of comm_init (RCCL resolved, private stream created): can fail on one rank alone, so agree on it before comm_init blocks."""
        L.check(self.lib.hulc_comm_prepare(self.ctx))

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        L.check(self.lib.hulc_comm_init(self.ctx, buf, int(rank), int(world)))
        self.has_comm = True

    def comm_destroy(self):
        if getattr(self, "has_comm", False):
            self.lib.hulc_comm_destroy(self.ctx)
            self.has_comm = False

    def comm_buckets(self):
        """[(lo, hi)] element ranges of the flat gradient buffer in the order hulc_backward_allreduce reduces them."""
        lo, hi = (C.c_int64 * 8)(), (C.c_int64 * 8)()
        n = self.lib.hulc_comm_buckets(self.ctx, lo, hi, 8)
        if n < 0:
            L.check(1)
        return [(int(lo[i]), int(hi[i])) for i in range(n)]

    def comm_size(self):
        """(rank, world) of the live library communicator as RCCL itself reports them (hulc_comm_size)."""
        r, w = C.c_int32(-1), C.c_int32(-1)
        L.check(self.lib.hulc_comm_size(self.ctx, C.byref(r), C.byref(w)))
        return r.value, w.value

    def comm_stats(self) -> Dict:
        n, b = C.c_int64(), C.c_double()
        L.check(self.lib.hulc_comm_stats(self.ctx, C.byref(n), C.byref(b)))
        return dict(collectives=n.value, bytes=b.value)

    def comm_timeline(self) -> Dict:
        """hulc_comm_timeline (after a hulc_backward_allreduce with set_option('comm_timing', 1)): per bucket, when its collective started / ended
        relative to the END of the backward on the engine stream (us; negative = hidden under the backward), and the backward's own duration."""
        out = (C.c_double * 32)()
        bwd = C.c_double()
        n = self.lib.hulc_comm_timeline(self.ctx, out, 8, C.byref(bwd))
        if n < 0:
            L.check(1)
        b = [dict(bucket=int(out[4 * i + 3]), issued_at_us=round(out[4 * i], 1), done_at_us=round(out[4 * i + 1], 1), bytes=int(out[4 * i + 2])) for i in range(n)]
        exposed = max([x["done_at_us"] for x in b] + [0.0])
        return dict(backward_us=round(bwd.value, 1), buckets=b, exposed_after_backward_us=round(exposed, 1))

    def get_option(self, name: str) -> int:
        v = C.c_int64()
        L.check(self.lib.hulc_get_option(self.ctx, name.encode(), C.byref(v)))
        return int(v.value)

    def encoder_frames(self) -> int:
        """Frames the perceptual encoders ran on in the last forward_loss / forward_loss_pair / validate: B*S (the pair: both batches), or the
        number of real frames N' of a batch with `window_len_host` (hulc_get_option "encoder_frames")."""
        return self.get_option("encoder_frames")

    def allreduce_grads(self, bucket_dtype: str = "fp32"):
        """One SUM all-reduce of the whole gradient buffer (after backward()); stream-ordered, no host sync."""
        L.check(self.lib.hulc_allreduce_grads(self.ctx, L.DTYPE[bucket_dtype]))

    def backward_allreduce(self, bucket_dtype: str = "fp32"):
        """backward() of the step's last forward with the bucketed SUM all-reduce overlapped (reverse-forward order)."""
        L.check(self.lib.hulc_backward_allreduce(self.ctx, L.DTYPE[bucket_dtype]))
        self._staged_done()

    # ---- dynamic loss scaling (fp16 mode; torch.cuda.amp.GradScaler semantics, include/hulc_hip.h: hulc_scaler_*) ----------
    def scaler_enable(self, init_scale: float = 65536.0, growth_factor: float = 2.0, backoff_factor: float = 0.5, growth_interval: int = 2000):
        """init_scale <= 0 switches scaling off.  fp16 engines start with GradScaler's defaults, fp32 / bf16 engines with it off."""
        L.check(self.lib.hulc_scaler_enable(self.ctx, float(init_scale), float(growth_factor), float(backoff_factor), int(growth_interval)))

    def scaler_state(self) -> Dict:
        """{"scale", "growth_tracker", "skipped_steps", "last_found_inf", "taken_steps"} — synchronises the stream.  flat_grads holds gradients x scale."""
        sc, tr, sk, fi, tk = C.c_float(), C.c_int32(), C.c_int64(), C.c_int32(), C.c_int64()
        L.check(self.lib.hulc_scaler_get(self.ctx, C.byref(sc), C.byref(tr), C.byref(sk), C.byref(fi), C.byref(tk)))
        return dict(scale=sc.value, growth_tracker=tr.value, skipped_steps=sk.value, last_found_inf=fi.value, taken_steps=tk.value)

    def scaler_load(self, scale: float, growth_tracker: int = 0, taken_steps: int = -1):
        """taken_steps >= 0 also restores the device-side count of optimizer steps taken (Adam's bias corrections in fp16 mode)."""
        L.check(self.lib.hulc_scaler_set(self.ctx, float(scale), int(growth_tracker), int(taken_steps)))

    # ---- gradient clipping / gradient norms inside the optimizer step (include/hulc_hip.h: hulc_grad_clip_set / hulc_grad_norm_get) -------
    def set_grad_clip(self, algo: Optional[str], limit: Optional[float], track: bool = False):
        """Lightning's gradient_clip_algorithm / gradient_clip_val for every following adam_step / optimizer_step: algo "norm" (clip_grad_norm_),
        "value" (clip_grad_value_) or "off" / None; limit None / <= 0 = off.  track: compute the norms on every step whatever the algorithm.
        `flat_grads` (and the modules' .grad views) are NOT rewritten: the clipped values exist only inside the optimizer kernel."""
        algo = "off" if algo is None else str(algo)
        if algo not in L.CLIP:
            raise ValueError(f"gradient clip algorithm {algo!r}: expected 'norm', 'value' or 'off'")
        L.check(self.lib.hulc_grad_clip_set(self.ctx, L.CLIP[algo], float(limit or 0.0), int(bool(track))))

    def grad_norms(self, per_tensor: bool = False) -> Dict:
        """{"total", "coef"[, "per_tensor": {name: norm}]} of the LAST optimizer step's effective gradient (G x grad_scale / loss scale) before
        clipping — synchronises the stream.  Raises if that step computed no norm (clipping by norm or track not enabled)."""
        tot, coef = C.c_float(), C.c_float()
        n = len(self.layout)
        per = np.empty(n, np.float32) if per_tensor else None
        L.check(self.lib.hulc_grad_norm_get(self.ctx, C.byref(tot), C.byref(coef), per.ctypes.data if per_tensor else None, n))
        out = dict(total=tot.value, coef=coef.value)
        if per_tensor:
            out["per_tensor"] = {name: float(per[i]) for i, name in enumerate(self.layout.keys())}
        return out

    # ---- frozen parameters: the per-tensor trainable mask (include/hulc_hip.h: hulc_trainable_*) ---------------------------------------------
    def set_trainable(self, mask) -> None:
        """hulc_trainable_set: `mask` = {name: bool} (missing names keep their state) or a sequence of len(layout) flags in layout order.  A frozen
        tensor is left alone by the optimizer step (parameter, moments, 16-bit copies, no weight decay), its gradient is never read, and with every
        perceptual_encoder.* tensor frozen the encoder backward is not run.  Rebuilds the optimizer's tables: call it between steps, not in them."""
        names = list(self.layout.keys())
        if isinstance(mask, dict):
            unknown = [n for n in mask if n not in self.layout]
            if unknown:
                raise KeyError(f"set_trainable: unknown tensors {unknown[:5]}")
            cur = self.trainable()
            flags = [bool(mask.get(n, cur[n])) for n in names]
        else:
            flags = [bool(x) for x in mask]
        arr = np.ascontiguousarray(flags, np.uint8)
        L.check(self.lib.hulc_trainable_set(self.ctx, len(arr), arr.ctypes.data))

    def _trainable_get(self):
        n = len(self.layout)
        m, k = np.empty(n, np.uint8), np.empty(n, np.int64)
        L.check(self.lib.hulc_trainable_get(self.ctx, n, m.ctypes.data, k.ctypes.data))
        return m, k

    def trainable(self) -> Dict[str, bool]:
        """{name: trainable} as the engine holds it (all True before any set_trainable)."""
        m, _ = self._trainable_get()
        return {name: bool(m[i]) for i, name in enumerate(self.layout.keys())}

    def frozen_steps(self) -> Dict[str, int]:
        """{name: optimizer steps the tensor has sat out}: what torch.optim's per-parameter `step` is short of the global count."""
        _, k = self._trainable_get()
        return {name: int(k[i]) for i, name in enumerate(self.layout.keys())}

    def set_frozen_steps(self, steps, steps_taken: int = -1) -> None:
        """hulc_trainable_steps_set (checkpoint restore, after set_trainable): {name: count} (missing = 0) or a sequence in layout order, as of
        `steps_taken` optimizer steps (-1: the count the context holds)."""
        names = list(self.layout.keys())
        vals = [int(steps.get(n, 0)) for n in names] if isinstance(steps, dict) else [int(x) for x in steps]
        arr = np.ascontiguousarray(vals, np.int64)
        L.check(self.lib.hulc_trainable_steps_set(self.ctx, len(arr), arr.ctypes.data, int(steps_taken)))

    # ---- averaged weights: an EMA of the parameters kept behind the optimizer step (include/hulc_hip.h: hulc_ema_*) ------------------------------
    def ema_enable(self, decay: Optional[float], start_step: int = 0, warmup: bool = True) -> None:
        """hulc_ema_enable: allocate `flat_ema` (numel fp32, +4 bytes per parameter), fill it with the current parameters and average from the next
        optimizer step on: e += (1 - d)(p - e), d = spec.ema_decay_at(update number, decay, warmup); a copy e = p while the update number is below
        start_step.  decay None switches the average off."""
        if decay is None:
            L.check(self.lib.hulc_ema_enable(self.ctx, None, 0.0, 0, 0))
            self.flat_ema = None
            return
        spec.ema_check(decay, start_step)
        buf = torch.empty(self.numel, dtype=torch.float32, device=self.device)
        L.check(self.lib.hulc_ema_enable(self.ctx, buf.data_ptr(), float(decay), int(start_step), int(bool(warmup))))
        self.flat_ema = buf
        self._ema_cfg = dict(decay=float(decay), start_step=int(start_step), warmup=bool(warmup))

    flat_ema: Optional[torch.Tensor] = None

    def ema_state(self) -> Dict:
        """{"updates", "last_decay", "decay", "start_step", "warmup"} — synchronises the stream."""
        n, d = C.c_int64(), C.c_float()
        L.check(self.lib.hulc_ema_state_get(self.ctx, C.byref(n), C.byref(d)))
        return dict(updates=int(n.value), last_decay=float(d.value), **self._ema_cfg)

    def ema_load(self, named_tensors: Dict, updates: int) -> None:
        """Checkpoint restore: {name: tensor} for every tensor of the layout into `flat_ema`, and the update count (hulc_ema_state_set)."""
        if self.flat_ema is None:
            raise RuntimeError("ema_load: the average is off (ema_enable first)")
        if self.ema_swapped:
            raise RuntimeError("ema_load: the averaged weights are swapped in (ema_swap back first)")
        missing = [n for n in self.layout if n not in named_tensors]
        if missing:
            raise KeyError(f"ema_load: missing tensors {missing[:5]}")
        for n, t in self.views(self.flat_ema).items():
            t.copy_(torch.as_tensor(named_tensors[n]).to(self.device, torch.float32).reshape(t.shape))
        L.check(self.lib.hulc_ema_state_set(self.ctx, int(updates)))

    def ema_swap(self) -> None:
        """hulc_ema_swap: exchange `flat_params` and `flat_ema` bit for bit and rebuild every weight copy; a second call swaps back.  While swapped,
        validate / forward_loss / the rollouts run on the averaged weights and optimizer_step / backward / set_trainable / ema_enable raise."""
        L.check(self.lib.hulc_ema_swap(self.ctx))

    @property
    def ema_swapped(self) -> bool:
        out = C.c_int32()
        L.check(self.lib.hulc_ema_swapped(self.ctx, C.byref(out)))
        return bool(out.value)

    def get_tensor(self, name: str, n: int) -> np.ndarray:
        out = np.zeros(n, np.float32)
        got = C.c_int64()
        L.check(self.lib.hulc_get_tensor(self.ctx, name.encode(), out.ctypes.data, n, C.byref(got)))
        return out[:got.value]

    def plan_idx(self, B: int) -> np.ndarray:
        out = np.zeros(B * 32, np.int32)
        L.check(self.lib.hulc_get_plan_idx(self.ctx, out.ctypes.data, out.size))
        return out.reshape(B, 32)

    def workspace_bytes(self) -> int:
        return int(self.lib.hulc_workspace_bytes(self.ctx))

    def close(self):
        if getattr(self, "ctx", None):
            self.comm_destroy()
            self.lib.hulc_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
