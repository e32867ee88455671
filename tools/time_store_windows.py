"""Step time of the frame-store path with fixed and with variable-length padded windows (hulc_batch::window_len) — vision-only, B=64, S=32, bf16, a
store of 16384 frames, new random windows every step (bench.py's `--ingest u8 --store 16384` row), median ms/step over bench.py's default number of
timed steps, each step timed with its own pair of events.

    python tools/time_store_windows.py                                   # fixed windows, then lens uniform 20..32, of this tree's library
    HULC_LIB_PATH=<older libhulc_hip.so> python tools/time_store_windows.py --modes fixed      # the same fixed-window run on another build

    python tools/time_store_windows.py --modes padded --host-share 0,0.25,1.0      # two-tier store: that share of the frames in pinned host memory
    python tools/time_store_windows.py --modes padded,ragged,ragged_full [--pair]  # the ragged encoder pass (hulc_batch::window_len_host) against the padded one

Modes: `fixed` (window_start alone), `padded` (+ window_len, lens uniform min_window..S), `ragged` (the same lens also as window_len_host: the encoders
run on the real frames only), `ragged_full` (window_len_host with every len = S: the ragged pass's own overhead at an unchanged frame count).
--pair: the vis + lang paired pass (hulc_forward_loss_pair) on 2 x batch windows, each modality with its own windows and lens.
profiles/ragged_windows.txt records the numbers of the commit that added window_len_host.

Prints one JSON line per mode.  profiles/store_windows.txt records the numbers of the commit that added window_len, profiles/store_tiers.txt those
of the two-tier store.

--host-share f (a list): the store is cut so that the last f of its frames (whole 64-frame episodes) live on the host; the padded windows of every
step are staged through FrameStore.stage — once one step ahead (`lookahead`: stage n + 1, then run n) and once serialised (`serial`: stage n, run n).
Each line adds the bytes staged per step, the achieved copy rate of the serialised form's staging alone and persistent_rnn_fallbacks.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hulc_amd import spec  # noqa: E402
from hulc_amd.engine import StepEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq", type=int, default=32)
    ap.add_argument("--store", type=int, default=16384)
    ap.add_argument("--min-window", type=int, default=20)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--modes", default="fixed,padded")
    ap.add_argument("--repeat", type=int, default=1, help="timed passes per mode (run-to-run spread inside one process)")
    ap.add_argument("--pair", action="store_true", help="time the paired vis + lang pass (2 x batch windows) instead of one modality")
    ap.add_argument("--host-share", default="", help="comma-separated shares of the store kept in pinned host memory (two-tier store; padded windows)")
    args = ap.parse_args()
    B, S, F, dev = args.batch, args.seq, args.store, torch.device("cuda:0")
    dims = spec.ModelDims(kind="hulc", max_window=max(32, S), use_clip=False)
    eng = StepEngine(dims, 2 * B if args.pair else B, S, dtype=args.dtype, device=str(dev), dropout_p=0.1, seed=42, num_classes=dims.mix_classes)
    eng.load_numpy(spec.init_all(dims, seed=0))
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    store = lambda h: torch.cat([torch.randint(0, 256, (min(1024, F - f0), h, h, 3), device=dev, generator=g, dtype=torch.int32).to(torch.uint8) for f0 in range(0, F, 1024)]).contiguous()
    act = torch.rand(B, S, 7, device=dev, generator=g) * 2 - 1
    act[..., 6] = torch.where(torch.rand(B, S, device=dev, generator=g) < 0.5, -1.0, 1.0)
    ro = torch.randn(B, S, 15, device=dev, generator=g) * 0.3
    mb = dict(rgb_static=store(200), rgb_gripper=store(84), actions=act.contiguous(), robot_obs=ro.contiguous(), pad_static=10, pad_gripper=4,
              shift_static=torch.randint(0, 21, (B * S, 2), device=dev, generator=g, dtype=torch.int32),
              shift_gripper=torch.randint(0, 9, (B * S, 2), device=dev, generator=g, dtype=torch.int32))
    starts = torch.randint(0, F - S + 1, (64, B), device=dev, generator=g, dtype=torch.int64)
    lens = torch.randint(args.min_window, S + 1, (64, B), device=dev, generator=g, dtype=torch.int32)
    full = torch.full((B,), S, device=dev, dtype=torch.int32)
    lens_host, full_host = lens.cpu().numpy(), np.full(B, S, np.int32)      # the host arrays a datamodule holds of its own draws
    lang = torch.nn.functional.normalize(torch.randn(B, 384, device=dev, generator=g), dim=-1)
    mb_l = dict(mb, lang=lang, shift_static=mb["shift_static"].flip(0).contiguous(), shift_gripper=mb["shift_gripper"].flip(0).contiguous())

    def windows(d, i, mode):
        d = dict(d, window_start=starts[i % 64])
        if mode in ("padded", "ragged"):
            d["window_len"] = lens[i % 64]
        if mode == "ragged":
            d["window_len_host"] = lens_host[i % 64]
        if mode == "ragged_full":
            d["window_len"], d["window_len_host"] = full, full_host
        return d

    def step(i, mode):
        eng.zero_grads()
        if args.pair:      # the lang modality draws the windows of another step
            eng.forward_loss_pair(windows(mb, i, mode), windows(mb_l, i + 17, mode), 0.5, 3.0, step=i, sync_losses=False)
        else:
            eng.forward_loss(windows(mb, i, mode), False, 1.0, 3.0, step=i, sync_losses=False)
        eng.backward()
        eng.adam_step(lr=2e-4)

    if args.host_share:
        tiers(args, eng, mb, starts, lens)
        eng.close()
        return
    for mode in args.modes.split(","):
        if mode not in ("fixed", "padded", "ragged", "ragged_full"):
            raise SystemExit(f"unknown mode {mode!r}")
        padded = mode in ("padded", "ragged")
        for rep in range(args.repeat):
            for i in range(args.warmup):
                step(i, mode)
            torch.cuda.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
            for i, (a, b) in enumerate(ev):
                a.record()
                step(args.warmup + i, mode)
                b.record()
            torch.cuda.synchronize()
            ms = np.array([a.elapsed_time(b) for a, b in ev])
            print(json.dumps(dict(mode=mode, pair=bool(args.pair), encoder_frames=eng.encoder_frames() if hasattr(eng.lib, "hulc_k_rows_reduce") else None, rep=rep, lib=os.environ.get("HULC_LIB_PATH") or "in-tree", B=B, S=S, store_frames=F, dtype=args.dtype, steps=args.steps,
                                  median_ms=round(float(np.median(ms)), 4), mean_ms=round(float(ms.mean()), 4), p10_ms=round(float(np.percentile(ms, 10)), 4),
                                  p90_ms=round(float(np.percentile(ms, 90)), 4), mean_window_len=round(float(lens.float().mean()), 2) if padded else float(S))), flush=True)
    eng.close()


def tiers(args, eng, mb, starts, lens):
    """The padded-window step on a two-tier store built from the same frames: episodes of 64 frames, the last `share` of them on the host."""
    from hulc_amd.utils.frame_store import FrameStore
    B, S, F = args.batch, args.seq, args.store
    ends = list(range(64, F, 64)) + [F]
    # every window inside one 64-frame episode (the all-resident tool draws them anywhere; a tiered store cuts on episode boundaries)
    st_h = starts.cpu().numpy()
    ln_h = lens.cpu().numpy()
    st_h = np.minimum(st_h, (st_h // 64) * 64 + 64 - ln_h)
    st_h = np.minimum(st_h, F - ln_h)
    host_s, host_g = mb["rgb_static"].cpu(), mb["rgb_gripper"].cpu()
    for share in [float(x) for x in args.host_share.split(",")]:
        store = FrameStore(host_s, host_g, episode_ends=ends, device="cuda:0", resident_frames=int(round(F * (1.0 - share))), stage_slots=2 * B,
                           stage_slot_frames=S).attach(eng)

        def run(i, h):
            d = dict(mb, rgb_static=store.rgb_static, rgb_gripper=store.rgb_gripper, window_start=torch.from_numpy(h.frame_starts).cuda(),
                     window_len=torch.from_numpy(h.lens).cuda(), staged=h)
            if h.ticket:
                eng.store_stage_join(h.ticket)
            eng.zero_grads()
            eng.forward_loss(d, False, 1.0, 3.0, step=i, sync_losses=False)
            eng.backward()
            eng.adam_step(lr=2e-4)

        stage = lambda i: store.stage(st_h[i % 64], S, ln_h[i % 64])
        for order in ("lookahead", "serial"):
            for rep in range(args.repeat):
                n = args.warmup + args.steps
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
                torch.cuda.synchronize()
                b0 = eng.store_stage_stats()["bytes"]
                ahead = stage(0) if order == "lookahead" else None
                host_t = 0.0                   # time the launching thread spends inside FrameStore.stage (planning + one hulc_store_stage)
                for i, (a, b) in enumerate(ev):
                    a.record()
                    t_host = time.perf_counter()
                    if order == "lookahead":
                        cur, ahead = ahead, (stage(i + 1) if i + 1 < n else None)
                    else:
                        cur = stage(i)
                    host_t += time.perf_counter() - t_host
                    run(i, cur)
                    b.record()
                torch.cuda.synchronize()
                ms = np.array([a.elapsed_time(b) for a, b in ev])[args.warmup:]
                per_step = (eng.store_stage_stats()["bytes"] - b0) / n
                # the copy rate: the same staging calls alone, nothing else on the device
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                c0 = eng.store_stage_stats()["bytes"]
                t0.record()
                for i in range(8):
                    h = stage(i)
                    if h.ticket:
                        eng.store_stage_join(h.ticket)
                    h.release()
                t1.record()
                torch.cuda.synchronize()
                copied = eng.store_stage_stats()["bytes"] - c0
                rate = copied / (t0.elapsed_time(t1) * 1e-3) / 1e9 if copied else 0.0
                print(json.dumps(dict(mode="tiers", order=order, host_share=share, resident_frames=store.R, rep=rep, B=B, S=S, store_frames=F, dtype=args.dtype, steps=args.steps,
                                      median_ms=round(float(np.median(ms)), 4), mean_ms=round(float(ms.mean()), 4), p10_ms=round(float(np.percentile(ms, 10)), 4),
                                      p90_ms=round(float(np.percentile(ms, 90)), 4), staged_mb_per_step=round(per_step / 1e6, 2), copy_gb_per_s=round(rate, 2), stage_host_us=round(host_t / n * 1e6, 1),
                                      persistent_rnn_fallbacks=eng.get_option("persistent_rnn_fallbacks"))), flush=True)
        del store


if __name__ == "__main__":
    main()
