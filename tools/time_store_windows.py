"""Step time of the frame-store path with fixed and with variable-length padded windows (hulc_batch::window_len) — vision-only, B=64, S=32, bf16, a
store of 16384 frames, new random windows every step (bench.py's `--ingest u8 --store 16384` row), median ms/step over bench.py's default number of
timed steps, each step timed with its own pair of events.

    python tools/time_store_windows.py                                   # fixed windows, then lens uniform 20..32, of this tree's library
    HULC_LIB_PATH=<older libhulc_hip.so> python tools/time_store_windows.py --modes fixed      # the same fixed-window run on another build

Prints one JSON line per mode.  profiles/store_windows.txt records the numbers of the commit that added window_len.
"""
import argparse
import json
import os
import sys

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
    args = ap.parse_args()
    B, S, F, dev = args.batch, args.seq, args.store, torch.device("cuda:0")
    dims = spec.ModelDims(kind="hulc", max_window=max(32, S), use_clip=False)
    eng = StepEngine(dims, B, S, dtype=args.dtype, device=str(dev), dropout_p=0.1, seed=42, num_classes=dims.mix_classes)
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

    def step(i, padded):
        d = dict(mb, window_start=starts[i % 64])
        if padded:
            d["window_len"] = lens[i % 64]
        eng.zero_grads()
        eng.forward_loss(d, False, 1.0, 3.0, step=i, sync_losses=False)
        eng.backward()
        eng.adam_step(lr=2e-4)

    for mode in args.modes.split(","):
        padded = mode == "padded"
        for rep in range(args.repeat):
            for i in range(args.warmup):
                step(i, padded)
            torch.cuda.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
            for i, (a, b) in enumerate(ev):
                a.record()
                step(args.warmup + i, padded)
                b.record()
            torch.cuda.synchronize()
            ms = np.array([a.elapsed_time(b) for a, b in ev])
            print(json.dumps(dict(mode=mode, rep=rep, lib=os.environ.get("HULC_LIB_PATH") or "in-tree", B=B, S=S, store_frames=F, dtype=args.dtype, steps=args.steps,
                                  median_ms=round(float(np.median(ms)), 4), mean_ms=round(float(ms.mean()), 4), p10_ms=round(float(np.percentile(ms, 10)), 4),
                                  p90_ms=round(float(np.percentile(ms, 90)), 4), mean_window_len=round(float(lens.float().mean()), 2) if padded else float(S))), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
