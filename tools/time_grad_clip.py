"""Cost of gradient clipping by norm inside the optimizer step (hulc_grad_clip_set): the bench.py headline step (hulc, vision batch, B = 64, S = 32)
timed with clipping OFF and ON in ONE process, alternating blocks, every block ended by a synchronise.  The off arm is the unchanged step, so the
comparison needs no number from another machine.

    python tools/time_grad_clip.py [--dtype bf16|fp16] [--steps 200] [--blocks 3] [--arms off,norm,track,value] [--out FILE]

Arms: off; norm (HULC_CLIP_NORM, limit 1.0); track (norms only); value (HULC_CLIP_VALUE: no norm pass, a clamp inside the optimizer kernel).
Prints one table; --out appends it to a file."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import synth_batch  # noqa: E402
from hulc_amd import spec  # noqa: E402
from hulc_amd.engine import StepEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq", type=int, default=32)
    ap.add_argument("--steps", type=int, default=200, help="steps per block")
    ap.add_argument("--blocks", type=int, default=3, help="blocks per arm")
    ap.add_argument("--preroll", type=int, default=300)
    ap.add_argument("--arms", default="off,norm")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    B, S = args.batch, args.seq
    dims = spec.ModelDims(kind="hulc", max_window=max(32, S), use_clip=False)
    eng = StepEngine(dims, B, S, dtype=args.dtype, device=str(dev), dropout_p=0.1, seed=42, num_classes=dims.mix_classes)
    eng.load_numpy(spec.init_all(dims, seed=0))
    mb = synth_batch(B, S, dev, 1, False)
    n_step = [0]

    def step():
        eng.zero_grads()
        eng.forward_loss(mb, False, 1.0, 3.0, step=n_step[0], sync_losses=False)
        eng.backward()
        eng.adam_step(lr=2e-4)
        n_step[0] += 1

    def arm_on(name):
        if name == "off":
            eng.set_grad_clip("off", None)
        elif name == "norm":
            eng.set_grad_clip("norm", 1.0)
        elif name == "track":
            eng.set_grad_clip("off", None, track=True)
        elif name == "value":
            eng.set_grad_clip("value", 1e-3)
        else:
            raise SystemExit(f"unknown arm {name!r}")

    arms = args.arms.split(",")
    for _ in range(args.preroll):
        step()
    torch.cuda.synchronize()
    ms = {a: [] for a in arms}
    for _ in range(args.blocks):
        for a in arms:
            arm_on(a)
            for _ in range(10):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            ms[a].append((time.perf_counter() - t0) * 1e3 / args.steps)
    gbytes = sum(int(torch.tensor(shape).prod()) if len(shape) else 1 for _, shape in eng.layout.values()) * 4 / 1e9
    lines = [f"# tools/time_grad_clip.py --dtype {args.dtype} --batch {B} --seq {S} --steps {args.steps} --blocks {args.blocks}: ms/step per block, one process, alternating blocks",
             f"# the norm pass reads {gbytes * 1e3:.1f} MB of gradients per step",
             "arm          mean_ms   min_ms    max_ms    added_us_vs_off"]
    base = statistics.mean(ms[arms[0]])
    for a in arms:
        m = statistics.mean(ms[a])
        lines.append(f"{a:<12} {m:8.4f}  {min(ms[a]):8.4f}  {max(ms[a]):8.4f}  {(m - base) * 1e3:+8.1f}")
    txt = "\n".join(lines)
    print(txt)
    if args.out:
        with open(args.out, "a") as f:
            f.write(txt + "\n")
    eng.close()


if __name__ == "__main__":
    main()
