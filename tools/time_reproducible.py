#!/usr/bin/env python
"""Cost of the reproducible mode (hulc_set_option "reproducible") on the flagship shape: B = 64 windows per modality as one paired pass, S = 32, bf16, dropout 0.1,
forward + backward + Adam.

The modes `default` and `reproducible` alternate in ONE process and on ONE engine (the option is latched by the next hulc_zero_grads), --rounds rounds of --steps
steps each after a warm-up of both; per mode the median over the rounds of the mean ms/step of a round (host clock around steps that end in a synchronise), the
range of the rounds, and the per-class launch counts of one step (hulc_timers, a pass of its own that is not timed).

A library that predates the option (HULC_LIB_PATH = the parent commit's build, tools/ab_lib.sh shows how to make one) runs the default mode alone: its rounds are
the parent's own run-to-run range, and its launch counts are what the default mode of this build has to equal.

  python tools/time_reproducible.py [--rounds 6] [--steps 20] [--out profiles/reproducible.txt]
  HULC_LIB_PATH=tools/bin/libhulc_parent.so python tools/time_reproducible.py --out -          # the parent's figures, same job
Prints one JSON line; --out FILE appends a readable table to FILE."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench import synth_batch  # noqa: E402
from hulc_amd import spec  # noqa: E402
from hulc_amd.engine import StepEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq", type=int, default=32)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_reproducible.py needs a HIP device: a timing without one says nothing")
    B, S, dev = args.batch, args.seq, torch.device("cuda:0")
    dims = spec.ModelDims(kind="hulc", max_window=max(32, S), use_clip=True)
    eng = StepEngine(dims, 2 * B, S, dtype="bf16", device="cuda:0", dropout_p=0.1, seed=3, num_classes=dims.mix_classes)
    eng.load_numpy(spec.init_all(dims, seed=0, ln_jitter=True))
    vis, lang = synth_batch(B, S, dev, 7, False, "fp32"), synth_batch(B, S, dev, 8, True, "fp32")
    try:
        eng.set_option("reproducible", 0)
        modes = ["default", "reproducible"]
    except RuntimeError:
        modes = ["default"]                      # an older build of the library: the option does not exist
    which = os.environ.get("HULC_LIB_PATH") or "in-tree build"
    n = [0]

    def step():
        eng.zero_grads()
        eng.forward_loss_pair(vis, lang, 0.5, 3.0, step=n[0], sync_losses=False)
        eng.backward()
        eng.adam_step(lr=1e-4)
        n[0] += 1

    def select(mode):
        if len(modes) > 1:
            eng.set_option("reproducible", int(mode == "reproducible"))

    launches = {}
    for mode in modes:                            # warm-up of both routings, then the launch counts of one step
        select(mode)
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        eng.timers_enable(True)
        eng.timers_read(reset=True)
        step()
        torch.cuda.synchronize()
        launches[mode] = {k: int(v["launches"]) for k, v in sorted(eng.timers_read(reset=True).items())}
        eng.timers_enable(False)
    rounds = {m: [] for m in modes}
    for _ in range(args.rounds):
        for mode in modes:
            select(mode)
            step()                                # the switch itself (latched by this step's zero_grads) stays outside the clock
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            rounds[mode].append((time.perf_counter() - t0) * 1e3 / args.steps)
    res = dict(library=which, B=B, S=S, dtype="bf16", dropout=0.1, rounds=args.rounds, steps=args.steps,
               ms_per_step={m: dict(median=statistics.median(v), min=min(v), max=max(v), rounds=[round(x, 4) for x in v]) for m, v in rounds.items()},
               launches=launches, nondeterministic_sites=eng.get_option("nondeterministic_sites") if len(modes) > 1 else None)
    eng.close()
    print(json.dumps(res))
    if args.out and args.out != "-":
        with open(args.out, "a") as f:
            f.write(f"\nlibrary: {which}   (paired pass, B = {B} per modality, S = {S}, bf16, dropout 0.1; {args.rounds} rounds x {args.steps} steps per mode, alternating)\n")
            for m in modes:
                r = res["ms_per_step"][m]
                f.write(f"  {m:13s} median {r['median']:.4f} ms/step   rounds min {r['min']:.4f} max {r['max']:.4f}   {r['rounds']}\n")
            classes = sorted(set().union(*[set(v) for v in launches.values()]))
            f.write("  launches per step by timer class (" + " / ".join(modes) + "):\n")
            for c in classes:
                f.write(f"    {c:28s} " + " / ".join(str(launches[m].get(c, 0)) for m in modes) + "\n")


if __name__ == "__main__":
    main()
