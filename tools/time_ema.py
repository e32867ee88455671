"""What the averaged weights (hulc_ema_enable) cost per training step on one MI355X, and what they cost a run that leaves them off.

    python tools/time_ema.py --parent PARENT_BUILD.so [--B 64] [--S 32] [--dtype bf16] [--rounds 3] [--steps 30] [--out profiles/ema_weights.txt]

Three cases, each the paired pass of a step (B visual + B language windows x S frames: forward + loss + backward + AdamW), median ms per step:
  (a) the parent commit's build of the library (HULC_LIB_PATH, hulc_amd/lib.py; tools/ab_lib.sh builds one) — measured as TWO independent series a1, a2;
  (b) this tree's build with the average off (hulc_ema_enable never called);
  (c) this tree's build with the average on (decay 0.999, warm-up).
The project has no run-time switch between builds, so every sample is a fresh child process: a1, b, a2, c alternate for `rounds` rounds, each child warms up,
then times `steps` steps between two device synchronisations, five times, and reports the five figures.  The spread of the two (a) series is the margin: (b)
passes when its median lies inside [min, max] over both.  (c) - (b) is recorded next to the pass's byte floor (12 bytes per parameter at the bandwidth the
Adam pass reaches), not gated.  A child of (c) also times the update kernel alone (hulc_k_ema_update over buffers of the model's size, between
two events) and one swap (exchange kernel + the full hulc_prepare_weights, host synchronised), and checks that the average moved.  A child that fails ends the run."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ADAM_TBS = 6.1      # TB/s of the Adam pass: the floor's bandwidth


def sample(a):
    import torch

    from bench import synth_batch
    from hulc_amd import lib as L
    from hulc_amd import spec
    from hulc_amd.engine import StepEngine
    dev = torch.device("cuda:0")
    dims = spec.ModelDims(kind="hulc", max_window=32, use_clip=True)
    eng = StepEngine(dims, 2 * a.B, a.S, dtype=a.dtype, dropout_p=0.1, device="cuda:0", seed=1)
    eng.load_numpy(spec.init_all(dims, seed=0))
    mv, ml = synth_batch(a.B, a.S, dev, 1, False), synth_batch(a.B, a.S, dev, 2, True)
    if a.ema:
        eng.ema_enable(0.999)

    def step(i):
        eng.zero_grads()
        eng.forward_loss_pair(mv, ml, 0.5, 3.0, step=i, sync_losses=False)
        eng.backward()
        eng.optimizer_step("adamw", weight_decay=0.01)

    for i in range(5):
        step(i)
    torch.cuda.synchronize()
    if a.ema and (eng.ema_state()["updates"] != 5 or torch.equal(eng.flat_ema, eng.flat_params)):
        sys.exit("the average did not follow the steps")
    ms = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.steps):
            step(5 + i)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
    out = dict(ms=ms, numel=int(eng.numel))
    if a.ema:
        # the update kernel alone, on buffers of the model's size that nothing else reads
        e, p = eng.flat_ema.clone(), eng.flat_params.clone()
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        run = lambda: L.check(eng.lib.hulc_k_ema_update(e.data_ptr(), p.data_ptr(), e.numel(), 1e-3, None, None, 0, st))
        for _ in range(5):
            run()
        k_us = []
        for _ in range(5):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(50):
                run()
            t1.record()
            torch.cuda.synchronize()
            k_us.append(t0.elapsed_time(t1) * 1e3 / 50)
        sw = []
        for _ in range(6):      # in and out, three times: the run ends on the raw weights
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.ema_swap()
            torch.cuda.synchronize()
            sw.append((time.perf_counter() - t0) * 1e3)
        out.update(kernel_us=k_us, swap_ms=sw)
    eng.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, metavar="PARENT_BUILD.so", help="the parent commit's build of libhulc_hip.so")
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--S", type=int, default=32)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sample", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--ema", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.sample:
        return sample(a)
    if not a.parent or not os.path.exists(a.parent):
        sys.exit("--parent PARENT_BUILD.so: the parent commit's build of the library is needed for case (a)")
    parent = os.path.abspath(a.parent)
    sides = [("a1", parent, False), ("b", None, False), ("a2", parent, False), ("c", None, True)]
    ms = {k: [] for k, _, _ in sides}
    k_us, sw, numel = [], [], 0
    for _ in range(a.rounds):
        for k, path, ema in sides:
            env = dict(os.environ)
            env.pop("HULC_LIB_PATH", None)
            if path:
                env["HULC_LIB_PATH"] = path
            cmd = [sys.executable, os.path.abspath(__file__), "--sample", "--B", str(a.B), "--S", str(a.S), "--dtype", a.dtype, "--steps", str(a.steps)] + (["--ema"] if ema else [])
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit(f"case {k}: the sampling process ended with {r.returncode}\n{r.stdout[-1000:]}{r.stderr[-3000:]}")
            res = json.loads(r.stdout.strip().splitlines()[-1])
            ms[k] += res["ms"]
            numel = res["numel"]
            k_us += res.get("kernel_us", [])
            sw += res.get("swap_ms", [])

    def line(v, unit="ms"):
        v = sorted(v)
        return f"{np.median(v):8.4f} {unit}   [{v[0]:.4f} .. {v[-1]:.4f}]   n = {len(v)}"
    lo, hi = min(ms["a1"] + ms["a2"]), max(ms["a1"] + ms["a2"])
    b, c = float(np.median(ms["b"])), float(np.median(ms["c"]))
    inside = lo <= b <= hi
    nbytes = 12.0 * numel
    floor_ms = nbytes / (ADAM_TBS * 1e12) * 1e3
    kern_ms = float(np.median(k_us)) * 1e-3
    out = [f"averaged weights (EMA), one MI355X, {a.dtype}, paired pass of B = {a.B} + {a.B} windows x S = {a.S} frames, forward + loss + backward + AdamW",
           f"ms per step, median [min .. max]; {a.rounds} alternating rounds of fresh processes per case, 5 samples of {a.steps} steps each",
           f"  (a1) parent build                      {line(ms['a1'])}",
           f"  (a2) parent build, second series       {line(ms['a2'])}",
           f"  (b)  this build, average off           {line(ms['b'])}",
           f"  (c)  this build, average on            {line(ms['c'])}",
           f"margin = the spread of the two parent series [{lo:.4f} .. {hi:.4f}]: median of (b) {b:.4f} ms is {'INSIDE' if inside else 'OUTSIDE'}",
           f"update pass: {numel} bound elements x 12 bytes = {nbytes / 1e9:.3f} GB; floor at the Adam pass's {ADAM_TBS} TB/s = {floor_ms:.4f} ms",
           f"  (c) - (b) = {c - b:+.4f} ms per step ({(c - b) / floor_ms:.2f} x the floor) — recorded, not gated"
           + ("; MORE THAN TWICE THE FLOOR" if c - b > 2 * floor_ms else ""),
           f"  ema_update_kernel alone                {line(k_us, 'us')}   = {nbytes / (kern_ms * 1e-3) / 1e12:.2f} TB/s achieved",
           f"  one swap (exchange + full weight refresh, host synchronised)   {line(sw)}"]
    print("\n".join(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")
    sys.exit(0 if inside else 2)


if __name__ == "__main__":
    main()
