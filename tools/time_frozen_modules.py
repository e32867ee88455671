"""What freezing the perceptual encoders saves per training step on one MI355X, and what the trainable mask costs a run that freezes nothing.

    python tools/time_frozen_modules.py --parent PARENT_BUILD.so [--B 64] [--S 32] [--dtype bf16] [--rounds 3] [--steps 30] [--out profiles/frozen_modules.txt]

Three cases, each the paired pass of a step (B visual + B language windows x S frames: forward + loss + backward + AdamW), median ms per step:
  (a) the parent commit's build of the library (HULC_LIB_PATH, hulc_amd/lib.py; tools/ab_lib.sh builds one) — measured as TWO independent series a1, a2;
  (b) this tree's build with nothing frozen (hulc_trainable_set never called);
  (c) this tree's build with every perceptual_encoder.* tensor frozen.
The project has no run-time switch between builds, so every sample is a fresh child process: a1, b, a2, c alternate for `rounds` rounds, each child warms up,
then times `steps` steps between two device synchronisations, five times, and reports the five figures.  The spread of the two (a) series is the margin: (b)
passes when its median lies inside [min, max] over both.  (c) is recorded, not gated.  A child that fails ends the run.  Before timing, a child of (c) checks
on its own seeded inputs that the frozen tensors kept their bits and the others moved."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sample(a):
    import torch

    from bench import synth_batch
    from hulc_amd import spec
    from hulc_amd.engine import StepEngine
    dev = torch.device("cuda:0")
    dims = spec.ModelDims(kind="hulc", max_window=32, use_clip=True)
    eng = StepEngine(dims, 2 * a.B, a.S, dtype=a.dtype, dropout_p=0.1, device="cuda:0", seed=1)
    eng.load_numpy(spec.init_all(dims, seed=0))
    mv, ml = synth_batch(a.B, a.S, dev, 1, False), synth_batch(a.B, a.S, dev, 2, True)
    enc = [n for n in eng.layout if n.startswith("perceptual_encoder.")]
    if a.freeze:
        eng.set_trainable({n: False for n in enc})
    p0 = eng.flat_params.clone()

    def step(i):
        eng.zero_grads()
        eng.forward_loss_pair(mv, ml, 0.5, 3.0, step=i, sync_losses=False)
        eng.backward()
        eng.optimizer_step("adamw", weight_decay=0.01)

    for i in range(5):
        step(i)
    torch.cuda.synchronize()
    k = eng.encoder_numel
    if a.freeze and (not torch.equal(p0[:k], eng.flat_params[:k]) or torch.equal(p0[k:], eng.flat_params[k:])):
        sys.exit("frozen encoders moved, or nothing else did")
    ms = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.steps):
            step(5 + i)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
    eng.close()
    print(json.dumps(ms))


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
    ap.add_argument("--freeze", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.sample:
        return sample(a)
    if not a.parent or not os.path.exists(a.parent):
        sys.exit("--parent PARENT_BUILD.so: the parent commit's build of the library is needed for case (a)")
    parent = os.path.abspath(a.parent)
    sides = [("a1", parent, False), ("b", None, False), ("a2", parent, False), ("c", None, True)]
    ms = {k: [] for k, _, _ in sides}
    for _ in range(a.rounds):
        for k, path, frz in sides:
            env = dict(os.environ)
            env.pop("HULC_LIB_PATH", None)
            if path:
                env["HULC_LIB_PATH"] = path
            cmd = [sys.executable, os.path.abspath(__file__), "--sample", "--B", str(a.B), "--S", str(a.S), "--dtype", a.dtype, "--steps", str(a.steps)] + (["--freeze"] if frz else [])
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit(f"case {k}: the sampling process ended with {r.returncode}\n{r.stdout[-1000:]}{r.stderr[-3000:]}")
            ms[k] += json.loads(r.stdout.strip().splitlines()[-1])

    def line(v):
        v = sorted(v)
        return f"{np.median(v):8.4f} ms   [{v[0]:.4f} .. {v[-1]:.4f}]   n = {len(v)}"
    lo, hi = min(ms["a1"] + ms["a2"]), max(ms["a1"] + ms["a2"])
    b, c, am = float(np.median(ms["b"])), float(np.median(ms["c"])), float(np.median(ms["a1"] + ms["a2"]))
    inside = lo <= b <= hi
    out = [f"frozen modules, one MI355X, {a.dtype}, paired pass of B = {a.B} + {a.B} windows x S = {a.S} frames, forward + loss + backward + AdamW",
           f"ms per step, median [min .. max]; {a.rounds} alternating rounds of fresh processes per case, 5 samples of {a.steps} steps each",
           f"  (a1) parent build                      {line(ms['a1'])}",
           f"  (a2) parent build, second series       {line(ms['a2'])}",
           f"  (b)  this build, nothing frozen        {line(ms['b'])}",
           f"  (c)  this build, encoders frozen       {line(ms['c'])}",
           f"margin = the spread of the two parent series [{lo:.4f} .. {hi:.4f}]: median of (b) {b:.4f} ms is {'INSIDE' if inside else 'OUTSIDE'}",
           f"(c) against the parent median {am:.4f} ms: {c - am:+.4f} ms per step ({100.0 * (c - am) / am:+.1f} %) — recorded, not gated"]
    print("\n".join(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")
    sys.exit(0 if inside else 2)


if __name__ == "__main__":
    main()
