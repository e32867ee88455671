"""Step and rollout times of the two decoder bodies on one MI355X: action_decoder.rnn_model = rnn_decoder (the two 2048-wide recurrences) against
mlp_decoder (three feed-forward layers, hulc_decoder_body_select).

    python tools/time_mlp_decoder.py [--B 64] [--S 32] [--dtype bf16] [--rounds 6] [--steps 20]
    python tools/time_mlp_decoder.py --rollout-ab OTHER_BUILD.so [--dtype bf16] [--rounds 6]

Training step: one modality pass of B windows x S frames (forward + loss + backward + Adam), host clock over `steps` steps ending in a synchronise, the two
bodies alternating for `rounds` rounds in one process; then the engine's own timers (hulc_timers_enable) of one step per body: the decoder's kernel classes.
Batched rollout: hulc_rollout_envs_act at n = 1, 16, 64 for both bodies, each through its row kernels (rollout_step.h; the feed-forward body runs their
recurrence-free forms, four launches).

--rollout-ab: the feed-forward body's hulc_rollout_envs_act in this tree's build against ANOTHER build of the library (HULC_LIB_PATH, hulc_amd/lib.py; see
tools/ab_lib.sh) — the way the row kernels were measured against dec_fwd composed at B = n, S = 1 (a build whose hulc_rollout_envs_act routes this body there).
The project has no run-time routing switch, so the two sides are two builds: one fresh child process per build and round, alternating; a child that fails
ends the run."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import synth_batch  # noqa: E402
from hulc_amd import spec  # noqa: E402
from hulc_amd.engine import StepEngine  # noqa: E402


def engine(body, B, S, dtype):
    dims = spec.ModelDims(kind="hulc", max_window=32, use_clip=False, decoder_body=body)
    eng = StepEngine(dims, B, S, dtype=dtype, dropout_p=0.1, device="cuda:0", seed=1)
    eng.load_numpy(spec.init_all(dims, seed=0))
    return eng


def step(eng, mb):
    eng.zero_grads()
    eng.forward_loss(mb, False, 1.0, 0.0, step=0)
    eng.backward()
    eng.adam_step()


def stats(v):
    v = sorted(v)
    return f"{np.median(v):8.4f} ms   [{v[0]:.4f} .. {v[-1]:.4f}]"


def rollout_us(engs, mb, n, rounds, dev):
    """us per hulc_rollout_envs_act call at n rows: `rounds` samples of 20 calls per engine, the engines alternating"""
    obs = dict(rgb_static=mb["rgb_static"][:n, 0].contiguous(), rgb_gripper=mb["rgb_gripper"][:n, 0].contiguous(), robot_obs_raw=mb["robot_obs"][:n, 0].contiguous())
    lang = torch.randn(n, 384, device=dev)
    us = {b: [] for b in engs}
    for eng in engs.values():
        eng.rollout_envs_init(n)
        eng.rollout_envs_plan(obs, lang)
        for _ in range(3):
            eng.rollout_envs_act(obs)
    for _ in range(rounds):
        for b, eng in engs.items():
            t0 = time.perf_counter()
            for _ in range(20):
                eng.rollout_envs_act(obs)
            us[b].append((time.perf_counter() - t0) * 1e6 / 20)
    return us


def rollout_sample(a):
    """child of --rollout-ab: one JSON line {n: median us per call} for the feed-forward body with whatever build HULC_LIB_PATH names"""
    dev = torch.device("cuda:0")
    mb = synth_batch(64, 2, dev, 1, False)
    eng = engine("mlp", 64, 2, a.dtype)
    out = {n: float(np.median(rollout_us({"mlp": eng}, mb, n, 5, dev)["mlp"])) for n in (1, 16, 64)}
    eng.close()
    print(json.dumps(out))


def rollout_ab(a):
    other = os.path.abspath(a.rollout_ab)
    sides = {"this build": None, "other build": other}
    us = {k: {n: [] for n in ("1", "16", "64")} for k in sides}
    for _ in range(a.rounds):
        for k, path in sides.items():
            env = dict(os.environ)
            env.pop("HULC_LIB_PATH", None)
            if path:
                env["HULC_LIB_PATH"] = path
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--rollout-sample", "--dtype", a.dtype], env=env, capture_output=True, text=True, timeout=120)
            if r.returncode != 0:
                sys.exit(f"{k}: the sampling process ended with {r.returncode}\n{r.stderr[-2000:]}")
            d = json.loads(r.stdout.strip().splitlines()[-1])
            for n in us[k]:
                us[k][n].append(d[n])
    print(f"hulc_rollout_envs_act, feed-forward body, {a.dtype}, us per call: median [min .. max] over {a.rounds} alternating processes per build (each: median of 5 x 20 calls)")
    print(f"  other build = {a.rollout_ab}")
    for n in ("1", "16", "64"):
        for k in sides:
            v = sorted(us[k][n])
            print(f"  n = {int(n):2d}  {k:11s}  {np.median(v):8.1f} us   [{v[0]:.1f} .. {v[-1]:.1f}]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--S", type=int, default=32)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rollout-ab", default=None, metavar="OTHER_BUILD.so")
    ap.add_argument("--rollout-sample", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.rollout_sample:
        return rollout_sample(a)
    if a.rollout_ab:
        return rollout_ab(a)
    dev = torch.device("cuda:0")
    mb = synth_batch(a.B, a.S, dev, 1, False)
    engs = {b: engine(b, a.B, a.S, a.dtype) for b in ("rnn", "mlp")}
    print(f"decoder bodies, one MI355X, {a.dtype}, B = {a.B} windows x S = {a.S} frames, one modality pass; {a.rounds} alternating rounds of {a.steps} steps")
    print(f"  workspace: rnn {engs['rnn'].workspace_bytes() / 2**20:.0f} MiB, mlp {engs['mlp'].workspace_bytes() / 2**20:.0f} MiB")
    for eng in engs.values():
        for _ in range(5):
            step(eng, mb)
    torch.cuda.synchronize()
    ms = {b: [] for b in engs}
    for _ in range(a.rounds):
        for b, eng in engs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step(eng, mb)
            torch.cuda.synchronize()
            ms[b].append((time.perf_counter() - t0) * 1e3 / a.steps)
    print("whole step (forward + loss + backward + Adam), ms per step: median [min .. max]")
    for b in engs:
        print(f"  {b}   {stats(ms[b])}")
    print("kernel classes of one step (the engine's timers; us, launches)")
    for b, eng in engs.items():
        eng.timers_enable(True)
        step(eng, mb)
        torch.cuda.synchronize()
        t = eng.timers_read()
        eng.timers_enable(False)
        rows = t.get("timers", t) if isinstance(t, dict) else t
        print(f"  {b}:")
        if isinstance(rows, dict):
            for k, v in sorted(rows.items()):
                print(f"     {k:28s} {v}")
        else:
            for r in rows:
                print(f"     {r}")
    # ---- batched rollout
    print("hulc_rollout_envs_act, us per call: median [min .. max] over the rounds (20 calls each)")
    for n in (1, 16, 64):
        us = rollout_us(engs, mb, n, a.rounds, dev)
        for b in engs:
            v = sorted(us[b])
            print(f"  n = {n:2d}  {b}   {np.median(v):8.1f} us   [{v[0]:.1f} .. {v[-1]:.1f}]")
    for eng in engs.values():
        eng.close()


if __name__ == "__main__":
    main()
