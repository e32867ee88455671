#!/usr/bin/env python
"""Environment steps per second of the rollout, two ways, for n environments in {1, 8, 32, 64} (bf16 engine, HULC, a replan every 30 steps):

  (a) b1_sequential   n sequential calls of the B = 1 hulc_rollout_act per step (the B = 1 context holds ONE environment's state, so this is the
                      device work and host cost of serving n environments one call at a time; the replan is one hulc_rollout_plan per environment)
  (b) envs_batched    one hulc_rollout_envs_act over the n slots per step (one hulc_rollout_envs_plan over all of them at a replan)

One process, both ways alternating on the same device after a warm-up of every shape; each sample is a host clock around `--steps` policy steps (every
call ends in a stream synchronisation inside the library); the medians over `--repeats` samples are reported.  Prints ONE JSON line.

  python tools/time_rollout_envs.py [--ns 1,8,32,64] [--steps 60] [--repeats 5] [--trace-n 32]

--trace-n N: instead of timing, warm up and run exactly ONE hulc_rollout_envs_act at n = N between two marker prints (for a kernel trace of one act).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hulc_amd import spec  # noqa: E402
from hulc_amd.engine import StepEngine  # noqa: E402

REPLAN = 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="1,8,32,64")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace-n", type=int, default=0)
    ap.add_argument("--dtype", default="bf16")
    args = ap.parse_args()
    ns = [int(x) for x in args.ns.split(",")]
    nmax = max(ns + [args.trace_n])
    dims = spec.ModelDims(kind="hulc", max_window=32, use_clip=False)
    eng = StepEngine(dims, nmax, 2, dtype=args.dtype, device="cuda:0", seed=1)
    eng.load_numpy(spec.init_all(dims, seed=1, ln_jitter=True))
    eng.rollout_envs_init(nmax)
    g = torch.Generator(device="cuda").manual_seed(0)
    rs = torch.rand(nmax, 3, 200, 200, device="cuda", generator=g) * 2 - 1
    rg = torch.rand(nmax, 3, 84, 84, device="cuda", generator=g) * 2 - 1
    ro = (torch.rand(nmax, 15, device="cuda", generator=g) - 0.5)
    lang = torch.randn(nmax, 384, device="cuda", generator=g)
    ro_host = ro.cpu().numpy()

    def b1(n, steps):
        for t in range(steps):
            for e in range(n):
                obs = dict(rgb_static=rs[e:e + 1], rgb_gripper=rg[e:e + 1], robot_obs_raw=ro_host[e])
                if t % REPLAN == 0:
                    eng.rollout_plan(obs, lang[e])
                eng.rollout_act(obs)

    def envs(n, steps):
        obs = dict(rgb_static=rs[:n], rgb_gripper=rg[:n], robot_obs_raw=ro[:n])
        for t in range(steps):
            if t % REPLAN == 0:
                eng.rollout_envs_plan(obs, lang[:n])
            eng.rollout_envs_act(obs)

    if args.trace_n:
        n = args.trace_n
        envs(n, 3)
        torch.cuda.synchronize()
        print("TRACE_ACT_BEGIN", flush=True)
        eng.rollout_envs_act(dict(rgb_static=rs[:n], rgb_gripper=rg[:n], robot_obs_raw=ro[:n]))
        torch.cuda.synchronize()
        print("TRACE_ACT_END", flush=True)
        eng.close()
        return

    for n in ns:                                        # warm-up: every shape of the timed window
        b1(n, 2)
        envs(n, 2)
    res = {}
    for n in ns:
        sa, sb = [], []
        for _ in range(args.repeats):                   # alternating
            for fn, dst in ((b1, sa), (envs, sb)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(n, args.steps)
                torch.cuda.synchronize()
                dst.append(time.perf_counter() - t0)
        ma, mb = statistics.median(sa), statistics.median(sb)
        res[str(n)] = dict(b1_sequential_env_steps_per_s=round(n * args.steps / ma, 1), envs_batched_env_steps_per_s=round(n * args.steps / mb, 1),
                           b1_sequential_ms_per_policy_step=round(1e3 * ma / args.steps, 4), envs_batched_ms_per_policy_step=round(1e3 * mb / args.steps, 4),
                           speedup=round(ma / mb, 3), spread_b1=round((max(sa) - min(sa)) / ma, 4), spread_envs=round((max(sb) - min(sb)) / mb, 4))
    eng.close()
    print(json.dumps(dict(tool="time_rollout_envs", dtype=args.dtype, kind="hulc", replan_every=REPLAN, steps=args.steps, repeats=args.repeats,
                          device=torch.cuda.get_device_name(0), n=res)))


if __name__ == "__main__":
    main()
