#!/usr/bin/env python
"""Times of the deterministic decoder's head kernels (csrc/det_head.h) at S*B = 2048 rows in bf16, next to the project's existing GEMM path on the same operands
with the head padded to 16 columns, and the whole training step with each decoder.

  det      hulc_k_det_head_loss (forward + loss + pre-activation gradient) and hulc_k_det_head_bwd (data gradient, weight-gradient slabs and their sum; the
           entry also allocates its slab scratch and synchronises, so its CALL time is an upper bound of the three kernels')
  padded   hulc_k_gemm_epi with the engine's routing (kernel 0): H1 [2048][2048] x W16^T -> fp32 [2048][16] (forward), dpre16 [2048][16] x W16T^T -> bf16
           [2048][2048] (data gradient), and dpre16^T [16][2048] x H1^T [2048][2048] -> fp32 accumulate (weight gradient: the product lin_wgrad issues
           behind its transposes, whose time is NOT counted)
  step     forward + backward + Adam of the hulc workload shape (B = 64 windows per modality as one paired pass, S = 32) with the logistic and with the
           deterministic decoder

Every figure is the median over --repeats samples of a device-event interval around --iters calls (the step: a host clock around calls that end in a
synchronise), after a warm-up of every shape; the two ways alternate in one process.  Kernel-level times come from a kernel trace of `--trace` (one call of each
between two marker prints).  Prints ONE JSON line; with --out FILE also writes the table there.

  python tools/time_det_head.py [--rows 2048] [--iters 50] [--repeats 7] [--steps 10] [--out profiles/det_decoder.txt] [--trace]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hulc_amd import lib as L  # noqa: E402
from hulc_amd import spec  # noqa: E402
from hulc_amd.engine import StepEngine  # noqa: E402
from hulc_amd.utils import synthetic  # noqa: E402

HID = 2048


def event_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq", type=int, default=32)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_det_head.py needs a HIP device: a timing without one says nothing")
    lib = L.load()
    bf = L.DTYPE["bf16"]
    n, S = args.rows, 32
    B = n // S
    g = torch.Generator(device="cuda").manual_seed(0)
    H1 = torch.relu(torch.randn(n, HID, device="cuda", generator=g)).to(torch.bfloat16)
    W16 = torch.zeros(16, HID, device="cuda")
    W16[:7] = torch.randn(7, HID, device="cuda", generator=g) * 0.02
    W16 = W16.to(torch.bfloat16)
    W16T = W16.t().contiguous()
    H1T = H1.t().contiguous()
    bias = torch.zeros(16, device="cuda")
    act = torch.rand(B, S, 7, device="cuda", generator=g) * 2 - 1
    ro = torch.rand(B, S, 15, device="cuda", generator=g) - 0.5
    row_loss, pred, dpre = torch.zeros(n, device="cuda"), torch.zeros(n, 7, device="cuda"), torch.zeros(n, 8, device="cuda")
    dH1, dZ1 = torch.zeros(n, HID, device="cuda", dtype=torch.bfloat16), torch.zeros(B, HID, device="cuda", dtype=torch.bfloat16)
    dW, db = torch.zeros(7, HID, device="cuda"), torch.zeros(7, device="cuda")
    heads16 = torch.zeros(n, 16, device="cuda")
    dpre16 = torch.zeros(n, 16, device="cuda", dtype=torch.bfloat16)
    dpre16T = torch.zeros(16, n, device="cuda", dtype=torch.bfloat16)
    dW16 = torch.zeros(16, HID, device="cuda")
    p = lambda t: t.data_ptr()

    def det_fwd():
        L.check(lib.hulc_k_det_head_loss(bf, p(H1), p(W16), p(bias), p(act), p(ro), B, S, 0, 0, 1.0 / n, None, p(row_loss), p(pred), p(dpre), None))

    def det_bwd():
        L.check(lib.hulc_k_det_head_bwd(bf, p(dpre), p(W16), p(H1), B, S, p(dH1), p(dZ1), p(dW), p(db), None))

    def job(A, Bm, M, N, K, out, out_f32, accumulate=0):
        return L.HulcGemmEpiJob(A=p(A), B=p(Bm), M=M, N=N, K=K, lda=K, ldb=K, ldc=N, out_R1=0, out_s0=0, nsplit=1, wfrag=0, out=p(out), out_f32=out_f32, accumulate=accumulate,
                                alpha=1.0)

    j_fwd, j_dgrad, j_wgrad = job(H1, W16, n, 16, HID, heads16, 1), job(dpre16, W16T, n, HID, 16, dH1, 0), job(dpre16T, H1T, 16, HID, n, dW16, 1, 1)
    j_fwd.bias = p(bias)
    ran = C.c_int32()

    def pad(j):
        def f():
            L.check(lib.hulc_k_gemm_epi(bf, C.byref(j), 0, C.byref(ran), None))
        return f

    ways = [("det_head_loss (fwd + loss + dpre)", det_fwd), ("padded16 forward GEMM", pad(j_fwd)), ("det_head_bwd call (dgrad + wgrad + sum; incl. scratch alloc + sync)", det_bwd),
            ("padded16 data-gradient GEMM", pad(j_dgrad)), ("padded16 weight-gradient GEMM (transposes not counted)", pad(j_wgrad))]
    for _, f in ways:
        f()
    torch.cuda.synchronize()
    if args.trace:
        print("TRACE-BEGIN", flush=True)
        for _, f in ways:
            f()
        torch.cuda.synchronize()
        print("TRACE-END", flush=True)
        return
    res = {}
    samples = {k: [] for k, _ in ways}
    for _ in range(args.repeats):
        for k, f in ways:
            samples[k].append(event_ms(f, args.iters) * 1e3)
    for k, _ in ways:
        res[k] = dict(us=round(statistics.median(samples[k]), 2), min_us=round(min(samples[k]), 2), max_us=round(max(samples[k]), 2))
    by = dict(fwd=n * HID * 2 + 7 * HID * 2, bwd=n * HID * 2 * 2 + n * HID * 2)          # H1 read (+ W); H1 read twice (mask rows aside) + dH1 written
    res["bytes"] = by

    # ---- the whole step with each decoder (paired pass, fwd + bwd + Adam)
    Bw, Sw = args.batch, args.seq
    batch = synthetic.make_batch(Bw, Bw, Sw, seed=3, edge_frac=0.0, aux_mask="all")
    dev = {sc: {k: (np.nonzero(v)[0].astype(np.int32) if k == "use_for_aux" else torch.from_numpy(v).cuda()) for k, v in mb.items()} for sc, mb in batch.items()}
    for sc in dev:
        if "use_for_aux" in dev[sc]:
            dev[sc]["aux_rows"] = dev[sc].pop("use_for_aux")
    engines = {}
    for name, dims in (("logistic", spec.ModelDims(kind="hulc", use_clip=True)), ("deterministic", spec.ModelDims(kind="hulc", use_clip=True, decoder="deterministic"))):
        eng = StepEngine(dims, 2 * Bw, Sw, dtype="bf16", dropout_p=0.1, seed=1)
        eng.load_numpy(spec.init_all(dims, seed=1, ln_jitter=True))
        engines[name] = eng

    def step(eng, k):
        eng.zero_grads()
        eng.forward_loss_pair(dev["vis"], dev["lang"], 0.5, 3.0, step=k, sync_losses=False)
        eng.backward()
        eng.adam_step()

    for eng in engines.values():
        for k in range(3):
            step(eng, k)
    torch.cuda.synchronize()
    st = {k: [] for k in engines}
    for _ in range(args.repeats):
        for name, eng in engines.items():
            t0 = time.perf_counter()
            for k in range(args.steps):
                step(eng, k)
            torch.cuda.synchronize()
            st[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    for name in engines:
        res[f"step_{name}"] = dict(ms=round(statistics.median(st[name]), 4), min_ms=round(min(st[name]), 4), max_ms=round(max(st[name]), 4))
        engines[name].close()
    res["shape"] = dict(rows=n, batch_per_modality=Bw, seq=Sw, dtype="bf16", iters=args.iters, repeats=args.repeats, steps=args.steps, gemm_ran=int(ran.value))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("Deterministic decoder head: kernel and step times on one MI355X (tools/time_det_head.py; bf16, medians with min / max over the repeats)\n")
            f.write(f"rows S*B = {n}, {args.iters} calls per sample, {args.repeats} samples, the ways alternate in one process\n\n")
            for k, _ in ways:
                f.write(f"  {k:78s} {res[k]['us']:9.2f} us   [{res[k]['min_us']:.2f} .. {res[k]['max_us']:.2f}]\n")
            f.write(f"\n  least bytes: forward {by['fwd'] / 1e6:.2f} MB, backward {by['bwd'] / 1e6:.2f} MB (H1 read by the data and the weight gradient, dH1 written)\n")
            f.write(f"\nwhole step (paired pass of {Bw} + {Bw} windows, S = {Sw}; forward + backward + Adam, host clock over {args.steps} steps ending in a synchronise)\n")
            for name in engines:
                r = res[f"step_{name}"]
                f.write(f"  {name:14s} {r['ms']:9.4f} ms   [{r['min_ms']:.4f} .. {r['max_ms']:.4f}]\n")


if __name__ == "__main__":
    main()
