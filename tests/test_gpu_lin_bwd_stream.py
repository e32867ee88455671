"""The streaming weight / bias gradient of the Linear layers (csrc/lin_bwd.h lin_bwd_stream_kernel) and the backward's weight-gradient queue
(csrc/engine.h wq_add / wq_flush).

Kernel level, through hulc_k_lin_bwd_stream, against fp64 of the SAME device inputs.  16-bit products are exact in fp32, so the only error is the fp32
accumulation: per element |dW - dW64| <= 4 M 2^-24 sum_m |dY||X| + one fp32 ulp of the result (the factor 4 covers the re-association across MFMA k-blocks,
waves and row ranges); the same form for db.  The slab buffer, the padding columns of X and dW and the rows behind dY and X are NaN-filled, so a slab cell
that is added to instead of stored, or an operand byte fetched from outside the matrix, leaves a NaN in the result.

Step level: the tensors and the two gates of tests/test_gpu_fullsize.py::test_row_split_weight_gradients_at_ragged_row_counts (bf16 against the fp32 engine:
worst <= 0.15, median < 0.03 — the project's gates for this comparison) at row counts on both sides of the one-range / two-range and the queue's M <= 64
thresholds; hulc_backward == hulc_backward_part(0) + (1) and two backward passes of one step, bit for bit in the reproducible mode; and the gradients of
hulc_backward_allreduce on a 1-rank communicator (the bucket must be flushed before it goes on the wire)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import synth_batch  # noqa: E402
from hulc_amd import lib as L  # noqa: E402
from hulc_amd import spec  # noqa: E402
from hulc_amd.engine import StepEngine  # noqa: E402

ROWS = (1, 63, 65, 191, 257, 1030)      # one row; a ring shorter than its depth (1, 2 steps); ranges that end inside a 64-row tile; three ranges of several steps
SHAPES = [(60, 128), (128, 128), (384, 128), (128, 2048), (128, 3136), (2048, 128)]
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _ulp32(x):
    """One fp32 ulp at |x| (x: float64 tensor)."""
    _, e = torch.frexp(x.abs().float().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x, dtype=torch.float32), e - 24).double()


def _inputs(dtype, M, N, K, dev, seed):
    """dY [M][N] dense and X [M][K] at pitch K + 8, both inside buffers with 64 more rows; everything outside the matrices is NaN."""
    g = torch.Generator(device=dev); g.manual_seed(seed)
    ldx = K + 8
    ybuf = torch.full((M + 64, N), float("nan"), device=dev, dtype=TDT[dtype])
    xbuf = torch.full((M + 64, ldx), float("nan"), device=dev, dtype=TDT[dtype])
    ybuf[:M] = torch.randn(M, N, device=dev, generator=g).to(TDT[dtype])
    xbuf[:M, :K] = torch.randn(M, K, device=dev, generator=g).to(TDT[dtype])
    y64, x64 = ybuf[:M].double(), xbuf[:M, :K].double()
    ref = dict(dw=y64.t() @ x64, dw_abs=y64.abs().t() @ x64.abs(), db=y64.sum(0), db_abs=y64.abs().sum(0))
    return ybuf, xbuf, ldx, ref


@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_stream_kernel_against_fp64_of_its_inputs(dtype, N, K):
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible — the product path has no CPU fallback")
    dev = torch.device("cuda:0")
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    lddw = K + 4
    g = torch.Generator(device=dev); g.manual_seed(1)
    base_w = torch.randn(N, K, device=dev, generator=g)
    base_b = torch.randn(N, device=dev, generator=g)
    worst = 0.0
    for M in ROWS:
        ybuf, xbuf, ldx, ref = _inputs(dtype, M, N, K, dev, 100 + M)
        tol_w = 4.0 * M * 2.0 ** -24 * ref["dw_abs"]
        tol_b = 4.0 * M * 2.0 ** -24 * ref["db_abs"]
        # (row ranges, slabs): one range writing dW itself; two and three ranges through slabs; and the two other forms the engine launches — one range through a
        # single slab (the decoder heads, re-packed on the way) and two ranges without slabs (fp32 atomics: a job the slab arena has no room for)
        for nsplit, with_slabs in ((1, False), (2, True), (3, True), (1, True), (2, False)):
            for store in (1, 0):
                dw = torch.full((N, lddw), float("nan"), device=dev)
                if not store:
                    dw[:, :K] = base_w
                db = base_b.clone()
                slabs = torch.full((nsplit * N * K,), float("nan"), device=dev)
                L.check(lib.hulc_k_lin_bwd_stream(L.DTYPE[dtype], ybuf.data_ptr(), xbuf.data_ptr(), ldx, M, N, K, nsplit, store, dw.data_ptr(), lddw, db.data_ptr(),
                                                  slabs.data_ptr() if with_slabs else None, st))
                torch.cuda.synchronize()
                what = (dtype, N, K, M, nsplit, with_slabs, store)
                assert torch.isfinite(dw[:, :K]).all() and torch.isfinite(db).all(), what
                assert torch.isnan(dw[:, K:]).all(), what                                     # nothing was written past a row's K columns
                if with_slabs:
                    assert torch.isfinite(slabs).all(), what                                  # every slab cell was stored (empty row ranges included)
                else:
                    assert torch.isnan(slabs).all(), what
                want_w = ref["dw"] if store else ref["dw"] + base_w.double()
                want_b = ref["db"] + base_b.double()
                ew = (dw[:, :K].double() - want_w).abs() - (tol_w + _ulp32(want_w))
                eb = (db.double() - want_b).abs() - (tol_b + _ulp32(want_b))
                print(f"[lin_bwd_stream {dtype} N={N} K={K} M={M} nsplit={nsplit} slabs={int(with_slabs)} store={store}] max |err| / bound: dW "
                      f"{float(((dw[:, :K].double() - want_w).abs() / (tol_w + _ulp32(want_w))).max()):.3f}, db {float(((db.double() - want_b).abs() / (tol_b + _ulp32(want_b))).max()):.3f}")
                worst = max(worst, float(((dw[:, :K].double() - want_w).abs() / (tol_w + _ulp32(want_w))).max()))
                assert float(ew.max()) <= 0.0, (what, float(ew.max()))
                assert float(eb.max()) <= 0.0, (what, float(eb.max()))
    assert worst > 0.0      # (the comparison saw rounding at all: the result is not the reference itself)


def test_stream_entry_refuses_what_the_dma_cannot_fetch():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible — the product path has no CPU fallback")
    dev = torch.device("cuda:0")
    lib = L.load()
    y = torch.zeros(8, 64, device=dev, dtype=torch.bfloat16)
    x = torch.zeros(8, 136, device=dev, dtype=torch.bfloat16)
    dw = torch.zeros(64, 128, device=dev)
    a = (L.DTYPE["bf16"], y.data_ptr(), x.data_ptr())
    assert lib.hulc_k_lin_bwd_stream(*a, 134, 8, 64, 128, 1, 1, dw.data_ptr(), 128, None, None, None) != 0           # pitch 134: every second row starts 4-byte aligned only
    assert b"8-byte aligned" in lib.hulc_last_error()
    assert lib.hulc_k_lin_bwd_stream(*a, 136, 8, 62, 128, 1, 1, dw.data_ptr(), 128, None, None, None) != 0           # the same for dY (N = 62)
    assert b"8-byte aligned" in lib.hulc_last_error()
    assert lib.hulc_k_lin_bwd_stream(*a, 136, 8, 64, 128, 2, 1, dw.data_ptr(), 128, None, dw.data_ptr() + 4, None) != 0
    assert b"slab buffer" in lib.hulc_last_error()
    assert lib.hulc_k_lin_bwd_stream(L.DTYPE["fp32"], y.data_ptr(), x.data_ptr(), 136, 8, 64, 128, 1, 1, dw.data_ptr(), 128, None, None, None) != 0
    assert b"not a 16-bit type" in lib.hulc_last_error()


# ------------------------------------------------------------------------------------------------------------------ step level
_DIMS = dict(kind="hulc", max_window=32, use_clip=False)
_PARAMS = {}


def _engine(dtype, B, S, repro=False):
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible — the product path has no CPU fallback")
    dims = spec.ModelDims(**_DIMS)
    if "p" not in _PARAMS:
        _PARAMS["p"] = spec.init_all(dims, seed=0, ln_jitter=True)
    eng = StepEngine(dims, B, S, dtype=dtype, device="cuda:0", dropout_p=0.0, seed=3)
    eng.load_numpy(_PARAMS["p"])
    if repro:
        eng.set_option("reproducible", 1)
    return eng, dims


def _batch(B, S, seed=5):
    dev = torch.device("cuda:0")
    mb = synth_batch(B, S, dev, seed=seed)
    g = torch.Generator(device=dev); g.manual_seed(3)
    mb["plan_idx"] = torch.randint(0, 32, (B, 32), device=dev, generator=g, dtype=torch.int32)
    return mb


def _step(eng, mb, backward):
    eng.zero_grads()
    eng.forward_loss(mb, False, 1.0, 3.0, step=0)
    backward(eng)
    torch.cuda.synchronize()
    return eng.flat_grads.clone()


ROW_SPLIT = ("fc1.0.", "fc2.", "conv_model.7.", "self_attn.in_proj", "self_attn.out_proj", ".linear1.", ".linear2.", "mean_fc", "log_scale_fc", "prob_fc", "gripper_fc")


@pytest.mark.parametrize("Bb,Ss", [(9, 32), (11, 30), (4, 8)])
def test_queued_weight_gradients_track_the_fp32_engine(Bb, Ss):
    """288 / 330 rows: the heads and the transformer's Linears in one range that ends inside a 64-row tile, the encoder tails in two; 32 rows: every job of the
    queue in the one-step launch."""
    mb = _batch(Bb, Ss)
    grads = {}
    for dtype in ("fp32", "bf16"):
        eng, dims = _engine(dtype, Bb, Ss)
        grads[dtype] = _step(eng, mb, lambda e: e.backward())
        eng.close()
    lay, _ = spec.layout(dims)
    worst = {}
    for name, (off, shape) in lay.items():
        if not any(s in name for s in ROW_SPLIT) or "rgb_static_encoder.conv_model.7" in name:
            continue
        n = int(np.prod(shape))
        a, b = grads["bf16"][off:off + n].double(), grads["fp32"][off:off + n].double()
        assert torch.isfinite(a).all(), name
        worst[name] = ((a - b).norm() / (b.norm() + 1e-30)).item()
    assert len(worst) >= 30, sorted(worst)
    top = sorted(worst.items(), key=lambda kv: -kv[1])
    print(f"[weight-gradient queue, B*S = {Bb * Ss}] worst tensors:", [(k, round(v, 4)) for k, v in top[:4]], "median", round(float(np.median(list(worst.values()))), 4))
    bad = {k: v for k, v in worst.items() if v > 0.15}
    assert not bad, bad
    assert np.median(list(worst.values())) < 0.03, top[:5]


def test_backward_in_two_parts_leaves_the_same_buffer():
    B, S = 4, 8
    mb = _batch(B, S, seed=7)
    eng, _ = _engine("bf16", B, S, repro=True)
    whole = _step(eng, mb, lambda e: e.backward())

    def parts(e):
        e.backward(0)
        e.backward(1)
    split = _step(eng, mb, parts)
    eng.close()
    assert float(whole.abs().max()) > 0 and torch.isfinite(whole).all()
    assert torch.equal(whole.view(torch.int32), split.view(torch.int32)), int((whole != split).sum())


def test_reproducible_backward_repeats_at_a_ragged_row_count():
    B, S = 9, 32
    mb = _batch(B, S, seed=7)
    eng, _ = _engine("bf16", B, S, repro=True)
    a = _step(eng, mb, lambda e: e.backward())
    b = _step(eng, mb, lambda e: e.backward())
    assert eng.get_option("nondeterministic_sites") == 0
    eng.close()
    assert float(a.abs().max()) > 0 and torch.isfinite(a).all()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), int((a != b).sum())


def test_one_rank_allreduce_sends_flushed_buckets():
    """hulc_backward_allreduce on a 1-rank communicator: the SUM over one rank is the identity, so with fp32 buckets the buffer must equal hulc_backward's.  That
    alone does not pin the flush-before-bucket rule (a gradient enqueued behind its bucket lands in the same buffer with the same value), so the step is repeated
    with bf16 buckets: a bucket is narrowed to bf16, reduced and widened back, so every element that was final when its bucket was sent comes back as the bf16
    rounding of hulc_backward's value, and one written behind its bucket keeps fp32 bits."""
    B, S = 4, 8
    mb = _batch(B, S, seed=7)
    eng, dims = _engine("bf16", B, S, repro=True)
    plain = _step(eng, mb, lambda e: e.backward())
    eng.comm_init(eng.comm_unique_id(), 0, 1)
    try:
        reduced = _step(eng, mb, lambda e: e.backward_allreduce("fp32"))
        narrowed = _step(eng, mb, lambda e: e.backward_allreduce("bf16"))
    finally:
        eng.comm_destroy()
    eng.close()
    lay, _ = spec.layout(dims)
    queued = [n for n in lay if any(s in n for s in ROW_SPLIT + ("plan_proposal.", "visual_goal.", "plan_recognition.fc"))]
    assert len(queued) >= 40, len(queued)
    for n in queued:
        off, shape = lay[n]
        k = int(np.prod(shape)) if len(shape) else 1
        assert torch.equal(plain[off:off + k].view(torch.int32), reduced[off:off + k].view(torch.int32)), n
    assert torch.equal(plain.view(torch.int32), reduced.view(torch.int32))
    want = plain.bfloat16().float()
    assert not torch.equal(want, plain)                                               # (the rounding is visible at all)
    for n in queued:
        off, shape = lay[n]
        k = int(np.prod(shape)) if len(shape) else 1
        assert torch.equal(want[off:off + k].view(torch.int32), narrowed[off:off + k].view(torch.int32)), n
