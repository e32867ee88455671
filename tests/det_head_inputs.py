"""Inputs, gates and float32-vs-float64 measurements shared by tests/test_gpu_det_head.py (GPU) and tests/test_det_decoder_host.py (host, which re-measures
every tabulated figure so that no gate rests on a kernel's output).  Inputs come from hulc_amd.utils.portable_rng (fixed seeds, built on the host)."""
import functools

import numpy as np

import det_head_ref as R
from hulc_amd.utils import portable_rng as prng
from plan_ln_inputs import DTYPES, frozen, rel_err, round_t

HID = 2048
# (B, S): a single row; a partial last workgroup of the one-wave-per-row kernels (6 rows, 4 per workgroup); 15 rows (two 8-row workgroups of the data
# gradient); 258 rows: they cross one 256-row slab of the weight gradient
CASES = ((1, 1), (3, 2), (5, 3), (43, 6))
CRITERIA = (R.HUBER, R.MSE)
FRAMES = (0, 1)
GRAD_SCALE = 0.37          # the engine's lw / (S Bm) in spirit; any value that is not 1
DW_START = 0.25            # dW / db start at this value: the weight gradient accumulates


@functools.lru_cache(maxsize=None)
def inputs(B, S):
    """fp32 operands in TIME-MAJOR row order r = t B + b for H1, batch-major (B, S, .) for actions / robot_obs.
    H1: rectified normals (the decoder state is a ReLU output: half of it is exactly zero); row 0 is three times larger, so that some of its pre-activations
    pass |pre| = 6 (a saturated tanh).  W ~ N(0, 0.16^2): pre-activations ~2.5 wide.  actions uniform in [-1, 1], the gripper +-1; the gripper action of every
    third row opposes the prediction (|d| > 1 in both frames), window 0's first position action is small."""
    tag = f"det{B}_{S}"
    n = B * S
    H1 = np.maximum(prng.normal(tag + "h", (n, HID), seed=31).astype(np.float64), 0.0) * 0.5
    H1[0] *= 3.0
    W = prng.normal(tag + "w", (7, HID), seed=32).astype(np.float64) * 0.16
    bias = prng.uniform(tag + "b", (7,), -0.3, 0.3, seed=33).astype(np.float64)
    act = prng.uniform(tag + "a", (B, S, 7), -1.0, 1.0, seed=34).astype(np.float64)
    ro = prng.uniform(tag + "r", (B, S, 15), -1.0, 1.0, seed=35).astype(np.float64)
    ro[..., 3:6] *= 2.5          # tcp euler angles up to +-2.5 rad
    p = np.tanh(H1.astype(np.float32).astype(np.float64) @ W.T + bias)          # time-major
    grip = np.where(p[:, 6] >= 0, 1.0, -1.0)
    grip[::3] *= -1.0
    act[..., 6] = grip.reshape(S, B).T
    act[0, 0, :3] *= 0.1
    return frozen(H1.astype(np.float32), W.astype(np.float32), bias.astype(np.float32), act.astype(np.float32), ro.astype(np.float32))


def time_major(x, B, S):
    """(B, S, k) -> (S B, k), row t B + b"""
    return np.ascontiguousarray(np.swapaxes(x, 0, 1)).reshape(S * B, -1)


def batch_major(x, B, S):
    """(S B, k) time-major -> (B, S, k)"""
    return np.ascontiguousarray(np.swapaxes(x.reshape(S, B, -1), 0, 1))


def operands(B, S, dtype, as_type=np.float64):
    """the case's operands as the device holds them (H1 and W rounded to `dtype`, the rest fp32), time-major rows, in `as_type`"""
    H1, W, bias, act, ro = inputs(B, S)
    return (round_t(H1, dtype).astype(as_type), round_t(W, dtype).astype(as_type), bias.astype(as_type), time_major(act, B, S).astype(as_type),
            time_major(ro, B, S).astype(as_type))


def last_rows(B, S):
    m = np.zeros(B * S, bool)
    m[(S - 1) * B:] = True
    return m


def reference(B, S, dtype, crit, frame, as_type=np.float64):
    H1, W, bias, act, ro = operands(B, S, dtype, as_type)
    return R.loss(H1, W, bias, act, ro, crit, frame, GRAD_SCALE)


def reference_bwd(B, S, dtype, as_type=np.float64):
    """the backward on the float64 dpre of (Huber, frame 0) rounded to fp32 — what the GPU test feeds the kernels"""
    H1, W, bias, act, ro = operands(B, S, dtype, as_type)
    dpre = reference(B, S, dtype, R.HUBER, 0)["dpre"].astype(np.float32).astype(as_type)
    return dpre, R.bwd(dpre, W, H1, last_rows(B, S))


def loss_measure(B, S, dtype, crit, frame):
    """rel_err of the float32 evaluation against float64 on the same rounded operands: (row_loss, pred, dpre)"""
    r64, r32 = reference(B, S, dtype, crit, frame), reference(B, S, dtype, crit, frame, np.float32)
    return tuple(rel_err(r32[k], r64[k]) for k in ("row_loss", "pred", "dpre"))


def bwd_measure(B, S, dtype):
    """(dW, db) likewise, each added to its start value DW_START in the evaluation's own precision (the kernel accumulates into fp32)"""
    (_, r64), (_, r32) = reference_bwd(B, S, dtype), reference_bwd(B, S, dtype, np.float32)
    return tuple(rel_err(np.float32(DW_START) + r32[k], DW_START + r64[k]) for k in (2, 3))


# measured float32-vs-float64 error per case, rounded up by at most a tenth; the gate is 5 x (tests/test_det_decoder_host.py re-measures).
# key (B, S, dtype, criterion, frame) -> (row_loss, pred, dpre)
LOSS_F32 = {
    (1, 1, "bf16", 0, 0): (5.87e-08, 3.28e-07, 1.31e-06),          # measured 5.865e-08, 3.276e-07, 1.308e-06
    (1, 1, "bf16", 0, 1): (1.24e-06, 3.28e-07, 1.4e-06),          # measured 1.240e-06, 3.276e-07, 1.392e-06
    (1, 1, "bf16", 1, 0): (6.63e-09, 3.28e-07, 1.28e-06),          # measured 6.625e-09, 3.276e-07, 1.274e-06
    (1, 1, "bf16", 1, 1): (1.12e-06, 3.28e-07, 2.76e-06),          # measured 1.114e-06, 3.276e-07, 2.758e-06
    (1, 1, "fp16", 0, 0): (9.32e-08, 1.71e-07, 1.08e-06),          # measured 9.317e-08, 1.707e-07, 1.073e-06
    (1, 1, "fp16", 0, 1): (1.31e-06, 1.71e-07, 1.06e-06),          # measured 1.307e-06, 1.707e-07, 1.052e-06
    (1, 1, "fp16", 1, 0): (5.31e-08, 1.71e-07, 1.05e-06),          # measured 5.302e-08, 1.707e-07, 1.045e-06
    (1, 1, "fp16", 1, 1): (1.25e-06, 1.71e-07, 4.21e-07),          # measured 1.249e-06, 1.707e-07, 4.209e-07
    (1, 1, "fp32", 0, 0): (9.82e-08, 2.99e-07, 1.84e-06),          # measured 9.812e-08, 2.988e-07, 1.832e-06
    (1, 1, "fp32", 0, 1): (1.3e-06, 2.99e-07, 1.9e-06),          # measured 1.295e-06, 2.988e-07, 1.895e-06
    (1, 1, "fp32", 1, 0): (1.05e-07, 2.99e-07, 1.79e-06),          # measured 1.045e-07, 2.988e-07, 1.784e-06
    (1, 1, "fp32", 1, 1): (1.33e-06, 2.99e-07, 3.09e-06),          # measured 1.329e-06, 2.988e-07, 3.087e-06
    (3, 2, "bf16", 0, 0): (9.17e-08, 1.4e-05, 3.2e-06),          # measured 9.169e-08, 1.395e-05, 3.194e-06
    (3, 2, "bf16", 0, 1): (4.12e-06, 1.4e-05, 5.4e-05),          # measured 4.113e-06, 1.395e-05, 5.396e-05
    (3, 2, "bf16", 1, 0): (1.76e-07, 1.4e-05, 3.19e-06),          # measured 1.751e-07, 1.395e-05, 3.184e-06
    (3, 2, "bf16", 1, 1): (5.03e-06, 1.4e-05, 5.4e-05),          # measured 5.021e-06, 1.395e-05, 5.396e-05
    (3, 2, "fp16", 0, 0): (1.24e-07, 2.05e-05, 1.36e-06),          # measured 1.233e-07, 2.042e-05, 1.356e-06
    (3, 2, "fp16", 0, 1): (4.23e-06, 2.05e-05, 5.47e-05),          # measured 4.221e-06, 2.042e-05, 5.464e-05
    (3, 2, "fp16", 1, 0): (1.3e-07, 2.05e-05, 1.33e-06),          # measured 1.290e-07, 2.042e-05, 1.327e-06
    (3, 2, "fp16", 1, 1): (5.23e-06, 2.05e-05, 5.47e-05),          # measured 5.220e-06, 2.042e-05, 5.464e-05
    (3, 2, "fp32", 0, 0): (8.84e-08, 3.23e-05, 5.41e-06),          # measured 8.830e-08, 3.221e-05, 5.405e-06
    (3, 2, "fp32", 0, 1): (4.05e-06, 3.23e-05, 5.38e-05),          # measured 4.047e-06, 3.221e-05, 5.379e-05
    (3, 2, "fp32", 1, 0): (5.52e-08, 3.23e-05, 5.39e-06),          # measured 5.520e-08, 3.221e-05, 5.389e-06
    (3, 2, "fp32", 1, 1): (5.01e-06, 3.23e-05, 5.38e-05),          # measured 5.000e-06, 3.221e-05, 5.379e-05
    (5, 3, "bf16", 0, 0): (1.71e-07, 1.94e-05, 2.06e-06),          # measured 1.702e-07, 1.931e-05, 2.058e-06
    (5, 3, "bf16", 0, 1): (5.25e-06, 1.94e-05, 0.000297),          # measured 5.243e-06, 1.931e-05, 2.964e-04
    (5, 3, "bf16", 1, 0): (1.8e-07, 1.94e-05, 2.02e-06),          # measured 1.796e-07, 1.931e-05, 2.015e-06
    (5, 3, "bf16", 1, 1): (6.8e-06, 1.94e-05, 0.000292),          # measured 6.794e-06, 1.931e-05, 2.918e-04
    (5, 3, "fp16", 0, 0): (3.16e-07, 2.2e-05, 2.7e-06),          # measured 3.151e-07, 2.199e-05, 2.691e-06
    (5, 3, "fp16", 0, 1): (5.41e-06, 2.2e-05, 0.000193),          # measured 5.401e-06, 2.199e-05, 1.926e-04
    (5, 3, "fp16", 1, 0): (2.51e-07, 2.2e-05, 2.69e-06),          # measured 2.503e-07, 2.199e-05, 2.685e-06
    (5, 3, "fp16", 1, 1): (7e-06, 2.2e-05, 0.000191),          # measured 7.000e-06, 2.199e-05, 1.907e-04
    (5, 3, "fp32", 0, 0): (2.83e-07, 2.88e-05, 9.16e-06),          # measured 2.827e-07, 2.871e-05, 9.157e-06
    (5, 3, "fp32", 0, 1): (5.38e-06, 2.88e-05, 0.00019),          # measured 5.370e-06, 2.871e-05, 1.899e-04
    (5, 3, "fp32", 1, 0): (1.57e-07, 2.88e-05, 8.98e-06),          # measured 1.567e-07, 2.871e-05, 8.978e-06
    (5, 3, "fp32", 1, 1): (6.79e-06, 2.88e-05, 0.000188),          # measured 6.784e-06, 2.871e-05, 1.879e-04
    (43, 6, "bf16", 0, 0): (2.21e-07, 0.000436, 2.46e-05),          # measured 2.202e-07, 4.359e-04, 2.460e-05
    (43, 6, "bf16", 0, 1): (1.37e-05, 0.000436, 0.00049),          # measured 1.364e-05, 4.359e-04, 4.894e-04
    (43, 6, "bf16", 1, 0): (2.78e-07, 0.000436, 2.35e-05),          # measured 2.775e-07, 4.359e-04, 2.345e-05
    (43, 6, "bf16", 1, 1): (1.4e-05, 0.000436, 0.000465),          # measured 1.395e-05, 4.359e-04, 4.647e-04
    (43, 6, "fp16", 0, 0): (9.32e-07, 0.00116, 2.15e-05),          # measured 9.319e-07, 1.153e-03, 2.142e-05
    (43, 6, "fp16", 0, 1): (1.39e-05, 0.00116, 0.000551),          # measured 1.382e-05, 1.153e-03, 5.505e-04
    (43, 6, "fp16", 1, 0): (9.25e-07, 0.00116, 2.09e-05),          # measured 9.244e-07, 1.153e-03, 2.085e-05
    (43, 6, "fp16", 1, 1): (1.42e-05, 0.00116, 0.00052),          # measured 1.414e-05, 1.153e-03, 5.197e-04
    (43, 6, "fp32", 0, 0): (7.94e-07, 0.00169, 4.08e-05),          # measured 7.930e-07, 1.685e-03, 4.077e-05
    (43, 6, "fp32", 0, 1): (1.39e-05, 0.00169, 0.000514),          # measured 1.382e-05, 1.685e-03, 5.139e-04
    (43, 6, "fp32", 1, 0): (7.92e-07, 0.00169, 3.97e-05),          # measured 7.911e-07, 1.685e-03, 3.963e-05
    (43, 6, "fp32", 1, 1): (1.42e-05, 0.00169, 0.000487),          # measured 1.412e-05, 1.685e-03, 4.863e-04
}
# key (B, S, dtype) -> (dW, db)
BWD_F32 = {
    (1, 1, "bf16"): (5.96e-08, 5.58e-08),          # measured 5.950e-08, 5.573e-08
    (1, 1, "fp16"): (5.95e-08, 5.17e-08),          # measured 5.946e-08, 5.168e-08
    (1, 1, "fp32"): (5.96e-08, 5.39e-08),          # measured 5.950e-08, 5.380e-08
    (3, 2, "bf16"): (6.4e-08, 3.01e-08),          # measured 6.397e-08, 3.000e-08
    (3, 2, "fp16"): (6.65e-08, 5.08e-08),          # measured 6.642e-08, 5.076e-08
    (3, 2, "fp32"): (6.79e-08, 5.67e-08),          # measured 6.784e-08, 5.668e-08
    (5, 3, "bf16"): (9.68e-08, 6.31e-08),          # measured 9.671e-08, 6.303e-08
    (5, 3, "fp16"): (1.19e-07, 6.67e-08),          # measured 1.187e-07, 6.668e-08
    (5, 3, "fp32"): (1.04e-07, 4.77e-08),          # measured 1.036e-07, 4.760e-08
    (43, 6, "bf16"): (6.36e-05, 9.74e-07),          # measured 6.354e-05, 9.737e-07
    (43, 6, "fp16"): (8.13e-05, 6.24e-07),          # measured 8.129e-05, 6.236e-07
    (43, 6, "fp32"): (8.63e-05, 8.11e-07),          # measured 8.627e-05, 8.101e-07
}
LOSS_GATE = {k: tuple(5 * x for x in v) for k, v in LOSS_F32.items()}
BWD_GATE = {k: tuple(5 * x for x in v) for k, v in BWD_F32.items()}
