"""Helpers shared by tests/test_gpu_plan_kernels.py and tests/test_gpu_layernorm.py: device buffers that start at 7.0 with guard elements past the end,
and the per-element comparisons (conventions of tests/test_gpu_encoder_head.py)."""
import numpy as np
import pytest
import torch

from plan_ln_inputs import ACC, ULP, tdt

GUARD = 3          # rows (or elements of a vector) past the end of every output buffer


def load():
    from hulc_amd import lib as L
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    return L, L.load()


def dev(x, dtype="fp32"):
    """x on the device, rounded to the storage type"""
    return torch.from_numpy(np.array(x, dtype=np.float32)).cuda().to(tdt(dtype)).contiguous()


def devi(x):
    return torch.from_numpy(np.array(x, dtype=np.int32)).cuda()


def f64(t):
    return t.float().cpu().numpy().astype(np.float64)


def sevens(shape, dtype="fp32"):
    """an output buffer: `shape` plus GUARD rows, all 7.0"""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return torch.full((shape[0] + GUARD,) + shape[1:], 7.0, device="cuda", dtype=tdt(dtype) if isinstance(dtype, str) else dtype)


def ptr(t):
    return None if t is None else t.data_ptr()


def guard_intact(t, n, what):
    assert (t[n:].float() == 7.0).all(), f"{what}: elements past the end were written"


def refused(lib, rc, entry):
    """the entry returned non-zero and its message names it"""
    msg = lib.hulc_last_error().decode("utf-8", "replace")
    assert rc != 0 and entry in msg, (rc, msg)
    return msg


def check16(got, ref, dtype, what):
    """an output of storage type `dtype`, per element: one ulp of the type + the fp32 accumulation bound (fp32: the bound alone).  -> worst err / tol"""
    ref = np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    tol = ULP[dtype] * np.abs(ref) + ACC * np.abs(ref).max()
    return check_tol(err, tol, got, ref, f"{what} [{dtype}]")


def check32(got, ref, what):
    """an fp32 output of a short sum of products: 2e-5 max|ref|"""
    return check16(got, ref, "fp32", what)


def check_tol(err, tol, got, ref, what):
    """per element err <= tol; elements with tol == 0 must be exact.  -> worst err / tol"""
    tol = np.broadcast_to(tol, err.shape)
    ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"{what}: worst err/tol = {worst:.3g} (max|ref| {float(np.abs(ref).max()) if ref.size else 0.0:.4g})")
    if not (err <= tol).all():
        k = np.unravel_index(np.argmax(ratio), err.shape)
        raise AssertionError(f"{what}: element {k}: got {got[k]!r} ref {ref[k]!r} tol {tol[k]:.3g} ({int((err > tol).sum())} of {err.size} elements off)")
    return worst


def check_rel(got, ref, gate, what):
    """plan_ln_inputs.rel_err against a measured gate.  -> err / gate"""
    from plan_ln_inputs import rel_err
    e = rel_err(got, ref)
    print(f"{what}: rel_err {e:.3g}, gate {gate:.3g}, err/gate = {e / gate:.3g}")
    assert e <= gate, f"{what}: rel_err {e:.4g} above the gate {gate:.4g} ({e / gate:.2f} x)"
    return e / gate
