"""Kernel-level tests of the deterministic decoder's head (hulc_amd/csrc/det_head.h) through its test entries hulc_k_det_head_loss / _bwd / _act, against
the float64 restatement tests/det_head_ref.py on the device's own (rounded) operands.  Conventions of tests/plan_ln_gpu_util.py: outputs start at 7.0 with
guard rows that must survive; 16-bit outputs per element to one ulp + the fp32 accumulation bound (check16); fp32 outputs to 5 x the error of a float32 numpy
evaluation of the same operands (tests/det_head_inputs.py, re-measured on the host by tests/test_det_decoder_host.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import det_head_inputs as I
import det_head_ref as R
from plan_ln_gpu_util import GUARD, check16, check_rel, dev, f64, guard_intact, load, ptr, refused, sevens
from plan_ln_inputs import DTYPES

pytestmark = pytest.mark.gpu


def dev_case(B, S, dtype):
    H1, W, bias, act, ro = I.inputs(B, S)
    return dev(H1, dtype), dev(W, dtype), dev(bias), dev(act), dev(ro)


@pytest.mark.parametrize("frame", I.FRAMES)
@pytest.mark.parametrize("crit", I.CRITERIA)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,S", I.CASES)
def test_det_head_loss(B, S, dtype, crit, frame):
    L, lib = load()
    n = B * S
    H1, W, bias, act, ro = dev_case(B, S, dtype)
    row_loss, pred, dpre = sevens(n), sevens((n, 7)), sevens((n, 8))
    rc = lib.hulc_k_det_head_loss(L.DTYPE[dtype], ptr(H1), ptr(W), ptr(bias), ptr(act), ptr(ro), B, S, crit, frame, I.GRAD_SCALE, None, ptr(row_loss), ptr(pred), ptr(dpre),
                                  None)
    L.check(rc)
    torch.cuda.synchronize()
    for t, what in ((row_loss, "row_loss"), (pred, "pred"), (dpre, "dpre")):
        guard_intact(t, n, what)
    ref = I.reference(B, S, dtype, crit, frame)
    d = np.abs(ref["d"])
    assert (d > 1).any() and (d < 1).any() and (np.abs(ref["pre"]) > 6).any(), "the inputs cover both Huber branches and a saturated prediction"
    g = I.LOSS_GATE[(B, S, dtype, crit, frame)]
    check_rel(f64(row_loss[:n]), ref["row_loss"], g[0], f"row_loss B={B} S={S} crit={crit} frame={frame} [{dtype}]")
    check_rel(f64(pred[:n]).reshape(B, S, 7), I.batch_major(ref["pred"], B, S), g[1], f"pred [{dtype}]")
    got = f64(dpre[:n])
    assert (got[:, 7] == 0).all(), "column 7 of dpre is zero"
    check_rel(got[:, :7], ref["dpre"], g[2], f"dpre [{dtype}]")


@pytest.mark.parametrize("dtype", DTYPES)
def test_det_head_loss_scale_pointer(dtype):
    """the optional device loss scale multiplies dpre only"""
    L, lib = load()
    B, S = 3, 2
    n = B * S
    H1, W, bias, act, ro = dev_case(B, S, dtype)
    outs = []
    for ls in (None, dev(np.array([64.0]))):
        row_loss, pred, dpre = sevens(n), sevens((n, 7)), sevens((n, 8))
        L.check(lib.hulc_k_det_head_loss(L.DTYPE[dtype], ptr(H1), ptr(W), ptr(bias), ptr(act), ptr(ro), B, S, R.HUBER, 0, I.GRAD_SCALE, ptr(ls), ptr(row_loss), ptr(pred),
                                         ptr(dpre), None))
        torch.cuda.synchronize()
        outs.append((row_loss[:n].clone(), pred[:n].clone(), dpre[:n].clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    ref = I.reference(B, S, dtype, R.HUBER, 0)
    check_rel(f64(outs[1][2])[:, :7], 64.0 * ref["dpre"], I.LOSS_GATE[(B, S, dtype, R.HUBER, 0)][2], f"dpre x 64 [{dtype}]")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,S", I.CASES)
def test_det_head_bwd(B, S, dtype):
    L, lib = load()
    n = B * S
    H1, W, _, _, _ = dev_case(B, S, dtype)
    dpre64, (dH1_r, dZ1_r, dW_r, db_r) = I.reference_bwd(B, S, dtype)
    dpre = dev(np.concatenate([dpre64, np.zeros((n, 1))], 1))

    def run():
        dH1, dZ1 = sevens((n, I.HID), dtype), sevens((B, I.HID), dtype)
        dW, db = torch.full((7 + GUARD, I.HID), 7.0, device="cuda"), torch.full((7 + GUARD,), 7.0, device="cuda")
        dW[:7] = I.DW_START
        db[:7] = I.DW_START
        L.check(lib.hulc_k_det_head_bwd(L.DTYPE[dtype], ptr(dpre), ptr(W), ptr(H1), B, S, ptr(dH1), ptr(dZ1), ptr(dW), ptr(db), None))
        torch.cuda.synchronize()
        return dH1, dZ1, dW, db

    dH1, dZ1, dW, db = run()
    guard_intact(dH1, n, "dH1"), guard_intact(dZ1, B, "dZ1"), guard_intact(dW, 7, "dW"), guard_intact(db, 7, "db")
    check16(f64(dH1[:n]), dH1_r, dtype, f"dH1 B={B} S={S}")
    check16(f64(dZ1[:B]), dZ1_r, dtype, f"dZ1 B={B} S={S}")
    assert (f64(dZ1[:B])[f64(H1)[(S - 1) * B:] <= 0] == 0).all(), "dZ1 is zero where H1 is not positive"
    g = I.BWD_GATE[(B, S, dtype)]
    check_rel(f64(dW[:7]), I.DW_START + dW_r, g[0], f"dW (accumulated onto {I.DW_START}) [{dtype}]")
    check_rel(f64(db[:7]), I.DW_START + db_r, g[1], f"db (accumulated onto {I.DW_START}) [{dtype}]")
    again = run()
    assert torch.equal(again[2], dW) and torch.equal(again[3], db), "two runs of the weight gradient give the same bits"
    assert torch.equal(again[0], dH1) and torch.equal(again[1], dZ1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,S", I.CASES)
def test_det_head_act(B, S, dtype):
    """n = B S rows as a rollout sees them (one row per environment): robot_obs and the output are indexed by the row"""
    L, lib = load()
    n = B * S
    H1, W, bias, _, _ = dev_case(B, S, dtype)
    H, Wr, b, _, ro = I.operands(B, S, dtype)
    out = sevens((n, 7))
    L.check(lib.hulc_k_det_head_act(L.DTYPE[dtype], ptr(H1), ptr(W), ptr(bias), ptr(dev(ro)), n, ptr(out), None))
    torch.cuda.synchronize()
    guard_intact(out, n, "actions")
    ref = R.tcp_to_world(R.head(H, Wr, b)[1], ro)
    check_rel(f64(out[:n]), ref, I.LOSS_GATE[(B, S, dtype, R.HUBER, 0)][1], f"actions n={n} [{dtype}]")


def test_det_head_entries_refuse_bad_arguments():
    L, lib = load()
    B, S = 3, 2
    n = B * S
    H1, W, bias, act, ro = dev_case(B, S, "bf16")
    row_loss, pred, dpre = sevens(n), sevens((n, 7)), sevens((n, 8))
    dH1, dZ1, dW, db = sevens((n, I.HID), "bf16"), sevens((B, I.HID), "bf16"), sevens((7, I.HID)), sevens(7)
    bf = L.DTYPE["bf16"]

    def loss(**kw):
        a = dict(dtype=bf, H1=ptr(H1), W=ptr(W), bias=ptr(bias), act=ptr(act), ro=ptr(ro), B=B, S=S, crit=0, frame=0, out=ptr(row_loss), pred=ptr(pred), dpre=ptr(dpre))
        a.update(kw)
        return lib.hulc_k_det_head_loss(a["dtype"], a["H1"], a["W"], a["bias"], a["act"], a["ro"], a["B"], a["S"], a["crit"], a["frame"], 1.0, None, a["out"], a["pred"],
                                        a["dpre"], None)

    for kw in (dict(H1=None), dict(W=None), dict(bias=None), dict(act=None), dict(ro=None), dict(out=None), dict(dpre=None), dict(H1=ptr(H1) + 2), dict(W=ptr(W) + 8),
               dict(dpre=ptr(dpre) + 4), dict(B=0), dict(S=0), dict(B=1 << 12, S=1 << 11), dict(crit=2), dict(frame=2), dict(dtype=7)):
        refused(lib, loss(**kw), "hulc_k_det_head_loss")

    def bwd(**kw):
        a = dict(dtype=bf, dpre=ptr(dpre), W=ptr(W), H1=ptr(H1), B=B, S=S, dH1=ptr(dH1), dZ1=ptr(dZ1), dW=ptr(dW), db=ptr(db))
        a.update(kw)
        return lib.hulc_k_det_head_bwd(a["dtype"], a["dpre"], a["W"], a["H1"], a["B"], a["S"], a["dH1"], a["dZ1"], a["dW"], a["db"], None)

    for kw in (dict(dpre=None), dict(W=None), dict(H1=None), dict(dH1=None), dict(dZ1=None), dict(dW=None), dict(db=None), dict(dH1=ptr(dH1) + 2), dict(dpre=ptr(dpre) + 4),
               dict(B=0), dict(S=-1), dict(B=1 << 12, S=1 << 11), dict(dtype=7)):
        refused(lib, bwd(**kw), "hulc_k_det_head_bwd")

    def act_(**kw):
        a = dict(dtype=bf, h1=ptr(H1), W=ptr(W), bias=ptr(bias), ro=ptr(ro), n=n, out=ptr(pred))
        a.update(kw)
        return lib.hulc_k_det_head_act(a["dtype"], a["h1"], a["W"], a["bias"], a["ro"], a["n"], a["out"], None)

    for kw in (dict(h1=None), dict(W=None), dict(bias=None), dict(ro=None), dict(out=None), dict(h1=ptr(H1) + 2), dict(n=0), dict(n=(1 << 22) + 1), dict(dtype=7)):
        refused(lib, act_(**kw), "hulc_k_det_head_act")
    torch.cuda.synchronize()
    for t, k in ((row_loss, n), (pred, n), (dpre, n), (dH1, n), (dZ1, B), (dW, 7), (db, 7)):
        assert (t.float() == 7.0).all(), "a refused call launched nothing"
