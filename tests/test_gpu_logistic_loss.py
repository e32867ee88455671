"""GPU (-m gpu): the action-loss kernels alone through hulc_k_logistic_loss — logistic_loss_wide_kernel<T> (one lane per mixture component, the 16-bit engines'
kernel) for T = float, bf16 and fp16, and the serial logistic_loss_kernel<float, 10> as the anchor — per row and per dimension against float64
(tests/enc_head_ref.py) on inputs that take every branch of the loss (tests/enc_head_inputs.py: ll_inputs).

Gates.  row_loss and float dheads: 4 x what the reference formulas lose in numpy float32 against float64 on these inputs, per column group, measured as
|error| / (|ref| + 1e-3 max|ref|) (enc_head_inputs.LL_F32 / LL_GATE: row_loss 2.9e-6 -> 1.16e-5, d logits 8.0e-5 -> 3.2e-4, d means 4.1e-5 -> 1.64e-4,
d log-scales 9.2e-5 -> 3.68e-4, d gripper 1.25e-6 -> 5e-6; re-measured by tests/test_enc_head_ref_host.py, which also checks on the host that float32 and
float64 take the same branch in every component).  16-bit dheads: the same plus one ulp of the storage type (2^-7 bf16, 2^-10 fp16; below fp16's normal
range its absolute step 2^-24).  a_tcp_out: 3e-4 against the float64 frame change, the project's bound for the fp32 one; with gripper_control the loss is then
checked from the device's own a_tcp_out."""
import numpy as np
import pytest

import enc_head_inputs as I
import enc_head_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 2
LSCALE = 128.0
# (gripper_control, discrete_gripper, lscale given)
VARIANTS = {"plain": (0, 1, False), "tcp_scaled": (1, 1, True), "mcil_heads_scaled": (0, 0, True), "tcp_mcil_heads": (1, 0, False)}
# (T of dheads, wide)
KERNELS = {"serial_f32": ("fp32", 0), "wide_f32": ("fp32", 1), "wide_bf16": ("bf16", 1), "wide_fp16": ("fp16", 1)}
TD = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _lib():
    from hulc_amd import lib as L
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    return L, L.load()


def pack_heads(inp, discrete):
    """[S*B][LDH] fp32, time-major rows r = t * B + b; pad columns hold 7.0 (the kernels must not read them)"""
    B, S = inp["logits"].shape[:2]
    h = np.full((B, S, I.LDH), 7.0, np.float32)
    NO = I.NMIX * I.NDIM
    h[..., :NO] = inp["logits"].reshape(B, S, NO)
    h[..., NO:2 * NO] = inp["means"].reshape(B, S, NO)
    h[..., 2 * NO:3 * NO] = inp["lsr"].reshape(B, S, NO)
    if discrete:
        h[..., 3 * NO:3 * NO + 2] = inp["grip"]
    return np.ascontiguousarray(h.transpose(1, 0, 2).reshape(S * B, I.LDH))


def run(B, S, variant, kernel):
    """-> row_loss (B, S, 8), a_tcp_out (B, S, 7), dheads (B, S, LDH) as float64, guard rows checked"""
    L, lib = _lib()
    gc, disc, scaled = VARIANTS[variant]
    T, wide = KERNELS[kernel]
    inp = I.ll_inputs(B, S, gc)
    SB = S * B
    heads = torch.from_numpy(pack_heads(inp, disc)).cuda()
    act, ro = torch.from_numpy(inp["actions"].copy()).cuda(), torch.from_numpy(inp["robot_obs"].copy()).cuda()
    row_loss = torch.full((SB + GUARD, 8), 7.0, device="cuda")
    a_tcp = torch.full((SB + GUARD, 7), 7.0, device="cuda")
    dheads = torch.full((SB + GUARD, I.LDH), 7.0, device="cuda", dtype=TD[T])
    lscale = torch.tensor([LSCALE], device="cuda") if scaled else None
    L.check(lib.hulc_k_logistic_loss(L.DTYPE[T], wide, heads.data_ptr(), I.LDH, act.data_ptr(), ro.data_ptr(), B, S, I.NMIX, I.NDIM, I.NCLS, I.LSMIN, 1.0, gc, disc,
                                     1.0 / SB, None if lscale is None else lscale.data_ptr(), row_loss.data_ptr(), a_tcp.data_ptr(), dheads.data_ptr(), None))
    torch.cuda.synchronize()
    for t, n in ((row_loss, "row_loss"), (a_tcp, "a_tcp_out"), (dheads, "dheads")):
        assert (t[SB:].float() == 7.0).all(), f"{n}: rows past S*B were written"
    tm = lambda t, w: t[:SB].float().cpu().numpy().astype(np.float64).reshape(S, B, w).transpose(1, 0, 2)      # time-major rows -> (B, S, .)
    return tm(row_loss, 8), a_tcp[:SB].cpu().numpy().astype(np.float64).reshape(B, S, 7), tm(dheads, I.LDH)


def reference(B, S, variant, a_dev):
    """float64 sections from the inputs; with gripper_control from the DEVICE's tcp-frame actions a_dev (the stage before), which are checked against the float64
    frame change and to take the float64 actions' branches"""
    gc, disc, scaled = VARIANTS[variant]
    inp = I.ll_inputs(B, S, gc)
    a64 = inp["actions"].astype(np.float64)
    at = a64
    if gc:
        at64 = R.world_to_tcp(a64, inp["robot_obs"].astype(np.float64))
        at = a_dev
        assert np.abs(at - at64).max() < 3e-4, "a_tcp_out"
    ref = I.ll_reference(inp, at, disc)
    I.ll_check_branches(ref, at)
    return I.ll_sections(ref, disc)


def split(dheads, disc):
    NO = I.NMIX * I.NDIM
    out = dict(dlogits=dheads[..., :NO], dmeans=dheads[..., NO:2 * NO], dlsr=dheads[..., 2 * NO:3 * NO])
    if disc:
        out["dgrip"] = dheads[..., 3 * NO:3 * NO + 2]
    return out, dheads[..., 3 * NO + (2 if disc else 0):]


def within(got, ref, gate, what, ulp=0.0, tiny=0.0):
    err = np.abs(got - ref)
    tol = gate * (np.abs(ref) + 1e-3 * np.abs(ref).max()) + ulp * np.abs(ref) + tiny
    print(f"{what}: worst err/tol = {float((err / tol).max()):.3f}")
    k = np.unravel_index(np.argmax(err - tol), err.shape)
    assert (err <= tol).all(), f"{what}: element {k}: got {got[k]!r} ref {ref[k]!r} tol {tol[k]:.3g} ({int((err > tol).sum())} elements off)"


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("B,S", I.LL_SHAPES)
def test_logistic_loss_matches_fp64(B, S, variant, kernel):
    gc, disc, scaled = VARIANTS[variant]
    T, wide = KERNELS[kernel]
    row_loss, a_tcp, dheads = run(B, S, variant, kernel)
    inp = I.ll_inputs(B, S, gc)
    if not gc:
        assert (a_tcp == inp["actions"]).all(), "without gripper_control a_tcp_out is the action itself"
    ref = reference(B, S, variant, a_tcp)
    # the gradient scale (1 / rows, times the loss scale when given) reaches dheads only
    within(row_loss, ref["row_loss"], I.LL_GATE["row_loss"], "row_loss")
    assert (row_loss[..., 7] == 0).all() and (disc or (row_loss[..., 6] == 0).all())
    gs = (LSCALE if scaled else 1.0) / (B * S)
    got, pad = split(dheads, disc)
    assert pad.shape[-1] >= 10 and (pad == 0).all(), "the pad columns of dheads must come back zero"
    for k, g in got.items():
        within(g, ref[k] * gs, I.LL_GATE[k], f"{k} [{kernel}]", ulp=I.ULP.get(T, 0.0), tiny=I.TINY.get(T, 0.0))
    assert (got["dlsr"][inp["lsr"].reshape(B, S, -1) < I.LSMIN] == 0).all(), "a clamped log-scale has no gradient"


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("B,S", I.LL_SHAPES)
def test_wide_kernel_agrees_with_serial_kernel(B, S, variant):
    """T = float: the wide kernel associates its sums as a tree, the serial one left to right; they agree within the same measured fp32 bound."""
    gc, disc, scaled = VARIANTS[variant]
    rl_s, at_s, dh_s = run(B, S, variant, "serial_f32")
    rl_w, at_w, dh_w = run(B, S, variant, "wide_f32")
    assert np.abs(at_s - at_w).max() < 3e-4
    ref = reference(B, S, variant, at_s)
    gs = (LSCALE if scaled else 1.0) / (B * S)
    err = np.abs(rl_w - rl_s)
    assert (err <= I.LL_GATE["row_loss"] * (np.abs(ref["row_loss"]) + 1e-3 * np.abs(ref["row_loss"]).max())).all()
    gw, pw = split(dh_w, disc)
    gser, ps = split(dh_s, disc)
    assert (pw == 0).all() and (ps == 0).all()
    for k in gw:
        r = ref[k] * gs
        assert (np.abs(gw[k] - gser[k]) <= I.LL_GATE[k] * (np.abs(r) + 1e-3 * np.abs(r).max())).all(), k


def test_logistic_loss_entry_validates():
    L, lib = _lib()
    t = torch.full((16, 192), 7.0, device="cuda")
    p = t.data_ptr()
    ok = dict(dtype=1, wide=1, heads=p, ldh=192, actions=p, robot_obs=p, B=1, S=1, n_mix=10, n_dim=6, ncls=10, lsmin=-7.0, alpha=1.0, gc=1, disc=1, gs=1.0, lscale=None,
              row_loss=p, a_tcp=None, dheads=p, stream=None)
    for bad in (dict(B=0), dict(n_mix=8), dict(n_dim=7), dict(ldh=181), dict(heads=None), dict(robot_obs=None), dict(dheads=None), dict(row_loss=None), dict(dtype=3), dict(ncls=1)):
        assert lib.hulc_k_logistic_loss(*{**ok, **bad}.values()) == 1, bad
        assert b"hulc_k_logistic_loss" in lib.hulc_last_error()
    torch.cuda.synchronize()
    assert (t == 7.0).all()
