"""GPU (-m gpu): the encoder's convolution kernels (conv_tile.h, conv_reg.h, conv_wgrad.h, conv1_wgrad.h) alone, through the per-type test entries hulc_k_conv_tile_t, hulc_k_conv_pair_t,
hulc_k_conv_wgrad_t and hulc_k_conv1_wgrad_u8_t, in bf16 and in fp16, against the float64 reference of tests/conv_ref.py on the inputs of tests/conv_inputs.py.

Every element is compared, none is left out: |got - ref| <= bound + max(ulp |ref|, smallest subnormal) for the 16-bit outputs (conv_inputs.tol16), bound alone for the fp32
weight gradients, exact zeros where the mask is off.  The 16-bit outputs are held to half an ulp as well (conv_inputs.tol16_nearest: what round-to-nearest guarantees and
truncation breaks).  Output buffers start at 7.0 with guard rows (plan_ln_gpu_util).  tests/test_conv_ref_host.py shows on the CPU that these tolerances see a dropped tap,
swapped kh / kw, a missing bias, truncation, a neighbour's border row, a zero taken for positive in the mask and a slab left out.  Nothing here is tuned to a kernel."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import conv_inputs as CI
import conv_ref as CR
from plan_ln_gpu_util import GUARD, check_tol, dev, f64, guard_intact, load, ptr, refused, sevens

pytestmark = pytest.mark.gpu
DT = CI.DTYPES16

# the modes of the conv tile entry per layer.  Forward: LDS-resident (0 / 1 / 7), weights in registers with 8 waves (10 / 11 / 17) and 4 waves (20 / 21 / 27); 7 / 17 / 27 emit
# conv2's ReLU bit words.  Data gradient: (mode, mask form)
FWD_FORMS = {3: (0, 10, 20), 2: (1, 7, 11, 17, 21, 27)}
DG_FORMS = {3: ((2, "values"), (22, "values"), (8, "bits"), (28, "bits")), 2: ((3, "values"), (23, "values"), (9, "bits"), (29, "bits"))}
EMITS_BITS = (7, 17, 27)
PAIR_FWD = {3: 3, 2: 2}
PAIR_DGRAD = {3: 13, 2: 12}
PAIR_WGRAD = {3: 23, 2: 22, 1: 21}
PAIR_FORM = {3: 10, 2: 17, 13: 28, 12: 29}          # the plan form a pair stage launches (conv_reg.h)
PAIR_WGS = ((1, 1), (3, 2))
FD_IDS = [f"conv{c[0]}-{c[1]}x{c[2]}" for c in CI.FD_CASES]


def _wgs_list(mode, frames):
    """workgroup counts of a case: the launcher's own grid, and for the weights-in-registers forms with several frames 1 and 3 workgroups (several items per workgroup, stacks)"""
    return (0, 1, 3) if mode >= 10 and frames > 1 else (0,)


def _plan(lib, form, frames, in_side, out_side, wgs):
    o = [C.c_int32() for _ in range(4)]
    assert lib.hulc_k_conv_plan(form, frames, in_side, out_side, wgs, *[C.byref(x) for x in o]) == 0, lib.hulc_last_error()
    return tuple(x.value for x in o)          # nbands, rows_per_band, frames_per_band, items


def _sides(layer, side, dgrad):
    """(in_side, out_side) as the tile entry takes them: the data gradient reads dY (the smaller map) and writes dX"""
    g = CI.LAYERS[layer]
    oh = CR.out_side(side, g["k"], g["s"])
    return (oh, side) if dgrad else (side, oh)


def _wdev(layer, dtype, dgrad=False):
    W = CI.weights(layer, dtype)[0]
    g = CI.LAYERS[layer]
    return dev(CR.pack_dgrad(W, g["s"]) if dgrad else (CR.pack_c1(W) if layer == 1 else CR.pack_fwd(W)), dtype)


def _bias(layer, dtype):
    return dev(CI.weights(layer, dtype)[1])


def _mask16(vals, dtype):
    """the mask values on the device, bit for bit: the subnormals and -0.0 included"""
    m = dev(vals, dtype)
    back = f64(m)
    assert np.array_equal(back, vals) and np.array_equal(np.signbit(back), np.signbit(vals))
    return m


def _bits_dev(keep):
    return torch.from_numpy(CR.pack_bits(keep)).cuda()


def _bit_buffer(shape):
    return torch.full((shape[0] + GUARD,) + tuple(shape[1:]), -1, device="cuda", dtype=torch.int32)


def _check16(got, ref, bound, dtype, what, keep=None):
    err = np.abs(got - ref)
    w = check_tol(err, CI.tol16(ref, bound, dtype, keep), got, ref, f"{what} [{dtype}]")
    check_tol(err, CI.tol16_nearest(ref, bound, dtype, keep), got, ref, f"{what} [{dtype}] (half an ulp)")
    return w


def _check_bits(words, out_t, n, ref, tol, C_, what):
    """the emitted ReLU bit words equal out > 0 exactly, and ref > 0 wherever |ref| > tol"""
    assert (words[n:] == -1).all(), f"{what}: bit words past the end were written"
    got = CR.unpack_bits(words[:n].cpu().numpy(), C_)
    assert np.array_equal(got, (out_t[:n] > 0).cpu().numpy()), f"{what}: bit words differ from out > 0"
    sure = np.abs(ref) > tol
    assert np.array_equal(got[sure], (ref > 0)[sure]), f"{what}: bit words differ from ref > 0"


def _tile(L, lib, dtype, mode, img, w, bias, mask, out, bits1, nf, in_side, out_side_, relu, wgs):
    return lib.hulc_k_conv_tile_t(L.DTYPE[dtype], mode, ptr(img), ptr(w), ptr(bias), ptr(mask), ptr(out), ptr(bits1), nf, in_side, out_side_, relu, wgs, None)


# ==================================================================================================== the case list reaches the edges
def test_case_list_reaches_every_geometry_edge():
    """hulc_k_conv_plan (host arithmetic) over the cases below: every weights-in-registers form meets stacked frames with a short last stack, several bands with a ragged last
    band, and more work items than workgroups.  (The LDS-resident forms 0 .. 3 / 7 .. 9 plan inside conv_tile.h and take no workgroup count: their stacks need hundreds of
    frames, which tests/test_gpu_kernels.py keeps.)  Stacks form only where a workgroup has several items, so they come from the 1- and 3-workgroup runs of the 7-frame cases."""
    L, lib = load()
    seen = {}
    for layer, side, frames in CI.FD_CASES:
        g = CI.LAYERS[layer]
        singles = [(m, False) for m in FWD_FORMS[layer] if m >= 10] + [(m, True) for m, _ in DG_FORMS[layer] if m >= 10]
        for form, dgrad in singles:
            for wgs in _wgs_list(form, frames):
                nb, rb, fpb, items = _plan(lib, form, frames, *_sides(layer, side, dgrad), wgs)
                rows = -(-side // g["s"]) if (dgrad and g["s"] == 2) else _sides(layer, side, dgrad)[1]          # the rows the bands cover (class rows for conv2's data gradient)
                e = seen.setdefault(form, set())
                if fpb > 1 and frames % fpb:
                    e.add("short stack")
                if nb > 1 and rows % rb:
                    e.add("ragged band")
                if items > (wgs if wgs else 256):
                    e.add("items > workgroups")
    for form, e in sorted(seen.items()):
        assert e == {"short stack", "ragged band", "items > workgroups"}, (form, e)
    assert set(seen) == {10, 11, 17, 20, 21, 27, 22, 23, 28, 29}
    # the pair stages: 7 frames per camera on (1, 1) and (3, 2) workgroups
    for layer in (3, 2):
        for stage, dgrad in ((PAIR_FWD[layer], False), (PAIR_DGRAD[layer], True)):
            e = set()
            for k, side in enumerate(CI.WG_PAIR_SIDES[layer]):
                for wg in PAIR_WGS:
                    nb, rb, fpb, items = _plan(lib, PAIR_FORM[stage], 7, *_sides(layer, side, dgrad), wg[k])
                    e |= {"short stack"} if fpb > 1 and 7 % fpb else set()
                    e |= {"items > workgroups"} if items > wg[k] else set()
            # (several bands: the static camera's 23 x 23 conv3 input is one band, so the ragged band of these kernel instances comes from the single launches above)
            assert e == {"short stack", "items > workgroups"}, (stage, e)
    # non-zero where the form does not take the shape, or is no weights-in-registers form
    o = [C.c_int32() for _ in range(4)]
    assert lib.hulc_k_conv_plan(10, 1, 23, 20, 0, *[C.byref(x) for x in o]) != 0 and b"hulc_k_conv_plan" in lib.hulc_last_error()
    assert lib.hulc_k_conv_plan(0, 1, 23, 21, 0, *[C.byref(x) for x in o]) != 0 and b"hulc_k_conv_plan" in lib.hulc_last_error()


# ==================================================================================================== forward
@pytest.mark.parametrize("layer,side,frames", CI.FD_CASES, ids=FD_IDS)
@pytest.mark.parametrize("dtype", DT)
def test_conv_forward_per_element(dtype, layer, side, frames):
    L, lib = load()
    g = CI.LAYERS[layer]
    oh = CR.out_side(side, g["k"], g["s"])
    X = dev(CI.acts(layer, side, frames, dtype)[0], dtype)
    w, b = _wdev(layer, dtype), _bias(layer, dtype)
    ref, bound = CI.fwd_ref(layer, side, frames, dtype)
    for mode in FWD_FORMS[layer]:
        for wgs in _wgs_list(mode, frames):
            out = sevens((frames, oh, oh, 64), dtype)
            bits = _bit_buffer((frames, oh, oh, 2)) if mode in EMITS_BITS else None
            L.check(_tile(L, lib, dtype, mode, X, w, b, bits, out, None, frames, side, oh, 1, wgs))
            torch.cuda.synchronize()
            what = f"conv{layer} forward mode {mode} side {side} frames {frames} wgs {wgs}"
            guard_intact(out, frames, what)
            _check16(f64(out[:frames]), ref, bound, dtype, what)
            if bits is not None:
                _check_bits(bits, out, frames, ref, CI.tol16(ref, bound, dtype), 64, what)


# ==================================================================================================== data gradient
@pytest.mark.parametrize("layer,side,frames", CI.FD_CASES, ids=FD_IDS)
@pytest.mark.parametrize("dtype", DT)
def test_conv_data_gradient_per_element(dtype, layer, side, frames):
    """16-bit mask VALUES carry +0.0, -0.0, both smallest subnormals and ordinary values in both halves of every packed pair: kept only where the value is > 0.  The bit-word
    forms run with dynamic work claiming, as in the engine"""
    L, lib = load()
    g = CI.LAYERS[layer]
    oh = CR.out_side(side, g["k"], g["s"])
    dY = dev(CI.acts(layer, side, frames, dtype)[1], dtype)
    w = _wdev(layer, dtype, True)
    vals, _ = CI.mask_values(layer, side, frames, dtype)
    masks = {"values": (_mask16(vals, dtype), CI.mask_keep(vals)), "bits": (_bits_dev(CI.keep_bits(layer, side, frames)), CI.keep_bits(layer, side, frames))}
    for mode, form in DG_FORMS[layer]:
        m, keep = masks[form]
        ref, bound = CI.dgrad_ref(layer, side, frames, dtype, keep)
        for wgs in _wgs_list(mode, frames):
            dx = sevens((frames, side, side, g["ci"]), dtype)
            L.check(_tile(L, lib, dtype, mode, dY, w, None, m, dx, None, frames, oh, side, 32 if form == "bits" else 0, wgs))
            torch.cuda.synchronize()
            what = f"conv{layer} data gradient mode {mode} ({form}) side {side} frames {frames} wgs {wgs}"
            guard_intact(dx, frames, what)
            _check16(f64(dx[:frames]), ref, bound, dtype, what, keep)


# ==================================================================================================== both cameras in one launch
def _job(L, inp, w, bias, out, bits, frames, in_side, out_side_):
    j = L.HulcConvJob()
    j.input, j.w, j.bias, j.out, j.bits = ptr(inp), ptr(w), ptr(bias), ptr(out), ptr(bits)
    j.frames, j.in_side, j.out_side = frames, in_side, out_side_
    return j


@pytest.mark.parametrize("wgs", PAIR_WGS, ids=["wg1-1", "wg3-2"])
@pytest.mark.parametrize("layer,dgrad", [(3, False), (2, False), (3, True), (2, True)], ids=["conv3-fwd", "conv2-fwd", "conv3-dgrad", "conv2-dgrad"])
@pytest.mark.parametrize("dtype", DT)
def test_two_camera_launch_per_element_and_equal_to_single_jobs(dtype, layer, dgrad, wgs):
    """the static and the gripper camera's maps, 7 frames each, as the two jobs of one launch: each job's result is bit-identical to the same job launched alone (job b NULL) on
    the same workgroups, and every element is inside the tolerance"""
    L, lib = load()
    g = CI.LAYERS[layer]
    frames = 7
    stage = (PAIR_DGRAD if dgrad else PAIR_FWD)[layer]
    emits = not dgrad and layer == 2
    w, b = _wdev(layer, dtype, dgrad), (None if dgrad else _bias(layer, dtype))
    cams = []
    for side in CI.WG_PAIR_SIDES[layer]:
        X, dY = CI.acts(layer, side, frames, dtype)
        ins, outs_ = _sides(layer, side, dgrad)
        if dgrad:
            keep = CI.keep_bits(layer, side, frames)
            ref, bound = CI.dgrad_ref(layer, side, frames, dtype, keep)
            cams.append(dict(inp=dev(dY, dtype), bits=_bits_dev(keep), keep=keep, ref=ref, bound=bound, shape=(frames, side, side, g["ci"]), ins=ins, outs=outs_))
        else:
            ref, bound = CI.fwd_ref(layer, side, frames, dtype)
            cams.append(dict(inp=dev(X, dtype), bits=None, keep=None, ref=ref, bound=bound, shape=(frames, outs_, outs_, 64), ins=ins, outs=outs_))

    def run(pair):
        outs = [sevens(c["shape"], dtype) for c in cams]
        bws = [_bit_buffer(c["shape"][:3] + (2,)) if emits else None for c in cams]
        jobs = [_job(L, c["inp"], w, b, o, bw if emits else c["bits"], frames, c["ins"], c["outs"]) for c, o, bw in zip(cams, outs, bws)]
        slabs = (C.c_int32 * 2)(5, 5)
        if pair:
            L.check(lib.hulc_k_conv_pair_t(L.DTYPE[dtype], stage, C.byref(jobs[0]), C.byref(jobs[1]), wgs[0], wgs[1], slabs, None))
        else:
            for k in range(2):
                L.check(lib.hulc_k_conv_pair_t(L.DTYPE[dtype], stage, C.byref(jobs[k]), None, wgs[k], 0, slabs, None))
        torch.cuda.synchronize()
        assert tuple(slabs) == (0, 0)
        return outs, bws

    outs, bws = run(True)
    souts, sbws = run(False)
    for k, c in enumerate(cams):
        what = f"pair stage {stage} job {'ab'[k]} wgs {wgs}"
        assert torch.equal(outs[k].view(torch.int16), souts[k].view(torch.int16)), f"{what}: differs from the job launched alone"
        guard_intact(outs[k], frames, what)
        _check16(f64(outs[k][:frames]), c["ref"], c["bound"], dtype, what, c["keep"])
        if emits:
            assert torch.equal(bws[k], sbws[k])
            _check_bits(bws[k], outs[k], frames, c["ref"], CI.tol16(c["ref"], c["bound"], dtype), 64, what)


# ==================================================================================================== weight gradients
def _check_wgrad(gw, gb, refs, K, slabs, pack, what):
    dW, db, bw, bb = refs
    assert slabs >= 1
    w = check_tol(np.abs(gw - pack(dW)), pack(CI.wgrad_bound(bw, K, slabs)), gw, pack(dW), f"{what}: dW ({slabs} slabs)")
    if gb is not None:
        # the bias partials land with fp32 atomics, one per workgroup and band: no more of them than slabs x bands, which the frame's rows bound
        check_tol(np.abs(gb - db), CI.wgrad_bound(bb, K, slabs), gb, db, f"{what}: db")
    return w


@pytest.mark.parametrize("layer,side,frames", CI.WG_CASES, ids=[f"conv{c[0]}-{c[1]}x{c[2]}" for c in CI.WG_CASES])
@pytest.mark.parametrize("dtype", DT)
def test_conv_weight_gradient_per_element(dtype, layer, side, frames):
    """single launches: 9 / 20 = the stacked-band kernel at the gripper camera's width, 18 / 23 / 31 and 49 / 57 = the LDS-DMA kernel (2 .. 5 bands per frame)"""
    L, lib = load()
    g = CI.LAYERS[layer]
    oh = CR.out_side(side, g["k"], g["s"])
    X, dY = CI.acts(layer, side, frames, dtype)
    KC = g["k"] * g["k"] * g["ci"]
    gw, gb = sevens((64, KC)), sevens(64)
    slabs = C.c_int32(-1)
    x, dy = dev(X, dtype), dev(dY, dtype)
    L.check(lib.hulc_k_conv_wgrad_t(L.DTYPE[dtype], layer, ptr(x), ptr(dy), ptr(gw), ptr(gb), frames, side, C.byref(slabs), None))
    what = f"conv{layer} weight gradient side {side} frames {frames} [{dtype}]"
    guard_intact(gw, 64, what); guard_intact(gb, 64, what)
    _check_wgrad(f64(gw[:64]), f64(gb[:64]), CI.wgrad_ref(layer, side, frames, dtype), frames * oh * oh, slabs.value, CR.pack_fwd, what)


@pytest.mark.parametrize("wgs", [(3, 2), (1, 1)], ids=["wg3-2", "wg1-1"])
@pytest.mark.parametrize("frames", CI.WG_PAIR_FRAMES, ids=["f3-1", "f1-3"])
@pytest.mark.parametrize("layer", [3, 2, 1])
@pytest.mark.parametrize("dtype", DT)
def test_two_camera_weight_gradient_per_element(dtype, layer, frames, wgs):
    """the three pair stages at the two cameras' own sides; conv1 reads fp32 NCHW frames"""
    L, lib = load()
    g = CI.LAYERS[layer]
    KC = g["k"] * g["k"] * g["ci"]
    jobs, outs, refs, keepalive = [], [], [], []
    for k, side in enumerate(CI.WG_PAIR_SIDES[layer]):
        oh = CR.out_side(side, g["k"], g["s"])
        if layer == 1:
            Xf, _, _, dY = CI.c1_inputs(side, frames[k], dtype)
            x = torch.from_numpy(np.ascontiguousarray(Xf)).cuda()
            refs.append((CI.c1_wgrad_ref(side, frames[k], dtype, "f32"), frames[k] * oh * oh))
        else:
            X, dY = CI.acts(layer, side, frames[k], dtype)
            x = dev(X, dtype)
            refs.append((CI.wgrad_ref(layer, side, frames[k], dtype), frames[k] * oh * oh))
        dy = dev(dY, dtype)
        gw, gb = sevens((g["co"], KC)), sevens(g["co"])
        keepalive += [x, dy]
        outs.append((gw, gb))
        jobs.append(_job(L, x, dy, None, gw, gb, frames[k], side, oh))
    slabs = (C.c_int32 * 2)(-1, -1)
    L.check(lib.hulc_k_conv_pair_t(L.DTYPE[dtype], PAIR_WGRAD[layer], C.byref(jobs[0]), C.byref(jobs[1]), wgs[0], wgs[1], slabs, None))
    for k in range(2):
        what = f"pair weight gradient conv{layer} job {'ab'[k]} frames {frames} wgs {wgs} [{dtype}]"
        gw, gb = outs[k]
        guard_intact(gw, g["co"], what); guard_intact(gb, g["co"], what)
        assert 1 <= slabs[k] <= wgs[k]
        _check_wgrad(f64(gw[:g["co"]]), f64(gb[:g["co"]]), refs[k][0], refs[k][1], slabs[k], CR.pack_c1 if layer == 1 else CR.pack_fwd, what)


# ==================================================================================================== conv1
@pytest.mark.parametrize("side,frames", CI.C1_CASES, ids=[f"{c[0]}x{c[1]}" for c in CI.C1_CASES])
@pytest.mark.parametrize("dtype", DT)
def test_conv1_forward_and_weight_gradient_per_element(dtype, side, frames):
    """forward modes 4 (fp32 NCHW), 5 (uint8) and 6 (uint8 + RandomShiftsAug shifts that include 0, pad = no shift and 2 pad) with the ReLU bit words the engine hands to conv2's
    data gradient; the weight gradient from fp32 NCHW and, in the form the engine runs, from uint8 with the same shifts, with and without the folded affine"""
    L, lib = load()
    oh = CR.out_side(side, 8, 4)
    pad = CI.c1_pad(side)
    Xf, u8, sh, dY = CI.c1_inputs(side, frames, dtype)
    xf, xu, shd, dy = torch.from_numpy(np.ascontiguousarray(Xf)).cuda(), torch.from_numpy(np.ascontiguousarray(u8)).cuda(), torch.from_numpy(np.ascontiguousarray(sh)).cuda(), dev(dY, dtype)
    w, b = _wdev(1, dtype), _bias(1, dtype)
    for mode, src, img, m in ((4, "f32", xf, None), (5, "u8", xu, None), (6, "u8s", xu, shd)):
        ref, bound = CI.c1_fwd_ref(side, frames, dtype, src)
        out, bits = sevens((frames, oh, oh, 32), dtype), _bit_buffer((frames, oh, oh, 1))
        L.check(_tile(L, lib, dtype, mode, img, w, b, m, out, bits, frames, side, oh, 1, 0))
        torch.cuda.synchronize()
        what = f"conv1 forward mode {mode} side {side}"
        guard_intact(out, frames, what)
        _check16(f64(out[:frames]), ref, bound, dtype, what)
        _check_bits(bits, out, frames, ref, CI.tol16(ref, bound, dtype), 32, what)
    K = frames * oh * oh
    gw, gb = sevens((32, 192)), sevens(32)
    slabs = C.c_int32(-1)
    L.check(lib.hulc_k_conv_wgrad_t(L.DTYPE[dtype], 1, ptr(xf), ptr(dy), ptr(gw), ptr(gb), frames, side, C.byref(slabs), None))
    guard_intact(gw, 32, "conv1 wgrad"); guard_intact(gb, 32, "conv1 wgrad")
    _check_wgrad(f64(gw[:32]), f64(gb[:32]), CI.c1_wgrad_ref(side, frames, dtype, "f32"), K, slabs.value, CR.pack_c1, f"conv1 weight gradient from fp32 side {side} [{dtype}]")
    for fold in (1, 0):
        gw, gb = sevens((32, 192)), sevens(32)
        L.check(lib.hulc_k_conv1_wgrad_u8_t(L.DTYPE[dtype], ptr(xu), ptr(shd), pad, ptr(dy), ptr(gw), ptr(gb), frames, side, 2, fold, C.byref(slabs), None))
        guard_intact(gw, 32, "conv1 wgrad u8"); guard_intact(gb, 32, "conv1 wgrad u8")
        _check_wgrad(f64(gw[:32]), f64(gb[:32]), CI.c1_wgrad_ref(side, frames, dtype, "u8s", fold), K, slabs.value, CR.pack_c1, f"conv1 weight gradient from uint8 fold {fold} side {side} [{dtype}]")


# ==================================================================================================== exact impulses
def _impulse_positions(lib, form, layer, side, frames, dgrad, wgs):
    """(frame, row, column) in the map the impulse lives in: each corner, an edge centre, the centre, the first pixel of the second band and of the second stacked frame"""
    g = CI.LAYERS[layer]
    n = _sides(layer, side, dgrad)[0]
    pos = [(0, 0, 0), (0, 0, n - 1), (0, n - 1, 0), (0, n - 1, n - 1), (0, 0, n // 2), (0, n // 2, n // 2), (1, 0, 0)]
    if form is not None:
        nb, rb, fpb, _ = _plan(lib, form, frames, *_sides(layer, side, dgrad), wgs)
        if nb > 1:
            pos.append((0, min(rb if dgrad else rb * g["s"], n - 1), 0))
        if fpb > 1 and fpb < frames:
            pos.append((fpb, 0, 0))
    return pos


@pytest.mark.parametrize("layer", [3, 2])
@pytest.mark.parametrize("dtype", DT)
def test_conv_impulses_are_exact(dtype, layer):
    """one input pixel 1.0 in one channel, everything else and the bias 0: the forward output is max(W, 0) at the taps' positions exactly and 0 elsewhere; the data-gradient
    analogue (a one-hot dY, all-on mask) is the weights exactly.  Sides with several bands (31 / 49) and with stacked frames (9 / 20 on one workgroup), 3 frames"""
    L, lib = load()
    g = CI.LAYERS[layer]
    W = CI.weights(layer, dtype)[0]
    frames = 3
    zero_b = dev(np.zeros(64))
    for side, wgs in (((31, 0), (9, 1)) if layer == 3 else ((49, 0), (20, 1))):
        oh = CR.out_side(side, g["k"], g["s"])
        allon = {"values": dev(np.ones((frames, side, side, g["ci"])), dtype), "bits": _bits_dev(np.ones((frames, side, side, g["ci"]), bool))}
        runs = [(m, False, None) for m in FWD_FORMS[layer]] + [(m, True, f) for m, f in DG_FORMS[layer]]
        for mode, dgrad, form in runs:
            w = _wdev(layer, dtype, dgrad)
            n, ch = (oh, 64) if dgrad else (side, g["ci"])
            for q, (f, r, c) in enumerate(_impulse_positions(lib, mode if mode >= 10 else None, layer, side, frames, dgrad, wgs if mode >= 10 else 0)):
                c0 = (7 * q + 3) % ch
                src = np.zeros((frames, n, n, ch)); src[f, r, c, c0] = 1.0
                srcd = dev(src, dtype)
                reach = n if dgrad else (side - g["k"]) // g["s"] * g["s"] + g["k"]          # an odd side under stride 2: the last row / column is read by no tap
                if dgrad:
                    ref = CR.dgrad(src, W, g["s"], side, np.ones((frames, side, side, g["ci"]), bool))[0]
                    out = sevens((frames, side, side, g["ci"]), dtype)
                    L.check(_tile(L, lib, dtype, mode, srcd, w, None, allon[form], out, None, frames, oh, side, 32 if form == "bits" else 0, wgs if mode >= 10 else 0))
                else:
                    ref = CR.fwd(src, W, np.zeros(64), g["s"])[0]
                    out = sevens((frames, oh, oh, 64), dtype)
                    bits = _bit_buffer((frames, oh, oh, 2)) if mode in EMITS_BITS else None
                    L.check(_tile(L, lib, dtype, mode, srcd, w, zero_b, bits, out, None, frames, side, oh, 1, wgs if mode >= 10 else 0))
                torch.cuda.synchronize()
                got = f64(out[:frames])
                assert ((ref != 0).any() or r >= reach or c >= reach) and np.array_equal(got, ref), (f"conv{layer} mode {mode} side {side} impulse at {(f, r, c, c0)} [{dtype}]", int((got != ref).sum()))
                guard_intact(out, frames, f"impulse mode {mode}")


@pytest.mark.parametrize("dtype", DT)
def test_weight_gradient_impulses_are_exact(dtype):
    """a one-hot X times a one-hot dY gives exactly one nonzero weight-gradient element, of exactly the right value"""
    L, lib = load()
    for layer, side in ((3, 23), (3, 9), (2, 49), (2, 20), (1, 84)):
        g = CI.LAYERS[layer]
        k, s = g["k"], g["s"]
        oh = CR.out_side(side, k, s)
        frames = 3
        KC = k * k * g["ci"]
        for q, (f, i, j, kh, kw) in enumerate(((0, 0, 0, 0, 0), (1, oh // 2, oh // 2, k - 1, 1), (2, oh - 1, oh - 1, k - 1, k - 1), (2, 0, oh - 1, 1, k - 1))):
            ci0, co0 = (5 * q + 1) % g["ci"], (11 * q + 7) % g["co"]
            X = np.zeros((frames, side, side, g["ci"])); X[f, i * s + kh, j * s + kw, ci0] = 0.75
            dY = np.zeros((frames, oh, oh, g["co"])); dY[f, i, j, co0] = -1.5
            ref = np.zeros((g["co"], g["ci"], k, k)); ref[co0, ci0, kh, kw] = -1.125
            x = torch.from_numpy(np.ascontiguousarray(X.transpose(0, 3, 1, 2), dtype=np.float32)).cuda() if layer == 1 else dev(X, dtype)
            gw, gb, dy = sevens((g["co"], KC)), sevens(g["co"]), dev(dY, dtype)
            L.check(lib.hulc_k_conv_wgrad_t(L.DTYPE[dtype], layer, ptr(x), ptr(dy), ptr(gw), ptr(gb), frames, side, None, None))
            got = f64(gw[:g["co"]])
            want = (CR.pack_c1 if layer == 1 else CR.pack_fwd)(ref)
            assert np.array_equal(got, want), (f"conv{layer} side {side} impulse {q} [{dtype}]", np.argwhere(got != want)[:4].tolist())
            dbw = np.zeros(g["co"]); dbw[co0] = -1.5
            assert np.array_equal(f64(gb[:g["co"]]), dbw)
            guard_intact(gw, g["co"], "wgrad impulse")


# ==================================================================================================== refusals
def test_typed_entries_refuse_before_they_touch_anything():
    """unknown dtype, fp32, a bench-only form, an out_side that does not belong to in_side, a data-gradient form without its mask: non-zero, the entry's name in the message,
    the sentinel-filled outputs untouched"""
    L, lib = load()
    BF, F16, F32 = L.DTYPE["bf16"], L.DTYPE["fp16"], L.DTYPE["fp32"]
    x = dev(np.ones((1, 23, 23, 64)), "bf16"); w = dev(np.ones((64, 576)), "bf16"); b = dev(np.zeros(64))
    out = sevens((1, 23, 23, 64), "bf16"); gw = sevens((64, 576)); gb = sevens(64)
    m = dev(np.ones((1, 23, 23, 64)), "bf16")
    u8 = torch.zeros((1, 84, 84, 3), dtype=torch.uint8, device="cuda"); dy1 = dev(np.ones((1, 20, 20, 32)), "bf16"); g1 = sevens((32, 192)); b1 = sevens(32)
    tile = lambda dt, mode, mask, ins, outs, relu=1, wgs=0: lib.hulc_k_conv_tile_t(dt, mode, ptr(x), ptr(w), ptr(b), ptr(mask), ptr(out), None, 1, ins, outs, relu, wgs, None)
    for dt in (7, -1, F32):
        refused(lib, tile(dt, 10, None, 23, 21), "hulc_k_conv_tile_t")
        refused(lib, lib.hulc_k_conv_wgrad_t(dt, 3, ptr(x), ptr(x), ptr(gw), ptr(gb), 1, 23, None, None), "hulc_k_conv_wgrad_t")
        refused(lib, lib.hulc_k_conv1_wgrad_u8_t(dt, ptr(u8), None, 4, ptr(dy1), ptr(g1), ptr(b1), 1, 84, 2, 1, None, None), "hulc_k_conv1_wgrad_u8_t")
        j = _job(L, x, w, b, out, None, 1, 23, 21)
        refused(lib, lib.hulc_k_conv_pair_t(dt, 3, C.byref(j), None, 1, 0, None, None), "hulc_k_conv_pair_t")
    for dt in (BF, F16):
        for mode in (12, 13, 18, 19):          # the 8-wave data-gradient forms: bench only
            refused(lib, tile(dt, mode, m, 21, 23, 0), "hulc_k_conv_tile_t")
        refused(lib, lib.hulc_k_conv_tile_t(dt, 5, ptr(u8), ptr(w), ptr(b), None, ptr(out), None, 1, 84, 20, 1 | 256, 0, None), "hulc_k_conv_tile_t")          # the register-staged cross-check
        refused(lib, lib.hulc_k_conv1_wgrad_u8_t(dt, ptr(u8), None, 4, ptr(dy1), ptr(g1), ptr(b1), 1, 84, 1, 1, None, None), "hulc_k_conv1_wgrad_u8_t")          # form 1
        refused(lib, tile(dt, 10, None, 23, 20), "hulc_k_conv_tile_t")          # out_side that does not belong to in_side
        refused(lib, tile(dt, 21, None, 23, 11), "hulc_k_conv_tile_t")
        refused(lib, tile(dt, 28, m, 21, 24, 0), "hulc_k_conv_tile_t")
        refused(lib, tile(dt, 4, None, 84, 21), "hulc_k_conv_tile_t")
        for mode in (2, 8, 22, 28):          # a data-gradient form without its mask
            refused(lib, tile(dt, mode, None, 21, 23, 0), "hulc_k_conv_tile_t")
        refused(lib, tile(dt, 0, None, 23, 21, 1, 3), "hulc_k_conv_tile_t")          # a workgroup count for a form that takes none
        j = _job(L, x, w, b, out, None, 1, 23, 20)
        refused(lib, lib.hulc_k_conv_pair_t(dt, 3, C.byref(j), None, 1, 0, None, None), "hulc_k_conv_pair_t")
        j = _job(L, x, w, None, out, None, 1, 21, 23)
        refused(lib, lib.hulc_k_conv_pair_t(dt, 13, C.byref(j), None, 1, 0, None, None), "hulc_k_conv_pair_t")          # data gradient without its bit words
        refused(lib, lib.hulc_k_conv_wgrad_t(dt, 4, ptr(x), ptr(x), ptr(gw), ptr(gb), 1, 23, None, None), "hulc_k_conv_wgrad_t")
        refused(lib, lib.hulc_k_conv_wgrad_t(dt, 3, ptr(x), ptr(x), ptr(gw), ptr(gb), 1, 2, None, None), "hulc_k_conv_wgrad_t")
    # the bf16 wrappers keep their names in their messages
    refused(lib, lib.hulc_k_conv_tile(30, None, None, None, None, None, 1, 23, 21, 1, None), "hulc_k_conv_tile")
    torch.cuda.synchronize()
    for t in (out, gw, gb, g1, b1):
        assert (t.float() == 7.0).all(), "a refused call wrote to an output"
