"""Gradient clipping and gradient-norm logging fused into the optimizer step (csrc/kernels.h grad_sumsq_kernel / grad_norm_combine_kernel, ClipState;
include/hulc_hip.h hulc_grad_clip_set / hulc_grad_norm_get).

The gradient buffer is the caller's, so every optimizer test WRITES its gradients and never runs a backward: seeded normal values with a per-tensor scale
drawn log-uniformly from [1e-3, 1], every alignment-padding element set to the finite sentinel 1e30 (its square overflows fp32: one padding element that
leaks into a sum shows up as an infinite norm).  zero_grads() is never called here, so no tensor is marked stale.  References are numpy fp64 and torch's CPU
clip_grad_norm_ / clip_grad_value_ / optim.Adam / AdamW / SGD run in FLOAT64 on copies of the same inputs — never a second run of the library.

Gates (from the precision of the formats, not from what the kernels give): norms rel 1e-5 (a chunk sum of non-negative fp32 terms: <= 17 sequential adds
per thread (16 + one tail element) + 8 tree levels <= 25 u = 1.5e-6, halved by the square root, fp64 across chunks); SGD update rel-L2 1e-3 and momentum 5e-6; Adam first moment 5e-6,
second moment 1e-5, parameters golden_util.adam_close with >= 99 % of the entries in its strict branch.  Every clipping test carries a negative control:
the same torch reference WITHOUT clipping must miss the same gates.

Engines are built once per compute type at max_batch 2, max_seq 4 (the optimizer pass covers the whole parameter buffer whatever the batch); the
file takes ~ 40 s on the GPU (measured: 40.5 s, most of it the float64 torch references on the host).  Measured worst figures against the gates: norms
6.9e-8; SGD update 3.6e-6, momentum 7.6e-8; exp_avg 7.1e-8, exp_avg_sq 1.8e-7, |dp| after step 2 4.4e-7; every negative control misses by 0.9 .. 1.0."""
import os
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from golden_util import adam_close  # noqa: E402
from hulc_amd import spec  # noqa: E402
from hulc_amd.engine import StepEngine  # noqa: E402

PAD = 1e30
DIMS = spec.ModelDims(kind="hulc", max_window=32, use_clip=True)
_T0 = time.time()


def _numel(shape):
    return int(np.prod(shape)) if len(shape) else 1


def _tensors(eng):
    return [(n, off, _numel(shape)) for n, (off, shape) in eng.layout.items()]


def _listed_mask(eng):
    m = np.zeros(eng.numel, bool)
    for _, off, k in _tensors(eng):
        m[off:off + k] = True
    return m


@pytest.fixture(scope="module")
def P0():
    return spec.init_all(DIMS, seed=0, ln_jitter=True)


@pytest.fixture(scope="module")
def engines(P0):
    made = {}

    def get(dtype):
        if dtype not in made:
            e = StepEngine(DIMS, 2, 4, dtype=dtype, device="cuda:0", dropout_p=0.0, seed=1)
            e.load_numpy(P0)
            torch.cuda.synchronize()
            made[dtype] = (e, e.flat_params.clone())
        return made[dtype][0]

    get.made = made
    yield get
    for e, _ in made.values():
        e.close()
    print("test_gpu_grad_clip: module wall time %.1f s" % (time.time() - _T0))


def _reset(engines, eng, scale=None):
    """Initial parameters, zero moments, step count 0, clipping off (fp16: a fresh scaler at `scale`, set through hulc_scaler_set)."""
    p0 = [v[1] for v in engines.made.values() if v[0] is eng][0]
    eng.flat_params.copy_(p0)
    eng.adam_m.zero_(); eng.adam_v.zero_()
    eng.adam_t = 0
    eng.prepare_weights()
    eng.set_grad_clip("off", None, track=False)
    if eng.dtype == "fp16":
        eng.scaler_enable(init_scale=65536.0)
        eng.scaler_load(float(scale or 1.0), 0, 0)


def make_grads(eng, seed, mult=1.0):
    """(numel,) fp32 device buffer: padding = 1e30, tensor t ~ N(0, (mult sigma_t)^2) with sigma_t log-uniform in [1e-3, 1] (the scales are the same for
    every seed, the values are independent draws: a draw with mult = 20 has ~ 20 x the norm)."""
    dev = eng.device
    g = torch.Generator(device=dev); g.manual_seed(seed)
    rs = np.random.RandomState(7)
    flat = torch.full((eng.numel,), PAD, dtype=torch.float32, device=dev)
    for _, off, k in _tensors(eng):
        sigma = float(10.0 ** rs.uniform(-3.0, 0.0))
        flat[off:off + k] = torch.randn(k, device=dev, generator=g) * (sigma * mult)
    return flat


def np_norms(eng, G64):
    """fp64 per-tensor and total L2 norm of the listed elements of a host copy."""
    per = {n: float(np.sqrt(np.dot(G64[off:off + k], G64[off:off + k]))) for n, off, k in _tensors(eng)}
    return per, float(np.sqrt(sum(v * v for v in per.values())))


def rel(a, b):
    return abs(a - b) / abs(b)


def check_norms(eng, G_host, factor=1.0, gate=1e-5, got=None):
    """The engine's report of the last step (or `got`: a report taken earlier) against numpy fp64 of `G_host` x factor; prints the worst figure before asserting."""
    got = eng.grad_norms(per_tensor=True) if got is None else got
    per, tot = np_norms(eng, G_host.astype(np.float64) * factor)
    assert set(got["per_tensor"]) == set(per)
    assert np.isfinite(got["total"]) and all(np.isfinite(v) for v in got["per_tensor"].values()), "a padding element (1e30) reached a norm"
    worst = max((rel(got["per_tensor"][n], per[n]), n) for n in per if per[n] > 0)
    print("norms: total rel err %.2e, worst tensor %.2e (%s)" % (rel(got["total"], tot), worst[0], worst[1]))
    assert rel(got["total"], tot) <= gate, (got["total"], tot)
    bad = [(n, got["per_tensor"][n], per[n]) for n in per if per[n] > 0 and rel(got["per_tensor"][n], per[n]) > gate]
    assert not bad, bad[:5]
    return got, per, tot


# ---------------------------------------------------------------------------------------------------------------- torch fp64 reference
def torch_ref(eng, P0flat, grads, opt, lr, clip=None, wd=0.0):
    """Two (len(grads)) optimizer steps of torch on the CPU in float64.  grads: host fp32 arrays (effective gradients).  clip: None, ("norm", limit) or
    ("value", limit).  Returns per step {"p", "m", "v"}: flat fp64 arrays in the engine's layout (padding zero)."""
    ts = _tensors(eng)
    params = [torch.nn.Parameter(torch.from_numpy(P0flat[off:off + k].astype(np.float64))) for _, off, k in ts]
    # the hyper-parameters are inputs too: the C-ABI takes them as C floats, so the reference gets the values the library was actually handed.  (With the
    # decimal 0.999 instead of float32(0.999) = 0.99900001287 torch's 1 - beta2 differs from the kernel's by 1.29e-5 relative — in EVERY second moment,
    # clipping or not; measured: exp_avg_sq rel-L2 1.30e-5 on every tensor before this line was written, 1e-7 level after.)
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    lr, wd = f32(lr), f32(wd)
    if opt == "sgd":
        o = torch.optim.SGD(params, lr=lr, momentum=f32(0.9), weight_decay=wd)
    elif opt == "adamw":
        o = torch.optim.AdamW(params, lr=lr, betas=(f32(0.9), f32(0.999)), eps=f32(1e-8), weight_decay=wd)
    else:
        o = torch.optim.Adam(params, lr=lr, betas=(f32(0.9), f32(0.999)), eps=f32(1e-8), weight_decay=wd)
    out = []
    for G in grads:
        for p, (_, off, k) in zip(params, ts):
            p.grad = torch.from_numpy(G[off:off + k].astype(np.float64))
        if clip and clip[0] == "norm":
            torch.nn.utils.clip_grad_norm_(params, clip[1])
        elif clip and clip[0] == "value":
            torch.nn.utils.clip_grad_value_(params, clip[1])
        o.step()
        rec = {k_: np.zeros(eng.numel, np.float64) for k_ in ("p", "m", "v")}
        for p, (_, off, k) in zip(params, ts):
            st = o.state[p]
            rec["p"][off:off + k] = p.detach().numpy()
            if opt == "sgd":
                rec["m"][off:off + k] = st["momentum_buffer"].numpy()
            else:
                rec["m"][off:off + k] = st["exp_avg"].numpy()
                rec["v"][off:off + k] = st["exp_avg_sq"].numpy()
        out.append(rec)
    return out


def worst_rel_l2(eng, got, ref):
    w = (0.0, "")
    for n, off, k in _tensors(eng):
        den = np.linalg.norm(ref[off:off + k])
        if den > 0:
            w = max(w, (float(np.linalg.norm(got[off:off + k] - ref[off:off + k]) / den), n))
    return w


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def run_engine(eng, grads_dev, opt, lr, wd=0.0, scale=1.0, grad_scale=1.0):
    """The same steps on the engine; returns per step host copies {"p", "m", "v"} (fp32)."""
    out = []
    for G in grads_dev:
        eng.flat_grads.copy_(G if scale == 1.0 else torch.where(G == PAD, G, G * scale))
        if opt == "sgd":
            eng.optimizer_step("sgd", lr=lr, momentum=0.9, weight_decay=wd, grad_scale=grad_scale)
        elif opt == "adam" and wd == 0.0:
            eng.adam_step(lr=lr, grad_scale=grad_scale)
        else:
            eng.optimizer_step(opt, lr=lr, weight_decay=wd, grad_scale=grad_scale)
        out.append(dict(p=host(eng.flat_params).copy(), m=host(eng.adam_m).copy(), v=host(eng.adam_v).copy()))
    return out


def sgd_gates(eng, P0flat, got, ref, tag):
    """SGD is linear in the gradient: the two-step parameter update against torch's (rel-L2 <= 1e-3 per tensor) and the momentum buffer (<= 5e-6)."""
    up = worst_rel_l2(eng, got[1]["p"].astype(np.float64) - P0flat, ref[1]["p"] - P0flat)
    mo = worst_rel_l2(eng, got[1]["m"].astype(np.float64), ref[1]["m"])
    print("%s: SGD update worst rel-L2 %.2e (%s), momentum %.2e (%s)" % (tag, up[0], up[1], mo[0], mo[1]))
    return up[0] <= 1e-3 and mo[0] <= 5e-6


def adam_gates(eng, got, ref, g2, lr, tag, mask):
    """First / second moments after step 1 (rel-L2 <= 5e-6 / 1e-5 per tensor), parameters after step 2 with the project's adam_close."""
    m = worst_rel_l2(eng, got[0]["m"].astype(np.float64), ref[0]["m"])
    v = worst_rel_l2(eng, got[0]["v"].astype(np.float64), ref[0]["v"])
    err = np.abs(got[1]["p"][mask].astype(np.float64) - ref[1]["p"][mask])
    ok_p = adam_close(got[1]["p"][mask], ref[1]["p"][mask], g2[mask], lr, steps=2)
    print("%s: exp_avg worst rel-L2 %.2e (%s), exp_avg_sq %.2e (%s), max |dp| after step 2 %.2e, adam_close %s" % (tag, m[0], m[1], v[0], v[1], float(err.max()), ok_p))
    return m[0] <= 5e-6 and v[0] <= 1e-5 and ok_p


def two_draws(eng, first_mult=20.0):
    """Step 1: an independent draw scaled `first_mult` x; step 2: the base draw.  Device buffers and host copies."""
    gd = [make_grads(eng, 101, first_mult), make_grads(eng, 202)]
    return gd, [host(g).copy() for g in gd]


# ---------------------------------------------------------------------------------------------------------------- 4, 5, 10: the norms themselves
def test_norms_match_numpy_fp64_and_padding_never_counts(engines):
    eng = engines("fp32")
    _reset(engines, eng)
    G = make_grads(eng, 202)
    Gh = host(G).copy()
    assert (Gh[~_listed_mask(eng)] == np.float32(PAD)).all() and (~_listed_mask(eng)).sum() > 0       # the layout has padding and it holds the sentinel
    sizes = {n: k for n, _, k in _tensors(eng)}
    assert sizes["logit_scale"] == 1 and sizes["action_decoder.gripper_fc.bias"] == 2                   # the single-element tensor and the numel % 4 != 0 one
    assert max(sizes.values()) >= 2048 * 2048
    eng.set_grad_clip("off", None, track=True)
    eng.flat_grads.copy_(G)
    eng.optimizer_step("sgd", lr=0.0)
    got, per, tot = check_norms(eng, Gh)
    assert got["coef"] == 1.0
    assert per["logit_scale"] > 0 and per["action_decoder.gripper_fc.bias"] > 0
    # without track and without clipping by norm nothing is computed: reading is an error, not a stale value
    eng.set_grad_clip("value", 1.0, track=False)
    eng.optimizer_step("sgd", lr=0.0)
    with pytest.raises(RuntimeError):
        eng.grad_norms()
    with pytest.raises(ValueError):
        eng.set_grad_clip("l1", 1.0)


def test_norms_repeat_bit_for_bit_and_do_not_depend_on_the_compute_type(engines):
    seen = {}
    for dtype in ("fp32", "bf16", "fp16"):
        eng = engines(dtype)
        _reset(engines, eng, scale=1.0)
        G = make_grads(eng, 202)
        eng.set_grad_clip("off", None, track=True)
        runs = []
        for _ in range(2):
            eng.flat_grads.copy_(G)
            eng.optimizer_step("sgd", lr=0.0)
            r = eng.grad_norms(per_tensor=True)
            runs.append(np.array([r["total"]] + [r["per_tensor"][n] for n, _, _ in _tensors(eng)], np.float32))
        assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32)), dtype
        seen[dtype] = runs[0]
    assert np.array_equal(seen["fp32"].view(np.uint32), seen["bf16"].view(np.uint32))
    assert np.array_equal(seen["fp32"].view(np.uint32), seen["fp16"].view(np.uint32))


def test_grad_scale_enters_norm_and_coefficient(engines):
    """grad_scale = 1/4 (a world of 4 after a SUM all-reduce): norm and coefficient are those of G / 4."""
    eng = engines("fp32")
    _reset(engines, eng)
    G = make_grads(eng, 202)
    Gh = host(G).copy()
    _, tot = np_norms(eng, Gh.astype(np.float64) * 0.25)
    limit = 0.3 * tot
    eng.set_grad_clip("norm", limit, track=False)
    eng.flat_grads.copy_(G)
    eng.optimizer_step("sgd", lr=0.0, grad_scale=0.25)
    got, _, _ = check_norms(eng, Gh, factor=0.25)
    want = min(1.0, limit / (tot + 1e-6))
    print("coef %.8f, expected %.8f" % (got["coef"], want))
    assert want < 0.31 and rel(got["coef"], want) <= 1e-5


# ---------------------------------------------------------------------------------------------------------------- 6: clipping by norm
def test_sgd_clipped_by_norm_matches_torch(engines, P0):
    eng = engines("fp32")
    _reset(engines, eng)
    P0flat = host(eng.flat_params).astype(np.float64)
    gd, gh = two_draws(eng)
    _, n2 = np_norms(eng, gh[1].astype(np.float64))
    _, n1 = np_norms(eng, gh[0].astype(np.float64))
    limit = 2.0 * n2
    assert 0.05 < limit / n1 < 0.2                           # coef ~ 0.1 on step 1, exactly 1 on step 2
    eng.set_grad_clip("norm", limit)
    got = run_engine(eng, gd, "sgd", 1.0)
    check_norms(eng, gh[1])
    assert eng.grad_norms()["coef"] == 1.0
    ref = torch_ref(eng, P0flat, gh, "sgd", 1.0, clip=("norm", limit))
    assert sgd_gates(eng, P0flat, got, ref, "clipped reference")
    ctrl = torch_ref(eng, P0flat, gh, "sgd", 1.0, clip=None)
    assert not sgd_gates(eng, P0flat, got, ctrl, "negative control (unclipped reference)")


@pytest.mark.parametrize("opt,wd", [("adam", 0.0), ("adam", 1e-2), ("adamw", 1e-2)])
def test_adam_clipped_by_norm_matches_torch(engines, opt, wd):
    """A single Adam step from zero moments moves every parameter by ~ lr sign(g) whatever the gradient's scale, so the coefficient is only visible in the
    moments and in the SECOND step: two steps with different gradients, coef ~ 0.1 on the first and exactly 1 on the second."""
    lr = 1e-3
    eng = engines("bf16")
    _reset(engines, eng)
    P0flat = host(eng.flat_params).astype(np.float64)
    mask = _listed_mask(eng)
    gd, gh = two_draws(eng)
    _, n2 = np_norms(eng, gh[1].astype(np.float64))
    limit = 2.0 * n2
    eng.set_grad_clip("norm", limit)
    got = run_engine(eng, gd, opt, lr, wd=wd)
    assert eng.grad_norms()["coef"] == 1.0
    strict = float((np.abs(gh[1][mask]) > 1e-5).mean())
    print("entries in adam_close's strict branch: %.4f %%" % (100 * strict))
    assert strict >= 0.99
    ref = torch_ref(eng, P0flat, gh, opt, lr, clip=("norm", limit), wd=wd)
    assert adam_gates(eng, got, ref, gh[1], lr, "clipped reference", mask)
    ctrl = torch_ref(eng, P0flat, gh, opt, lr, clip=None, wd=wd)
    assert not adam_gates(eng, got, ctrl, gh[1], lr, "negative control (unclipped reference)", mask)


# ---------------------------------------------------------------------------------------------------------------- 7: coef = 1 is free
def _shadow(eng):
    return eng.get_tensor("wshadow", eng.numel).copy()


def _two_steps_state(eng, gd, opt="adam", wd=0.0):
    run_engine(eng, gd[:1], opt, 1e-3, wd=wd)
    r = run_engine(eng, gd[1:], opt, 1e-3, wd=wd)[0]
    r["s"] = _shadow(eng)
    return r


def _same_bits(a, b, mask):
    return all(np.array_equal(a[k][mask].view(np.uint32), b[k][mask].view(np.uint32)) for k in ("p", "m", "v", "s"))


def test_coefficient_one_and_tracking_leave_the_step_bit_identical(engines, P0):
    eng = engines("bf16")
    mask = _listed_mask(eng)
    gd, gh = two_draws(eng)
    _, n1 = np_norms(eng, gh[0].astype(np.float64))
    # the baseline: a context that never heard of clipping
    base_eng = StepEngine(DIMS, 2, 4, dtype="bf16", device="cuda:0", dropout_p=0.0, seed=1)
    base_eng.load_numpy(P0)
    base = _two_steps_state(base_eng, gd)
    base_eng.close()
    assert np.abs(base["s"][mask]).max() > 0
    _reset(engines, eng)
    eng.set_grad_clip("norm", 2.0 * n1)                       # twice the larger of the two norms: coef == 1 on both steps
    a = _two_steps_state(eng, gd)
    assert eng.grad_norms()["coef"] == 1.0
    assert _same_bits(a, base, mask)
    _reset(engines, eng)
    eng.set_grad_clip("off", None, track=True)
    b = _two_steps_state(eng, gd)
    assert np.isfinite(eng.grad_norms()["total"])
    assert _same_bits(b, base, mask)


@pytest.mark.parametrize("algo", ["norm", "value"])
def test_flat_and_tiled_adam_stay_bit_identical_with_clipping_active(engines, algo):
    eng = engines("bf16")
    mask = _listed_mask(eng)
    gd, gh = two_draws(eng)
    _, n2 = np_norms(eng, gh[1].astype(np.float64))
    limit = 2.0 * n2 if algo == "norm" else float(np.median(np.abs(gh[1][mask])))
    out = {}
    try:
        for fuse in (0, 1):
            _reset(engines, eng)
            eng.set_option("adam_fused_transposes", fuse)
            eng.set_grad_clip(algo, limit)
            out[fuse] = _two_steps_state(eng, gd, "adam", wd=1e-2)
    finally:
        eng.set_option("adam_fused_transposes", 1)
    assert _same_bits(out[0], out[1], mask)


# ---------------------------------------------------------------------------------------------------------------- 8: clipping by value
@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_clipping_by_value_matches_torch(engines, opt):
    """clip_grad_value_ + SGD / Adam with weight_decay 1e-2 (the clamp comes BEFORE wd p is added)."""
    eng = engines("fp32" if opt == "sgd" else "bf16")
    _reset(engines, eng)
    P0flat = host(eng.flat_params).astype(np.float64)
    mask = _listed_mask(eng)
    gd, gh = two_draws(eng, first_mult=1.0)
    limit = float(np.median(np.abs(gh[1][mask])))
    for G in gh:
        frac = float((np.abs(G[mask]) > limit).mean())
        print("limit %.3e clamps %.1f %% of the entries" % (limit, 100 * frac))
        assert 0.2 <= frac <= 0.8
    eng.set_grad_clip("value", limit)
    lr = 1.0 if opt == "sgd" else 1e-3
    got = run_engine(eng, gd, opt, lr, wd=1e-2)
    ref = torch_ref(eng, P0flat, gh, opt, lr, clip=("value", limit), wd=1e-2)
    ctrl = torch_ref(eng, P0flat, gh, opt, lr, clip=None, wd=1e-2)
    if opt == "sgd":
        assert sgd_gates(eng, P0flat, got, ref, "clamped reference")
        assert not sgd_gates(eng, P0flat, got, ctrl, "negative control (unclamped reference)")
    else:
        # a clamped entry is +-limit >> 1e-5, an unclamped one keeps its value: the strict share is that of the raw draw
        assert float((np.abs(gh[1][mask]) > 1e-5).mean()) >= 0.99
        g2c = np.clip(gh[1], -limit, limit)
        assert adam_gates(eng, got, ref, g2c, lr, "clamped reference", mask)
        assert not adam_gates(eng, got, ctrl, g2c, lr, "negative control (unclamped reference)", mask)


# ---------------------------------------------------------------------------------------------------------------- 9: fp16
def test_fp16_unscales_before_clipping_and_a_skipped_step_stays_skipped(engines):
    lr, scale = 1e-3, 1024.0
    eng = engines("fp16")
    _reset(engines, eng, scale=scale)
    P0flat = host(eng.flat_params).astype(np.float64)
    mask = _listed_mask(eng)
    gd, gh = two_draws(eng)                                   # the UNSCALED gradients; run_engine writes them x 1024 (a power of two: exact)
    _, n2 = np_norms(eng, gh[1].astype(np.float64))
    limit = 2.0 * n2
    eng.set_grad_clip("norm", limit)
    got = run_engine(eng, gd, "adam", lr, scale=scale)
    check_norms(eng, gh[1])                                   # the reported norm is that of the unscaled gradients
    st = eng.scaler_state()
    assert st["taken_steps"] == 2 and st["skipped_steps"] == 0 and st["scale"] == scale
    ref = torch_ref(eng, P0flat, gh, "adam", lr, clip=("norm", limit))
    assert adam_gates(eng, got, ref, gh[1], lr, "clipped reference", mask)
    ctrl = torch_ref(eng, P0flat, gh, "adam", lr, clip=None)
    assert not adam_gates(eng, got, ctrl, gh[1], lr, "negative control (unclipped reference)", mask)
    # one inf planted in a tensor: the norm pass itself raises found_inf (no separate check runs), the step is skipped
    before = dict(p=eng.flat_params.clone(), m=eng.adam_m.clone(), v=eng.adam_v.clone())
    bad = torch.where(gd[1] == PAD, gd[1], gd[1] * scale)
    off = eng.layout["plan_proposal.fc_model.2.weight"][0]
    bad[off + 12345] = float("inf")
    eng.flat_grads.copy_(bad)
    eng.adam_step(lr=lr)
    torch.cuda.synchronize()
    st2 = eng.scaler_state()
    assert st2["last_found_inf"] == 1 and st2["skipped_steps"] == 1 and st2["taken_steps"] == 2 and st2["scale"] == scale * 0.5
    for k, t in (("p", eng.flat_params), ("m", eng.adam_m), ("v", eng.adam_v)):
        assert torch.equal(before[k], t), k
    assert not np.isfinite(eng.grad_norms()["total"])         # whatever IEEE gives; not used
    # and the next finite step is taken again
    eng.flat_grads.copy_(torch.where(gd[1] == PAD, gd[1], gd[1] * (scale * 0.5)))
    eng.adam_step(lr=lr)
    st3 = eng.scaler_state()
    assert st3["taken_steps"] == 3 and st3["last_found_inf"] == 0
    check_norms(eng, gh[1])


# ---------------------------------------------------------------------------------------------------------------- 11: module level
def _build_module(precision="bf16"):
    from hulc_amd import config
    cfg = config.compose(os.path.join(ROOT, "conf"), "config", ["model=hulc", f"trainer.precision={precision}", "datamodule.batch_size=4"])
    return config.instantiate(cfg.model, device="cuda:0", max_seq_len=32)


def test_trainer_clips_and_logs_gradient_norms(tmp_path):
    """Trainer.fit with clipping by norm and tracking on: EVERY history record's grad_2.0_norm_total and per-tensor norms against numpy fp64 of the gradient
    buffer of that very step (item 4's gate).  The buffer is copied inside the Trainer's own run, between training_step and the optimizer kernel: the
    engine's adam_step / optimizer_step are wrapped for the duration of fit() — never a second run (the backward's atomics make two runs differ)."""
    from hulc_amd import parallel
    from hulc_amd.trainer import SyntheticDataModule, Trainer
    dm = SyntheticDataModule(batch_size=4, max_window_size=8, modalities=["vis", "lang"], steps_per_epoch=3, seed=3)
    kw = dict(max_steps=3, gradient_clip_val=0.05, track_grad_norm=2, log_every=1, log_dir=str(tmp_path))
    model = _build_module()
    eng = model.engine
    snaps = []

    def snapshotting(fn):
        def call(*a, **k):
            snaps.append(host(eng.flat_grads).copy())         # what this optimizer step is about to consume
            return fn(*a, **k)
        return call
    eng.adam_step, eng.optimizer_step = snapshotting(eng.adam_step), snapshotting(eng.optimizer_step)
    tr = Trainer(**kw)
    hist = tr.fit(model, dm)
    names = [n for n, _ in model.named_parameters()]
    assert len(hist) == 3 and len(snaps) == 3
    for i, rec in enumerate(hist):
        per = {k[len("grad_2.0_norm/"):]: v for k, v in rec.items() if k.startswith("grad_2.0_norm/")}
        assert set(per) == set(names) and len(names) == len(per)                                 # exactly the named_parameters() names
        _, _, tot = check_norms(eng, snaps[i], got=dict(total=rec["grad_2.0_norm_total"], per_tensor=per))
        assert rec["grad_clip_coef"] < 1.0 and rel(rec["grad_clip_coef"], 0.05 / (tot + 1e-6)) <= 1e-5      # clipping is active (first-step norms of this model are ~ 10)
    eng.close()
    # a caller who drives the optimizer by hand reads the same numbers through FusedAdam.grad_norm
    model = _build_module()
    tr2 = Trainer(**kw)
    tr2.rank, tr2.world, tr2.local = parallel.init_from_env()
    tr2.datamodule = dm
    model.trainer = tr2
    oc = model.configure_optimizers()
    opt, sched = oc["optimizer"], oc["lr_scheduler"]["scheduler"]
    assert tr2._configure_grad_clip(model)
    model.on_fit_start()
    model.train()
    eng = model.engine
    for bi, batch in enumerate(dm.train_dataloader(0)):
        model.training_step(batch, bi)
        Gh = host(eng.flat_grads).copy()
        opt.step()
        sched.step()
        got, _, tot = check_norms(eng, Gh, got=opt.grad_norm(per_tensor=True))
        assert got["coef"] < 1.0 and rel(got["coef"], 0.05 / (tot + 1e-6)) <= 1e-5
    eng.close()


def _dp_worker(rank, world, port, out, log_dir):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "oracle"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    os.environ["HULC_DP_COMM"] = "auto"
    import torch.distributed as dist
    from hulc_amd import parallel
    from hulc_amd.trainer import SyntheticDataModule, Trainer
    parallel.init_from_env("gloo")
    model = _build_module("fp32")
    dm = SyntheticDataModule(batch_size=4, max_window_size=8, modalities=["vis", "lang"], steps_per_epoch=2, seed=3)
    tr = Trainer(max_steps=2, gradient_clip_val=0.05, log_every=1, log_dir=log_dir)
    tr.fit(model, dm)
    gn = model.engine.grad_norms()
    import hashlib
    eng = model.engine
    p = host(eng.flat_params)[_listed_mask(eng)]              # every listed element of the parameter buffer
    out[rank] = (gn["total"], gn["coef"], (hashlib.sha256(p.tobytes()).hexdigest(), int(p.size), bool(np.isfinite(p).all())), len(tr.history))
    model.engine.close()
    dist.destroy_process_group()


def test_two_ranks_derive_the_same_coefficient(tmp_path):
    """The norm is taken inside the optimizer step, behind the all-reduce: both ranks (different batches) report the same total and coefficient and hold
    identical parameters afterwards, with no collective of its own."""
    import torch.multiprocessing as mp
    out = mp.Manager().dict()
    try:
        mp.spawn(_dp_worker, args=(2, 29200 + os.getpid() % 100, out, str(tmp_path)), nprocs=2, join=True)
    except Exception as e:                      # a torch build whose gloo cannot reduce device tensors
        msg = str(e).lower()
        if "gloo" in msg and ("allreduce" in msg or "all_reduce" in msg or "all-reduce" in msg):
            pytest.skip(f"gloo cannot all-reduce device tensors here: {e}")
        raise
    (t0, c0, w0, h0), (t1, c1, w1, h1) = out[0], out[1]
    assert t0 == t1 and c0 == c1 and c0 < 1.0 and np.isfinite(t0)
    assert w0 == w1 and w0[1] > 40e6 and w0[2]                # identical bits in all 47 M parameters, all finite
    assert h0 == 2 and h1 == 0                  # only rank 0 reads the norms back for its log
