"""GPU (-m gpu): averaged weights — the EMA of the parameters from the kernel up to the module and the trainer (include/hulc_hip.h hulc_ema_enable /
_state_get / _state_set / _swap / _swapped, hulc_k_ema_update; csrc/engine_ema.inc; kernels.h ema_update_kernel / ema_count_kernel / ema_swap_kernel;
Hulc.ema_scope; Trainer.validate / save_checkpoint / fit(ckpt_path=...)).

Bounds.  One update is e' = e + w (p - e) in fp32 with the product rounded before the sum: three roundings (the difference, the product, the sum), each of a
quantity no larger than |e| + |p| in magnitude, so |e' - fp64| <= 3 * 2^-24 (|e| + |p|) < 2^-22 (|e| + |p|) per element — derived, not measured.  Over k
steps the errors add (each later step shrinks the earlier ones by 1 - w <= 1): k times the bound, taken at the largest |e| + |p| of the k steps; the fp64
reference takes the same fp32 weight the kernel derives (1 - the fp32 decay of spec.ema_decay_at).  Everything else is bit equality.

Every engine is fixture sized: 2 windows per modality (one paired pass of 4), S = 4; the parameters and the two batches are made once and never written."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from bench import synth_batch  # noqa: E402
from hulc_amd import lib as L  # noqa: E402
from hulc_amd import spec  # noqa: E402
from hulc_amd.engine import StepEngine  # noqa: E402

DIMS = spec.ModelDims(kind="hulc", max_window=32, use_clip=False)
NAMES = [n for n, _, _ in spec.param_table(DIMS)]
ENC = [n for n in NAMES if n.startswith("perceptual_encoder.")]
OTHER = "plan_proposal.fc_model.0.weight"
U = 2.0 ** -22                 # the per-update bound's factor (module docstring)
NAN_BITS = 0x7FC00123
_CACHE = {}


def params():
    if "P" not in _CACHE:
        _CACHE["P"] = spec.init_all(DIMS, seed=0, ln_jitter=True)
    return _CACHE["P"]


def batches():
    if "mb" not in _CACHE:
        dev = torch.device("cuda:0")
        _CACHE["mb"] = (synth_batch(2, 4, dev, 7, False, "fp32"), synth_batch(2, 4, dev, 8, True, "fp32"))
    return _CACHE["mb"]


def make(dtype, repro=False, P=None):
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible — the product path has no CPU fallback")
    eng = StepEngine(DIMS, 4, 4, dtype=dtype, device="cuda:0", dropout_p=0.1, seed=3)
    if dtype == "fp16":
        eng.scaler_enable(init_scale=1024.0)
    eng.load_numpy(params() if P is None else P)
    if repro:
        eng.set_option("reproducible", 1)
    return eng


def fwd(eng, step):
    mv, ml = batches()
    lv, ll = eng.forward_loss_pair(mv, ml, 0.5, 3.0, step=step)
    return tuple(sorted(lv.items())), tuple(sorted(ll.items()))


def fwd_bwd(eng, step):
    eng.zero_grads()
    out = fwd(eng, step)
    eng.backward()
    return out


OPT = {"adam": dict(kind="adam"), "adamw": dict(kind="adamw", weight_decay=0.01), "sgd": dict(kind="sgd", lr=1e-3, momentum=0.9)}


def train_step(eng, i, opt="adamw"):
    fwd_bwd(eng, i)
    eng.optimizer_step(**OPT[opt])
    torch.cuda.synchronize()


def view(eng, flat, name):
    off, shape = eng.layout[name]
    k = int(np.prod(shape)) if len(shape) else 1
    return flat[off:off + k]


def bits(t):
    return t.view(torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def w32(n, decay, warmup=True):
    """The fp32 weight 1 - d the kernel derives for update number n: the ramp's quotient in fp64, rounded to fp32, compared with the fp32 decay."""
    d = np.float32(decay)
    if warmup:
        d = min(d, np.float32((1.0 + n) / (10.0 + n)))
    return float(np.float32(1.0) - d)


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel against fp64
def k_update(e, p, w, chunks=None):
    lib = L.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if chunks is None:
        L.check(lib.hulc_k_ema_update(e.data_ptr(), p.data_ptr(), e.numel(), w, None, None, 0, st))
    else:
        cs = torch.tensor([c[0] for c in chunks], dtype=torch.int64, device=e.device)
        cn = torch.tensor([c[1] for c in chunks], dtype=torch.int32, device=e.device)
        L.check(lib.hulc_k_ema_update(e.data_ptr(), p.data_ptr(), e.numel(), w, cs.data_ptr(), cn.data_ptr(), len(chunks), st))
    torch.cuda.synchronize()


def rand_pair(n, seed):
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    e = torch.randn(n, device="cuda:0", generator=g) * torch.exp(torch.randn(n, device="cuda:0", generator=g))      # magnitudes over a few decades
    p = e + torch.randn(n, device="cuda:0", generator=g) * 0.1
    return e, p


def check_close(got, e, p, w):
    ref = e.double() + w * (p.double() - e.double())
    err = (got.double() - ref).abs()
    bound = U * (e.double().abs() + p.double().abs())
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"ema update: n = {got.numel()}, worst error / bound = {worst:.3f}")
    assert bool((err <= bound).all()), worst


@pytest.mark.parametrize("n", [4, 64, 2097152 + 148])
def test_flat_form_against_fp64(n):
    """n = 2 097 152 + 148: one element quad more than a sweep of 2048 blocks x 256 threads x 4 holds, plus a ragged tail of quads — the grid-stride loop takes
    a second trip on some threads only."""
    w = float(np.float32(0.1))
    e, p = rand_pair(n, 11 + n % 7)
    p[n // 2] = e[n // 2]                       # an element that equals its parameter keeps its bits
    e0 = e.clone()
    k_update(e, p, w)
    check_close(e, e0, p, w)
    assert bits(e)[n // 2] == bits(e0)[n // 2]
    assert not same(e, e0)
    if n > 2097152:
        assert not same(e[2097152:], e0[2097152:]) and not same(e[-4:], e0[-4:])      # the second trip ran, to the last quad


def test_chunk_form_against_fp64_and_leaves_the_rest_alone():
    """Chunk lengths 4, 64, 4096 and 4100 with gaps between them.  The gaps of e hold a NaN bit pattern and must keep it; so must a region inside a chunk
    where p == e (signed zeros included).  The chunk form and the flat form give the same bits on the same data."""
    w = float(np.float32(0.25))
    lens, gaps = [4, 64, 4096, 4100], [8, 12, 20, 36, 16]
    chunks, pos = [], gaps[0]
    for ln, gap in zip(lens, gaps[1:]):
        chunks.append((pos, ln))
        pos += ln + gap
    n = pos
    e, p = rand_pair(n, 5)
    listed = torch.zeros(n, dtype=torch.bool, device=e.device)
    for s, ln in chunks:
        listed[s:s + ln] = True
    bits(e)[~listed] = NAN_BITS
    s3 = chunks[2][0]
    p[s3:s3 + 100] = e[s3:s3 + 100]                                   # a frozen region inside a chunk
    e[s3], p[s3] = -0.0, -0.0
    e[s3 + 1], p[s3 + 1] = -0.0, 0.0
    e0 = e.clone()
    k_update(e, p, w, chunks)
    assert torch.equal(bits(e)[~listed], bits(e0)[~listed]) and bool((bits(e)[~listed] == NAN_BITS).all())
    assert torch.equal(bits(e)[s3:s3 + 100], bits(e0)[s3:s3 + 100])
    for s, ln in chunks:
        check_close(e[s:s + ln], e0[s:s + ln], p[s:s + ln], w)
        assert not same(e[s + ln - 4:s + ln], e0[s + ln - 4:s + ln])      # every chunk was walked to its last quad
    s4, l4 = chunks[3]
    flat = e0[s4:s4 + l4].clone()
    k_update(flat, p[s4:s4 + l4].clone(), w)
    assert same(flat, e[s4:s4 + l4])


# ------------------------------------------------------------------------------------------------------------------ 2. the average over steps
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_average_over_three_steps_against_the_fp64_recurrence(dtype):
    eng = make(dtype)
    eng.ema_enable(0.9)
    torch.cuda.synchronize()
    assert same(eng.flat_ema, eng.flat_params) and eng.ema_state()["updates"] == 0 and not eng.ema_swapped
    ref = eng.flat_ema.double()
    bound = torch.zeros_like(ref)
    for i in range(3):
        train_step(eng, i)
        p = eng.flat_params.double()
        bound = torch.maximum(bound, ref.abs() + p.abs())
        ref = ref + w32(i + 1, 0.9) * (p - ref)
    err = (eng.flat_ema.double() - ref).abs()
    worst = float((err / (3 * U * bound).clamp_min(1e-300)).max())
    print(f"ema over 3 steps ({dtype}): worst error / (3 x bound) = {worst:.3f}")
    assert bool((err <= 3 * U * bound).all()), worst
    assert not same(eng.flat_ema, eng.flat_params)
    st = eng.ema_state()
    assert st["updates"] == 3 and st["decay"] == 0.9 and st["start_step"] == 0 and st["warmup"] is True
    assert st["last_decay"] == float(np.float32(4.0 / 13.0))
    assert st["last_decay"] == pytest.approx(spec.ema_decay_at(3, 0.9), rel=1e-6)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 3. the trajectory is untouched
@pytest.mark.parametrize("opt", ["adam", "adamw", "sgd"])
def test_training_trajectory_is_bit_identical_with_the_average_on(opt):
    out = []
    for on in (False, True):
        eng = make("bf16", repro=True)
        if on:
            eng.ema_enable(0.9)
        for i in range(3):
            train_step(eng, i, opt)
        out.append((eng.flat_params.clone(), eng.adam_m.clone(), eng.adam_v.clone()))
        if on:
            assert eng.ema_state()["updates"] == 3 and not same(eng.flat_ema, eng.flat_params)
        eng.close()
    for a, b in zip(*out):
        assert same(a, b)


# ------------------------------------------------------------------------------------------------------------------ 4. a skipped step
def test_skipped_step_leaves_average_and_count_alone():
    eng = make("fp16")
    eng.ema_enable(0.9)
    train_step(eng, 0)
    e1 = eng.flat_ema.clone()
    assert eng.ema_state()["updates"] == 1
    fwd_bwd(eng, 1)
    view(eng, eng.flat_grads, OTHER)[3] = float("inf")
    p1 = eng.flat_params.clone()
    eng.optimizer_step(**OPT["adamw"])
    torch.cuda.synchronize()
    assert eng.scaler_state()["skipped_steps"] == 1 and same(eng.flat_params, p1)
    assert same(eng.flat_ema, e1) and eng.ema_state()["updates"] == 1
    train_step(eng, 2)
    assert eng.scaler_state()["taken_steps"] == 2
    assert not same(eng.flat_ema, e1) and eng.ema_state()["updates"] == 2
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 5. frozen tensors
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_average_of_a_frozen_tensor_is_not_written(dtype):
    eng = make(dtype)
    eng.ema_enable(0.9)
    eng.set_trainable({n: False for n in ENC})
    # a mark in the average of one frozen tensor: the pass must neither read it into a result nor overwrite it
    mark = view(eng, eng.flat_ema, ENC[0])
    bits(mark)[:4] = NAN_BITS
    for i in range(2):
        train_step(eng, i)
    assert bool((bits(view(eng, eng.flat_ema, ENC[0]))[:4] == NAN_BITS).all())
    for n in ENC:
        a, b = view(eng, eng.flat_ema, n), view(eng, eng.flat_params, n)
        assert same(a[4:], b[4:]) if n == ENC[0] else same(a, b), n
    assert not same(view(eng, eng.flat_ema, OTHER), view(eng, eng.flat_params, OTHER))
    assert eng.ema_state()["updates"] == 2
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 6. start_step
def test_start_step_copies_until_it_is_reached():
    eng = make("bf16")
    eng.ema_enable(0.9, start_step=2)
    train_step(eng, 0)
    assert same(eng.flat_ema, eng.flat_params) and eng.ema_state()["updates"] == 1 and eng.ema_state()["last_decay"] == 0.0
    train_step(eng, 1)
    train_step(eng, 2)
    assert not same(eng.flat_ema, eng.flat_params) and eng.ema_state()["updates"] == 3
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 7. swap
def _validate(eng):
    mv, ml = batches()
    out = []
    for mb, lang in ((mv, False), (ml, True)):
        r = eng.validate(mb, lang)
        out.append({k: (v.cpu().numpy().tolist() if torch.is_tensor(v) else np.asarray(v).tolist()) for k, v in r.items()})
    return out


def test_swap_exchanges_the_buffers_and_every_reader_follows():
    eng = make("bf16", repro=True)
    eng.ema_enable(0.9, warmup=False)
    for i in range(2):
        train_step(eng, i)
    p0, e0 = eng.flat_params.clone(), eng.flat_ema.clone()
    assert not same(p0, e0)
    before = fwd(eng, 5)
    val_raw = _validate(eng)
    eng.rollout_envs_init(2)
    mv, ml = batches()
    obs = dict(rgb_static=mv["rgb_static"][:, 0], rgb_gripper=mv["rgb_gripper"][:, 0], robot_obs_raw=mv["robot_obs"][:, 0])
    eng.rollout_envs_plan(obs, ml["lang"], env_ids=[0, 1])
    eng.rollout_envs_act(obs, env_ids=[0, 1])

    eng.ema_swap()
    torch.cuda.synchronize()
    assert eng.ema_swapped and same(eng.flat_params, e0) and same(eng.flat_ema, p0)
    val_avg = _validate(eng)
    assert val_avg != val_raw
    with pytest.raises(RuntimeError, match="has no plan"):      # the slots cached a decoder input term computed from the other weights
        eng.rollout_envs_act(obs, env_ids=[0, 1])
    with pytest.raises(RuntimeError, match="swapped"):
        eng.optimizer_step(**OPT["adamw"])
    with pytest.raises(RuntimeError, match="swapped"):
        eng.adam_step()
    fwd(eng, 6)
    with pytest.raises(RuntimeError, match="swapped"):
        eng.backward()
    with pytest.raises(RuntimeError, match="swapped"):
        eng.backward(0)
    with pytest.raises(RuntimeError, match="swapped"):
        eng.set_trainable({ENC[0]: False})
    with pytest.raises(RuntimeError, match="swapped"):
        eng.ema_enable(0.5)
    torch.cuda.synchronize()
    assert same(eng.flat_params, e0) and same(eng.flat_ema, p0)      # no refusal launched anything
    assert eng.adam_t == 2                                           # ... nor counted as an optimizer step
    # a fresh engine that was handed the averaged weights validates to the same bits
    fresh = make("bf16", repro=True, P={n: v.cpu().numpy() for n, v in eng.views(e0).items()})
    assert _validate(fresh) == val_avg
    fresh.close()

    eng.ema_swap()
    torch.cuda.synchronize()
    assert not eng.ema_swapped and same(eng.flat_params, p0) and same(eng.flat_ema, e0)
    assert fwd(eng, 5) == before and _validate(eng) == val_raw
    train_step(eng, 7)                                               # and training goes on
    assert eng.ema_state()["updates"] == 3 and not same(eng.flat_params, p0)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 8. module and trainer
def _module(**kw):
    from hulc_amd.hulc import Hulc
    return Hulc(precision="bf16", max_batch_size=2, max_seq_len=4, seed=5, **kw)


def _dm(steps):
    from hulc_amd.trainer import SyntheticDataModule
    return SyntheticDataModule(batch_size=2, max_window_size=4, steps_per_epoch=steps, seed=3)


def test_module_scope_checkpoint_resume_and_validation(tmp_path, capsys):
    from hulc_amd.trainer import ModelCheckpoint, Trainer

    def run(log_dir, epochs, ckpt=None, **kw):
        m = _module(**kw)
        tr = Trainer(max_epochs=epochs, log_dir=str(log_dir), callbacks=[ModelCheckpoint()], log_every=1000, deterministic=True)
        tr.fit(m, _dm(2), ckpt_path=ckpt)
        torch.cuda.synchronize()
        return m, tr

    m, tr = run(tmp_path / "a", 2, ema_decay=0.99)
    whole = (m.engine.flat_params.clone(), m.engine.flat_ema.clone())
    assert m.engine.ema_state()["updates"] == 4 and not m.engine.ema_swapped and len(tr.val_history) == 2
    pnames = [n for n, _ in m.named_parameters()]
    ck = torch.load(str(tmp_path / "a" / "saved_models" / "epoch=1.ckpt"), map_location="cpu", weights_only=False)
    es = ck["ema_state"]
    assert list(es["params"]) == pnames and set(pnames) <= set(ck["state_dict"])
    assert es["updates"] == 4 and es["decay"] == 0.99 and es["start_step"] == 0 and es["warmup"] is True
    raw = m.state_dict()
    for n in pnames:      # the checkpoint's state_dict is the raw weights, its ema_state the averaged ones
        assert torch.equal(ck["state_dict"][n], raw[n].cpu()) and torch.equal(es["params"][n], view(m.engine, m.engine.flat_ema, n).view(raw[n].shape).cpu()), n
    assert any(not torch.equal(es["params"][n], ck["state_dict"][n]) for n in pnames)
    # ema_scope: state_dict() follows the swap, also when the body raises
    with m.ema_scope():
        assert m.engine.ema_swapped
        inside = m.state_dict()
        with pytest.raises(RuntimeError, match="swapped"):
            m.configure_optimizers()["optimizer"].step()
    assert all(torch.equal(inside[n].cpu(), es["params"][n]) for n in pnames)
    with pytest.raises(KeyError):
        with m.ema_scope():
            raise KeyError("from the body")
    assert not m.engine.ema_swapped and all(torch.equal(m.state_dict()[n], raw[n]) for n in pnames)
    last_val, gstep = tr.val_history[-1], m.global_step
    m.engine.close()

    # stopped after epoch 1 and resumed from its checkpoint: the same bits as the uninterrupted run
    m1, _ = run(tmp_path / "b", 1, ema_decay=0.99)
    m1.engine.close()
    m2, _ = run(tmp_path / "b", 2, ckpt=str(tmp_path / "b" / "saved_models" / "epoch=0.ckpt"), ema_decay=0.99)
    assert same(m2.engine.flat_params, whole[0]) and same(m2.engine.flat_ema, whole[1]) and m2.engine.ema_state()["updates"] == 4
    m2.engine.close()

    # the validation of the last epoch ran on the averaged weights: a module that is handed them reports the same metrics
    f = _module()
    f.engine.set_option("reproducible", 1)
    f.load_state_dict(es["params"])
    f.global_step = gstep
    assert not f.ema_enabled
    with f.ema_scope():                                              # a module without the average passes through
        assert not f.engine.ema_swapped
    got = Trainer(deterministic=True).validate(f, _dm(2))
    assert got == last_val and len(got) > 0
    f.engine.close()

    # a module without ema_decay writes no ema_state; resuming it with the average on starts from the loaded weights, with one line
    run(tmp_path / "c", 1)[0].engine.close()
    ckc = tmp_path / "c" / "saved_models" / "epoch=0.ckpt"
    assert "ema_state" not in torch.load(str(ckc), map_location="cpu", weights_only=False)
    capsys.readouterr()
    m3 = _module(ema_decay=0.99)
    tr3 = Trainer(max_epochs=1, log_dir=str(tmp_path / "c"), log_every=1000, limit_val_batches=0, deterministic=True)
    tr3.fit(m3, _dm(2), ckpt_path=str(ckc))                          # max_epochs reached: no step follows the restore
    torch.cuda.synchronize()
    assert capsys.readouterr().out.count("holds no ema_state") == 1
    assert same(m3.engine.flat_ema, m3.engine.flat_params) and m3.engine.ema_state()["updates"] == 0
    m3.engine.close()
