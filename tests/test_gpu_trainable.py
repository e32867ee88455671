"""GPU (-m gpu): frozen parameters — the per-tensor trainable mask from the kernels up to the module (include/hulc_hip.h hulc_trainable_set / _get /
_steps_set; csrc/engine_trainable.inc; kernels.h adam_grouped_kernel / sgd_grouped_kernel; Hulc.freeze_modules; FusedAdam.state_dict).

Every engine is fixture sized: 2 windows per modality (one paired pass of 4), S = 4, spec.init_all parameters with ln_jitter (no parameter is exactly zero).
The parameters and the two batches are made once and never written.  Bounds: bit equality wherever the issue asks for it; golden_util.adam_close for the
per-tensor step count (the bound of the optimizer fixtures); rel 1e-5 for the norms (test_gpu_grad_clip.py's gate: <= 25 u per chunk sum, halved by the root).

"changed" for a trainable element means its parameter OR its second moment differs from the initial value: three AdamW steps always move one of the two
(a non-zero gradient makes exp_avg_sq positive; with all-zero gradients the decoupled decay alone shrinks a non-zero parameter), whereas the parameter
alone can come back to its initial bits when three updates cancel."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from bench import synth_batch  # noqa: E402
from golden_util import adam_close  # noqa: E402
from hulc_amd import spec  # noqa: E402
from hulc_amd.engine import StepEngine  # noqa: E402

DIMS = spec.ModelDims(kind="hulc", max_window=32, use_clip=True)
NAMES = [n for n, _, _ in spec.param_table(DIMS)]
LONE_BIAS = "plan_proposal.fc_model.0.bias"
TILED = "action_decoder.rnn.weight_hh_l0"
ENC = [n for n in NAMES if n.startswith("perceptual_encoder.")]
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


def make(dtype, repro=False, load=True):
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible — the product path has no CPU fallback")
    eng = StepEngine(DIMS, 4, 4, dtype=dtype, device="cuda:0", dropout_p=0.1, seed=3)
    if dtype == "fp16":
        eng.scaler_enable(init_scale=1024.0)
    if load:
        eng.load_numpy(params())
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


def freeze(eng, frozen):
    eng.set_trainable({n: False for n in frozen})


def state(eng):
    torch.cuda.synchronize()
    return eng.flat_params.clone(), eng.adam_m.clone(), eng.adam_v.clone()


def view(eng, flat, name):
    off, shape = eng.layout[name]
    k = int(np.prod(shape)) if len(shape) else 1
    return flat[off:off + k]


def same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ refusals on a live context
def test_refusals_on_a_live_context():
    eng = make("fp32", load=False)
    with pytest.raises(RuntimeError, match="hulc_trainable_set before hulc_bind_params"):
        eng.set_trainable([True] * len(NAMES))
    eng.load_numpy(params())
    p0, m0, v0 = state(eng)
    short = np.ones(len(NAMES) - 1, np.uint8)
    assert eng.lib.hulc_trainable_set(eng.ctx, len(short), short.ctypes.data) != 0
    assert eng.lib.hulc_last_error() == b"hulc_trainable_set: %d entries, %d tensors are bound" % (len(NAMES) - 1, len(NAMES))
    assert all(eng.trainable().values()) and not any(eng.frozen_steps().values())
    # a ninth distinct frozen-step count among the trainable tensors: refused, names the limit, changes nothing
    nine = NAMES[10:19]
    freeze(eng, nine)
    for i, n in enumerate(nine):
        eng.adam_step()                                    # zero gradients: the steps only count
        if i < 7:
            eng.set_trainable({n: True})                   # sat out i + 1 steps
        elif i == 7:
            with pytest.raises(RuntimeError, match="9 distinct frozen-step counts, the limit is 8"):
                eng.set_trainable({n: True})
    tr, fs = eng.trainable(), eng.frozen_steps()
    assert [tr[n] for n in nine] == [True] * 7 + [False, False]
    assert [fs[n] for n in nine] == [1, 2, 3, 4, 5, 6, 7, 9, 9] and fs[NAMES[0]] == 0
    p1, _, _ = state(eng)
    assert same(p0, p1)                                    # zero gradients, no decay: nothing moved
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 1. frozen means untouched
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_frozen_means_untouched(dtype):
    eng = make(dtype)
    frozen = [n for n in NAMES if n.startswith("perceptual_encoder.") or n.startswith("language_goal.")] + [LONE_BIAS, TILED]
    freeze(eng, frozen)
    assert eng.trainable() == {n: n not in frozen for n in NAMES}
    p0, m0, v0 = state(eng)
    for step in range(3):
        fwd_bwd(eng, step)
        eng.optimizer_step("adamw", weight_decay=0.01)
    p1, m1, v1 = state(eng)
    if dtype == "fp16":
        assert eng.scaler_state()["taken_steps"] == 3
    for n in frozen:
        assert same(view(eng, p0, n), view(eng, p1, n)) and same(view(eng, m0, n), view(eng, m1, n)) and same(view(eng, v0, n), view(eng, v1, n)), n
    i = NAMES.index(LONE_BIAS)
    neighbours = [NAMES[i - 1], NAMES[i + 1]]
    assert not set(neighbours) & set(frozen)
    for n in NAMES:
        if n in frozen:
            continue
        moved = (view(eng, p0, n) != view(eng, p1, n)) | (view(eng, v0, n) != view(eng, v1, n))
        assert bool(moved[0]) and bool(moved[-1]), n       # segment edges: the first and the last element of every trainable tensor
        assert not torch.equal(view(eng, p0, n), view(eng, p1, n)), n
        if n in neighbours:                                # the tensors on both sides of the lone frozen bias: every element, up to the padding
            assert bool(moved.all()), (n, int((~moved).sum()))
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 2. all frozen is a no-op
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_all_frozen_is_a_noop(dtype):
    eng = make(dtype, repro=True)                          # the forward's sums in a fixed order: equal weights give equal bits
    freeze(eng, NAMES)
    p0, m0, v0 = state(eng)
    first = fwd_bwd(eng, 5)
    eng.optimizer_step("adamw", weight_decay=0.01)
    p1, m1, v1 = state(eng)
    assert same(p0, p1) and same(m0, m1) and same(v0, v1)
    assert fwd(eng, 5) == first                            # the 16-bit shadow, the transposed and the fragment-ordered copies still belong to these parameters
    # the caller's step count went on by one and every tensor sat that step out; under the loss scaler the device counts the steps TAKEN, and this was none
    assert all(v == (0 if dtype == "fp16" else 1) for v in eng.frozen_steps().values())
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 3. pruning cuts nothing that is needed
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_pruned_backward_leaves_the_trainable_tensors_bit_identical(dtype):
    out = []
    for frozen in (ENC, []):
        eng = make(dtype, repro=True)
        eng.set_grad_clip("off", None)
        if frozen:
            freeze(eng, frozen)
        fwd_bwd(eng, 0)
        eng.optimizer_step("adamw", weight_decay=0.01)
        out.append(state(eng))
        lay = eng
        assert eng.get_option("nondeterministic_sites") == 0
        eng.close()
    (pa, ma, va), (pb, mb, vb) = out
    for n in NAMES:
        if n in ENC:
            continue
        assert same(view(lay, pa, n), view(lay, pb, n)) and same(view(lay, ma, n), view(lay, mb, n)) and same(view(lay, va, n), view(lay, vb, n)), n
    assert not same(view(lay, pa, ENC[0]), view(lay, pb, ENC[0]))      # the unfrozen context did train its encoders


# ------------------------------------------------------------------------------------------------------------------ 4. per-tensor step count
@pytest.mark.parametrize("opt", ["adam", "adamw", "sgd"])
def test_per_tensor_step_count_against_torch_optim(opt):
    """visual_goal sits out steps 1 and 2 and joins at step 3: its bias corrections (SGD: its first-step rule) must be those of ITS step 1 and 2.  The
    reference is torch.optim on the CPU in float64, fed the engine's own read-back gradients, .grad = None while the tensor is frozen — on visual_goal.*
    and, as tensors that never froze, language_goal.* and plan_proposal.fc_state.0.* (the whole table in float64 would take most of a minute)."""
    eng = make("fp32")
    vg = [n for n in NAMES if n.startswith("visual_goal.")]
    watch = vg + [n for n in NAMES if n.startswith("language_goal.") or n.startswith("plan_proposal.fc_state.0.")]
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    lr, wd = (1e-2, 0.0) if opt == "sgd" else (2e-4, 0.01 if opt == "adamw" else 0.0)
    ref = {n: torch.nn.Parameter(torch.from_numpy(params()[n].astype(np.float64).reshape(-1))) for n in watch}
    if opt == "sgd":
        o = torch.optim.SGD(list(ref.values()), lr=f32(lr), momentum=f32(0.9))
    else:
        cls = torch.optim.AdamW if opt == "adamw" else torch.optim.Adam
        o = cls(list(ref.values()), lr=f32(lr), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8), weight_decay=f32(wd))
    freeze(eng, vg)
    for step in range(1, 5):
        if step == 3:
            eng.set_trainable({n: True for n in vg})
            assert all(eng.frozen_steps()[n] == 2 for n in vg) and eng.frozen_steps()[watch[-1]] == 0
        fwd_bwd(eng, step)
        torch.cuda.synchronize()
        G = {n: view(eng, eng.flat_grads, n).cpu().numpy().copy() for n in watch}
        eng.optimizer_step(opt, lr=lr, weight_decay=wd, momentum=0.9 if opt == "sgd" else 0.0)
        for n in watch:
            ref[n].grad = None if (step <= 2 and n in vg) else torch.from_numpy(G[n].astype(np.float64))
        o.step()
        torch.cuda.synchronize()
        worst = 0.0
        for n in watch:
            got = view(eng, eng.flat_params, n).cpu().numpy()
            want = ref[n].detach().numpy()
            worst = max(worst, float(np.abs(got - want).max()))
            assert adam_close(got, want, G[n], lr=lr), (opt, step, n, float(np.abs(got - want).max()))
            if step <= 2 and n in vg:
                assert np.array_equal(got, params()[n].reshape(-1)), n
        print("%s step %d: worst |p - ref| %.3e" % (opt, step, worst))
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 5. norm and clip
def test_norm_and_clip_cover_the_trainable_tensors_only():
    eng = make("bf16")
    frozen = [n for n in NAMES if n.startswith("language_goal.")] + [LONE_BIAS, TILED]
    freeze(eng, frozen)
    eng.set_grad_clip("norm", 0.05, track=True)
    fwd_bwd(eng, 0)
    torch.cuda.synchronize()
    G = eng.flat_grads.cpu().numpy().astype(np.float64)
    eng.optimizer_step("adamw", weight_decay=0.01)
    got = eng.grad_norms(per_tensor=True)
    sq = {n: float(np.dot(view(eng, G, n), view(eng, G, n))) for n in NAMES}
    tot = float(np.sqrt(sum(v for n, v in sq.items() if n not in frozen)))
    tot_all = float(np.sqrt(sum(sq.values())))
    print("total %.9g, fp64 of the trainable tensors %.9g (rel %.2e), fp64 of all tensors %.9g" % (got["total"], tot, abs(got["total"] - tot) / tot, tot_all))
    assert abs(got["total"] - tot) <= 1e-5 * tot
    assert abs(tot_all - tot) > 1e-3 * tot                 # control: the frozen tensors' gradients would have shown
    for n in NAMES:
        if n in frozen:
            assert got["per_tensor"][n] == 0.0, n
        elif sq[n] > 0:
            assert abs(got["per_tensor"][n] - np.sqrt(sq[n])) <= 1e-5 * np.sqrt(sq[n]), n
    assert tot > 0.05 and abs(got["coef"] - 0.05 / (tot + 1e-6)) <= 1e-5 * got["coef"]
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 6. fp16 non-finite check
@pytest.mark.parametrize("track", [False, True])
def test_fp16_nonfinite_check_reads_the_trainable_gradients_only(track):
    eng = make("fp16")
    frozen = [n for n in NAMES if n.startswith("language_goal.")]
    freeze(eng, frozen)
    eng.set_grad_clip("off", None, track=track)            # track: the check rides on the norm pass; off: it is a pass of its own
    fwd_bwd(eng, 0)
    view(eng, eng.flat_grads, frozen[0])[3] = float("inf")
    p0, _, _ = state(eng)
    eng.optimizer_step("adamw", weight_decay=0.01)
    st = eng.scaler_state()
    assert st == dict(scale=1024.0, growth_tracker=1, skipped_steps=0, last_found_inf=0, taken_steps=1), st
    p1, m1, _ = state(eng)
    assert not same(p0, p1) and same(view(eng, p0, frozen[0]), view(eng, p1, frozen[0]))
    fwd_bwd(eng, 1)
    view(eng, eng.flat_grads, "visual_goal.mlp.0.weight")[3] = float("inf")
    eng.optimizer_step("adamw", weight_decay=0.01)
    st = eng.scaler_state()
    assert st == dict(scale=512.0, growth_tracker=0, skipped_steps=1, last_found_inf=1, taken_steps=1), st
    p2, m2, _ = state(eng)
    assert same(p1, p2) and same(m1, m2)                   # skipped, as without a mask
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 7. encoder backward is gone
def _classes(t):
    return {k for k, v in t.items() if v["launches"] > 0}


def test_encoder_backward_is_not_run_when_the_encoders_are_frozen():
    eng = make("bf16")
    eng.timers_enable(True)

    def parts():
        eng.zero_grads()
        fwd(eng, 0)
        eng.timers_read(reset=True)
        assert eng.lib.hulc_backward_part(eng.ctx, 0) == 0
        t0 = _classes(eng.timers_read(reset=True))
        assert eng.lib.hulc_backward_part(eng.ctx, 1) == 0, eng.lib.hulc_last_error()
        t1 = _classes(eng.timers_read(reset=True))
        return t0, t1

    u0, u1 = parts()
    part1_only = u1 - u0
    assert part1_only, (u0, u1)                            # the unfrozen step does report encoder-only classes
    freeze(eng, ENC)
    f0, f1 = parts()
    assert not f1, f1                                      # part 1 launched nothing
    assert not (f0 & part1_only), f0 & part1_only
    eng.zero_grads()
    fwd(eng, 1)
    eng.timers_read(reset=True)
    eng.backward()
    whole = _classes(eng.timers_read(reset=True))
    assert not (whole & part1_only), whole & part1_only
    eng.optimizer_step("adamw", weight_decay=0.01)         # and the step goes on from there
    fwd_bwd(eng, 2)
    torch.cuda.synchronize()
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 8. module surface
def _module(**kw):
    from hulc_amd.hulc import Hulc
    return Hulc(precision="bf16", max_batch_size=2, max_seq_len=4, seed=5, **kw)


def _dm(steps):
    from hulc_amd.trainer import SyntheticDataModule
    return SyntheticDataModule(batch_size=2, max_window_size=4, steps_per_epoch=steps, seed=3)


def test_module_flags_freeze_modules_and_freeze():
    m = _module()
    opt = m.configure_optimizers()["optimizer"]
    batch = next(iter(_dm(1).train_dataloader()))
    P = dict(m.named_parameters())
    assert all(p.grad is not None for p in P.values())

    def step():
        before = {n: p.detach().clone() for n, p in P.items()}
        m.training_step(batch, 0)
        opt.step()
        torch.cuda.synchronize()
        return {n for n, p in P.items() if not torch.equal(before[n], p.detach())}

    # requires_grad_(False) on the parameters themselves
    for n, p in P.items():
        if n.startswith("visual_goal."):
            p.requires_grad_(False)
    moved = step()
    assert not any(n.startswith("visual_goal.") for n in moved) and "plan_proposal.fc_model.0.weight" in moved and ENC[0] in moved
    assert all((p.grad is None) == n.startswith("visual_goal.") for n, p in P.items())
    assert m.engine.trainable() == {n: not n.startswith("visual_goal.") for n in P}
    # freeze_modules / unfreeze_modules
    m.unfreeze_modules("visual_goal")
    m.freeze_modules(["perceptual_encoder", "language_goal"])
    moved = step()
    assert not any(n.startswith(("perceptual_encoder.", "language_goal.")) for n in moved) and "visual_goal.mlp.0.weight" in moved
    assert all((p.grad is None) == n.startswith(("perceptual_encoder.", "language_goal.")) for n, p in P.items())
    with pytest.raises(KeyError):
        m.freeze_modules("perceptual_encoderx")
    # LightningModule.freeze / unfreeze
    m.freeze()
    assert not any(p.requires_grad for p in P.values()) and not m._train_mode
    m.train()
    assert step() == set() and all(p.grad is None for p in P.values())
    m.unfreeze()
    assert all(p.requires_grad for p in P.values()) and m._train_mode
    moved = step()
    assert {"visual_goal.mlp.0.weight", "language_goal.mlp.1.weight", "plan_proposal.fc_model.0.weight", ENC[0]} <= moved and all(p.grad is not None for p in P.values())
    sd = opt.state_dict()
    assert all(sd["trainable"].values()) and sd["frozen_steps"]["visual_goal.mlp.0.weight"] == 2 and sd["frozen_steps"][ENC[0]] == 2
    assert sd["frozen_steps"]["plan_proposal.fc_model.0.weight"] == 1 and sd["step"] == 4
    m.engine.close()
    # the constructor argument
    m2 = _module(freeze_modules=["perceptual_encoder"])
    assert {n for n, p in m2.named_parameters() if not p.requires_grad} == set(ENC) and m2.engine.trainable() == {n: n not in ENC for n in NAMES}
    m2.engine.close()


class _Thaw:
    """visual_goal joins at the start of epoch 1."""

    def on_train_epoch_start(self, trainer, module):
        if trainer.current_epoch == 1:
            module.unfreeze_modules("visual_goal")


def test_checkpoint_resume_of_a_frozen_run_is_bit_identical(tmp_path):
    from hulc_amd.trainer import ModelCheckpoint, Trainer

    def run(log_dir, epochs, ckpt=None):
        m = _module(freeze_modules=["perceptual_encoder", "visual_goal"])
        tr = Trainer(max_epochs=epochs, log_dir=str(log_dir), callbacks=[_Thaw(), ModelCheckpoint()], limit_val_batches=0, log_every=1000, deterministic=True)
        tr.fit(m, _dm(2), ckpt_path=ckpt)
        torch.cuda.synchronize()
        out = (m.engine.flat_params.clone(), m.engine.adam_m.clone(), m.engine.adam_v.clone(), m.engine.frozen_steps(), m.engine.trainable())
        m.engine.close()
        return out

    whole = run(tmp_path / "a", 2)
    run(tmp_path / "b", 1)
    ckpt = tmp_path / "b" / "saved_models" / "epoch=0.ckpt"
    assert ckpt.exists()
    ck = torch.load(str(ckpt), map_location="cpu", weights_only=False)["optimizer_states"][0]
    assert ck["frozen_steps"]["visual_goal.mlp.0.weight"] == 2 and not ck["trainable"]["visual_goal.mlp.0.weight"] and ck["trainable"]["language_goal.mlp.1.weight"]
    resumed = run(tmp_path / "b", 2, ckpt=str(ckpt))
    assert whole[3] == resumed[3] and whole[4] == resumed[4]
    assert whole[3]["visual_goal.mlp.0.weight"] == 2 and whole[3][ENC[0]] == 4 and whole[4]["visual_goal.mlp.0.weight"] and not whole[4][ENC[0]]
    for a, b in zip(whole[:3], resumed[:3]):
        assert same(a, b)


# ------------------------------------------------------------------------------------------------------------------ 9. data parallel
def test_all_frozen_bucket_is_not_reduced():
    eng = make("bf16", repro=True)
    eng.comm_init(eng.comm_unique_id(), 0, 1)

    def collectives():
        eng.zero_grads()
        fwd(eng, 0)
        n0 = eng.comm_stats()["collectives"]
        eng.backward_allreduce("fp32")
        torch.cuda.synchronize()
        return eng.comm_stats()["collectives"] - n0

    base = collectives()
    g0 = eng.flat_grads.clone()
    freeze(eng, ENC)
    assert collectives() == base - 1
    for n in NAMES:                                        # a 1-rank SUM: what is still reduced is what the backward wrote
        if n not in ENC:
            assert same(view(eng, g0, n), view(eng, eng.flat_grads, n)), n
    freeze(eng, [n for n in NAMES if n.startswith(("visual_goal.", "language_goal."))])
    assert collectives() == base - 1                       # encoders and goal encoders frozen: two buckets less, the skip vote travels as a word of its own
    eng.set_trainable({n: True for n in NAMES})
    assert collectives() == base
    # hulc_allreduce_grads: the runs of buckets that are still trained, one collective each
    freeze(eng, [n for n in NAMES if n.startswith("plan_recognition.")])
    fwd_bwd(eng, 1)
    n0 = eng.comm_stats()["collectives"]
    eng.allreduce_grads("fp32")
    torch.cuda.synchronize()
    assert eng.comm_stats()["collectives"] - n0 == 2
    eng.close()
