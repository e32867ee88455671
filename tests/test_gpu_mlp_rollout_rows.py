"""GPU (-m gpu): the recurrence-free row kernels of the 16-bit hulc_rollout_envs_act (csrc/rollout_step.h: env_rnn_layer_kernel<false, .>,
env_heads_sample_kernel<NT, true>) under the feed-forward decoder body, at a row count that fills two 16-row tiles and part of a third, rows on permuted
slots.  Each layer is compared with tests/mlp_decoder_ref.py applied to THAT layer's own device input (only one product's rounding enters; the per-element
bound is tests/gemm_epi_ref.py's for K = 64 / 2048), ReLU decisions exactly away from zero; the actions with the B = 1 rollout (dec_fwd) of the same rows."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import gemm_epi_ref as G  # noqa: E402
import mlp_decoder_ref as R  # noqa: E402
import plan_ln_inputs as PI  # noqa: E402
from mlp_golden_util import BODY  # noqa: E402
from plan_ln_gpu_util import check_tol  # noqa: E402
from hulc_amd import spec  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, SLOTS, H = 37, 48, 2048          # rows of the call (2 full tiles + 5 rows), policy slots, decoder width


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_row_kernels_against_float64_of_their_own_device_inputs(dtype):
    sys.path.insert(0, ROOT)
    from bench import synth_batch
    from hulc_amd.engine import StepEngine
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible — the product path has no CPU fallback")
    dims = spec.ModelDims(kind="hulc", max_window=32, use_clip=False, decoder_body="mlp")
    P = spec.init_all(dims, seed=4, ln_jitter=True)
    eng = StepEngine(dims, SLOTS, 2, dtype=dtype, dropout_p=0.0, seed=1)
    eng.load_numpy(P)
    dev = torch.device("cuda:0")
    mb = synth_batch(N, 2, dev, 3, False)
    rng = np.random.default_rng(11)
    slots = rng.permutation(SLOTS)[:N].astype(np.int32)          # row r of the call steps slot slots[r]
    plan = rng.integers(0, 32, (SLOTS, 32)).astype(np.int32)          # per SLOT
    goal = PI.round_t(rng.standard_normal((SLOTS, 32)).astype(np.float32), dtype).astype(np.float32)
    eng.rollout_envs_init(SLOTS)
    order = rng.permutation(SLOTS)          # installed in two calls and another order than the act call names them
    for part in (order[:20], order[20:]):
        eng.rollout_envs_set_state(part.astype(np.int32), plan[part], goal[part])
    obs = dict(rgb_static=mb["rgb_static"][:, 0].contiguous(), rgb_gripper=mb["rgb_gripper"][:, 0].contiguous(), robot_obs_raw=mb["robot_obs"][:, 0].contiguous())
    u_mix = np.full((N, 6, 10), 0.999, np.float32)
    for r in range(N):
        for d in range(6):
            u_mix[r, d, (r + 3 * d) % 10] = 0.0          # a Gumbel gap of ~13.9 in favour of one component: rounding cannot change the choice
    u_act = np.linspace(0.2, 0.8, N * 6, dtype=np.float32).reshape(N, 6)
    act = eng.rollout_envs_act(obs, env_ids=slots, u_mix=u_mix, u_act=u_act)
    emb = eng.get_tensor("emb", N * 128).astype(np.float64).reshape(N, 128)
    T = {k: eng.get_tensor(k, N * H).astype(np.float64).reshape(N, H) for k in ("dec_a0", "dec_a1", "dec_y")}
    act2 = eng.rollout_envs_act(obs, env_ids=slots, u_mix=u_mix, u_act=u_act)
    assert np.array_equal(act, act2), "a second step with the same inputs: no state"
    assert all(np.isfinite(v).all() for v in T.values()) and np.isfinite(act).all()

    W = {n: PI.round_t(P[n], dtype).astype(np.float64) for n in BODY if n.endswith("weight")}          # the engine's 16-bit shadow of the fp32 parameters
    bias = {n: P[n].astype(np.float64) for n in BODY if n.endswith("bias")}
    kp = dims.dec_plan
    # the per-slot constant of layer 0 (env_plan_store_kernel): bias + the 32 one-hot plan columns + the goal product, 66 fp32 adds in a fixed order
    W0 = W[BODY[0]]
    cols = np.arange(32)[None, :] * 32 + plan[slots]          # [N][32] plan columns of every row's slot
    terms = np.concatenate([np.broadcast_to(bias[BODY[1]], (N, H))[:, None, :], W0[:, cols].transpose(1, 2, 0),
                            goal[slots].astype(np.float64)[:, :, None] * W0[:, kp + 64:kp + 96].T[None]], 1)          # [N][65][H]
    cache, cache_tol = terms.sum(1), 67 * G.EPS32 * np.abs(terms).sum(1)

    def fwd(what, X, Wm, b, got, act_, res=None, extra=0.0):
        ref, tol, pre, ptol = R.stage_fwd(X, Wm, b, dtype, act_, res=res, res_rowmod=0)
        check_tol(np.abs(got - ref), tol + extra, got, ref, f"{what} [{dtype} n={N}]")
        if act_:
            sure = np.abs(pre) > ptol + extra
            frac = float((got > 0).mean())
            assert 0.2 < frac < 0.8 and sure.mean() > 0.99, (what, frac, sure.mean())
            assert np.array_equal((got > 0)[sure], (pre > 0)[sure]), f"{what}: a ReLU decision differs away from zero"

    fwd("a0", emb[:, 64:], np.ascontiguousarray(W0[:, kp:kp + 64]), None, T["dec_a0"], True, res=cache, extra=cache_tol)
    fwd("a1", T["dec_a0"], W[BODY[2]], bias[BODY[3]], T["dec_a1"], True)
    fwd("y", T["dec_a1"], W[BODY[4]], bias[BODY[5]], T["dec_y"], False)
    assert (T["dec_y"] < 0).mean() > 0.2, "the third layer has no ReLU"

    # heads + sampler by row: a row of each tile against the B = 1 rollout, which goes through dec_fwd and the validation sampler.  Gate as in
    # tests/test_gpu_mlp_decoder.py::test_batched_rollout_16bit_equals_the_b1_path: the five 16-bit tensors between the frames and the heads (emb, a0, a1, y,
    # the time-invariant term) each round to half an ulp (a quarter of the type's largest relative ulp: 2^-9 for bf16), x the action range 4
    gate = 5 * (PI.ULP[dtype] / 4) * 4
    for r in (0, 20, 36):
        s = int(slots[r])
        eng.rollout_reset()
        eng.rollout_set_state(plan[s], goal[s])
        one = {k: v[r:r + 1] for k, v in obs.items()}
        b1 = np.asarray(eng.rollout_act(one, u_mix=u_mix[r], u_act=u_act[r])).reshape(7)
        err = np.abs(act[r] - b1).max()
        print(f"   row {r} (slot {s}): max |batched - B=1| {err:.2e} (gate {gate:.2e})")
        assert err <= gate, (r, err)
    eng.close()
