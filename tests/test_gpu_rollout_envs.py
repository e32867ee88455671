"""GPU, through the C-ABI and the module: the batched multi-environment rollout (hulc_rollout_envs_*: N policy slots per context) against the
reference's rollout fixtures, against the existing B = 1 rollout, and for isolation between slots."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from golden_util import load_rollout_case  # noqa: E402
from hulc_amd import spec  # noqa: E402
from hulc_amd.engine import StepEngine  # noqa: E402
from hulc_amd.utils import synthetic  # noqa: E402


def t_(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


# ------------------------------------------------------------------------------------------------ 1. reference fixtures, fp32 engine
def _fixture_case(case):
    """-> dims, P, frames, fx, goal frame index, chain lengths {mode: steps}, replan_freq (None for gcbc: the goal is encoded once per chain)."""
    if case != "rollout_gcbc":
        dims, P, frames, nsteps, replan_freq, fx = load_rollout_case(case)
        return dims, P, frames, fx, nsteps, dict(vis=nsteps, lang=nsteps), replan_freq
    fx = np.load(os.path.join(ROOT, "tests", "golden", "rollout_gcbc.npz"))
    nvis, nlang, seed = (int(v) for v in fx["meta"])
    n = max(nvis, nlang)
    dims = spec.ModelDims(kind="gcbc", max_window=32, use_clip=True)
    P = spec.init_all(dims, seed=seed, ln_jitter=True)
    frames = synthetic.make_batch(1, 1, n + 1, seed=seed, edge_frac=0.0, aux_mask="all")
    return dims, P, frames, fx, n, dict(vis=nvis, lang=nlang), None


@pytest.mark.parametrize("case", ["rollout_hulc", "rollout_mcil", "rollout_gcbc"])
def test_envs_reproduce_reference_rollouts_in_scattered_slots(case):
    """max_envs = 5, rows mapped to slots [4, 0, 2]: slot 4 runs the fixture's vis chain, slot 0 the lang chain, slot 2 the lang chain again starting ONE CALL
    LATER (its replan phase and hidden state never coincide with slot 0's).  Lang and vis replans of one step are separate plan calls, the act is one call over
    all live rows (n changes from call to call), plans and noise are the fixture's.  Every action within 2e-3 of the reference, echoed plans equal.
    gcbc: the reference's GCBC keeps the decoder state across reset(), and its lang fixture was recorded BEHIND the vis chain (test_oracle_val.py); a slot
    that checks the lang chain therefore runs the vis chain first, then hulc_rollout_envs_reset(clear_hidden = 0), then the lang chain — all of it checked."""
    dims, P, frames, fx, gidx, nsteps, replan_freq = _fixture_case(case)
    gcbc, mcil = dims.kind == "gcbc", dims.kind == "mcil"
    pkey = "plan" if mcil else "plan_idx"
    vis = [("vis", t) for t in range(nsteps["vis"])]
    lang = [("lang", t) for t in range(nsteps["lang"])]
    prog = {4: vis, 0: (vis + lang) if gcbc else lang, 2: [None] + ((vis + lang) if gcbc else lang)}
    eng = StepEngine(dims, 5, 2, dtype="fp32", device="cuda:0", seed=3, num_classes=dims.mix_classes)
    eng.load_numpy(P)
    eng.rollout_envs_init(5)
    frame = lambda mode, key, t: frames[mode][key][0, t]
    checked = 0
    for k in range(max(len(p) for p in prog.values())):
        live = [(s, *prog[s][k]) for s in (4, 0, 2) if k < len(prog[s]) and prog[s][k] is not None]
        for s, mode, t in live:
            if gcbc and t == 0 and k > 0 and prog[s][k - 1] is not None:       # chain switch of a gcbc slot: GCBC.reset drops the goal only
                eng.rollout_envs_reset([s], clear_hidden=False)
        for kind in ("lang", "vis"):
            rows = [(s, mode, t) for s, mode, t in live if mode == kind and (t == 0 if gcbc else t % replan_freq == 0)]
            if not rows:
                continue
            obs = dict(rgb_static=t_(np.stack([frame(m, "rgb_static", t) for _, m, t in rows])), rgb_gripper=t_(np.stack([frame(m, "rgb_gripper", t) for _, m, t in rows])))
            if kind == "vis":
                goal = dict(rgb_static=t_(np.stack([frame(m, "rgb_static", gidx) for _, m, _ in rows])), rgb_gripper=t_(np.stack([frame(m, "rgb_gripper", gidx) for _, m, _ in rows])))
            else:
                goal = t_(np.stack([frames["lang"]["lang"][0] for _ in rows]))
            inj = None if gcbc else np.stack([fx[f"{pkey}_{m}"][t][0] for _, m, t in rows])
            plan = eng.rollout_envs_plan(obs, goal, env_ids=[s for s, _, _ in rows], plan=inj)
            if not gcbc:
                assert np.array_equal(plan.cpu().numpy(), inj)
        obs = dict(rgb_static=t_(np.stack([frame(m, "rgb_static", t) for _, m, t in live])), rgb_gripper=t_(np.stack([frame(m, "rgb_gripper", t) for _, m, t in live])),
                   robot_obs_raw=t_(np.stack([frame(m, "robot_obs", t) for _, m, t in live])))
        a = eng.rollout_envs_act(obs, env_ids=[s for s, _, _ in live], u_mix=np.stack([fx[f"u_mix_{m}"][t][0, 0] for _, m, t in live]),
                                 u_act=np.stack([fx[f"u_act_{m}"][t][0, 0] for _, m, t in live]))
        assert a.shape == (len(live), 7)
        for r, (s, m, t) in enumerate(live):
            err = float(np.abs(a[r] - fx[f"actions_{m}"][0, t]).max())
            assert err <= 2e-3, (case, k, s, m, t, err)
            checked += 1
    assert checked == sum(len([x for x in p if x is not None]) for p in prog.values())
    eng.close()


# ------------------------------------------------------------------------------------------------ shared synthetic data (tests 2 - 5)
_DATA = {}


def _data():
    """64 environments x 3 frames of synthetic observations with a language goal each, an injected plan per environment and the sampler noise of test 3."""
    if not _DATA:
        dims = spec.ModelDims(kind="hulc", max_window=32, use_clip=False)
        mb = synthetic.make_batch(0, 64, 3, seed=21, edge_frac=0.0)["lang"]
        rng = np.random.RandomState(5)
        # per row and dimension: u_mix = 0 on ONE component (chosen by the row index), 0.999 on the others — a Gumbel gap of ~13.9 in favour of that component
        # (oracle/hulc_oracle.py:920-931), so that 16-bit rounding of the mixture logits cannot change the discrete choice; u_act in [0.2, 0.8]
        u_mix = np.full((64, 3, 6, 10), 0.999, np.float32)
        for r in range(64):
            for d in range(6):
                u_mix[r, :, d, (r + 3 * d) % 10] = 0.0
        _DATA.update(dims=dims, P=spec.init_all(dims, seed=21, ln_jitter=True), mb=mb, plan=mb["plan_idx"].astype(np.int32), u_mix=u_mix,
                     u_act=rng.uniform(0.2, 0.8, (64, 3, 6)).astype(np.float32), u_any=rng.uniform(0.0, 1.0, (64, 8, 6, 10)).astype(np.float32))
    return _DATA


def _engine(dtype, max_batch=64, seed=3):
    D = _data()
    eng = StepEngine(D["dims"], max_batch, 2, dtype=dtype, device="cuda:0", seed=seed)
    eng.load_numpy(D["P"])
    return eng


def _obs_rows(rows, t, robot=True):
    mb = _data()["mb"]
    o = dict(rgb_static=t_(mb["rgb_static"][rows, t]), rgb_gripper=t_(mb["rgb_gripper"][rows, t]))
    if robot:
        o["robot_obs_raw"] = t_(mb["robot_obs"][rows, t])
    return o


def _b1_rollout(eng, rows, steps=3):
    """The EXISTING B = 1 rollout per environment: plan at step 0 (injected), `steps` acts with the noise of test 3.  -> actions (len(rows), steps, 7), and the
    largest spread of the mixture logits over the 10 components seen in any (row, step, dimension)."""
    D = _data()
    mb = D["mb"]
    out = np.zeros((len(rows), steps, 7), np.float32)
    spread = 0.0
    for i, r in enumerate(rows):
        eng.rollout_reset()
        for t in range(steps):
            obs = dict(rgb_static=t_(mb["rgb_static"][r:r + 1, t:t + 1]), rgb_gripper=t_(mb["rgb_gripper"][r:r + 1, t:t + 1]), robot_obs_raw=t_(mb["robot_obs"][r, t]))
            if t == 0:
                eng.rollout_plan(obs, t_(mb["lang"][r]), plan_idx=D["plan"][r])
            out[i, t] = eng.rollout_act(obs, u_mix=D["u_mix"][r, t], u_act=D["u_act"][r, t])
            lp = eng.get_tensor("heads", 192)[:60].reshape(6, 10)
            spread = max(spread, float((lp.max(1) - lp.min(1)).max()))
    return out, spread


def _envs_rollout(eng, rows, slots, steps=3):
    """The same through the batched calls: one plan call and `steps` act calls over all rows."""
    D = _data()
    mb = D["mb"]
    out = np.zeros((len(rows), steps, 7), np.float32)
    for t in range(steps):
        if t == 0:
            plan = eng.rollout_envs_plan(_obs_rows(rows, 0, robot=False), t_(mb["lang"][rows]), env_ids=slots, plan=D["plan"][rows])
            assert np.array_equal(plan.cpu().numpy(), D["plan"][rows])
        out[:, t] = eng.rollout_envs_act(_obs_rows(rows, t), env_ids=slots, u_mix=D["u_mix"][rows, t], u_act=D["u_act"][rows, t])
    return out


# ------------------------------------------------------------------------------------------------ 2. isolation and placement, bf16
def test_envs_rows_do_not_depend_on_slot_position_or_neighbours():
    """Three environments (4 steps, replans at steps 0 and 2, injected plans and noise) in slots [1, 5, 6] of 8, then the same three in slots [6, 0, 3] with the
    rows in another order while the other five slots are planned, stepped (and one of them reset) with other data in calls of their own between every two calls:
    per-environment actions are BIT-IDENTICAL, and get_state of an untouched slot does not change under foreign calls."""
    D = _data()
    mb = D["mb"]
    eng = _engine("bf16", max_batch=8)
    envs = [0, 1, 2]                                            # data rows of the three environments
    plans = {0: D["plan"][[0, 1, 2]], 2: D["plan"][[10, 11, 12]]}      # step -> injected plans (per environment)

    def run(slot_of, order, foreign):
        eng.rollout_envs_init(8)                                # callable again: clears every slot
        others = [s for s in range(8) if s not in slot_of]
        acts = np.zeros((3, 4, 7), np.float32)
        for t in range(4):
            fr = t % 3                                          # frame index (the data has 3 frames)
            rows = [envs[e] for e in order]
            slots = [slot_of[e] for e in order]
            if t in plans:
                eng.rollout_envs_plan(dict(rgb_static=t_(mb["rgb_static"][rows, fr]), rgb_gripper=t_(mb["rgb_gripper"][rows, fr])), t_(mb["lang"][rows]), env_ids=slots,
                                      plan=plans[t][order])
            if foreign:
                before = eng.rollout_envs_get_state(slots)
                frows = [20 + s for s in others]
                if t == 0:
                    eng.rollout_envs_plan(_obs_rows(frows, 0, robot=False), t_(mb["lang"][frows]), env_ids=others)          # device-sampled plans
                if t == 2:
                    eng.rollout_envs_reset([others[1]])
                    eng.rollout_envs_plan(_obs_rows(frows[1:2], 1, robot=False), t_(mb["lang"][frows[1:2]]), env_ids=[others[1]])
                eng.rollout_envs_act(_obs_rows(frows, fr), env_ids=others)                                                  # device-drawn noise
                after = eng.rollout_envs_get_state(slots)
                assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
                assert np.array_equal(before[0], (plans[0] if t < 2 else plans[2])[order])
            a = eng.rollout_envs_act(dict(rgb_static=t_(mb["rgb_static"][rows, fr]), rgb_gripper=t_(mb["rgb_gripper"][rows, fr]), robot_obs_raw=t_(mb["robot_obs"][rows, fr])),
                                     env_ids=slots, u_mix=D["u_any"][rows, t], u_act=D["u_any"][rows, 4 + t, :, 0])
            acts[order, t] = a
        return acts

    a = run([1, 5, 6], [0, 1, 2], False)
    b = run([6, 0, 3], [2, 0, 1], True)
    eng.close()
    assert np.isfinite(a).all() and np.abs(a[:, 1] - a[:, 0]).max() > 0
    assert np.array_equal(a, b), np.abs(a - b).max()


# ------------------------------------------------------------------------------------------------ 3. 16-bit accuracy at the row-tile edges
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _close_cached_engines():
    yield
    for k in [k for k in _REF if k != "fp32"]:
        _REF.pop(k)[0].close()


def _truth():
    if "fp32" not in _REF:
        eng = _engine("fp32")
        _REF["fp32"] = _b1_rollout(eng, list(range(64)))
        eng.close()
    return _REF["fp32"]


def _half(dtype):
    if dtype not in _REF:
        eng = _engine(dtype)
        _REF[dtype] = (eng, _b1_rollout(eng, list(range(64)))[0])
    return _REF[dtype]


@pytest.mark.parametrize("n", [1, 2, 17, 64])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_envs_16bit_step_is_as_accurate_as_the_b1_step(dtype, n):
    """n rows (one row, two, one past a 16-row tile, the full 64) of the 16-bit batched step against the EXISTING fp32 B = 1 rollout run per environment on the
    same frames, language goals, injected plans and noise (3 steps, replan at step 0).  Scale d = the deviation of the EXISTING 16-bit B = 1 rollout from that
    truth over the same rows (max over dims 0..5).  Pass: |batched - truth| <= 2 d + 1e-3 on dims 0..5 (two independent 16-bit evaluations of similar error can
    add; the floor is half the fp32 fixture tolerance); the gripper command is exactly +-1 and differs from the truth only where the 16-bit B = 1 result does.
    The noise pins the mixture component (a Gumbel gap of ~13.9, see _data), so rounding cannot flip a component as long as the fp32 mixture-logit spread
    (max - min over the 10 components of one row and dimension) stays below half that gap.  Checked once on the CPU with the numpy oracle (oracle/hulc_oracle.py
    encode / goal_encode / decoder_heads on these 64 rows x 3 steps): the largest spread is 0.191; the test asserts the same bound on the fp32 engine's heads."""
    D = _data()
    truth, spread = _truth()
    assert spread < 0.5 * 13.4, spread
    eng, b1 = _half(dtype)
    rows = list(range(n))
    d = float(np.abs(b1[:n, :, :6] - truth[:n, :, :6]).max())
    print(f"rollout_envs accuracy {dtype} n={n}: d (16-bit B=1 vs fp32 B=1) = {d:.3e}, fp32 mixture-logit spread = {spread:.3f}")
    eng.rollout_envs_init(64)
    slots = [(7 * r + 3) % 64 for r in rows]                    # distinct (7 is coprime to 64), scattered over the table
    got = _envs_rollout(eng, rows, slots)
    err = float(np.abs(got[:, :, :6] - truth[:n, :, :6]).max())
    print(f"rollout_envs accuracy {dtype} n={n}: batched vs fp32 B=1 = {err:.3e} (bound {2 * d + 1e-3:.3e})")
    assert err <= 2 * d + 1e-3, (dtype, n, err, d)
    assert np.isin(got[:, :, 6], (-1.0, 1.0)).all()
    differs = got[:, :, 6] != truth[:n, :, 6]
    assert not (differs & (b1[:n, :, 6] == truth[:n, :, 6])).any()


# ------------------------------------------------------------------------------------------------ 4. device draws
def test_envs_device_draws_differ_between_rows_and_are_reproducible():
    D = _data()
    mb = D["mb"]
    res = []
    for _ in range(2):
        eng = _engine("bf16", max_batch=4, seed=11)
        eng.rollout_envs_init(4)
        rows = [5, 5, 5, 5]                                      # identical observation and goal in every row
        plan = eng.rollout_envs_plan(_obs_rows(rows, 0, robot=False), t_(mb["lang"][rows]))
        acts = [eng.rollout_envs_act(_obs_rows(rows, t)) for t in range(2)]
        res.append((plan.cpu().numpy(), np.stack(acts)))
        eng.close()
    plan, acts = res[0]
    assert plan.shape == (4, 32) and plan.min() >= 0 and plan.max() < 32
    assert any(not np.array_equal(plan[0], plan[r]) for r in range(1, 4))
    assert np.isfinite(acts).all() and np.isin(acts[..., 6], (-1.0, 1.0)).all()
    assert any(not np.array_equal(acts[0, 0], acts[0, r]) for r in range(1, 4))
    assert np.array_equal(plan, res[1][0]) and np.array_equal(acts, res[1][1])


# ------------------------------------------------------------------------------------------------ 5. error paths
def test_envs_argument_errors_leave_the_state_untouched():
    D = _data()
    mb = D["mb"]
    rows = [0, 1]

    def valid(eng, slots):
        return eng.rollout_envs_act(_obs_rows(rows, 1), env_ids=slots, u_mix=D["u_any"][rows, 0], u_act=D["u_any"][rows, 1, :, 0])

    def plan(eng, slots):
        eng.rollout_envs_plan(_obs_rows(rows, 0, robot=False), t_(mb["lang"][rows]), env_ids=slots, plan=D["plan"][rows])

    eng = _engine("bf16", max_batch=4)
    with pytest.raises(RuntimeError, match="before hulc_rollout_envs_init"):
        plan(eng, [0, 1])
    with pytest.raises(RuntimeError, match="before hulc_rollout_envs_init"):
        valid(eng, [0, 1])
    with pytest.raises(RuntimeError, match="max_envs 5 outside"):
        eng.rollout_envs_init(5)                                # above max_batch
    eng.rollout_envs_init(3)
    plan(eng, [2, 0])
    fresh = valid(eng, [2, 0])
    # the same start again, then every error, then the valid call
    eng.rollout_envs_init(3)
    plan(eng, [2, 0])
    with pytest.raises(RuntimeError, match="slot 2 is named more than once"):
        valid(eng, [2, 2])
    with pytest.raises(RuntimeError, match="slot 3 outside"):
        valid(eng, [2, 3])                                      # a slot equal to max_envs
    with pytest.raises(RuntimeError, match="slot 3 outside"):
        plan(eng, [3, 0])
    import ctypes as C
    from hulc_amd import lib as L
    with pytest.raises(RuntimeError, match="n = 0 outside"):
        keep = []
        eo, _ = eng._envs_obs(_obs_rows(rows, 1), [2, 0], keep, True)
        eo.n = 0
        L.check(eng.lib.hulc_rollout_envs_act(eng.ctx, C.byref(eo), None, None, np.zeros((2, 7), np.float32).ctypes.data))
    with pytest.raises(RuntimeError, match="slot 1 has no plan"):
        valid(eng, [2, 1])                                      # act on an unplanned slot: the message names it
    with pytest.raises(RuntimeError, match="exactly one goal kind"):
        o = _obs_rows(rows, 0, robot=False)
        keep = []
        eo, _ = eng._envs_obs(o, [2, 0], keep, False)
        L.check(eng.lib.hulc_rollout_envs_plan(eng.ctx, C.byref(eo), o["rgb_static"].data_ptr(), o["rgb_gripper"].data_ptr(), t_(mb["lang"][rows]).data_ptr(), None, None, None))
    with pytest.raises(RuntimeError, match="max_envs 5 outside"):
        eng.rollout_envs_init(5)                                # a failed init keeps the three slots
    again = valid(eng, [2, 0])
    eng.close()
    assert np.array_equal(fresh, again)


# ------------------------------------------------------------------------------------------------ 6. module level
def test_batched_policy_reproduces_the_reference_next_to_the_b1_step():
    """BatchedPolicy on a Hulc with the rollout fixture's weights: three environments (lang chain, vis chain, lang chain one step behind), sentence and image goals
    mixed in one step call, reproduce the fixture within 2e-3 (fp32); the B = 1 model.step interleaved with the batched calls returns exactly what it returns alone."""
    from hulc_amd import BatchedPolicy
    from hulc_amd.hulc import Hulc
    dims, P, frames, nsteps, replan_freq, fx = load_rollout_case()
    m = Hulc(precision="fp32", max_batch_size=3, max_seq_len=4, use_clip_auxiliary_loss=True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    m.eval()
    m.replan_freq = replan_freq
    m.lang_embeddings = {"do the task": frames["lang"]["lang"][0:1]}
    goals = {"lang": "do the task", "vis": dict(rgb_obs=dict(rgb_static=torch.from_numpy(frames["vis"]["rgb_static"][:, nsteps:nsteps + 1]),
                                                              rgb_gripper=torch.from_numpy(frames["vis"]["rgb_gripper"][:, nsteps:nsteps + 1])))}

    def b1_obs(mode, t):
        mb = frames[mode]
        return dict(rgb_obs=dict(rgb_static=torch.from_numpy(mb["rgb_static"][:, t:t + 1]), rgb_gripper=torch.from_numpy(mb["rgb_gripper"][:, t:t + 1])),
                    depth_obs={}, robot_obs=torch.zeros(1, 1, 8), robot_obs_raw=torch.from_numpy(mb["robot_obs"][:, t:t + 1]))

    def b1_step(t):
        return m.step(b1_obs("lang", t), goals["lang"], noise=dict(plan_idx=fx["plan_idx_lang"][t][0], u_mix=fx["u_mix_lang"][t][0, 0], u_act=fx["u_act_lang"][t][0, 0])).numpy()

    m.reset()
    alone = [b1_step(t) for t in range(nsteps)]
    m.reset()
    pol = BatchedPolicy(m, 3)
    prog = {0: [("lang", t) for t in range(nsteps)], 1: [("vis", t) for t in range(nsteps)], 2: [None] + [("lang", t) for t in range(nsteps)]}
    for k in range(nsteps + 1):
        live = [(e, *prog[e][k]) for e in (1, 0, 2) if k < len(prog[e]) and prog[e][k] is not None]
        cat = lambda key: torch.from_numpy(np.stack([frames[mo][key][0, t][None] for _, mo, t in live]))
        obs = dict(rgb_obs=dict(rgb_static=cat("rgb_static"), rgb_gripper=cat("rgb_gripper")), robot_obs_raw=cat("robot_obs"))
        noise = dict(plan_idx=np.stack([fx[f"plan_idx_{mo}"][t][0] for _, mo, t in live]), u_mix=np.stack([fx[f"u_mix_{mo}"][t][0, 0] for _, mo, t in live]),
                     u_act=np.stack([fx[f"u_act_{mo}"][t][0, 0] for _, mo, t in live]))
        a = pol.step(obs, [goals[mo] for _, mo, _ in live], env_ids=[e for e, _, _ in live], noise=noise)
        assert tuple(a.shape) == (len(live), 1, 7)
        for r, (e, mo, t) in enumerate(live):
            assert np.abs(a.numpy()[r, 0] - fx[f"actions_{mo}"][0, t]).max() <= 2e-3, (k, e, mo, t)
        if k < nsteps:
            assert np.array_equal(b1_step(k), alone[k]), k
    assert pol.rollout_step_counter == [nsteps, nsteps, nsteps]
    m.engine.close()
