"""CPU (-m "not gpu"): the host side of the batched multi-environment rollout — the ctypes mirror of hulc_rollout_envs_obs against the C
compiler's view of the header, and BatchedPolicy's per-environment replan scheduling against a recording fake engine (no GPU, no library call)."""
import ctypes
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rollout_envs_obs_layout_matches_header(tmp_path):
    from hulc_amd import lib
    st, cls = "hulc_rollout_envs_obs", lib.HulcRolloutEnvsObs
    fields = [f[0] for f in cls._fields_]
    assert fields == ["n", "slots", "rgb_static", "rgb_gripper", "robot_obs_raw"]
    body = f'printf("{st} %zu\\n", sizeof({st}));' + "".join(f'printf("{st}.{fl} %zu\\n", offsetof({st}, {fl}));' for fl in fields)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hulc_hip.h"\nint main(void) {' + body + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(cls) == int(out[st])
    for fl in fields:
        assert getattr(cls, fl).offset == int(out[f"{st}.{fl}"]), fl
    for name in ("init", "reset", "plan", "act", "get_state", "set_state"):
        assert f"hulc_rollout_envs_{name}" in lib.EXPORTS


class FakeEngine:
    """Records every hulc_rollout_envs_* call BatchedPolicy makes."""

    def __init__(self):
        self.calls = []

    def rollout_envs_init(self, max_envs):
        self.calls.append(("init", max_envs))

    def rollout_envs_reset(self, env_ids=None, clear_hidden=False):
        self.calls.append(("reset", None if env_ids is None else list(env_ids), bool(clear_hidden)))

    def rollout_envs_plan(self, obs, goal, env_ids=None, plan=None, want_goal=False):
        kind = "vis" if isinstance(goal, dict) else "lang"
        rows = obs["rgb_static"].shape[0]
        assert rows == len(env_ids) == (goal["rgb_static"].shape[0] if kind == "vis" else goal.shape[0])
        tag = [float(x) for x in (goal["rgb_static"].reshape(rows, -1)[:, 0] if kind == "vis" else goal[:, 0])]
        self.calls.append(("plan", list(env_ids), kind, [float(x) for x in obs["rgb_static"].reshape(rows, -1)[:, 0]], tag,
                           None if plan is None else np.asarray(plan).tolist()))

    def rollout_envs_act(self, obs, env_ids=None, u_mix=None, u_act=None):
        n = obs["rgb_static"].shape[0]
        assert obs["robot_obs_raw"].shape[0] == n == len(env_ids)
        self.calls.append(("act", list(env_ids), [float(x) for x in obs["rgb_static"].reshape(n, -1)[:, 0]]))
        return np.tile(np.asarray(env_ids, np.float32)[:, None], (1, 7))


def _obs(vals):
    """n rows whose first pixel carries `vals` (so the fake engine can tell which rows reached it)."""
    n = len(vals)
    rs = torch.zeros(n, 1, 3, 200, 200)
    rs[:, 0, 0, 0, 0] = torch.tensor(vals, dtype=torch.float32)
    return dict(rgb_obs=dict(rgb_static=rs, rgb_gripper=torch.zeros(n, 1, 3, 84, 84)), robot_obs_raw=torch.zeros(n, 1, 15))


def _img_goal(v):
    return dict(rgb_obs=dict(rgb_static=torch.full((1, 1, 3, 200, 200), float(v)), rgb_gripper=torch.zeros(1, 1, 3, 84, 84)))


def _model(kind, replan_freq=2):
    emb = {"push": np.full(384, 7.0, np.float32), "lift": np.full(384, 9.0, np.float32)}
    return SimpleNamespace(engine=FakeEngine(), kind=kind, replan_freq=replan_freq, lang_embeddings=emb)


def test_batched_policy_replans_per_environment():
    from hulc_amd import BatchedPolicy
    m = _model("hulc", replan_freq=2)
    pol = BatchedPolicy(m, 3)
    eng = m.engine
    assert eng.calls == [("init", 3)]
    eng.calls.clear()
    g0, g1, g2 = "push", _img_goal(5.0), "lift"
    # steps 0, 1: environments 0 (sentence) and 1 (image) only; environment 2 joins two steps late
    a = pol.step(_obs([10, 11]), [g0, g1], env_ids=[0, 1])
    assert tuple(a.shape) == (2, 1, 7) and a[:, 0, 0].tolist() == [0.0, 1.0]
    assert eng.calls == [("plan", [0], "lang", [10.0], [7.0], None), ("plan", [1], "vis", [11.0], [5.0], None), ("act", [0, 1], [10.0, 11.0])]
    eng.calls.clear()
    pol.step(_obs([20, 21]), [g0, g1], env_ids=[0, 1])
    assert eng.calls == [("act", [0, 1], [20.0, 21.0])]
    assert pol.rollout_step_counter == [2, 2, 0]
    eng.calls.clear()
    # step 2: all three replan (counters 2, 2, 0); rows given in another order than the environments; both sentences share ONE lang plan call
    pol.step(_obs([32, 30, 31]), [g2, g0, g1], env_ids=[2, 0, 1])
    assert eng.calls == [("plan", [2, 0], "lang", [32.0, 30.0], [9.0, 7.0], None), ("plan", [1], "vis", [31.0], [5.0], None), ("act", [2, 0, 1], [32.0, 30.0, 31.0])]
    eng.calls.clear()
    # step 3: nobody replans
    pol.step(_obs([40, 41, 42]), [g0, g1, g2])
    assert eng.calls == [("act", [0, 1, 2], [40.0, 41.0, 42.0])]
    assert pol.rollout_step_counter == [4, 4, 2]
    eng.calls.clear()
    # reset of environment 1 touches environment 1 only: it replans at once, the others by their own counters (0: 4 % 2 == 0, 2: 2 % 2 == 0)
    pol.reset(env_ids=[1])
    assert eng.calls == [("reset", [1], False)] and pol.rollout_step_counter == [4, 0, 2]
    eng.calls.clear()
    pol.step(_obs([50, 51, 52]), [g0, g1, g2])
    pol.step(_obs([60, 61, 62]), [g0, g1, g2])
    assert eng.calls[:3] == [("plan", [0, 2], "lang", [50.0, 52.0], [7.0, 9.0], None), ("plan", [1], "vis", [51.0], [5.0], None), ("act", [0, 1, 2], [50.0, 51.0, 52.0])]
    assert eng.calls[3:] == [("act", [0, 1, 2], [60.0, 61.0, 62.0])]
    assert pol.rollout_step_counter == [6, 2, 4]
    # injected plans follow their rows into the plan calls
    eng.calls.clear()
    plan_idx = np.arange(3 * 32, dtype=np.int32).reshape(3, 32)
    pol.step(_obs([70, 71, 72]), [g0, g1, g2], noise=dict(plan_idx=plan_idx))
    assert eng.calls[0][1] == [0, 2] and eng.calls[0][5] == plan_idx[[0, 2]].tolist() and eng.calls[1][5] == plan_idx[[1]].tolist()
    # reset() without ids: every environment, one engine call
    eng.calls.clear()
    pol.reset()
    assert eng.calls == [("reset", None, False)] and pol.rollout_step_counter == [0, 0, 0]
    with pytest.raises(ValueError):
        pol.step(_obs([1, 2]), [g0, g0], env_ids=[1, 1])
    with pytest.raises(ValueError):
        pol.step(_obs([1]), [g0], env_ids=[3])


def test_batched_policy_gcbc_plans_goal_once_until_reset():
    from hulc_amd import BatchedPolicy
    m = _model("gcbc", replan_freq=2)
    pol = BatchedPolicy(m, 2)
    eng = m.engine
    eng.calls.clear()
    goals = ["push", _img_goal(3.0)]
    for t in range(3):
        pol.step(_obs([t, t + 0.5]), goals)
    plans = [c for c in eng.calls if c[0] == "plan"]
    assert plans == [("plan", [0], "lang", [0.0], [7.0], None), ("plan", [1], "vis", [0.5], [3.0], None)]      # the first step only, whatever replan_freq says
    assert [c[0] for c in eng.calls] == ["plan", "plan", "act", "act", "act"]
    eng.calls.clear()
    pol.reset(env_ids=[0])
    assert eng.calls == [("reset", [0], False)]           # clear_hidden = 0: the reference's GCBC.reset never clears the decoder state
    eng.calls.clear()
    pol.step(_obs([9.0, 9.5]), goals)
    assert eng.calls == [("plan", [0], "lang", [9.0], [7.0], None), ("act", [0, 1], [9.0, 9.5])]
