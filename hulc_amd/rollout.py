"""BatchedPolicy — several environments stepped against ONE policy context (hulc_rollout_envs_*, include/hulc_hip.h).

The reference's evaluation (hulc/evaluation/evaluate_policy.py: 1000 instruction chains x 5 tasks x up to 360 steps) calls
``model.reset()`` / ``model.step(obs, goal)`` for one environment at a time.  BatchedPolicy keeps what ``Hulc.step`` keeps — the
``rollout_step_counter`` and the replan rule of hulc.py:851-869, the goal-once rule of gcbc.py:287-320 — once PER ENVIRONMENT on the
host, and hands the work of all of them to the engine in at most two plan calls (one per goal kind) and one act call per step.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch


class BatchedPolicy:
    """``num_envs`` independent policy instances (slots) of ``model`` (a ``Hulc`` — hulc / mcil — or a ``GCBC``).

    reset(env_ids=None)                      start new rollouts in the given environments (None = all)
    step(obs, goals, env_ids=None, noise)    one step of inference for n environments -> (n,1,7) world-frame actions

    obs:   rgb_obs {rgb_static (n,1,3,200,200), rgb_gripper (n,1,3,84,84)}, robot_obs_raw (n,1,15)
    goals: n entries, each a sentence (a key of ``model.load_lang_embeddings``) or a dict with ``rgb_obs`` goal images
           {rgb_static (1,1,3,200,200), rgb_gripper (1,1,3,84,84)}; kinds may be mixed within one call.
    env_ids: the environment of every row (distinct, each in [0, num_envs)); None = rows 0..n-1.
    noise (optional, parity tests): ``plan_idx`` (n,32) / ``plan`` (n,256, mcil) injected plans (rows that do not replan are ignored),
           ``u_mix`` (n,D,10), ``u_act`` (n,D) uniform draws of the sampler.
    The B = 1 ``model.step`` keeps its own state and may be used next to this object.
    """

    def __init__(self, model, num_envs: int):
        self.model = model
        self.engine = model.engine
        self.kind = model.kind
        self.num_envs = int(num_envs)
        self.engine.rollout_envs_init(self.num_envs)
        self.rollout_step_counter: List[int] = [0] * self.num_envs
        self.has_goal: List[bool] = [False] * self.num_envs

    @property
    def replan_freq(self) -> int:
        return int(self.model.replan_freq)

    def _ids(self, env_ids: Optional[Sequence[int]], n: int) -> List[int]:
        ids = list(range(n)) if env_ids is None else [int(e) for e in env_ids]
        if len(ids) != n:
            raise ValueError(f"{len(ids)} env ids for {n} rows")
        if len(set(ids)) != n or any(e < 0 or e >= self.num_envs for e in ids):
            raise ValueError(f"env ids must be distinct and in [0, {self.num_envs}): {ids}")
        return ids

    def reset(self, env_ids: Optional[Sequence[int]] = None) -> None:
        """Hulc.reset (hulc.py:843-849) / GCBC.reset (gcbc.py:281-285) for the given environments: the counter restarts and plan and goal
        are dropped; the reference's GCBC never clears the decoder's hidden state, so neither does this (clear_hidden = 0)."""
        ids = list(range(self.num_envs)) if env_ids is None else self._ids(env_ids, len(env_ids))
        for e in ids:
            self.rollout_step_counter[e] = 0
            self.has_goal[e] = False
        self.engine.rollout_envs_reset(None if env_ids is None else ids, clear_hidden=False)

    @staticmethod
    def _rows(t, rows: List[int]):
        t = torch.as_tensor(t)
        return t[torch.as_tensor(rows, dtype=torch.long, device=t.device)]

    def _lang_goal(self, sentence: str) -> np.ndarray:
        if self.model.lang_embeddings is None:
            raise RuntimeError("call load_lang_embeddings() before stepping with a language goal (hulc.py:871)")
        return np.asarray(self.model.lang_embeddings[sentence], np.float32).reshape(-1)

    def step(self, obs: Dict[str, Any], goals: Sequence[Any], env_ids: Optional[Sequence[int]] = None, noise: Optional[Dict] = None) -> torch.Tensor:
        noise = noise or {}
        rs, rg = obs["rgb_obs"]["rgb_static"], obs["rgb_obs"]["rgb_gripper"]
        n = int(rs.shape[0])
        ids = self._ids(env_ids, n)
        if len(goals) != n:
            raise ValueError(f"{len(goals)} goals for {n} rows")
        # hulc / mcil: replan exactly the environments whose counter is a multiple of replan_freq (hulc.py:858); gcbc: encode the goal once per rollout (gcbc.py:300)
        if self.kind == "gcbc":
            replan = [r for r, e in enumerate(ids) if not self.has_goal[e]]
        else:
            replan = [r for r, e in enumerate(ids) if self.rollout_step_counter[e] % self.replan_freq == 0]
        inject = noise.get("plan") if self.kind == "mcil" else noise.get("plan_idx")
        groups = ([r for r in replan if isinstance(goals[r], str)], [r for r in replan if not isinstance(goals[r], str)])       # language first, then visual
        for is_vis, rows in enumerate(groups):
            if not rows:
                continue
            o = dict(rgb_static=self._rows(rs, rows), rgb_gripper=self._rows(rg, rows))
            if is_vis:
                g = dict(rgb_static=torch.cat([torch.as_tensor(goals[r]["rgb_obs"]["rgb_static"]).reshape(1, 3, 200, 200) for r in rows]),
                         rgb_gripper=torch.cat([torch.as_tensor(goals[r]["rgb_obs"]["rgb_gripper"]).reshape(1, 3, 84, 84) for r in rows]))
            else:
                g = torch.from_numpy(np.stack([self._lang_goal(goals[r]) for r in rows]))
            self.engine.rollout_envs_plan(o, g, env_ids=[ids[r] for r in rows], plan=self._rows(inject, rows) if inject is not None else None)
            for r in rows:
                self.has_goal[ids[r]] = True
        action = self.engine.rollout_envs_act(dict(rgb_static=rs, rgb_gripper=rg, robot_obs_raw=obs["robot_obs_raw"]), env_ids=ids,
                                              u_mix=noise.get("u_mix"), u_act=noise.get("u_act"))
        for e in ids:
            self.rollout_step_counter[e] += 1
        return torch.from_numpy(np.asarray(action, np.float32)).reshape(n, 1, 7)
