"""CPU (-m "not gpu"): the host side of the per-tensor trainable mask (include/hulc_hip.h hulc_trainable_set / hulc_trainable_get /
hulc_trainable_steps_set, csrc/trainable_plan.h, spec.prefix_mask, FusedAdam.state_dict).

A context cannot be created without a device, so the refusals that need one in hand (a call before the bind, a wrong tensor count, a ninth group) are
checked on csrc/trainable_plan.h itself — the header the engine's entries call for exactly these decisions, compiled here into a program of its own;
the null-argument refusals go through the built library.  The optimizer's state dict is driven against a recording stand-in for the engine."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from hulc_amd import spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("hulc_trainable_set", "hulc_trainable_get", "hulc_trainable_steps_set")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from hulc_amd import lib as L
    return L.load()


def test_entries_are_exported_and_declared(lib):
    from hulc_amd import lib as L
    hdr = open(os.path.join(ROOT, "include", "hulc_hip.h")).read()
    capi = open(os.path.join(ROOT, "hulc_amd", "csrc", "capi.hip")).read()
    iface = open(os.path.join(ROOT, "hulc_amd", "csrc", "iengine.h")).read()
    for name in ENTRIES:
        assert name in L.EXPORTS and hasattr(lib, name), name
        assert re.search(r"\bint %s\s*\(hulc_ctx\* ctx" % name, hdr), name
        assert re.search(r"\bint %s\s*\(hulc_ctx\* ctx" % name, capi), name
        assert ("virtual int %s(" % name[len("hulc_"):]) in iface, name
        assert getattr(lib, name).argtypes[0] is ctypes.c_void_p
    from hulc_amd.engine import StepEngine
    for m in ("set_trainable", "trainable", "frozen_steps", "set_frozen_steps"):
        assert callable(getattr(StepEngine, m))


def test_null_arguments_are_refused_with_their_message(lib):
    mask = np.ones(4, np.uint8)
    cnt = np.zeros(4, np.int64)
    assert lib.hulc_trainable_set(None, 4, mask.ctypes.data) != 0
    assert lib.hulc_last_error() == b"hulc_trainable_set: null context"
    assert lib.hulc_trainable_set(None, 4, None) != 0
    assert lib.hulc_last_error() == b"hulc_trainable_set: null mask"
    assert lib.hulc_trainable_get(None, 4, mask.ctypes.data, cnt.ctypes.data) != 0
    assert lib.hulc_last_error() == b"hulc_trainable_get: null context"
    assert lib.hulc_trainable_steps_set(None, 4, cnt.ctypes.data, 0) != 0
    assert lib.hulc_last_error() == b"hulc_trainable_steps_set: null context"
    assert lib.hulc_trainable_steps_set(None, 4, None, 0) != 0
    assert lib.hulc_last_error() == b"hulc_trainable_steps_set: null counts"


PLAN_MAIN = r"""
#include "trainable_plan.h"
#include <cstdio>
using namespace hulc_trainable;
int main() {
    char e[256]; int rc;
    e[0] = 0; printf("before_bind %d|%s\n", check_call("hulc_trainable_set", false, 0, 5, e, sizeof(e)), e);
    e[0] = 0; printf("count %d|%s\n", check_call("hulc_trainable_set", true, 7, 5, e, sizeof(e)), e);
    e[0] = 0; printf("ok %d|%s\n", check_call("hulc_trainable_set", true, 5, 5, e, sizeof(e)), e);
    // ten tensors, each frozen for a different number of steps, then all unfrozen: tensor t is frozen at step t and everything thaws at step 20
    std::vector<uint8_t> mask(10, 1); std::vector<int64_t> cnt(10, 0), offs;
    for (int t = 1; t < 10; ++t) { std::vector<uint8_t> want(mask); want[t] = 0; apply_mask(want.data(), t, mask, cnt); }
    e[0] = 0; rc = plan_groups("hulc_trainable_set", mask, cnt, offs, e, sizeof(e)); printf("one_trainable %d %d|%s\n", rc, (int)offs.size(), e);
    std::vector<uint8_t> m8(mask), m9(mask); std::vector<int64_t> c8(cnt), c9(cnt);
    std::vector<uint8_t> w8(10, 0), w9(10, 0);
    for (int t = 0; t < 8; ++t) w8[t] = 1;
    for (int t = 0; t < 9; ++t) w9[t] = 1;
    apply_mask(w8.data(), 20, m8, c8); apply_mask(w9.data(), 20, m9, c9);
    e[0] = 0; rc = plan_groups("hulc_trainable_set", m8, c8, offs, e, sizeof(e)); printf("eight %d %d|%s\n", rc, (int)offs.size(), e);
    printf("eight_offsets"); for (long long o : offs) printf(" %lld", o); printf("\n");
    e[0] = 0; rc = plan_groups("hulc_trainable_set", m9, c9, offs, e, sizeof(e)); printf("nine %d %d|%s\n", rc, (int)offs.size(), e);
    // counts reported while frozen and after the thaw
    printf("frozen_steps %lld %lld %lld\n", frozen_steps(mask[3], cnt[3], 12), frozen_steps(m9[3], c9[3], 25), frozen_steps(m9[0], c9[0], 25));
    return 0;
}
"""


def test_refusals_of_the_planning_header(tmp_path):
    """csrc/trainable_plan.h on its own: the bind / count refusals and the eight-group limit with the messages the C entries hand on."""
    src = tmp_path / "plan_main.cpp"
    src.write_text(PLAN_MAIN)
    exe = tmp_path / "plan_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "hulc_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert out["before_bind"] == "1|hulc_trainable_set before hulc_bind_params"
    assert out["count"] == "1|hulc_trainable_set: 5 entries, 7 tensors are bound"
    assert out["ok"] == "0|"
    assert out["one_trainable"] == "0 1|"
    assert out["eight"] == "0 8|"
    assert out["eight_offsets"] == "0 13 14 15 16 17 18 19"      # tensor 0 never froze; tensor t sat out steps t+1 .. 20, ascending
    rc, rest = out["nine"].split(" ", 1)
    assert rc == "1" and rest.startswith("9|hulc_trainable_set: ") and "9 distinct frozen-step counts" in rest and "limit is 8" in rest
    # tensor 3 froze after 3 steps: 9 sat out at step 12; thawed at 20 it keeps 17 whatever the count then; tensor 0 never froze
    assert out["frozen_steps"] == "9 17 0"
    # the kernels' group slots and the header's limit are the same number
    k = open(os.path.join(ROOT, "hulc_amd", "csrc", "kernels.h")).read()
    assert re.search(r"constexpr int OPT_GROUPS = 8;", k)


@pytest.mark.parametrize("kind", ["hulc", "gcbc", "mcil"])
def test_prefix_mask_on_the_parameter_tables(kind):
    dims = spec.ModelDims(kind=kind, max_window=32, use_clip=kind != "mcil")
    names = [n for n, _, _ in spec.param_table(dims)]
    m = spec.prefix_mask(names, ["perceptual_encoder", "language_goal."])
    assert [n for n, f in zip(names, m) if f] == [n for n in names if n.startswith("perceptual_encoder.") or n.startswith("language_goal.")]
    assert any(m) and not all(m)
    # a module path, not a string prefix; an exact tensor name; one string instead of a list
    assert not any(spec.prefix_mask(names, [])) and not any(spec.prefix_mask(names, None))
    one = "visual_goal.mlp.0.bias"
    assert [n for n, f in zip(names, spec.prefix_mask(names, one)) if f] == [one]
    sub = spec.prefix_mask(names, "visual_goal.mlp")
    assert [n for n, f in zip(names, sub) if f] == [n for n in names if n.startswith("visual_goal.mlp.")]
    with pytest.raises(KeyError):
        spec.prefix_mask(names, "visual_goal.ml")            # a string prefix of a module name selects nothing
    with pytest.raises(KeyError):
        spec.prefix_mask(names, ["perceptual_encoder", "no_such_module"])
    if kind == "mcil":
        assert sum(spec.prefix_mask(names, "plan_recognition.birnn_model")) == 16
    else:
        assert sum(spec.prefix_mask(names, "plan_recognition.transformer_encoder.layers.1")) == 12


# ---------------------------------------------------------------------------------------------------------------- optimizer state dict
class _Engine:
    """What FusedAdam and Hulc._sync_trainable touch of a StepEngine, recording the mask calls."""

    def __init__(self, names, dtype="bf16"):
        import torch
        self.layout = {n: (64 * i, (4,)) for i, n in enumerate(names)}
        self.dtype = dtype
        self.adam_t = 0
        self.adam_m, self.adam_v = torch.zeros(8), torch.zeros(8)
        self.mask = {n: True for n in names}
        self.steps = {n: 0 for n in names}
        self.taken = 0
        self.calls = []

    def set_trainable(self, mask):
        self.calls.append(("set_trainable", dict(mask)))
        self.mask.update(mask)

    def trainable(self):
        return dict(self.mask)

    def frozen_steps(self):
        return dict(self.steps)

    def set_frozen_steps(self, steps, steps_taken=-1):
        self.calls.append(("set_frozen_steps", dict(steps), steps_taken))
        self.steps = {n: int(steps.get(n, 0)) for n in self.layout}
        self.taken = steps_taken


def _module(names):
    import torch
    from hulc_amd.hulc import Hulc

    class M:
        _sync_trainable = Hulc._sync_trainable
        freeze_modules = Hulc.freeze_modules
        unfreeze_modules = Hulc.unfreeze_modules

        def __init__(self):
            self.engine = _Engine(names)
            self._params = {n: torch.nn.Parameter(torch.zeros(4)) for n in names}
            self._grad_views = {n: torch.zeros(4) for n in names}
            self._mask_pushed = None
            self._grads_reduced = True

        def parameters(self):
            return iter(self._params.values())
    return M()


NAMES = ["perceptual_encoder.a.weight", "perceptual_encoder.a.bias", "visual_goal.mlp.0.weight", "action_decoder.rnn.weight_hh_l0"]


def test_optimizer_state_dict_round_trips_mask_and_counts():
    from hulc_amd.hulc import FusedAdam
    m = _module(NAMES)
    opt = FusedAdam(m, kind="adamw", weight_decay=0.01)
    m.freeze_modules(["perceptual_encoder"])
    assert m.engine.calls == [("set_trainable", {n: not n.startswith("perceptual_encoder.") for n in NAMES})]
    assert all((p.grad is None) == n.startswith("perceptual_encoder.") for n, p in m._params.items())
    m.engine.adam_t = 7
    m.engine.steps = {NAMES[0]: 5, NAMES[1]: 5, NAMES[2]: 2, NAMES[3]: 0}
    sd = opt.state_dict()
    assert sd["step"] == 7
    assert sd["trainable"] == {NAMES[0]: False, NAMES[1]: False, NAMES[2]: True, NAMES[3]: True}
    assert sd["frozen_steps"] == {NAMES[0]: 5, NAMES[1]: 5, NAMES[2]: 2, NAMES[3]: 0}
    # into a fresh module: flags, engine mask and counts come back, the counts as of the restored step
    m2 = _module(NAMES)
    opt2 = FusedAdam(m2, kind="adamw", weight_decay=0.01)
    opt2.load_state_dict(sd)
    assert m2.engine.adam_t == 7
    assert {n: p.requires_grad for n, p in m2._params.items()} == sd["trainable"]
    assert m2.engine.mask == sd["trainable"] and m2.engine.steps == sd["frozen_steps"] and m2.engine.taken == 7
    assert m2.engine.calls[-1][0] == "set_frozen_steps" and m2.engine.calls[-2][0] == "set_trainable"      # the mask first, then the counts
    assert all((p.grad is None) == (not sd["trainable"][n]) for n, p in m2._params.items())
    assert opt2.state_dict()["trainable"] == sd["trainable"] and opt2.state_dict()["frozen_steps"] == sd["frozen_steps"]


def test_old_format_state_dict_loads_as_all_trainable():
    import torch
    from hulc_amd.hulc import FusedAdam
    old = dict(step=3, exp_avg=torch.ones(8), exp_avg_sq=torch.ones(8), param_groups=[{}])
    # a module that never froze anything: the engine is not handed a mask at all
    m = _module(NAMES)
    FusedAdam(m).load_state_dict(old)
    assert m.engine.calls == [] and m.engine.adam_t == 3 and all(p.requires_grad for p in m._params.values())
    # a module with frozen tensors: everything thaws, every count is zero
    m = _module(NAMES)
    opt = FusedAdam(m)
    m.freeze_modules("visual_goal")
    m.engine.steps = {n: 2 for n in NAMES}
    opt.load_state_dict(old)
    assert all(p.requires_grad for p in m._params.values()) and all(p.grad is not None for p in m._params.values())
    assert m.engine.mask == {n: True for n in NAMES} and m.engine.steps == {n: 0 for n in NAMES} and m.engine.taken == 3


def test_freeze_modules_is_reachable_from_the_training_cli():
    """`+model.freeze_modules=[...]` lands in the model group that config.instantiate hands to the constructor, for both model classes."""
    import inspect
    from hulc_amd import config
    from hulc_amd.hulc import GCBC, Hulc
    from hulc_amd.training import CONF_DIR, config_fingerprint
    c = config.compose(CONF_DIR, "config", ["+model.freeze_modules=[perceptual_encoder,language_goal]"])
    assert list(c.model.freeze_modules) == ["perceptual_encoder", "language_goal"]
    assert config_fingerprint(c)["model"]["freeze_modules"] == ["perceptual_encoder", "language_goal"]      # another mask is another run
    c = config.compose(CONF_DIR, "config", ["model=gcbc", "model.freeze_modules=perceptual_encoder"])
    assert c.model.freeze_modules == "perceptual_encoder"
    for cls in (Hulc, GCBC):
        p = inspect.signature(cls.__init__).parameters
        assert "freeze_modules" in p and p["freeze_modules"].default is None
