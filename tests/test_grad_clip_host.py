"""Gradient clipping / gradient-norm tracking, the parts that need no GPU: the Trainer's keywords (Lightning's gradient_clip_val,
gradient_clip_algorithm, track_grad_norm), their way from a composed config to the Trainer (hulc_amd.training.trainer_kwargs), and the C-ABI
entry points (include/hulc_hip.h hulc_grad_clip_set / hulc_grad_norm_get) with their ctypes mirrors."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hulc_amd import config, training  # noqa: E402
from hulc_amd.trainer import Trainer  # noqa: E402

CONF = os.path.join(ROOT, "conf")


def test_trainer_keeps_the_clipping_keywords_and_rejects_what_it_cannot_do():
    tr = Trainer(gradient_clip_val=0.5, gradient_clip_algorithm="value", track_grad_norm=2)
    assert tr.gradient_clip_val == 0.5 and tr.gradient_clip_algorithm == "value" and tr.track_grad_norm == 2.0
    assert tr.clips_gradients
    with pytest.raises(ValueError):
        Trainer(gradient_clip_val=0.5, gradient_clip_algorithm="l2")
    with pytest.raises(NotImplementedError):
        Trainer(track_grad_norm=1)
    with pytest.raises(NotImplementedError):
        Trainer(track_grad_norm="inf")
    for on in (2, 2.0, "2"):
        assert Trainer(track_grad_norm=on).track_grad_norm == 2.0
    off = Trainer()
    assert not off.clips_gradients and off.gradient_clip_val is None and off.gradient_clip_algorithm == "norm" and off.track_grad_norm == -1.0
    for none in (None, 0, 0.0):
        assert not Trainer(gradient_clip_val=none).clips_gradients
    assert Trainer(gradient_clip_val=1, gradient_clip_algorithm=None).gradient_clip_algorithm == "norm"


class _NoEngine:
    pass


class _FakeEngine:
    def __init__(self):
        self.calls = []

    def set_grad_clip(self, algo, limit, track=False):
        self.calls.append((algo, limit, track))


class _FakeModule:
    def __init__(self):
        self.engine = _FakeEngine()


def test_trainer_configures_the_engine_once_and_refuses_a_module_without_one():
    m = _FakeModule()
    assert Trainer(gradient_clip_val=0.25)._configure_grad_clip(m) is True
    assert m.engine.calls == [("norm", 0.25, False)]
    m = _FakeModule()
    assert Trainer(gradient_clip_val=0.25, gradient_clip_algorithm="value")._configure_grad_clip(m) is False      # a clamp needs no norm
    assert m.engine.calls == [("value", 0.25, False)]
    m = _FakeModule()
    assert Trainer(track_grad_norm=2)._configure_grad_clip(m) is True
    assert m.engine.calls == [("off", None, True)]
    m = _FakeModule()
    assert Trainer()._configure_grad_clip(m) is False
    assert m.engine.calls == [("off", None, False)]
    assert Trainer()._configure_grad_clip(_NoEngine()) is False
    with pytest.raises(RuntimeError):
        Trainer(gradient_clip_val=1.0)._configure_grad_clip(_NoEngine())


def test_cli_forwards_the_three_keys_from_the_trainer_group():
    cfg = config.compose(CONF, "config", ["trainer.gradient_clip_val=0.25"])
    kw = training.trainer_kwargs(cfg, callbacks=[])
    assert kw["gradient_clip_val"] == 0.25 and "gradient_clip_algorithm" not in kw and "track_grad_norm" not in kw
    assert kw["max_epochs"] == cfg.trainer.max_epochs and kw["log_dir"] == cfg.log_dir and kw["callbacks"] == []
    tr = Trainer(**kw)
    assert tr.gradient_clip_val == 0.25 and tr.gradient_clip_algorithm == "norm"
    cfg = config.compose(CONF, "config", ["trainer.gradient_clip_val=0.5", "trainer.gradient_clip_algorithm=value", "trainer.track_grad_norm=2"])
    tr = Trainer(**training.trainer_kwargs(cfg))
    assert (tr.gradient_clip_val, tr.gradient_clip_algorithm, tr.track_grad_norm) == (0.5, "value", 2.0)
    # nothing configured: the Trainer's defaults (off), and only the keys the CLI forwarded before
    kw = training.trainer_kwargs(config.compose(CONF, "config", []))
    assert set(kw) == {"max_epochs", "max_steps", "log_dir", "callbacks"} and not Trainer(**kw).clips_gradients
    # run bookkeeping, like max_steps: a run directory may be re-entered with another clipping value
    a = training.config_fingerprint(config.compose(CONF, "config", []))
    b = training.config_fingerprint(config.compose(CONF, "config", ["trainer.gradient_clip_val=0.25", "trainer.track_grad_norm=2"]))
    assert a == b


def test_header_declares_and_ctypes_binds_the_entry_points():
    import __graft_entry__ as g
    g.build()
    from hulc_amd import lib
    hdr = open(os.path.join(ROOT, "include", "hulc_hip.h")).read()
    declared = set(re.findall(r"\b(hulc_[a-z_0-9]+)\s*\(", hdr))
    assert {"hulc_grad_clip_set", "hulc_grad_norm_get"} <= declared
    assert re.search(r"enum\s*\{\s*HULC_CLIP_OFF = 0, HULC_CLIP_NORM = 1, HULC_CLIP_VALUE = 2\s*\}", hdr)
    assert lib.CLIP == {"off": 0, "norm": 1, "value": 2}
    l = lib.load()
    assert {"hulc_grad_clip_set", "hulc_grad_norm_get"} <= set(lib.EXPORTS)
    assert l.hulc_grad_clip_set.argtypes == [C.c_void_p, C.c_int32, C.c_float, C.c_int32]
    assert l.hulc_grad_norm_get.argtypes == [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.c_int64]
    # null context: an error code and a message, never a crash
    assert l.hulc_grad_clip_set(None, 1, 1.0, 0) == 1 and b"hulc_grad_clip_set" in l.hulc_last_error()
    assert l.hulc_grad_norm_get(None, None, None, None, 0) == 1 and b"hulc_grad_norm_get" in l.hulc_last_error()
