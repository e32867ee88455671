"""Reproducible training mode, the parts that need no GPU: Lightning's Trainer(deterministic=...) keyword, its way from a composed config to the
Trainer (hulc_amd.training.trainer_kwargs forwards it only when the trainer group sets it), the engine option it sets, and the run fingerprint."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hulc_amd import config, training  # noqa: E402
from hulc_amd.trainer import Trainer  # noqa: E402

CONF = os.path.join(ROOT, "conf")


class _NoEngine:
    pass


class _FakeEngine:
    def __init__(self):
        self.options = []

    def set_option(self, name, value):
        self.options.append((name, value))


class _FakeModule:
    def __init__(self):
        self.engine = _FakeEngine()


def test_trainer_accepts_deterministic_and_sets_the_engine_option():
    assert Trainer().deterministic is False
    tr = Trainer(deterministic=True)
    assert tr.deterministic is True
    m = _FakeModule()
    tr._configure_deterministic(m)
    assert m.engine.options == [("reproducible", 1)]
    m = _FakeModule()
    Trainer()._configure_deterministic(m)
    Trainer(deterministic=False)._configure_deterministic(m)
    assert m.engine.options == []                              # off: the engine is not touched at all


def test_a_module_without_an_engine_is_refused_only_when_the_key_is_on():
    Trainer()._configure_deterministic(_NoEngine())
    with pytest.raises(RuntimeError):
        Trainer(deterministic=True)._configure_deterministic(_NoEngine())


def test_cli_forwards_the_key_only_when_the_trainer_group_sets_it():
    kw = training.trainer_kwargs(config.compose(CONF, "config", []))
    assert set(kw) == {"max_epochs", "max_steps", "log_dir", "callbacks"}      # the default key set is what it was
    assert Trainer(**kw).deterministic is False
    kw = training.trainer_kwargs(config.compose(CONF, "config", ["trainer.deterministic=true"]))
    assert kw["deterministic"] is True and set(kw) == {"max_epochs", "max_steps", "log_dir", "callbacks", "deterministic"}
    assert Trainer(**kw).deterministic is True
    kw = training.trainer_kwargs(config.compose(CONF, "config", ["trainer.deterministic=false", "trainer.gradient_clip_val=0.5"]))
    assert kw["deterministic"] is False and kw["gradient_clip_val"] == 0.5
    for name in ("mi355x", "play_trainer"):
        assert "deterministic" not in open(os.path.join(CONF, "trainer", name + ".yaml")).read()


def test_the_key_is_run_bookkeeping_not_part_of_the_fingerprint():
    a = training.config_fingerprint(config.compose(CONF, "config", []))
    b = training.config_fingerprint(config.compose(CONF, "config", ["trainer.deterministic=true"]))
    assert a == b
