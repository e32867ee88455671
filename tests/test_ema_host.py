"""CPU (-m "not gpu"): the host side of the averaged weights (include/hulc_hip.h hulc_ema_enable / hulc_ema_state_get / hulc_ema_state_set / hulc_ema_swap /
hulc_ema_swapped / hulc_k_ema_update, spec.ema_decay_at, the `ema_decay` options of Hulc / GCBC and their way in from the training command line).

A context cannot be created without a device: what is checked on the built library is that the entries exist with their prototypes, and the refusals that
are decided on the arguments alone."""
import ctypes
import inspect
import os
import re

import pytest

from hulc_amd import spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTX_ENTRIES = ("hulc_ema_enable", "hulc_ema_state_get", "hulc_ema_state_set", "hulc_ema_swap", "hulc_ema_swapped")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from hulc_amd import lib as L
    return L.load()


def test_entries_are_declared_and_exported(lib):
    from hulc_amd import lib as L
    hdr = open(os.path.join(ROOT, "include", "hulc_hip.h")).read()
    capi = open(os.path.join(ROOT, "hulc_amd", "csrc", "capi.hip")).read()
    for name in CTX_ENTRIES:
        assert name in L.EXPORTS and hasattr(lib, name), name
        assert re.search(r"\bint %s\s*\(hulc_ctx\* ctx" % name, hdr), name
        assert re.search(r"\bint %s\s*\(hulc_ctx\* ctx" % name, capi), name
        assert getattr(lib, name).argtypes[0] is ctypes.c_void_p
    assert "hulc_k_ema_update" in L.EXPORTS and hasattr(lib, "hulc_k_ema_update")
    proto = r"\bint hulc_k_ema_update\s*\(float\* ema, const float\* p, int64_t n, float w, const int64_t\* chunk_start, const int32_t\* chunk_n, int32_t chunks, void\*"
    assert re.search(proto, hdr) and re.search(proto, capi)
    assert len(lib.hulc_k_ema_update.argtypes) == 8
    from hulc_amd.engine import StepEngine
    for m in ("ema_enable", "ema_state", "ema_load", "ema_swap"):
        assert callable(getattr(StepEngine, m)), m
    assert isinstance(StepEngine.ema_swapped, property)


def test_refusals_decided_on_the_arguments(lib):
    buf = (ctypes.c_float * 4)()
    for bad in (0.0, 1.0, -0.5, 1.5, float("nan")):
        assert lib.hulc_ema_enable(None, buf, bad, 0, 1) != 0
        assert lib.hulc_last_error().startswith(b"hulc_ema_enable: need 0 < decay < 1"), (bad, lib.hulc_last_error())
    assert lib.hulc_ema_enable(None, buf, 0.9, -1, 1) != 0
    assert lib.hulc_last_error().startswith(b"hulc_ema_enable: need 0 < decay < 1 and start_step >= 0")
    assert lib.hulc_ema_enable(None, buf, 0.9, 0, 1) != 0
    assert lib.hulc_last_error() == b"hulc_ema_enable: null context"
    assert lib.hulc_ema_state_set(None, -1) != 0
    assert lib.hulc_last_error() == b"hulc_ema_state_set: updates -1 is negative"
    for name, args in (("hulc_ema_state_get", (None, None)), ("hulc_ema_state_set", (3,)), ("hulc_ema_swap", ())):
        assert getattr(lib, name)(None, *args) != 0
        assert lib.hulc_last_error() == name.encode() + b": null context"
    assert lib.hulc_ema_swapped(None, None) != 0
    assert lib.hulc_last_error() == b"hulc_ema_swapped: null argument"
    assert lib.hulc_k_ema_update(None, None, 4, 0.5, None, None, 0, None) != 0
    assert lib.hulc_last_error().startswith(b"hulc_k_ema_update: null or misaligned argument")


def test_decay_schedule():
    assert spec.ema_decay_at(1, 0.999) == 2.0 / 11.0
    d = [spec.ema_decay_at(n, 0.999) for n in range(1, 20001)]
    assert all(b >= a for a, b in zip(d, d[1:]))                      # monotone
    assert all(0.0 < x <= 0.999 for x in d) and d[-1] == 0.999        # ... up to `decay`, which it reaches
    first = next(n for n, x in enumerate(d, 1) if x == 0.999)
    assert first in (8990, 8991)                                      # (1 + n) / (10 + n) >= 0.999  <=>  n >= 8990 (8991 / 9000 may round below 0.999)
    assert spec.ema_decay_at(first - 1, 0.999) == (1.0 + first - 1) / (10.0 + first - 1) < 0.999
    assert [spec.ema_decay_at(n, 0.9, warmup=False) for n in (1, 2, 50, 10 ** 6)] == [0.9] * 4
    assert spec.ema_decay_at(1, 0.1) == 0.1                           # a decay below the ramp's first value is used as it is
    with pytest.raises(ValueError):
        spec.ema_decay_at(0, 0.9)


@pytest.mark.parametrize("bad", [1.0, 0, 0.0, -0.1, 1.5, float("nan"), "0.9"])
def test_module_refuses_a_decay_outside_the_open_interval_before_an_engine_is_built(bad, monkeypatch):
    from hulc_amd import hulc as H

    def no_engine(*a, **k):
        raise AssertionError("an engine was built before the decay was checked")
    monkeypatch.setattr(H, "StepEngine", no_engine)
    for cls in (H.Hulc, H.GCBC):
        with pytest.raises(ValueError, match="ema_decay"):
            cls(ema_decay=bad)
    with pytest.raises(ValueError, match="ema_start_step"):
        H.Hulc(ema_decay=0.9, ema_start_step=-1)


def test_options_are_reachable_from_the_training_cli():
    """`+model.ema_decay=0.999` lands in the model group that config.instantiate hands to the constructor, for both model classes; the conf files hold no EMA key."""
    from hulc_amd import config
    from hulc_amd.hulc import GCBC, Hulc
    from hulc_amd.training import CONF_DIR, config_fingerprint
    c = config.compose(CONF_DIR, "config", [])
    assert "ema_decay" not in c.model
    c = config.compose(CONF_DIR, "config", ["+model.ema_decay=0.999", "+model.ema_start_step=100", "+model.ema_warmup=false"])
    assert c.model.ema_decay == 0.999 and c.model.ema_start_step == 100 and c.model.ema_warmup is False
    assert config_fingerprint(c)["model"]["ema_decay"] == 0.999      # another average is another run
    c = config.compose(CONF_DIR, "config", ["model=gcbc", "+model.ema_decay=0.99"])
    assert c.model.ema_decay == 0.99
    for cls in (Hulc, GCBC):
        p = inspect.signature(cls.__init__).parameters
        assert p["ema_decay"].default is None and p["ema_start_step"].default == 0 and p["ema_warmup"].default is True
