"""Host tests (-m "not gpu") of the deterministic action decoder: the composed config option, the parameter table against the reference's (fixtures of
tools/gen_golden_det.py), the rejected options, the float64 restatement tests/det_head_ref.py against torch autograd and against the reference's recorded
losses, and every tabulated float32 figure behind the gates of tests/test_gpu_det_head.py."""
import os

import numpy as np
import pytest
import torch

import det_head_inputs as I
import det_head_ref as R
from det_golden_util import DET_CASES, HEAD_SCALE, HEAD_W, VAL_DET_CASES, case_batch, case_dims, case_params, fixture_table, load_det_case, load_manifest
from hulc_amd import config, spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS = ("mean_fc", "log_scale_fc", "prob_fc", "gripper_fc")


def compose(*overrides):
    return config.compose(os.path.join(ROOT, "conf"), "config", ["model=hulc", "model/action_decoder=deterministic", *overrides])


# ---------------------------------------------------------------------------------------------------- config option, parameter table, state dict
def test_config_option_composes_with_the_reference_keys():
    ad = compose().model.action_decoder
    assert ad["_target_"] == "hulc.models.decoders.deterministic_decoder.DeterministicDecoder"
    want = dict(criterion="HuberLoss", hidden_size=2048, num_layers=2, rnn_model="rnn_decoder", policy_rnn_dropout_p=0.0, gripper_control=True, out_features=7,
                latent_goal_features=32)
    for k, v in want.items():
        assert ad[k] == v, (k, ad[k])
    assert list(ad["perceptual_emb_slice"]) == [64, 128]
    assert set(ad.keys()) == set(want) | {"_target_", "perceptual_emb_slice", "perceptual_features", "plan_features"}, "the reference option's key set"
    assert compose("model.action_decoder.criterion=MSELoss").model.action_decoder["criterion"] == "MSELoss"
    assert "Logistic" in config.compose(os.path.join(ROOT, "conf"), "config", ["model=hulc"]).model.action_decoder["_target_"], "the default stays the mixture"


@pytest.mark.parametrize("name", list(DET_CASES))
def test_param_table_and_layout_match_the_reference(name):
    dims, P, batch, fx = load_det_case(name)
    ref = dict(fixture_table(fx))
    table = {n: tuple(s) for n, s, _ in spec.param_table(dims)}
    assert table == ref
    assert table["action_decoder.actions.0.weight"] == (7, 2048) and table["action_decoder.actions.0.bias"] == (7,)
    assert not any(h in n for n in table for h in HEADS)
    layout, numel = spec.layout(dims)
    assert set(layout) == set(ref) and all(tuple(layout[n][1]) == ref[n] for n in ref)
    offs = sorted((off, int(np.prod(shape)) if len(shape) else 1) for off, shape in layout.values())
    assert all(a[0] + a[1] <= b[0] for a, b in zip(offs, offs[1:])) and offs[-1][0] + offs[-1][1] <= numel and all(o % 64 == 0 for o, _ in offs)
    assert float(fx["meta/head_scale"]) == HEAD_SCALE
    assert np.array_equal(P[HEAD_W], (spec.init_all(dims, seed=DET_CASES[name]["seed"], ln_jitter=True)[HEAD_W] * np.float32(HEAD_SCALE)))


def test_logistic_table_is_unchanged():
    """a logistic config produces today's table: the four mixture heads, no actions.0, the same names in the same order whether or not the new fields are given"""
    for kind in ("hulc", "gcbc", "mcil"):
        a = spec.param_table(spec.ModelDims(kind=kind, use_clip=kind != "mcil"))
        b = spec.param_table(spec.ModelDims(kind=kind, use_clip=kind != "mcil", decoder="logistic", criterion="MSELoss"))
        assert a == b
        names = [n for n, _, _ in a]
        assert "action_decoder.actions.0.weight" not in names
        assert [n for n in names if n.startswith("action_decoder.") and "rnn" not in n] == \
            [f"action_decoder.{h}.{k}" for h in HEADS[:3 if kind == "mcil" else 4] for k in ("weight", "bias")]
    det = [n for n, _, _ in spec.param_table(case_dims(DET_CASES["det_huber_hulc"]))]
    log = [n for n, _, _ in spec.param_table(spec.ModelDims(kind="hulc", use_clip=True))]
    assert [n for n in det if "action_decoder.rnn." in n] == [n for n in log if "action_decoder.rnn." in n], "the recurrence's entries do not change"
    i, j = det.index("action_decoder.actions.0.weight"), log.index("action_decoder.mean_fc.weight")
    assert det[:i] == log[:j] and det[i + 2:] == log[j + 8:], "the head's two tensors take the place of the mixture heads' eight"
    for bad in (dict(kind="gcbc", decoder="deterministic"), dict(kind="mcil", use_clip=False, decoder="deterministic"), dict(decoder="deterministic", criterion="L1Loss"),
                dict(decoder="gaussian")):
        with pytest.raises(ValueError):
            spec.param_table(spec.ModelDims(**bad))


def test_state_manifest_is_the_spec_layout():
    """tests/golden/state_manifest_det.json = the reference's state_dict() of this configuration: the parameter keys and shapes are the table's; its buffers
    are the static camera's spatial softmax maps only (DeterministicDecoder registers none) — what load_state_dict(strict=True) accepts."""
    man = load_manifest()["hulc_det_w32"]["state_dict"]
    table = {n: list(s) for n, s, _ in spec.param_table(case_dims(DET_CASES["det_huber_hulc"]))}
    assert {k: v["shape"] for k, v in man.items() if v["param"]} == table
    buffers = {k for k, v in man.items() if not v["param"]}
    assert buffers == {"perceptual_encoder.rgb_static_encoder.spatial_softmax." + k for k in ("x_map", "y_map", "temperature")}


# ---------------------------------------------------------------------------------------------------- rejected options
def _hulc_kwargs(*overrides, kind="hulc"):
    cfg = config.compose(os.path.join(ROOT, "conf"), "config", [f"model={kind}", "model/action_decoder=deterministic", *overrides])
    kw = dict(cfg.model)
    kw.pop("_target_"), kw.pop("_recursive_", None)
    return kw


@pytest.mark.parametrize("overrides,kind,word", [
    (["model.action_decoder.criterion=L1Loss"], "hulc", "HuberLoss and MSELoss"),
    (["model.action_decoder.gripper_control=false"], "hulc", "gripper_control"),
    (["model.action_decoder.hidden_size=1024"], "hulc", "hidden_size"),
    (["model.action_decoder.num_layers=1"], "hulc", "num_layers"),
    (["model.action_decoder.rnn_model=gru_decoder"], "hulc", "rnn_model"),
    (["model.action_decoder.policy_rnn_dropout_p=0.1"], "hulc", "policy_rnn_dropout_p"),
    (["model.action_decoder.perceptual_emb_slice=[0,128]"], "hulc", "perceptual_emb_slice"),
    (["model.action_decoder.out_features=8"], "hulc", "out_features"),
    ([], "gcbc", "gcbc"),
    (["model.distribution.dist=continuous"], "hulc", "mcil"),
])
def test_rejected_options_raise_before_any_engine_is_built(overrides, kind, word):
    from hulc_amd import hulc as H
    cls = H.Hulc if kind == "hulc" else H.GCBC
    with pytest.raises(NotImplementedError, match=word):
        cls(**_hulc_kwargs(*overrides, kind=kind))


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("frame", I.FRAMES)
@pytest.mark.parametrize("crit", I.CRITERIA)
def test_restatement_matches_torch_autograd(crit, frame):
    B, S = 5, 3
    H1, W, bias, act, ro = I.operands(B, S, "fp32")
    r = R.loss(H1, W, bias, act, ro, crit, frame, I.GRAD_SCALE)
    dH1, dZ1, dW, db = R.bwd(r["dpre"], W, H1, I.last_rows(B, S))
    t_loss, t_dH1, t_dW, t_db, t_dpre = R.torch_autograd(H1, W, bias, act, ro, crit, frame, I.GRAD_SCALE)
    for got, ref, what in ((r["row_loss"], t_loss, "row_loss"), (r["dpre"], t_dpre, "dpre"), (dH1, t_dH1, "dH1"), (dW, t_dW, "dW"), (db, t_db, "db")):
        assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), what
    assert np.array_equal(dZ1, np.where(H1[I.last_rows(B, S)] > 0, dH1[I.last_rows(B, S)], 0.0))
    a6 = np.concatenate([r["p"][:, :6], act[:, 6:]], -1)          # tcp -> world -> tcp is the identity on the six continuous dimensions
    from enc_head_ref import world_to_tcp
    assert np.abs(world_to_tcp(R.tcp_to_world(a6, ro), ro) - a6)[:, :6].max() <= 1e-9


@pytest.mark.parametrize("name", list(DET_CASES))
def test_restatement_reproduces_the_references_training_loss(name):
    """train/action_loss_<scope> of the unmodified reference from its own recorded decoder states: the criterion against the WORLD-frame actions"""
    dims, P, batch, fx = load_det_case(name)
    crit = R.MSE if DET_CASES[name]["criterion"] == "MSELoss" else R.HUBER
    n_hi = n_lo = 0
    for sc, mb in batch.items():
        B, S_ = mb["actions"].shape[:2]
        H1 = fx[f"dec_h1_{sc}"].astype(np.float64).reshape(B * S_, 2048)
        r = R.loss(H1, P[HEAD_W].astype(np.float64), P["action_decoder.actions.0.bias"].astype(np.float64), mb["actions"].astype(np.float64).reshape(B * S_, 7),
                   mb["robot_obs"].astype(np.float64).reshape(B * S_, 15), crit, 0)
        got, ref = float(r["row_loss"].mean()), float(fx[f"log/train/action_loss_{sc}"])
        print(f"[{name}/{sc}] restated {got:.7f} reference {ref:.7f}")
        assert abs(got - ref) <= 1e-5 * abs(ref), (sc, got, ref)
        tcp = float(R.loss(H1, P[HEAD_W].astype(np.float64), P["action_decoder.actions.0.bias"].astype(np.float64), mb["actions"].astype(np.float64).reshape(B * S_, 7),
                           mb["robot_obs"].astype(np.float64).reshape(B * S_, 15), crit, 1)["row_loss"].mean())
        assert abs(tcp - ref) > 1e-2 * abs(ref), "the tcp-frame criterion is a different number: the fixture tells the two frames apart"
        n_hi += int((np.abs(r["d"]) > 1.2).sum())
        n_lo += int((np.abs(r["d"]) < 0.8).sum())
    assert n_hi >= 10 and n_lo >= 10, (n_hi, n_lo)          # both Huber branches, with margin


# ---------------------------------------------------------------------------------------------------- the gates of the GPU kernel tests
def recorded(value, measured):
    """a recorded float32-vs-float64 figure is the measured one, rounded up by at most a tenth"""
    return measured <= value * (1 + 1e-6) and value <= 1.1 * measured


def test_kernel_gates_are_five_times_the_float32_error():
    assert set(I.LOSS_F32) == {(B, S, d, c, f) for B, S in I.CASES for d in I.DTYPES for c in I.CRITERIA for f in I.FRAMES}
    assert set(I.BWD_F32) == {(B, S, d) for B, S in I.CASES for d in I.DTYPES}
    for key, v in I.LOSS_F32.items():
        m = I.loss_measure(*key)
        assert all(recorded(a, b) for a, b in zip(v, m)), (key, m, v)
        assert I.LOSS_GATE[key] == tuple(5 * a for a in v)
    for key, v in I.BWD_F32.items():
        m = I.bwd_measure(*key)
        assert all(recorded(a, b) for a, b in zip(v, m)), (key, m, v)
        assert I.BWD_GATE[key] == tuple(5 * a for a in v)


def test_kernel_inputs_cover_both_branches_and_saturation():
    for B, S in I.CASES:
        for f in I.FRAMES:
            r = I.reference(B, S, "bf16", R.HUBER, f)
            d = np.abs(r["d"])
            assert (d > 1).any() and (d < 1).any() and (np.abs(r["pre"]) > 6).any(), (B, S, f)
        H1 = I.inputs(B, S)[0]
        assert (H1 == 0).any() and (H1 > 0).any()
    assert I.CASES[-1][0] * I.CASES[-1][1] == 258 and I.CASES[1][0] * I.CASES[1][1] % 4 != 0
