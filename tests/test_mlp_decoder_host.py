"""Host tests (-m "not gpu") of the feed-forward action decoder body (action_decoder.rnn_model=mlp_decoder): the float64 restatement tests/mlp_decoder_ref.py
against the unmodified reference's recorded losses and float64 gradients (fixtures of tools/gen_golden_mlp.py), the parameter table against the reference's,
the rejected option mixes, the exported entry, and the GEMM routes of the body's M x 2048 x 2048 products."""
import os

import numpy as np
import pytest

import mlp_decoder_ref as R
from golden_util import rel_l2, sample_idx
from mlp_golden_util import BODY, MLP_CASES, RELU_POS, ROUTES, case_dims, fixture_table, load_manifest, load_mlp_case, route
from hulc_amd import config, spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AD = "action_decoder."
RNN8 = [f"{AD}rnn.{k}_l{l}" for l in (0, 1) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


# ---------------------------------------------------------------------------------------------------- the restatement against the reference
@pytest.mark.parametrize("name", list(MLP_CASES))
def test_restatement_reproduces_the_references_losses_and_float64_gradients(name):
    """train/action_loss_<scope> and the decoder's float64 gradients of the unmodified reference from the decoder inputs its float64 run recorded.  Loss gate as
    tests/test_det_decoder_host.py (1e-5 relative, against the fp32 run's logged value and the float64 run's); gradients 1e-6 rel-L2: the fixture stores the
    float64 gradients rounded to float32 (2^-24 relative per element)."""
    dims, P, batch, fx = load_mlp_case(name)
    grads = {}
    for sc, mb in batch.items():
        B, S_ = mb["actions"].shape[:2]
        assert RELU_POS[0] <= float(fx[f"relu_pos_a0_{sc}"]) <= RELU_POS[1] and RELU_POS[0] <= float(fx[f"relu_pos_a1_{sc}"]) <= RELU_POS[1]
        x = R.decoder_input(fx[f"plan_idx_{sc}"] if dims.kind == "hulc" else None, fx[f"emb64_{sc}"], fx[f"goal64_{sc}"])
        assert x.shape[-1] == dims.dec_in
        loss, g, _ = R.decoder_loss(P, x.reshape(B * S_, -1), fx[f"a_tcp_{sc}"].astype(np.float64).reshape(B * S_, 7), scale=1.0 / len(batch))
        ref64, ref32 = float(fx[f"log64/train/action_loss_{sc}"]), float(fx[f"log/train/action_loss_{sc}"])
        print(f"[{name}/{sc}] restated {loss:.9f} reference fp64 {ref64:.9f} fp32 {ref32:.7f}")
        assert abs(loss - ref64) <= 1e-5 * abs(ref64) and abs(loss - ref32) <= 1e-5 * abs(ref32), (sc, loss, ref64, ref32)
        for n, v in g.items():
            grads[n] = grads.get(n, 0.0) + v
    assert set(BODY) <= set(grads)
    for n, g in sorted(grads.items()):
        norm = float(fx["gradnorm64/" + n])
        assert abs(np.linalg.norm(g) - norm) <= 1e-6 * norm, (n, np.linalg.norm(g), norm)
        if "grad64/" + n in fx.files:
            err = rel_l2(g.reshape(-1), fx["grad64/" + n].reshape(-1).astype(np.float64))
        else:
            err = rel_l2(g.reshape(-1)[sample_idx(n, g.size)], fx["gradsamp64/" + n].astype(np.float64))
        print(f"   {n}: rel-L2 {err:.2e}")
        assert err <= 1e-6, (n, err)


def test_restatement_masks_matter():
    """the same restatement without one ReLU mask misses the fixture's gradients by far more than the gate: the fixture can tell"""
    dims, P, batch, fx = load_mlp_case("mlp_hulc")
    mb = batch["vis"]
    B, S_ = mb["actions"].shape[:2]
    x = R.decoder_input(fx["plan_idx_vis"], fx["emb64_vis"], fx["goal64_vis"]).reshape(B * S_, -1)
    W = tuple(P[f"{AD}rnn.{i}.{k}"].astype(np.float64) for i in (0, 2, 4) for k in ("weight", "bias"))
    a0, a1, y = R.body_fwd(x, W)
    dy = np.cos(np.arange(y.size, dtype=np.float64)).reshape(y.shape)
    g, da1, da0, _ = R.body_bwd(dy, x, a0, a1, W)
    assert rel_l2((dy @ W[4]).T @ a0, g[2]) > 0.1 and rel_l2((da1 @ W[2]).T @ x, g[0]) > 0.1
    assert np.array_equal(da1 == 0, ~(a1 > 0) | ((dy @ W[4]) == 0)) and np.array_equal(da0 == 0, ~(a0 > 0) | ((da1 @ W[2]) == 0))


# ---------------------------------------------------------------------------------------------------- parameter table, state dict
@pytest.mark.parametrize("name", list(MLP_CASES))
def test_param_table_equals_the_references_in_order(name):
    dims, P, batch, fx = load_mlp_case(name)
    ref = fixture_table(fx)
    table = [(n, tuple(s)) for n, s, _ in spec.param_table(dims)]
    assert dict(table) == dict(ref)
    dec_ref = [e for e in ref if e[0].startswith(AD)]
    dec = [e for e in table if e[0].startswith(AD)]
    assert dec == dec_ref, "the decoder's entries come in named_parameters order"
    kin = 1120 if dims.kind == "hulc" else 96
    assert dec[:6] == [(BODY[0], (2048, kin)), (BODY[1], (2048,)), (BODY[2], (2048, 2048)), (BODY[3], (2048,)), (BODY[4], (2048, 2048)), (BODY[5], (2048,))]
    assert [n for n, _ in dec[6:]] == [f"{AD}{h}.{k}" for h in ("mean_fc", "log_scale_fc", "prob_fc", "gripper_fc") for k in ("weight", "bias")]
    assert not any(n in dict(table) for n in RNN8)
    man = load_manifest()[name]
    assert [n for n, _ in table if n.startswith(AD)] == [n for n in man["order"] if n.startswith(AD)]
    assert {k: tuple(v["shape"]) for k, v in man["state_dict"].items() if v["param"]} == dict(table)
    buffers = {k for k, v in man["state_dict"].items() if not v["param"]}
    assert {b for b in buffers if b.startswith(AD)} == {AD + k for k in ("one_hot_embedding_eye", "ones", "action_max_bound", "action_min_bound", "gripper_bounds")}, \
        "the decoder's buffers are those of the recurrent body"
    # default init: nn.Linear's U(+-1/sqrt(fan_in)) — rnn.0 draws from 1/sqrt(KIN), not the RNN's 1/sqrt(2048)
    fans = {n: i[1] for n, _, i in spec.param_table(dims) if n in BODY}
    assert fans == {BODY[0]: kin, BODY[1]: kin, BODY[2]: 2048, BODY[3]: 2048, BODY[4]: 2048, BODY[5]: 2048}
    w0 = spec.init_all(dims, seed=0)[BODY[0]]
    assert 0.9 / np.sqrt(kin) < np.abs(w0).max() <= 1.0 / np.sqrt(kin)


def test_recurrent_table_is_unchanged():
    for kind in ("hulc", "gcbc", "mcil"):
        a = spec.param_table(spec.ModelDims(kind=kind, use_clip=kind != "mcil"))
        b = spec.param_table(spec.ModelDims(kind=kind, use_clip=kind != "mcil", decoder_body="rnn"))
        assert a == b and all(n in [x[0] for x in a] for n in RNN8) and BODY[0] not in [x[0] for x in a]
    rnn = [n for n, _, _ in spec.param_table(spec.ModelDims(kind="hulc", use_clip=True))]
    mlp = [n for n, _, _ in spec.param_table(case_dims(MLP_CASES["mlp_hulc"]))]
    i = rnn.index(RNN8[0])
    assert mlp[:i] == rnn[:i] and mlp[i:i + 6] == list(BODY) and mlp[i + 6:] == rnn[i + 8:], "the body's six tensors take the place of the recurrence's eight"
    for bad in (dict(kind="mcil", use_clip=False, decoder_body="mlp"), dict(decoder="deterministic", decoder_body="mlp"), dict(decoder_body="gru")):
        with pytest.raises(ValueError):
            spec.param_table(spec.ModelDims(**bad))


# ---------------------------------------------------------------------------------------------------- accepted and rejected options
def _kwargs(*overrides, kind="hulc", group=()):
    cfg = config.compose(os.path.join(ROOT, "conf"), "config", [f"model={kind}", *group, *overrides])
    kw = dict(cfg.model)
    kw.pop("_target_"), kw.pop("_recursive_", None)
    return kw


MLP = "model.action_decoder.rnn_model=mlp_decoder"


@pytest.mark.parametrize("overrides,kind,group,word", [
    ([MLP], "hulc", ("model/action_decoder=deterministic",), "deterministic"),
    ([MLP, "model.distribution.dist=continuous"], "hulc", (), "mcil"),
    ([MLP, "model.action_decoder.gripper_control=false"], "hulc", (), "mcil"),
    (["model.action_decoder.rnn_model=gru_decoder"], "hulc", (), "differs from the built architecture"),
    (["model.action_decoder.rnn_model=lstm_decoder"], "gcbc", (), "differs from the built architecture"),
    (["model.action_decoder.rnn_model=gru_decoder"], "hulc", ("model/action_decoder=deterministic",), "rnn_model"),
    ([MLP, "model.action_decoder.hidden_size=1024"], "hulc", (), "differs from the built architecture"),
])
def test_rejected_option_mixes_raise_before_any_engine_is_built(overrides, kind, group, word):
    from hulc_amd import hulc as H
    cls = H.Hulc if kind == "hulc" else H.GCBC
    with pytest.raises(NotImplementedError, match=word):
        cls(**_kwargs(*overrides, kind=kind, group=group))


def test_the_mlp_option_composes():
    for kind in ("hulc", "gcbc"):
        ad = config.compose(os.path.join(ROOT, "conf"), "config", [f"model={kind}", MLP]).model.action_decoder
        assert ad["rnn_model"] == "mlp_decoder" and "Logistic" in ad["_target_"]


# ---------------------------------------------------------------------------------------------------- the C-ABI entry and the routes
def test_library_exports_the_entry():
    from hulc_amd import lib as L
    lib = L.load()
    assert "hulc_decoder_body_select" in L.EXPORTS and hasattr(lib, "hulc_decoder_body_select")
    assert L.BODY == {"rnn": 0, "mlp": 1}
    hdr = open(os.path.join(ROOT, "include", "hulc_hip.h")).read()
    assert "#define HULC_BODY_RNN 0" in hdr and "#define HULC_BODY_MLP 1" in hdr and "int hulc_decoder_body_select(hulc_ctx* ctx, int32_t body);" in hdr
    assert lib.hulc_decoder_body_select(None, 1) != 0 and "null context" in lib.hulc_last_error().decode()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("M,want,bk", ROUTES)
def test_routes_of_the_bodys_products(M, want, bk, dtype):
    got = route(dtype, M)
    print(f"M = {M} {dtype}: {got}")
    assert got == (want, bk), (M, dtype, got)
