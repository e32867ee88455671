"""CPU (-m "not gpu"): the host side of the BC-Z / MIA language auxiliary losses — the parameter table against the reference's own (stored in the
fixtures of tools/gen_golden_aux.py), the constructor's accept / reject matrix, the three C-ABI entry points, the conf groups."""
import os
import re

import numpy as np
import pytest

from aux_golden_util import AUX_CASES, VAL_AUX_CASES, case_dims, fixture_table, load_aux_case
from hulc_amd import config, spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BCZ = [("bc_z_lang_decoder.mlp.0.weight", (512, 4096)), ("bc_z_lang_decoder.mlp.0.bias", (512,)), ("bc_z_lang_decoder.mlp.2.weight", (384, 512)),
       ("bc_z_lang_decoder.mlp.2.bias", (384,))]
MIA = [("mia_lang_discriminator.mlp.0.weight", (512, 64)), ("mia_lang_discriminator.mlp.0.bias", (512,)), ("mia_lang_discriminator.mlp.3.weight", (1, 512)),
       ("mia_lang_discriminator.mlp.3.bias", (1,))]


def _table(d):
    return [(n, tuple(s)) for n, s, _ in spec.param_table(d)]


@pytest.mark.parametrize("name", list(AUX_CASES) + list(VAL_AUX_CASES))
def test_param_table_is_the_references(name):
    """Names and shapes of every flag combination the fixtures cover — CLIP + MIA, MIA without CLIP (proj_vis_lang.* but no logit_scale), CLIP + BC-Z,
    all three — equal the reference module's named_parameters()."""
    dims, P, batch, fx = load_aux_case(name)
    ours, ref = dict(_table(dims)), dict(fixture_table(fx))
    assert set(ours) == set(ref), set(ours) ^ set(ref)
    assert all(tuple(ours[n]) == tuple(ref[n]) for n in ref), [(n, ours[n], ref[n]) for n in ref if tuple(ours[n]) != tuple(ref[n])]
    assert set(P) == set(ref)
    c = (AUX_CASES.get(name) or VAL_AUX_CASES[name])
    assert ("logit_scale" in ours) == c["clip"] and ("proj_vis_lang.mlp_im.0.weight" in ours) == (c["clip"] or c["mia"])


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("bcz", [False, True])
@pytest.mark.parametrize("mia", [False, True])
@pytest.mark.parametrize("kind", ["hulc", "gcbc"])
def test_heads_are_appended_and_the_rest_of_the_table_does_not_move(kind, clip, bcz, mia):
    base = spec.ModelDims(kind=kind, use_clip=clip)
    d = spec.ModelDims(kind=kind, use_clip=clip, use_bc_z=bcz, use_mia=mia)
    tb, t = _table(base), _table(d)
    proj = [x for x in _table(spec.ModelDims(kind=kind, use_clip=True)) if x[0].startswith("proj_vis_lang.")]
    want = [x for x in tb if x[0] != "logit_scale" and not x[0].startswith("proj_vis_lang.")]
    want += proj if (clip or mia) else []
    want += [("logit_scale", ())] if clip else []
    want += (BCZ if bcz else []) + (MIA if mia else [])
    assert t == want
    if not bcz and not mia:          # flags off: table, layout and counts are the parent's
        assert spec.param_table(d) == spec.param_table(base) and spec.layout(d) == spec.layout(base) and spec.n_params(d) == spec.n_params(base)
    lay, numel = spec.layout(d)
    lay_b, numel_b = spec.layout(base)
    if clip or not mia:              # every tensor of the flags-off table keeps its offset: the heads only extend the buffer
        assert all(lay[n] == lay_b[n] for n in lay_b) and numel >= numel_b
    # the heads sit behind the action decoder: inside the first all-reduce bucket [action_decoder.lo, numel)
    dec_lo = min(off for n, (off, _) in lay.items() if n.startswith("action_decoder."))
    assert all(lay[n][0] > dec_lo for n, _ in (BCZ if bcz else []) + (MIA if mia else []))
    for n, s, i in spec.param_table(d):          # the heads initialise like torch's nn.Linear: U(+-1/sqrt(fan_in))
        if n.startswith(("bc_z_lang_decoder.", "mia_lang_discriminator.")):
            v = spec.init_param(n, s, i, seed=3)
            assert v.shape == tuple(s) and i[0] == "u" and np.abs(v).max() <= 1.0 / np.sqrt(i[1])


def test_default_dims_have_no_heads():
    d = spec.ModelDims()
    assert d.use_bc_z is False and d.use_mia is False
    assert not any(n.startswith(("bc_z_lang_decoder.", "mia_lang_discriminator.")) for n, _ in _table(d))


def _construct(**kw):
    """Hulc(**kw) as far as this machine allows: the option checks run before the engine is created, so without a GPU an accepted configuration ends in the
    engine's 'needs a HIP device' error and a rejected one in its own exception."""
    from hulc_amd.hulc import GCBC, Hulc
    cls = GCBC if kw.pop("gcbc", False) else Hulc
    try:
        m = cls(precision="fp32", max_batch_size=2, max_seq_len=4, **kw)
    except RuntimeError as e:
        if "HIP device" in str(e):
            return "accepted"
        raise
    m.engine.close()
    return "accepted"


BCZ_CFG = dict(_target_="hulc.models.auxiliary_loss_networks.bc_z_lang_decoder.BCZLangDecoder", in_features=4096, lang_dim=384)
MIA_CFG = dict(_target_="hulc.models.auxiliary_loss_networks.mia_lang_discriminator.MIALangDiscriminator", in_features=32, lang_dim=32, dropout_p=0.0)


def test_constructor_accepts_the_four_options():
    assert _construct(use_bc_z_auxiliary_loss=True, bc_z_lang_decoder=BCZ_CFG) == "accepted"
    assert _construct(use_clip_auxiliary_loss=False, use_mia_auxiliary_loss=True, mia_lang_discriminator=MIA_CFG) == "accepted"
    assert _construct(gcbc=True, use_bc_z_auxiliary_loss=True, bc_z_lang_decoder=BCZ_CFG, use_mia_auxiliary_loss=True, mia_lang_discriminator=MIA_CFG) == "accepted"
    assert _construct(bc_z_lang_decoder={}, mia_lang_discriminator={}) == "accepted"          # the `none` options of the two groups


def test_constructor_rejects():
    with pytest.raises(ValueError, match="bc_z_lang_decoder"):
        _construct(use_bc_z_auxiliary_loss=True)
    with pytest.raises(ValueError, match="use_bc_z_auxiliary_loss"):
        _construct(bc_z_lang_decoder=BCZ_CFG)
    with pytest.raises(ValueError, match="mia_lang_discriminator"):
        _construct(use_mia_auxiliary_loss=True)
    with pytest.raises(ValueError, match="use_mia_auxiliary_loss"):
        _construct(mia_lang_discriminator=MIA_CFG)
    with pytest.raises(NotImplementedError, match="proprio encoder"):
        _construct(state_recons=True)
    with pytest.raises(NotImplementedError, match="dropout_p"):
        _construct(use_mia_auxiliary_loss=True, mia_lang_discriminator=dict(MIA_CFG, dropout_p=0.1))
    with pytest.raises(NotImplementedError, match="in_features"):
        _construct(use_mia_auxiliary_loss=True, mia_lang_discriminator=dict(MIA_CFG, in_features=64))
    with pytest.raises(NotImplementedError, match="lang_dim"):
        _construct(use_bc_z_auxiliary_loss=True, bc_z_lang_decoder=dict(BCZ_CFG, lang_dim=768))
    with pytest.raises(NotImplementedError, match="in_features"):
        _construct(use_bc_z_auxiliary_loss=True, bc_z_lang_decoder=dict(BCZ_CFG, in_features=2048))
    mcil = dict(distribution=dict(dist="continuous", plan_features=256), plan_recognition=dict(_target_="x.PlanRecognitionBiRNNNetwork", plan_features=256),
                action_decoder=dict(gripper_control=False, discrete_gripper=False, perceptual_emb_slice=None, num_classes=256), use_clip_auxiliary_loss=False)
    with pytest.raises(NotImplementedError, match="mcil"):
        _construct(use_mia_auxiliary_loss=True, mia_lang_discriminator=MIA_CFG, **mcil)
    with pytest.raises(NotImplementedError, match="mcil"):
        _construct(use_bc_z_auxiliary_loss=True, bc_z_lang_decoder=BCZ_CFG, **mcil)


def test_c_abi_declares_and_exports_the_three_calls():
    from hulc_amd import lib
    hdr = open(os.path.join(ROOT, "include", "hulc_hip.h")).read()
    for name, args in (("hulc_aux_heads_enable", r"hulc_ctx\* ctx, int32_t bc_z, int32_t mia"), ("hulc_aux_weights_set", r"hulc_ctx\* ctx, float bc_z_weight, float mia_weight"),
                       ("hulc_aux_losses_get", r"hulc_ctx\* ctx, float\* out_host")):
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*" + args, hdr), name
        assert name in lib.EXPORTS
        assert hasattr(lib.load(), name), f"{name} is not exported by the built library"


def test_conf_groups_compose():
    conf = os.path.join(ROOT, "conf")
    for grp in ("bc_z_lang_decoder", "mia_lang_discriminator"):
        for opt in ("default", "none"):
            assert os.path.exists(os.path.join(conf, "model", grp, opt + ".yaml"))
    for model in ("hulc", "gcbc"):
        c = config.compose(conf, "config", [f"model={model}"])
        assert not c.model.bc_z_lang_decoder and not c.model.mia_lang_discriminator
        assert c.model.use_bc_z_auxiliary_loss is False and c.model.use_mia_auxiliary_loss is False
        c = config.compose(conf, "config", [f"model={model}", "model.use_mia_auxiliary_loss=true", "model/mia_lang_discriminator=default",
                                            "model.use_bc_z_auxiliary_loss=true", "model/bc_z_lang_decoder=default"])
        assert dict(c.model.bc_z_lang_decoder) == BCZ_CFG and dict(c.model.mia_lang_discriminator) == MIA_CFG
        assert c.model.use_bc_z_auxiliary_loss is True and c.model.use_mia_auxiliary_loss is True
        assert c.model.bc_z_auxiliary_loss_beta == 1.0 and c.model.mia_auxiliary_loss_beta == 1.0
        assert not config.missing_keys(c.model.bc_z_lang_decoder) and not config.missing_keys(c.model.mia_lang_discriminator)
