"""CPU: the float64 stage references of tests/tr_fused_ref.py against torch (nn.TransformerEncoderLayer in double, and a plain torch-double restatement of
the layer under explicit dropout masks with autograd for every gradient the GPU tests compare), the input conditions tests/test_gpu_tr_fused.py relies on, and
every measured number of tests/tr_fused_inputs.py re-measured from the references alone."""
import numpy as np
import pytest
import torch

import tr_fused_inputs as I
import tr_fused_ref as T

REL = 1e-10


def close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    e = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)
    assert e <= REL, f"{what}: relative error {e:.3g}"


def td(a):
    return torch.from_numpy(np.array(a, dtype=np.float64))


@pytest.mark.parametrize("B,S", [(1, 1), (3, 17), (2, 40)])
def test_stages_chained_equal_torch_transformer_encoder_layer(B, S):
    """no dropout, no 16-bit rounding: LayerNorm2 of the chain's y2 is the output of nn.TransformerEncoderLayer (double, eval, post-LN, relu)"""
    P = I.params("bf16")
    layer = torch.nn.TransformerEncoderLayer(T.D, T.NH, T.FF, dropout=0.1, activation="relu", batch_first=True, norm_first=False).double().eval()
    with torch.no_grad():
        a = layer.self_attn
        a.in_proj_weight.copy_(td(P["Wqkv"])); a.in_proj_bias.copy_(td(P["bqkv"])); a.out_proj.weight.copy_(td(P["Wo"])); a.out_proj.bias.copy_(td(P["bo"]))
        layer.linear1.weight.copy_(td(P["W1"])); layer.linear1.bias.copy_(td(P["b1"])); layer.linear2.weight.copy_(td(P["W2"])); layer.linear2.bias.copy_(td(P["b2"]))
        layer.norm1.weight.copy_(td(P["n1g"])); layer.norm1.bias.copy_(td(P["n1b"])); layer.norm2.weight.copy_(td(P["n2g"])); layer.norm2.bias.copy_(td(P["ln_b"]))
    x = I.xin(B, S, 0)
    c = T.chain_fwd(x, P, B, S, 0, 0.0, None)
    out = T.ln(c["y2"], P["n2g"], P["ln_b"])[0]
    ref = layer(td(x).reshape(B, S, T.D).requires_grad_(True)).detach().numpy().reshape(B * S, T.D)
    close(out, ref, "encoder layer output")
    # the same behind the previous layer's norm2 (ln_in): the layer applied to LayerNorm(xin)
    xl = I.xin(B, S, 1)
    c = T.chain_fwd(xl, P, B, S, 1, 0.0, None)
    xn = torch.nn.functional.layer_norm(td(xl), (T.D,), td(P["ln_g"]), td(P["ln_b"]), 1e-5)
    close(c["xf_out"], xn.numpy(), "ln_in output")
    ref = layer(xn.reshape(B, S, T.D).requires_grad_(True)).detach().numpy().reshape(B * S, T.D)
    close(T.ln(c["y2"], P["n2g"], P["ln_b"])[0], ref, "encoder layer output behind ln_in")


def torch_layer(x, t, B, S, p, mk, y2_0):
    """the layer restated in torch double with explicit multiplier masks, bias of linear2 inside its dropout as in the model (x1 + drop(linear2(...)));
    every intermediate the kernels save, or whose gradient they write, keeps its gradient.  t: dict of (leaf) parameter tensors"""
    m = {k: td(np.where(v, T.mult(p), 0.0)) for k, v in mk.items()}
    s = {}

    def keep(name, v):
        v.retain_grad()
        s[name] = v
        return v
    qkv = keep("qkv", x @ t["Wqkv"].T + t["bqkv"])
    q, k, v = qkv.reshape(B, S, 3, T.NH, T.HD).permute(2, 0, 3, 1, 4)
    Pat = keep("Pat", torch.softmax(q @ k.transpose(-1, -2) / 4.0, -1))
    ao = keep("ao", ((Pat * m["att"]) @ v).permute(0, 2, 1, 3).reshape(B * S, T.D))
    z1 = keep("z1", ao @ t["Wo"].T + t["bo"])
    y1 = keep("y1", x + m["o"] * z1)
    x1 = keep("x1", torch.nn.functional.layer_norm(y1, (T.D,), t["n1g"], t["n1b"], 1e-5))
    a1 = keep("a1", x1 @ t["W1"].T + t["b1"])
    h = keep("hff", m["h"] * torch.relu(a1))
    z2 = keep("z2", h @ t["W2"].T + t["b2"])
    s["out"] = torch.nn.functional.layer_norm(keep("y2", td(y2_0) + x1 + m["y"] * z2), (T.D,), t["n2g"], t["ln_b"], 1e-5)
    return s


@pytest.mark.parametrize("B,S,p", [(3, 17, 0.1), (1, 33, 0.5), (2, 2, 0.5)])
def test_stages_under_masks_equal_torch_restatement_and_autograd(B, S, p):
    """explicit masks, no rounding: every forward tensor and every gradient the GPU tests compare, parameter gradients of both norms included"""
    P = I.params("fp16")
    mk = I.masks(B, S, p)
    x, y2_0 = I.xin(B, S, 0), I.y2_start(B, S, True)
    c = T.chain_fwd(x, P, B, S, 0, p, mk, y2_0=y2_0)
    leaf = {k: td(v).requires_grad_(True) for k, v in P.items()}
    t_in = td(x).requires_grad_(True)
    s = torch_layer(t_in, leaf, B, S, p, mk, y2_0)
    for name in ("qkv", "Pat", "ao", "y1", "hff", "y2"):
        close(c[name], s[name].detach().numpy(), name)
    close(c["x1f"], s["x1"].detach().numpy(), "x1")
    dx2 = I.ffn_bwd_dx(B, S, 0)
    s["out"].backward(td(dx2))
    st2 = T.ln(c["y2"], P["n2g"], P["ln_b"])[1]
    g = T.chain_bwd(c, P, B, S, p, mk, dx2, st2, P["n2g"])
    gr = lambda name: s[name].grad.numpy()
    close(g["dy2"], gr("y2"), "dy2")
    close(g["dg2"], leaf["n2g"].grad.numpy(), "dg2")
    close(g["db2"], leaf["ln_b"].grad.numpy(), "db2")
    close(g["dt_c"], gr("z2"), "dt_c")
    close(g["dt_a"], gr("a1"), "dt_a")
    close(g["parts"].sum(0), gr("x1"), "sum of the partials")
    close(g["dy_f"], gr("y1"), "dy_f")
    close(g["dg1"], leaf["n1g"].grad.numpy(), "dg1")
    close(g["db1"], leaf["n1b"].grad.numpy(), "db1")
    close(g["b_d"], gr("z1"), "b_d")
    close(g["b_b"], gr("qkv"), "b_b")
    close(g["dx"], t_in.grad.numpy(), "dx")
    # the hidden-quarter slabs: slab q carries its own 512 hidden units, dy2 sits in slab 0 only
    for q in range(T.NQ):
        ref = gr("a1")[:, q * T.HQ:(q + 1) * T.HQ] @ P["W1"][q * T.HQ:(q + 1) * T.HQ] + (gr("y2") if q == 0 else 0.0)
        close(g["parts"][q], ref, f"partial {q}")
    # the broadcast form: one row per window divided by S stands for S equal rows
    dxw = I.ffn_bwd_dx(B, S, 1)
    close(T.bcast_rows(dxw, S, float(S)).reshape(B, S, T.D).sum(1), dxw, "broadcast rows")


def test_accumulation_bounds_hold_for_fp32_arithmetic():
    """the bounds that gate the GPU tests, against the same sums carried out in float32 on the host (any order of summation obeys them)"""
    P, B, S, p = I.params("bf16"), 3, 17, 0.1
    mk, c = I.masks(B, S, p), I.host_forward("bf16", B, S, 0, p)
    f = lambda a: np.asarray(a, np.float32)
    ref, bnd = T.qkv(c["xt"], P["Wqkv"], P["bqkv"])
    assert (np.abs((f(c["xt"]) @ f(P["Wqkv"]).T + f(P["bqkv"])).astype(np.float64) - ref) <= bnd).all() and (bnd > 0).all()
    ref, bnd = T.y2(c["y2_0"], c["x1f"], c["hff"], P["W2"], P["b2"], mk["y"], p)
    got = f(c["y2_0"]) + f(c["x1f"]) + f(np.where(mk["y"], T.mult(p), 0.0)) * (f(c["hff"]) @ f(P["W2"]).T + f(P["b2"]))
    assert (np.abs(got.astype(np.float64) - ref) <= bnd).all()
    assert bnd.max() < 1e-3 * np.abs(ref).max(), "the bound stays far below what a defect would change"


def test_input_conditions():
    for dtype in I.DTYPES16:
        P = I.params(dtype)
        for k in ("n1g", "ln_g", "n2g"):
            assert np.abs(P[k] - 1).min() > 0 and np.abs(P[k] - 1).max() > 0.3, "LayerNorm gains carry jitter"
        for k in ("n1b", "ln_b", "bqkv", "bo", "b1", "b2"):
            assert (P[k] != 0).all() and np.abs(P[k]).max() > 0.2, k
        for S in sorted(set(I.S_FWD + I.S_ATTN)):
            for B in I.BS:
                for ln_in in (0, 1):
                    c = I.host_forward(dtype, B, S, ln_in, 0.0)
                    if S >= 8:
                        assert 0.15 < c["Pat"].max() < 0.95, (dtype, B, S, ln_in, c["Pat"].max())
                    assert 0.3 < (c["hff"] > 0).mean() < 0.7, (dtype, B, S, ln_in)
    for B, S, p in ((1, 15, 0.1), (3, 33, 0.5), (3, 2, 0.5)):
        for k, m in I.masks(B, S, p).items():
            assert 0 < (~m).sum() < m.size, (k, B, S, p)
    assert I.masks(3, 64, 0.5)["h"].mean() == pytest.approx(0.5, abs=0.01)
    assert (I.y2_start(3, 5, True) != 0).all() and (I.param_grad_start("dg", True) != 0).all()
    for ln_in in (0, 1):          # the low-variance rows: the LayerNorm's epsilon is more than 1 % of their rstd, and 10 x less of it would show far above LN_STAT
        x = I.xin(3, 17, ln_in)
        for r in (0, 16):
            v = x[r].var()
            assert v < 1e-3 and abs(np.sqrt((v + 1e-5) / (v + 1e-6)) - 1) > 100 * 2e-5, (ln_in, r, v)
    a, b = I.xin(3, 17, 1), I.xin(3, 17, 1, other=(0, 2))
    assert (a[17:34] == b[17:34]).all() and (a[:17] != b[:17]).any() and (a[34:] != b[34:]).any()


@pytest.mark.parametrize("dtype", I.DTYPES16)
def test_dao_rounding_allowance_is_what_the_references_measure(dtype):
    """tr_fused_inputs.BB_DAO: every recorded number is the host measurement rounded up by at most a tenth"""
    for B in I.BS:
        for S in I.S_ATTN:
            for p in I.DPS:
                rec, got = I.BB_DAO[(dtype, B, S, p)], I.bb_measure(dtype, B, S, p)
                for r, m in zip(rec, got):
                    assert m <= r <= 1.1 * m + 1e-300, (dtype, B, S, p, rec, got)
