"""Host: tests/enc_head_ref.py (the float64 references the GPU tests of the encoder head and the action loss compare against) pinned to the functions of
oracle/hulc_oracle.py that the golden fixtures pin to the reference implementation.

Bounds.  The oracle's functions accept float64 inputs but cast what they return (and some constants: the linspace coordinates, the half-bin width, cached
probabilities and LayerNorm statistics) to float32, so 1e-10 is out of reach against them: a float32 cast costs 2^-24 = 6e-8 relative per value.  Against the
oracle the bound is therefore CAST = 2e-7 of the tensor's largest magnitude (4 CAST where a result is a product of several cast values); each test says which.
What the oracle cannot pin to 1e-10 is pinned to float64 arithmetic directly: definitions written out element by element and central differences.

The last two tests re-measure, on the host, every measured gate of the GPU tests (tests/enc_head_inputs.py), so that no gate rests on a kernel's output."""
import numpy as np
import pytest

import enc_head_inputs as I
import enc_head_ref as R
import hulc_oracle as O

CAST = 2e-7


def close(got, ref, tol):
    ref = np.asarray(ref, np.float64)
    return np.abs(np.asarray(got, np.float64) - ref).max() <= tol * max(np.abs(ref).max(), 1e-300)


@pytest.mark.parametrize("H", [3, 7, 21])
def test_spatial_softmax_equals_oracle_on_square_maps(H):
    """CAST bound: the oracle's linspace coordinates, probabilities and outputs are float32."""
    rng = np.random.default_rng(H)
    f = np.abs(rng.standard_normal((3, H, H, 5))) * 3 + 0.01          # > 0 everywhere: the oracle's backward has no ReLU mask
    out, st = R.spatial_softmax_fwd(f)
    o_out, cache = O.spatial_softmax(f.transpose(0, 3, 1, 2))
    assert close(out, o_out, CAST)
    dout = rng.standard_normal((3, 10))
    df = R.spatial_softmax_bwd(f, st, dout)
    o_df = O.spatial_softmax_bwd(dout, cache, (3, 5, H, H))
    assert close(df.transpose(0, 3, 1, 2), o_df, 4 * CAST)          # p, ex, ey float32 in the oracle's cache: a product of three cast values
    # statistics: exp(f - max) / sum is the oracle's softmax
    p = np.exp(f.reshape(3, H * H, 5) - st[0][:, None, :]) * st[1][:, None, :]
    assert close(p.transpose(0, 2, 1), cache[0], CAST)


def test_spatial_softmax_rectangular_and_mask():
    """H != W against the definition written out position by position (float64, 1e-10), and the f > 0 mask of the backward."""
    rng = np.random.default_rng(5)
    H, W = 4, 6
    f = rng.standard_normal((2, H, W, 3)) * 2
    out, st = R.spatial_softmax_fwd(f)
    dout = rng.standard_normal((2, 6))
    df = R.spatial_softmax_bwd(f, st, dout)
    for n in range(2):
        for c in range(3):
            e = np.exp(f[n, :, :, c] - f[n, :, :, c].max())
            p = e / e.sum()
            ex = sum(p[h, w] * (-1 + 2 * h / (H - 1)) for h in range(H) for w in range(W))
            ey = sum(p[h, w] * (-1 + 2 * w / (W - 1)) for h in range(H) for w in range(W))
            assert abs(out[n, 2 * c] - ex) < 1e-10 and abs(out[n, 2 * c + 1] - ey) < 1e-10
            for h in range(H):
                for w in range(W):
                    g = p[h, w] * (dout[n, 2 * c] * (-1 + 2 * h / (H - 1) - ex) + dout[n, 2 * c + 1] * (-1 + 2 * w / (W - 1) - ey))
                    assert abs(df[n, h, w, c] - (g if f[n, h, w, c] > 0 else 0.0)) < 1e-10
    assert (df[f <= 0] == 0).all() and (f <= 0).any()
    # the backward is the derivative of the forward where the mask is open: central differences on one map
    fp = np.abs(f) + 0.1
    _, st = R.spatial_softmax_fwd(fp)
    df = R.spatial_softmax_bwd(fp, st, dout)
    eps = 1e-6
    for (h, w) in ((0, 0), (2, 5), (3, 1)):
        d = np.zeros_like(fp)
        d[1, h, w, 2] = eps
        num = ((R.spatial_softmax_fwd(fp + d)[0] - R.spatial_softmax_fwd(fp - d)[0]) * dout).sum() / (2 * eps)
        assert abs(num - df[1, h, w, 2]) < 1e-8


def test_tail_equals_oracle_linear_and_layer_norm():
    """CAST bound: linear, layer_norm and layer_norm_bwd return float32."""
    rng = np.random.default_rng(1)
    n = 9
    x = rng.standard_normal((n, 128))
    W1, b1 = rng.standard_normal((512, 128)) * 0.09, rng.standard_normal(512) * 0.1
    W2, b2 = rng.standard_normal((64, 512)) * 0.05, rng.standard_normal(64) * 0.1
    g, b = 1 + 0.1 * rng.standard_normal(64), 0.1 * rng.standard_normal(64)
    f1 = R.tail_fc1(x, W1, b1)
    assert close(f1, O.relu(O.linear(x, W1, b1)), CAST)
    f2 = R.tail_fc2(f1, W2, b2)
    assert close(f2, O.linear(f1, W2, b2), CAST)
    emb, mean, rstd = R.tail_ln(f2, g, b)
    o_emb, cache = O.layer_norm(f2, g, b)
    assert close(emb, o_emb, CAST)
    assert close(rstd, cache[1][:, 0], CAST) and close((f2 - mean[:, None]) * rstd[:, None], cache[0], CAST)
    demb = rng.standard_normal((n, 64))
    d_f2, dg, db = R.tail_ln_bwd(demb, f2, mean, rstd, g)
    o_d, o_dg, o_db = O.layer_norm_bwd(demb, g, cache)
    assert close(d_f2, o_d, 4 * CAST) and close(dg, o_dg, 4 * CAST) and close(db, o_db, CAST)          # the cache (xh, rstd) is float32
    xm = rng.standard_normal((n, 128))
    d_f1 = R.tail_fc2_bwd(d_f2, W2, f1)
    assert close(d_f1, O.linear_bwd(f1, W2, d_f2)[0] * (f1 > 0), CAST)
    assert (d_f1[f1 <= 0] == 0).all() and (f1 <= 0).any()
    assert close(R.tail_fc1_bwd(d_f1, W1), O.linear_bwd(x, W1, d_f1)[0], CAST)
    assert close(R.tail_fc1_bwd(d_f1, W1, xm), O.linear_bwd(x, W1, d_f1)[0] * (xm > 0), CAST)


def test_layer_norm_statistics_float64():
    """1e-10: mean / rstd and the backward against numpy's own float64 moments and central differences (no float32 anywhere)."""
    rng = np.random.default_rng(2)
    f2 = rng.standard_normal((5, 64)) * 3 + 1
    g, b = 1 + 0.1 * rng.standard_normal(64), 0.1 * rng.standard_normal(64)
    emb, mean, rstd = R.tail_ln(f2, g, b)
    assert close(mean, f2.mean(1), 1e-10) and close(rstd, 1 / np.sqrt(f2.var(1) + 1e-5), 1e-10)
    demb = rng.standard_normal((5, 64))
    d, dg, db = R.tail_ln_bwd(demb, f2, mean, rstd, g)
    eps = 1e-6
    for (r, c) in ((0, 0), (3, 17), (4, 63)):
        e = np.zeros_like(f2)
        e[r, c] = eps
        num = ((R.tail_ln(f2 + e, g, b)[0] - R.tail_ln(f2 - e, g, b)[0]) * demb).sum() / (2 * eps)
        assert abs(num - d[r, c]) < 1e-8
    assert close(dg, (demb * (emb - b) / g).sum(0), 1e-10) and close(db, demb.sum(0), 1e-10)


def test_tail_x0_dropout():
    rng = np.random.default_rng(3)
    emb, pos = rng.standard_normal((10, 128)), rng.standard_normal((5, 128))
    keep = O.engine_keep_mask(1234, (10, 128), 0.1)
    x0 = R.tail_x0(emb, pos, 5, keep, 0.1)
    assert 0.02 < 1 - keep.mean() < 0.25
    assert (x0[~keep] == 0).all()
    assert close(x0[keep], ((emb + np.tile(pos, (2, 1))) / 0.9)[keep], 1e-10)
    assert close(R.tail_x0(emb, pos, 5, keep, 0.0), emb + np.tile(pos, (2, 1)), 1e-10)


def loss_inputs(rng, B, S, D=6, K=10):
    """float64 heads and float32-representable actions that reach every branch of the loss (the oracle casts the actions to float32)."""
    logits = rng.standard_normal((B, S, D, K))
    means = rng.uniform(-1, 1, (B, S, D, K))
    lsr = rng.uniform(-9, 0, (B, S, D, K))
    grip = rng.standard_normal((B, S, 2))
    a = rng.uniform(-0.95, 0.95, (B, S, 7))
    edge = rng.integers(0, 4, (B, S, 6))
    a[..., :6] = np.where(edge == 0, -1.0, np.where(edge == 1, 1.0, a[..., :6]))
    a[..., 6] = rng.choice([-1.0, 1.0], (B, S))
    return logits, means, lsr, grip, a.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("discrete", [1, 0])
def test_logistic_rows_equal_oracle(discrete):
    """CAST bound: the oracle casts the loss and every gradient to float32; its half-bin constant is float32 (passed to the reference here so that both evaluate
    the same function)."""
    rng = np.random.default_rng(7)
    B, S = 3, 5
    logits, means, lsr, grip, a = loss_inputs(rng, B, S)
    if not discrete:
        grip = None
    r = R.logistic_mixture_rows(logits, means, lsr, grip, a, hb=float(np.float32((2.0 / 2.0) / 9)))
    for c in range(4):
        assert (r["case"] == c).mean() > 0.05
    assert (lsr < -7).mean() > 0.05
    with np.errstate(over="ignore"):          # the oracle's sigmoid is 1 / (1 + exp(-x)): exp overflows to inf at sharp components, the quotient is still right
        loss, (dlogit, dls, dmean, dgl) = O.logistic_loss(logits, lsr, means, grip, a)
    tot = r["loss"].sum() / (B * S) + (r["gloss"].sum() / (B * S) if discrete else 0.0)
    assert abs(tot - float(loss)) <= CAST * abs(tot)
    n = B * S
    assert close(r["dlogits"] / n, dlogit, CAST) and close(r["dmeans"] / n, dmean, CAST) and close(r["dlsr"] / n, dls, CAST)
    assert (r["dlsr"][lsr < -7] == 0).all()
    if discrete:
        assert close(r["dgrip"] / n, dgl, CAST)


def test_logistic_rows_gradient_is_the_derivative():
    """float64, central differences: each row's gradient is the derivative of that row's loss (away from the branch thresholds)."""
    rng = np.random.default_rng(8)
    logits, means, lsr, grip, a = loss_inputs(rng, 2, 3)
    lsr = np.where(np.abs(lsr + 7) < 1e-3, -6.5, lsr)
    r = R.logistic_mixture_rows(logits, means, lsr, grip, a)
    eps = 1e-6
    for name, arr in (("dlogits", logits), ("dmeans", means), ("dlsr", lsr)):
        for idx in ((0, 0, 0, 0), (1, 2, 5, 9), (0, 1, 3, 4), (1, 0, 2, 7)):
            args = dict(logits=logits, means=means, lsr=lsr)
            key = {"dlogits": "logits", "dmeans": "means", "dlsr": "lsr"}[name]
            e = np.zeros_like(arr)
            e[idx] = eps
            hi = R.logistic_mixture_rows(**{**args, key: arr + e}, grip=grip, a_tcp=a)
            lo = R.logistic_mixture_rows(**{**args, key: arr - e}, grip=grip, a_tcp=a)
            if (hi["case"] != lo["case"]).any() or abs(lsr[idx] + 7) < 1e-3:
                continue
            num = (hi["loss"][idx[:3]] - lo["loss"][idx[:3]]) / (2 * eps)
            assert abs(num - r[name][idx]) <= 1e-6 * max(1.0, abs(num)), (name, idx, num, r[name][idx])


def test_world_to_tcp_equals_oracle():
    """The oracle's transform is float32 throughout: agreement at the project's 3e-4 (tests of a_tcp), measured far below it."""
    rng = np.random.default_rng(9)
    a = rng.uniform(-1, 1, (4, 6, 7)).astype(np.float32)
    ro = rng.uniform(-1.5, 1.5, (4, 6, 15)).astype(np.float32)
    got = R.world_to_tcp(a.astype(np.float64), ro.astype(np.float64))
    ref = O.world_to_tcp_frame(a, ro)
    assert np.abs(got - ref).max() < 3e-4


def recorded(value, measured):
    """a recorded float32-vs-float64 figure is the measured one, rounded up by at most a tenth"""
    return measured <= value * (1 + 1e-6) and value <= 1.1 * measured


def test_softmax_stat_gates_are_five_times_the_float32_error():
    """The gates of the fp32 softmax statistics (GPU tests), shape by shape: 5 x what enc_head_ref.spatial_softmax_fwd loses in numpy float32 against float64 on
    that shape's own inputs, both storage types."""
    assert set(I.SS_F32) == set(I.SS_SHAPES)
    for (H, W) in I.SS_SHAPES:
        worst_c, worst_i = I.ss_measure(H, W)
        print(f"{H}x{W} float32 vs float64: coordinates {worst_c:.4g} absolute, 1/sum {worst_i:.4g} relative")
        assert recorded(I.SS_F32[H, W][0], worst_c) and recorded(I.SS_F32[H, W][1], worst_i), (H, W)
        assert I.SS_GATE[H, W] == (5 * I.SS_F32[H, W][0], 5 * I.SS_F32[H, W][1])


def test_logistic_gates_are_four_times_the_float32_error_and_branches_are_safe():
    """The gates of row_loss and of float dheads (GPU tests): 4 x what the reference formulas lose in numpy float32 against float64 on the GPU tests' own inputs.
    Also checked here, before any GPU run: every branch of the loss is taken by at least 5 % of the components of every input set, no component's delta lies in
    [5e-6, 2e-5] and no action within 1e-4 of a bound's threshold, so float32 and float64 take the same branch everywhere; some log-scales are clamped."""
    worst = dict.fromkeys(I.LL_F32, 0.0)
    for (B, S) in I.LL_SHAPES:
        for gc in (0, 1):
            inp = I.ll_inputs(B, S, gc)
            a64, ro64 = inp["actions"].astype(np.float64), inp["robot_obs"].astype(np.float64)
            at = R.world_to_tcp(a64, ro64) if gc else a64
            assert (inp["lsr"] < I.LSMIN).mean() > 0.05 and {-1.0, 1.0} <= set(inp["actions"][..., :6].ravel().tolist())
            assert set(inp["actions"][..., 6].ravel().tolist()) == ({-1.0, 1.0} if B * S > 1 else {-1.0})
            for disc in (1, 0):
                ref = I.ll_reference(inp, at, disc)
                I.ll_check_branches(ref, at)
                for k, v in I.ll_measure(inp, at, disc).items():
                    worst[k] = max(worst[k], v)
    print({k: f"{v:.4g}" for k, v in worst.items()})
    for k, v in worst.items():
        assert recorded(I.LL_F32[k], v), (k, v, I.LL_F32[k])
        assert I.LL_GATE[k] == 4 * I.LL_F32[k]
