"""Host: tests/plan_ln_ref.py (the float64 references the GPU tests of the latent-plan kernels and of the LayerNorm family compare against) pinned to
float64 central differences of the functions they are gradients of (1e-10), to definitions written out element by element (1e-10), and to
oracle/hulc_oracle.py where it has the same operation (CAST = 2e-7 of the tensor's largest magnitude: the oracle casts what it returns to float32).

The last tests re-measure, on the host, every measured gate of the GPU tests (tests/plan_ln_inputs.py) and check the conditions those tests rest on (the
undecided share of the sampled rows, the margin between one window and the scatter's gate), so that none of them rests on a kernel's output."""
import types

import numpy as np
import pytest

import hulc_oracle as O
import plan_ln_inputs as I
import plan_ln_ref as R

CAST = 2e-7
FD = 1e-10


def close(got, ref, tol):
    ref = np.asarray(ref, np.float64)
    return np.abs(np.asarray(got, np.float64) - ref).max() <= tol * max(np.abs(ref).max(), 1e-300)


def grad_fd(f, x, h=1e-3):
    """fourth-order central difference of the scalar f at x, element by element (truncation h^4, round-off 1e-16 / h)"""
    g = np.zeros_like(x)
    for k in np.ndindex(*x.shape):
        def at(d):
            y = x.copy()
            y[k] += d
            return f(y)
        g[k] = (8 * (at(h) - at(-h)) - (at(2 * h) - at(-2 * h))) / (12 * h)
    return g


def rng_normal(tag, shape, scale=1.0):
    return I.prng.normal(tag, shape, seed=5).astype(np.float64) * scale


# ---------------------------------------------------------------------------------------------------- categorical plan
def test_softmax_and_kl_follow_their_definitions():
    x, z = rng_normal("hx", (2, 3, 5), 2.0), rng_normal("hz", (2, 3, 5), 2.0)
    for b in range(2):
        for c in range(3):
            e = [np.exp(v) for v in x[b, c]]
            p = [v / sum(e) for v in e]
            q = [np.exp(v) / sum(np.exp(z[b, c])) for v in z[b, c]]
            assert np.abs(R.softmax(x)[b, c] - p).max() < FD and np.abs(R.log_softmax(x)[b, c] - np.log(p)).max() < FD
            assert abs(R.kl_categorical(x, z)[b, c] - sum(pi * np.log(pi / qi) for pi, qi in zip(p, q))) < FD
    assert close(R.softmax(x), O.softmax(x), 1e-14) and close(R.log_softmax(x), O.log_softmax(x), 1e-14)


def test_plan_kl_gradients_against_central_differences_and_the_oracle():
    pr, pp = rng_normal("kpr", (2, 3, 5), 2.0), rng_normal("kpp", (2, 3, 5), 2.0)
    w_pp, w_pr = 0.37, 0.21
    p, klc, dpp, dpr = R.plan_kl(pr, pp, w_pp, w_pr)
    assert close(p, R.softmax(pr), 1e-14) and close(klc, R.kl_categorical(pr, pp), 1e-14)
    assert close(dpp, grad_fd(lambda y: w_pp * R.kl_categorical(pr, y).sum(), pp), FD)
    assert close(dpr, grad_fd(lambda y: w_pr * R.kl_categorical(y, pp).sum(), pr), FD)
    dims = types.SimpleNamespace(n_cat=3, n_cls=5)
    beta, alpha = 0.01, 0.8
    _, o_dpp, o_dpr = O.kl_loss(pp.reshape(2, -1), pr.reshape(2, -1), dims, beta, alpha)
    _, _, dpp2, dpr2 = R.plan_kl(pr, pp, beta * alpha / 2, beta * (1 - alpha) / 2)
    assert close(dpp2.reshape(2, -1), o_dpp, CAST) and close(dpr2.reshape(2, -1), o_dpr, CAST)


def test_straight_through_backward_against_central_differences():
    x, d, k = rng_normal("sx", (4, 7), 2.0), rng_normal("sd", (4, 7)), rng_normal("sk", (4, 7), 0.1)
    got = R.st_softmax_bwd(R.softmax(x), d, k)
    assert close(got, grad_fd(lambda y: (R.softmax(y) * d).sum() + (y * k).sum(), x), FD)


def test_gather_and_scatter_are_one_hot_products():
    B, ncat, ncls, H = 5, 3, 4, 6
    idx = I.plan_indices(B, ncat, ncls, 0, "h")
    w, b1, b2, dC = rng_normal("gw", (ncat * ncls + 2, H)), rng_normal("g1", (H,)), rng_normal("g2", (H,)), rng_normal("gc", (B, H))
    oh = R.one_hot(idx, ncls)
    assert oh.shape == (B, ncat * ncls) and (oh.sum(1) == ncat).all()
    out, sc = R.plan_gather(w, idx, ncls, b1, b2), R.plan_scatter(dC, idx, ncls)
    want_sc = np.zeros((H, ncat * ncls))
    for b in range(B):
        want = b1 + b2
        for c in range(ncat):
            assert oh[b, c * ncls + idx[b, c]] == 1
            want = want + w[c * ncls + idx[b, c]]
            want_sc[:, c * ncls + idx[b, c]] += dC[b]
        assert np.abs(out[b] - want).max() < FD
    assert np.abs(sc - want_sc).max() < FD
    assert np.abs(R.plan_gather(w, idx[:, :0], ncls, b1, b2) - (b1 + b2)).max() == 0          # no plan (gcbc): the biases alone
    # the scatter is the gradient of the gather with respect to the plan rows of w
    assert close(sc.T, grad_fd(lambda y: (R.plan_gather(y, idx, ncls, b1, b2) * dC).sum(), w)[:ncat * ncls], FD)
    dims = types.SimpleNamespace(n_cat=ncat, n_cls=ncls)
    assert close(oh, np.asarray(O.onehot_plan(idx, dims)).reshape(B, -1), 1e-14)


# ---------------------------------------------------------------------------------------------------- continuous plan
def nk_states():
    n = 6
    v = np.array([-25.0, -5.0, 0.0, 5.0, 25.0, 1.0])
    pr = np.concatenate([rng_normal("nm1", (3, n)), v[None, :] + rng_normal("nv1", (3, n), 0.3)], -1)
    pp = np.concatenate([rng_normal("nm2", (3, n)), v[::-1][None, :] + rng_normal("nv2", (3, n), 0.3)], -1)
    return pr, pp


def test_normal_kl_follows_its_definition_and_the_oracle():
    pr, pp = nk_states()
    n = pr.shape[1] // 2
    kl = R.kl_normal(pr, pp)
    for b in range(3):
        for j in range(n):
            s1, s2 = np.log1p(np.exp(pr[b, n + j])) + 1e-4, np.log1p(np.exp(pp[b, n + j])) + 1e-4
            want = np.log(s2 / s1) + (s1 ** 2 + (pr[b, j] - pp[b, j]) ** 2) / (2 * s2 ** 2) - 0.5
            assert abs(kl[b, j] - want) <= FD * max(1.0, abs(want))
    beta, alpha = 0.01, 0.8
    # the oracle's std is float32: moderate var only (at var = -25 a float32 std of 1e-4 carries a relative error of 6e-8 into terms of 1e8)
    prm, ppm = pr.copy(), pp.copy()
    prm[:, n:], ppm[:, n:] = np.clip(pr[:, n:], -5, 5), np.clip(pp[:, n:], -5, 5)
    _, o_dpp, o_dpr = O.kl_normal_balanced(ppm, prm, beta, alpha)
    dpp, dpr = R.kl_normal_grads(prm, ppm, beta * alpha / 3, beta * (1 - alpha) / 3)
    assert close(dpp, o_dpp, 8 * CAST) and close(dpr, o_dpr, 8 * CAST)          # products and quotients of up to four float32-cast values


def test_normal_kl_and_rsample_gradients_against_central_differences():
    pr, pp = nk_states()
    n = pr.shape[1] // 2
    w_pp, w_pr = 0.37, 0.21
    dpp, dpr = R.kl_normal_grads(pr, pp, w_pp, w_pr)
    # moderate states: central differences of the summed KL with respect to the states themselves
    mod = (np.abs(pr[:, n:]) < 10) & (np.abs(pp[:, n:]) < 10)
    sel = np.concatenate([mod, mod], -1)
    prm, ppm = np.where(sel, pr, 0.5), np.where(sel, pp, -0.5)
    dppm, dprm = R.kl_normal_grads(prm, ppm, w_pp, w_pr)
    assert close(dppm, grad_fd(lambda y: w_pp * R.kl_normal(prm, y).sum(), ppm), FD) and close(dprm, grad_fd(lambda y: w_pr * R.kl_normal(y, ppm).sum(), prm), FD)
    assert mod.any() and (np.abs(dpp - dppm)[sel] <= 1e-12 * np.abs(dppm)[sel]).all() and (np.abs(dpr - dprm)[sel] <= 1e-12 * np.abs(dprm)[sel]).all()
    # every state, var = +-25 included (std from 1e-4 to 25, terms from 1e-11 to 1e9): element by element, central differences of the element's own KL term in
    # (mean, std) with a relative step, times d std / d var = sigmoid(var) (the chain rule's other factor, pinned by its definition) -- relative 1e-9
    def kl_term(m1, s1, m2, s2):
        return np.log(s2 / s1) + (s1 ** 2 + (m1 - m2) ** 2) / (2 * s2 ** 2) - 0.5

    def fd1(f, x):
        h = 1e-3 * max(abs(x), 1e-4)
        return (8 * (f(x + h) - f(x - h)) - (f(x + 2 * h) - f(x - 2 * h))) / (12 * h)
    for bb in range(3):
        for j in range(n):
            m1, v1, m2, v2 = pr[bb, j], pr[bb, n + j], pp[bb, j], pp[bb, n + j]
            s1, s2 = np.log1p(np.exp(v1)) + 1e-4, np.log1p(np.exp(v2)) + 1e-4
            sg1, sg2 = 1 / (1 + np.exp(-v1)), 1 / (1 + np.exp(-v2))
            want = ((dpr[bb, j], w_pr * fd1(lambda t: kl_term(t, s1, m2, s2), m1)), (dpr[bb, n + j], w_pr * sg1 * fd1(lambda t: kl_term(m1, t, m2, s2), s1)),
                    (dpp[bb, j], w_pp * fd1(lambda t: kl_term(m1, s1, t, s2), m2)), (dpp[bb, n + j], w_pp * sg2 * fd1(lambda t: kl_term(m1, s1, m2, t), s2)))
            for got, num in want:
                assert abs(got - num) <= 1e-9 * abs(num) + 1e-9 * abs(kl_term(m1, s1, m2, s2)) * w_pr * 1e-3, (bb, j, got, num)
    eps, dplan, dkl = rng_normal("ne", (3, n)), rng_normal("nd", (3, n)), rng_normal("nk", (3, 2 * n), 0.1)
    got = R.rsample_bwd(dplan, eps, pr, dkl)
    assert close(got, grad_fd(lambda y: (R.rsample(y, eps) * dplan).sum() + (y * dkl).sum(), pr), FD)


# ---------------------------------------------------------------------------------------------------- LayerNorm
def test_layernorm_follows_its_definition_the_oracle_and_central_differences():
    rows, n = 5, 7
    x, g, b, dy = rng_normal("lx", (rows, n), 1.5) + 0.7, 1 + rng_normal("lg", (n,), 0.2), rng_normal("lb", (n,), 0.2), rng_normal("ld", (rows, n))
    y, mean, rstd = R.ln_fwd(x, g, b)
    for r in range(rows):
        m = sum(x[r]) / n
        v = sum((t - m) ** 2 for t in x[r]) / n
        assert abs(mean[r] - m) < FD and abs(rstd[r] - 1 / np.sqrt(v + 1e-5)) < FD
        assert np.abs(y[r] - ((x[r] - m) / np.sqrt(v + 1e-5) * g + b)).max() < FD
    o_y, cache = O.layer_norm(x, g, b)
    assert close(y, o_y, CAST)
    dx, ag, ab = R.ln_bwd(dy, x, mean, rstd, g)
    o_dx, o_dg, o_db = O.layer_norm_bwd(dy, g, cache)
    assert close(dx, o_dx, 4 * CAST) and close(ag.sum(0), o_dg, 4 * CAST) and close(ab.sum(0), o_db, CAST)          # xh and rstd float32 in the oracle's cache
    loss = lambda xx, gg, bb: (R.ln_fwd(xx, gg, bb)[0] * dy).sum()
    assert close(dx, grad_fd(lambda t: loss(t, g, b), x), FD)
    assert close(ag.sum(0), grad_fd(lambda t: loss(x, t, b), g), FD) and close(ab.sum(0), grad_fd(lambda t: loss(x, g, t), b), FD)
    x3 = rng_normal("l3", (2, 4, n), 1.5)
    m3, y3, _, _ = R.ln_mean(x3, g, b)
    assert close(y3, R.ln_fwd(x3.reshape(8, n), g, b)[0].reshape(2, 4, n), 1e-14) and close(m3, sum(y3[:, t] for t in range(4)) / 4, 1e-14)


# ---------------------------------------------------------------------------------------------------- the GPU tests' gates and conditions
def recorded(value, measured):
    """a recorded float32-vs-float64 figure is the measured one, rounded up by at most a tenth"""
    return measured <= value * (1 + 1e-6) and value <= 1.1 * measured


def test_plan_kl_gates_are_five_times_the_float32_error():
    assert set(I.KL_F32) == set(I.KL_CASES)
    for case in I.KL_CASES:
        m = I.kl_measure(*case)
        print(case, " ".join(f"{v:.4g}" for v in m))
        assert all(recorded(v, x) for v, x in zip(I.KL_F32[case], m)), (case, m, I.KL_F32[case])
        assert I.KL_GATE[case] == tuple(5 * v for v in I.KL_F32[case])


def test_normal_kl_gates_are_five_times_the_float32_error():
    assert set(I.NK_F32) == set(I.NK_CASES) == set(I.NKB_F32)
    for case in I.NK_CASES:
        m = I.nk_measure(*case)
        print(case, " ".join(f"{v:.4g}" for v in m))
        assert all(recorded(v, x) for v, x in zip(I.NK_F32[case], m)), (case, m, I.NK_F32[case])
        assert I.NK_GATE[case] == tuple(5 * v for v in I.NK_F32[case])
        mb = I.nkb_measure(*case)
        print(case, f"rsample_bwd {mb:.4g}")
        assert recorded(I.NKB_F32[case], mb) and I.NKB_GATE[case] == 5 * I.NKB_F32[case], (case, mb, I.NKB_F32[case])
        pr, pp, _ = I.nk_inputs(*case)
        n = case[1]
        if n >= 5:
            assert (pr[:, n:] > 20).any() and (pr[:, n:] < -20).any() and (np.abs(pr[:, n:]) < 20).any(), "var crosses both branches of the device's softplus"


def test_layernorm_cancellation_gates_are_five_times_the_float32_error():
    for n, v in I.LN_CANCEL_F32.items():
        m = max(I.ln_cancel_measure(rows, n) for rows in I.LN_CANCEL_ROWS)
        print(n, f"{m:.4g}")
        assert recorded(v, m) and I.LN_CANCEL_GATE[n] == 5 * v, (n, m, v)
    x, _, _ = I.ln_inputs(5, 64)
    assert np.ptp(x[I.LN_ROW_CONST]) == 0 and abs(x[I.LN_ROW_CANCEL].mean() - 1e3) < 0.1
    for rows in (5, 1027):
        for n in (32, 64, 100, 128):
            x = I.ln_inputs(rows, n)[0].astype(np.float64)
            assert np.abs(x.mean(-1)).min() > 0.3, "the relative gate on the mean needs means away from zero"


def test_sample_seeds_leave_at_most_one_per_cent_of_the_rows_undecided():
    for seed in I.KL_SEEDS:
        for case in I.KL_CASES:
            idx, decided = I.gumbel_draw(I.kl_inputs(*case)[0], seed)
            assert (~decided).mean() <= 0.01, (seed, case, int((~decided).sum()))
            assert idx[0, 0] == I.KL_SPIKE % case[2]
    # the uniforms are engine_keep_mask's: u >= p there
    u = I.hash_uniform(123, 1000, first=7)
    assert ((u >= 0.3) == O.engine_keep_mask(123, (1000,), 0.3, first=7)).all() and (u > 0).all() and (u < 1).all()


def test_one_scatter_window_stands_a_hundred_gates_high():
    for B in (1, 129):
        for dtype in ("bf16", "fp16", "fp32"):
            dC = I.scatter_inputs(B, 320, dtype)
            for pattern in (0, 1, 2):
                idx = I.plan_indices(B, 5, 7, pattern)
                _, gate = I.scatter_reference(dC, idx, 7, np.ones((320, 35)))
                assert np.abs(dC).min() >= I.SC_DC_MIN >= 100 * gate.max()
    w = I.gather_weight(1024 + 3 + 32, 256, "bf16")
    assert all(len(np.unique(w[:, c])) == w.shape[0] for c in range(0, 256, 17)), "every row of a column is distinct"
