"""Plain numpy float64 restatement of the feed-forward decoder body (action_decoder.rnn_model = mlp_decoder; hulc/models/decoders/utils/rnn.py) and of the
logistic-mixture loss behind it (logistic_decoder_rnn.py:136-231), written from the reference's description:

    x[b,t] = [plan_b | emb[b,t,64:128] | goal_b];  a0 = relu(W0 x + b0);  a1 = relu(W1 a0 + b1);  y = W2 a1 + b2 (no activation);  the four heads read y.

`body_fwd` / `body_bwd` are the whole body, `stage_*` one product each with the per-element bound tests/gemm_epi_ref.py derives for it (the GPU stage tests
apply them to each stage's own device inputs).  Pinned against the unmodified reference's recorded losses and float64 gradients by
tests/test_mlp_decoder_host.py."""
import numpy as np

import gemm_epi_ref as G
import plan_ln_inputs as PI

HEADS = ("prob_fc", "mean_fc", "log_scale_fc", "gripper_fc")
AD = "action_decoder."
TINY = {"bf16": 2.0 ** -133, "fp16": 2.0 ** -24}          # spacing of the type's subnormal numbers: one ulp is never less


def relu(x):
    return np.maximum(x, 0.0)


def decoder_input(plan_idx, emb, goal, n_cls=32):
    """(B,S,KIN) float64: the one-hot plan (hulc; plan_idx None for gcbc), the gripper half of the embedding, the goal"""
    B, S_, _ = emb.shape
    parts = []
    if plan_idx is not None:
        oh = np.zeros((B, plan_idx.shape[1], n_cls))
        np.put_along_axis(oh, plan_idx[..., None].astype(np.int64), 1.0, -1)
        parts.append(np.repeat(oh.reshape(B, 1, -1), S_, 1))
    parts += [emb[..., 64:128], np.repeat(goal[:, None, :], S_, 1)]
    return np.concatenate(parts, -1).astype(np.float64)


def body_fwd(x, W):
    """x [M][KIN], W = (W0, b0, W1, b1, W2, b2) -> a0, a1, y"""
    a0 = relu(x @ W[0].T + W[1])
    a1 = relu(a0 @ W[2].T + W[3])
    return a0, a1, a1 @ W[4].T + W[5]


def body_bwd(dy, x, a0, a1, W):
    """-> dict of the six parameter gradients (keys 0..5 as W), da1 / da0 (gradients of the pre-activations: the ReLU mask applied), dx"""
    g = {4: dy.T @ a1, 5: dy.sum(0)}
    da1 = np.where(a1 > 0, dy @ W[4], 0.0)
    g[2], g[3] = da1.T @ a0, da1.sum(0)
    da0 = np.where(a0 > 0, da1 @ W[2], 0.0)
    g[0], g[1] = da0.T @ x, da0.sum(0)
    return g, da1, da0, da0 @ W[0]


def log_softmax(x):
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def softplus(x):
    return np.logaddexp(0.0, x)


def sigmoid(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))


def mixture_loss(logit_probs, log_scales_raw, means, gripper_logits, a_tcp, num_classes=10, log_scale_min=-7.0, gripper_alpha=1.0):
    """logistic_decoder_rnn.py:136-152, :184-231 in float64: the loss (bounds +-1) and its gradients w.r.t. the four head outputs.
    logit_probs / log_scales_raw / means [n][6][10], gripper_logits [n][2], a_tcp [n][7]."""
    n, Dd, K = means.shape
    a = a_tcp[:, :Dd, None] * np.ones((1, 1, K))
    ls = np.maximum(log_scales_raw, log_scale_min)
    inv = np.exp(-ls)
    hb = 1.0 / (num_classes - 1)
    cen = a - means
    plus, minus, mid = inv * (cen + hb), inv * (cen - hb), inv * cen
    sp, sm = sigmoid(plus), sigmoid(minus)
    delta = sp - sm
    cA = a < -1.0 + 1e-3
    cB = (~cA) & (a > 1.0 - 1e-3)
    cC = (~cA) & (~cB) & (delta > 1e-5)
    cD = ~(cA | cB | cC)
    logp = np.where(cA, plus - softplus(plus), np.where(cB, -softplus(minus), np.where(cC, np.log(np.maximum(delta, 1e-12)),
                                                                                       mid - ls - 2.0 * softplus(mid) - np.log((num_classes - 1) / 2.0))))
    lsm = log_softmax(logit_probs)
    lp = logp + lsm
    m = lp.max(-1, keepdims=True)
    lse = m[..., 0] + np.log(np.exp(lp - m).sum(-1))
    g = a_tcp[:, -1]
    lab = np.where(g == -1, 0, g).astype(np.int64)
    glsm = log_softmax(gripper_logits)
    loss = -(lse.sum(-1)).mean() + gripper_alpha * (-np.take_along_axis(glsm, lab[:, None], -1)[:, 0].mean())
    wk = np.exp(lp - lse[..., None])
    dlogp = -wk / n
    dlogit = -(wk - np.exp(lsm)) / n
    safe = np.where(cC, delta, 1.0)
    g_plus = np.where(cA, sigmoid(-plus), np.where(cC, sp * (1 - sp) / safe, 0.0))
    g_minus = np.where(cB, -sm, np.where(cC, -sm * (1 - sm) / safe, 0.0))
    g_mid = np.where(cD, 1.0 - 2.0 * sigmoid(mid), 0.0)
    dmean = dlogp * (-inv) * (g_plus + g_minus + g_mid)
    dls = dlogp * (-(g_plus * plus + g_minus * minus + g_mid * mid) - np.where(cD, 1.0, 0.0))
    dls = np.where(log_scales_raw >= log_scale_min, dls, 0.0)
    dgl = np.exp(glsm)
    np.put_along_axis(dgl, lab[:, None], np.take_along_axis(dgl, lab[:, None], -1) - 1.0, -1)
    return loss, dict(prob_fc=dlogit.reshape(n, -1), mean_fc=dmean.reshape(n, -1), log_scale_fc=dls.reshape(n, -1), gripper_fc=gripper_alpha * dgl / n)


def decoder_loss(P, x, a_tcp, scale=1.0):
    """the whole decoder in float64 from its input x [M][KIN] (rows in any order) and the tcp-frame actions [M][7]:
    -> loss, {parameter name: gradient * scale}, dx"""
    P = {k: np.asarray(v, np.float64) for k, v in P.items() if k.startswith(AD)}
    W = tuple(P[f"{AD}rnn.{i}.{k}"] for i in (0, 2, 4) for k in ("weight", "bias"))
    a0, a1, y = body_fwd(x, W)
    n = x.shape[0]
    out = {h: y @ P[f"{AD}{h}.weight"].T + P[f"{AD}{h}.bias"] for h in HEADS}
    loss, d = mixture_loss(out["prob_fc"].reshape(n, 6, 10), out["log_scale_fc"].reshape(n, 6, 10), out["mean_fc"].reshape(n, 6, 10), out["gripper_fc"], a_tcp)
    grads, dy = {}, np.zeros_like(y)
    for h in HEADS:
        dh = d[h] * scale
        grads[f"{AD}{h}.weight"], grads[f"{AD}{h}.bias"] = dh.T @ y, dh.sum(0)
        dy += dh @ P[f"{AD}{h}.weight"]
    g, da1, da0, dx = body_bwd(dy, x, a0, a1, W)
    for j, (i, k) in enumerate((i, k) for i in (0, 2, 4) for k in ("weight", "bias")):
        grads[f"{AD}rnn.{i}.{k}"] = g[j]
    return loss, grads, dx


# ---------------------------------------------------------------------------------------------------- one product per stage, with its derived bound
def ulp16(ref, dtype):
    return np.maximum(PI.ULP[dtype] * np.abs(ref), TINY[dtype])


def stage_fwd(X, W, bias, dtype, act, res=None, res_rowmod=0):
    """out = act(X W^T + bias (+ res[row % res_rowmod])) stored in the 16-bit type: the fp64 value, the per-element bound (the product's fp32 accumulation
    bound + the epilogue's + one ulp of the storage type) and the bound on the PRE-activation (for the ReLU decisions)."""
    acc, pb = G.product(X, W)
    f = dict(bias=bias, relu=0)
    if res is not None:
        f.update(res=res, res_rowmod=res_rowmod)
    pre, _, eb, _ = G.epilogue(acc, f)
    ref = relu(pre) if act else pre
    return ref, pb + eb + ulp16(ref, dtype), pre, pb + eb


def stage_dgrad(dY, Wt, mask, dtype):
    """out = (dY W) where mask > 0 else 0, stored in the 16-bit type; Wt [K][N] = W^T as the engine's transposed copy holds it"""
    acc, pb = G.product(dY, Wt)
    ref, _, eb, _ = G.epilogue(acc, dict(mask=mask))
    pb = np.where(mask > 0, pb, 0.0)
    return ref, pb + eb + ulp16(ref, dtype)


def stage_wgrad(dY, X, nsplit):
    """dW = dY^T X in fp32 (stored into a zeroed gradient; split K over nsplit slabs adds one rounding per slab)"""
    return G.product(dY.T, X.T, nsplit)


def stage_bgrad(dY):
    """db = column sums of dY, fp32 adds in any order: (rows + 1) 2^-24 sum |dy|"""
    return dY.sum(0), (dY.shape[0] + 1) * G.EPS32 * np.abs(dY).sum(0)
