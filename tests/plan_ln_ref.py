"""Plain numpy references of the latent-plan operations (categorical plan: KL balancing, Gumbel-max sample, straight-through backward, one-hot gather and
scatter; continuous mcil plan: Normal KL and the reparametrised sample) and of LayerNorm (forward, backward, parameter gradients, mean over S), written from
their definitions.  Everything runs in the dtype it is given (float64 for the reference, float32 to measure what fp32 arithmetic alone costs); pinned by
tests/test_plan_ln_ref_host.py to central differences and to oracle/hulc_oracle.py."""
import numpy as np


def _exp(x):
    """exp in x's dtype, correctly rounded (through float64): the float32 measurements then do not depend on the host's vector math library"""
    return np.exp(np.asarray(x, np.float64)).astype(x.dtype)


def _log(x):
    return np.log(np.asarray(x, np.float64)).astype(x.dtype)


# ---------------------------------------------------------------------------------------------------- categorical plan
def log_softmax(x):
    z = x - x.max(-1, keepdims=True)
    return z - _log(_exp(z).sum(-1, keepdims=True))


def softmax(x):
    e = _exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def kl_categorical(pr, pp):
    """KL(softmax(pr) || softmax(pp)) over the last axis"""
    a, b = log_softmax(pr), log_softmax(pp)
    return (_exp(a) * (a - b)).sum(-1)


def plan_kl(pr, pp, w_pp, w_pr):
    """probs = softmax(pr), kl_cat, and the gradients of sum(kl_cat) with respect to pp (times w_pp) and pr (times w_pr): the two halves of the balanced KL,
    each with the other side held constant"""
    a, b = log_softmax(pr), log_softmax(pp)
    p, q = _exp(a), _exp(b)
    klc = (p * (a - b)).sum(-1)
    dt = pr.dtype.type
    return p, klc, dt(w_pp) * (q - p), dt(w_pr) * p * ((a - b) - klc[..., None])


def st_softmax_bwd(probs, dplan, dpr_kl):
    """gradient of the straight-through sample (one_hot + probs - stop_gradient(probs)) with respect to the logits: the softmax Jacobian applied to dplan, plus
    the KL's share"""
    return probs * (dplan - (probs * dplan).sum(-1, keepdims=True)) + dpr_kl


def one_hot(idx, ncls, dt=np.float64):
    """idx (B, NCAT) -> (B, NCAT * NCLS)"""
    B, ncat = idx.shape
    oh = np.zeros((B, ncat, ncls), dt)
    np.put_along_axis(oh, idx[..., None].astype(np.int64), 1, -1)
    return oh.reshape(B, ncat * ncls)


def plan_gather(w_t, idx, ncls, b1, b2):
    """Cplan (B, H) = one_hot(idx) @ w_t[:NCAT * NCLS] + b1 + b2, w_t (KIN, H)"""
    ncat = idx.shape[1]
    s = (b1 + b2)[None, :] + np.zeros((idx.shape[0], 1), w_t.dtype)
    return s + one_hot(idx, ncls, w_t.dtype) @ w_t[:ncat * ncls] if ncat else s


def plan_scatter(dC, idx, ncls):
    """(H, NCAT * NCLS) = (one_hot(idx).T @ dC).T"""
    return (one_hot(idx, ncls, dC.dtype).T @ dC).T


# ---------------------------------------------------------------------------------------------------- continuous plan (mcil)
def softplus(x):
    """log(1 + exp(x)) = max(x, 0) + log1p(exp(-|x|))"""
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(np.asarray(x, np.float64)))).astype(x.dtype)


def sigmoid(x):
    return 1 / (1 + _exp(-x))


def normal_std(v):
    return softplus(v) + v.dtype.type(1e-4)


def kl_normal(pr, pp):
    """per element KL(N(m1, s1) || N(m2, s2)); state = [mean | var] over the last axis, std = softplus(var) + 1e-4"""
    n = pr.shape[-1] // 2
    m1, s1, m2, s2 = pr[..., :n], normal_std(pr[..., n:]), pp[..., :n], normal_std(pp[..., n:])
    return _log(s2 / s1) + (s1 * s1 + (m1 - m2) ** 2) / (2 * s2 * s2) - pr.dtype.type(0.5)


def kl_normal_grads(pr, pp, w_pp, w_pr):
    """gradients of sum(kl_normal) with respect to the states pp (times w_pp) and pr (times w_pr), chain rule through std = softplus(var) + 1e-4"""
    n = pr.shape[-1] // 2
    dt = pr.dtype.type
    m1, v1, m2, v2 = pr[..., :n], pr[..., n:], pp[..., :n], pp[..., n:]
    s1, s2 = normal_std(v1), normal_std(v2)
    dm = m1 - m2
    d_m2, d_s2 = -dm / s2 ** 2, 1 / s2 - (s1 ** 2 + dm ** 2) / s2 ** 3
    d_m1, d_s1 = dm / s2 ** 2, -1 / s1 + s1 / s2 ** 2
    return dt(w_pp) * np.concatenate([d_m2, d_s2 * sigmoid(v2)], -1), dt(w_pr) * np.concatenate([d_m1, d_s1 * sigmoid(v1)], -1)


def rsample(pr, eps):
    n = pr.shape[-1] // 2
    return pr[..., :n] + normal_std(pr[..., n:]) * eps


def rsample_bwd(dplan, eps, pr, dpr_kl):
    """gradient of plan = mean + std * eps with respect to the state, plus the KL's share"""
    n = pr.shape[-1] // 2
    return np.concatenate([dplan, dplan * eps * sigmoid(pr[..., n:])], -1) + dpr_kl


# ---------------------------------------------------------------------------------------------------- LayerNorm over the last axis
def ln_fwd(x, g, b, eps=1e-5):
    """-> y, mean, rstd (biased variance)"""
    mean = x.mean(-1)
    d = x - mean[..., None]
    rstd = 1 / np.sqrt((d * d).mean(-1) + x.dtype.type(eps))
    return d * rstd[..., None] * g + b, mean, rstd


def ln_bwd(dy, x, mean, rstd, g):
    """-> dx, and the ADDENDS (rows, n) of dg and db (their column sums are the parameter gradients)"""
    xh = (x - mean[..., None]) * rstd[..., None]
    q = dy * g
    dx = rstd[..., None] * (q - q.mean(-1, keepdims=True) - xh * (q * xh).mean(-1, keepdims=True))
    return dx, dy * xh, dy


def ln_mean(x, g, b):
    """x (B, S, n) -> mean over S of LayerNorm(x), y, mean, rstd"""
    y, mean, rstd = ln_fwd(x, g, b)
    return y.mean(1), y, mean, rstd
