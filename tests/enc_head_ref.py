"""Plain numpy references of the operations behind the 16-bit encoder head and the action loss, stage by stage: the spatial softmax of the static camera
(csrc/kernels.h), the dense tail of both encoders (csrc/enc_tail.h) and the discretised logistic mixture loss (csrc/kernels.h).  Everything runs in the dtype
it is given (float64 for the reference; float32 to measure what fp32 arithmetic alone costs) and is pinned to oracle/hulc_oracle.py by
tests/test_enc_head_ref_host.py."""
import numpy as np


# ---------------------------------------------------------------------------------------------------- spatial softmax, maps (N, H, W, C)
def _coords(H, W, dt):
    lh = np.linspace(-1.0, 1.0, H).astype(dt)
    lw = np.linspace(-1.0, 1.0, W).astype(dt)
    return np.repeat(lh, W), np.tile(lw, H)          # position q = h * W + w


def spatial_softmax_fwd(f):
    """f (N, H, W, C) -> out (N, 2C) with out[:, 2c] = E[linspace(-1,1,H)[h]], out[:, 2c+1] = E[linspace(-1,1,W)[w]] under softmax over the H*W positions,
    and the statistics (max, 1/sum exp(f - max), ex, ey), each (N, C)."""
    n, H, W, C = f.shape
    dt = f.dtype
    v = f.reshape(n, H * W, C)
    lx, ly = _coords(H, W, dt)
    M = v.max(1)
    e = np.exp(v - M[:, None, :])
    inv = dt.type(1) / e.sum(1)
    ex = (e * lx[None, :, None]).sum(1) * inv
    ey = (e * ly[None, :, None]).sum(1) * inv
    out = np.stack([ex, ey], -1).reshape(n, 2 * C)
    return out, (M, inv, ex, ey)


def spatial_softmax_bwd(f, stats, dout):
    """df (N, H, W, C) = p * (dex * (lx - ex) + dey * (ly - ey)) where f > 0, else 0 (the ReLU in front of the softmax is folded into its backward)."""
    n, H, W, C = f.shape
    dt = f.dtype
    M, inv, ex, ey = stats
    v = f.reshape(n, H * W, C)
    lx, ly = _coords(H, W, dt)
    p = np.exp(v - M[:, None, :]) * inv[:, None, :]
    d = dout.reshape(n, C, 2)
    dex, dey = d[:, None, :, 0], d[:, None, :, 1]
    g = p * (dex * (lx[None, :, None] - ex[:, None, :]) + dey * (ly[None, :, None] - ey[:, None, :]))
    return np.where(v > 0, g, dt.type(0)).reshape(f.shape)


# ---------------------------------------------------------------------------------------------------- dense tail, one camera
def tail_fc1(x, W1, b1):
    return np.maximum(x @ W1.T + b1, 0)


def tail_fc2(f1, W2, b2):
    return f1 @ W2.T + b2


def tail_ln(f2, g, b, eps=1e-5):
    """LayerNorm over the last axis -> (y, mean, rstd)."""
    mean = f2.mean(-1)
    d = f2 - mean[:, None]
    rstd = 1.0 / np.sqrt((d * d).mean(-1) + eps)
    return d * rstd[:, None] * g + b, mean, rstd


def tail_x0(emb, pos, S, keep, p):
    """x0[row] = dropout(emb[row] + pos[row % S]) with the given keep mask (inverted dropout)."""
    t = np.arange(emb.shape[0]) % S
    v = emb + pos[t]
    return np.where(keep, v / (1.0 - p), 0.0) if p > 0 else v


def tail_ln_bwd(dy, f2, mean, rstd, g):
    """-> (d_f2, dgamma, dbeta); dgamma / dbeta summed over the rows."""
    xh = (f2 - mean[:, None]) * rstd[:, None]
    q = dy * g
    d = rstd[:, None] * (q - q.mean(-1, keepdims=True) - xh * (q * xh).mean(-1, keepdims=True))
    return d, (dy * xh).sum(0), dy.sum(0)


def tail_fc2_bwd(d_f2, W2, f1):
    return np.where(f1 > 0, d_f2 @ W2, 0.0)


def tail_fc1_bwd(d_f1, W1, xmask=None):
    dx = d_f1 @ W1
    return dx if xmask is None else np.where(xmask > 0, dx, 0.0)


# ---------------------------------------------------------------------------------------------------- action loss
def _euler_xyz(e):
    a, b, c = e[..., 0], e[..., 1], e[..., 2]
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    R = np.empty(e.shape[:-1] + (3, 3), e.dtype)
    R[..., 0, 0] = cb * cc
    R[..., 0, 1] = -cb * sc
    R[..., 0, 2] = sb
    R[..., 1, 0] = ca * sc + sa * sb * cc
    R[..., 1, 1] = ca * cc - sa * sb * sc
    R[..., 1, 2] = -sa * cb
    R[..., 2, 0] = sa * sc - ca * sb * cc
    R[..., 2, 1] = sa * cc + ca * sb * sc
    R[..., 2, 2] = ca * cb
    return R


def world_to_tcp(action, robot_obs):
    """relative world-frame action (.., 7) + robot_obs (.., 15) -> the action in the tcp frame (R = Rx Ry Rz of the tcp's euler angles; position R^T a,
    orientation = euler(Rn^T R) * 100 with Rn the orientation after the step)."""
    e = robot_obs[..., 3:6]
    R = _euler_xyz(e)
    pos = (np.swapaxes(R, -1, -2) @ action[..., :3, None])[..., 0]
    Rn = _euler_xyz(e + action[..., 3:6] * 0.01)
    M = np.swapaxes(Rn, -1, -2) @ R
    orn = np.stack([np.arctan2(-M[..., 1, 2], M[..., 2, 2]), np.arcsin(np.clip(M[..., 0, 2], -1, 1)), np.arctan2(-M[..., 0, 1], M[..., 0, 0])], -1)
    orn = np.where(orn < -np.pi, orn + 2 * np.pi, orn)
    orn = np.where(orn > np.pi, orn - 2 * np.pi, orn)
    return np.concatenate([pos, orn * 100, action[..., 6:]], -1)


def _softplus(x):
    return np.logaddexp(x.dtype.type(0), x)


def _sigmoid(x):
    return np.exp(-_softplus(-x))          # 1 / (1 + exp(-x)) without the overflow at large -x


def _lse(x):
    m = x.max(-1, keepdims=True)
    return m[..., 0] + np.log(np.exp(x - m).sum(-1))


def logistic_mixture_rows(logits, means, lsr, grip, a_tcp, num_classes=10, log_scale_min=-7.0, gripper_alpha=1.0, hb=None):
    """The discretised logistic mixture loss per row and per dimension, with the gradient of each ROW's loss (no 1 / rows factor).

    logits, means, lsr (.., D, K); grip (.., 2) or None; a_tcp (.., >= D [7 with grip]).  Runs in logits.dtype.  hb = half a bin, 1 / (num_classes - 1).
    Returns a dict: loss (.., D), dlogits, dmeans, dlsr (.., D, K), and with grip: gloss (..), dgrip (.., 2); `case` (.., D, K) in 0..3 (action at the lower
    bound | at the upper bound | delta > 1e-5 | mid-point fallback) and `delta`."""
    dt = logits.dtype.type
    D, K = means.shape[-2:]
    hb = dt(1) / dt(num_classes - 1) if hb is None else dt(hb)
    a = a_tcp[..., :D, None].astype(dt) + np.zeros(means.shape, dt)
    ls = np.maximum(lsr, dt(log_scale_min))
    inv = np.exp(-ls)
    cen = a - means
    plus, minus, mid = inv * (cen + hb), inv * (cen - hb), inv * cen
    sp, sm = _sigmoid(plus), _sigmoid(minus)
    delta = sp - sm
    case = np.where(a < dt(-1) + dt(1e-3), 0, np.where(a > dt(1) - dt(1e-3), 1, np.where(delta > dt(1e-5), 2, 3)))
    sd = np.where(case == 2, delta, dt(1))
    logp = np.select([case == 0, case == 1, case == 2],
                     [plus - _softplus(plus), -_softplus(minus), np.log(np.maximum(sd, dt(1e-12)))],
                     mid - ls - 2 * _softplus(mid) - np.log(dt((num_classes - 1) * 0.5)))
    gp = np.select([case == 0, case == 2], [_sigmoid(-plus), sp * (1 - sp) / sd], dt(0))
    gm = np.select([case == 1, case == 2], [-sm, -sm * (1 - sm) / sd], dt(0))
    gmid = np.where(case == 3, 1 - 2 * _sigmoid(mid), dt(0))
    dlogp_dmean = -inv * (gp + gm + gmid)
    dlogp_dls = np.where(lsr >= dt(log_scale_min), -(gp * plus + gm * minus + gmid * mid) - (case == 3), dt(0))
    lsm = logits - _lse(logits)[..., None]
    lp = logp + lsm
    lse = _lse(lp)
    w = np.exp(lp - lse[..., None])
    out = dict(loss=-lse, dlogits=-(w - np.exp(lsm)), dmeans=-w * dlogp_dmean, dlsr=-w * dlogp_dls, case=case, delta=delta)
    if grip is not None:
        g = a_tcp[..., 6]
        lab = np.where(g == -1, 0, g).astype(np.int64)
        glsm = grip - _lse(grip)[..., None]
        out["gloss"] = dt(gripper_alpha) * -np.take_along_axis(glsm, lab[..., None], -1)[..., 0]
        out["dgrip"] = dt(gripper_alpha) * (np.exp(glsm) - (np.arange(2) == lab[..., None]))
    return {k: (v.astype(dt) if v.dtype.kind == "f" else v) for k, v in out.items()}
