"""Plain numpy float64 references of the stages of the fused plan-recognition transformer layer kernels (hulc_amd/csrc/tr_fused.h): one function per saved
tensor, each computing it from the tensors in front of it, written from the layer's definition — nn.TransformerEncoderLayer(d_model 128, 8 heads, 2048 hidden
units, post-LN, relu):  x1 = LN1(x + drop_o(out_proj(attention(x W_qkv^T + b)))),  y2 = x1 + drop_y(linear2(drop_h(relu(linear1(x1))))),  with the bias of
linear2 INSIDE its dropout, as the model has it.  A dropout mask is a boolean keep array (None: no dropout) over the row-major index spaces (N, 128) (drop_o,
drop_y), (B, 8, S, S) (attention weights) and (N, 2048) (hidden); kept values are divided by 1 - p.

Functions that stand for a sum of products also return the rigorous fp32 accumulation bound of that sum per element, (K + 2 + extra) 2^-24 sum|terms|: K
additions, the bias / residual additions, and `extra` further fp32 roundings per term where the kernel has them (the 1 / (1 - p) factor, a product of two fp32
values, the four atomic partial sums).  Nothing here rounds to 16 bit unless the caller passes a rounding function: chain_fwd / chain_bwd run the stages end
to end, either exactly (tests/test_tr_fused_ref_host.py compares that with torch) or with the kernels' storage roundings (tests/tr_fused_inputs.py builds the
backward kernels' inputs that way).  Pinned by tests/test_tr_fused_ref_host.py."""
import numpy as np

import plan_ln_ref as R

EPS32 = 2.0 ** -24
D, NH, HD, FF, NQ = 128, 8, 16, 2048, 4
HQ = FF // NQ


def mult(p):
    """1 / (1 - p) with 1 - p taken in fp32 as on the device"""
    return 1.0 / np.float64(np.float32(1.0) - np.float32(p)) if p > 0 else 1.0


def _m(keep, p):
    """the multiplier array of a keep mask (1.0: no dropout)"""
    return 1.0 if keep is None else np.where(keep, mult(p), 0.0)


def acc_bound(abs_terms, K, extra=0):
    return (K + 2 + extra) * EPS32 * abs_terms


def ident(x):
    return x


# ---------------------------------------------------------------------------------------------------- forward
def ln(x, g, b):
    """-> y, stats (rows, 2) = mean, rstd"""
    y, mean, rstd = R.ln_fwd(x, g, b)
    return y, np.stack([mean, rstd], -1)


def qkv(x16, Wqkv, bqkv):
    return x16 @ Wqkv.T + bqkv, acc_bound(np.abs(x16) @ np.abs(Wqkv).T + np.abs(bqkv), D)


def split_heads(t, B, S):
    """(N, 384) -> q, k, v (B, NH, S, HD)"""
    x = t.reshape(B, S, 3, NH, HD).transpose(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def merge_heads(t, B, S):
    """(B, NH, S, HD) -> (N, 128)"""
    return t.transpose(0, 2, 1, 3).reshape(B * S, D)


def pat(qkv_, B, S):
    """attention probabilities (B, NH, S, S) before their dropout"""
    q, k, _ = split_heads(qkv_, B, S)
    return R.softmax(q @ k.transpose(0, 1, 3, 2) * 0.25)


def ao(Pat, qkv_, B, S, keep_att, p):
    """attention output (N, 128).  Per term two more fp32 roundings than a sum of exact products: P * 1/(1-p), and its product with v"""
    _, _, v = split_heads(qkv_, B, S)
    Pm = Pat * _m(keep_att, p)
    return merge_heads(Pm @ v, B, S), merge_heads(acc_bound(np.abs(Pm) @ np.abs(v), S, 2), B, S)


def y1(x, ao_, Wo, bo, keep_o, p):
    m = _m(keep_o, p)
    return x + m * (ao_ @ Wo.T + bo), acc_bound(np.abs(x) + m * (np.abs(ao_) @ np.abs(Wo).T + np.abs(bo)), D, 2)


def hff(x1t, W1, b1, keep_h, p):
    m = _m(keep_h, p)
    return m * np.maximum(x1t @ W1.T + b1, 0.0), acc_bound(m * (np.abs(x1t) @ np.abs(W1).T + np.abs(b1)), D, 1)


def y2(y2_0, x1f, hff_, W2, b2, keep_y, p):
    """y2_0 + x1 + drop_y(hff W2^T + b2): 2048 products in four partial sums joined by atomics (4 more additions), the mask multiplier, y2_0 and x1"""
    m = _m(keep_y, p)
    return y2_0 + x1f + m * (hff_ @ W2.T + b2), acc_bound(np.abs(y2_0) + np.abs(x1f) + m * (np.abs(hff_) @ np.abs(W2).T + np.abs(b2)), FF, 4 + 2)


# ---------------------------------------------------------------------------------------------------- backward
def ln_bwd(dy, x, stats, g):
    """-> dx, addends of dg, addends of db (rows, n)"""
    return R.ln_bwd(dy, x, stats[:, 0], stats[:, 1], g)


def bcast_rows(dxw, S, bdiv):
    """one row per window, divided by bdiv -> (N, 128)"""
    return np.repeat(dxw, S, 0) / bdiv


def drop(t, keep, p):
    return t * _m(keep, p)


def dt_a(dt_c, W2t, hff_, p):
    """(dt_c W2) / (1 - p) where the saved hidden is positive.  W2t (2048, 128) = linear2.weight^T"""
    a = mult(p)
    on = hff_ > 0
    return np.where(on, dt_c @ W2t.T * a, 0.0), np.where(on, acc_bound(a * (np.abs(dt_c) @ np.abs(W2t).T), D, 1), 0.0)


def parts(dt_a_, W1t, dy2):
    """the four hidden-quarter partials (4, N, 128): quarter q of dt_a through its 512 rows of linear1.weight; dy2 (the residual path) in quarter 0 only.
    W1t (128, 2048) = linear1.weight^T"""
    ref, bnd = [], []
    for q in range(NQ):
        a, w = dt_a_[:, q * HQ:(q + 1) * HQ], W1t[:, q * HQ:(q + 1) * HQ]
        r, t = a @ w.T, np.abs(a) @ np.abs(w).T
        if q == 0:
            r, t = r + dy2, t + np.abs(dy2)
        ref.append(r); bnd.append(acc_bound(t, HQ, 1))
    return np.stack(ref), np.stack(bnd)


def dao(b_d, Wot):
    """b_d W_o.  Wot (128, 128) = out_proj.weight^T"""
    return b_d @ Wot.T


def attn_bwd(dao_, qkv_, Pat, B, S, keep_att, p):
    """gradient of qkv (N, 384) from the gradient of the attention output, and its accumulation bound, carried through the chain to first order:
    dP = (dO v^T) m, dot = sum_j dP P, dS = P (dP - dot), dq = dS k / 4, dk = dS^T q / 4, dv = (P m)^T dO"""
    q, k, v = split_heads(qkv_, B, S)
    dO = dao_.reshape(B, S, NH, HD).transpose(0, 2, 1, 3)
    m = _m(keep_att, p)
    T = lambda a: a.transpose(0, 1, 3, 2)
    dP = (dO @ T(v)) * m
    e_dP = acc_bound(np.abs(dO) @ T(np.abs(v)), HD, 1) * m
    dot = (dP * Pat).sum(-1, keepdims=True)
    e_dot = (e_dP * Pat).sum(-1, keepdims=True) + acc_bound(np.abs(dP * Pat).sum(-1, keepdims=True), S, 1)
    dS = Pat * (dP - dot)
    e_dS = Pat * (e_dP + e_dot) + 2 * EPS32 * Pat * (np.abs(dP) + np.abs(dot))
    qs = 0.25 * q
    dq = 0.25 * (dS @ k)
    e_dq = 0.25 * (e_dS @ np.abs(k) + acc_bound(np.abs(dS) @ np.abs(k), S, 1))
    dk = T(dS) @ qs
    e_dk = T(e_dS) @ np.abs(qs) + acc_bound(T(np.abs(dS)) @ np.abs(qs), S, 1)
    Pm = Pat * m
    dv = T(Pm) @ dO
    e_dv = acc_bound(T(Pm) @ np.abs(dO), S, 2)
    pack = lambda a, b, c: np.stack([a, b, c]).transpose(1, 3, 0, 2, 4).reshape(B * S, 3 * D)
    return pack(dq, dk, dv), pack(e_dq, e_dk, e_dv)


def b_b(b_d, Wot, qkv_, Pat, B, S, keep_att, p, r16=ident):
    """the gradient of qkv from b_d: through out_proj (rounded by r16 as the kernel rounds it in LDS), then the attention backward"""
    return attn_bwd(r16(dao(b_d, Wot)), qkv_, Pat, B, S, keep_att, p)


def dx_attn(b_b_, Wint, dy_f):
    """b_b W_in + dy_f.  Wint (128, 384) = in_proj_weight^T"""
    return b_b_ @ Wint.T + dy_f, acc_bound(np.abs(b_b_) @ np.abs(Wint).T + np.abs(dy_f), 3 * D, 1)


# ---------------------------------------------------------------------------------------------------- the stages end to end
def chain_fwd(xin, P, B, S, ln_in, p, masks, y2_0=None, r16=ident, r32=ident):
    """P: dict of float64 parameters (Wqkv, Wo, W1, W2, bqkv, bo, b1, b2, n1g, n1b, ln_g, ln_b); masks: dict att, o, h, y of keep arrays (or None each).
    r16 / r32 round a saved 16-bit / fp32 tensor as the kernel stores it (identity: exact float64).  -> dict of every saved tensor"""
    c = {}
    mk = (lambda k: None) if masks is None else masks.get
    if ln_in:
        xf, st = ln(xin, P["ln_g"], P["ln_b"])
        c["xf_out"], c["st_out"] = r32(xf), r32(st)
        xf = c["xf_out"]
    else:
        xf = xin
    c["xf"] = xf
    c["xt"] = r16(xf)
    c["qkv"] = r16(qkv(c["xt"], P["Wqkv"], P["bqkv"])[0])
    c["Pat"] = r32(pat(c["qkv"], B, S))
    c["ao"] = r16(ao(c["Pat"], c["qkv"], B, S, mk("att"), p)[0])
    c["y1"] = r32(y1(xf, c["ao"], P["Wo"], P["bo"], mk("o"), p)[0])
    x1, st1 = ln(c["y1"], P["n1g"], P["n1b"])
    c["x1f"], c["st1"] = r32(x1), r32(st1)
    c["x1t"] = r16(c["x1f"])
    c["hff"] = r16(hff(c["x1t"], P["W1"], P["b1"], mk("h"), p)[0])
    c["y2_0"] = np.zeros_like(c["y1"]) if y2_0 is None else y2_0
    c["y2"] = r32(y2(c["y2_0"], c["x1f"], c["hff"], P["W2"], P["b2"], mk("y"), p)[0])
    return c


def chain_bwd(c, P, B, S, p, masks, dx2, st2, n2g, r16=ident, r32=ident):
    """the layer's backward from dx2 = the gradient of LN2(y2; n2g)'s output, st2 = that norm's statistics: FFN half, then attention half.
    -> dict dy2, dg2, db2 (column sums), dt_c, dt_a, parts, dy_f, dg1, db1, b_d, b_b, dx"""
    mk = (lambda k: None) if masks is None else masks.get
    g = {}
    dy2, ag, ab = ln_bwd(dx2, c["y2"], st2, n2g)
    g["dy2"], g["dg2"], g["db2"] = dy2, ag.sum(0), ab.sum(0)
    g["dt_c"] = r16(drop(dy2, mk("y"), p))
    g["dt_a"] = r16(dt_a(g["dt_c"], P["W2"].T, c["hff"], p)[0])
    g["parts"] = r32(parts(g["dt_a"], P["W1"].T, r32(dy2))[0])
    dy_f, ag, ab = ln_bwd(g["parts"].sum(0), c["y1"], c["st1"], P["n1g"])
    g["dy_f"], g["dg1"], g["db1"] = r32(dy_f), ag.sum(0), ab.sum(0)
    g["b_d"] = r16(drop(g["dy_f"], mk("o"), p))
    g["b_b"] = r16(b_b(g["b_d"], P["Wo"].T, c["qkv"], c["Pat"], B, S, mk("att"), p, r16)[0])
    g["dx"] = r32(dx_attn(g["b_b"], P["Wqkv"].T, g["dy_f"])[0])
    return g
