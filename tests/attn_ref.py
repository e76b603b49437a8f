"""Restatement, in numpy, of fused sparse attention (tcgnn_attn_forward / _backward / _source_grad), the bounds the kernels are held to and
the input sets.  Used by tests/test_gpu_fused_attention.py; no GPU needed to import.

Reference: s = fl32(fl32(dot64) scale) as the contract says; then fp64: softmax by row, L, Y, and the three gradients.  The backward
calls are given fl32 of the REFERENCE's Y, L and delta, so each call is held to a bound of its own.
Bounds, with u = 2^-24 and to first order.
  the score     another summation order of the fp64 dot moves it by parts in 2^40 and can flip fl32(dot), and with it the fp32 product
                with scale, by an ulp each: |ds| <= 2^-22 |s|, which an exponential turns into that relative error of its value.
  es_exp(x)     x = fl32(a - b) rounds (u |x|), the product with log2 e and the constant round (2 u |x|), the hardware exponential is
                good to 1 ulp = 2 u (edge_ops_ref's allowance):  EXP(x) = u (3 |x| + 2) relative.
  forward       an edge's weight is es_exp(s - m_then) times the rescale factors es_exp(m_old - m_new) on its way to the row's maximum
                M: the arguments add up to |s - M|, and there is at most one factor per kSegUnroll = 4 edges of the row (one per trip of
                a lane) plus 6 butterfly levels and 3 wavefront folds:  W = 2^-22 |s| + 3 u |s - M| + 2 u (ceil(deg / 4) + 10) + OWN_SUM
                (the fp64 sums, gat_ref's 2^-40).  Y = sum w v / sum w moves by sum p W |v - Y|; it rounds once:
                    |Y - ref| <= sum_e p W (|v| + |ref|) + FLOOR sum_e (|v| + 1) + u |ref| + 2^-149
                (FLOOR = 2^-125: a weight below the normal range may come out as 0),   |L - ref| <= sum_e p W + u |ref| + 2^-40.
  delta         fl32 of an fp64 dot: u |ref| + OWN_SUM sum |dY Y| + 2^-149.
  p (backward)  es_exp(s - L): P = 2^-22 |s| + EXP(s - L) relative; a = <dY, v> is fp64: OWN_SUM sum |dY v|.
  dq, dk        g = p (a - delta):  |dg| <= p (P |a - delta| + [row side: delta's bound] + OWN_SUM sum |dY v|) + FLOOR (|a - delta| + 1);
                    |dq - ref| <= |scale| sum_e (|dg| |k| + OWN_SUM |g k|) + u |ref| + 2^-149,   dk the same with q[row e], by source;
  dv            |dv - ref| <= sum_e (p (P + OWN_SUM) + FLOOR) |dY| + u |ref| + 2^-149.
Nothing was fitted to the kernel; measured worst shares (profiles/r34/gpu_fused_attention_tests_figures.txt): Y 0.106,
L 0.183, delta 0.998 (half an ulp of a correctly rounded result), dq 0.998 (delta's term), dk 0.586, dv 0.586."""
import numpy as np

import gated_ref as G
from gated_ref import FLOOR, OWN_SUM, U, row_class_graphs, worst_share  # noqa: F401  (the graph and the measure are gated_ref's)

SHAPES = ((1, 1), (3, 5), (8, 8), (4, 32), (5, 24), (2, 64), (1, 256), (1, 260))
SETS = ("normal_x1", "normal_x8", "increasing", "decreasing", "constant_k", "aliased")
NAMES = ("Y", "L", "delta", "dq", "dk", "dv")


def sorted_rows(rp, col):
    """the same rows with every row's column ids ascending: a score that grows with the column id then grows along every row"""
    rows = G.edge_rows(rp)
    return rp, np.asarray(col[:int(rp[-1])])[np.lexsort((col[:int(rp[-1])], rows))]


def inputs(name, n, H, F, seed=31):
    """(q, k, v, dY), fp32 [n, H F]: normal; q and k x 8 (scores of a few hundred: the rescales matter); scores that rise / fall with
    the column id over +-30 (on sorted_rows the maximum changes at every step / never); k constant (all scores of a row equal); one array"""
    rng = np.random.default_rng([seed, H, F])
    q, k, v, dY = (rng.standard_normal((n, H * F)).astype(np.float32) for _ in range(4))
    if name == "normal_x8":
        q, k = 8 * q, 8 * k
    elif name in ("increasing", "decreasing"):
        q = np.full_like(q, 1.0 if name == "increasing" else -1.0)
        k = np.repeat(((np.arange(n) / n - 0.5) * 60.0 / np.sqrt(F)).astype(np.float32)[:, None], H * F, axis=1)
    elif name == "constant_k":
        k = np.repeat(k[:1], n, axis=0)
    elif name == "aliased":
        k = v = q
    return q, k, v, dY


def attn_f64(rp, col, q, k, v, dY, H, scale):
    """{name: (fp64 reference, bound)} for NAMES - Y, dq, dk, dv [n, H F]; L, delta [n, H] - and "given": fl32 of the reference's
    Y, L and delta, what the backward calls are handed"""
    n, rows, cols = len(rp) - 1, G.edge_rows(rp), np.asarray(col[:int(rp[-1])], np.int64)
    E, F, deg = len(rows), q.shape[1] // H, np.diff(np.asarray(rp, np.int64))
    q3, k3, v3, g3 = (np.asarray(t, np.float64).reshape(n, H, F) for t in (q, k, v, dY))
    qr, kc, vc, gr = q3[rows], k3[cols], v3[cols], g3[rows]
    by = lambda index, T: G._sum_by(index, T.reshape(E, -1), n)   # noqa: E731
    f32 = lambda a: a.astype(np.float32).astype(np.float64)   # noqa: E731
    s = (np.einsum("ehf,ehf->eh", qr, kc).astype(np.float32) * np.float32(scale)).astype(np.float64)
    has = deg > 0
    M = np.zeros((n, H))
    M[has] = np.maximum.reduceat(s, np.asarray(rp, np.int64)[:-1][has], axis=0)
    w = np.exp(s - M[rows])
    l = by(rows, w)
    L = np.where(has[:, None], M + np.log(np.where(l > 0, l, 1.0)), 0.0)
    p = w / l[rows]
    Y = by(rows, p[:, :, None] * vc)
    pW = p * (2.0 ** -22 * np.abs(s) + 3 * U * np.abs(s - M[rows]) + 2 * U * (np.ceil(deg / 4.0)[rows, None] + 10) + OWN_SUM)
    out = {"Y": (Y, by(rows, pW[:, :, None] * (np.abs(vc) + np.abs(Y.reshape(n, H, F)[rows])) + FLOOR * (np.abs(vc) + 1)) + U * np.abs(Y) + 2.0 ** -149),
           "L": (L, by(rows, pW) + U * np.abs(L) + 2.0 ** -40)}
    Y32, L32 = f32(Y), f32(L)
    delta = (g3 * Y32.reshape(n, H, F)).sum(-1)
    b_delta = U * np.abs(delta) + OWN_SUM * np.abs(g3 * Y32.reshape(n, H, F)).sum(-1) + 2.0 ** -149
    out["delta"], d32 = (delta, b_delta), f32(delta)
    pb, x = np.exp(s - L32[rows]), np.abs(s - L32[rows])
    P = 2.0 ** -22 * np.abs(s) + U * (3 * x + 2)
    a, abs_a = np.einsum("ehf,ehf->eh", gr, vc), OWN_SUM * np.einsum("ehf,ehf->eh", np.abs(gr), np.abs(vc))

    def grad(index, d, extra, other):   # scale sum_e g other[e] by index, g = p (a - d[row e]), and its bound
        c = a - d[rows]
        g, dg = pb * c, pb * (P * np.abs(c) + extra + abs_a) + FLOOR * (np.abs(c) + 1)
        ref = scale * by(index, g[:, :, None] * other)
        return ref, abs(scale) * by(index, (dg[:, :, None] + OWN_SUM * np.abs(g)[:, :, None]) * np.abs(other)) + U * np.abs(ref) + 2.0 ** -149

    out["dq"] = grad(rows, delta, b_delta[rows], kc)
    out["dk"] = grad(cols, d32, 0.0, qr)
    dv = by(cols, pb[:, :, None] * gr)
    out["dv"] = (dv, by(cols, (pb * (P + OWN_SUM) + FLOOR)[:, :, None] * np.abs(gr)) + U * np.abs(dv) + 2.0 ** -149)
    out["given"] = tuple(t.astype(np.float32) for t in (Y, L, delta))
    return out


def dense_f64(rp, col, q, k, v, H, scale=None):   # torch's plain composition, differentiable, by index_add_
    import torch
    rows, cols = torch.from_numpy(G.edge_rows(rp)), torch.from_numpy(np.asarray(col[:int(rp[-1])], np.int64))
    n, E, F = q.shape[0], len(rows), q.shape[1] // H
    s = (q[rows].view(E, H, F) * k[cols].view(E, H, F)).sum(-1) * (F ** -0.5 if scale is None else scale)
    m = torch.zeros(n, H, dtype=s.dtype).scatter_reduce(0, rows[:, None].expand(-1, H), s.detach(), "amax", include_self=False)
    w = torch.exp(s - m[rows])
    p = w / torch.zeros(n, H, dtype=s.dtype).index_add_(0, rows, w)[rows]
    return torch.zeros(n, H, F, dtype=s.dtype).index_add_(0, rows, p[:, :, None] * v[cols].view(E, H, F)).reshape(n, H * F)
