"""Restatement, in numpy, of fused sparse attention with edge features (tcgnn_attn_edge_forward / _backward / _source_grad), the bounds
the kernels are held to and the input sets.  Used by tests/test_gpu_attn_edge.py and tests/test_attn_edge_cpu.py; no GPU needed.

Reference: t = dot64(q, k) + dot64(q, ee), s = fl32(fl32(t) scale) as the contract says; then fp64 with the message m = v + ee.  The
row-side call is given fl32 of the REFERENCE's Y and L, the source call fl32 of the reference's p and g: each call has a bound of its own.
Bounds: attn_ref's derivation (u = 2^-24, first order) with these changes.
  the score     t is a sum of two dots that may cancel, so the fp64 error of the sums (OWN_SUM of their absolute terms) is no longer small
                against an ulp of fl32(t) by construction: |ds| <= S = 2^-22 |s| + |scale| OWN_SUM (sum |q k| + sum |q ee|), and S stands
                wherever attn_ref has 2^-22 |s| (an exponential turns it into that relative error).
  Y, dq         |v| becomes |v + ee| and |k| becomes |k + ee| (the fp64 sum of two floats is exact to 2^-53: under OWN_SUM);
                a = <dY, v> + <dY, ee>: OWN_SUM (sum |dY v| + sum |dY ee|).
  pg            p = fl32(es_exp(s - L)): p (P + u) + FLOOR + 2^-149;   g = fl32(p (a - delta)): |dg| + u |g| + 2^-149, |dg| as for dq.
  dee           fl32(scale g q + p dY): |scale| |dg| |q| + (p P + FLOOR) |dY| + OWN_SUM (|scale g q| + |p dY|) + u |ref| + 2^-149.
  dk, dv        from the GIVEN fl32(p), fl32(g) nothing is recomputed: the rounding of what was given, u |g| resp. u p (+ 2^-149) per edge,
                the fp64 sum and one rounding:  |dk - ref| <= |scale| sum_e ((u + OWN_SUM) |g| + 2^-149) |q| + u |ref| + 2^-149, dv alike.
Nothing was fitted to the kernel; the measured worst shares are in DESIGN.md 4.24 and profiles/r35/gpu_attn_edge_tests_figures.txt."""
import numpy as np

import attn_ref as A
import gated_ref as G
from attn_ref import SHAPES, row_class_graphs, sorted_rows, worst_share  # noqa: F401
from gated_ref import FLOOR, OWN_SUM, U

SETS = ("normal_x1", "normal_x8", "increasing", "edge_only")
NAMES = ("Y", "L", "delta", "dq", "dee", "pg", "dk", "dv")


def width(name, H, F):   # columns of an output per node (Y, L, delta, dq, dk, dv) or per edge (dee, pg)
    return {"L": H, "delta": H, "pg": 2 * H}.get(name, H * F)


def inputs(name, rp, col, H, F, seed=37):
    """(q, k, v, dY, ee): attn_ref's sets with ee [E, H F] - normal (x 8 with q and k); half the source's key (scores still rise along a
    sorted row); edge_only: k = v = 0, every score and every message comes from ee alone (a wrong edge position or perm index shows)"""
    n, cols = len(rp) - 1, np.asarray(col[:int(rp[-1])], np.int64)
    q, k, v, dY = A.inputs("normal_x1" if name == "edge_only" else name, n, H, F)
    ee = np.random.default_rng([seed, H, F]).standard_normal((len(cols), H * F)).astype(np.float32)
    if name == "normal_x8":
        ee = 8 * ee
    elif name == "increasing":
        ee = (0.5 * k[cols]).astype(np.float32)
    elif name == "edge_only":
        k, v = np.zeros_like(k), np.zeros_like(v)
    return q, k, v, dY, ee


def attn_edge_f64(rp, col, q, k, v, dY, ee, H, scale):
    """{name: (fp64 reference, bound)} for NAMES - Y, dq, dk, dv [n, H F]; L, delta [n, H]; dee [E, H F]; pg [E, 2 H] - and "given":
    fl32 of the reference's (Y, L, delta, pg), what the backward calls are handed"""
    n, rows, cols = len(rp) - 1, G.edge_rows(rp), np.asarray(col[:int(rp[-1])], np.int64)
    E, F, deg = len(rows), q.shape[1] // H, np.diff(np.asarray(rp, np.int64))
    q3, k3, v3, g3 = (np.asarray(t, np.float64).reshape(n, H, F) for t in (q, k, v, dY))
    ec = np.asarray(ee, np.float64).reshape(E, H, F)
    qr, kc, vc, gr = q3[rows], k3[cols], v3[cols], g3[rows]
    by = lambda index, T: G._sum_by(index, T.reshape(E, -1), n)   # noqa: E731
    f32 = lambda a: a.astype(np.float32).astype(np.float64)   # noqa: E731
    dot, absdot = (lambda a, b: np.einsum("ehf,ehf->eh", a, b)), (lambda a, b: np.einsum("ehf,ehf->eh", np.abs(a), np.abs(b)))
    s = ((dot(qr, kc) + dot(qr, ec)).astype(np.float32) * np.float32(scale)).astype(np.float64)
    S = 2.0 ** -22 * np.abs(s) + abs(scale) * OWN_SUM * (absdot(qr, kc) + absdot(qr, ec))
    has = deg > 0
    M = np.zeros((n, H))
    M[has] = np.maximum.reduceat(s, np.asarray(rp, np.int64)[:-1][has], axis=0)
    w = np.exp(s - M[rows])
    l = by(rows, w)
    L = np.where(has[:, None], M + np.log(np.where(l > 0, l, 1.0)), 0.0)
    p, mc, kec = w / l[rows], vc + ec, kc + ec
    Y = by(rows, p[:, :, None] * mc)
    pW = p * (S + 3 * U * np.abs(s - M[rows]) + 2 * U * (np.ceil(deg / 4.0)[rows, None] + 10) + OWN_SUM)
    out = {"Y": (Y, by(rows, pW[:, :, None] * (np.abs(mc) + np.abs(Y.reshape(n, H, F)[rows])) + FLOOR * (np.abs(mc) + 1)) + U * np.abs(Y) + 2.0 ** -149),
           "L": (L, by(rows, pW) + U * np.abs(L) + 2.0 ** -40)}
    Y32, L32 = f32(Y), f32(L)
    delta = (g3 * Y32.reshape(n, H, F)).sum(-1)
    b_delta = U * np.abs(delta) + OWN_SUM * np.abs(g3 * Y32.reshape(n, H, F)).sum(-1) + 2.0 ** -149
    out["delta"] = (delta, b_delta)
    pb, x = np.exp(s - L32[rows]), np.abs(s - L32[rows])
    P = S + U * (3 * x + 2)
    c = dot(gr, vc) + dot(gr, ec) - delta[rows]
    g = pb * c
    dg = pb * (P * np.abs(c) + b_delta[rows] + OWN_SUM * (absdot(gr, vc) + absdot(gr, ec))) + FLOOR * (np.abs(c) + 1)
    dq = scale * by(rows, g[:, :, None] * kec)
    out["dq"] = (dq, abs(scale) * by(rows, (dg + OWN_SUM * np.abs(g))[:, :, None] * np.abs(kec)) + U * np.abs(dq) + 2.0 ** -149)
    t1, t2 = scale * g[:, :, None] * qr, pb[:, :, None] * gr
    dee = (t1 + t2).reshape(E, H * F)
    out["dee"] = (dee, (abs(scale) * dg[:, :, None] * np.abs(qr) + (pb * P + FLOOR)[:, :, None] * np.abs(gr) + OWN_SUM * (np.abs(t1) + np.abs(t2))
                        ).reshape(E, H * F) + U * np.abs(dee) + 2.0 ** -149)
    pg = np.stack([pb, g], axis=2).reshape(E, 2 * H)
    out["pg"] = (pg, np.stack([pb * (P + U) + FLOOR, dg + U * np.abs(g)], axis=2).reshape(E, 2 * H) + 2.0 ** -149)
    p32, g32 = f32(pb), f32(g)   # what the source call is handed: its reference is formed from the unrounded p and g
    dk, dv = scale * by(cols, g[:, :, None] * qr), by(cols, pb[:, :, None] * gr)
    out["dk"] = (dk, abs(scale) * by(cols, ((U + OWN_SUM) * np.abs(g) + 2.0 ** -149)[:, :, None] * np.abs(qr)) + U * np.abs(dk) + 2.0 ** -149)
    out["dv"] = (dv, by(cols, ((U + OWN_SUM) * pb + 2.0 ** -149)[:, :, None] * np.abs(gr)) + U * np.abs(dv) + 2.0 ** -149)
    out["given"] = tuple(t.astype(np.float32) for t in (Y, L, delta, np.stack([p32, g32], axis=2)))
    return out


def dense_f64(rp, col, q, k, v, ee, H, scale=None):   # torch's plain composition, differentiable, by index_add_
    import torch
    rows, cols = torch.from_numpy(G.edge_rows(rp)), torch.from_numpy(np.asarray(col[:int(rp[-1])], np.int64))
    n, E, F = q.shape[0], len(rows), q.shape[1] // H
    ke, ve = (k[cols] + ee).view(E, H, F), (v[cols] + ee).view(E, H, F)
    s = (q[rows].view(E, H, F) * ke).sum(-1) * (F ** -0.5 if scale is None else scale)
    m = torch.zeros(n, H, dtype=s.dtype).scatter_reduce(0, rows[:, None].expand(-1, H), s.detach(), "amax", include_self=False)
    w = torch.exp(s - m[rows])
    p = w / torch.zeros(n, H, dtype=s.dtype).index_add_(0, rows, w)[rows]
    return torch.zeros(n, H, F, dtype=s.dtype).index_add_(0, rows, p[:, :, None] * ve).reshape(n, H * F)


def layer_f64(rp, col, X, edge_attr, w, H, F, concat):
    """TransformerConv(edge_dim, beta) from its parameters w (a dict of fp64 tensors; weights_beta may be absent)"""
    import torch
    Y = dense_f64(rp, col, *(X @ w["weights_" + c] + w["bias_" + c] for c in "qkv"), edge_attr @ w["weights_edge"], H)
    Y, Xr = (Y if concat else Y.view(-1, H, F).mean(1)), X @ w["weights_root"]
    if w.get("weights_beta") is None:
        return Y + Xr + w["bias"]
    b = torch.sigmoid(torch.cat([Y, Xr, Y - Xr], 1) @ w["weights_beta"])
    return b * Xr + (1 - b) * Y + w["bias"]
