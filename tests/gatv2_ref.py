"""Restatements, in numpy and torch, of GATv2 attention (tcgnn_gatv2_softmax / _backward / tcgnn_gatv2_source_grad, the operator
gatv2_attention and the layer GATv2Conv), the bounds the kernels are held to - each with its derivation - and the input sets.  Shared
by tests/test_gatv2_cpu.py and tests/test_gpu_gatv2.py; no GPU needed to import.

The activation term.  z = fl32(xl[col e] + xr[row e]), l = z > 0 ? z : fl32(z slope): two fp32 roundings, exactly GAT's (act_f32);
c = z > 0 ? attn : fl32(attn slope), the factor of the backward (slope_factor_f32).

Score.  The kernel forms s = fl32(sum_f (double)attn_f (double)l_f).  A product of two fp32 numbers has 48 significant bits: exact in
fp64.  An fp64 sum of F terms in ANY order differs from the true sum s64 by at most (F - 1) u (1 + u)^(F-1) sum |term| with u = 2^-53,
which for every F < 2^20 is below F 2^-50 sum |term| with room to spare (it also covers this file's own s64, an fp64 sum in numpy's
order); the one rounding to fp32 adds 2^-24 |s64|, or 2^-149 where the result is subnormal:
    |score - s64| <= 2^-24 |s64| + 2^-149 + F 2^-50 sum_f |attn_f l_f|                                             (score_bound)

Probabilities.  p is tcgnn_edge_softmax's arithmetic with beta = 1 on the rounded scores the same call wrote (the same device code):
the reference is edge_ops_ref.softmax_f64 of those scores and the bounds are edge_ops_ref's REL / ABS / ROW_SUM unchanged.

g.  g = p (float)((double)dp - sum_row p dp) is tcgnn_gat_softmax_backward's arithmetic with slope 1 (the same device code as
tcgnn_edge_softmax_backward's): the reference is gat_ref.gat_bwd_f64 with slope = 1 and the bound its C_GAT_BWD with
edge_ops_ref.BWD_FLOOR, unchanged (g_worst).

d_xr, d_xl.  Each is ONE rounding of an fp64 sum of fp32 terms the test can form exactly from what the call wrote: term = fl32(g c).
Against S, the fp64 sum of those very terms, the result may differ by its own rounding plus the error of the fp64 additions, which is
at most (additions on the longest chain) 2^-53 sum |term|: a lane adds its share of a segment - the 300 000-edge row is 1 172 terms
per lane at (H, F) = (1, 4) and 9 375 at (3, 8) - and the trees add a dozen levels, so the worst case is 2^-39 sum |term| and the
expected error (a random walk) some 2^-46.  gat_ref.OWN_SUM = 2^-40 is what tcgnn_gat's sums are held to on the same graph; it is
kept, unchanged:
    |d - S| <= 2^-24 |S| + 2^-149 + OWN_SUM sum |term|                                                            (own_sum_share)

d_attn.  fl32 of the fp64 sum over ALL edges of the exact products (double)g (double)l.  Fewer than 2^23 fp64 additions in any order
err by at most n 2^-53 <= 2^-30 of the sum of magnitudes:
    |d_attn - S| <= 2^-24 |S| + 2^-149 + 2^-30 sum_e |g l|                                                        (own_sum_share, D_ATTN_SUM)

Measured on the MI355X (tests/test_gpu_gatv2.py, all 80 cases; profiles/r20/gpu_gatv2_tests_figures.txt), worst share of each bound:
score 0.999 and d_xr / d_xl 1.00 (their own rounding - beyond it 0, 3.7e-4 and 9.6e-5 of the summation's allowance), d_attn 0.69
(beyond its rounding 7.9e-7 of 2^-30), p 0.22 / 0.55 / 0.06 of REL / ABS / ROW_SUM, g 0.038 of C_GAT_BWD.
"""
import zlib

import numpy as np

import edge_ops_ref as R
import gat_ref as G
import graphs

D_ATTN_SUM = 2.0 ** -30
SLOPES = G.SLOPES
SETS = G.SETS
ROW_SHAPES = ((1, 4), (3, 8))                  # (H, F) of the row-class cases
POWERLAW_SHAPES = ((1, 1), (2, 3), (1, 41), (5, 24), (8, 8), (4, 32), (2, 136), (3, 100))
LAYER_CASE = dict(heads=3, out=8, inp=24, seed=5)   # the layer tests/test_gpu_gatv2.py runs


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

# attn's scale per row-class graph.  On the transposed graph EVERY row has 7 600 - 8 100 edges; with attn of order 1 the scores of the
# wider sets spread over tens to thousands, most rows then hold one probability between 0.3 and 0.9, and there the flat 1e-7 of
# edge_ops_ref.ABS is at the edge of what fp32 can do at all: the p's own rounding is 3e-8, and the rounded exponents of the entries it
# competes with move it by p (1 - p) 1.5e-7 more.  The numpy restatement (correctly rounded exp2) needs 0.51 - 1.94 of ABS there for
# every one of 37 seeds tried, so by the rule of tests/test_gatv2_cpu.py the INPUTS change: on that graph attn is scaled by 2^-14, which
# keeps a row's scores within a few units for every set (|z| still reaches 2e4: z does not depend on attn; the sums d_xl, the reason
# that graph is run, are relative to their terms and do not care).  The wide spreads are run on the row-class graph itself.
ATTN_SCALE = {"row_classes": 1.0, "row_classes_T": 2.0 ** -14}


def x_sets(n, H, F, seed=23, attn_scale=1.0):
    """{name: (xl, xr, attn)}: fp32 [n, H F] twice and [H, F], in the manner of gat_ref.el_er_sets - normal x {1, 8, 30}; constant: xl
    the same for every node (a row's scores are all equal); magnitude 1e4: |z| reaches 2e4 and, where the signs differ, a few hundred.
    attn is standard normal over sqrt(F), so a score has the magnitude of one term, times attn_scale (a power of two: ATTN_SCALE)."""
    rng = np.random.default_rng([seed, H, F])
    zl, zr = rng.standard_normal((n, H * F)).astype(np.float32), rng.standard_normal((n, H * F)).astype(np.float32)
    attn = (rng.standard_normal((H, F)) / np.sqrt(F) * attn_scale).astype(np.float32)
    out = {"normal_x1": (zl, zr), "normal_x8": ((8 * zl).astype(np.float32), (8 * zr).astype(np.float32)),
           "normal_x30": ((30 * zl).astype(np.float32), (30 * zr).astype(np.float32))}
    out["constant"] = (np.repeat(rng.standard_normal((1, H * F)).astype(np.float32), n, axis=0), zr.copy())
    big = lambda z: (1e4 * np.sign(z) * (1 + 0.01 * np.abs(z))).astype(np.float32)   # noqa: E731
    out["magnitude_1e4"] = (big(zl), big(zr))
    return {k: (np.ascontiguousarray(a), np.ascontiguousarray(b), attn) for k, (a, b) in out.items()}


def transposed_graph(rp, col):
    """(rowptr, col) of A^T as a graph of its own, int32: its rows are A's columns"""
    import walks
    rp_t, col_t, _ = walks.transposed_csr(rp, col[:int(rp[-1])])
    return rp_t.astype(np.int32), col_t.astype(np.int32)


_GRAPHS = {}


def row_class_graphs():
    """{"row_classes": gat_ref.row_class_graph(), "row_classes_T": its transpose}: on the second the source-side kernel walks the rows
    of every length class.  Built once."""
    if not _GRAPHS:
        rp, col = G.row_class_graph()
        _GRAPHS["row_classes"] = (rp, col)
        _GRAPHS["row_classes_T"] = transposed_graph(rp, col)
    return _GRAPHS


def powerlaw():
    return graphs.powerlaw_graph(3000, 12, seed=31, symmetric=False)


def dp_for(H, E, salt=0):
    return np.random.default_rng(zlib.crc32(("gatv2/dp/%d/%d/%d" % (H, E, salt)).encode())).standard_normal((H, E)).astype(np.float32)


# ---- numpy restatements ------------------------------------------------------------------------------------------------------------------

def _edge_rows(rp):
    rp = np.asarray(rp, dtype=np.int64)
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


def z_f32(rp, col, xl, xr):
    """z[e, hF + f] = fl32(xl[col e] + xr[row e]) for the edges rows cover, fp32 [E, H F]: one rounding"""
    E = int(np.asarray(rp)[-1])
    return np.asarray(xl, np.float32)[np.asarray(col[:E], dtype=np.int64)] + np.asarray(xr, np.float32)[_edge_rows(rp)]


def act_f32(z, slope):
    """l = z > 0 ? z : fl32(z slope): the second rounding (numpy multiplies two fp32 numbers in fp32, rounded once)"""
    return np.where(z > 0, z, z * np.float32(slope)).astype(np.float32)


def slope_factor_f32(z, attn, slope):
    """c[e, hF + f] = z > 0 ? attn[h, f] : fl32(attn[h, f] slope), fp32 [E, H F]"""
    a = np.asarray(attn, np.float32).reshape(1, -1)
    return np.where(z > 0, a, a * np.float32(slope)).astype(np.float32)


def scores_f64(l, attn):
    """(s64 [H, E], mag [H, E]) - the fp64 dot product of attn and l per head and the sum of the products' magnitudes"""
    H, F = attn.shape
    t = l.astype(np.float64).reshape(len(l), H, F) * np.asarray(attn, dtype=np.float64)[None]
    return np.ascontiguousarray(t.sum(2).T), np.ascontiguousarray(np.abs(t).sum(2).T)


def score_bound(s64, mag, F):
    return 2.0 ** -24 * np.abs(s64) + 2.0 ** -149 + F * 2.0 ** -50 * mag


def score_share(score, s64, mag, F):
    """(whole, excess): whole = worst |score - s64| / score_bound, which must be <= 1; excess = what the score needs BEYOND its own
    rounding, as a share of the summation's allowance alone - worst (|score - s64| - 2^-24 |s64| - 2^-149) / (F 2^-50 mag).  (A correctly
    rounded result uses up to all of the rounding term, whatever the inputs: only the excess says how the sum was formed.)"""
    if s64.size == 0:
        return 0.0, 0.0
    err = np.abs(np.asarray(score, dtype=np.float64) - s64)
    whole = float((err / score_bound(s64, mag, F)).max())
    over = np.maximum(err - 2.0 ** -24 * np.abs(s64) - 2.0 ** -149, 0.0)
    if np.any(over[mag == 0] != 0):
        return whole, float("inf")
    return whole, (float((over[mag > 0] / (F * 2.0 ** -50 * mag[mag > 0])).max()) if (mag > 0).any() else 0.0)


def softmax_shares(rp, p, score):
    """worst shares (relative, absolute, row sum) of edge_ops_ref's bounds over the heads: p [H, E] against softmax_f64 of score [H, E]"""
    shares = [0.0, 0.0, 0.0]
    for h in range(len(p)):
        p64, dist = R.softmax_f64(rp, score[h], 1.0)
        shares = [max(a, b) for a, b in zip(shares, R.softmax_bounds_hold(rp, p[h], p64, dist))]
    return shares


def g_worst(rp, col, p, dp, g):
    """the constant g needs: gat_ref's fp64 backward with slope 1 (ds = g whatever the sign of raw), to be held against C_GAT_BWD"""
    n, H = len(rp) - 1, len(p)
    zero = np.zeros((n, H), np.float32)
    return G.ds_worst(rp, g, G.gat_bwd_f64(rp, col, zero, zero, 1.0, p, dp))


def segment_sums(terms, seg, n):
    """(S, A) [n, D]: the fp64 sums of terms [E, D] and of their magnitudes over the segments seg[e]"""
    terms = np.asarray(terms, dtype=np.float64)
    S, A = np.zeros((n, terms.shape[1])), np.zeros((n, terms.shape[1]))
    if len(terms):
        order = np.argsort(seg, kind="stable")
        cnt = np.bincount(seg, minlength=n)[:n]
        full = np.nonzero(cnt > 0)[0]
        starts = (np.cumsum(cnt) - cnt)[full]
        t = terms[order]
        S[full], A[full] = np.add.reduceat(t, starts, axis=0), np.add.reduceat(np.abs(t), starts, axis=0)
    return S, A


def own_sum_share(got, S, A, rel):
    """(whole, excess): whole = worst |got - S| / (2^-24 |S| + 2^-149 + rel A), which must be <= 1; a sum without terms must be exactly 0
    (inf otherwise).  excess = beyond the result's own rounding, as a share of the summation's allowance alone - worst
    (|got - S| - 2^-24 |S| - 2^-149) / (rel A), as gat_ref.sum_of_own_terms_worst measures it (see score_share)."""
    got = np.asarray(got, dtype=np.float64)
    if np.any(got[A == 0] != 0) or not np.isfinite(got).all():
        return float("inf"), float("inf")
    if not got.size:
        return 0.0, 0.0
    err = np.abs(got - S)
    ok = A > 0
    excess = float((np.maximum(err - 2.0 ** -24 * np.abs(S) - 2.0 ** -149, 0.0)[ok] / (rel * A[ok])).max()) if ok.any() else 0.0
    return float((err / (2.0 ** -24 * np.abs(S) + 2.0 ** -149 + rel * A)).max()), excess


def node_terms(g, c):
    """term[e, hF + f] = fl32(g[h, e] c[e, hF + f]), fp32 [E, H F]: what d_xr sums by row and d_xl by source node"""
    H = len(g)
    F = c.shape[1] // H
    return (np.repeat(np.asarray(g, np.float32).T, F, axis=1) * c).astype(np.float32)


def attn_terms(g, l):
    """(S, A) [H, F]: the fp64 sums over all edges of the exact products g[h, e] l[e, hF + f] and of their magnitudes"""
    H = len(g)
    F = l.shape[1] // H
    t = np.repeat(np.asarray(g, np.float64).T, F, axis=1) * l.astype(np.float64)
    return t.sum(0).reshape(H, F), np.abs(t).sum(0).reshape(H, F)


def gatv2_sequential_f32(rp, col, xl, xr, attn, slope, dp):
    """The whole operator as the contract states it, with every sum taken LEFT TO RIGHT (the kernels use trees and lane-strided
    partial sums): dict(score, p, g, d_xr, d_xl, d_attn, z, l, c).  fp32 where the contract rounds to fp32, fp64 sums rounded once."""
    n, E = len(rp) - 1, int(np.asarray(rp)[-1])
    H, F = attn.shape
    rows, cols = _edge_rows(rp), np.asarray(col[:E], dtype=np.int64)
    z = z_f32(rp, col, xl, xr)
    l, c = act_f32(z, slope), slope_factor_f32(z, attn, slope)
    prod = l.astype(np.float64).reshape(E, H, F) * np.asarray(attn, dtype=np.float64)[None]
    score = np.ascontiguousarray(np.cumsum(prod, axis=2)[:, :, -1].T.astype(np.float32)) if E else np.zeros((H, 0), np.float32)
    p = np.stack([R.softmax_f32_sum64(rp, score[h], 1.0) for h in range(H)]) if E else np.zeros((H, 0), np.float32)
    g = np.zeros((H, E), np.float32)
    rp64 = np.asarray(rp, dtype=np.int64)
    for h in range(H):
        pd = p[h].astype(np.float64) * dp[h].astype(np.float64)
        dot = np.zeros(n)
        for i in np.nonzero(np.diff(rp64) > 0)[0]:
            dot[i] = np.cumsum(pd[rp64[i]:rp64[i + 1]])[-1]
        g[h] = p[h] * (dp[h].astype(np.float64) - dot[rows]).astype(np.float32)
    terms = node_terms(g, c)

    def seq(seg):
        out = np.zeros((n, H * F), np.float32)
        order = np.argsort(seg, kind="stable")
        cnt = np.bincount(seg, minlength=n)[:n]
        ptr = np.concatenate([[0], np.cumsum(cnt)])
        t = terms[order].astype(np.float64)
        for i in np.nonzero(cnt > 0)[0]:
            out[i] = np.cumsum(t[ptr[i]:ptr[i + 1]], axis=0)[-1].astype(np.float32)
        return out
    d_attn = np.cumsum(np.repeat(g.astype(np.float64).T, F, axis=1) * l.astype(np.float64), axis=0)[-1].astype(np.float32).reshape(H, F) if E \
        else np.zeros((H, F), np.float32)
    return dict(score=score, p=p, g=g, d_xr=seq(rows), d_xl=seq(cols), d_attn=d_attn, z=z, l=l, c=c)


def shares_of_all_bounds(rp, col, attn, dp, out, z=None, l=None, c=None):
    """(whole, excess): two {name: share} of every bound for the outputs `out` (score, p, g, d_xr, d_xl, d_attn) of one call on (rp, col).
    Every entry of whole must be <= 1 for the bounds to hold; excess has the four rounded sums (score, d_xr, d_xl, d_attn) by what they
    need beyond their own rounding (score_share, own_sum_share) and the others as in whole.  z, l, c: the activation terms if the caller
    has them already (else out must carry them)."""
    n, E = len(rp) - 1, int(np.asarray(rp)[-1])
    H, F = attn.shape
    z = out["z"] if z is None else z
    l = out["l"] if l is None else l
    c = out["c"] if c is None else c
    rows, cols = _edge_rows(rp), np.asarray(col[:E], dtype=np.int64)
    rel, abs_, rs = softmax_shares(rp, out["p"], out["score"]) if E else (0.0, 0.0, 0.0)
    same = {"p relative": rel, "p absolute": abs_, "p row sum": rs,
            "g": (g_worst(rp, col, out["p"], dp, out["g"]) / G.C_GAT_BWD) if E else 0.0}
    terms = node_terms(out["g"], c)
    pairs = {"score": score_share(out["score"], *scores_f64(l, attn), F),
             "d_xr": own_sum_share(out["d_xr"], *segment_sums(terms, rows, n), G.OWN_SUM),
             "d_xl": own_sum_share(out["d_xl"], *segment_sums(terms, cols, n), G.OWN_SUM),
             "d_attn": own_sum_share(out["d_attn"], *attn_terms(out["g"], l), D_ATTN_SUM)}
    return dict(same, **{k: v[0] for k, v in pairs.items()}), dict(same, **{k: v[1] for k, v in pairs.items()})


FORWARD_KEYS = ("score", "p relative", "p absolute", "p row sum")


# ---- the dense fp64 model ------------------------------------------------------------------------------------------------------------------

def gpu_layer_case(name, concat, share_weights=False):
    """The inputs of tests/test_gpu_gatv2.py's layer test, as fp64 leaves: (rp, col, X, Wl, Wr or None, attn, bias, dY)"""
    import torch
    rp, col = G.golden_graph() if name == "layers_n200" else powerlaw()
    n, H, Fo, Fi = len(rp) - 1, LAYER_CASE["heads"], LAYER_CASE["out"], LAYER_CASE["inp"]
    g = torch.Generator().manual_seed(LAYER_CASE["seed"])
    rnd = lambda *shape: torch.randn(*shape, dtype=torch.float64, generator=g)   # noqa: E731
    X, Wl, Wr = rnd(n, Fi), rnd(Fi, H * Fo) * (2.0 / (Fi + H * Fo)) ** 0.5, rnd(Fi, H * Fo) * (2.0 / (Fi + H * Fo)) ** 0.5
    attn, b = rnd(1, H, Fo) * 0.5, rnd(H * Fo if concat else Fo) * 0.1
    dY = rnd(n, H * Fo if concat else Fo)
    return rp, col, X, Wl, (None if share_weights else Wr), attn, b, dY


def dense_gatv2_attention(A, xl, xr, attn, negative_slope=0.2):
    """P [H, n, n] on a dense 0/1 adjacency A (rows = destination nodes): softmax over each row's edges of
    <attn_h, leaky_relu(xl_h[j] + xr_h[i])>; zero off the edges, rows without edges all zero.  Differentiable."""
    import torch
    import torch.nn.functional as F
    n, H, Fh = A.shape[0], attn.shape[0], attn.shape[1]
    none = A.sum(1, keepdim=True) == 0
    out = []
    for h in range(H):
        zl, zr = xl[:, h * Fh:(h + 1) * Fh], xr[:, h * Fh:(h + 1) * Fh]
        S = (F.leaky_relu(zl.unsqueeze(0) + zr.unsqueeze(1), negative_slope) * attn[h]).sum(-1)      # [dst, src]
        S = S.masked_fill(A == 0, float("-inf")).masked_fill(none, 0.0)
        P = torch.softmax(S, dim=1)
        out.append(torch.where(A != 0, P, torch.zeros_like(P)))
    return torch.stack(out)


def dense_gatv2_model(A, X, Wl, Wr, attn, bias, heads, negative_slope=0.2, concat=True, round_operands=False):
    """GATv2Conv on a dense adjacency matrix in torch, differentiable: Zl = X Wl, Zr = X Wr (Wr None: Zr is Zl), P from
    dense_gatv2_attention with attn [1, H, F], Y_h = P_h Zl_h, heads concatenated or averaged, plus bias.  round_operands: the
    aggregation's operands rounded as the kernels round them (gat_ref.dense_gat_model says how)."""
    import torch
    n = A.shape[0]
    Zl = X @ Wl
    Zr = Zl if Wr is None else X @ Wr
    Fh = Zl.shape[1] // heads
    P = dense_gatv2_attention(A, Zl, Zr, attn.reshape(heads, Fh), negative_slope)
    Zh = Zl.view(n, heads, Fh)
    Zagg = Zh + (G._round_tf32_t(Zh) - Zh).detach() if round_operands else Zh
    outs = []
    for h in range(heads):
        Yh = P[h] @ Zagg[:, h]
        outs.append(G._make_round_grad().apply(Yh) if round_operands else Yh)
    Y = torch.cat(outs, dim=1) if concat else torch.stack(outs, dim=1).mean(1)
    return Y + bias if bias is not None else Y


# ---- a pure-torch backend ----------------------------------------------------------------------------------------------------------------------

class TorchBackend(G.TorchBackend):
    """gat_ref.TorchBackend with the three GATv2 calls, composed of torch index operations, any dtype"""

    def _act(self, xl, xr, attn, rp, col, slope):
        import torch
        z = xl[col.long()] + xr[self._rows(rp)]                          # [E, H F]
        H, F = attn.shape
        return z, torch.nn.functional.leaky_relu(z, slope).view(-1, H, F)

    def gatv2_softmax(self, xl, xr, attn, rp, col, negative_slope=0.2, out=None, score_out=None):
        import torch
        _, l = self._act(xl, xr, attn, rp, col, negative_slope)
        s = (l * attn.unsqueeze(0)).sum(-1).t()                           # [H, E]
        return torch.stack([self.edge_softmax(s[h], rp) for h in range(s.shape[0])])

    def gatv2_softmax_backward(self, p, dp, xl, xr, attn, rp, col, negative_slope=0.2, out=None):
        import torch
        z, l = self._act(xl, xr, attn, rp, col, negative_slope)
        H, F = attn.shape
        g = torch.stack([self.edge_softmax_backward(p[h], dp[h], rp)[0] for h in range(H)])
        c = torch.where(z.view(-1, H, F) > 0, attn.unsqueeze(0), attn.unsqueeze(0) * negative_slope)
        terms = (g.t().unsqueeze(-1) * c).reshape(-1, H * F)
        d_xr = torch.zeros_like(xr).index_add_(0, self._rows(rp), terms)
        return g, d_xr, (g.t().unsqueeze(-1) * l).sum(0)

    def gatv2_source_grad(self, g, xl, xr, attn, rp, col, negative_slope=0.2):
        import torch
        z, _ = self._act(xl, xr, attn, rp, col, negative_slope)
        H, F = attn.shape
        c = torch.where(z.view(-1, H, F) > 0, attn.unsqueeze(0), attn.unsqueeze(0) * negative_slope)
        return torch.zeros_like(xl).index_add_(0, col.long(), (g.t().unsqueeze(-1) * c).reshape(-1, H * F))
