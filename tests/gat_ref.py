"""Restatements, in numpy and torch, of multi-head GAT attention (tcgnn_gat_softmax / _backward / tcgnn_edge_colsum, the operators
gat_attention / aggregate_heads and the layer GATConv), the constants of the backward bounds and the input sets.  Shared by
tests/test_gat_cpu.py and tests/test_gpu_gat.py; no GPU needed to import.

Forward.  The kernel forms s[h,e] = lrelu(fl32(el[col e, h] + er[row e, h])), lrelu(x) = x > 0 ? x : fl32(x slope) - two fp32
roundings, gat_scores_f32 - and takes the softmax of THAT number over each row: the reference is edge_ops_ref.softmax_f64 of s32 with
beta = 1 and the bounds are edge_ops_ref's REL / ABS / ROW_SUM unchanged.

Backward, relative to the scale of its own terms (g = p (dp - sum_row p dp), ds = g lrelu'(raw)):
    |ds - ds64|     <= C_GAT_BWD p64 (|dp| + sum_row p64 |dp|) + 2^-125                       (edge_ops_ref.BWD_FLOOR)
    |d_er - d_er64| <= C_GAT_SUM sum_{e in row} |ds64| + 2^-24 |d_er64|,  d_el alike over the edges of a source node
(the 2^-24: the result's own rounding to fp32).  Each constant is 4 x the worst that gat_bwd_f32 - this file's fp32 restatement with
SEQUENTIAL sums - needs against gat_bwd_f64 on the test inputs (the row-class graph, the five el / er sets, eight heads, slope in
{0.2, 0, 1}, standard-normal dp, p = softmax_f32_sum64 of the scores); 4 is C_BWD's margin, for the same reason: another summation
order may be that much worse.  tests/test_gat_cpu.py measures the restatement, prints the worst and asserts the constants are at
least 4 x it.  Measured worst: 7.33e-7 for ds (a sequential fp32 dot product over a row of 300 000 edges), 1.003 for d_er and 1.000 for
d_el, so C_GAT_BWD = 3e-6 and C_GAT_SUM = 4.1.
C_GAT_SUM says little: measured this way the sum bound is nearly empty.  The restatement's ds carries an error that follows
`scale`, not |ds| - its dot product is an fp32 sum - and in a row that one edge dominates (p close to 1, dp - dot cancelling) the
terms of the sum are far smaller than their scale, so the restatement's sums miss sum |ds64| by about all of it.  The kernels form
dp - dot in fp64 and do not share that loss; what pins THEIR sums is the derived check beside it (sum_of_own_terms_worst): d_er and
d_el are fp64 sums of the fp32 ds the same call wrote, rounded once, so against the fp64 sum of those very numbers they may differ
by 2^-24 of the result (the rounding; 2^-149 where the result is subnormal) plus 2^-40 of sum |ds| (fp64 adds of up to 2^13 terms per lane, far below it) - nothing else.
On the MI355X (tests/test_gpu_gat.py, all 86 kernel cases; profiles/r10/gpu_gat_tests_figures.txt) the kernels need 1.17e-7 for ds, 1.4e-2 / 2.6e-5 of sum |ds64| for d_er /
d_el (rows in which one edge holds all but ~1e-14 of the probability: there fp64's own rounding of sum p dp, in the kernel and in
this reference alike, is a percent of the dominant edge's dp - dot) and 6.6e-16 / 0 of their own terms.
"""
import os

import numpy as np

import edge_ops_ref as R
import graphs
import walks

C_GAT_BWD = 3e-6
C_GAT_SUM = 4.1
OWN_SUM = 2.0 ** -40   # fp64 accumulation of a segment's fp32 terms, relative to sum |term|

GPU_LAYER_TOL = 2e-3      # tests/test_gpu_gat.py: values and gradients of the operators and the layer, of the largest entry
LAYER_CASE = dict(heads=3, out=8, inp=24, seed=3)   # the layer that test runs
HEADS = (1, 3, 4, 8)   # (4: not among the issue's head counts - the width of the long rows' head chunk and of a 16-byte el / er row,
                       #  and what the benchmark and the harness run)
SLOPES = (0.2, 0.0, 1.0)
SETS = ("normal_x1", "normal_x8", "normal_x30", "constant", "magnitude_1e4")
MAX_HEADS = max(HEADS)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

def row_class_graph(seed=13):
    """(rowptr, col) of edge_ops_ref's row-class graph with seeded random column ids in [0, N) (duplicates welcome)"""
    rp = R.row_class_rowptr()
    n, E = len(rp) - 1, int(rp[-1])
    return rp, np.random.default_rng(seed).integers(0, n, E).astype(np.int32)


def el_er_sets(n, seed=17):
    """{name: (el, er)}, fp32 [n, MAX_HEADS] each; a test with H heads takes the first H columns (head h's scores do not depend on H).
    normal x {1, 8, 30}; constant: el the same for every node of a head (a row's scores are all equal); magnitude 1e4: sums near
    +-2e4 and, where the signs differ, differences of a few hundred."""
    rng = np.random.default_rng(seed)
    zl, zr = rng.standard_normal((n, MAX_HEADS)).astype(np.float32), rng.standard_normal((n, MAX_HEADS)).astype(np.float32)
    out = {"normal_x1": (zl, zr), "normal_x8": ((8 * zl).astype(np.float32), (8 * zr).astype(np.float32)),
           "normal_x30": ((30 * zl).astype(np.float32), (30 * zr).astype(np.float32))}
    out["constant"] = (np.repeat(rng.standard_normal((1, MAX_HEADS)).astype(np.float32), n, axis=0), zr.copy())
    big = lambda z: (1e4 * np.sign(z) * (1 + 0.01 * np.abs(z))).astype(np.float32)   # noqa: E731
    out["magnitude_1e4"] = (big(zl), big(zr))
    return {k: (np.ascontiguousarray(a), np.ascontiguousarray(b)) for k, (a, b) in out.items()}


def golden_graph():
    f = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layers_n200.npz"))
    return f["rowptr"], f["col"]


def gpu_layer_case(name, concat):
    """The inputs of tests/test_gpu_gat.py's layer test, as fp64 leaves: (rp, col, X, W, attn_l, attn_r, bias, dY)"""
    rp, col = golden_graph() if name == "layers_n200" else graphs.powerlaw_graph(3000, 12, seed=31, symmetric=False)
    import torch
    n, H, Fo, Fi = len(rp) - 1, LAYER_CASE["heads"], LAYER_CASE["out"], LAYER_CASE["inp"]
    g = torch.Generator().manual_seed(LAYER_CASE["seed"])
    rnd = lambda *shape: torch.randn(*shape, dtype=torch.float64, generator=g)   # noqa: E731
    X, W = rnd(n, Fi), rnd(Fi, H * Fo) * (2.0 / (Fi + H * Fo)) ** 0.5
    al, ar, b = rnd(1, H, Fo) * 0.5, rnd(1, H, Fo) * 0.5, rnd(H * Fo if concat else Fo) * 0.1
    dY = rnd(n, H * Fo if concat else Fo)
    return rp, col, X, W, al, ar, b, dY


# ---- numpy restatements ------------------------------------------------------------------------------------------------------------------

def _edge_rows(rp):
    rp = np.asarray(rp, dtype=np.int64)
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


def gat_raw_f32(rp, col, el, er):
    """raw[h, e] = fl32(el[col e, h] + er[row e, h]) for the edges rows cover, fp32 [H, E]"""
    E = int(np.asarray(rp)[-1])
    rows, col = _edge_rows(rp), np.asarray(col[:E], dtype=np.int64)
    return np.ascontiguousarray((np.asarray(el, np.float32)[col] + np.asarray(er, np.float32)[rows]).T)


def gat_scores_f32(rp, col, el, er, slope):
    """s32[h, e] with exactly the kernel's two fp32 roundings: the sum, then the product with the slope where the sum is not positive"""
    raw = gat_raw_f32(rp, col, el, er)
    return np.where(raw > 0, raw, raw * np.float32(slope)).astype(np.float32)


def gat_bwd_f64(rp, col, el, er, slope, p, dp):
    """dict(ds, scale, d_er, d_er_scale, d_el, d_el_scale) in fp64 from fp32 p, dp [H, E]: scale = p (|dp| + sum_row p |dp|), the sums'
    scales = sum |ds64| over the segment.  ds / scale are [H, E], the node arrays [N, H]."""
    n, E = len(rp) - 1, int(np.asarray(rp)[-1])
    rows, cols = _edge_rows(rp), np.asarray(col[:E], dtype=np.int64)
    raw = gat_raw_f32(rp, col, el, er)
    k = np.float64(np.float32(slope))
    H = raw.shape[0]
    out = {key: np.zeros((H, E)) for key in ("ds", "scale")}
    out.update({key: np.zeros((n, H)) for key in ("d_er", "d_er_scale", "d_el", "d_el_scale")})
    for h in range(H):
        ph, dh = np.asarray(p[h][:E], dtype=np.float64), np.asarray(dp[h][:E], dtype=np.float64)
        dot = np.bincount(rows, weights=ph * dh, minlength=n)
        ds = ph * (dh - dot[rows]) * np.where(raw[h] > 0, 1.0, k)
        out["ds"][h] = ds
        out["scale"][h] = ph * (np.abs(dh) + np.bincount(rows, weights=ph * np.abs(dh), minlength=n)[rows])
        out["d_er"][:, h] = np.bincount(rows, weights=ds, minlength=n)
        out["d_er_scale"][:, h] = np.bincount(rows, weights=np.abs(ds), minlength=n)
        out["d_el"][:, h] = np.bincount(cols, weights=ds, minlength=n)[:n]
        out["d_el_scale"][:, h] = np.bincount(cols, weights=np.abs(ds), minlength=n)[:n]
    return out


def _sequential_sums(values, ptr):
    """fp32 sums of the segments ptr[i] .. ptr[i + 1] of an fp32 array, each added left to right"""
    out = np.zeros(len(ptr) - 1, dtype=np.float32)
    for i in np.nonzero(np.diff(ptr) > 0)[0]:
        out[i] = np.cumsum(values[ptr[i]:ptr[i + 1]], dtype=np.float32)[-1]
    return out


def gat_bwd_f32(rp, col, el, er, slope, p, dp):
    """(ds, d_er, d_el) all in fp32 with sequential sums: the row's dot product, the row sums of ds and the per-source-node sums of ds
    (the edges of a node in CSR order, as the transposed CSR lists them)"""
    n, E = len(rp) - 1, int(np.asarray(rp)[-1])
    rp64 = np.asarray(rp, dtype=np.int64)
    rows, cols = _edge_rows(rp), np.asarray(col[:E], dtype=np.int64)
    raw = gat_raw_f32(rp, col, el, er)
    k = np.float32(slope)
    H = raw.shape[0]
    order = np.argsort(cols, kind="stable")
    ptr_t = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int64)
    ds, d_er, d_el = np.zeros((H, E), np.float32), np.zeros((n, H), np.float32), np.zeros((n, H), np.float32)
    for h in range(H):
        ph, dh = np.asarray(p[h][:E], dtype=np.float32), np.asarray(dp[h][:E], dtype=np.float32)
        dot = _sequential_sums(ph * dh, rp64)
        g = ph * (dh - dot[rows])
        ds[h] = np.where(raw[h] > 0, g, g * k)
        d_er[:, h] = _sequential_sums(ds[h], rp64)
        d_el[:, h] = _sequential_sums(ds[h][order], ptr_t)[:n]
    return ds, d_er, d_el


def sum_worst(got, want, scale):
    """worst (|got - want| - 2^-24 |want|) / scale over the segments with a positive scale: the constant a row / column sum needs"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.maximum(np.abs(got - want) - 2.0 ** -24 * np.abs(want), 0.0)
    ok = scale > 0
    assert np.all(got[~ok] == 0), "a segment without terms must sum to exactly 0"
    return float((err[ok] / scale[ok]).max()) if ok.any() else 0.0


def sum_of_own_terms_worst(got, terms, seg, n):
    """worst (|got - S| - 2^-24 |S|) / sum |term| with S the fp64 sum of the fp32 `terms` [H, E] over the segments seg[e] (a row or a
    source node per edge): what a sum needs beyond its own rounding against the numbers it was formed from; got is [n, H].  (The 2^-149:
    a result below fp32's normal range is rounded to that grid, not to 24 bits.)"""
    worst = 0.0
    for h in range(len(terms)):
        t = np.asarray(terms[h], dtype=np.float64)
        S, A = np.bincount(seg, weights=t, minlength=n)[:n], np.bincount(seg, weights=np.abs(t), minlength=n)[:n]
        err = np.maximum(np.abs(np.asarray(got[:, h], dtype=np.float64) - S) - 2.0 ** -24 * np.abs(S) - 2.0 ** -149, 0.0)
        ok = A > 0
        if not np.all(np.asarray(got[:, h])[~ok] == 0):
            return float("inf")
        if ok.any():
            worst = max(worst, float((err[ok] / A[ok]).max()))
    return worst


def ds_worst(rp, ds, ref):
    """worst |ds - ds64| / scale (minus the floor) over all heads: the constant ds needs (edge_ops_ref.bwd_worst per head)"""
    return max(R.bwd_worst(rp, ds[h], ref["ds"][h], ref["scale"][h]) for h in range(len(ds)))


# ---- the dense fp64 model ------------------------------------------------------------------------------------------------------------------

def _round_tf32_t(t):
    import torch
    return torch.from_numpy(walks.round_tf32(t.detach().to(torch.float32).numpy()).astype(np.float64)).reshape(t.shape)


def _make_round_grad():
    import torch

    class RoundGrad(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            return _round_tf32_t(g)
    return RoundGrad


def dense_gat_model(A, X, W, attn_l, attn_r, bias, heads, negative_slope=0.2, concat=True, round_operands=False):
    """GATConv on a dense 0/1 adjacency matrix A [n, n] (rows = destination nodes) in torch, differentiable: Z = X W, el / er the
    per-head products with attn_l / attn_r [1, H, F], S_h[i, j] = lrelu(el[j, h] + er[i, h]) on the edges, softmax over each row's
    edges, Y_h = P_h Z_h, heads concatenated or averaged, plus bias.  Rows without edges give the bias only.
    round_operands: the aggregation's operands as the kernels round them - Z where it is aggregated (and where dP is formed) and dY
    where it is aggregated back - to 10 mantissa bits (walks.round_tf32); the gradients then are those of the rounded computation."""
    import torch
    import torch.nn.functional as F
    n = A.shape[0]
    Z = X @ W
    Fh = Z.shape[1] // heads
    Zh = Z.view(n, heads, Fh)
    el, er = (Zh * attn_l).sum(-1), (Zh * attn_r).sum(-1)
    Zagg = Zh + (_round_tf32_t(Zh) - Zh).detach() if round_operands else Zh
    none = A.sum(1, keepdim=True) == 0
    outs = []
    for h in range(heads):
        S = F.leaky_relu(el[:, h].unsqueeze(0) + er[:, h].unsqueeze(1), negative_slope)
        S = S.masked_fill(A == 0, float("-inf")).masked_fill(none, 0.0)
        P = torch.softmax(S, dim=1)
        P = torch.where(A != 0, P, torch.zeros_like(P))
        Yh = P @ Zagg[:, h]
        outs.append(_make_round_grad().apply(Yh) if round_operands else Yh)
    Y = torch.cat(outs, dim=1) if concat else torch.stack(outs, dim=1).mean(1)
    return Y + bias if bias is not None else Y


def dense_adjacency(rp, col):
    import torch
    n = len(rp) - 1
    A = torch.zeros(n, n, dtype=torch.float64)
    A[torch.from_numpy(_edge_rows(rp)).long(), torch.from_numpy(np.asarray(col)).long()] = 1.0
    return A


# ---- a pure-torch backend ----------------------------------------------------------------------------------------------------------------------

class TorchBackend:
    """The operators tcgnn_edge_ops asks the backend for, composed of torch index operations, any dtype: forward_ef2, edge_softmax,
    edge_softmax_backward, forward_AGNN(transpose=), and gat_softmax / gat_softmax_backward / edge_colsum."""

    def _rows(self, rp):
        import torch
        rp = rp.long()
        return torch.repeat_interleave(torch.arange(rp.numel() - 1), rp[1:] - rp[:-1])

    def forward_ef2(self, X, Z, rp, col, *rest):
        return [(X[self._rows(rp)] * Z[col.long()]).sum(1)]

    def forward_AGNN(self, X, rp, col, att, *rest, transpose=False):
        import torch
        rows, cols = self._rows(rp), col.long()
        src, dst = (rows, cols) if transpose else (cols, rows)
        return [torch.zeros_like(X).index_add_(0, dst, att[0].unsqueeze(1) * X[src])]

    def edge_softmax(self, s, rp, beta=None):
        import torch
        rows, n = self._rows(rp), rp.numel() - 1
        x = s if beta is None else beta.reshape(()) * s
        m = torch.full((n,), -float("inf"), dtype=s.dtype).scatter_reduce(0, rows, x, "amax")
        ex = torch.exp(x - m[rows])
        return ex / torch.zeros(n, dtype=s.dtype).index_add_(0, rows, ex)[rows]

    def edge_softmax_backward(self, p, dp, rp, beta=None, score=None, need_dbeta=False, out=None):
        import torch
        rows, n = self._rows(rp), rp.numel() - 1
        g = p * (dp - torch.zeros(n, dtype=p.dtype).index_add_(0, rows, p * dp)[rows])
        return (g if beta is None else beta.reshape(()) * g), ((score * g).sum().reshape(1) if need_dbeta else None)

    def _raw(self, el, er, rp, col):
        return (el[col.long()] + er[self._rows(rp)]).t()          # [H, E]

    def gat_softmax(self, el, er, rp, col, negative_slope=0.2, out=None):
        import torch
        s = torch.nn.functional.leaky_relu(self._raw(el, er, rp, col), negative_slope)
        return torch.stack([self.edge_softmax(s[h], rp) for h in range(s.shape[0])])

    def gat_softmax_backward(self, p, dp, el, er, rp, col, negative_slope=0.2, out=None):
        import torch
        raw = self._raw(el, er, rp, col)
        g = torch.stack([self.edge_softmax_backward(p[h], dp[h], rp)[0] for h in range(p.shape[0])])
        ds = torch.where(raw > 0, g, g * negative_slope)
        d_er = torch.zeros_like(er).index_add_(0, self._rows(rp), ds.t())
        return ds, d_er

    def edge_colsum(self, val, rp, col):
        import torch
        return torch.zeros(rp.numel() - 1, val.shape[0], dtype=val.dtype).index_add_(0, col.long(), val.t())
