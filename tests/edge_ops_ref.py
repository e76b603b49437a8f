"""Restatements, in numpy, of the edge operators (edge softmax forward / backward, the two-operand SDDMM), the bounds the kernels are
held to and the graph with a row of every length class.  Shared by tests/test_edge_ops_cpu.py and tests/test_gpu_edge_ops.py; no
GPU needed to import.

The softmax bound is derived, not measured: the subtraction b s - m and the multiply by log2(e) each round a number of magnitude
|b s - m| (2^-24 relative each, which the exponential turns into a relative error of that size times |b s - m|), the exponential
itself is good to about 1 ulp, a tree sum of n terms to about log2 n ulps relative to the sum, and the divide rounds once:
    |p - p64| <= 2^-21 (4 + |b s_e - m_r|) p64        for entries with p64 >= 1e-30,      |p - p64| <= 1e-7 everywhere,
    |sum_row p - 1| <= 1e-6.
The backward bound is relative to the scale of its own terms, g = p (dp - sum_row p dp):
    |ds - ds64| <= C_BWD |b| p64 (|dp| + sum_row p64 |dp|) + 2^-125,
(the floor: a result below fp32's normal range carries no relative precision - a p of 1e-40 times anything underflows)
C_BWD = 4 x the worst value of softmax_bwd_f32 - this file's fp32 restatement - on the test inputs (another summation order may be
that much worse; test_edge_ops_cpu.py measures the restatement and asserts it uses at most a quarter).  Measured worst: 2.17e-7 for ds
and 2.12e-7 for dbeta (relative to sum |s| |g|) on the row-class graph with its five score sets, beta in {1, 0.37, -1.3} and
standard-normal dp, so C_BWD = 9e-7 for both.
"""
import numpy as np

import walks

REL = 2.0 ** -21
ABS = 1e-7
ROW_SUM = 1e-6
P_FLOOR = 1e-30
C_BWD = 9e-7
BWD_FLOOR = 2.0 ** -125

ROW_LENGTHS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4096, 65535, 65536, 300000)
EMPTY_EDGE = 40   # empty rows at the head and at the tail


def row_class_rowptr(seed=7):
    """Row pointers of a graph with a row of every length class: ROW_LENGTHS in that order, then again shuffled, with EMPTY_EDGE empty
    rows in front and behind."""
    rng = np.random.default_rng(seed)
    lens = np.concatenate([np.zeros(EMPTY_EDGE, np.int64), np.array(ROW_LENGTHS), rng.permutation(np.array(ROW_LENGTHS)), np.zeros(EMPTY_EDGE, np.int64)])
    rp = np.zeros(len(lens) + 1, dtype=np.int64)
    rp[1:] = np.cumsum(lens)
    return rp.astype(np.int32)


def score_sets(rp, seed=11):
    """{name: fp32 scores}: standard normal x {1, 8, 30}, constant rows, magnitude 1e4."""
    E, n = int(rp[-1]), len(rp) - 1
    rng = np.random.default_rng(seed)
    z = rng.standard_normal(E).astype(np.float32)
    out = {"normal_x1": z, "normal_x8": (8 * z).astype(np.float32), "normal_x30": (30 * z).astype(np.float32)}
    out["constant_rows"] = np.repeat(rng.standard_normal(n).astype(np.float32), np.diff(rp))
    out["magnitude_1e4"] = (1e4 * np.sign(z) * (1 + 0.01 * np.abs(z))).astype(np.float32)
    return out


def _rows(rp):
    rp = np.asarray(rp, dtype=np.int64)
    return [(int(rp[r]), int(rp[r + 1])) for r in np.nonzero(np.diff(rp) > 0)[0]]


def softmax_f64(rp, s, beta=1.0):
    """(p64, dist) with dist[e] = |b s_e - m_r|; positions no row covers stay nan"""
    x = np.float64(np.float32(beta)) * np.asarray(s, dtype=np.float64)
    p = np.full(len(x), np.nan)
    dist = np.zeros(len(x))
    for lo, hi in _rows(rp):
        d = x[lo:hi] - x[lo:hi].max()
        ex = np.exp(d)
        p[lo:hi] = ex / ex.sum()
        dist[lo:hi] = -d
    return p, dist


def softmax_f32(rp, s, beta=1.0):
    """fp32 all the way: the exponent rounded once (the kernels form it with one fma), fp32 exp, fp32 pairwise sums, one divide"""
    x = np.float64(np.float32(beta)) * np.asarray(s, dtype=np.float64)   # (24 x 24 bits: exact in fp64)
    p = np.full(len(x), np.nan, dtype=np.float32)
    for lo, hi in _rows(rp):
        m = np.float32(x[lo:hi].max())
        ex = np.exp((x[lo:hi] - np.float64(m)).astype(np.float32))
        p[lo:hi] = ex / ex.sum(dtype=np.float32)
    return p


def softmax_f32_sum64(rp, s, beta=1.0):
    """what the kernels do: the exponent rounded once to fp32, the multiply by log2(e) and exp2 in fp32, the row sum and the
    quotient in fp64, one rounding of p to fp32"""
    x = np.float64(np.float32(beta)) * np.asarray(s, dtype=np.float64)
    p = np.full(len(x), np.nan, dtype=np.float32)
    log2e = np.float32(1.4426950408889634)
    for lo, hi in _rows(rp):
        m = np.float32(x[lo:hi].max())
        ex = np.exp2((x[lo:hi] - np.float64(m)).astype(np.float32) * log2e).astype(np.float32)
        p[lo:hi] = (ex.astype(np.float64) / ex.astype(np.float64).sum()).astype(np.float32)
    return p


def softmax_bounds_hold(rp, p, p64, dist):
    """worst ratios (relative, absolute, row sum) of p against the three bounds; each must be <= 1"""
    p = np.asarray(p, dtype=np.float64)
    rel = abs_ = rs = 0.0
    for lo, hi in _rows(rp):
        err = np.abs(p[lo:hi] - p64[lo:hi])
        big = p64[lo:hi] >= P_FLOOR
        if big.any():
            rel = max(rel, float((err[big] / (REL * (4 + dist[lo:hi][big]) * p64[lo:hi][big])).max()))
        abs_ = max(abs_, float(err.max()) / ABS)
        rs = max(rs, abs(float(p[lo:hi].sum()) - 1.0) / ROW_SUM)
    return rel, abs_, rs


def softmax_bwd_f64(rp, p, dp, s=None, beta=1.0):
    """(ds64, scale, dbeta64, dbeta_scale): scale[e] = |b| p (|dp| + sum_row p |dp|), dbeta_scale = sum |s| |g|"""
    b = np.float64(np.float32(beta))
    p, dp = np.asarray(p, dtype=np.float64), np.asarray(dp, dtype=np.float64)
    ds, scale = np.full(len(p), np.nan), np.zeros(len(p))
    dbeta = dscale = 0.0
    for lo, hi in _rows(rp):
        pr, dr = p[lo:hi], dp[lo:hi]
        g = pr * (dr - (pr * dr).sum())
        ds[lo:hi] = b * g
        scale[lo:hi] = abs(b) * pr * (np.abs(dr) + (pr * np.abs(dr)).sum())
        if s is not None:
            sr = np.asarray(s[lo:hi], dtype=np.float64)
            dbeta += float((sr * g).sum()); dscale += float((np.abs(sr) * np.abs(g)).sum())
    return ds, scale, dbeta, dscale


def softmax_bwd_f32(rp, p, dp, s=None, beta=1.0):
    """fp32 products and fp32 pairwise row sums; dbeta's fp32 terms are added in fp64 (the kernels keep fp64 partials)"""
    b = np.float32(beta)
    p, dp = np.asarray(p, dtype=np.float32), np.asarray(dp, dtype=np.float32)
    ds = np.full(len(p), np.nan, dtype=np.float32)
    dbeta = 0.0
    for lo, hi in _rows(rp):
        pr, dr = p[lo:hi], dp[lo:hi]
        g = pr * (dr - (pr * dr).sum(dtype=np.float32))
        ds[lo:hi] = b * g
        if s is not None:
            dbeta += float((np.asarray(s[lo:hi], dtype=np.float32) * g).astype(np.float64).sum())
    return ds, np.float32(dbeta)


def bwd_worst(rp, ds, ds64, scale):
    """worst |ds - ds64| / scale over the entries rows cover (the constant c of the backward bound that ds needs)"""
    worst = 0.0
    for lo, hi in _rows(rp):
        sc = scale[lo:hi]
        ok = sc > 0
        if ok.any():
            err = np.maximum(np.abs(np.asarray(ds[lo:hi], dtype=np.float64) - ds64[lo:hi]) - BWD_FLOOR, 0.0)
            worst = max(worst, float((err[ok] / sc[ok]).max()))
    return worst


def _edge_rows(rp):
    rp = np.asarray(rp, dtype=np.int64)
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


def sddmm2_f64(X, Z, rp, col, chunk=1 << 18):
    """(ef64, scale) with ef[e] = <X[row e], Z[col e]> in fp64 and scale[e] = sum_k |x||z|"""
    rows, col = _edge_rows(rp), np.asarray(col, dtype=np.int64)
    X, Z = np.asarray(X, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    ef, sc = np.empty(len(col)), np.empty(len(col))
    for a in range(0, len(col), chunk):
        xr, zc = X[rows[a:a + chunk]], Z[col[a:a + chunk]]
        ef[a:a + chunk] = (xr * zc).sum(1)
        sc[a:a + chunk] = (np.abs(xr) * np.abs(zc)).sum(1)
    return ef, sc


def sddmm2_tf32(X, Z, rp, col):
    """the contract's operand rounding (10-bit mantissa, ties away: walks.round_tf32) on both operands, fp64 dots"""
    return sddmm2_f64(walks.round_tf32(X), walks.round_tf32(Z), rp, col)


def dense_attention_model(A, X, W, beta):
    """The softmax-AGNN layer on a dense 0/1 adjacency matrix A [n, n] (rows = destination nodes) in torch, differentiable:
    H = X W, cosine scores, softmax over each row's edges, Y = P H.  Rows without edges give zero rows."""
    import torch
    H = X @ W
    Hn = H / H.norm(dim=1, keepdim=True).clamp_min(1e-12)
    S = beta.reshape(()) * (Hn @ Hn.t())
    S = S.masked_fill(A == 0, float("-inf")).masked_fill(A.sum(1, keepdim=True) == 0, 0.0)
    P = torch.softmax(S, dim=1)
    P = torch.where(A != 0, P, torch.zeros_like(P))
    return P @ H
