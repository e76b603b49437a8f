"""Restatements for the one-gather aggregation (tcgnn_segment_stats / _backward) and the PNA layer, numpy (and dense torch for the
layer): what tests/test_segstats_cpu.py checks against a brute-force comparator and tests/test_gpu_segstats.py holds the kernels to.

Extrema: max / argmax are segmax_ref.segment_max's; min / argmin are the mirror image, numpy.argmin over the row's slice - the smaller
value wins, among equal values (-0.0 == +0.0) the first position, a NaN beats every number and the first NaN wins.  Values are copies
of the winner (its bits).  Moments: fp64 two-pass mean and population variance, std = sqrt(max(var, 0) + eps).  A row without edges:
0 in all four values, -1 in both args.

Bounds for an fp32 result formed from fp64 sums of the fp32 inputs (k the row's edge count; one final rounding, 2^-24 relative, doubled
for the conversion of the fp64 intermediate; the fp64 sums lose at most about k 2^-53 of the summed magnitudes, written (k + 4) 2^-50):
    |mean32 - mean| <= 2^-23 |mean| + (k + 4) 2^-50 max_e |x_e|
    |std32  - std | <= 2^-23 std    + (k + 4) 2^-50 (var + max_e (x_e - mean)^2) / std
The second term of the std bound is what a summation that keeps the DEVIATIONS small - sums shifted by an element of the row - can
hold, and what sums of raw squares cannot on inputs far from zero (test_segstats_cpu.py shows both)."""
import numpy as np

import segmax_ref as S

SETS = S.SETS + ("offset", "constant")
AGGREGATORS = ("mean", "std", "max", "min")
LAYER_TOL_Y, LAYER_TOL_G = 1e-5, 1e-4   # PNAConv against dense fp64, of the largest entry: output, gradients (tests/test_gpu_segstats.py)


def input_set(name, n, D, seed=0):
    """segmax_ref's four sets, `offset` (1000 + 1e-3 normal: a variance thirteen orders below the square of the mean) and `constant`
    (one value per column: the variance is exactly 0)."""
    if name in S.SETS:
        return S.input_set(name, n, D, seed)
    rng = np.random.default_rng(seed + 1000 * SETS.index(name))
    if name == "offset":
        return (1000.0 + 1e-3 * rng.standard_normal((n, D))).astype(np.float32)
    return np.repeat(rng.standard_normal((1, D)).astype(np.float32), n, axis=0)


def segment_stats(rp, col, X, eps=1e-5):
    """-> dict: mean, std (fp64 [n, D]), max, min (fp32, the winner's bits), argmax, argmin (int32), k (int64 [n]) and the bounds
    mean_bound, std_bound (fp64 [n, D]; 0 on rows without edges, where the results are exactly 0)"""
    rp = np.asarray(rp, dtype=np.int64)
    n, D = len(rp) - 1, X.shape[1]
    out = {"mean": np.zeros((n, D)), "std": np.zeros((n, D)), "max": np.zeros((n, D), np.float32), "min": np.zeros((n, D), np.float32),
           "argmax": np.full((n, D), -1, np.int32), "argmin": np.full((n, D), -1, np.int32), "k": np.maximum(np.diff(rp), 0),
           "mean_bound": np.zeros((n, D)), "std_bound": np.zeros((n, D))}
    cols = np.arange(D)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            lo, hi = int(rp[i]), int(rp[i + 1])
            if hi <= lo or not D:
                continue
            k = hi - lo
            Sx = X[np.asarray(col[lo:hi], dtype=np.int64)]
            ax, an = np.argmax(Sx, axis=0), np.argmin(Sx, axis=0)
            out["argmax"][i], out["max"][i] = lo + ax, Sx[ax, cols]
            out["argmin"][i], out["min"][i] = lo + an, Sx[an, cols]
            x = Sx.astype(np.float64)
            mean = x.sum(0) / k
            dev = x - mean
            var = (dev * dev).sum(0) / k
            std = np.sqrt(np.maximum(var, 0.0) + eps)
            out["mean"][i], out["std"][i] = mean, std
            out["mean_bound"][i] = 2.0 ** -23 * np.abs(mean) + (k + 4) * 2.0 ** -50 * np.abs(x).max(0)
            out["std_bound"][i] = 2.0 ** -23 * std + (k + 4) * 2.0 ** -50 * (var + (dev * dev).max(0)) / std
    return out


def wins_min(v1, p1, v2, p2):
    """the min side of the contract's combine, spelt out: does (v1, p1) beat (v2, p2)?"""
    n1, n2 = np.isnan(v1), np.isnan(v2)
    if n1 or n2:
        return bool(n1 and (not n2 or p1 < p2))
    return bool(v1 < v2 or (v1 == v2 and p1 < p2))


def segment_min_brute(rp, col, X):
    """min / argmin by the comparator, edge by edge from the row's LAST edge to its first (the order must not matter) - small graphs only"""
    n, D = len(rp) - 1, X.shape[1]
    Y = np.zeros((n, D), dtype=np.float32)
    arg = np.full((n, D), -1, dtype=np.int32)
    for i in range(n):
        for d in range(D):
            best = None
            for e in range(int(rp[i + 1]) - 1, int(rp[i]) - 1, -1):
                if best is None or wins_min(X[col[e], d], e, X[col[best], d], best):
                    best = e
            if best is not None:
                arg[i, d], Y[i, d] = best, X[col[best], d]
    return Y, arg


def kernel_moments(rp, col, X, eps=1e-5, shifted=True, parts=4, seed=0):
    """(mean32, std32) by the kernel's arithmetic: fp64 sums of t = x - s and t^2 (s the row's first neighbour; 0 with shifted=False),
    the row's edges in a permuted order dealt over `parts` partial sums that are added at the end, mean = s + S1 / k,
    var = S2 / k - (S1 / k)^2, one rounding to fp32 each."""
    rp = np.asarray(rp, dtype=np.int64)
    n, D = len(rp) - 1, X.shape[1]
    mean, std = np.zeros((n, D), np.float32), np.zeros((n, D), np.float32)
    rng = np.random.default_rng(seed)
    old = np.seterr(invalid="ignore", over="ignore")           # (the `specials` set: inf - inf)
    for i in range(n):
        lo, hi = int(rp[i]), int(rp[i + 1])
        if hi <= lo or not D:
            continue
        k = hi - lo
        x = X[np.asarray(col[lo:hi], dtype=np.int64)].astype(np.float64)
        s = x[0] if shifted else np.zeros(D)
        t = (x - s)[rng.permutation(k)]
        s1, s2 = np.zeros(D), np.zeros(D)
        for p in range(parts):                       # np.cumsum adds one element after the other, as a lane does
            if len(t[p::parts]):
                s1 = s1 + np.cumsum(t[p::parts], axis=0)[-1]
                s2 = s2 + np.cumsum(t[p::parts] * t[p::parts], axis=0)[-1]
        m1 = s1 / k
        mean[i] = (s + m1).astype(np.float32)
        std[i] = np.sqrt(np.maximum(s2 / k - m1 * m1, 0.0) + np.float64(np.float32(eps))).astype(np.float32)
    np.seterr(**old)
    return mean, std


def _edge_rows(rp):
    rp = np.asarray(rp, dtype=np.int64)
    return np.repeat(np.arange(len(rp) - 1), np.maximum(np.diff(rp), 0))


def segment_stats_backward(rp, col, Z=None, a=None, b=None, argmax=None, dmax=None, argmin=None, dmin=None):
    """-> (dZ fp64 [n, D], k int64 [n, D], sabs fp64 [n, D]): for every edge e = (i <- j) the addends a[i, d], b[i, d] Z[j, d],
    dmax[i, d] where argmax[i, d] == e and dmin[i, d] where argmin[i, d] == e, summed into dZ[j, d]; k the number of addends of an
    element and sabs the sum of their magnitudes (|dZ32 - dZ| <= k 2^-24 sabs for an fp32-or-better sum in any order).  Every addend
    is a term; a group that is None contributes none."""
    first = next(t for t in (a, b, argmax, argmin, Z) if t is not None)
    n, D = first.shape
    E = int(np.asarray(rp)[-1])
    dZ, k, sabs = np.zeros((n, D)), np.zeros((n, D), np.int64), np.zeros((n, D))
    if not E:
        return dZ, k, sabs
    cols = np.asarray(col[:E], dtype=np.int64)
    pos = np.argsort(cols, kind="stable")                       # the edges grouped by source: A^T's order
    src, dst = cols[pos], _edge_rows(rp)[:E][pos]
    starts = np.flatnonzero(np.concatenate([[True], src[1:] != src[:-1]]))
    named = src[starts]

    def add(into, vals):                                        # the sums of vals [E, D] over every source's segment
        into[named] += np.add.reduceat(vals, starts, axis=0)

    f64 = lambda t: t.astype(np.float64)                        # noqa: E731
    terms = []
    if a is not None:
        terms.append((f64(a)[dst], None))
    if b is not None:
        terms.append((f64(b)[dst] * f64(Z)[src], None))
    if argmax is not None:
        terms.append((f64(dmax)[dst], argmax[dst] == pos[:, None]))
    if argmin is not None:
        terms.append((f64(dmin)[dst], argmin[dst] == pos[:, None]))
    for t, mask in terms:
        if mask is None:
            k[named] += np.diff(np.concatenate([starts, [E]]))[:, None]
        else:
            t = np.where(mask, t, 0.0)
            add(k, mask.astype(np.int64))
        add(dZ, t)
        add(sabs, np.abs(t))
    return dZ, k, sabs


def coefficients(rp, d_mean, d_std, mean, std):
    """(a, b) of the backward contract from the gradients of mean and std (either may be None): on rows with k > 0 edges
    b = d_std / (k std), a = d_mean / k - b mean; 0 on rows without.  In the dtype of the inputs."""
    k = np.maximum(np.diff(np.asarray(rp, dtype=np.int64)), 0)[:, None]
    has = k > 0
    ref = d_mean if d_mean is not None else d_std
    b = np.where(has, d_std / (np.maximum(k, 1) * np.where(has, std, 1)), 0).astype(ref.dtype) if d_std is not None else None
    a = np.where(has, d_mean / np.maximum(k, 1), 0).astype(ref.dtype) if d_mean is not None else np.zeros_like(ref)
    if b is not None:
        a = a - b * mean
    return a, b


def dense_pna(A, X, W_src, W_dst, b_pre, W_post, b_post, aggregators=AGGREGATORS, scalers=("identity", "amplification", "attenuation"), delta=None,
              eps=1e-5):
    """PNAConv as dense torch operations (any dtype: the tests use fp64): A [n, n] with A[i, j] = the number of edges i <- j; the
    message of an edge is X[j] W_src + X[i] W_dst + b_pre, aggregated per destination, scaled by degree and sent through W_post."""
    import torch
    n = A.shape[0]
    deg = A.sum(1, keepdim=True)
    has, k = deg > 0, deg.clamp(min=1)
    zero = torch.zeros((), dtype=X.dtype)
    Z = X @ W_src
    c = X @ W_dst + (b_pre if b_pre is not None else 0)
    msg = Z.unsqueeze(0) + c.unsqueeze(1)                                   # [dst, src, m]
    w = (A / k).unsqueeze(2)
    mean = (w * msg).sum(1)
    var = (w * (msg - mean.unsqueeze(1)) ** 2).sum(1)
    absent = (A == 0).unsqueeze(2)
    agg = {"mean": torch.where(has, mean, zero), "std": torch.where(has, torch.sqrt(var.clamp(min=0) + eps), zero),
           "max": torch.where(has, msg.masked_fill(absent, float("-inf")).max(1).values, zero),
           "min": torch.where(has, msg.masked_fill(absent, float("inf")).min(1).values, zero)}
    log_deg = torch.log(k + 1)
    if delta is None:
        delta = torch.log(deg + 1).mean()
    scale = {"identity": torch.ones_like(deg), "amplification": log_deg / delta, "attenuation": delta / log_deg}
    block = torch.cat([X] + [scale[s] * agg[a] for s in scalers for a in aggregators], dim=1)
    out = block @ W_post
    return out + b_post if b_post is not None else out
