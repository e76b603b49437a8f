"""Restatements for the max aggregation (tcgnn_segment_max / _backward), numpy only: what tests/test_segmax_cpu.py checks against a
brute-force comparator and tests/test_gpu_segmax.py holds the kernels to.

The tie rule of the contract is numpy.argmax over the row's slice: the greater value wins, among equal values (-0.0 == +0.0) the first
position, a NaN beats every number and the first NaN wins.  Y is a copy of the winner (its bits), 0 for a row without edges; arg is the
winner's CSR position, -1 for such a row."""
import numpy as np

SETS = ("ties", "signed_zero", "specials", "normal")
# SAGEConv against dense fp64, of the largest entry: (output, gradients) per aggregator (tests/test_gpu_segmax.py says why)
SAGE_TOL = {"mean": (2e-3, 2e-3), "max": (1e-5, 1e-4), "pool": (1e-5, 1e-4)}


def segment_max(rp, col, X):
    """-> (Y fp32 [n, D], arg int32 [n, D])"""
    rp = np.asarray(rp, dtype=np.int64)
    n, D = len(rp) - 1, X.shape[1]
    Y = np.zeros((n, D), dtype=np.float32)
    arg = np.full((n, D), -1, dtype=np.int32)
    cols = np.arange(D)
    for i in range(n):
        lo, hi = int(rp[i]), int(rp[i + 1])
        if hi > lo and D:
            S = X[np.asarray(col[lo:hi], dtype=np.int64)]
            a = np.argmax(S, axis=0)
            arg[i] = lo + a
            Y[i] = S[a, cols]
    return Y, arg


def segment_max_backward(rp, col, arg, dY):
    """-> (dX fp64 [n, D], k int64 [n, D], sabs fp64 [n, D]): dX[j, d] = the sum of dY[i, d] over the (i, d) whose winner is an edge from
    j, k the number of its terms and sabs the sum of their magnitudes (|dX32 - dX| <= k 2^-24 sabs for an fp32 sum in any order)."""
    n, D = arg.shape
    dX, k, sabs = np.zeros(n * D), np.zeros(n * D, dtype=np.int64), np.zeros(n * D)
    i, d = np.nonzero(arg >= 0)
    at = np.asarray(col, dtype=np.int64)[arg[i, d].astype(np.int64)] * D + d
    t = dY[i, d].astype(np.float64)
    np.add.at(dX, at, t)
    np.add.at(k, at, 1)
    np.add.at(sabs, at, np.abs(t))
    return dX.reshape(n, D), k.reshape(n, D), sabs.reshape(n, D)


def input_set(name, n, D, seed=0):
    """fp32 [n, D]: `ties` integers in [-2, 2] (nearly every maximum is shared: the smallest position decides), `signed_zero` +-0.0
    only, `specials` random values with a NaN (two payloads), +inf or -inf in one row out of eight, `normal` random values."""
    rng = np.random.default_rng(seed + 1000 * SETS.index(name))
    if name == "ties":
        return rng.integers(-2, 3, (n, D)).astype(np.float32)
    if name == "signed_zero":
        return np.where(rng.random((n, D)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    X = rng.standard_normal((n, D)).astype(np.float32)
    if name == "specials":
        bits = X.view(np.uint32)
        kinds = np.array([0x7FC00000, 0xFFC00123, 0x7F800000, 0xFF800000], dtype=np.uint32)   # quiet NaN, a negative NaN with a payload, +inf, -inf
        rows = np.arange(0, n, 8)
        for r in rows:
            hit = rng.random(D) < 0.5
            bits[r, hit] = kinds[rng.integers(0, 4, int(hit.sum()))]
    return X


def wins(v1, p1, v2, p2):
    """the contract's combine, spelt out: does (v1, p1) beat (v2, p2)?"""
    n1, n2 = np.isnan(v1), np.isnan(v2)
    if n1 or n2:
        return bool(n1 and (not n2 or p1 < p2))
    return bool(v1 > v2 or (v1 == v2 and p1 < p2))


def segment_max_brute(rp, col, X):
    """segment_max by the comparator, edge by edge from the row's LAST edge to its first (the order must not matter) - small graphs only"""
    n, D = len(rp) - 1, X.shape[1]
    Y = np.zeros((n, D), dtype=np.float32)
    arg = np.full((n, D), -1, dtype=np.int32)
    for i in range(n):
        for d in range(D):
            best = None
            for e in range(int(rp[i + 1]) - 1, int(rp[i]) - 1, -1):
                v = X[col[e], d]
                if best is None or wins(v, e, X[col[best], d], best):
                    best = e
            if best is not None:
                arg[i, d] = best
                Y[i, d] = X[col[best], d]
    return Y, arg


def dense_sage(A, X, W_self, W_neigh, bias, aggregator, W_pool=None, b_pool=None):
    """SAGEConv as dense torch operations (any dtype: the tests use fp64): A [n, n] with A[i, j] = the number of edges i <- j."""
    import torch
    deg = A.sum(1, keepdim=True)
    if aggregator == "mean":
        agg = (A @ X) / deg.clamp(min=1)
    else:
        H = torch.relu(X @ W_pool + b_pool) if aggregator == "pool" else X
        masked = H.unsqueeze(0).expand(A.shape[0], -1, -1).masked_fill((A == 0).unsqueeze(2), float("-inf"))   # [dst, src, d]
        agg = torch.where(deg > 0, masked.max(1).values, torch.zeros((), dtype=X.dtype))
    out = X @ W_self + agg @ W_neigh
    return out + bias if bias is not None else out
