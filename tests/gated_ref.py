"""Restatement, in numpy, of the gated aggregation (tcgnn_gated_sum / tcgnn_gated_source_grad), the bounds the kernels are held to and
the input sets.  Shared by tests/test_gated_cpu.py and tests/test_gpu_gated.py; no GPU needed to import.

Reference: z = fl32(k[row e] + q[col e]), rounded once as the contract says; then fp64: eta = sigmoid(z), c = 1 - eta, products, sums.
Bounds, with u = 2^-24 and to first order.  a = fl32(-|z| log2 e): the constant and the product round, |a - a_true| <= 2 u |a|, which
exp2 turns into 2 u |z| relative in t; the hardware exponential 1 ulp = 2 u (edge_ops_ref's allowance for es_exp); r = fl32(1 + t): u;
a division: u.  1 / r inherits t's error times t / (1 + t) <= 1/2, t / r times 1 / (1 + t) <= 1, so either gate is within
2 u (|z| + 1) + 2 u relatively; second order is below 2^-16 of that wherever t != 0 (|z| < 104) and covered by rounding up:
    EPS_GATE = 2^-23 (|z| + 3);   Y's and dv's term fl32(eta w): EPS_GATE + u;   S's and dq's fl32(fl32(eta c) w): 2 EPS_GATE + 2 u.
Beyond |z| log2 e = 126 t is below the normal range and the hardware may return 0, and a tiny gate times a small w may be subnormal:
an absolute FLOOR (|w| + 1) per term, FLOOR = 2^-125.  An fp64 sum of n < 2^13 terms errs by less than OWN_SUM = 2^-40 (gat_ref's) of
sum |term|; the result rounds once:
    |got - ref| <= sum_e (EPS(z_e) + OWN_SUM) |term64_e| + FLOOR sum_e (|w_e| + 1) + u |ref| + 2^-149,
and dq = v[j] times such a sum: |v[j]| times the sum's part.  Nothing was fitted to the kernel; measured shares: DESIGN.md 4.21,
profiles/r32/gpu_gated_tests_figures.txt."""
import functools

import numpy as np

OWN_SUM, FLOOR, U = 2.0 ** -40, 2.0 ** -125, 2.0 ** -24
ROW_LENGTHS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4100, 9000)   # the walk's thresholds are segment_max's: 1024
WIDTHS = (1, 3, 4, 41, 64, 65, 128, 256, 260)
SETS = ("normal_x1", "normal_x8", "constant_q", "magnitude_1e4", "aliased")


@functools.lru_cache(maxsize=None)
def row_class_graphs(seed=5, n=9000):
    """{"A": (rowptr, col) with a row of every length of ROW_LENGTHS, random column ids (duplicates certain), "T": its transpose}, int32"""
    import walks
    rng = np.random.default_rng(seed)
    lens = np.zeros(n, np.int64)
    lens[8 + rng.permutation(n - 16)[:len(ROW_LENGTHS)]] = ROW_LENGTHS
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = rng.integers(0, n, int(rp[-1])).astype(np.int32)
    rp_t, col_t, _ = walks.transposed_csr(rp, col)
    return {"A": (rp, col), "T": (rp_t.astype(np.int32), col_t.astype(np.int32))}


def inputs(name, n, D, seed=29):
    """(k, q, v, dY), fp32 [n, D]: normal x {1, 8}; q constant; |z| up to 2e4 (gates exactly 0 or 1, c underflows); k, q, v ONE array"""
    rng = np.random.default_rng([seed, D])
    k, q, v, dY = (rng.standard_normal((n, D)).astype(np.float32) for _ in range(4))
    if name == "normal_x8":
        k, q = 8 * k, 8 * q
    elif name == "constant_q":
        q = np.repeat(q[:1], n, axis=0)
    elif name == "magnitude_1e4":
        k, q = ((1e4 * np.sign(t) * (1 + 0.01 * np.abs(t))).astype(np.float32) for t in (k, q))
    elif name == "aliased":
        q = v = k
    return k, q, v, dY


def edge_rows(rp):
    return np.repeat(np.arange(len(rp) - 1), np.diff(np.asarray(rp, np.int64)))


def _sum_by(index, T, n):   # out[r] = the fp64 sum of the rows of T whose index is r, [n, D]
    counts = np.bincount(index, minlength=n)
    out, has = np.zeros((n, T.shape[1])), counts > 0
    out[has] = np.add.reduceat(T[np.argsort(index, kind="stable")], (np.cumsum(counts) - counts)[has], axis=0)
    return out


def _bounded(index, n, eps, term, w, scale=1.0):
    ref = scale * _sum_by(index, term, n)
    err = np.abs(scale) * _sum_by(index, (eps + OWN_SUM) * np.abs(term) + FLOOR * (np.abs(w) + 1.0), n)
    return ref, err + U * np.abs(ref) + 2.0 ** -149


def gated_f64(rp, col, k, q, v, dY=None):
    """{name: (fp64 reference [n, D], bound [n, D])} for Y and S - and, given dY, dq and dv (sums by source node)"""
    n, rows, cols = len(rp) - 1, edge_rows(rp), np.asarray(col[:int(rp[-1])], np.int64)
    z = (np.asarray(k, np.float32)[rows] + np.asarray(q, np.float32)[cols]).astype(np.float64)   # fp32: one rounding
    t = np.exp(-np.abs(z))
    eta, c = np.where(z >= 0, 1.0, t) / (1.0 + t), np.where(z >= 0, t, 1.0) / (1.0 + t)
    eg, w = 2.0 ** -23 * (np.abs(z) + 3.0), np.asarray(v, np.float64)[cols]
    out = {"Y": _bounded(rows, n, eg + U, eta * w, w), "S": _bounded(rows, n, 2 * eg + 2 * U, eta * c * w, w)}
    if dY is not None:
        g = np.asarray(dY, np.float64)[rows]
        out["dv"] = _bounded(cols, n, eg + U, eta * g, g)
        out["dq"] = _bounded(cols, n, 2 * eg + 2 * U, eta * c * g, g, scale=np.asarray(v, np.float64))
    return out


def worst_share(got, ref, bound):   # max |got - ref| / bound; a NaN or an infinity anywhere in got counts as infinite
    got = np.asarray(got, np.float64)
    return float(np.max(np.abs(got - ref) / bound)) if np.isfinite(got).all() else np.inf


def dense_f64(rp, col, k, q, v):   # torch's plain composition, by index_add_
    import torch
    rows, cols = torch.from_numpy(edge_rows(rp)), torch.from_numpy(np.asarray(col[:int(rp[-1])], np.int64))
    return torch.zeros_like(k).index_add_(0, rows, torch.sigmoid(k[rows] + q[cols]) * v[cols])
