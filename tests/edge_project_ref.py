"""fp64 NumPy restatement of the fused edge-projection operators (tcgnn_edge_project_*) and the bounds the GPU tests hold them to.

    p[e, d]  = be[d] + sum_k A[e, k] We[k, d];   z = X[col e, d] + p[e, d];   m = act(z);   pass = identity or !(z <= 0)
    forward      Y[i, d]   = sum over e in row i of m[e, d]
    row side     g[e, d]   = pass ? dY[row e, d] : 0;   dA = g We^T;   dWe = A^T g;   dbe = column sums of g
    source side  dX[j, d]  = sum over the edges e with col e = j of g[e, d]

u = 2^-24 is fp32's unit roundoff.  K' = 4 ceil((K + 1) / 4) is the padded length of the projection's dot product."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149


def _rows(rp):
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


def _parts(rp, col, X, A, We, be, act):
    X, A, We, be = (np.asarray(t, np.float64) for t in (X, A, We, be))
    p = be[None, :] + A @ We
    z = X[col] + p
    ok = np.ones(z.shape, bool) if act == "identity" else ~(z <= 0)
    mag = np.abs(X[col]) + np.abs(be)[None, :] + np.abs(A) @ np.abs(We)   # what the K + 1 products and the one addition are made of
    return z, ok, mag


def forward(rp, col, X, A, We, be, act):
    """-> (S, bound): the exact sums and
    |Y - S| <= u |S| + 2^-149 + 2^-40 sum |m| + (K' + 2) u sum_e (|X[col e, d]| + |be[d]| + sum_k |A[e, k]| |We[k, d]|):
    the final rounding, the fp64 sum (the segment family's terms), and a dot product of K + 1 terms in any order plus one addition,
    passed through a 1-Lipschitz activation."""
    z, ok, mag = _parts(rp, col, X, A, We, be, act)
    m = np.where(ok, z, 0.0)
    n, rows = len(rp) - 1, _rows(rp)
    S, absm, T = (np.zeros((n, z.shape[1])) for _ in range(3))
    for acc, term in ((S, m), (absm, np.abs(m)), (T, mag)):
        np.add.at(acc, rows, term)
    kp = 4 * ((A.shape[1] + 1 + 3) // 4)
    return S, U * np.abs(S) + TINY + 2.0 ** -40 * absm + (kp + 2) * U * T


def backward(rp, col, X, A, We, be, dY, act):
    """-> (dA, dWe, dbe, dX) exact and their first-order bounds (same order):
    dA   a D-term fp32 dot product in any order:                     (D + 1) u sum_d |g[e, d]| |We[k, d]| + 2^-149
    dWe  an fp32 accumulation over a wavefront's edges, n of them:   n u sum_e |A[e, k]| |g[e, d]| + 2^-149            (dbe: A[e, K] = 1)
         with n = E, every edge charged to one wavefront.  That covers the rest of the path too: however the n terms are split over
         wavefronts and workgroups they meet in n - 1 additions that are not additions of a zero (those are exact), so a term passes
         at most n - 1 roundings besides its product's own, and the one final rounding stands where the fp64 pass added exactly.
    dX   the segment family's fp64 sum of fp32 values, rounded once: u |dX| + 2^-149 + 2^-40 sum |g|
    The bounds hold where no mask can flip (act = 'identity', or inputs on which z is exact)."""
    z, ok, _ = _parts(rp, col, X, A, We, be, act)
    A, We, dY = (np.asarray(t, np.float64) for t in (A, We, dY))
    g = np.where(ok, dY[_rows(rp)], 0.0)
    n_e, D = g.shape
    dA, dWe, dbe = g @ We.T, A.T @ g, g.sum(0)
    dX, absg = np.zeros_like(dY), np.zeros_like(dY)
    np.add.at(dX, col, g)
    np.add.at(absg, col, np.abs(g))
    bounds = ((D + 1) * U * (np.abs(g) @ np.abs(We).T) + TINY,
              n_e * U * (np.abs(A).T @ np.abs(g)) + TINY,
              n_e * U * np.abs(g).sum(0) + TINY,
              U * np.abs(dX) + TINY + 2.0 ** -40 * absg)
    return (dA, dWe, dbe, dX), bounds
