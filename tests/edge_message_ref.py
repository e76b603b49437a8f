"""Restatements, in numpy and torch, of message passing with a feature vector per edge (tcgnn_edge_message / _backward, tcgnn_edge_sum,
the operators aggregate_ue / edge_sum and the layer GINEConv), the bound the kernels are held to - with its derivation - and the input
sets.  Shared by tests/test_edge_message_cpu.py and tests/test_gpu_edge_message.py; no GPU needed to import.

The message.  z = fl32(X[col e, d] + Ef[e, d]): one fp32 rounding, numpy's fp32 addition.  m = z under the identity; under ReLU m = z
where !(z <= 0) and +0 otherwise - torch.relu's values: a NaN stays a NaN, -0.0 and +0.0 give a zero (message).

Y and edge_sum.  The kernel forms Y = fl32(sum_e (double)m_e): the terms are fp32 numbers, exact in fp64.  An fp64 sum of k terms in ANY
order differs from the true sum by at most (additions on the longest chain) 2^-53 sum |term|.  A lane adds its share of a row - the
70 000-edge row is 70 000 / 4 = 17 500 terms a lane at D = 256, where a lane group is a whole wavefront - and the trees add a dozen
levels: 2^-39 sum |term| at worst, some 2^-46 as a random walk.  The family's allowance (gat_ref.OWN_SUM, what tcgnn_gat's,
tcgnn_gatv2's and tcgnn_segment_stats' sums are held to) is 2^-40; it is kept, unchanged, and it also covers the reference S below,
itself an fp64 sum in numpy's order.  The one rounding to fp32 adds 2^-24 |S|, or 2^-149 where the result is subnormal:
    |Y - S| <= 2^-24 |S| + 2^-149 + 2^-40 sum_e |m_e|                                                              (bound, share)
With integer-valued inputs of small magnitude every partial sum is an integer below 2^24: the result is exact, and held to equality.

dM.  No arithmetic reaches the result: dM[e, d] has the bits of dY[row e, d] or is +0.0.  Held to equality of the bits on every set.
A position no row covers (in front of rowptr[0] or behind rowptr[N]) is +0.0.
"""
import numpy as np

OWN_SUM = 2.0 ** -40
SETS = ("integer", "normal", "large", "boundary")
ACTS = {None: 0, "identity": 0, "relu": 1}
TOL_Y, TOL_G = 1e-5, 1e-4   # the operator and GINEConv against dense fp64, of the largest entry (tests/test_gpu_edge_message.py says why)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

def input_set(name, n, E, D, seed=0):
    """(X [n, D], Ef [E, D], dY [n, D]) fp32.  `integer`: integers in [-4, 4] (every sum exact, a fifth of the z exactly 0); `normal`:
    standard normal; `large`: magnitude 1e4 with mixed signs (z of order 2e4 or, where the signs differ, a few hundred: the sums cancel);
    `boundary`: normal, with -0.0, +0.0, the smallest subnormals of both signs and two NaNs planted in a third of X and half of Ef set
    to -0.0: where both meet, z IS the planted value (x + -0.0 = x, the sign of a zero included)."""
    rng = np.random.default_rng([seed, SETS.index(name), n, D])
    if name == "integer":
        return tuple(rng.integers(-4, 5, s).astype(np.float32) for s in ((n, D), (E, D), (n, D)))
    X, Ef, dY = (rng.standard_normal(s).astype(np.float32) for s in ((n, D), (E, D), (n, D)))
    if name == "large":
        big = lambda z: (1e4 * np.sign(z) * (1 + 0.01 * np.abs(z))).astype(np.float32)   # noqa: E731
        return big(X), big(Ef), dY
    if name == "boundary":
        kinds = np.array([0x80000000, 0x00000000, 0x00000001, 0x80000001, 0x7FC00000, 0xFFC00123], dtype=np.uint32)
        hit = rng.random((n, D)) < 0.3
        X.view(np.uint32)[hit] = kinds[rng.integers(0, len(kinds), int(hit.sum()))]
        Ef[rng.random((E, D)) < 0.5] = np.float32(-0.0)
    return X, Ef, dY


# ---- numpy restatements ----------------------------------------------------------------------------------------------------------------

def edge_rows(rp):
    """the row of every covered position rp[0] .. rp[n] - 1"""
    rp = np.asarray(rp, dtype=np.int64)
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


def message_f32(rp, col, X, Ef, act):
    """(z, m) fp32 [covered positions, D]: z = fl32(X[col e] + Ef[e]), m = act(z)"""
    rp = np.asarray(rp, dtype=np.int64)
    lo, hi = int(rp[0]), int(rp[-1])
    z = np.asarray(X, np.float32)[np.asarray(col[lo:hi], dtype=np.int64)] + np.asarray(Ef, np.float32)[lo:hi]
    if ACTS[act]:
        with np.errstate(invalid="ignore"):
            return z, np.where(z <= 0, np.float32(0.0), z).astype(np.float32)
    return z, z


def segment_sums(terms, seg, n):
    """(S, A) [n, D]: the fp64 sums of terms [k, D] and of their magnitudes over the segments seg[k] (ascending)"""
    terms = np.asarray(terms, dtype=np.float64)
    S, A = np.zeros((n, terms.shape[1])), np.zeros((n, terms.shape[1]))
    if len(terms) and terms.shape[1]:
        cnt = np.bincount(seg, minlength=n)[:n]
        full = np.nonzero(cnt > 0)[0]
        starts = (np.cumsum(cnt) - cnt)[full]
        S[full], A[full] = np.add.reduceat(terms, starts, axis=0), np.add.reduceat(np.abs(terms), starts, axis=0)
    return S, A


def edge_message(rp, col, X, Ef, act):
    """-> (Y fp32 [n, D], S fp64, A fp64): the operator, its fp64 sums and the sums of the terms' magnitudes"""
    _, m = message_f32(rp, col, X, Ef, act)
    S, A = segment_sums(m, edge_rows(rp), len(rp) - 1)
    with np.errstate(over="ignore", invalid="ignore"):
        return S.astype(np.float32), S, A


def edge_message_backward(rp, col, X, Ef, dY, act, num_edges=None):
    """-> dM fp32 [num_edges, D] (num_edges: len(col) unless given): the bits of dY[row e] or +0.0"""
    rp = np.asarray(rp, dtype=np.int64)
    lo, hi = int(rp[0]), int(rp[-1])
    dY = np.asarray(dY, np.float32)
    dM = np.zeros((len(col) if num_edges is None else num_edges, dY.shape[1]), np.float32)
    g = dY[edge_rows(rp)]
    if ACTS[act]:
        z, _ = message_f32(rp, col, X, Ef, act)
        with np.errstate(invalid="ignore"):
            g = np.where(z <= 0, np.float32(0.0), g).astype(np.float32)
    dM[lo:hi] = g
    return dM


def edge_sum(rp, perm, M):
    """-> (Y fp32 [n, D], S, A): the rows M[perm[t]] (perm None: M[t]) summed over the positions t of every row"""
    rp = np.asarray(rp, dtype=np.int64)
    lo, hi = int(rp[0]), int(rp[-1])
    src = np.asarray(M, np.float32)[lo:hi] if perm is None else np.asarray(M, np.float32)[np.asarray(perm[lo:hi], dtype=np.int64)]
    S, A = segment_sums(src, edge_rows(rp), len(rp) - 1)
    with np.errstate(over="ignore", invalid="ignore"):
        return S.astype(np.float32), S, A


def bound(S, A):
    return 2.0 ** -24 * np.abs(S) + 2.0 ** -149 + OWN_SUM * A


def share(got, S, A):
    """(whole, excess): whole = worst |got - S| / bound, which must be <= 1 - inf where a sum without terms is not exactly 0, where got is
    not finite although S is, or where a NaN / infinite S is not met by the same; excess = what the result needs BEYOND its own
    rounding, as a share of the summation's allowance alone (a correctly rounded result uses up to all of the rounding term)."""
    got = np.asarray(got, dtype=np.float64)
    if not got.size:
        return 0.0, 0.0
    fin = np.isfinite(S)
    if np.any(got[A == 0] != 0) or not np.isfinite(got[fin]).all():
        return float("inf"), float("inf")
    with np.errstate(invalid="ignore"):
        if not np.array_equal(np.isnan(S), np.isnan(got)) or np.any(got[~fin & ~np.isnan(S)] != S[~fin & ~np.isnan(S)]):
            return float("inf"), float("inf")
    err = np.abs(got[fin] - S[fin])
    Sf, Af = S[fin], A[fin]
    ok = Af > 0
    excess = float((np.maximum(err - 2.0 ** -24 * np.abs(Sf) - 2.0 ** -149, 0.0)[ok] / (OWN_SUM * Af[ok])).max()) if ok.any() else 0.0
    return (float((err / bound(Sf, Af)).max()) if err.size else 0.0), excess


# ---- brute force and the dense fp64 model ----------------------------------------------------------------------------------------------

def brute_edge_message(rp, col, X, Ef, act):
    """fp64 [n, D] by unbuffered scatter-add, position by position from the LAST to the first (the order must not matter): another
    algorithm than segment_sums.  The message is the contract's: fl32 of the sum, then the activation."""
    rp = np.asarray(rp, dtype=np.int64)
    n, D = len(rp) - 1, X.shape[1]
    Y = np.zeros((n, D))
    for i in range(n):
        for e in range(int(rp[i + 1]) - 1, int(rp[i]) - 1, -1):
            z = (np.asarray(X[col[e]], np.float32) + np.asarray(Ef[e], np.float32)).astype(np.float32)
            if ACTS[act]:
                with np.errstate(invalid="ignore"):
                    z = np.where(z <= 0, np.float32(0.0), z)
            Y[i] += z.astype(np.float64)
    return Y


def scatter_edge_message(rp, col, X, Ef, act):
    """the same by numpy.add.at (sequential, unbuffered): brute force that scales to the boundary graphs"""
    _, m = message_f32(rp, col, X, Ef, act)
    Y = np.zeros((len(rp) - 1, X.shape[1]))
    np.add.at(Y, edge_rows(rp)[::-1], m.astype(np.float64)[::-1])
    return Y


def incidence(rp, col, dtype=None, sparse=False):
    """(B [n, E], Sel [E, n]) torch matrices: B[i, e] = 1 where position e is in row i, Sel[e, j] = 1 where col e = j.  sparse: the same
    two matrices in COO storage (a graph of thousands of nodes: n E dense entries would not fit), for the same products."""
    import torch
    dtype = dtype or torch.float64
    n, E = len(rp) - 1, int(np.asarray(rp)[-1])
    e = torch.arange(E)
    rows, cols = torch.from_numpy(edge_rows(rp)), torch.from_numpy(np.asarray(col[:E], dtype=np.int64))
    if sparse:
        one = torch.ones(E, dtype=dtype)
        return (torch.sparse_coo_tensor(torch.stack([rows, e]), one, (n, E)).coalesce(),
                torch.sparse_coo_tensor(torch.stack([e, cols]), one, (E, n)).coalesce())
    B, Sel = torch.zeros(n, E, dtype=dtype), torch.zeros(E, n, dtype=dtype)
    B[rows, e] = 1
    Sel[e, cols] = 1
    return B, Sel


def dense_aggregate_ue(B, Sel, X, Ef, act="relu"):
    """Y = B act(Sel X + Ef): the operator as dense products, any dtype, differentiable"""
    import torch
    Z = Sel @ X + Ef
    return B @ (torch.relu(Z) if ACTS[act] else Z)


def dense_gine(B, Sel, X, edge_attr, W, bias, eps, W_e=None, b_e=None):
    """GINEConv on the dense incidence matrices in torch, differentiable: h = (1 + eps) X + B relu(Sel X + Ef'), out = h W + b"""
    Ef = edge_attr @ W_e + b_e if W_e is not None else edge_attr
    out = ((1.0 + eps) * X + dense_aggregate_ue(B, Sel, X, Ef, "relu")) @ W
    return out + bias if bias is not None else out


# ---- a pure-torch backend ------------------------------------------------------------------------------------------------------------------

class TorchBackend:
    """forward_ue, backward_ue, edge_sum and transpose_graph composed of torch index operations, any dtype, on the CPU"""

    @staticmethod
    def _rows(rp):
        import torch
        return torch.repeat_interleave(torch.arange(rp.numel() - 1), (rp[1:] - rp[:-1]).long())

    def forward_ue(self, X, Ef, rp, col, act="relu", out=None):
        import torch
        z = X[col.long()] + Ef
        return torch.zeros_like(X).index_add_(0, self._rows(rp), torch.relu(z) if ACTS[act] else z)

    def backward_ue(self, dY, X, Ef, rp, col, act="relu", out=None):
        import torch
        g = dY[self._rows(rp)]
        if ACTS[act]:
            g = torch.where(X[col.long()] + Ef <= 0, torch.zeros((), dtype=g.dtype), g)
        return g

    def edge_sum(self, M, rp, perm=None, out=None):
        import torch
        src = M if perm is None else M[perm.long()]
        return torch.zeros(rp.numel() - 1, M.shape[1], dtype=M.dtype).index_add_(0, self._rows(rp), src)

    def transpose_graph(self, rp, col):
        import torch
        import walks
        rp_t, col_t, perm = walks.transposed_csr(rp.numpy(), col.numpy())
        return torch.from_numpy(rp_t), torch.from_numpy(col_t), torch.from_numpy(perm.astype(np.int32)), False
