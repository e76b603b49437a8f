"""What tests/test_sddmm_heads_cpu.py and tests/test_gpu_sddmm_heads.py share: the shapes, the data and the reference of the
multi-head SDDMM (tcgnn_sddmm_heads / TCGNN.forward_ef_heads), ef[h, e] = <X[row e, hF:(h+1)F], Z[col e, hF:(h+1)F]>.  The reference
goes head by head through edge_ops_ref.sddmm2_tf32 and sddmm2_f64, stacked to [H, E]; test_gpu_parity.assert_parity judges against it
with the project's three bounds, unchanged.  (Its 10-bit operand rounding is scale-free, so one power-of-two scale per operand
instead of one per head does not move it.)  No GPU needed to import."""
import math
import zlib

import numpy as np

import edge_ops_ref as R
import graphs
import walks

# (H, F) -> what the case is there for (tests/test_gpu_sddmm_heads.py runs every one on every graph)
SHAPES = {
    (1, 16): "one head: tcgnn_sddmm2 itself, bit-equal to forward_ef2",
    (3, 8): "one pass of three heads in one K-step whose last column group is empty (24 columns padded to 32)",
    (8, 8): "two passes of four heads: four heads share a K-step",
    (4, 16): "two heads share a K-step, two K-steps",
    (4, 32): "a K-step per head",
    (2, 64): "two K-steps per head",
    (5, 8): "passes of 3 + 2 heads: two launches, the second from head 3 on",
    (7, 16): "passes of 4 + 3 heads: the second pass's whole-line gathers start at column 64, its last K-step is half empty",
    (2, 16): "one pass of two heads in one K-step",
    (2, 32): "one pass of two heads, a K-step each",
    (3, 32): "three K-steps: the landing layout without whole-line gathers, a K-step per head",
    (5, 24): "F not a fused width: head by head inside the library",
    (3, 12): "F no multiple of 8: head by head inside the library",
    (9, 16): "144 columns: beyond the fused walk's 128, head by head",
    (2, 136): "heads wider than 128 columns: head by head on sddmm_wide_kernel",
}
FUSED_WIDTHS = (8, 16, 32, 64)


def fused_expected(H, F, canonical, nnz, windows):
    """what include/tcgnn.h says of the route: the fused walk for these shapes on a canonical plan with windows and E >= 4"""
    return H >= 2 and F in FUSED_WIDTHS and H * F <= 128 and canonical and nnz >= 4 and windows > 0


def heads_data(name, n, H, F):
    """Standard-normal X and Z [n, H F] (walks.case_data's kind), seeded per (name, H, F)."""
    rng = np.random.default_rng(zlib.crc32(("sddmm/%s/%d/%d" % (name, H, F)).encode()))
    return rng.standard_normal((n, H * F)).astype(np.float32), rng.standard_normal((n, H * F)).astype(np.float32)


def heads_reference(rp, col, X, Z, H, rows=None):
    """(ref_tf32, ref64, scale64), each [H, E].  rows: the scores of the edges of rows from this one on are zeros (a plan that was
    handed fewer windows than the graph has leaves them so)."""
    n, nnz = len(rp) - 1, len(col)
    F = X.shape[1] // H
    assert X.shape == Z.shape == (n, H * F)
    ref, r64, s64 = np.zeros((H, nnz)), np.zeros((H, nnz)), np.zeros((H, nnz))
    for h in range(H):
        cols = slice(h * F, (h + 1) * F)
        ref[h], _ = R.sddmm2_tf32(X[:, cols], Z[:, cols], rp, col)
        r64[h], s64[h] = R.sddmm2_f64(X[:, cols], Z[:, cols], rp, col)
    if rows is not None and rows < n:
        cut = int(rp[rows])
        ref[:, cut:] = 0; r64[:, cut:] = 0; s64[:, cut:] = 0
    return ref, r64, s64


def rows_handed_over(name, n):
    return min(walks.windows_handed_over(name, n) * 16, n)


def dense_heads_f64(rp, col, X, Z, H):
    """the dense fp64 Q_h K_h^T read at the edges, head by head: what heads_reference's fp64 part must equal"""
    n = len(rp) - 1
    F = X.shape[1] // H
    rows = np.repeat(np.arange(n), np.diff(rp))
    out = np.zeros((H, len(col)))
    for h in range(H):
        cols = slice(h * F, (h + 1) * F)
        out[h] = (X[:, cols].astype(np.float64) @ Z[:, cols].astype(np.float64).T)[rows, col]
    return out


def gpu_graphs():
    """the graphs of tests/test_gpu_heads.py: edge_case_graphs() (an empty middle window among them), hub rows, four wavefronts per
    window, E = 1, E = 5, unsorted rows (a non-canonical plan), short metadata (windows that are not handed over)"""
    g = {name: (rp, col) for name, rp, col in graphs.edge_case_graphs()}
    g["hub_rows_n2500"] = graphs.hub_rows_graph(2500, seed=77)
    g["dense_n3000_deg150"] = graphs.uniform_graph(3000, 150, seed=2)
    g["five_edges_n40"] = graphs.csr_from_edges(np.array([0, 3, 3, 17, 39]), np.array([5, 3, 30, 17, 0]), 40)
    b = {name: (rp, col) for name, rp, col in graphs.boundary_graphs()}
    for name in ("single_edge_corner_n5000", "unsorted_rows_n4100", "short_metadata_n4100"):
        g[name] = b[name]
    return g


# the range guard at level 2: one row of X, then of Z, x 2^30 on this graph at (4, 8) - the fused route - and at (3, 12), head by head
WIDE = ("uniform_n1000", 4, 8)
WIDE_SHAPES = ((4, 8), (3, 12))


def wide_case(which, shape=WIDE[1:]):
    """(rp, col, X, Z, references) with the longest row's row of `which` scaled by 2^30: a power of two on a row scales the rounded
    operands, every product and every sum of the edges that touch it exactly"""
    name, (H, F) = WIDE[0], shape
    rp, col = {n: (r, c) for n, r, c in graphs.edge_case_graphs()}[name]
    n = len(rp) - 1
    X, Z = heads_data(name + "/wide", n, H, F)
    hot = int(np.argmax(np.diff(rp)))
    ref = heads_reference(rp, col, X, Z, H)
    (X if which == "X" else Z)[hot] *= np.float32(2.0 ** 30)
    edge_rows = np.repeat(np.arange(n), np.diff(rp))
    factor = np.where((edge_rows if which == "X" else col) == hot, 2.0 ** 30, 1.0)
    return rp, col, X, Z, tuple(a * factor for a in ref)


def fp32_way(rp, col, X, Z, H):
    """sddmm_heads_csr_kernel restated: operands rounded to 10 mantissa bits, per head the F products (exact in fp32) summed in fp32 -
    lane d takes columns d, d + 64, ... in order, then the 64 lanes in a butterfly (xor 32, 16, ... 1)"""
    n = len(rp) - 1
    F = X.shape[1] // H
    rows = np.repeat(np.arange(n), np.diff(rp))
    Xr, Zr = walks.round_tf32(X), walks.round_tf32(Z)
    out = np.zeros((H, len(col)), np.float32)
    for h in range(H):
        cols = slice(h * F, (h + 1) * F)
        prod = (Xr[rows, cols] * Zr[col, cols]).astype(np.float32)
        lanes = np.zeros((len(col), 64), np.float32)
        for d in range(F):
            lanes[:, d % 64] = (lanes[:, d % 64] + prod[:, d]).astype(np.float32)
        off = 32
        while off:
            lanes = (lanes + lanes[:, np.arange(64) ^ off]).astype(np.float32)
            off >>= 1
        out[h] = lanes[:, 0]
    return out


# ---- the dense fp64 model of TransformerConv ---------------------------------------------------------------------------------------------

def dense_transformer_model(A, X, layer, heads):
    """TransformerConv on a dense 0/1 adjacency matrix A [n, n] (rows = destination nodes) in torch, differentiable in X and in the
    layer's parameters: per head softmax over each row's edges of Q_h K_h^T / sqrt(F), Y_h = P_h V_h, heads concatenated or averaged,
    the root term and the bias added.  Rows without edges give root term and bias only."""
    import torch

    def lin(W, b):
        Y = X @ W
        return Y + b if b is not None else Y
    Q, K, V = lin(layer.weights_q, layer.bias_q), lin(layer.weights_k, layer.bias_k), lin(layer.weights_v, layer.bias_v)
    F = Q.shape[1] // heads
    none = A.sum(1, keepdim=True) == 0
    outs = []
    for h in range(heads):
        c = slice(h * F, (h + 1) * F)
        S = (Q[:, c] @ K[:, c].t()) / math.sqrt(F)
        S = S.masked_fill(A == 0, float("-inf")).masked_fill(none, 0.0)
        P = torch.where(A != 0, torch.softmax(S, dim=1), torch.zeros_like(S))
        outs.append(P @ V[:, c])
    Y = torch.cat(outs, dim=1) if layer.concat else torch.stack(outs, dim=1).mean(1)
    if layer.weights_root is not None:
        Y = Y + X @ layer.weights_root
    return Y + layer.bias if layer.bias is not None else Y
