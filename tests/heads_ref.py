"""What tests/test_heads_cpu.py and tests/test_gpu_heads.py share: the data and the reference of a multi-head edge-valued SpMM
(tcgnn_spmm_heads / TCGNN.forward_heads), Y[:, hF:(h+1)F] = A_val(P[h]) Z[:, hF:(h+1)F].  The reference is the project's own oracle,
head by head - O.spmm_val(..., round_mode=ROUND_TF32) and O.spmm_f64 - concatenated over the heads; walks.judge / assert_parity
judge against it with the project's three bounds, unchanged.  No GPU needed to import."""
import zlib

import numpy as np

import graphs
import walks
from oracle import oracle as O

# (H, F) -> what the case is there for (tests/test_gpu_heads.py runs every one on every graph)
SHAPES = {
    (1, 16): "one head: tcgnn_spmm_val itself, bit-equal to forward_AGNN",
    (2, 8): "two heads in one 16-column slice",
    (3, 8): "the layer test's shape: the last slice half empty, D = 24 padded to 32",
    (8, 8): "two passes of four heads, every slice shared by two heads",
    (5, 24): "head boundaries alternately mid-slice; passes of 2 + 2 + 1 heads",
    (4, 32): "two passes of two heads, heads own whole slices",
    (9, 16): "144 columns: passes of 4 + 4 + 1 whole heads",
    (3, 12): "F no multiple of 8: head by head inside the library",
}


def heads_data(name, n, nnz, H, F):
    """Standard-normal Z [n, H F] and P [H, nnz] (walks.case_data's kind), seeded per (name, H, F)."""
    rng = np.random.default_rng(zlib.crc32(("%s/%d/%d" % (name, H, F)).encode()))
    return rng.standard_normal((n, H * F)).astype(np.float32), rng.standard_normal((H, nnz)).astype(np.float32)


def heads_reference(rp, col, Z, P, rows=None):
    """(ref_tf32, ref64, scale64), each [n, H F]: the oracle head by head.  rows: rows from this one on are zeros (a plan that was
    handed fewer windows than the graph has leaves them as zeros_like does)."""
    n, nnz = len(rp) - 1, len(col)
    H = P.shape[0]
    F = Z.shape[1] // H
    assert Z.shape == (n, H * F) and P.shape == (H, nnz)
    ref, r64, s64 = np.zeros((n, H * F), np.float32), np.zeros((n, H * F)), np.zeros((n, H * F))
    if nnz:
        bp, e2c, e2r = walks.host_meta(rp, col)
        for h in range(H):
            cols = slice(h * F, (h + 1) * F)
            Zh, Ph = np.ascontiguousarray(Z[:, cols]), np.ascontiguousarray(P[h])
            ref[:, cols] = O.spmm_val(Zh, rp, col, Ph, bp, e2c, e2r, round_mode=O.ROUND_TF32)
            r64[:, cols], s64[:, cols] = O.spmm_f64(Zh, rp, col, Ph)
    if rows is not None and rows < n:
        ref[rows:] = 0; r64[rows:] = 0; s64[rows:] = 0
    return ref, r64, s64


def transposed_reference(rp, col, Z, P, rows=None):
    """the same for A^T: on walks.transposed_csr with every head's values permuted into A^T's order -> (refs, rows of A^T without edges)"""
    trp, tcol, perm = walks.transposed_csr(rp, col)
    return heads_reference(trp, tcol, Z, np.ascontiguousarray(P[:, perm]), rows), np.diff(trp) == 0


def dense_heads_f64(rp, col, Z, P):
    """the dense fp64 product, head by head: what heads_reference's fp64 part must equal"""
    n = len(rp) - 1
    H = P.shape[0]
    F = Z.shape[1] // H
    rows = np.repeat(np.arange(n), np.diff(rp))
    out = np.zeros((n, H * F))
    for h in range(H):
        A = np.zeros((n, n))
        np.add.at(A, (rows, col), P[h].astype(np.float64))
        out[:, h * F:(h + 1) * F] = A @ Z[:, h * F:(h + 1) * F].astype(np.float64)
    return out


def wide_case():
    """(name, H, F, Z, P) with head 2 of P scaled by 2^24 on uniform_n1000: the range guard's edge-valued rule holds for the call -
    max|P| max|Z| is about 2^27, far beyond 2^28 / the longest row, and P holds values more than 2^28 below its largest - so the fp32
    way does the work (spmm_wide_fallback_kernel's body, per head)."""
    name, H, F = "uniform_n1000", 4, 8
    rp, col = {n: (r, c) for n, r, c in graphs.edge_case_graphs()}[name]
    Z, P = heads_data(name + "/wide", len(rp) - 1, len(col), H, F)
    P[2] *= np.float32(2.0 ** 24)
    return name, H, F, Z, P


def fp32_way(rp, col, Z, P):
    """spmm_wide_fallback_kernel restated, head by head: operands rounded to 10 mantissa bits, the products (exact in fp32) summed in
    fp32 in CSR order"""
    n = len(rp) - 1
    H = P.shape[0]
    F = Z.shape[1] // H
    Zr, Pr = walks.round_tf32(Z), walks.round_tf32(P)
    out = np.zeros((n, H * F), np.float32)
    deg = np.diff(rp)
    for k in range(int(deg.max()) if n else 0):
        live = np.nonzero(deg > k)[0]
        e = rp[live] + k
        for h in range(H):
            cols = slice(h * F, (h + 1) * F)
            out[live, cols] = (out[live, cols] + (Pr[h, e][:, None] * Zr[col[e], cols]).astype(np.float32)).astype(np.float32)
    return out
