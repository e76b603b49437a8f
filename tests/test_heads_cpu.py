"""The multi-head edge-valued SpMM on the host: the yardstick of tests/test_gpu_heads.py against a dense fp64 product, the two new
entry points in header, library, ctypes table, binding and module, their degenerate calls (what is reachable without a device), and
that aggregate_heads is ONE backend call forward and one over A^T backward.  tests/test_gpu_heads.py runs the kernels."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gat_ref as G
import graphs
import heads_ref as HR
import walks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"tcgnn_spmm_heads_workspace_bytes": 3, "tcgnn_spmm_heads": 9}
TOY = [(name, rp, col) for name, rp, col in graphs.edge_case_graphs() if len(rp) - 1 <= 48]
TOY.append(("directed_n64", *graphs.powerlaw_graph(64, 5, seed=12, symmetric=False)))


@pytest.mark.parametrize("shape", [(1, 16), (3, 8), (5, 24), (3, 12)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("case", TOY, ids=[c[0] for c in TOY])
def test_the_reference_is_the_dense_product_head_by_head(case, shape):
    name, rp, col = case
    H, F = shape
    n, nnz = len(rp) - 1, len(col)
    Z, P = HR.heads_data(name, n, nnz, H, F)
    assert Z.shape == (n, H * F) and P.shape == (H, nnz) and Z.dtype == P.dtype == np.float32
    Z2, P2 = HR.heads_data(name, n, nnz, H, F)
    assert np.array_equal(Z, Z2) and np.array_equal(P, P2)                    # seeded per (name, H, F)
    if nnz:
        assert not np.array_equal(P, HR.heads_data(name + "x", n, nnz, H, F)[1])
    ref, r64, s64 = HR.heads_reference(rp, col, Z, P)
    dense = HR.dense_heads_f64(rp, col, Z, P)
    scale = HR.dense_heads_f64(rp, col, np.abs(Z), np.abs(P))
    assert np.abs(r64 - dense).max() <= 1e-12 * (scale.max() + 1) and np.abs(s64 - scale).max() <= 1e-12 * (scale.max() + 1)
    # the TF32-mode part: the dense product of the ROUNDED operands up to accumulation noise, the unrounded one up to operand rounding
    rounded = HR.dense_heads_f64(rp, col, walks.round_tf32(Z), walks.round_tf32(P))
    assert (np.abs(ref - rounded) / (s64 + 1)).max() <= walks.TIGHT * walks.NOISE_SHARE
    assert (np.abs(ref - r64) / (s64 + 1)).max() <= walks.LOOSE * walks.ROUNDING_SHARE
    assert not ref[np.diff(rp) == 0].any()
    # A^T: the reference on the transposed CSR with permuted values is the dense product with every head's matrix transposed
    (tref, t64, ts64), tzero = HR.transposed_reference(rp, col, Z, P)
    rows = np.repeat(np.arange(n), np.diff(rp))
    want = np.zeros((n, H * F))
    for h in range(H):
        A = np.zeros((n, n))
        np.add.at(A, (rows, col), P[h].astype(np.float64))
        want[:, h * F:(h + 1) * F] = A.T @ Z[:, h * F:(h + 1) * F].astype(np.float64)
    assert np.abs(t64 - want).max() <= 1e-12 * (ts64.max() + 1)
    assert np.array_equal(tzero, np.bincount(col, minlength=n) == 0) and not tref[tzero].any()
    cut, _, _ = HR.heads_reference(rp, col, Z, P, rows=16)
    assert not cut[16:].any() and np.array_equal(cut[:16], ref[:16])


def test_the_fp32_way_restated_passes_the_judge_on_the_wide_case():
    """the condition of test_gpu_heads.test_range_guard_takes_the_whole_call: on its input the range guard's rule holds (restated from
    include/tcgnn.h "Operand range"), and what the fallback kernels compute - restated in numpy - is inside the three bounds of the
    oracle.  Were it not, the graph or the seed of the case would change, not a bound."""
    name, H, F, Z, P = HR.wide_case()
    rp, col = {n: (r, c) for n, r, c in graphs.edge_case_graphs()}[name]
    k = int(np.diff(rp).max())
    nz = np.abs(P[P != 0])
    assert np.log2(nz.max()) - np.log2(nz.min()) > 29                                            # values that lose bits under one scale
    assert np.floor(np.log2(nz.max())) + np.floor(np.log2(np.abs(Z).max())) >= 28 - np.ceil(np.log2(k))
    got = HR.fp32_way(rp, col, Z, P)
    assert not walks.judge(name, got, *HR.heads_reference(rp, col, Z, P), "the fp32 way restated", walks.zero_rows(name, rp))


def test_shapes_are_the_ones_the_kernel_can_go_wrong_at():
    assert set(HR.SHAPES) == {(1, 16), (2, 8), (3, 8), (8, 8), (5, 24), (4, 32), (9, 16), (3, 12)}


def test_new_entry_points_are_declared_exported_and_bound():
    import tcgnn_capi
    lib = ctypes.CDLL(tcgnn_capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "tcgnn.h")).read()
    binding = open(os.path.join(ROOT, "integration", "TCGNN_binding.cpp")).read()
    for name, nargs in ENTRY_POINTS.items():
        assert name in tcgnn_capi.SIGNATURES and len(tcgnn_capi.SIGNATURES[name][1]) == nargs, name
        assert getattr(lib, name) is not None
        assert re.search(r"\b(int|size_t) %s\(" % name, header), name
        assert name in binding, name
    assert re.search(r'm\.def\("forward_heads"', binding)
    import TCGNN
    assert callable(TCGNN.forward_heads) and "forward_heads" in TCGNN.__all__
    assert lib.tcgnn_abi_version() == 1          # (an added entry point does not move the ABI version: the GAT entries did not)


def test_degenerate_calls_answer_without_a_device():
    import tcgnn_capi
    lib = tcgnn_capi.lib
    assert lib.tcgnn_spmm_heads_workspace_bytes(None, 8, 8) == 0
    assert lib.tcgnn_spmm_heads(None, None, None, None, 8, 8, None, 0, None) == 1       # TCGNN_ERR_INVALID_ARG
    assert b"tcgnn_spmm_heads" in lib.tcgnn_last_error()


class _Recorder(G.TorchBackend):
    """the pure-torch backend plus a forward_heads that says it was called"""

    def __init__(self):
        self.calls = []

    def forward_AGNN(self, *a, **k):
        self.calls.append(("forward_AGNN", k.get("transpose", False)))
        return super().forward_AGNN(*a, **k)

    def forward_heads(self, X, rp, col, att, bp, e2c, e2r, heads, transpose=False):
        self.calls.append(("forward_heads", transpose))
        F = X.shape[1] // heads
        return [torch.cat([super(_Recorder, self).forward_AGNN(X[:, h * F:(h + 1) * F], rp, col, att[h].view(1, -1), transpose=transpose)[0]
                           for h in range(heads)], 1)]


def test_aggregate_heads_is_one_backend_call_each_way():
    import tcgnn_edge_ops as E
    import tcgnn_layers as L
    rp, col = graphs.powerlaw_graph(64, 5, seed=12, symmetric=False)
    n, nnz = len(rp) - 1, len(col)
    meta = (torch.from_numpy(rp), torch.from_numpy(col), None, None, None)
    old, rec = L._backend, _Recorder()
    L.set_backend(rec)
    try:
        torch.manual_seed(0)
        P = torch.randn(3, nnz, dtype=torch.float64, requires_grad=True)
        Z = torch.randn(n, 15, dtype=torch.float64, requires_grad=True)
        Y = E.aggregate_heads(P, Z, meta)
        assert rec.calls == [("forward_heads", False)]
        dP, dZ = torch.autograd.grad(Y.sum(), (P, Z))
        assert [c for c in rec.calls if c[0] != "forward_heads"] == [] and rec.calls.count(("forward_heads", True)) == 1 and len(rec.calls) == 2
        want = torch.from_numpy(HR.dense_heads_f64(rp, col, Z.detach().numpy(), P.detach().numpy()))
        assert float((Y.detach() - want).abs().max()) <= 1e-12 * float(want.abs().max())
        assert dP.shape == P.shape and dZ.shape == Z.shape
    finally:
        L.set_backend(old)
