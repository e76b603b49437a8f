"""The multi-head SDDMM on the host: the yardstick of tests/test_gpu_sddmm_heads.py against a dense fp64 Q_h K_h^T, the share of the
bounds the reference alone uses on every (graph, shape) the GPU file runs, the two new entry points in header, library, ctypes table,
binding and module, that aggregate_heads forms dP with ONE forward_ef_heads call, and sddmm_heads / edge_softmax_heads /
TransformerConv on a pure-torch backend against a dense fp64 model.  tests/test_gpu_sddmm_heads.py runs the kernels."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import gat_ref as G
import graphs
import sddmm_heads_ref as HR
import walks
from sddmm_heads_ref import dense_transformer_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"tcgnn_sddmm_heads_workspace_bytes": 3, "tcgnn_sddmm_heads": 9}
TOY = [(name, rp, col) for name, rp, col in graphs.edge_case_graphs() if len(rp) - 1 <= 48]
TOY.append(("directed_n64", *graphs.powerlaw_graph(64, 5, seed=12, symmetric=False)))
GPU_GRAPHS = HR.gpu_graphs()


@pytest.mark.parametrize("shape", [(1, 16), (3, 8), (4, 32), (3, 12)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("case", TOY, ids=[c[0] for c in TOY])
def test_the_reference_is_the_dense_product_read_at_the_edges(case, shape):
    name, rp, col = case
    H, F = shape
    n, nnz = len(rp) - 1, len(col)
    X, Z = HR.heads_data(name, n, H, F)
    assert X.shape == Z.shape == (n, H * F) and X.dtype == Z.dtype == np.float32 and not np.array_equal(X, Z)
    assert all(np.array_equal(a, b) for a, b in zip((X, Z), HR.heads_data(name, n, H, F)))     # seeded per (name, H, F)
    ref, r64, s64 = HR.heads_reference(rp, col, X, Z, H)
    assert ref.shape == r64.shape == s64.shape == (H, nnz)
    dense = HR.dense_heads_f64(rp, col, X, Z, H)
    scale = HR.dense_heads_f64(rp, col, np.abs(X), np.abs(Z), H)
    assert np.abs(r64 - dense).max(initial=0) <= 1e-12 * (scale.max(initial=0) + 1) and np.abs(s64 - scale).max(initial=0) <= 1e-12 * (scale.max(initial=0) + 1)
    rounded = HR.dense_heads_f64(rp, col, walks.round_tf32(X), walks.round_tf32(Z), H)
    assert np.abs(ref - rounded).max(initial=0) <= 1e-12 * (scale.max(initial=0) + 1)
    if n > 16:
        cut, c64, _ = HR.heads_reference(rp, col, X, Z, H, rows=16)
        e = int(rp[16])
        assert not cut[:, e:].any() and not c64[:, e:].any() and np.array_equal(cut[:, :e], ref[:, :e])


@pytest.mark.parametrize("shape", sorted(HR.SHAPES), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(GPU_GRAPHS))
def test_the_reference_alone_uses_a_small_share_of_each_bound_on_the_gpu_cases(name, shape):
    """tests/test_structures_cpu.py's rule on every (graph, shape) of the GPU file: the TF32-mode reference, rounded to the fp32 a
    kernel returns (its dots are fp64 already: that rounding is all the noise it has), uses at most a quarter of the 1e-3 and TIGHT
    bounds, and its distance from the fp64 contract - operand rounding - at most half of 2^-9."""
    H, F = shape
    rp, col = GPU_GRAPHS[name]
    n = len(rp) - 1
    X, Z = HR.heads_data(name, n, H, F)
    ref, r64, s64 = HR.heads_reference(rp, col, X, Z, H, HR.rows_handed_over(name, n))
    if not len(col):
        return
    as32 = ref.astype(np.float32).astype(np.float64)
    fig = (float((np.abs(as32 - ref) / np.maximum(1.0, np.abs(ref))).max()), float((np.abs(as32 - ref) / (s64 + 1.0)).max()),
           float((np.abs(ref - r64) / (s64 + 1.0)).max()))
    print("FIG reference alone %s %dx%d: bar %.2e tight %.2e fp64 %.2e" % (name, H, F, *fig))
    assert fig[0] <= walks.TOL * walks.NOISE_SHARE and fig[1] <= walks.TIGHT * walks.NOISE_SHARE and fig[2] <= walks.LOOSE * walks.ROUNDING_SHARE, fig


def test_shapes_are_the_ones_the_kernel_can_go_wrong_at():
    assert set(HR.SHAPES) == {(1, 16), (3, 8), (8, 8), (4, 16), (4, 32), (2, 64), (5, 8), (7, 16), (2, 16), (2, 32), (3, 32), (5, 24), (3, 12), (9, 16), (2, 136)}
    assert len(GPU_GRAPHS) == 16
    assert HR.fused_expected(3, 8, True, 4, 1) and not HR.fused_expected(3, 8, False, 100, 9) and not HR.fused_expected(3, 8, True, 3, 1)
    assert not HR.fused_expected(1, 16, True, 100, 9) and not HR.fused_expected(9, 16, True, 100, 9) and not HR.fused_expected(5, 24, True, 100, 9)


@pytest.mark.parametrize("shape", HR.WIDE_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("which", ["X", "Z"])
def test_the_fp32_way_restated_passes_the_judge_on_the_wide_cases(which, shape):
    """the condition of the GPU file's range-guard case: what sddmm_heads_csr_kernel computes - restated in numpy - is inside the
    bounds of the reference on the input with one row x 2^30, and that input holds elements the fp16 image of its operand loses"""
    from test_gpu_parity import assert_parity
    rp, col, X, Z, ref = HR.wide_case(which, shape)
    A = X if which == "X" else Z
    assert np.log2(np.abs(A).max()) - np.log2(np.abs(A[A != 0]).min()) > 29
    got = HR.fp32_way(rp, col, X, Z, shape[0])
    assert_parity(got.astype(np.float64), *ref, "the fp32 way restated, a row of %s x 2^30" % which, unit_scale=False)


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
    assert re.search(r'm\.def\("forward_ef_heads"', binding)
    import TCGNN
    assert callable(TCGNN.forward_ef_heads) and "forward_ef_heads" in TCGNN.__all__
    assert lib.tcgnn_abi_version() == 1          # (an added entry point does not move the ABI version)


def test_degenerate_calls_answer_without_a_device():
    import tcgnn_capi
    lib = tcgnn_capi.lib
    assert lib.tcgnn_sddmm_heads_workspace_bytes(None, 8, 8) == 0
    assert lib.tcgnn_sddmm_heads(None, None, None, None, 8, 8, None, 0, None) == 1       # TCGNN_ERR_INVALID_ARG
    assert b"tcgnn_sddmm_heads" in lib.tcgnn_last_error()


# ---- the operators on stand-in backends -----------------------------------------------------------------------------------------------------

class _Torch(G.TorchBackend):
    """the pure-torch backend, its edge_softmax taking out= as the product's does (and ignoring it, as its backward does)"""

    def edge_softmax(self, s, rp, beta=None, out=None):
        return super().edge_softmax(s, rp, beta)

    def forward_heads(self, X, rp, col, att, bp, e2c, e2r, heads, transpose=False):
        F = X.shape[1] // heads
        return [torch.cat([self.forward_AGNN(X[:, h * F:(h + 1) * F], rp, col, att[h].view(1, -1), transpose=transpose)[0] for h in range(heads)], 1)]


class _Counting(_Torch):
    """... plus a forward_ef_heads of its own, and a count of both SDDMM calls"""

    def __init__(self):
        self.calls = []

    def forward_ef2(self, *a):
        self.calls.append("forward_ef2")
        return super().forward_ef2(*a)

    def forward_ef_heads(self, X, Z, rp, col, bp, e2c, e2r, heads):
        self.calls.append("forward_ef_heads")
        F = X.shape[1] // heads
        return [torch.stack([super(_Counting, self).forward_ef2(X[:, h * F:(h + 1) * F], Z[:, h * F:(h + 1) * F], rp, col)[0] for h in range(heads)])]


class _Lacking(_Torch):
    """... without forward_ef_heads: set_backend gives it the per-head definition"""

    def __init__(self):
        self.calls = []

    def forward_ef2(self, *a):
        self.calls.append("forward_ef2")
        return super().forward_ef2(*a)


def _directed64():
    return graphs.powerlaw_graph(64, 5, seed=12, symmetric=False)


def _meta(rp, col):
    return (torch.from_numpy(rp), torch.from_numpy(col), None, None, None)


@pytest.fixture()
def backend():
    import tcgnn_layers as L
    old = L._backend

    def install(b):
        L.set_backend(b)
        return b
    yield install
    L.set_backend(old)


def _dP_dense(rp, col, dY, Z, H):
    return torch.from_numpy(HR.dense_heads_f64(rp, col, dY.numpy(), Z.numpy(), H))


def test_aggregate_heads_forms_dP_with_one_forward_ef_heads_call(backend):
    import tcgnn_edge_ops as E
    rp, col = _directed64()
    n, nnz = len(rp) - 1, len(col)
    rec = backend(_Counting())
    torch.manual_seed(0)
    P = torch.randn(3, nnz, dtype=torch.float64, requires_grad=True)
    Z = torch.randn(n, 15, dtype=torch.float64, requires_grad=True)
    w = torch.randn(n, 15, dtype=torch.float64)
    Y = E.aggregate_heads(P, Z, _meta(rp, col))
    assert rec.calls == []
    dP, = torch.autograd.grad((Y * w).sum(), (P,))
    assert rec.calls == ["forward_ef_heads"]
    want = _dP_dense(rp, col, w, Z.detach(), 3)
    assert float((dP - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_a_backend_without_the_call_gets_the_per_head_definition(backend):
    import tcgnn_edge_ops as E
    rp, col = _directed64()
    n, nnz = len(rp) - 1, len(col)
    lacking = _Lacking()
    assert not hasattr(lacking, "forward_ef_heads")
    backend(lacking)
    assert callable(lacking.forward_ef_heads)
    torch.manual_seed(0)
    P = torch.randn(3, nnz, dtype=torch.float64, requires_grad=True)
    Z = torch.randn(n, 15, dtype=torch.float64)
    w = torch.randn(n, 15, dtype=torch.float64)
    dP, = torch.autograd.grad((E.aggregate_heads(P, Z, _meta(rp, col)) * w).sum(), (P,))
    assert lacking.calls == ["forward_ef2"] * 3
    want = _dP_dense(rp, col, w, Z, 3)
    assert float((dP - want).abs().max()) <= 1e-12 * float(want.abs().max())
    import TCGNN
    assert "forward_ef_heads" in vars(TCGNN)          # (the product's own module never takes the fallback: it has the name)


def _close(got, want, what, tol=1e-9, floor=0.0):
    err, top = float((got.detach() - want.detach()).abs().max()), max(float(want.detach().abs().max()), floor)
    assert got.shape == want.shape and err <= tol * max(top, 1e-300), "%s: %.3e of the largest entry" % (what, err / max(top, 1e-300))


def test_sddmm_heads_and_edge_softmax_heads_have_the_gradients_of_the_dense_formulas(backend):
    import tcgnn_edge_ops as E
    backend(_Torch())
    rp, col = _directed64()
    n, nnz = len(rp) - 1, len(col)
    A = G.dense_adjacency(rp, col)
    rows = torch.from_numpy(np.repeat(np.arange(n), np.diff(rp))).long()
    cols = torch.from_numpy(col).long()
    H, F = 3, 5
    torch.manual_seed(1)
    X = torch.randn(n, H * F, dtype=torch.float64, requires_grad=True)
    Z = torch.randn(n, H * F, dtype=torch.float64, requires_grad=True)
    w = torch.randn(H, nnz, dtype=torch.float64)
    beta = torch.tensor([0.37], dtype=torch.float64)
    S = E.sddmm_heads(X, Z, _meta(rp, col), H)
    P = E.edge_softmax_heads(S, torch.from_numpy(rp), beta)
    assert S.shape == P.shape == (H, nnz)
    got = torch.autograd.grad((P * w).sum() + (S * w).sum(), (X, Z))
    Xd, Zd = X.detach().clone().requires_grad_(True), Z.detach().clone().requires_grad_(True)
    Sd, Pd = [], []
    for h in range(H):
        c = slice(h * F, (h + 1) * F)
        full = Xd[:, c] @ Zd[:, c].t()
        Sd.append(full[rows, cols])
        soft = torch.softmax((0.37 * full).masked_fill(A == 0, float("-inf")).masked_fill(A.sum(1, keepdim=True) == 0, 0.0), dim=1)
        Pd.append(soft[rows, cols])
    Sd, Pd = torch.stack(Sd), torch.stack(Pd)
    want = torch.autograd.grad((Pd * w).sum() + (Sd * w).sum(), (Xd, Zd))
    _close(S, Sd, "sddmm_heads")
    _close(P, Pd, "edge_softmax_heads")
    _close(got[0], want[0], "dX")
    _close(got[1], want[1], "dZ")
    with pytest.raises(RuntimeError, match="heads"):
        E.sddmm_heads(X, Z, _meta(rp, col), 4)


@pytest.mark.parametrize("root_weight", [True, False], ids=["root", "noroot"])
@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
@pytest.mark.parametrize("heads", [1, 3])
def test_transformer_layer_equals_the_dense_model_in_values_and_gradients(backend, heads, concat, root_weight):
    import tcgnn_layers as L
    backend(_Torch())
    rp, col = _directed64()
    assert (np.diff(rp) == 0).any()                         # (nodes without incoming edges: the root term and the bias only)
    n = len(rp) - 1
    A = G.dense_adjacency(rp, col)
    torch.manual_seed(2)
    layer = L.TransformerConv(10, 4, heads=heads, concat=concat, root_weight=root_weight).double()
    for b in (layer.bias_q, layer.bias_k, layer.bias_v, layer.bias):
        b.data.normal_()
    assert (layer.weights_root is not None) == root_weight and layer.weights_q.shape == (10, heads * 4)
    X = torch.randn(n, 10, dtype=torch.float64, requires_grad=True)
    w = torch.randn(n, heads * 4 if concat else 4, dtype=torch.float64)
    params = [p for p in layer.parameters()]
    Y = layer(X, *_meta(rp, col))
    got = torch.autograd.grad((Y * w).sum(), [X] + params)
    Yd = dense_transformer_model(A, X, layer, heads)
    want = torch.autograd.grad((Yd * w).sum(), [X] + params)
    _close(Y, Yd, "Y")
    none = torch.from_numpy(np.diff(rp) == 0)
    alone = (X @ layer.weights_root if root_weight else torch.zeros_like(Y)) + layer.bias
    _close(Y[none], alone[none], "rows without edges")
    # (d bias_k is zero in exact arithmetic - a shift of every key moves a row's scores by one constant, which the softmax drops -
    #  so it is judged on the scale of the other bias gradients, not on its own rounding noise)
    floor = max(float(w_.abs().max()) for w_, (k, _) in zip(want[1:], layer.named_parameters()) if k.startswith("bias"))
    for g, wnt, name in zip(got, want, ["X"] + [k for k, _ in layer.named_parameters()]):
        _close(g, wnt, "d" + name, floor=floor if name == "bias_k" else 0.0)


def test_transformer_layer_initialisation_and_harness():
    import tcgnn_harness as H
    import tcgnn_layers as L
    torch.manual_seed(0)
    layer = L.TransformerConv(12, 8, heads=4)
    bound = math.sqrt(6.0 / (12 + 32))
    for w in (layer.weights_q, layer.weights_k, layer.weights_v, layer.weights_root):
        assert w.shape == (12, 32) and float(w.detach().abs().max()) <= bound and float(w.detach().abs().max()) > 0.5 * bound
    assert all(not b.any() for b in (layer.bias_q, layer.bias_k, layer.bias_v, layer.bias))
    assert abs(float(layer.scale) - 8 ** -0.5) < 1e-7 and "scale" not in layer.state_dict()
    bare = L.TransformerConv(12, 8, heads=4, concat=False, root_weight=False, bias=False)
    assert bare.weights_root is None and bare.bias is None and bare.bias_q is None and len(list(bare.parameters())) == 3
    with pytest.raises(ValueError, match="heads"):
        L.TransformerConv(4, 4, heads=0)
    args = H.build_parser().parse_args(["--model", "transformer", "--heads", "4"])
    assert args.model == "transformer" and args.heads == 4
    meta = (torch.zeros(2, dtype=torch.int32),) * 5
    with pytest.raises(ValueError, match="multiple"):
        H.time_training("transformer", meta, torch.zeros(1, 4), torch.zeros(1).long(), 4, 6, 2, 2, 0, heads=4)
    net = H.Net(lambda a, b: L.TransformerConv(a, b // 4, heads=4), 12, 8, 5, 3, out_cls=L.TransformerConv)
    assert net.conv1.weights_q.shape == (12, 8) and net.hidden_layers[0].weights_q.shape == (8, 8) and net.conv2.weights_q.shape == (8, 5)
    assert net.conv1.heads == 4 and net.conv2.heads == 1
    old = L._backend
    L.set_backend(_Torch())
    try:
        rp, col = _directed64()
        out = net.eval()(torch.randn(64, 12), _meta(rp, col))          # the harness' model runs a transformer layer as its output layer
        assert out.shape == (64, 5) and torch.isfinite(out).all()
    finally:
        L.set_backend(old)
