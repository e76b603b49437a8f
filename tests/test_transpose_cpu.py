"""Transposed aggregation (tcgnn_transpose_ws / tcgnn_permute_edge_values, the transpose= keyword, the layers' directed=, the
directed generators and the harness's --directed) on the host: what can be checked without a GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import graphs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"tcgnn_transpose_workspace_bytes": 3, "tcgnn_transpose_ws": 11, "tcgnn_permute_edge_values": 5}


def test_transpose_entry_points_are_declared_exported_and_bound():
    import tcgnn_capi
    lib = ctypes.CDLL(tcgnn_capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "tcgnn.h")).read()
    binding = open(os.path.join(ROOT, "integration", "TCGNN_binding.cpp")).read()
    for name, nargs in ENTRY_POINTS.items():
        assert name in tcgnn_capi.SIGNATURES and len(tcgnn_capi.SIGNATURES[name][1]) == nargs
        assert getattr(lib, name) is not None
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in binding, name


def test_generators_build_directed_graphs_on_request():
    import tcgnn_graph as G
    for gen in ("uniform", "rmat", "sbm", "sbm_reddit"):
        rp, col = G.GENERATORS[gen](3000, 30000, seed=5, directed=True)
        rp2, col2 = G.GENERATORS[gen](3000, 30000, seed=5, directed=True)
        assert torch.equal(rp, rp2) and torch.equal(col, col2), gen
        assert rp.dtype == torch.int32 and col.dtype == torch.int32 and int(rp[-1]) == col.numel()
        assert abs(col.numel() - 30000) <= 30 or gen == "rmat", (gen, col.numel())
        a = sp.csr_matrix((np.ones(col.numel()), col.numpy(), rp.numpy()), shape=(3000, 3000))
        assert a.has_canonical_format and a.diagonal().sum() == 0, gen
        assert (a != a.T).nnz > 0, gen
    rp, col, _, _ = G.synthetic_shape("reddit", scale=0.01, directed=True)
    a = sp.csr_matrix((np.ones(col.numel()), col.numpy(), rp.numpy()), shape=(rp.numel() - 1,) * 2)
    assert (a != a.T).nnz > 0


def test_harness_accepts_directed():
    import tcgnn_harness as H
    assert H.build_parser().parse_args(["--directed"]).directed is True
    assert H.build_parser().parse_args([]).directed is False


class _SciPyBackend:
    """The operators in fp64 with scipy: transpose=True multiplies by A.T (A_val.T) - the semantics the HIP backend implements"""

    def __init__(self, rp, col):
        n = len(rp) - 1
        self.rp, self.col, self.n = rp, col, n
        self.A = sp.csr_matrix((np.ones(len(col)), col, rp), shape=(n, n))

    def _mm(self, M, X):
        return torch.from_numpy(np.asarray(M @ X.detach().double().numpy()))

    def forward(self, X, *meta, transpose=False):
        return [self._mm(self.A.T if transpose else self.A, X)]

    def forward_fused(self, X, *meta, relu=False, gate=None, transpose=False):
        Xp = X * (gate > 0) if gate is not None else X
        Y = self.forward(Xp, transpose=transpose)[0]
        return [torch.relu(Y) if relu else Y]

    def forward_scaled(self, X, *meta, row_scale=None, col_scale=None, bias=None, relu=False, gate=None, transpose=False):
        Xp = X * (gate > 0) if gate is not None else X
        if col_scale is not None:
            Xp = col_scale.double()[:, None] * Xp
        Y = self.forward(Xp, transpose=transpose)[0]
        if row_scale is not None:
            Y = Y * row_scale.double()[:, None]
        if bias is not None:
            Y = Y + bias
        return [torch.relu(Y) if relu else Y]

    def forward_gemm(self, X, W, *meta, relu=False):
        Y = self.forward(X)[0] @ W
        return [torch.relu(Y) if relu else Y]

    def forward_ef(self, X, *meta):
        Xh = X.detach().double().numpy()
        rows = np.repeat(np.arange(self.n), np.diff(self.rp))
        return [torch.from_numpy((Xh[rows] * Xh[self.col]).sum(1)).float()]   # (fp32: the layer dots it with column_index.float())

    def forward_AGNN(self, X, rp, col, att, *meta, transpose=False):
        Av = sp.csr_matrix((att.detach().double().numpy()[0], self.col, self.rp), shape=(self.n, self.n))
        return [self._mm(Av.T if transpose else Av, X)]


@pytest.fixture
def directed_graph():
    rp, col = graphs.powerlaw_graph(150, 6, seed=12, symmetric=False)
    a = sp.csr_matrix((np.ones(len(col)), col, rp), shape=(150, 150))
    assert (a != a.T).nnz > 0
    return rp, col, torch.from_numpy(a.toarray())


@pytest.fixture
def scipy_layers(directed_graph):
    import tcgnn_layers as L
    rp, col, _ = directed_graph
    old = L._backend
    L.set_backend(_SciPyBackend(rp, col))
    yield L
    L.set_backend(old)


def _meta(rp, col):
    return (torch.from_numpy(rp), torch.from_numpy(col), None, None, None)


def _grads(loss_fn, *tensors):
    for t in tensors:
        t.grad = None
    loss_fn().backward()
    return [t.grad.clone() for t in tensors]


def _leaf(t):
    return t.detach().clone().requires_grad_(True)


def _same(got, want):
    for g, w in zip(got, want):
        assert torch.allclose(g, w, rtol=1e-9, atol=1e-9), (g - w).abs().max()


def test_directed_sag_and_gin_gradients_equal_autograd_of_the_dense_formula(scipy_layers, directed_graph):
    L = scipy_layers
    rp, col, A = directed_graph
    meta = _meta(rp, col)
    torch.manual_seed(0)
    x = torch.randn(150, 5, dtype=torch.float64)
    dy = torch.randn(150, 5, dtype=torch.float64)
    x1, x2 = _leaf(x), _leaf(x)
    _same(_grads(lambda: (L.SAG(*meta, directed=True)(x1) * dy).sum(), x1), _grads(lambda: ((A @ x2) * dy).sum(), x2))
    gin = L.GINConv(5, 4, directed=True).double()
    W = _leaf(gin.weights)
    dy4 = torch.randn(150, 4, dtype=torch.float64)
    x1, x2 = _leaf(x), _leaf(x)
    got = _grads(lambda: (gin(x1, *meta) * dy4).sum(), x1, gin.weights)
    _same(got, _grads(lambda: (((A @ x2) @ W) * dy4).sum(), x2, W))


@pytest.mark.parametrize("mode", ["plain", "gated", "aggregate_first"])
def test_directed_gcn_gradients_equal_autograd_of_the_dense_formula(scipy_layers, directed_graph, mode):
    L = scipy_layers
    rp, col, A = directed_graph
    meta = _meta(rp, col)
    torch.manual_seed(1)
    conv = L.GCNConv(6, 5, directed=True).double()
    W = _leaf(conv.weights)
    x = torch.randn(150, 6, dtype=torch.float64)
    dy = torch.randn(150, 5, dtype=torch.float64)
    x1, x2 = _leaf(x), _leaf(x)
    kw = {"fuse_relu": mode == "gated", "aggregate_first": mode == "aggregate_first"}
    got = _grads(lambda: (conv(x1, *meta, **kw) * dy).sum(), x1, conv.weights)

    def dense():
        y = (A @ x2) @ W if mode == "aggregate_first" else A @ (x2 @ W)
        return ((torch.relu(y) if mode == "gated" else y) * dy).sum()
    _same(got, _grads(dense, x2, W))


@pytest.mark.parametrize("norm,relu", [("both", True), ("right", False), ("left", True), ("both", False)])
def test_directed_normalised_gcn_gradients_equal_autograd_of_the_dense_formula(scipy_layers, directed_graph, norm, relu):
    import TCGNN
    L = scipy_layers
    rp, col, A = directed_graph
    meta = _meta(rp, col)
    torch.manual_seed(2)
    conv = L.GCNConv(6, 5, norm=norm, bias=True, directed=True).double()
    with torch.no_grad():
        conv.bias.normal_()
    W, b = _leaf(conv.weights), _leaf(conv.bias)
    x = torch.randn(150, 6, dtype=torch.float64)
    dy = torch.randn(150, 5, dtype=torch.float64)
    x1, x2 = _leaf(x), _leaf(x)
    got = _grads(lambda: (conv(x1, *meta, fuse_relu=relu) * dy).sum(), x1, conv.weights, conv.bias)
    r, c = TCGNN.degree_scales(meta[0], meta[1], norm)
    r = r.double() if r is not None else torch.ones(150, dtype=torch.float64)
    c = c.double() if c is not None else torch.ones(150, dtype=torch.float64)

    def dense():
        y = r[:, None] * (A @ (c[:, None] * (x2 @ W))) + b
        return ((torch.relu(y) if relu else y) * dy).sum()
    _same(got, _grads(dense, x2, W, b))


def test_directed_agnn_gradients_equal_autograd_of_the_dense_formula(scipy_layers, directed_graph):
    """dX, dW: autograd of Y = A_att (X W) with att held fixed (the reference's layer does not propagate through the scores);
    d(attention_w): the reference's formula <sddmm(dY), col>, which the directed layer keeps."""
    L = scipy_layers
    rp, col, A = directed_graph
    meta = _meta(rp, col)
    torch.manual_seed(3)
    conv = L.AGNNConv(6, 5, directed=True).double()
    x = torch.randn(150, 6, dtype=torch.float64)
    dy = torch.randn(150, 5, dtype=torch.float64)
    x1, x2 = _leaf(x), _leaf(x)
    W = _leaf(conv.weights)
    got = _grads(lambda: (conv(x1, *meta) * dy).sum(), x1, conv.weights, conv.attention_w)
    rows = np.repeat(np.arange(150), np.diff(rp))
    H = (x @ conv.weights.detach()).numpy()
    att = float(conv.attention_w.detach()) * (H[rows] * H[col]).sum(1).astype(np.float32).astype(np.float64)   # (scores in fp32, as the backend's)
    Aatt = torch.from_numpy(sp.csr_matrix((att, col, rp), shape=(150, 150)).toarray())
    want = _grads(lambda: ((Aatt @ (x2 @ W)) * dy).sum(), x2, W)
    dyh = dy.numpy()
    d_att_w = float(((dyh[rows] * dyh[col]).sum(1) * col).sum())
    _same(got[:2], want)
    assert abs(float(got[2]) - d_att_w) <= 1e-5 * max(1.0, float((np.abs((dyh[rows] * dyh[col]).sum(1)) * col).sum()))


def test_undirected_layers_still_match_the_reference_fixture():
    """directed=False (given explicitly) keeps the reference's gradients: layers_n200.npz through the oracle, which takes no transpose="""
    import tcgnn_layers as L
    from test_layers_cpu import GOLD, _close, oracle_backend
    f = np.load(os.path.join(GOLD, "layers_n200.npz"))
    t = lambda k: torch.from_numpy(f[k])  # noqa: E731
    meta = (t("rowptr"), t("col"), t("bp"), t("e2c"), t("e2r"))
    dY = t("dY")
    old = L._backend
    L.set_backend(oracle_backend())
    try:
        x = t("Xs").clone().requires_grad_(True)
        y = L.TCGNNFunction_SAG.apply(x, *meta, False); y.backward(dY)
        assert _close(y, f["sag_Y"]) and _close(x.grad, f["sag_dX"])
        x, w = t("X").clone().requires_grad_(True), t("W").clone().requires_grad_(True)
        y = L.TCGNNFunction.apply(x, w, *meta, False, False, False); y.backward(dY)
        assert _close(y, f["gcn_Y"]) and _close(x.grad, f["gcn_dX"]) and _close(w.grad, f["gcn_dW"])
        x, w = t("X").clone().requires_grad_(True), t("W").clone().requires_grad_(True)
        y = L.TCGNNFunction_GIN.apply(x, w, *meta, False); y.backward(dY)
        assert _close(y, f["gin_Y"]) and _close(x.grad, f["gin_dX"]) and _close(w.grad, f["gin_dW"])
        x, w, a = t("X").clone().requires_grad_(True), t("W").clone().requires_grad_(True), t("attention_w").clone().requires_grad_(True)
        y = L.TCGNNFunction_AGNN.apply(x, w, a, *meta, False); y.backward(dY)
        assert _close(y, f["agnn_Y"]) and _close(x.grad, f["agnn_dX"]) and _close(w.grad, f["agnn_dW"])
        assert _close(a.grad, f["agnn_dattention_w"], tol=1e-4)
        assert not L.GCNConv(4, 3).directed and not L.GINConv(4, 3).directed and not L.AGNNConv(4, 3).directed
    finally:
        L.set_backend(old)


def test_transposed_calls_check_their_arguments_like_the_plain_ones():
    import TCGNN
    rp, col = graphs.uniform_graph(20, 3, seed=1)
    n = len(rp) - 1
    meta = (torch.from_numpy(rp), torch.from_numpy(col), torch.zeros(2, dtype=torch.int32), torch.zeros(len(col), dtype=torch.int32),
            torch.zeros(len(col), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="input must be a CUDA tensor"):
        TCGNN.forward(torch.zeros(n, 8), *meta, transpose=True)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        TCGNN.transpose_graph(meta[0], meta[1])
