"""Message passing with a feature vector per edge, without a GPU: tests/edge_message_ref.py (what the kernels are held to in
tests/test_gpu_edge_message.py) against brute force on the small and the boundary graphs, the ReLU boundary values against torch.relu
and its autograd, aggregate_ue / edge_sum / GINEConv over the pure-torch backend against the dense fp64 model, the layer's refusals,
the harness parser and the library's symbols."""
import os

import numpy as np
import pytest
import torch

import edge_message_ref as R
import graphs
import walks as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _duplicates_graph():
    """directed, duplicate edges, unsorted rows, an empty first and last row and empty rows in between"""
    rng = np.random.default_rng(9)
    lens = np.concatenate([[0], rng.integers(0, 9, 28), [0]])
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return rp, rng.integers(0, 6, int(rp[-1])).astype(np.int32)


def _small_graphs():
    out = [g for g in graphs.edge_case_graphs() if len(g[1]) - 1 <= 48]
    out.append(("directed_n40", *graphs.uniform_graph(40, 4, seed=5, symmetric=False)))
    out.append(("duplicates_n30", *_duplicates_graph()))
    return out


SMALL = _small_graphs()
BOUNDARY = graphs.boundary_graphs()


@pytest.mark.parametrize("name,rp,col", SMALL, ids=[g[0] for g in SMALL])
@pytest.mark.parametrize("act", ["relu", "identity"])
def test_restatement_equals_the_position_by_position_sum_on_small_graphs(name, rp, col, act):
    n, E, D = len(rp) - 1, len(col), 5
    for which in R.SETS:
        X, Ef, dY = R.input_set(which, n, E, D, seed=n)
        Y, S, A = R.edge_message(rp, col, X, Ef, act)
        Yb = R.brute_edge_message(rp, col, X, Ef, act)
        if which == "integer":
            assert np.array_equal(Y.astype(np.float64), Yb) and np.array_equal(S, Yb)
        else:
            assert R.share(Y, Yb, A)[0] <= 1.0, which
        assert not Y[np.diff(rp) == 0].any()
        # backward: dM has the bits of dY[row e] or is +0.0, and sums back by row to what survived
        dM = R.edge_message_backward(rp, col, X, Ef, dY, act)
        rows = R.edge_rows(rp)
        for e in range(E):
            for d in range(D):
                z = np.float32(X[col[e], d] + Ef[e, d])
                passes = act == "identity" or not (z <= 0)
                want = dY[rows[e], d] if passes else np.float32(0.0)
                assert dM[e, d].view(np.uint32) == np.float32(want).view(np.uint32), (which, e, d)
        # edge_sum by destination and, through perm, by source
        Ys, Ss, As = R.edge_sum(rp, None, dM)
        want = np.zeros((n, D))
        np.add.at(want, rows, dM.astype(np.float64))
        assert R.share(Ys, want, As)[0] <= 1.0
        rp_t, col_t, perm = W.transposed_csr(rp, col)
        assert np.array_equal(np.sort(perm), np.arange(E))
        Yt, St, At = R.edge_sum(rp_t, perm, dM)
        want = np.zeros((n, D))
        np.add.at(want, col.astype(np.int64), dM.astype(np.float64))
        assert R.share(Yt, want, At)[0] <= 1.0


@pytest.mark.parametrize("name,rp,col", BOUNDARY, ids=[g[0] for g in BOUNDARY])
def test_restatement_equals_the_scatter_sum_on_the_boundary_graphs(name, rp, col):
    n, E, D = len(rp) - 1, len(col), 3
    X, Ef, _ = R.input_set("integer", n, E, D, seed=1)
    Y, S, A = R.edge_message(rp, col, X, Ef, "relu")
    assert np.array_equal(Y.astype(np.float64), R.scatter_edge_message(rp, col, X, Ef, "relu"))
    X, Ef, _ = R.input_set("normal", n, E, D, seed=1)
    Y, S, A = R.edge_message(rp, col, X, Ef, "relu")
    whole, _ = R.share(Y, R.scatter_edge_message(rp, col, X, Ef, "relu"), A)
    assert whole <= 1.0, whole


def test_relu_boundary_values_as_torch_relu_and_its_autograd():
    """z = -0.0, +0.0, the smallest subnormals, NaN, +-1 on a graph of one edge per row: the message is torch.relu(z) (a NaN stays NaN,
    both zeros give a zero) and dM is what torch's autograd sends back (threshold_backward: a NaN z PASSES the gradient)"""
    zs = np.array([0x80000000, 0x00000000, 0x00000001, 0x80000001, 0x7FC00000, 0xFFC00123, 0x3F800000, 0xBF800000], dtype=np.uint32).view(np.float32)
    n = len(zs)
    rp, col = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)
    X, Ef = zs.reshape(n, 1).copy(), np.full((n, 1), -0.0, np.float32)
    z, m = R.message_f32(rp, col, X, Ef, "relu")
    assert np.array_equal(z.view(np.uint32), X.view(np.uint32))                     # x + -0.0 = x, bit for bit
    zt = torch.from_numpy(zs.copy()).requires_grad_(True)
    want = torch.relu(zt)
    assert np.array_equal(np.isnan(m[:, 0]), torch.isnan(want).numpy())
    ok = ~np.isnan(m[:, 0])
    assert np.array_equal(m[ok, 0], want.detach().numpy()[ok])
    Y, _, _ = R.edge_message(rp, col, X, Ef, "relu")
    assert np.array_equal(np.isnan(Y[:, 0]), np.isnan(zs)) and np.array_equal(Y[ok, 0], want.detach().numpy()[ok])
    dY = np.arange(1, n + 1, dtype=np.float32).reshape(n, 1)
    want.backward(torch.from_numpy(dY[:, 0].copy()))
    dM = R.edge_message_backward(rp, col, X, Ef, dY, "relu")
    assert np.array_equal(dM[:, 0], zt.grad.numpy())
    assert list(dM[:, 0] != 0) == [False, False, True, False, True, True, True, False]
    assert not np.signbit(dM[dM == 0]).any()
    # the pure-torch backend agrees (it is what the CPU layer tests run on)
    b = R.TorchBackend()
    t = lambda a: torch.from_numpy(a)   # noqa: E731
    Yb = b.forward_ue(t(X), t(Ef), t(rp), t(col), act="relu")
    assert np.array_equal(np.isnan(Yb.numpy()), np.isnan(Y)) and np.array_equal(Yb.numpy()[ok], Y[ok])
    assert np.array_equal(b.backward_ue(t(dY), t(X), t(Ef), t(rp), t(col), act="relu").numpy(), dM)
    assert np.array_equal(b.backward_ue(t(dY), None, None, t(rp), t(col), act=None).numpy(), dY)


# ---- the operators and the layer over the pure-torch backend --------------------------------------------------------------------------

@pytest.fixture
def layers():
    import tcgnn_layers as L
    old = L._backend
    L.set_backend(R.TorchBackend())
    yield L
    L.set_backend(old)


def _golden():
    f = np.load(os.path.join(ROOT, "tests", "golden", "layers_n200.npz"))
    return f["rowptr"].astype(np.int32), f["col"].astype(np.int32)


GRAPHS = {"layers_n200": _golden, "duplicates_n30": _duplicates_graph}


def _rel(got, want):
    got, want = got.detach().double(), want.detach().double()
    assert got.shape == want.shape
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)


def _meta(rp, col):
    bp, e2c, e2r, _ = graphs.host_sgt(rp, col)
    return [torch.from_numpy(np.ascontiguousarray(a)) for a in (rp, col, bp, e2c, e2r)]


@pytest.mark.parametrize("graph", list(GRAPHS))
@pytest.mark.parametrize("act", ["relu", "identity"])
def test_aggregate_ue_and_edge_sum_against_the_dense_fp64_model(layers, graph, act):
    """fp32 operators, fp64 model: output within 1e-5, gradients within 1e-4 of the largest entry (the bounds of the other CPU layer tests)"""
    import tcgnn_edge_ops as E
    rp, col = GRAPHS[graph]()
    n, ne, D = len(rp) - 1, len(col), 7
    B, Sel = R.incidence(rp, col)
    trp, tcol = torch.from_numpy(rp), torch.from_numpy(col)
    torch.manual_seed(4)
    X, Ef = torch.randn(n, D), torch.randn(ne, D)
    dY = torch.randn(n, D, dtype=torch.float64)
    Xg, Eg = X.clone().requires_grad_(True), Ef.clone().requires_grad_(True)
    Y = E.aggregate_ue(Xg, Eg, trp, tcol, act)
    Xd, Ed = X.double().requires_grad_(True), Ef.double().requires_grad_(True)
    want = R.dense_aggregate_ue(B, Sel, Xd, Ed, act)
    assert _rel(Y, want) <= 1e-5
    assert not Y[np.diff(rp) == 0].any()
    got = torch.autograd.grad((Y * dY.float()).sum(), [Xg, Eg])
    ref = torch.autograd.grad((want * dY).sum(), [Xd, Ed])
    for g, r, what in zip(got, ref, ("dX", "dEf")):
        assert _rel(g, r) <= 1e-4, what
    # only one side asks for a gradient
    Y = E.aggregate_ue(X, Eg, trp, tcol, act)
    assert _rel(torch.autograd.grad((Y * dY.float()).sum(), [Eg])[0], ref[1]) <= 1e-4
    Y = E.aggregate_ue(Xg, Ef, trp, tcol, act)
    assert _rel(torch.autograd.grad((Y * dY.float()).sum(), [Xg])[0], ref[0]) <= 1e-4
    # copy_e / sum
    Mg = Ef.clone().requires_grad_(True)
    Ys = E.edge_sum(Mg, trp, tcol)
    Md = Ef.double().requires_grad_(True)
    assert _rel(Ys, B @ Md) <= 1e-5
    assert _rel(torch.autograd.grad((Ys * dY.float()).sum(), [Mg])[0], torch.autograd.grad(((B @ Md) * dY).sum(), [Md])[0]) <= 1e-4
    with pytest.raises(ValueError, match="act"):
        E.aggregate_ue(X, Ef, trp, tcol, "tanh")
    with pytest.raises(RuntimeError, match=r"\[E, D\]"):
        E.aggregate_ue(X, Ef[:, :3], trp, tcol)


@pytest.mark.parametrize("graph", list(GRAPHS))
@pytest.mark.parametrize("edge_dim", [None, 5], ids=["no_edge_dim", "edge_dim5"])
def test_gine_layer_against_the_dense_fp64_model(layers, graph, edge_dim):
    """gradients for X, edge_attr, W, the bias, W_e, b_e and a trained eps; output within 1e-5, gradients within 1e-4 of the largest entry"""
    rp, col = GRAPHS[graph]()
    n, ne = len(rp) - 1, len(col)
    B, Sel = R.incidence(rp, col)
    meta = _meta(rp, col)
    torch.manual_seed(6)
    conv = layers.GINEConv(9, 6, edge_dim=edge_dim, eps=0.25, train_eps=True)
    conv.bias.data.normal_()
    if edge_dim is not None:
        conv.bias_edge.data.normal_()
    assert isinstance(conv.eps, torch.nn.Parameter) and float(conv.eps.detach()) == 0.25
    X, EA = torch.randn(n, 9), torch.randn(ne, edge_dim or 9)
    dY = torch.randn(n, 6, dtype=torch.float64)
    Xg, EAg = X.clone().requires_grad_(True), EA.clone().requires_grad_(True)
    params = [conv.weights, conv.bias, conv.eps] + ([conv.weights_edge, conv.bias_edge] if edge_dim is not None else [])
    Y = conv(Xg, *meta, edge_attr=EAg)
    leaves = [t.detach().double().requires_grad_(True) for t in [X, EA] + params]
    want = R.dense_gine(B, Sel, leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], *leaves[5:])
    assert _rel(Y, want) <= 1e-5
    got = torch.autograd.grad((Y * dY.float()).sum(), [Xg, EAg] + params)
    ref = torch.autograd.grad((want * dY).sum(), leaves)
    for g, r, what in zip(got, ref, ("dX", "dedge_attr", "dW", "dbias", "deps", "dW_e", "db_e")):
        assert _rel(g, r) <= 1e-4, what
    for lonely in np.nonzero(np.diff(rp) == 0)[0][:3]:                                   # no incoming edges: the self term and the bias
        alone = (1.25 * X[lonely]) @ conv.weights + conv.bias
        assert torch.allclose(Y[lonely].detach(), alone.detach(), rtol=1e-5, atol=1e-6)
    assert graph != "duplicates_n30" or (np.diff(rp) == 0).any()
    assert conv(Xg, *meta, EAg).shape == Y.shape                                        # edge_attr positionally, as the issue's signature has it


def test_gine_layer_eps_is_a_buffer_unless_trained_and_refusals(layers):
    rp, col = _duplicates_graph()
    meta = _meta(rp, col)
    n, ne = len(rp) - 1, len(col)
    conv = layers.GINEConv(4, 3)
    assert not isinstance(conv.eps, torch.nn.Parameter) and "eps" in dict(conv.named_buffers()) and float(conv.eps) == 0.0
    assert conv.weights_edge is None and conv.bias is not None
    assert layers.GINEConv(4, 3, bias=False).bias is None
    X = torch.randn(n, 4)
    with pytest.raises(ValueError, match="needs edge_attr"):
        conv(X, *meta)
    with pytest.raises(ValueError, match="edge_dim=6"):
        conv(X, *meta, edge_attr=torch.randn(ne, 6))
    with pytest.raises(ValueError, match="num_edges"):
        conv(X, *meta, edge_attr=torch.randn(ne - 1, 4))
    with pytest.raises(ValueError, match="edge_dim=5"):
        layers.GINEConv(4, 3, edge_dim=5)(X, *meta, edge_attr=torch.randn(ne, 4))
    assert conv(X, *meta, edge_attr=torch.randn(ne, 4)).shape == (n, 3)


def test_harness_parser_knows_the_gine_model():
    import tcgnn_harness as H
    args = H.build_parser().parse_args(["--model", "gine", "--edge-dim", "7"])
    assert (args.model, args.edge_dim) == ("gine", 7)
    assert H.build_parser().parse_args(["--model", "gine"]).edge_dim == 16


def test_library_exports_the_three_entry_points_and_the_abi_version_is_unchanged():
    import tcgnn_capi as c
    assert c.lib.tcgnn_abi_version() == 1
    for name in ("tcgnn_edge_message", "tcgnn_edge_message_backward", "tcgnn_edge_sum"):
        assert name in c.SIGNATURES and callable(getattr(c.lib, name))
    # refused before anything could be launched: these paths need no GPU
    assert c.lib.tcgnn_edge_message(None, None, -1, 0, None, None, 4, 1, None, None) == 1
    assert c.lib.tcgnn_edge_message(None, None, 4, 1 << 31, None, None, 4, 1, None, None) == 1
    assert c.lib.tcgnn_edge_message(None, None, 4, 4, None, None, 4, 2, None, None) == 1
    assert c.lib.tcgnn_edge_message_backward(None, None, 4, 4, None, None, None, 4, -1, None, None) == 1
    assert c.lib.tcgnn_edge_sum(None, None, 4, -1, None, 4, None, None) == 1
    assert c.lib.tcgnn_edge_message(None, None, 0, 5, None, None, 4, 1, None, None) == 0          # no nodes: nothing to write
    assert c.lib.tcgnn_edge_message_backward(None, None, 3, 0, None, None, None, 4, 0, None, None) == 0
    assert c.lib.tcgnn_edge_sum(None, None, 3, 5, None, 0, None, None) == 0
