"""The max aggregation without a GPU: tests/segmax_ref.py (what the kernels are held to in tests/test_gpu_segmax.py) against a
brute-force comparator on small graphs, numpy.argmax's behaviour the contract rests on, and SAGEConv over a stand-in backend - the
helper for the maximum, the oracle's SpMM (unrounded) for the mean - against a dense fp64 model."""
import types

import numpy as np
import pytest
import torch

import graphs
import segmax_ref as S
from oracle import oracle as O


def _small_graphs():
    out = []
    rp, col = graphs.uniform_graph(60, 5, seed=3)
    out.append(("uniform_n60", rp, col))
    rp, col = graphs.with_empty_window(*graphs.uniform_graph(48, 3, seed=7), 16, 32)
    out.append(("empty_rows_n48", rp, col))
    rp, col = graphs.uniform_graph(40, 4, seed=5, symmetric=False)
    out.append(("directed_n40", rp, col))
    rng = np.random.default_rng(9)                                    # duplicate edges, unsorted rows, an empty first and last row
    lens = np.concatenate([[0], rng.integers(0, 9, 28), [0]])
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    out.append(("duplicates_n30", rp, rng.integers(0, 6, int(rp[-1])).astype(np.int32)))
    return out


@pytest.mark.parametrize("name,rp,col", _small_graphs(), ids=[g[0] for g in _small_graphs()])
@pytest.mark.parametrize("which", S.SETS)
def test_helper_equals_the_brute_force_comparator(name, rp, col, which):
    n = len(rp) - 1
    X = S.input_set(which, n, 7, seed=n)
    Y, arg = S.segment_max(rp, col, X)
    Yb, argb = S.segment_max_brute(rp, col, X)
    assert np.array_equal(arg, argb)
    assert np.array_equal(Y.view(np.int32), Yb.view(np.int32))        # bits: sign of zero, NaN payload
    has = arg >= 0
    assert np.array_equal(has, np.repeat((np.diff(rp) > 0)[:, None], 7, 1))
    assert not Y[~has].any() and not np.signbit(Y[~has]).any()
    d = np.nonzero(has)[1]
    assert np.array_equal(Y[has].view(np.int32), X[col[arg[has]], d].view(np.int32))
    # backward: every (i, d) with a winner sends its dY to exactly one source element
    dY = np.random.default_rng(1).integers(-8, 9, (n, 7)).astype(np.float32)
    dX, k, sabs = S.segment_max_backward(rp, col, arg, dY)
    want = np.zeros((n, 7))
    for i in range(n):
        for dd in range(7):
            if arg[i, dd] >= 0:
                want[col[arg[i, dd]], dd] += dY[i, dd]
    assert np.array_equal(dX, want) and int(k.sum()) == int(has.sum()) and np.all(sabs >= np.abs(dX))


def test_numpy_argmax_takes_the_first_nan_and_the_first_of_equal_values():
    nan = np.float32("nan")
    assert np.argmax(np.array([1.0, nan, 5.0, nan], np.float32)) == 1              # a NaN beats every number; the first NaN
    assert np.argmax(np.array([np.inf, nan], np.float32)) == 1
    assert np.argmax(np.array([2.0, 3.0, 3.0, 1.0], np.float32)) == 1              # first occurrence
    assert np.argmax(np.array([-0.0, 0.0, -0.0], np.float32)) == 0                 # -0.0 == +0.0
    assert np.argmax(np.array([0.0, -0.0], np.float32)) == 0
    assert np.argmax(np.array([-np.inf, -np.inf], np.float32)) == 0
    S2 = np.array([[1.0, nan], [nan, 2.0], [3.0, nan]], np.float32)                # per column, as the helper uses it
    assert list(np.argmax(S2, axis=0)) == [1, 0]
    for v1, p1, v2, p2, w in ((1.0, 5, 1.0, 3, False), (-0.0, 1, 0.0, 2, True), (nan, 9, np.inf, 0, True), (nan, 9, nan, 4, False), (2.0, 9, 1.0, 0, True)):
        assert S.wins(np.float32(v1), p1, np.float32(v2), p2) is w


# ---- SAGEConv over a stand-in backend -------------------------------------------------------------------------------------------------

def standin_backend():
    m = types.SimpleNamespace()
    npy = lambda *ts: [t.detach().cpu().numpy() for t in ts]   # noqa: E731

    def forward_scaled(X, rp, col, bp, e2c, e2r, row_scale=None, col_scale=None, bias=None, relu=False, gate=None, transpose=False):
        assert bias is None and not relu and gate is None
        x, rp_, col_, bp_, e2c_, e2r_ = npy(X, rp, col, bp, e2c, e2r)
        if col_scale is not None:
            x = x * col_scale.numpy()[:, None]
        if transpose:
            import walks as W
            rp_, col_, _ = W.transposed_csr(rp_, col_)
            rp_, col_ = rp_.astype(np.int32), col_.astype(np.int32)
            bp_, e2c_, e2r_, _ = graphs.host_sgt(rp_, col_)
        y = O.spmm(np.ascontiguousarray(x, dtype=np.float32), rp_, col_, bp_, e2c_, e2r_, round_mode=O.ROUND_NONE)
        if row_scale is not None:
            y = y * row_scale.numpy()[:, None]
        return [torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))]

    def forward_max(X, rp, col, return_arg=True, out=None):
        Y, arg = S.segment_max(*npy(rp, col), X.detach().numpy())
        return torch.from_numpy(Y), torch.from_numpy(arg)

    def backward_max(dY, arg, rp, col, out=None):
        dX, _, _ = S.segment_max_backward(*npy(rp, col), arg.numpy(), dY.detach().numpy())
        return torch.from_numpy(dX.astype(np.float32))

    m.forward_scaled, m.forward_max, m.backward_max = forward_scaled, forward_max, backward_max
    return m


@pytest.fixture
def layers():
    import tcgnn_layers as L
    old = L._backend
    L.set_backend(standin_backend())
    yield L
    L.set_backend(old)


def _rel(got, want):
    got, want = got.detach().double(), want.detach().double()
    assert got.shape == want.shape
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)


@pytest.mark.parametrize("dims", [(12, 7), (7, 12)], ids=["narrowing", "widening"])
@pytest.mark.parametrize("aggregator", ["mean", "max", "pool"])
def test_sage_layer_against_the_dense_fp64_model_on_a_directed_graph(layers, aggregator, dims):
    """output within 1e-5, gradients of X, every weight and both biases within 1e-4 of the largest entry; directed=True so that the mean
    path's backward goes through A^T (the max paths do whatever the flag says)"""
    import walks as W
    rp, col = graphs.uniform_graph(40, 2, seed=5, symmetric=False)
    assert not W.is_symmetric(rp, col) and (np.diff(rp) == 0).any()
    n = len(rp) - 1
    bp, e2c, e2r, _ = graphs.host_sgt(rp, col)
    meta = [torch.from_numpy(a) for a in (rp, col, bp, e2c, e2r)]
    A = torch.zeros(n, n, dtype=torch.float64)
    A.index_put_((torch.from_numpy(np.repeat(np.arange(n), np.diff(rp))), torch.from_numpy(col).long()), torch.ones(len(col), dtype=torch.float64), accumulate=True)
    torch.manual_seed(3)
    conv = layers.SAGEConv(*dims, aggregator=aggregator, directed=True)
    conv.bias.data.normal_()
    if aggregator == "pool":
        conv.bias_pool.data.normal_()
    X = torch.randn(n, dims[0])
    dY = torch.randn(n, dims[1], dtype=torch.float64)
    Xg = X.clone().requires_grad_(True)
    Y = conv(Xg, *meta)
    params = [conv.weights_self, conv.weights, conv.bias] + ([conv.weights_pool, conv.bias_pool] if aggregator == "pool" else [])
    leaves = [t.detach().double().requires_grad_(True) for t in [X] + params]
    want = S.dense_sage(A, leaves[0], leaves[1], leaves[2], leaves[3], aggregator, *leaves[4:])
    assert _rel(Y, want) <= 1e-5
    got = torch.autograd.grad((Y * dY.float()).sum(), [Xg] + params)
    ref = torch.autograd.grad((want * dY).sum(), leaves)
    for g, r, what in zip(got, ref, ("dX", "dW_self", "dW_neigh", "dbias", "dW_pool", "dbias_pool")):
        assert _rel(g, r) <= 1e-4, what
    lonely = int(np.nonzero(np.diff(rp) == 0)[0][0])
    assert torch.allclose(Y[lonely].detach(), (X[lonely] @ conv.weights_self + conv.bias).detach(), rtol=1e-5, atol=1e-6)   # no neighbours: the self term and the bias


def test_sage_layer_refuses_an_unknown_aggregator_and_the_harness_knows_the_model(layers):
    import tcgnn_harness as H
    with pytest.raises(ValueError, match="aggregator"):
        layers.SAGEConv(4, 4, aggregator="lstm")
    args = H.build_parser().parse_args(["--model", "sage", "--aggregator", "pool"])
    assert (args.model, args.aggregator) == ("sage", "pool")
    assert H.build_parser().parse_args([]).aggregator == "mean"
    with pytest.raises(ValueError, match="SAGE model only"):
        H.time_training("gcn", None, None, None, 4, 4, 2, 2, 1, aggregator="max")
