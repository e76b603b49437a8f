"""GATv2 on the host: the C ABI's new symbols and their degenerate calls, the numpy restatements and what they alone use of the bounds
(tests/gatv2_ref.py), the differentiable operator and GATv2Conv against a dense fp64 autograd model through a pure-torch backend, and
the condition of the GPU layer test.  tests/test_gpu_gatv2.py runs the kernels."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gat_ref as G
import gatv2_ref as V
import graphs
import walks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"tcgnn_gatv2_workspace_bytes": 4, "tcgnn_gatv2_softmax": 13, "tcgnn_gatv2_softmax_backward": 18, "tcgnn_gatv2_source_grad": 14}
MODULE_NAMES = ("gatv2_softmax", "gatv2_softmax_backward", "gatv2_source_grad")


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
    for name in MODULE_NAMES:
        assert re.search(r'm\.def\("%s"' % name, binding), name
    import TCGNN
    for name in MODULE_NAMES:
        assert callable(getattr(TCGNN, name)) and name in TCGNN.__all__ and getattr(TCGNN, name).__doc__
    assert tcgnn_capi.lib.tcgnn_abi_version() == 1
    import tcgnn_edge_ops as E
    import tcgnn_layers as L
    assert callable(E.gatv2_attention) and issubclass(L.GATv2Conv, torch.nn.Module)


def test_degenerate_and_invalid_calls_answer_without_a_device():
    import tcgnn_capi
    lib = tcgnn_capi.lib
    fwd = lambda N, E, H, F: lib.tcgnn_gatv2_softmax(None, None, N, E, H, F, None, None, None, 0.2, None, None, None)                      # noqa: E731
    bwd = lambda N, E, H, F: lib.tcgnn_gatv2_softmax_backward(None, None, N, E, H, F, None, None, None, 0.2, None, None, None, None, None,  # noqa: E731
                                                              None, 0, None)
    src = lambda N, E, H, F: lib.tcgnn_gatv2_source_grad(None, None, None, N, E, H, F, None, None, None, 0.2, None, None, None)           # noqa: E731
    for call in (fwd, bwd, src):
        assert call(0, 0, 1, 1) == 0          # N = 0
        assert call(5, 0, 3, 8) == 0          # E = 0 (the node outputs are null: nothing to zero)
        assert call(0, 7, 1, 4) == 0
        assert call(5, 0, 0, 8) == 1          # H = 0: TCGNN_ERR_INVALID_ARG
        assert call(5, 0, 2, 0) == 1          # F = 0
        assert call(5, -1, 1, 1) == 1         # E = -1
        assert call(-1, 0, 1, 1) == 1
        assert call(5, 1 << 31, 1, 1) == 1    # (int32 CSR positions only)
        assert call(5, 7, 2, 3) == 1          # sizes fine, arrays null
    assert b"tcgnn_gatv2_source_grad" in lib.tcgnn_last_error()
    # the scratch: one fp64 per workgroup of 32 rows and column, in 256-byte steps; nothing where there is nothing to reduce
    ws = lib.tcgnn_gatv2_workspace_bytes
    assert ws(0, 0, 1, 1) == 0 and ws(5, 7, 0, 1) == 0 and ws(5, 7, 1, 0) == 0 and ws(-1, 7, 1, 1) == 0 and ws(5, -1, 1, 1) == 0
    assert ws(1, 1, 1, 1) == 256 and ws(32, 9, 1, 32) == 256 and ws(33, 9, 1, 32) == 512 and ws(3000, 9, 3, 100) == (94 * 300 * 8 + 255) // 256 * 256


def test_activation_restatement_has_exactly_two_fp32_roundings():
    rp, col = graphs.powerlaw_graph(64, 5, seed=12, symmetric=False)
    rng = np.random.default_rng(0)
    H, F = 2, 3
    xl, xr = (3 * rng.standard_normal((64, H * F))).astype(np.float32), (3 * rng.standard_normal((64, H * F))).astype(np.float32)
    attn = rng.standard_normal((H, F)).astype(np.float32)
    rows = np.repeat(np.arange(64), np.diff(rp))
    z = V.z_f32(rp, col, xl, xr)
    l, c = V.act_f32(z, 0.2), V.slope_factor_f32(z, attn, 0.2)
    assert z.dtype == l.dtype == c.dtype == np.float32 and z.shape == l.shape == c.shape == (len(col), H * F)
    k = np.float64(np.float32(0.2))
    for e, j in ((0, 0), (17, 4), (len(col) - 1, 5)):
        x = np.float32(np.float64(xl[col[e], j]) + np.float64(xr[rows[e], j]))           # one rounding
        assert z[e, j] == x
        assert l[e, j] == (x if x > 0 else np.float32(np.float64(x) * k))                # and one more
        a = attn[j // F, j % F]
        assert c[e, j] == (a if x > 0 else np.float32(np.float64(a) * k))
    assert (l < 0).any() and (l > 0).any()
    assert np.array_equal(V.act_f32(z, 1.0), z) and (V.act_f32(z, 0.0) >= 0).all()
    # the score is one rounding of the exact sum: against a sum of the products in exact rational arithmetic
    from fractions import Fraction
    s64, mag = V.scores_f64(l, attn)
    for e in (0, 17):
        exact = sum(Fraction(float(attn[1, f])) * Fraction(float(l[e, F + f])) for f in range(F))
        assert abs(Fraction(float(s64[1, e])) - exact) <= Fraction(F * 2.0 ** -53) * Fraction(float(mag[1, e]))


CASES = [(g, H, F, slope, name) for g in sorted(V.ATTN_SCALE) for (H, F) in V.ROW_SHAPES for slope in V.SLOPES for name in V.SETS]


@pytest.mark.parametrize("graph,H,F,slope,name", CASES, ids=["%s-H%d-F%d-slope%.1f-%s" % c for c in CASES])
def test_sequential_restatement_uses_half_of_the_forward_and_a_quarter_of_the_backward_bounds(graph, H, F, slope, name):
    """The operator as the contract states it with every sum taken left to right (gatv2_sequential_f32), on the GPU test's inputs - the
    row-class graph and its transpose, every set and slope, both shapes: at most half of each forward bound and a quarter of each backward one.  Were it
    more, the INPUTS would change, not the bounds.  The four results that are ONE rounding of an fp64 sum (score, d_xr, d_xl, d_attn) are
    measured by what they need beyond that rounding, of the summation's allowance (gatv2_ref.score_share / own_sum_share: the excess, as
    gat_ref.sum_of_own_terms_worst does): a correctly rounded number uses up to all of its 2^-24 |S|, whatever the inputs are - and each
    must hold its whole bound as well."""
    rp, col = V.row_class_graphs()[graph]
    xl, xr, attn = V.x_sets(len(rp) - 1, H, F, attn_scale=V.ATTN_SCALE[graph])[name]
    assert np.abs(V.z_f32(rp, col, xl, xr)).max() >= (1e4 if name == "magnitude_1e4" else 0)
    dp = V.dp_for(H, int(rp[-1]))
    out = V.gatv2_sequential_f32(rp, col, xl, xr, attn, slope, dp)
    whole, shares = V.shares_of_all_bounds(rp, col, attn, dp, out)
    print("gatv2 sequential restatement %s H=%d F=%d slope=%.1f %-14s " % (graph, H, F, slope, name) + ", ".join("%s %.3g" % kv for kv in shares.items()))
    for key, share in shares.items():
        assert share <= (0.5 if key in V.FORWARD_KEYS else 0.25) and whole[key] <= 1.0, (key, share, whole[key])


# ---- the differentiable operator and the layer over the pure-torch backend against dense fp64 autograd ----------------------------------

@pytest.fixture
def torch_layers():
    import tcgnn_layers as L
    old = L._backend
    L.set_backend(V.TorchBackend())
    yield L
    L.set_backend(old)


def _directed64():
    rp, col = graphs.powerlaw_graph(64, 5, seed=12, symmetric=False)
    assert not walks.is_symmetric(rp, col)
    return rp, col


GRAPHS = {"layers_n200": G.golden_graph, "directed_n64": _directed64}


def _close(got, want, tol=1e-5):
    got, want = got.detach(), want.detach()
    assert got.shape == want.shape
    assert float((got.double() - want.double()).abs().max()) <= tol * max(float(want.double().abs().max()), 1e-300), (got - want).abs().max()


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_gatv2_attention_has_the_gradients_of_the_dense_formula(torch_layers, name, heads):
    import tcgnn_edge_ops as E
    rp, col = GRAPHS[name]()
    n, nnz, F = len(rp) - 1, len(col), 5
    A = G.dense_adjacency(rp, col)
    trp, tcol = torch.from_numpy(rp), torch.from_numpy(col)
    rows, cols = torch.repeat_interleave(torch.arange(n), torch.from_numpy(np.diff(rp)).long()), tcol.long()
    torch.manual_seed(1)
    leaf = lambda *shape: torch.randn(*shape, dtype=torch.float64).requires_grad_(True)   # noqa: E731
    xl, xr, attn, w = leaf(n, heads * F), leaf(n, heads * F), leaf(heads, F), torch.randn(heads, nnz, dtype=torch.float64)
    P = E.gatv2_attention(xl, xr, attn, trp, tcol, 0.2)
    assert P.shape == (heads, nnz)
    want = V.dense_gatv2_attention(A, xl, xr, attn, 0.2)[:, rows, cols]
    _close(P, want)
    for g, r in zip(torch.autograd.grad((P * w).sum(), (xl, xr, attn)), torch.autograd.grad((want * w).sum(), (xl, xr, attn))):
        _close(g, r)
    # one tensor on both sides: its gradient is the sum of both
    P1 = E.gatv2_attention(xl, xl, attn, trp, tcol, 0.2)
    want1 = V.dense_gatv2_attention(A, xl, xl, attn, 0.2)[:, rows, cols]
    _close(P1, want1)
    for g, r in zip(torch.autograd.grad((P1 * w).sum(), (xl, attn)), torch.autograd.grad((want1 * w).sum(), (xl, attn))):
        _close(g, r)
    with pytest.raises(RuntimeError):
        E.gatv2_attention(xl, xr[:, :-1], attn, trp, tcol)


def test_with_slope_one_gatv2_attention_is_gat_attention_of_the_projected_terms(torch_layers):
    """slope = 1: the activation is the identity, so s = <xl[col], attn> + <xr[row], attn> - GAT's score on el = <xl, attn>, er = <xr, attn>"""
    import tcgnn_edge_ops as E
    rp, col = _directed64()
    n, H, F = len(rp) - 1, 3, 4
    trp, tcol = torch.from_numpy(rp), torch.from_numpy(col)
    torch.manual_seed(4)
    xl, xr, attn = (torch.randn(*s, dtype=torch.float64) for s in ((n, H * F), (n, H * F), (H, F)))
    el, er = (xl.view(n, H, F) * attn).sum(-1), (xr.view(n, H, F) * attn).sum(-1)
    _close(E.gatv2_attention(xl, xr, attn, trp, tcol, 1.0), E.gat_attention(el, er, trp, tcol, 1.0), tol=1e-12)


@pytest.mark.parametrize("share_weights", [False, True], ids=["two_weights", "shared"])
@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_gatv2_layer_equals_the_dense_model_in_values_and_gradients(torch_layers, name, heads, concat, share_weights):
    L = torch_layers
    rp, col = GRAPHS[name]()
    n = len(rp) - 1
    A = G.dense_adjacency(rp, col)
    meta = (torch.from_numpy(rp), torch.from_numpy(col), None, None, None)
    torch.manual_seed(2)
    conv = L.GATv2Conv(9, 6, heads=heads, concat=concat, share_weights=share_weights).double()
    assert conv.weights.shape == (9, heads * 6) and conv.attn.shape == (1, heads, 6)
    assert (conv.weights_r is None) if share_weights else (conv.weights_r.shape == (9, heads * 6) and not torch.equal(conv.weights_r, conv.weights))
    assert conv.bias.shape == ((heads * 6,) if concat else (6,)) and not conv.bias.detach().any()
    conv.bias.data.normal_()
    X = torch.randn(n, 9, dtype=torch.float64, requires_grad=True)
    Y = conv(X, *meta)
    assert Y.shape == (n, heads * 6 if concat else 6)
    dY = torch.randn_like(Y)
    params = [p for p in (conv.weights, conv.weights_r, conv.attn, conv.bias) if p is not None]
    got = torch.autograd.grad((Y * dY).sum(), [X] + params)

    def dense(adj):
        return V.dense_gatv2_model(adj, X, conv.weights, conv.weights_r, conv.attn, conv.bias, heads=heads, concat=concat)
    Yd = dense(A)
    want = torch.autograd.grad((Yd * dY).sum(), [X] + params)
    _close(Y, Yd)
    for g, w in zip(got, want):
        _close(g, w)
    lonely = np.nonzero(np.diff(rp) == 0)[0]
    if len(lonely):      # a node without incoming edges gets the bias only
        assert torch.equal(Y[int(lonely[0])].detach(), conv.bias.detach())
    if name == "directed_n64":   # the gradient through A instead of A^T is wrong
        wrong = torch.autograd.grad((dense(A.t().contiguous()) * dY).sum(), (X,))[0]
        assert float((wrong - want[0]).abs().max()) > 1e-3 * float(want[0].abs().max())
    assert L.GATv2Conv(4, 4, bias=False).bias is None
    with pytest.raises(ValueError):
        L.GATv2Conv(4, 4, heads=0)


@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
@pytest.mark.parametrize("name", ["layers_n200", "directed_n3000"])
def test_operand_rounding_alone_stays_inside_half_of_the_gpu_layer_tolerance(name, concat):
    """The dense fp64 model with the aggregation's operands rounded as the kernels round them (10 mantissa bits on Zl and on dY) against
    the unrounded one, on the inputs of the GPU layer test: every compared tensor within HALF of gat_ref.GPU_LAYER_TOL of the largest
    entry.  Were it not, the seed or the size would change, not the tolerance."""
    rp, col, X, Wl, Wr, attn, b, dY = V.gpu_layer_case(name, concat)
    A = G.dense_adjacency(rp, col)
    H = V.LAYER_CASE["heads"]
    out = {}
    for rounded in (False, True):
        leaves = [t.clone().requires_grad_(True) for t in (X, Wl, Wr, attn, b)]
        Y = V.dense_gatv2_model(A, *leaves, heads=H, concat=concat, round_operands=rounded)
        out[rounded] = [Y.detach()] + list(torch.autograd.grad((Y * dY).sum(), leaves))
    for what, exact, rnd in zip(("Y", "dX", "dWl", "dWr", "dattn", "dbias"), out[False], out[True]):
        share = float((rnd - exact).abs().max()) / float(exact.abs().max()) / G.GPU_LAYER_TOL
        print("rounded operands %s concat=%s %-6s %.3f of the GPU tolerance" % (name, concat, what, share))
        assert share <= 0.5, (what, share)
    assert any(not torch.equal(a, b_) for a, b_ in zip(out[False], out[True]))


def test_harness_accepts_gatv2_and_heads():
    import tcgnn_harness as H
    args = H.build_parser().parse_args(["--model", "gatv2", "--heads", "4"])
    assert args.model == "gatv2" and args.heads == 4
    meta = (torch.zeros(2, dtype=torch.int32),) * 5
    with pytest.raises(ValueError, match="multiple"):
        H.time_training("gatv2", meta, torch.zeros(1, 4), torch.zeros(1).long(), 4, 6, 2, 2, 0, heads=4)
    with pytest.raises(ValueError, match="GAT model only"):
        H.time_training("gcn", meta, torch.zeros(1, 4), torch.zeros(1).long(), 4, 4, 2, 2, 0, heads=2)
    import tcgnn_layers as L
    net = H.Net(lambda a, b: L.GATv2Conv(a, b // 4, heads=4), 12, 8, 5, 3, out_cls=L.GATv2Conv)
    assert net.conv1.weights.shape == (12, 8) and net.hidden_layers[0].weights.shape == (8, 8) and net.conv2.weights.shape == (8, 5)
    assert net.conv1.heads == 4 and net.conv2.heads == 1
