"""Multi-head GAT on the host: the C ABI's new symbols and their degenerate calls, the numpy restatements and what they alone use of
the bounds (tests/gat_ref.py), the differentiable operators and GATConv against a dense fp64 autograd model through a pure-torch
backend, and the condition of the GPU layer test.  tests/test_gpu_gat.py runs the kernels."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import edge_ops_ref as R
import gat_ref as G
import graphs
import walks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
ENTRY_POINTS = {"tcgnn_gat_softmax": 10, "tcgnn_gat_softmax_backward": 13, "tcgnn_edge_colsum": 8}


def test_new_entry_points_are_declared_exported_and_bound():
    import tcgnn_capi
    lib = ctypes.CDLL(tcgnn_capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "tcgnn.h")).read()
    binding = open(os.path.join(ROOT, "integration", "TCGNN_binding.cpp")).read()
    for name, nargs in ENTRY_POINTS.items():
        assert name in tcgnn_capi.SIGNATURES and len(tcgnn_capi.SIGNATURES[name][1]) == nargs, name
        assert getattr(lib, name) is not None
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in binding, name
    for name in ("gat_softmax", "gat_softmax_backward", "edge_colsum"):
        assert re.search(r'm\.def\("%s"' % name, binding), name
    import TCGNN
    for name in ("gat_softmax", "gat_softmax_backward", "edge_colsum"):
        assert callable(getattr(TCGNN, name)) and name in TCGNN.__all__


def test_degenerate_calls_answer_without_a_device():
    import tcgnn_capi
    lib = tcgnn_capi.lib
    fwd = lambda N, E, H: lib.tcgnn_gat_softmax(None, None, N, E, H, None, None, 0.2, None, None)                      # noqa: E731
    bwd = lambda N, E, H: lib.tcgnn_gat_softmax_backward(None, None, N, E, H, None, None, 0.2, None, None, None, None, None)   # noqa: E731
    cs = lambda N, E, H: lib.tcgnn_edge_colsum(None, None, N, E, H, None, None, None)                                   # noqa: E731
    for call in (fwd, bwd, cs):
        assert call(0, 0, 1) == 0          # N = 0
        assert call(5, 0, 3) == 0          # E = 0
        assert call(0, 7, 1) == 0
        assert call(5, 0, 0) != 0          # H = 0
        assert call(5, -1, 1) != 0         # E = -1
        assert call(-1, 0, 1) != 0
        assert call(5, 1 << 31, 1) != 0    # (int32 CSR positions only)
        assert call(5, 7, 2) != 0          # sizes fine, arrays null
    assert b"tcgnn_edge_colsum" in lib.tcgnn_last_error()


def test_score_restatement_has_exactly_two_fp32_roundings():
    rp, col = graphs.powerlaw_graph(64, 5, seed=12, symmetric=False)
    rng = np.random.default_rng(0)
    el, er = (3 * rng.standard_normal((64, 3))).astype(np.float32), (3 * rng.standard_normal((64, 3))).astype(np.float32)
    rows = np.repeat(np.arange(64), np.diff(rp))
    s = G.gat_scores_f32(rp, col, el, er, 0.2)
    assert s.dtype == np.float32 and s.shape == (3, len(col))
    for h, e in ((0, 0), (1, 17), (2, len(col) - 1)):
        x = np.float32(np.float64(el[col[e], h]) + np.float64(er[rows[e], h]))           # one rounding
        want = x if x > 0 else np.float32(np.float64(x) * np.float64(np.float32(0.2)))    # and one more
        assert s[h, e] == want
    assert (s < 0).any() and (s > 0).any()
    assert np.array_equal(G.gat_scores_f32(rp, col, el, er, 1.0), G.gat_raw_f32(rp, col, el, er))
    assert (G.gat_scores_f32(rp, col, el, er, 0.0) >= 0).all()


def test_input_sets():
    rp, col = G.row_class_graph()
    n = len(rp) - 1
    assert col.dtype == np.int32 and len(col) == rp[-1] and col.min() >= 0 and col.max() < n
    lo, hi = int(rp[R.EMPTY_EDGE + 15]), int(rp[R.EMPTY_EDGE + 16])           # the row of 300 000: duplicates
    assert hi - lo == 300000 and len(np.unique(col[lo:hi])) <= n
    sets = G.el_er_sets(n)
    assert tuple(sets) == G.SETS
    for name, (el, er) in sets.items():
        assert el.shape == er.shape == (n, G.MAX_HEADS) and el.dtype == er.dtype == np.float32, name
    assert np.all(sets["constant"][0] == sets["constant"][0][0]) and np.abs(sets["magnitude_1e4"][0]).min() > 9e3
    s = G.gat_scores_f32(rp, col, *sets["constant"], 0.2)
    assert all(np.all(s[:, a:b] == s[:, a:a + 1]) for a, b in R._rows(rp))                  # every row's scores are equal


@pytest.mark.parametrize("slope", G.SLOPES)
def test_what_the_kernels_do_uses_at_most_half_of_each_forward_bound_on_the_gat_inputs(slope):
    """softmax_f32_sum64 (the exponent rounded once, fp32 exp2, fp64 row sum and quotient) of the fp32 scores against softmax_f64 of the
    same scores: at most half of REL, ABS and ROW_SUM for every set and head.  Were it more, the INPUTS would change, not the bounds."""
    rp, col = G.row_class_graph()
    worst = {}
    for name, (el, er) in G.el_er_sets(len(rp) - 1).items():
        s32 = G.gat_scores_f32(rp, col, el, er, slope)
        shares = [0.0, 0.0, 0.0]
        for h in range(G.MAX_HEADS):
            p64, dist = R.softmax_f64(rp, s32[h], 1.0)
            shares = [max(a, b) for a, b in zip(shares, R.softmax_bounds_hold(rp, R.softmax_f32_sum64(rp, s32[h], 1.0), p64, dist))]
        print("softmax_f32_sum64 of gat scores slope=%.1f %-14s shares: relative %.3f absolute %.3f row sum %.3f" % (slope, name, *shares))
        worst[name] = shares
    assert max(max(v) for v in worst.values()) <= 0.5, worst


@pytest.mark.parametrize("slope", G.SLOPES)
def test_backward_restatement_uses_at_most_a_quarter_of_its_constants(slope):
    """C_GAT_BWD and C_GAT_SUM are 4 x what gat_bwd_f32 (fp32, sequential sums) needs against gat_bwd_f64 on the test inputs; the worst
    values are printed and recorded in gat_ref's docstring and DESIGN 4.11."""
    rp, col = G.row_class_graph()
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
    rng = np.random.default_rng(3 + G.SLOPES.index(slope))
    wds = wer = wel = 0.0
    for name, (el, er) in G.el_er_sets(n).items():
        s32 = G.gat_scores_f32(rp, col, el, er, slope)
        p = np.stack([R.softmax_f32_sum64(rp, s32[h], 1.0) for h in range(G.MAX_HEADS)])
        dp = rng.standard_normal(p.shape).astype(np.float32)
        ref = G.gat_bwd_f64(rp, col, el, er, slope, p, dp)
        ds, d_er, d_el = G.gat_bwd_f32(rp, col, el, er, slope, p, dp)
        c = G.ds_worst(rp, ds, ref)
        cr, cl = G.sum_worst(d_er, ref["d_er"], ref["d_er_scale"]), G.sum_worst(d_el, ref["d_el"], ref["d_el_scale"])
        print("gat_bwd_f32 slope=%.1f %-14s ds c = %.3e, d_er %.3e and d_el %.3e of sum |ds64|" % (slope, name, c, cr, cl))
        wds, wer, wel = max(wds, c), max(wer, cr), max(wel, cl)
        # the derived check of the sums, on a restatement that sums as the kernels do (the fp32 terms in fp64, one rounding)
        assert G.sum_of_own_terms_worst(np.stack([np.bincount(rows, weights=ds[h].astype(np.float64), minlength=n) for h in range(len(ds))], 1)
                                        .astype(np.float32), ds, rows, n) <= G.OWN_SUM
    print("gat_bwd_f32 slope=%.1f worst: ds %.3e, d_er %.3e, d_el %.3e" % (slope, wds, wer, wel))
    assert 4 * wds <= G.C_GAT_BWD and 4 * max(wer, wel) <= G.C_GAT_SUM, (wds, wer, wel)


# ---- the differentiable operators over the pure-torch backend against dense fp64 autograd --------------------------------------------

@pytest.fixture
def torch_layers():
    import tcgnn_layers as L
    old = L._backend
    L.set_backend(G.TorchBackend())
    yield L
    L.set_backend(old)


def _golden_graph():
    f = np.load(os.path.join(GOLD, "layers_n200.npz"))
    return f["rowptr"], f["col"]


def _directed64():
    rp, col = graphs.powerlaw_graph(64, 5, seed=12, symmetric=False)
    assert not walks.is_symmetric(rp, col)
    return rp, col


GRAPHS = {"layers_n200": _golden_graph, "directed_n64": _directed64}


def _close(got, want, tol=1e-5):
    got, want = got.detach(), want.detach()
    assert got.shape == want.shape
    assert float((got.double() - want.double()).abs().max()) <= tol * max(float(want.double().abs().max()), 1e-300), (got - want).abs().max()


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_gat_operators_have_the_gradients_of_the_dense_formulas(torch_layers, name, heads):
    import tcgnn_edge_ops as E
    rp, col = GRAPHS[name]()
    n, nnz = len(rp) - 1, len(col)
    A = G.dense_adjacency(rp, col)
    meta = (torch.from_numpy(rp), torch.from_numpy(col), None, None, None)
    rows, cols = torch.repeat_interleave(torch.arange(n), torch.from_numpy(np.diff(rp)).long()), torch.from_numpy(col).long()
    torch.manual_seed(1)
    leaf = lambda *shape: torch.randn(*shape, dtype=torch.float64).requires_grad_(True)   # noqa: E731

    el, er, w = leaf(n, heads), leaf(n, heads), torch.randn(heads, nnz, dtype=torch.float64)
    P = E.gat_attention(el, er, meta[0], meta[1], 0.2)
    assert P.shape == (heads, nnz)

    def dense_p():
        out = []
        for h in range(heads):
            S = torch.nn.functional.leaky_relu(el[:, h].unsqueeze(0) + er[:, h].unsqueeze(1), 0.2)
            S = S.masked_fill(A == 0, float("-inf")).masked_fill(A.sum(1, keepdim=True) == 0, 0.0)
            out.append(torch.softmax(S, 1)[rows, cols])
        return torch.stack(out)
    want = dense_p()
    _close(P, want)
    got = torch.autograd.grad((P * w).sum(), (el, er))
    ref = torch.autograd.grad((want * w).sum(), (el, er))
    _close(got[0], ref[0]); _close(got[1], ref[1])

    Pl, Z, dY = leaf(heads, nnz), leaf(n, heads * 5), torch.randn(n, heads * 5, dtype=torch.float64)
    Y = E.aggregate_heads(Pl, Z, meta)
    dense = lambda: torch.cat([torch.zeros(n, n, dtype=torch.float64).index_put((rows, cols), Pl[h]) @ Z[:, 5 * h:5 * h + 5] for h in range(heads)], 1)   # noqa: E731
    _close(Y, dense())
    got = torch.autograd.grad((Y * dY).sum(), (Pl, Z))
    ref = torch.autograd.grad((dense() * dY).sum(), (Pl, Z))
    _close(got[0], ref[0]); _close(got[1], ref[1])
    with pytest.raises(RuntimeError):
        E.aggregate_heads(torch.zeros(2, nnz, dtype=torch.float64), torch.zeros(n, 5, dtype=torch.float64), meta)


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_gat_layer_equals_the_dense_model_in_values_and_gradients(torch_layers, name, heads, concat):
    L = torch_layers
    rp, col = GRAPHS[name]()
    n = len(rp) - 1
    A = G.dense_adjacency(rp, col)
    meta = (torch.from_numpy(rp), torch.from_numpy(col), None, None, None)
    torch.manual_seed(2)
    conv = L.GATConv(9, 6, heads=heads, concat=concat).double()
    assert conv.weights.shape == (9, heads * 6) and conv.attn_l.shape == conv.attn_r.shape == (1, heads, 6)
    assert conv.bias.shape == ((heads * 6,) if concat else (6,)) and not conv.bias.detach().any()
    conv.bias.data.normal_()
    X = torch.randn(n, 9, dtype=torch.float64, requires_grad=True)
    Y = conv(X, *meta)
    assert Y.shape == (n, heads * 6 if concat else 6)
    dY = torch.randn_like(Y)
    params = (conv.weights, conv.attn_l, conv.attn_r, conv.bias)
    got = torch.autograd.grad((Y * dY).sum(), (X,) + params)
    Yd = G.dense_gat_model(A, X, *params, heads=heads, concat=concat)
    want = torch.autograd.grad((Yd * dY).sum(), (X,) + params)
    _close(Y, Yd)
    for g, w in zip(got, want):
        _close(g, w)
    lonely = np.nonzero(np.diff(rp) == 0)[0]
    if len(lonely):      # a node without incoming edges gets the bias only
        assert torch.equal(Y[int(lonely[0])].detach(), conv.bias.detach())
    if name == "directed_n64":
        Yt = G.dense_gat_model(A.t().contiguous(), X, *params, heads=heads, concat=concat)
        wrong = torch.autograd.grad((Yt * dY).sum(), (X,))[0]
        assert float((wrong - want[0]).abs().max()) > 1e-3 * float(want[0].abs().max())
    assert L.GATConv(4, 4, bias=False).bias is None
    with pytest.raises(ValueError):
        L.GATConv(4, 4, heads=0)


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("name", ["layers_n200", "directed_n3000"])
def test_operand_rounding_alone_stays_inside_half_of_the_gpu_layer_tolerance(name, concat):
    """The dense fp64 model with the aggregation's operands rounded as the kernels round them (10 mantissa bits on Z and on dY) against
    the unrounded one, on the inputs of the GPU layer test: every compared tensor within HALF of that test's 2e-3 of the largest entry.
    Were it not, the seed or the size would change, not the tolerance."""
    rp, col, X, W, al, ar, b, dY = G.gpu_layer_case(name, concat)
    A = G.dense_adjacency(rp, col)
    H = G.LAYER_CASE["heads"]
    out = {}
    for rounded in (False, True):
        leaves = [t.clone().requires_grad_(True) for t in (X, W, al, ar, b)]
        Y = G.dense_gat_model(A, *leaves, heads=H, concat=concat, round_operands=rounded)
        out[rounded] = [Y.detach()] + list(torch.autograd.grad((Y * dY).sum(), leaves))
    for what, exact, rnd in zip(("Y", "dX", "dW", "dattn_l", "dattn_r", "dbias"), out[False], out[True]):
        share = float((rnd - exact).abs().max()) / float(exact.abs().max()) / G.GPU_LAYER_TOL
        print("rounded operands %s concat=%s %-8s %.3f of the GPU tolerance" % (name, concat, what, share))
        assert share <= 0.5, (what, share)
    assert any(not torch.equal(a, b_) for a, b_ in zip(out[False], out[True]))


def test_harness_accepts_gat_and_heads():
    import tcgnn_harness as H
    args = H.build_parser().parse_args(["--model", "gat", "--heads", "4"])
    assert args.model == "gat" and args.heads == 4
    assert H.build_parser().parse_args([]).heads == 1
    meta = (torch.zeros(2, dtype=torch.int32),) * 5
    with pytest.raises(ValueError, match="multiple"):
        H.time_training("gat", meta, torch.zeros(1, 4), torch.zeros(1).long(), 4, 6, 2, 2, 0, heads=4)
    with pytest.raises(ValueError, match="GAT model only"):
        H.time_training("gcn", meta, torch.zeros(1, 4), torch.zeros(1).long(), 4, 4, 2, 2, 0, heads=2)
    import tcgnn_layers as L
    net = H.Net(lambda a, b: L.GATConv(a, b // 4, heads=4), 12, 8, 5, 3, out_cls=L.GATConv)
    assert net.conv1.weights.shape == (12, 8) and net.hidden_layers[0].weights.shape == (8, 8) and net.conv2.weights.shape == (8, 5)
    assert net.conv1.heads == 4 and net.conv2.heads == 1
