"""Edge softmax, the two-operand SDDMM, the differentiable edge operators and AGNNConv(attention="softmax") on the host: the C ABI's
new symbols, the numpy restatements and what they alone use of the bounds (tests/edge_ops_ref.py), and the operator layer against a
dense fp64 autograd model through a pure-torch backend.  tests/test_gpu_edge_ops.py runs the kernels."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import edge_ops_ref as R
import graphs
import walks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
ENTRY_POINTS = {"tcgnn_edge_softmax": 7, "tcgnn_edge_softmax_backward": 12, "tcgnn_edge_softmax_workspace_bytes": 2, "tcgnn_sddmm2": 8,
                "tcgnn_sddmm2_workspace_bytes": 2}


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
    for name in ("forward_ef2", "edge_softmax", "edge_softmax_backward"):
        assert re.search(r'm\.def\("%s"' % name, binding), name
    assert tcgnn_capi.lib.tcgnn_edge_softmax_workspace_bytes(233000, 10 ** 8) >= 8 * ((233000 + 31) // 32)
    # the planless calls answer E = 0 / N = 0 without touching a device
    assert tcgnn_capi.lib.tcgnn_edge_softmax(None, 0, 0, None, None, None, None) == 0
    assert tcgnn_capi.lib.tcgnn_edge_softmax(None, 5, 0, None, None, None, None) == 0
    assert tcgnn_capi.lib.tcgnn_edge_softmax(None, 5, -1, None, None, None, None) != 0


def test_row_class_graph_has_every_length_twice_and_empty_ends():
    rp = R.row_class_rowptr()
    lens = np.diff(rp.astype(np.int64))
    assert sorted(lens[R.EMPTY_EDGE:-R.EMPTY_EDGE]) == sorted(R.ROW_LENGTHS * 2)
    assert tuple(lens[R.EMPTY_EDGE:R.EMPTY_EDGE + len(R.ROW_LENGTHS)]) == R.ROW_LENGTHS
    assert not lens[:R.EMPTY_EDGE].any() and not lens[-R.EMPTY_EDGE:].any()
    assert tuple(lens[R.EMPTY_EDGE + len(R.ROW_LENGTHS):-R.EMPTY_EDGE]) != R.ROW_LENGTHS
    sets = R.score_sets(rp)
    assert set(sets) == {"normal_x1", "normal_x8", "normal_x30", "constant_rows", "magnitude_1e4"}
    assert 9e3 < np.abs(sets["magnitude_1e4"]).min() and all(v.dtype == np.float32 and len(v) == rp[-1] for v in sets.values())


def test_softmax_restatements_agree_and_the_fp32_one_uses_at_most_half_of_the_bound():
    """softmax_f64 against a direct evaluation; softmax_f32 - fp32 exponent, exp and pairwise sums - against it on the GPU test's
    inputs plus a row of 2^20 edges: at most half of the relative bound (and inside the row-sum bound).  (The ABSOLUTE bound 1e-7 is not
    asserted on the restatement: an fp32 row sum alone exceeds it for a p near 1 - printed below - which is why the kernels add the
    row in fp64.)"""
    rp = R.row_class_rowptr().astype(np.int64)
    rp = np.concatenate([rp, [rp[-1] + (1 << 20)]])
    s0 = R.score_sets(rp)["normal_x8"]
    p64, dist = R.softmax_f64(rp, s0, 0.5)
    lo, hi = int(rp[R.EMPTY_EDGE + 5]), int(rp[R.EMPTY_EDGE + 6])     # the row of 17
    x = 0.5 * s0[lo:hi].astype(np.float64)
    want = np.exp(x) / np.exp(x).sum()
    assert np.allclose(p64[lo:hi], want, rtol=1e-13, atol=0) and np.allclose(dist[lo:hi], x.max() - x, rtol=1e-13, atol=1e-13)
    assert np.isnan(p64).sum() == 0 and abs(p64[lo:hi].sum() - 1) < 1e-14
    worst = {}
    for beta in (1.0, 0.37, -1.3):
        for name, s in R.score_sets(rp).items():
            p64, dist = R.softmax_f64(rp, s, beta)
            rel, abs_, rs = R.softmax_bounds_hold(rp, R.softmax_f32(rp, s, beta), p64, dist)
            print("softmax_f32 beta=%5.2f %-14s share of the relative bound %.3f, of the row-sum bound %.3f (of the absolute bound %.2f)" % (beta, name, rel, rs, abs_))
            worst[(beta, name)] = (rel, rs)
    assert max(v[0] for v in worst.values()) <= 0.5, worst
    assert max(v[1] for v in worst.values()) <= 1.0, worst
    # the restatement of what the kernels do - fp64 row sums and quotient - against ALL three bounds, at most half of each
    worst = {}
    for beta in (1.0, 0.37, -1.3):
        for name, s in R.score_sets(rp).items():
            p64, dist = R.softmax_f64(rp, s, beta)
            worst[(beta, name)] = R.softmax_bounds_hold(rp, R.softmax_f32_sum64(rp, s, beta), p64, dist)
            print("softmax_f32_sum64 beta=%5.2f %-14s shares: relative %.3f absolute %.3f row sum %.3f" % (beta, name, *worst[(beta, name)]))
    assert max(max(v) for v in worst.values()) <= 0.5, worst


def test_softmax_backward_restatement_uses_at_most_a_quarter_of_its_bound():
    """C_BWD = 4 x what softmax_bwd_f32 needs on the test inputs (printed; recorded in edge_ops_ref's docstring and DESIGN 4.10)"""
    rp = R.row_class_rowptr()
    rng = np.random.default_rng(3)
    worst = wbeta = 0.0
    for beta in (1.0, 0.37, -1.3):
        for name, s in R.score_sets(rp).items():
            p = R.softmax_f32(rp, s, beta)
            dp = rng.standard_normal(len(p)).astype(np.float32)
            ds64, scale, db64, dscale = R.softmax_bwd_f64(rp, p, dp, s, beta)
            ds32, db32 = R.softmax_bwd_f32(rp, p, dp, s, beta)
            c = R.bwd_worst(rp, ds32, ds64, scale)
            cb = abs(float(db32) - db64) / dscale
            print("softmax_bwd_f32 beta=%5.2f %-14s c = %.3e, dbeta %.3e of sum|s||g|" % (beta, name, c, cb))
            worst, wbeta = max(worst, c), max(wbeta, cb)
    assert 4 * worst <= R.C_BWD and 4 * wbeta <= R.C_BWD, (worst, wbeta)


def test_sddmm2_restatements():
    rp, col = graphs.powerlaw_graph(300, 9, seed=4, symmetric=False)
    rng = np.random.default_rng(0)
    X, Z = rng.standard_normal((300, 41)).astype(np.float32), (rng.standard_normal((300, 41)) * 2.0 ** -10).astype(np.float32)
    ef, sc = R.sddmm2_f64(X, Z, rp, col)
    rows = np.repeat(np.arange(300), np.diff(rp))
    for e in (0, 17, len(col) - 1):
        assert abs(ef[e] - float(X[rows[e]].astype(np.float64) @ Z[col[e]].astype(np.float64))) <= 1e-15 * sc[e]
        assert abs(sc[e] - float(np.abs(X[rows[e]]).astype(np.float64) @ np.abs(Z[col[e]]).astype(np.float64))) <= 1e-12 * sc[e]
    et, st = R.sddmm2_tf32(X, Z, rp, col)
    # operand rounding to 10 bits: each factor within 2^-11 relative, so the product sums within 2^-10 + 2^-22 of sum|x||z|
    assert np.all(np.abs(et - ef) <= (2.0 ** -10 + 2.0 ** -21) * sc) and np.any(et != ef)
    from oracle import oracle as O
    ref, _ = O.sddmm_f64(X, rp, col)
    assert np.allclose(R.sddmm2_f64(X, X, rp, col)[0], ref, rtol=0, atol=1e-13 * float(np.abs(ref).max()))   # (fp64, another summation order)


# ---- the differentiable operators over a pure-torch backend against dense fp64 autograd ------------------------------------------

class _TorchBackend:
    """forward_ef2 / edge_softmax / edge_softmax_backward / forward_AGNN(transpose=) composed of torch index operations, any dtype"""

    def _rows(self, rp):
        rp = rp.long()
        return torch.repeat_interleave(torch.arange(rp.numel() - 1), rp[1:] - rp[:-1])

    def forward_ef2(self, X, Z, rp, col, *rest):
        return [(X[self._rows(rp)] * Z[col.long()]).sum(1)]

    def forward_AGNN(self, X, rp, col, att, *rest, transpose=False):
        rows, cols = self._rows(rp), col.long()
        src, dst = (rows, cols) if transpose else (cols, rows)
        return [torch.zeros_like(X).index_add_(0, dst, att[0].unsqueeze(1) * X[src])]

    def edge_softmax(self, s, rp, beta=None):
        rows, n = self._rows(rp), rp.numel() - 1
        x = s if beta is None else beta.reshape(()) * s
        m = torch.full((n,), -float("inf"), dtype=s.dtype).scatter_reduce(0, rows, x, "amax")
        ex = torch.exp(x - m[rows])
        return ex / torch.zeros(n, dtype=s.dtype).index_add_(0, rows, ex)[rows]

    def edge_softmax_backward(self, p, dp, rp, beta=None, score=None, need_dbeta=False, out=None):
        rows, n = self._rows(rp), rp.numel() - 1
        g = p * (dp - torch.zeros(n, dtype=p.dtype).index_add_(0, rows, p * dp)[rows])
        return (g if beta is None else beta.reshape(()) * g), ((score * g).sum().reshape(1) if need_dbeta else None)


@pytest.fixture
def torch_layers():
    import tcgnn_layers as L
    old = L._backend
    L.set_backend(_TorchBackend())
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


def _dense(rp, col):
    n = len(rp) - 1
    A = torch.zeros(n, n, dtype=torch.float64)
    A[torch.repeat_interleave(torch.arange(n), torch.from_numpy(np.diff(rp)).long()), torch.from_numpy(col).long()] = 1.0
    return A


def _close(got, want, tol=1e-5):
    got, want = got.detach(), want.detach()
    assert got.shape == want.shape
    assert float((got.double() - want.double()).abs().max()) <= tol * max(float(want.double().abs().max()), 1e-300), (got - want).abs().max()


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_edge_functions_have_the_gradients_of_the_dense_formulas(torch_layers, name):
    import tcgnn_edge_ops as E
    rp, col = GRAPHS[name]()
    n, nnz = len(rp) - 1, len(col)
    A = _dense(rp, col)
    meta = (torch.from_numpy(rp), torch.from_numpy(col), None, None, None)
    rows, cols = torch.repeat_interleave(torch.arange(n), torch.from_numpy(np.diff(rp)).long()), torch.from_numpy(col).long()
    torch.manual_seed(1)
    leaf = lambda *shape: torch.randn(*shape, dtype=torch.float64).requires_grad_(True)

    # sddmm: the edge entries of X Z^T
    X, Z, w = leaf(n, 7), leaf(n, 7), torch.randn(nnz, dtype=torch.float64)
    ef = E.sddmm(X, Z, meta)
    _close(ef, (X @ Z.t())[rows, cols])
    gx, gz = torch.autograd.grad((ef * w).sum(), (X, Z))
    dx, dz = torch.autograd.grad(((X @ Z.t())[rows, cols] * w).sum(), (X, Z))
    _close(gx, dx); _close(gz, dz)

    # edge_softmax: the row softmax of the masked dense matrix
    s, beta = leaf(nnz), torch.tensor([[0.7]], dtype=torch.float64, requires_grad=True)
    p = E.edge_softmax(s, meta[0], beta)
    S = torch.full((n, n), -float("inf"), dtype=torch.float64).index_put((rows, cols), beta.reshape(()) * s)
    S = S.masked_fill(A.sum(1, keepdim=True) == 0, 0.0)
    want = torch.softmax(S, 1)[rows, cols]
    _close(p, want)
    gs, gb = torch.autograd.grad((p * w).sum(), (s, beta))
    ds, db = torch.autograd.grad((want * w).sum(), (s, beta))
    _close(gs, ds); _close(gb, db)
    assert gb.shape == beta.shape
    _close(E.edge_softmax(s, meta[0]), torch.softmax(S / beta.reshape(()).detach(), 1)[rows, cols].detach())

    # aggregate: the dense matrix with the edge values, times H
    P, H, dY = leaf(nnz), leaf(n, 5), torch.randn(n, 5, dtype=torch.float64)
    Y = E.aggregate(P, H, meta)
    dense = lambda: torch.zeros(n, n, dtype=torch.float64).index_put((rows, cols), P) @ H
    _close(Y, dense())
    gp, gh = torch.autograd.grad((Y * dY).sum(), (P, H))
    dp, dh = torch.autograd.grad((dense() * dY).sum(), (P, H))
    _close(gp, dp); _close(gh, dh)


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_softmax_agnn_layer_equals_the_dense_model_in_values_and_gradients(torch_layers, name):
    L = torch_layers
    rp, col = GRAPHS[name]()
    n = len(rp) - 1
    A = _dense(rp, col)
    meta = (torch.from_numpy(rp), torch.from_numpy(col), None, None, None)
    torch.manual_seed(2)
    conv = L.AGNNConv(9, 6, attention="softmax").double()
    assert float(conv.attention_w.detach()) == 1.0
    conv.attention_w.data.fill_(1.7)
    X = torch.randn(n, 9, dtype=torch.float64, requires_grad=True)
    dY = torch.randn(n, 6, dtype=torch.float64)
    Y = conv(X, *meta)
    got = torch.autograd.grad((Y * dY).sum(), (X, conv.weights, conv.attention_w))
    Yd = R.dense_attention_model(A, X, conv.weights, conv.attention_w)
    want = torch.autograd.grad((Yd * dY).sum(), (X, conv.weights, conv.attention_w))
    _close(Y, Yd)
    for g, w in zip(got, want):
        _close(g, w)
    if name == "directed_n64":
        # the case a backward through A in place of A^T, or a symmetric-P shortcut, would fail: the gradient really differs
        Yt = R.dense_attention_model(A.t().contiguous(), X, conv.weights, conv.attention_w)
        wrong = torch.autograd.grad((Yt * dY).sum(), (X,))[0]
        assert float((wrong - want[0]).abs().max()) > 1e-3 * float(want[0].abs().max())


def test_reference_mode_is_the_default_and_still_reproduces_the_golden_fixture():
    import tcgnn_layers as L
    from test_layers_cpu import oracle_backend
    old = L._backend
    L.set_backend(oracle_backend())
    try:
        f = np.load(os.path.join(GOLD, "layers_n200.npz"))
        t = lambda k: torch.from_numpy(f[k])
        meta = (t("rowptr"), t("col"), t("bp"), t("e2c"), t("e2r"))
        for conv in (L.AGNNConv(*f["W"].shape), L.AGNNConv(*f["W"].shape, attention="reference")):
            assert conv.attention == "reference"
            conv.weights.data.copy_(t("W")); conv.attention_w.data.copy_(t("attention_w"))
            x = t("X").clone().requires_grad_(True)
            y = conv(x, *meta)
            y.backward(t("dY"))
            for got, key, tol in ((y, "agnn_Y", 2e-5), (x.grad, "agnn_dX", 2e-5), (conv.weights.grad, "agnn_dW", 2e-5), (conv.attention_w.grad, "agnn_dattention_w", 1e-4)):
                ref = f[key]
                assert np.allclose(got.detach().numpy(), ref, rtol=tol, atol=tol * max(1.0, float(np.abs(ref).max()))), key
    finally:
        L.set_backend(old)
    with pytest.raises(ValueError):
        L.AGNNConv(4, 4, attention="sigmoid")


def test_harness_accepts_attention():
    import tcgnn_harness as H
    assert H.build_parser().parse_args([]).attention == "reference"
    assert H.build_parser().parse_args(["--model", "agnn", "--attention", "softmax"]).attention == "softmax"
    with pytest.raises(SystemExit):
        H.build_parser().parse_args(["--attention", "other"])
    with pytest.raises(ValueError):
        H.time_training("gcn", (torch.zeros(2, dtype=torch.int32),) * 5, torch.zeros(1, 4), torch.zeros(1).long(), 4, 4, 2, 2, 0, attention="softmax")
