"""The one-gather aggregation and the PNA layer without a GPU: tests/stats_ref.py (what the kernels are held to in
tests/test_gpu_segstats.py) against brute-force comparators on small graphs, numpy.argmin's behaviour the min rule rests on, a numpy
emulation of the kernel's arithmetic against the helper's bounds (shifted sums hold them on every input set, raw sums break the std
bound on `offset`), the a / b formulation of the backward against torch autograd, the C ABI's symbols and host-side refusals, and
PNAConv over a stand-in backend built on the helper against a dense fp64 model."""
import math
import types

import numpy as np
import pytest
import torch

import graphs
import segmax_ref as S
import stats_ref as R

INVALID_ARG = 1


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


GRAPHS = _small_graphs()


@pytest.mark.parametrize("name,rp,col", GRAPHS, ids=[g[0] for g in GRAPHS])
@pytest.mark.parametrize("which", R.SETS)
def test_helper_equals_the_brute_force_comparators(name, rp, col, which):
    n, D = len(rp) - 1, 7
    X = R.input_set(which, n, D, seed=n)
    r = R.segment_stats(rp, col, X)
    Yx, ax = S.segment_max_brute(rp, col, X)
    Yn, an = R.segment_min_brute(rp, col, X)
    assert np.array_equal(r["argmax"], ax) and np.array_equal(r["max"].view(np.int32), Yx.view(np.int32))
    assert np.array_equal(r["argmin"], an) and np.array_equal(r["min"].view(np.int32), Yn.view(np.int32))       # bits: sign of zero, NaN payload
    Ym, am = S.segment_max(rp, col, X)
    assert np.array_equal(r["argmax"], am) and np.array_equal(r["max"].view(np.int32), Ym.view(np.int32))       # what tcgnn_segment_max is held to
    empty = np.diff(rp) <= 0
    for key in ("mean", "std", "max", "min"):
        assert not r[key][empty].any() and not np.signbit(r[key][empty]).any()                                  # +0, std included
    assert (r["argmax"][empty] == -1).all() and (r["argmin"][empty] == -1).all()
    for i in range(n):                                                                                            # moments, element by element
        vals = [X[col[e]].astype(np.float64) for e in range(int(rp[i]), int(rp[i + 1]))]
        for d in range(D if vals else 0):
            col_d = [float(v[d]) for v in vals]
            if not np.isfinite(col_d).all():
                assert not np.isfinite(r["mean"][i, d]) or not np.isfinite(r["std"][i, d])
                continue
            mean = math.fsum(col_d) / len(col_d)
            var = math.fsum((v - mean) ** 2 for v in col_d) / len(col_d)
            assert abs(r["mean"][i, d] - mean) <= 1e-13 * max(abs(mean), max(abs(v) for v in col_d))
            assert abs(r["std"][i, d] - math.sqrt(var + 1e-5)) <= 1e-12 * math.sqrt(var + 1e-5)


def test_numpy_argmin_takes_the_first_nan_and_the_first_of_equal_values():
    nan = np.float32("nan")
    assert np.argmin(np.array([1.0, nan, -5.0, nan], np.float32)) == 1             # a NaN beats every number; the first NaN
    assert np.argmin(np.array([-np.inf, nan], np.float32)) == 1
    assert np.argmin(np.array([2.0, 1.0, 1.0, 3.0], np.float32)) == 1              # first occurrence
    assert np.argmin(np.array([0.0, -0.0, 0.0], np.float32)) == 0                  # -0.0 == +0.0
    assert np.argmin(np.array([np.inf, np.inf], np.float32)) == 0
    S2 = np.array([[1.0, nan], [nan, 2.0], [-3.0, nan]], np.float32)               # per column, as the helper uses it
    assert list(np.argmin(S2, axis=0)) == [1, 0]
    for v1, p1, v2, p2, w in ((1.0, 5, 1.0, 3, False), (0.0, 1, -0.0, 2, True), (nan, 9, -np.inf, 0, True), (nan, 9, nan, 4, False), (1.0, 9, 2.0, 0, True),
                              (2.0, 0, 1.0, 9, False)):
        assert R.wins_min(np.float32(v1), p1, np.float32(v2), p2) is w


def _long_rows_graph():
    """rows of 0, 1, 2, 3, 17, 300 and 5000 edges over 64 nodes: the bounds grow with k, the error must not outgrow them"""
    rng = np.random.default_rng(4)
    lens = [0, 1, 2, 3, 17, 300, 5000, 0, 40]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return rp, rng.integers(0, 64, int(rp[-1])).astype(np.int32)


@pytest.mark.parametrize("which", R.SETS)
def test_the_kernels_arithmetic_holds_the_bounds_on_every_input_set(which):
    rp, col = _long_rows_graph()
    X = R.input_set(which, 64, 5, seed=2)
    r = R.segment_stats(rp, col, X)
    for parts, seed in ((4, 0), (1, 1), (16, 2)):
        mean, std = R.kernel_moments(rp, col, X, parts=parts, seed=seed)
        ok = np.isfinite(r["mean"]) & np.isfinite(r["std"])
        assert ok.all() or which == "specials"
        assert (np.abs(mean.astype(np.float64)[ok] - r["mean"][ok]) <= r["mean_bound"][ok]).all()
        assert (np.abs(std.astype(np.float64)[ok] - r["std"][ok]) <= r["std_bound"][ok]).all()
        assert not np.isfinite(mean[~ok]).any() or not np.isfinite(std[~ok]).any() or not (~ok).any()
        empty = np.diff(rp) <= 0
        assert not mean[empty].any() and not std[empty].any()
    if which == "constant":
        assert np.array_equal(std[~empty], np.full_like(std[~empty], np.float32(math.sqrt(np.float32(1e-5)))))   # the variance is exactly 0


def test_unshifted_sums_break_the_std_bound_on_the_offset_set():
    """the bounds discriminate: fp64 sums of raw squares lose the variance of 1000 +- 1e-3; the shifted sums use under half the bound"""
    rp, col = _long_rows_graph()
    X = R.input_set("offset", 64, 5, seed=2)
    r = R.segment_stats(rp, col, X)
    has = np.diff(rp) > 0
    share = lambda std: float((np.abs(std.astype(np.float64) - r["std"])[has] / r["std_bound"][has]).max())   # noqa: E731
    shifted, raw = share(R.kernel_moments(rp, col, X)[1]), share(R.kernel_moments(rp, col, X, shifted=False)[1])
    print("FIG offset set: shifted sums use %.3f of the std bound, unshifted %.1f" % (shifted, raw))
    assert shifted <= 0.5 and raw > 10.0


@pytest.mark.parametrize("name,rp,col", GRAPHS[1:], ids=[g[0] for g in GRAPHS[1:]])
def test_the_a_b_formulation_equals_torch_autograd_in_fp64(name, rp, col):
    n, D = len(rp) - 1, 5
    rng = np.random.default_rng(n)
    Z = rng.standard_normal((n, D))
    d = {a: rng.standard_normal((n, D)) for a in R.AGGREGATORS}
    r = R.segment_stats(rp, col, Z.astype(np.float64))
    a, b = R.coefficients(rp, d["mean"], d["std"], r["mean"], r["std"])
    dZ, _, _ = R.segment_stats_backward(rp, col, Z, a, b, r["argmax"], d["max"], r["argmin"], d["min"])
    Zt = torch.from_numpy(Z).requires_grad_(True)
    loss = torch.zeros((), dtype=torch.float64)
    for i in range(n):
        lo, hi = int(rp[i]), int(rp[i + 1])
        if hi > lo:
            M = Zt[torch.from_numpy(col[lo:hi]).long()]
            mean = M.mean(0)
            std = torch.sqrt(((M - mean) ** 2).mean(0) + 1e-5)
            for key, val in (("mean", mean), ("std", std), ("max", M.max(0).values), ("min", M.min(0).values)):
                loss = loss + (val * torch.from_numpy(d[key][i])).sum()
    want, = torch.autograd.grad(loss, Zt)
    assert np.abs(dZ - want.numpy()).max() <= 1e-12 * max(1.0, float(want.abs().max()))
    a_m, _ = R.coefficients(rp, d["mean"], None, None, None)                             # the groups alone add up to the whole
    a_s, b_s = R.coefficients(rp, None, d["std"], r["mean"], r["std"])
    parts = [R.segment_stats_backward(rp, col, Z, a=a_m)[0], R.segment_stats_backward(rp, col, Z, a=a_s, b=b_s)[0],
             R.segment_stats_backward(rp, col, Z, argmax=r["argmax"], dmax=d["max"])[0], R.segment_stats_backward(rp, col, Z, argmin=r["argmin"], dmin=d["min"])[0]]
    assert np.abs(sum(parts) - dZ).max() <= 1e-12 * max(1.0, float(np.abs(dZ).max()))


def test_the_library_declares_both_entries_and_refuses_on_the_host():
    import tcgnn_capi as C
    assert "tcgnn_segment_stats" in C.SIGNATURES and "tcgnn_segment_stats_backward" in C.SIGNATURES
    assert C.lib.tcgnn_abi_version() == 1
    fwd, bwd = C.lib.tcgnn_segment_stats, C.lib.tcgnn_segment_stats_backward
    fake = 4096                                                                           # never dereferenced: these calls return before any device work
    six = [fake] * 6
    assert fwd(fake, fake, 0, 5, fake, 8, 1e-5, *six, None) == 0                          # N = 0
    assert fwd(fake, fake, 9, 5, fake, 0, 1e-5, *six, None) == 0                          # D = 0
    assert fwd(fake, fake, 9, 5, fake, 8, 1e-5, *[None] * 6, None) == INVALID_ARG         # no output
    assert b"no output" in C.lib.tcgnn_last_error()
    assert fwd(fake, fake, 9, 5, fake, 8, 1e-5, None, None, None, fake, fake, fake, None) == INVALID_ARG   # argmax without max
    assert fwd(fake, fake, 9, 5, fake, 8, 1e-5, fake, None, fake, fake, None, fake, None) == INVALID_ARG   # argmin without min
    for bad in ((-1, 5, 8), (9, -1, 8), (9, 1 << 31, 8), (9, 5, -1)):
        assert fwd(fake, fake, bad[0], bad[1], fake, bad[2], 1e-5, *six, None) == INVALID_ARG
        assert bwd(fake, fake, fake, bad[0], bad[1], fake, fake, fake, fake, fake, fake, fake, bad[2], fake, None) == INVALID_ARG
    assert bwd(fake, fake, fake, 0, 5, fake, fake, fake, fake, fake, fake, fake, 8, fake, None) == 0       # N = 0
    assert bwd(fake, fake, fake, 9, 5, fake, fake, fake, fake, fake, fake, fake, 0, fake, None) == 0       # D = 0
    #                         Z     a     b     argmax dmax  argmin dmin
    for half in ((None, None, fake, None, None, None, None), (fake, None, None, None, None, None, None), (None, None, None, fake, None, None, None),
                 (None, None, None, None, fake, None, None), (None, None, None, None, None, fake, None), (None, None, None, None, None, None, fake)):
        assert bwd(fake, fake, fake, 9, 5, *half, 8, fake, None) == INVALID_ARG, half


# ---- PNAConv over a stand-in backend ----------------------------------------------------------------------------------------------------

def standin_backend():
    m = types.SimpleNamespace()
    npy = lambda *ts: [t.detach().cpu().numpy() for t in ts]   # noqa: E731

    def forward_stats(X, rp, col, aggregators=R.AGGREGATORS, eps=1e-5, return_arg=True):
        r = R.segment_stats(*npy(rp, col), X.detach().numpy(), eps)
        keys = [a for a in R.AGGREGATORS if a in aggregators] + (["arg" + a for a in ("max", "min") if a in aggregators] if return_arg else [])
        return {k: torch.from_numpy(np.ascontiguousarray(r[k].astype(np.int32 if k.startswith("arg") else np.float32))) for k in keys}

    def backward_stats(grads, saved, rp, col, out=None):
        rp_, col_ = npy(rp, col)
        g = {k: v.numpy() for k, v in grads.items() if v is not None}
        a = b = None
        if "mean" in g or "std" in g:
            a, b = R.coefficients(rp_, g.get("mean"), g.get("std"), saved["mean"].numpy() if "std" in g else None, saved["std"].numpy() if "std" in g else None)
        dZ, _, _ = R.segment_stats_backward(rp_, col_, saved["Z"].numpy(), a, b, saved["argmax"].numpy() if "max" in g else None, g.get("max"),
                                            saved["argmin"].numpy() if "min" in g else None, g.get("min"))
        return torch.from_numpy(dZ.astype(np.float32))

    m.forward_stats, m.backward_stats = forward_stats, backward_stats
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


def _directed40():
    import walks as W
    rp, col = graphs.uniform_graph(40, 2, seed=5, symmetric=False)
    assert not W.is_symmetric(rp, col) and (np.diff(rp) == 0).any()
    n = len(rp) - 1
    bp, e2c, e2r, _ = graphs.host_sgt(rp, col)
    A = torch.zeros(n, n, dtype=torch.float64)
    A.index_put_((torch.from_numpy(np.repeat(np.arange(n), np.diff(rp))), torch.from_numpy(col).long()), torch.ones(len(col), dtype=torch.float64), accumulate=True)
    return rp, col, [torch.from_numpy(a) for a in (rp, col, bp, e2c, e2r)], A


PNA_CASES = [((12, 7), {}), ((7, 12), {}), ((9, 9), {"aggregators": ("std", "min"), "scalers": ("attenuation",), "delta": 1.5, "message_dim": 4}),
             ((6, 5), {"aggregators": ("max",), "scalers": ("identity", "amplification"), "bias": False})]


@pytest.mark.parametrize("dims,kw", PNA_CASES, ids=["narrowing", "widening", "std_min_attenuation", "max_no_bias"])
def test_pna_layer_against_the_dense_fp64_model_on_a_directed_graph(layers, dims, kw):
    """output within 1e-5, gradients of X, every weight and both biases within 1e-4 of the largest entry (the project's layer bounds)"""
    rp, col, meta, A = _directed40()
    n = len(rp) - 1
    torch.manual_seed(3)
    conv = layers.PNAConv(*dims, **kw)
    names = ["weights_src", "weights_dst", "bias_pre", "weights_post", "bias_post"]
    if conv.bias_pre is not None:
        conv.bias_pre.data.normal_()
        conv.bias_post.data.normal_()
    X = torch.randn(n, dims[0])
    dY = torch.randn(n, dims[1], dtype=torch.float64)
    Xg = X.clone().requires_grad_(True)
    Y = conv(Xg, *meta)
    params = [getattr(conv, k) for k in names]
    leaves = [X.double().requires_grad_(True)] + [p.detach().double().requires_grad_(True) if p is not None else None for p in params]
    want = R.dense_pna(A, *leaves, aggregators=conv.aggregators, scalers=conv.scalers, delta=kw.get("delta"))
    assert conv.message_dim == kw.get("message_dim", min(dims))
    assert abs(float(conv.delta) - (kw["delta"] if "delta" in kw else float(torch.log(A.sum(1) + 1).mean()))) <= 1e-6
    assert _rel(Y, want) <= 1e-5
    got = torch.autograd.grad((Y * dY.float()).sum(), [Xg] + [p for p in params if p is not None])
    ref = torch.autograd.grad((want * dY).sum(), [t for t in leaves if t is not None])
    for g, r, what in zip(got, ref, ["X"] + [k for k, p in zip(names, params) if p is not None]):
        assert _rel(g, r) <= 1e-4, what
    lonely = int(np.nonzero(np.diff(rp) == 0)[0][0])
    alone = X[lonely] @ conv.weights_post[:dims[0]] + (conv.bias_post if conv.bias_post is not None else 0)
    assert torch.allclose(Y[lonely].detach(), alone.detach(), rtol=1e-5, atol=1e-6)          # no neighbours: X W_post[:input_dim] + b_post


def test_a_layer_without_delta_keeps_the_first_graphs(layers):
    rp, col, meta, A = _directed40()
    conv = layers.PNAConv(4, 4)
    assert conv.delta is None
    conv(torch.randn(40, 4), *meta)
    first = float(conv.delta)
    assert abs(first - float(layers.pna_delta(meta[0]))) <= 1e-7
    rp2, col2 = graphs.uniform_graph(40, 6, seed=1)
    bp, e2c, e2r, _ = graphs.host_sgt(rp2, col2)
    conv(torch.randn(40, 4), *[torch.from_numpy(a) for a in (rp2, col2, bp, e2c, e2r)])
    assert float(conv.delta) == first


def test_unknown_names_are_refused_and_the_harness_knows_the_model(layers):
    import tcgnn_edge_ops as E
    import tcgnn_harness as H
    with pytest.raises(ValueError, match="aggregators"):
        layers.PNAConv(4, 4, aggregators=("mean", "sum"))
    with pytest.raises(ValueError, match="scalers"):
        layers.PNAConv(4, 4, scalers=("identity", "linear"))
    with pytest.raises(ValueError, match="aggregators"):
        E.aggregate_stats(torch.zeros(3, 2), torch.zeros(4, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), aggregators=("var",))
    assert H.build_parser().parse_args(["--model", "pna"]).model == "pna"
    with pytest.raises(ValueError, match="SAGE model only"):
        H.time_training("pna", None, None, None, 4, 4, 2, 2, 1, aggregator="max")
    with pytest.raises(ValueError, match="heads applies"):
        H.time_training("pna", None, None, None, 4, 4, 2, 2, 1, heads=2)
