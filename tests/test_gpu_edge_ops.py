"""Edge softmax (tcgnn_edge_softmax / _backward), the two-operand SDDMM (tcgnn_sddmm2 = TCGNN.forward_ef2), the differentiable edge
operators and AGNNConv(attention="softmax") on the MI355X.  The restatements and the bounds are tests/edge_ops_ref.py's; the walks,
the catalogue of boundary-shaped graphs and the exception table are those of tests/test_gpu_structures.py."""
import glob
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import edge_ops_ref as R
import graphs
import test_gpu_structures as S
import walks as W
from test_gpu_parity import ROOT, assert_parity, meta_for, to_dev

pytestmark = pytest.mark.gpu

GUARD = 64        # sentinel words behind the edge arrays
NO_ROW = 24       # positions of the edge array that no row covers (behind nodePointer[N])
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def T():
    import TCGNN
    return TCGNN


@pytest.fixture(scope="module")
def ext():
    found = glob.glob(os.path.join(ROOT, "integration", "TCGNN*.so"))
    assert found, "integration/TCGNN*.so is not built"
    spec = importlib.util.spec_from_file_location("TCGNN", found[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- edge softmax ---------------------------------------------------------------------------------------------------------------

def _buffer(dev, values, E):
    """an fp32 device buffer of E + NO_ROW + GUARD words: the values, then sentinels; ([: E + NO_ROW] is what a call is handed)"""
    buf = torch.full((E + NO_ROW + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    buf[:E] = torch.from_numpy(values).to(dev)
    return buf


def _softmax_case(dev, T, rp, s, what):
    """forward and backward on one (row pointers, scores) pair in every call form -> list of failures"""
    bad = []
    E = int(rp[-1])
    trp = torch.from_numpy(np.ascontiguousarray(rp, dtype=np.int32)).to(dev)
    rng = np.random.default_rng(E + 1)
    dp = rng.standard_normal(E).astype(np.float32)
    for beta in (None, 0.37):
        b = 1.0 if beta is None else beta
        tb = None if beta is None else torch.tensor([beta], dtype=torch.float32, device=dev)
        p64, dist = R.softmax_f64(rp, s, b)
        sbuf = _buffer(dev, s, E)
        out = torch.full_like(sbuf, SENTINEL)
        p = T.edge_softmax(sbuf[:E + NO_ROW], trp, tb, out=out[:E + NO_ROW])
        again = T.edge_softmax(sbuf[:E + NO_ROW], trp, tb, out=torch.full_like(sbuf, SENTINEL)[:E + NO_ROW])
        got = p[:E].cpu().numpy()
        rel, abs_, rs = R.softmax_bounds_hold(rp, got, p64, dist) if E else (0.0, 0.0, 0.0)
        print("FIG softmax %-40s beta=%-5s relative %.3f absolute %.3f row sum %.3f (shares of the bounds)" % (what, beta, rel, abs_, rs))
        if E and not np.isfinite(got).all():
            bad.append("%s beta=%s: non-finite probabilities" % (what, beta))
        if max(rel, abs_, rs) > 1.0:
            bad.append("%s beta=%s: %.3f / %.3f / %.3f of the relative / absolute / row-sum bound" % (what, beta, rel, abs_, rs))
        if not torch.equal(p, again):
            bad.append("%s beta=%s: the second call returns other bits" % (what, beta))
        if not bool((out[E:] == SENTINEL).all()):
            bad.append("%s beta=%s: positions no row covers, or guard words, were written" % (what, beta))
        inplace = sbuf.clone()
        T.edge_softmax(inplace[:E + NO_ROW], trp, tb, out=inplace[:E + NO_ROW])       # d_p aliases d_score
        if not torch.equal(inplace[:E], p[:E]) or not bool((inplace[E:] == SENTINEL).all()):
            bad.append("%s beta=%s: the in-place call differs from the separate one" % (what, beta))

        # backward, from the kernel's own probabilities
        pin = got
        ds64, scale, db64, dscale = R.softmax_bwd_f64(rp, pin, dp, s, b)
        dpbuf = _buffer(dev, dp, E)
        dsout = torch.full_like(dpbuf, SENTINEL)
        ds, dbeta = T.edge_softmax_backward(out[:E + NO_ROW], dpbuf[:E + NO_ROW], trp, beta=tb, score=sbuf[:E + NO_ROW], need_dbeta=True, out=dsout[:E + NO_ROW])
        ds2, dbeta2 = T.edge_softmax_backward(out[:E + NO_ROW], dpbuf[:E + NO_ROW], trp, beta=tb, score=sbuf[:E + NO_ROW], need_dbeta=True)
        gds = ds[:E].cpu().numpy()
        c = R.bwd_worst(rp, gds, ds64, scale) if E else 0.0
        cb = abs(float(dbeta) - db64) / dscale if dscale > 0 else abs(float(dbeta))
        print("FIG softmax backward %-31s beta=%-5s c %.3e dbeta %.3e (bound %.1e)" % (what, beta, c, cb, R.C_BWD))
        if c > R.C_BWD or (E and not np.isfinite(gds).all()):
            bad.append("%s beta=%s: ds needs c = %.3e, the bound has %.1e" % (what, beta, c, R.C_BWD))
        if cb > R.C_BWD + 2.0 ** -24:      # (+ the fp32 result's own rounding)
            bad.append("%s beta=%s: dbeta %.3e of sum|s||g|" % (what, beta, cb))
        if not torch.equal(ds[:E], ds2[:E]) or not torch.equal(dbeta, dbeta2):
            bad.append("%s beta=%s: the second backward call returns other bits" % (what, beta))
        if not bool((dsout[E:] == SENTINEL).all()):
            bad.append("%s beta=%s: backward wrote positions no row covers, or guard words" % (what, beta))
        alias = dpbuf.clone()
        ds3, none = T.edge_softmax_backward(out[:E + NO_ROW], alias[:E + NO_ROW], trp, beta=tb, out=alias[:E + NO_ROW])   # d_ds aliases d_dp, no dbeta
        if none is not None or not torch.equal(alias[:E], ds[:E]) or not bool((alias[E:] == SENTINEL).all()):
            bad.append("%s beta=%s: the aliased backward call (no dbeta) differs" % (what, beta))
    return bad


@pytest.mark.parametrize("scores", ["normal_x1", "normal_x8", "normal_x30", "constant_rows", "magnitude_1e4"])
def test_edge_softmax_on_rows_of_every_length_class(dev, T, scores):
    rp = R.row_class_rowptr()
    bad = _softmax_case(dev, T, rp, R.score_sets(rp)[scores], "row classes / " + scores)
    assert not bad, "\n  ".join(bad)


@pytest.mark.parametrize("name", list(S.GRAPHS))
def test_edge_softmax_on_boundary_shaped_graphs(dev, T, name):
    rp, col = S.GRAPHS[name]
    E = int(rp[-1])
    rng = np.random.default_rng(len(rp))
    bad = _softmax_case(dev, T, rp, (8 * rng.standard_normal(E)).astype(np.float32), name)
    assert not bad, "\n  ".join(bad)


def test_edge_softmax_degenerate_sizes(dev, T):
    empty = torch.empty(0, dtype=torch.float32, device=dev)
    rp0 = torch.zeros(1, dtype=torch.int32, device=dev)
    assert T.edge_softmax(empty, rp0).numel() == 0                                   # N = 0
    rp5 = torch.zeros(6, dtype=torch.int32, device=dev)
    assert T.edge_softmax(empty, rp5).numel() == 0                                   # E = 0
    ds, db = T.edge_softmax_backward(empty, empty, rp5, score=empty, need_dbeta=True)
    assert ds.numel() == 0 and float(db) == 0.0
    # row pointers beyond the array are clamped: nothing behind E is touched
    buf = torch.full((100 + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    buf[:100] = 1.0
    wild = torch.tensor([0, 50, 40, 5000], dtype=torch.int32, device=dev)
    T.edge_softmax(buf[:100], wild, out=buf[:100])
    torch.cuda.synchronize()
    assert bool((buf[100:] == SENTINEL).all()) and bool(torch.isfinite(buf[:100]).all())


def test_binding_edge_softmax_equals_the_ctypes_module(dev, T, ext):
    """The pybind module's edge_softmax / edge_softmax_backward on the row-class graph: the same bits as the ctypes module in every
    call form (beta given and None, out= aliased, with and without dbeta), and its argument checks."""
    rp = R.row_class_rowptr()
    E = int(rp[-1])
    trp = torch.from_numpy(rp).to(dev)
    s = torch.from_numpy(R.score_sets(rp)["normal_x8"]).to(dev)
    dp = torch.randn(E, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    for beta in (None, torch.tensor([0.37], device=dev)):
        want = T.edge_softmax(s, trp, beta)
        got = ext.edge_softmax(s, trp, beta)
        assert torch.equal(got, want)
        inplace = s.clone()
        ret = ext.edge_softmax(inplace, trp, beta=beta, out=inplace)                     # d_p aliases d_score
        assert ret.data_ptr() == inplace.data_ptr() and torch.equal(inplace, want)
        ds_w, db_w = T.edge_softmax_backward(want, dp, trp, beta=beta, score=s, need_dbeta=True)
        ds, db = ext.edge_softmax_backward(want, dp, trp, beta=beta, score=s, need_dbeta=True)
        assert torch.equal(ds, ds_w) and db.shape == (1,) and torch.equal(db, db_w)
        alias = dp.clone()
        ds2, none = ext.edge_softmax_backward(want, alias, trp, beta=beta, out=alias)   # d_ds aliases d_dp, no dbeta
        assert none is None and ds2.data_ptr() == alias.data_ptr() and torch.equal(alias, ds_w)
    p = T.edge_softmax(s, trp)
    with pytest.raises(RuntimeError, match="beta must hold one fp32 value"):
        ext.edge_softmax(s, trp, torch.ones(2, device=dev))
    with pytest.raises(RuntimeError, match="beta must hold one fp32 value"):
        ext.edge_softmax(s, trp, torch.ones(1))
    with pytest.raises(RuntimeError, match="out must be a contiguous fp32 tensor"):
        ext.edge_softmax(s, trp, None, torch.empty(E + 1, device=dev))
    with pytest.raises(RuntimeError, match="out must be a contiguous fp32 tensor"):
        ext.edge_softmax_backward(p, dp, trp, out=torch.empty(E, device=dev, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="dbeta needs the scores"):
        ext.edge_softmax_backward(p, dp, trp, need_dbeta=True)
    with pytest.raises(RuntimeError, match="dp must have the shape"):
        ext.edge_softmax_backward(p, dp[:-1].contiguous(), trp)
    with pytest.raises(RuntimeError, match="nodePointer must hold"):
        ext.edge_softmax(s, trp.long())
    torch.cuda.synchronize()


@pytest.mark.parametrize("gen", ["sbm_reddit", "rmat"])
def test_edge_softmax_at_full_size(dev, T, gen):
    """The Reddit shape, with communities and as R-MAT (hub rows beyond 10^5 edges): 2 000 sampled rows and the 50 longest against
    softmax_f64, forward and backward."""
    import tcgnn_graph as G
    n, nnz, _, _ = G.SHAPES["reddit"]
    rp, col = G.GENERATORS[gen](n, nnz, seed=0, device=dev)
    E = col.numel()
    del col
    g = torch.Generator(device=dev).manual_seed(5)
    s = 4 * torch.randn(E, device=dev, generator=g)
    dp = torch.randn(E, device=dev, generator=g)
    beta = torch.tensor([0.8], device=dev)
    p = T.edge_softmax(s, rp, beta)
    assert torch.equal(p, T.edge_softmax(s, rp, beta))
    ds, dbeta = T.edge_softmax_backward(p, dp, rp, beta=beta, score=s, need_dbeta=True)
    ds2, dbeta2 = T.edge_softmax_backward(p, dp, rp, beta=beta, score=s, need_dbeta=True)
    assert torch.equal(ds, ds2) and torch.equal(dbeta, dbeta2)
    rph = rp.cpu().numpy().astype(np.int64)
    lens = np.diff(rph)
    rows = np.unique(np.concatenate([np.random.default_rng(1).choice(n, 2000, replace=False), np.argsort(lens)[-50:]]))
    print("FIG full size %s: E = %d, longest row %d" % (gen, E, lens.max()))
    worst = [0.0, 0.0, 0.0, 0.0]
    for r in rows:
        lo, hi = int(rph[r]), int(rph[r + 1])
        if hi == lo:
            continue
        seg = np.array([0, hi - lo])
        sh, ph, dh, gh = (t[lo:hi].cpu().numpy() for t in (s, p, dp, ds))
        p64, dist = R.softmax_f64(seg, sh, 0.8)
        rel, abs_, rs = R.softmax_bounds_hold(seg, ph, p64, dist)
        ds64, scale, _, _ = R.softmax_bwd_f64(seg, ph, dh, sh, 0.8)
        worst = [max(a, b) for a, b in zip(worst, (rel, abs_, rs, R.bwd_worst(seg, gh, ds64, scale)))]
    print("FIG full size %s: relative %.3f absolute %.3f row sum %.3f of the bounds, backward c %.3e" % (gen, *worst))
    assert max(worst[:3]) <= 1.0 and worst[3] <= R.C_BWD, worst
    # dbeta against fp64 on the device (sum_e s g, g = ds / beta)
    want = float((s.double() * (ds.double() / 0.8)).sum())
    scale = float((s.double().abs() * (ds.double() / 0.8).abs()).sum())
    assert abs(float(dbeta) - want) <= (R.C_BWD + 2.0 ** -24) * scale


# ---- the two-operand SDDMM on every walk ------------------------------------------------------------------------------------------

WIDTHS = (16, 41, 64, 128, 160)
EF2_CASES = [(name, D) for name in S.GRAPHS for D in WIDTHS]


def _kernel_ran(walk, name, D, kernel, pred, failures):
    """tests/test_gpu_structures._kernel_check for forward_ef2, under the same exception table (entries of forward_ef)"""
    if pred is None:
        return
    ran = bool(pred(kernel, D))
    if ("forward_ef", walk) in S.SAME_NAME:
        n = len(S.GRAPHS[name][0]) - 1
        nr = W.expected_ranges(n, D, S._CTX["buckets"], W.range_kb_for_eight(n, D))
        ran = ran and S._CTX["buckets"] > 0 and nr >= 8 and nr % 8 == 0
    print("OBS forward_ef2 | %s | %s | D=%d | %s | %s" % (walk, name, D, kernel, "ran" if ran else "OTHER"))
    if walk != "auto" and D > 128:
        if kernel != ("" if W.is_unsorted(name) else "sddmm_wide_kernel"):
            failures.append("forward_ef2 %s D=%d: %r" % (walk, D, kernel))
        return
    why = S.EXCEPTIONS.get(("forward_ef", walk, name))
    if why is None and not ran:
        failures.append("forward_ef2/%s: last_kernel is %r, not the forced kernel, and EXCEPTIONS has no entry for the pair" % (walk, kernel))
    if why is not None and ran:
        failures.append("forward_ef2/%s: EXCEPTIONS says %r, but the forced kernel ran (%r)" % (walk, why, kernel))


def _judge(got, refs, what, bad, bar=True):
    ref, r64, s64 = refs
    if not np.isfinite(got).all():
        bad.append("%s: non-finite scores" % what)
        return
    fig = (float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()), float((np.abs(got - ref) / (s64 + 1.0)).max()),
           float((np.abs(got - r64) / (s64 + 1.0)).max())) if got.size else (0.0, 0.0, 0.0)
    print("FIG %-60s bar %.2e tight %.2e fp64 %.2e" % (what, *fig))
    try:
        assert_parity(got, ref, r64, s64, what, unit_scale=bar)
    except AssertionError as e:
        bad.append(str(e) or "%s: beyond 2^-9 of the fp64 contract (%.3e)" % (what, fig[2]))


@pytest.mark.parametrize("name,D", EF2_CASES, ids=["%s-D%d" % c for c in EF2_CASES])
def test_forward_ef2_on_every_sddmm_walk(dev, T, ext, monkeypatch, capfd, name, D):
    rp, col = S.GRAPHS[name]
    n, nnz = len(rp) - 1, len(col)
    meta = S._meta(dev, name)
    info = T.plan_info(*meta)
    S._CTX.update(capfd=capfd, n=n, D=D, buckets=info["column_buckets"])
    X, _ = W.case_data(n, nnz, D)
    rng = np.random.default_rng(7 * D + n)
    Z = rng.standard_normal((n, D)).astype(np.float32)
    Zs = (Z * np.float32(2.0 ** -10)).astype(np.float32)          # the two operands at different scales
    cut = int(rp[min(W.windows_handed_over(name, n) * 16, n)])     # (`short_metadata`: scores of the windows not handed over stay zero)

    (ref, _), (r64, s64) = R.sddmm2_tf32(X, Z, rp, col), R.sddmm2_f64(X, Z, rp, col)
    for a in (ref, r64, s64):
        a[cut:] = 0
    # (a power of two on an operand, or on one of its rows, scales the rounded operands, every product and every sum exactly)
    ref_z, ref_s = (ref, r64, s64), tuple(a * 2.0 ** -10 for a in (ref, r64, s64))
    tX, tZ, tZs = to_dev(dev, X, Z, Zs)
    failures, first = [], None
    for walk in S._walks_for(name, "forward_ef"):
        mode, env, pred = W.SDDMM_WALKS[walk]

        def body():
            ext.clear_plan_cache()
            ef = T.forward_ef2(tX, tZ, *meta)[0]
            k = T.last_kernel(*meta)
            out = dict(ef=ef, kernel=k, again=T.forward_ef2(tX, tZ, *meta)[0], scaled=T.forward_ef2(tX, tZs, *meta)[0],
                       xx=T.forward_ef2(tX, tX, *meta)[0], kernel_xx=T.last_kernel(*meta), one=T.forward_ef(tX, *meta)[0], kernel_one=T.last_kernel(*meta),
                       ext=ext.forward_ef2(tX, tZ, *meta)[0], ext_xx=ext.forward_ef2(tX, tX, *meta)[0], ext_one=ext.forward_ef(tX, *meta)[0])
            ext.clear_plan_cache()
            return out
        try:
            o = S._forced(T, monkeypatch, mode, env, body)
        except RuntimeError as e:
            failures.append("forward_ef2 %s: %s" % (walk, e))
            continue
        bad = []
        _judge(o["ef"].cpu().numpy(), ref_z, "forward_ef2 %s %s D=%d (%s)" % (name, walk, D, o["kernel"]), bad)
        _judge(o["scaled"].cpu().numpy(), ref_s, "forward_ef2 %s %s D=%d, Z x 2^-10" % (name, walk, D), bad)
        if not torch.equal(o["ef"], o["again"]):
            bad.append("forward_ef2 %s: the second call returns other bits" % walk)
        if not torch.equal(o["xx"], o["one"]) or o["kernel_xx"] != o["kernel_one"]:
            bad.append("forward_ef2 %s: forward_ef2(X, X) differs in bits from forward_ef(X) (%r / %r)" % (walk, o["kernel_xx"], o["kernel_one"]))
        if not (torch.equal(o["ext"], o["ef"]) and torch.equal(o["ext_xx"], o["ext_one"]) and torch.equal(o["ext_one"], o["one"])):
            bad.append("forward_ef2 %s: the pybind module differs in bits from the ctypes one" % walk)
        if first is None:
            first = o["ef"]
        elif not torch.equal(o["ef"], first):
            bad.append("forward_ef2 %s: scores differ in bits from the automatic walk's" % walk)
        _kernel_ran(walk, name, D, o["kernel"], pred, bad)
        failures += bad

    # the range guard at its default level (2): one row of X, then one row of Z, 2^30 times the rest
    if nnz:
        hot = int(np.argmax(np.diff(rp)))
        edge_rows = np.repeat(np.arange(n), np.diff(rp))
        for which in ("X", "Z"):
            A, B = X.copy(), Z.copy()
            (A if which == "X" else B)[hot] *= np.float32(2.0 ** 30)
            factor = np.where((edge_rows if which == "X" else col) == hot, 2.0 ** 30, 1.0)
            r = tuple(a * factor for a in ref_z)
            got = T.forward_ef2(*to_dev(dev, A, B), *meta)[0].cpu().numpy()
            _judge(got, r, "forward_ef2 %s D=%d range guard, row %d of %s x 2^30" % (name, D, hot, which), failures, bar=False)
        T.clear_plan_cache()
    sys.stdout.write(capfd.readouterr().out)
    assert not failures, "%s D=%d:\n  " % (name, D) + "\n  ".join(failures)


# ---- the differentiable operators and the layer -------------------------------------------------------------------------------------

def _dense(rp, col):
    n = len(rp) - 1
    A = torch.zeros(n, n, dtype=torch.float64)
    A[torch.from_numpy(np.repeat(np.arange(n), np.diff(rp))).long(), torch.from_numpy(col).long()] = 1.0
    return A


def _close(got, want, what, tol=2e-3):
    got, want = got.detach().double().cpu(), want.detach().double()
    err, top = float((got - want).abs().max()), float(want.abs().max())
    print("FIG %-40s %.3e of the largest entry" % (what, err / max(top, 1e-300)))
    assert got.shape == want.shape and err <= tol * top, "%s: %.3e of the largest entry" % (what, err / max(top, 1e-300))


def _golden_graph():
    f = np.load(os.path.join(os.path.dirname(__file__), "golden", "layers_n200.npz"))
    return f["rowptr"], f["col"]


@pytest.mark.parametrize("name", ["layers_n200", "directed_n3000"])
def test_edge_functions_and_softmax_layer_against_dense_fp64(dev, T, name):
    """2e-3 of the largest entry: the project's 1e-3 operator bar through two chained operators - a condition, not a measurement"""
    import tcgnn_edge_ops as E
    import tcgnn_layers as L
    rp, col = _golden_graph() if name == "layers_n200" else graphs.powerlaw_graph(3000, 12, seed=31, symmetric=False)
    if name == "directed_n3000":
        assert not W.is_symmetric(rp, col)
    n, nnz = len(rp) - 1, len(col)
    A = _dense(rp, col)
    _, meta = meta_for(dev, rp, col)
    rows, cols = torch.from_numpy(np.repeat(np.arange(n), np.diff(rp))).long(), torch.from_numpy(col).long()
    torch.manual_seed(3)
    pair = lambda *shape: (lambda t: (t.float().to(dev).requires_grad_(True), t.clone().requires_grad_(True)))(torch.randn(*shape, dtype=torch.float64))

    (Xg, Xd), (Zg, Zd), w = pair(n, 24), pair(n, 24), torch.randn(nnz, dtype=torch.float64)
    ef = E.sddmm(Xg, Zg, meta)
    want = (Xd @ Zd.t())[rows, cols]
    _close(ef, want, name + " sddmm")
    got = torch.autograd.grad((ef * w.float().to(dev)).sum(), (Xg, Zg))
    ref = torch.autograd.grad((want * w).sum(), (Xd, Zd))
    _close(got[0], ref[0], name + " sddmm dX"); _close(got[1], ref[1], name + " sddmm dZ")

    (sg, sd) = pair(nnz)
    bg = torch.tensor([[0.7]], device=dev, requires_grad=True)
    bd = torch.tensor([[0.7]], dtype=torch.float64, requires_grad=True)
    p = E.edge_softmax(sg, meta[0], bg)
    Sd = torch.full((n, n), -float("inf"), dtype=torch.float64).index_put((rows, cols), bd.reshape(()) * sd)
    Sd = Sd.masked_fill(A.sum(1, keepdim=True) == 0, 0.0)
    want = torch.softmax(Sd, 1)[rows, cols]
    _close(p, want, name + " edge_softmax")
    got = torch.autograd.grad((p * w.float().to(dev)).sum(), (sg, bg))
    ref = torch.autograd.grad((want * w).sum(), (sd, bd))
    _close(got[0], ref[0], name + " edge_softmax ds")
    assert got[1].shape == bg.shape
    _close(got[1], ref[1], name + " edge_softmax dbeta")

    (Pg, Pd), (Hg, Hd), dY = pair(nnz), pair(n, 24), torch.randn(n, 24, dtype=torch.float64)
    Y = E.aggregate(Pg, Hg, meta)
    want = torch.zeros(n, n, dtype=torch.float64).index_put((rows, cols), Pd) @ Hd
    _close(Y, want, name + " aggregate")
    got = torch.autograd.grad((Y * dY.float().to(dev)).sum(), (Pg, Hg))
    ref = torch.autograd.grad((want * dY).sum(), (Pd, Hd))
    _close(got[0], ref[0], name + " aggregate dP"); _close(got[1], ref[1], name + " aggregate dH")

    conv = L.AGNNConv(24, 12, attention="softmax")
    conv.attention_w.data.fill_(1.7)
    Wd, betad = conv.weights.detach().double().clone().requires_grad_(True), conv.attention_w.detach().double().clone().requires_grad_(True)
    conv = conv.to(dev)
    Y = conv(Xg, *meta)
    want = R.dense_attention_model(A, Xd, Wd, betad)
    _close(Y, want, name + " layer")
    dY = torch.randn(n, 12, dtype=torch.float64)
    got = torch.autograd.grad((Y * dY.float().to(dev)).sum(), (Xg, conv.weights, conv.attention_w))
    ref = torch.autograd.grad((want * dY).sum(), (Xd, Wd, betad))
    for g, r, what in zip(got, ref, ("dX", "dW", "dbeta")):
        _close(g, r, name + " layer " + what)      # (dbeta, one number: 2e-3 of its own value)
    T.clear_plan_cache()


def _sbm(dev, n=5000, seed=9):
    rp, col = graphs.community_graph(n, 10, 24, 0.8, seed=seed)
    return rp, col, meta_for(dev, rp, col)[1]


def _model(dev, attention, seed=5):
    import tcgnn_layers as L
    torch.manual_seed(seed)
    return [cv.to(dev) for cv in (L.AGNNConv(32, 16, attention=attention), L.AGNNConv(16, 6, attention=attention))]


def _forward(convs, x, meta):
    return convs[1](torch.relu(convs[0](x, *meta)), *meta)


def _step(convs, x, y, meta):
    for cv in convs:
        for p in cv.parameters():
            p.grad = None
    loss = torch.nn.functional.cross_entropy(_forward(convs, x, meta), y)
    loss.backward()
    return loss


def test_softmax_agnn_training_step_allocates_nothing_does_not_synchronise_and_replays_bit_equal(dev, T):
    rp, col, meta = _sbm(dev)
    n = len(rp) - 1
    convs = _model(dev, "softmax")
    params = [p for cv in convs for p in cv.parameters()]
    x = torch.randn(n, 32, device=dev)
    y = torch.randint(0, 6, (n,), device=dev)
    T.prepare([16, 6], *meta, transpose=True, edge_valued=True, attention=True)
    for _ in range(2):
        _step(convs, x, y, meta)
        torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    _step(convs, x, y, meta)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == m0
    torch.cuda.set_sync_debug_mode("error")
    try:
        _step(convs, x, y, meta)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            _step(convs, x, y, meta)
        eager_loss = _step(convs, x, y, meta).detach().clone()
        eager_grads = [p.grad.clone() for p in params]
        for p in params:
            p.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            static_loss = torch.nn.functional.cross_entropy(_forward(convs, x, meta), y)
            static_loss.backward()
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_loss, eager_loss)
    for p, g in zip(params, eager_grads):
        assert p.grad is not None and torch.equal(p.grad, g)
    del graph
    T.clear_plan_cache()


def test_softmax_agnn_trains_where_the_reference_layer_does_not_stay_bounded(dev, T):
    """Twenty Adam steps on a 5 000-node SBM graph: with attention='softmax' the loss falls (mean of the last five steps below the mean
    of the first five) and every activation stays finite.  With attention='reference' on the same data the activations are printed,
    not asserted (DESIGN.md 4.10 records what the MI355X printed)."""
    rp, col, meta = _sbm(dev)
    n = len(rp) - 1
    g = torch.Generator().manual_seed(1)
    y = torch.from_numpy(np.arange(n) // ((n + 9) // 10) % 6).long()
    x = (torch.randn(n, 32, generator=g) + 0.5 * torch.nn.functional.one_hot(y, 32).float()).to(dev)
    y = y.to(dev)
    seen = {}
    for attention in ("softmax", "reference"):
        convs = _model(dev, attention)
        opt = torch.optim.Adam([p for cv in convs for p in cv.parameters()], lr=0.01)
        losses, top = [], 0.0
        for _ in range(20):
            opt.zero_grad()
            h = convs[0](x, *meta)
            out = convs[1](torch.relu(h), *meta)
            loss = torch.nn.functional.cross_entropy(out, y)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
            top = max(top, float(h.detach().abs().max()), float(out.detach().abs().max())) if np.isfinite(losses[-1]) else float("inf")
        seen[attention] = (losses, top)
        print("FIG training attention=%-9s loss %.4g -> %.4g (first five %.4g, last five %.4g), largest activation %.3g"
              % (attention, losses[0], losses[-1], np.mean(losses[:5]), np.mean(losses[-5:]), top))
    losses, top = seen["softmax"]
    assert np.isfinite(losses).all() and np.isfinite(top)
    assert np.mean(losses[-5:]) < np.mean(losses[:5]), losses
    T.clear_plan_cache()
