"""Multi-head GAT on the MI355X: the fused kernels (tcgnn_gat_softmax / _backward, tcgnn_edge_colsum) on rows of every length class, on
the boundary-shaped graphs and at degenerate sizes, the pybind module against the ctypes one, the differentiable operators and GATConv
against the dense fp64 model, and training.  The restatements, constants and input sets are tests/gat_ref.py's; the forward bounds
are tests/edge_ops_ref.py's, unchanged."""
import glob
import importlib.util
import os

import numpy as np
import pytest
import torch

import edge_ops_ref as R
import gat_ref as G
import graphs
import walks as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64        # sentinel words behind the arrays
NO_ROW = 24       # positions of every head's edge array that no row covers (behind nodePointer[N])
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


def _dev(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _meta(dev, rp, col):
    """the five metadata tensors of a graph on the device (host SGT)"""
    bp, e2c, e2r, _ = graphs.host_sgt(rp, col)
    return [_dev(dev, a) for a in (rp, col, bp, e2c, e2r)]


def _heads_buffer(dev, values, H, E):
    """(flat fp32 buffer of H (E + NO_ROW) + GUARD words, its [H, E + NO_ROW] view): the values [H, E], sentinels everywhere else"""
    Ep = E + NO_ROW
    buf = torch.full((H * Ep + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    view = buf[:H * Ep].view(H, Ep)
    if values is not None:
        view[:, :E] = _dev(dev, values)
    return buf, view


def _untouched(buf, view, E):
    return bool((view[:, E:] == SENTINEL).all()) and bool((buf[view.numel():] == SENTINEL).all())


_FWD_REF = {}     # (graph key, set, slope, head) -> (p64, dist): computed once, shared by the H = 1 / 3 / 8 cases, never changed
_TRANSPOSED = {}  # graph key -> (rowptr_t, perm) on the host


def _fwd_ref(key, rp, s32h, h):
    k = key + (h,)
    if k not in _FWD_REF:
        _FWD_REF[k] = R.softmax_f64(rp, s32h, 1.0)
    return _FWD_REF[k]


def _transposed(key, rp, col):
    if key not in _TRANSPOSED:
        rp_t, _, perm = W.transposed_csr(rp, col[:int(rp[-1])])
        _TRANSPOSED[key] = (rp_t.astype(np.int32), perm.astype(np.int32))
    return _TRANSPOSED[key]


def _gat_case(dev, T, key, rp, col, el, er, slope, what):
    """forward, backward (with d_er) and the column sums (d_el) on one graph and one (el, er) pair in every call form -> failures.
    The edge arrays are handed over NO_ROW entries longer than the rows cover; every output lies in a sentinel-filled buffer."""
    import tcgnn_capi as C
    bad = []
    rp = np.ascontiguousarray(rp, dtype=np.int32)
    n, E, H = len(rp) - 1, int(rp[-1]), el.shape[1]
    Ep = E + NO_ROW
    trp = _dev(dev, rp)
    colp = np.zeros(Ep, dtype=np.int32)
    colp[:E] = col[:E]
    tcol, tel, ter = _dev(dev, colp), _dev(dev, el), _dev(dev, er)
    stream = torch.cuda.current_stream().cuda_stream

    # forward
    s32 = G.gat_scores_f32(rp, col, el, er, slope)
    pbuf, pview = _heads_buffer(dev, None, H, E)
    p = T.gat_softmax(tel, ter, trp, tcol, slope, out=pview)
    pbuf2, pview2 = _heads_buffer(dev, None, H, E)
    T.gat_softmax(tel, ter, trp, tcol, slope, out=pview2)
    got = p[:, :E].cpu().numpy()
    shares = [0.0, 0.0, 0.0]
    for h in range(H):
        p64, dist = _fwd_ref(key + (slope,), rp, s32[h], h)
        if E:
            shares = [max(a, b) for a, b in zip(shares, R.softmax_bounds_hold(rp, got[h], p64, dist))]
    print("FIG gat softmax %-44s H=%d slope=%.1f relative %.3f absolute %.3f row sum %.3f (shares of the bounds)" % (what, H, slope, *shares))
    if not np.isfinite(got).all():
        bad.append("%s: non-finite probabilities" % what)
    if max(shares) > 1.0:
        bad.append("%s: %.3f / %.3f / %.3f of the relative / absolute / row-sum bound" % (what, *shares))
    if not torch.equal(pbuf, pbuf2):
        bad.append("%s: the second forward call returns other bits" % what)
    if not _untouched(pbuf, pview, E):
        bad.append("%s: forward wrote positions no row covers, or guard words" % what)

    # backward, from the kernel's own probabilities
    dp = np.random.default_rng(E + 7 * H + 1).standard_normal((H, E)).astype(np.float32)
    ref = G.gat_bwd_f64(rp, col, el, er, slope, got, dp)
    dpbuf, dpview = _heads_buffer(dev, dp, H, E)
    dsbuf, dsview = _heads_buffer(dev, None, H, E)
    ds, d_er = T.gat_softmax_backward(pview, dpview, tel, ter, trp, tcol, slope, out=dsview)
    # ... and straight through the C ABI, d_er into a guarded buffer
    dsbuf2, dsview2 = _heads_buffer(dev, None, H, E)
    erbuf = torch.full((n * H + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    st = C.lib.tcgnn_gat_softmax_backward(trp.data_ptr(), tcol.data_ptr(), n, Ep, H, tel.data_ptr(), ter.data_ptr(), slope, pview.data_ptr(),
                                          dpview.data_ptr(), dsview2.data_ptr(), erbuf.data_ptr(), stream)
    assert st == 0, C.lib.tcgnn_last_error()
    gds, ger = ds[:, :E].cpu().numpy(), d_er.cpu().numpy()
    rows = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
    cols = np.asarray(col[:E], dtype=np.int64)
    c = G.ds_worst(rp, gds, ref) if E else 0.0
    cr, own_r = G.sum_worst(ger, ref["d_er"], ref["d_er_scale"]), G.sum_of_own_terms_worst(ger, gds, rows, n)
    print("FIG gat backward %-43s H=%d slope=%.1f ds c %.3e (bound %.1e), d_er %.3e of sum|ds64| (bound %.1f) and %.3e of its own terms (bound %.1e)"
          % (what, H, slope, c, G.C_GAT_BWD, cr, G.C_GAT_SUM, own_r, G.OWN_SUM))
    if c > G.C_GAT_BWD or not np.isfinite(gds).all():
        bad.append("%s: ds needs c = %.3e, the bound has %.1e" % (what, c, G.C_GAT_BWD))
    if cr > G.C_GAT_SUM or own_r > G.OWN_SUM or not np.isfinite(ger).all():
        bad.append("%s: d_er needs %.3e of sum |ds64| and %.3e of its own terms" % (what, cr, own_r))
    if not torch.equal(dsbuf, dsbuf2) or not torch.equal(erbuf[:n * H].view(n, H), d_er):
        bad.append("%s: the second backward call returns other bits" % what)
    if not _untouched(dsbuf, dsview, E) or not bool((erbuf[n * H:] == SENTINEL).all()):
        bad.append("%s: backward wrote positions no row covers, or guard words" % what)
    alias_buf, alias = _heads_buffer(dev, dp, H, E)
    ds3, d_er3 = T.gat_softmax_backward(pview, alias, tel, ter, trp, tcol, slope, out=alias)      # ds aliases dp
    if ds3.data_ptr() != alias.data_ptr() or not torch.equal(alias_buf, dsbuf) or not torch.equal(d_er3, d_er):
        bad.append("%s: the aliased backward call differs from the separate one" % what)

    # d_el = the column sums of ds, over the transposed CSR of tests/walks.py
    rp_t, perm = _transposed(key[:1], rp, col)
    trp_t, tperm = _dev(dev, rp_t), _dev(dev, perm if E else np.zeros(1, np.int32))
    outs = []
    for _ in range(2):
        obuf = torch.full((n * H + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        st = C.lib.tcgnn_edge_colsum(trp_t.data_ptr(), tperm.data_ptr(), n, Ep, H, dsview.data_ptr(), obuf.data_ptr(), stream)
        assert st == 0, C.lib.tcgnn_last_error()
        outs.append(obuf)
    gel = outs[0][:n * H].view(n, H).cpu().numpy()
    cl, own_l = G.sum_worst(gel, ref["d_el"], ref["d_el_scale"]), G.sum_of_own_terms_worst(gel, gds, cols, n)
    print("FIG gat colsum %-45s H=%d slope=%.1f d_el %.3e of sum|ds64| (bound %.1f) and %.3e of its own terms (bound %.1e)"
          % (what, H, slope, cl, G.C_GAT_SUM, own_l, G.OWN_SUM))
    if cl > G.C_GAT_SUM or own_l > G.OWN_SUM or not np.isfinite(gel).all():
        bad.append("%s: d_el needs %.3e of sum |ds64| and %.3e of its own terms" % (what, cl, own_l))
    if not torch.equal(outs[0], outs[1]):
        bad.append("%s: the second column-sum call returns other bits" % what)
    if not bool((outs[0][n * H:] == SENTINEL).all()):
        bad.append("%s: the column sums wrote guard words" % what)
    torch.cuda.synchronize()
    return bad


ROW_CASES = [(H, slope, name) for H in G.HEADS for slope in G.SLOPES for name in G.SETS]


@pytest.mark.parametrize("H,slope,name", ROW_CASES, ids=["H%d-slope%.1f-%s" % c for c in ROW_CASES])
def test_gat_kernels_on_rows_of_every_length_class(dev, T, H, slope, name):
    rp, col = G.row_class_graph()
    el, er = G.el_er_sets(len(rp) - 1)[name]
    bad = _gat_case(dev, T, ("row_classes", name), rp, col, np.ascontiguousarray(el[:, :H]), np.ascontiguousarray(er[:, :H]), slope,
                    "row classes / " + name)
    assert not bad, "\n  ".join(bad)


def test_one_head_without_a_destination_term_is_the_edge_softmax_of_the_gathered_scores(dev, T):
    """slope = 1, er = 0, H = 1: the score is el[col e] itself, so p is edge_softmax(el[col]) within the same bounds; with the building
    blocks shared the bits are expected to agree too - printed, not asserted"""
    rp, col = G.row_class_graph()
    n, E = len(rp) - 1, int(rp[-1])
    trp, tcol = _dev(dev, rp), _dev(dev, col)
    for name, (el, _) in G.el_er_sets(n).items():
        el1 = np.ascontiguousarray(el[:, :1])
        tel = _dev(dev, el1)
        p = T.gat_softmax(tel, torch.zeros_like(tel), trp, tcol, 1.0)
        s = el1[col.astype(np.int64), 0]
        q = T.edge_softmax(_dev(dev, s), trp)
        p64, dist = R.softmax_f64(rp, s, 1.0)
        shares = R.softmax_bounds_hold(rp, p[0].cpu().numpy(), p64, dist)
        print("FIG gat softmax as edge_softmax %-14s shares %.3f %.3f %.3f, bit-equal to edge_softmax: %s" % (name, *shares, torch.equal(p[0], q)))
        assert max(shares) <= 1.0 and max(R.softmax_bounds_hold(rp, q.cpu().numpy(), p64, dist)) <= 1.0, (name, shares)
        assert p.shape == (1, E)


def test_gat_kernels_at_full_size_with_four_heads(dev, T):
    """The Reddit shape with communities (114.6 M edges), H = 4: 2 000 sampled rows and the 50 longest against the fp64 softmax of the
    fp32 scores formed ON THE HOST from el / er and the row's own column ids (no device gather takes part in the reference), forward and
    backward; d_er of the sampled rows against the fp64 sums of the kernel's own ds."""
    import tcgnn_graph as TG
    n, nnz, _, _ = TG.SHAPES["reddit"]
    rp, col = TG.GENERATORS["sbm_reddit"](n, nnz, seed=0, device=dev)
    E, H, slope = col.numel(), 4, 0.2
    g = torch.Generator(device=dev).manual_seed(4)
    el, er = torch.randn(n, H, device=dev, generator=g), torch.randn(n, H, device=dev, generator=g)
    dp = torch.randn(H, E, device=dev, generator=g)
    p = T.gat_softmax(el, er, rp, col, slope)
    assert torch.equal(p, T.gat_softmax(el, er, rp, col, slope))
    ds, d_er = T.gat_softmax_backward(p, dp, el, er, rp, col, slope)
    elh, erh = el.cpu().numpy(), er.cpu().numpy()
    rph = rp.cpu().numpy().astype(np.int64)
    lens = np.diff(rph)
    rows = np.unique(np.concatenate([np.random.default_rng(1).choice(n, 2000, replace=False), np.argsort(lens)[-50:]]))
    worst = [0.0, 0.0, 0.0, 0.0, 0.0]
    for r in rows:
        lo, hi = int(rph[r]), int(rph[r + 1])
        if hi == lo:
            assert not bool(d_er[r].any())
            continue
        seg = np.array([0, hi - lo], dtype=np.int32)
        ch = col[lo:hi].cpu().numpy()
        ph, dh, gh = (t[:, lo:hi].cpu().numpy() for t in (p, dp, ds))
        raw = (elh[ch] + erh[r]).T.astype(np.float32)                                   # [H, len]: fl32(el[col e, h] + er[row, h])
        s32 = np.where(raw > 0, raw, raw * np.float32(slope)).astype(np.float32)
        for h in range(H):
            p64, dist = R.softmax_f64(seg, s32[h], 1.0)
            rel, abs_, rs = R.softmax_bounds_hold(seg, ph[h], p64, dist)
            ds64, scale, _, _ = R.softmax_bwd_f64(seg, ph[h], dh[h])
            ds64 = ds64 * np.where(raw[h] > 0, 1.0, np.float64(np.float32(slope)))
            c = R.bwd_worst(seg, gh[h], ds64, scale)
            S, A = float(gh[h].astype(np.float64).sum()), float(np.abs(gh[h].astype(np.float64)).sum())
            own = max(abs(float(d_er[r, h]) - S) - 2.0 ** -24 * abs(S) - 2.0 ** -149, 0.0) / A if A > 0 else 0.0
            worst = [max(a, b) for a, b in zip(worst, (rel, abs_, rs, c, own))]
    print("FIG gat full size H=4: relative %.3f absolute %.3f row sum %.3f of the bounds, backward c %.3e, d_er %.3e of its own terms" % tuple(worst))
    assert max(worst[:3]) <= 1.0 and worst[3] <= G.C_GAT_BWD and worst[4] <= G.OWN_SUM, worst


BOUNDARY = {name: (rp, col) for name, rp, col in graphs.boundary_graphs() + graphs.edge_case_graphs()}


@pytest.mark.parametrize("name", list(BOUNDARY))
def test_gat_kernels_on_boundary_shaped_graphs(dev, T, name):
    rp, col = BOUNDARY[name]
    n = len(rp) - 1
    rng = np.random.default_rng(n)
    el, er = (8 * rng.standard_normal((n, 3))).astype(np.float32), (8 * rng.standard_normal((n, 3))).astype(np.float32)
    bad = _gat_case(dev, T, (name, "normal_x8"), rp, col, el, er, 0.2, name)
    assert not bad, "\n  ".join(bad)


def test_gat_kernels_at_degenerate_sizes(dev, T):
    import tcgnn_capi as C
    stream = torch.cuda.current_stream().cuda_stream
    H = 3
    # N = 1 with a self loop; N = 45 (not a multiple of 32) is among the boundary graphs' sizes too
    for n, (rp, col) in ((1, (np.array([0, 1], np.int32), np.array([0], np.int32))), (45, graphs.uniform_graph(45, 4, seed=3, symmetric=False))):
        rng = np.random.default_rng(n)
        el, er = rng.standard_normal((n, H)).astype(np.float32), rng.standard_normal((n, H)).astype(np.float32)
        bad = _gat_case(dev, T, ("degenerate_n%d" % n, "normal_x1"), rp, col, el, er, 0.2, "N = %d" % n)
        assert not bad, "\n  ".join(bad)
    # E = 0 with N > 0: nothing to normalise, d_er and the column sums are all zero
    n = 37
    rp0 = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    col0 = torch.zeros(0, dtype=torch.int32, device=dev)
    el = torch.randn(n, H, device=dev)
    empty = torch.zeros(H, 0, device=dev)
    assert T.gat_softmax(el, el, rp0, col0).shape == (H, 0)
    ds, d_er = T.gat_softmax_backward(empty, empty, el, el, rp0, col0)
    assert ds.shape == (H, 0) and d_er.shape == (n, H) and not bool(d_er.any())
    obuf = torch.full((n * H + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    assert C.lib.tcgnn_edge_colsum(rp0.data_ptr(), rp0.data_ptr(), n, 0, H, rp0.data_ptr(), obuf.data_ptr(), stream) == 0
    assert not bool(obuf[:n * H].any()) and bool((obuf[n * H:] == SENTINEL).all())
    # a row-pointer array with a descending pair and an entry beyond the array: clamped, the descending pair an empty row
    E = 100
    wild = torch.tensor([0, 50, 40, 5000], dtype=torch.int32, device=dev)      # rows: [0, 50), empty, [40, 100)
    col = torch.arange(E, dtype=torch.int32, device=dev) % 3
    el3, er3 = torch.randn(3, H, device=dev), torch.randn(3, H, device=dev)
    pbuf = torch.full((H * E + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    p = T.gat_softmax(el3, er3, wild, col, 0.2, out=pbuf[:H * E].view(H, E))
    dsbuf = torch.full((H * E + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    ds, d_er = T.gat_softmax_backward(p, torch.ones_like(p), el3, er3, wild, col, 0.2, out=dsbuf[:H * E].view(H, E))
    torch.cuda.synchronize()
    assert bool((pbuf[H * E:] == SENTINEL).all()) and bool((dsbuf[H * E:] == SENTINEL).all())
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(ds).all()) and bool(torch.isfinite(d_er).all())
    assert not bool(d_er[1].any())                                                  # the descending pair: an empty row
    assert abs(float(p[:, 40:].sum()) - H) < 1e-4                                   # the last row is normalised over [40, 100)
    # column ids and perm entries out of range are clamped for the reads they index: nothing faults, everything stays finite
    badcol = col.clone()
    badcol[::7] = 1 << 30
    badcol[3::7] = -5
    tame = torch.tensor([0, 50, 50, 100], dtype=torch.int32, device=dev)
    p = T.gat_softmax(el3, er3, tame, badcol, 0.2)
    obuf = torch.full((3 * H + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    assert C.lib.tcgnn_edge_colsum(tame.data_ptr(), badcol.data_ptr(), 3, E, H, p.data_ptr(), obuf.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(obuf).all()) and bool((obuf[3 * H:] == SENTINEL).all())


def test_binding_gat_functions_equal_the_ctypes_module(dev, T, ext):
    rp, col = graphs.powerlaw_graph(3000, 12, seed=31, symmetric=False)
    n, E, H = len(rp) - 1, len(col), 3
    trp, tcol = _dev(dev, rp), _dev(dev, col)
    g = torch.Generator(device=dev).manual_seed(4)
    el, er = 4 * torch.randn(n, H, device=dev, generator=g), 4 * torch.randn(n, H, device=dev, generator=g)
    dp = torch.randn(H, E, device=dev, generator=g)
    want = T.gat_softmax(el, er, trp, tcol, 0.3)
    assert torch.equal(ext.gat_softmax(el, er, trp, tcol, 0.3), want)
    out = torch.empty_like(want)
    assert ext.gat_softmax(el, er, trp, tcol, negative_slope=0.3, out=out).data_ptr() == out.data_ptr() and torch.equal(out, want)
    ds_w, er_w = T.gat_softmax_backward(want, dp, el, er, trp, tcol, 0.3)
    ds, d_er = ext.gat_softmax_backward(want, dp, el, er, trp, tcol, 0.3)
    assert torch.equal(ds, ds_w) and torch.equal(d_er, er_w) and d_er.shape == (n, H)
    alias = dp.clone()
    ds2, _ = ext.gat_softmax_backward(want, alias, el, er, trp, tcol, negative_slope=0.3, out=alias)
    assert ds2.data_ptr() == alias.data_ptr() and torch.equal(alias, ds_w)
    el_w = T.edge_colsum(ds_w, trp, tcol)
    assert torch.equal(ext.edge_colsum(ds_w, trp, tcol), el_w) and torch.equal(ext.edge_colsum(ds_w, trp, tcol), el_w) and el_w.shape == (n, H)
    # (against torch's own scatter, in fp64)
    ref = torch.zeros(n, H, dtype=torch.float64, device=dev).index_add_(0, tcol.long(), ds_w.double().t())
    assert float((el_w.double() - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
    with pytest.raises(RuntimeError, match="heads"):
        ext.gat_softmax(el, er[:, :2].contiguous(), trp, tcol)
    with pytest.raises(RuntimeError, match="out must be a contiguous fp32"):
        ext.gat_softmax(el, er, trp, tcol, 0.2, torch.empty(H, E + 1, device=dev))
    with pytest.raises(RuntimeError, match="dp must be a contiguous fp32"):
        ext.gat_softmax_backward(want, dp[:, :-1].contiguous(), el, er, trp, tcol)
    with pytest.raises(RuntimeError, match="val must be"):
        ext.edge_colsum(ds_w[:, :-1].contiguous(), trp, tcol)
    with pytest.raises(RuntimeError, match="heads"):
        T.gat_softmax(el, er[:, :2].contiguous(), trp, tcol)
    with pytest.raises(RuntimeError, match="val must be"):
        T.edge_colsum(ds_w[:, :-1].contiguous(), trp, tcol)
    torch.cuda.synchronize()
    ext.clear_plan_cache()
    T.clear_plan_cache()


# ---- the differentiable operators and the layer against the dense fp64 model ----------------------------------------------------------

def _close(got, want, what, tol=G.GPU_LAYER_TOL):
    got, want = got.detach().double().cpu(), want.detach().double()
    err, top = float((got - want).abs().max()), float(want.abs().max())
    print("FIG %-44s %.3e of the largest entry" % (what, err / max(top, 1e-300)))
    assert got.shape == want.shape and err <= tol * top, "%s: %.3e of the largest entry" % (what, err / max(top, 1e-300))


@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
@pytest.mark.parametrize("name", ["layers_n200", "directed_n3000"])
def test_gat_operators_and_layer_against_dense_fp64(dev, T, name, concat):
    """2e-3 of the largest entry: the project's condition for chained operators (tests/test_gpu_edge_ops.py); tests/test_gat_cpu.py shows
    that operand rounding alone stays inside half of it on these inputs"""
    import tcgnn_edge_ops as E
    import tcgnn_layers as L
    rp, col, X, Wt, al, ar, b, dY = G.gpu_layer_case(name, concat)
    if name == "directed_n3000":
        assert not W.is_symmetric(rp, col)
    n, nnz, H, Fo = len(rp) - 1, len(col), G.LAYER_CASE["heads"], G.LAYER_CASE["out"]
    A = G.dense_adjacency(rp, col)
    meta = _meta(dev, rp, col)
    rows, cols = torch.from_numpy(np.repeat(np.arange(n), np.diff(rp))).long(), torch.from_numpy(col).long()
    f32 = lambda t: t.float().to(dev).requires_grad_(True)   # noqa: E731
    f64 = lambda t: t.clone().requires_grad_(True)           # noqa: E731

    if concat:     # the two operators on their own (once per graph)
        g = torch.Generator().manual_seed(11)
        el, er, w = (torch.randn(*s, dtype=torch.float64, generator=g) for s in ((n, H), (n, H), (H, nnz)))
        eg, rg, ed, rd = f32(el), f32(er), f64(el), f64(er)
        P = E.gat_attention(eg, rg, meta[0], meta[1], 0.2)
        S = torch.nn.functional.leaky_relu(ed.t().unsqueeze(1) + rd.t().unsqueeze(2), 0.2)                 # [H, dst, src]
        S = S.masked_fill(A.unsqueeze(0) == 0, float("-inf")).masked_fill(A.sum(1).view(1, n, 1) == 0, 0.0)
        want = torch.softmax(S, 2)[:, rows, cols]
        _close(P, want, name + " gat_attention")
        got = torch.autograd.grad((P * w.float().to(dev)).sum(), (eg, rg))
        ref = torch.autograd.grad((want * w).sum(), (ed, rd))
        _close(got[0], ref[0], name + " gat_attention d_el"); _close(got[1], ref[1], name + " gat_attention d_er")
        Pv, Z, dZ = (torch.randn(*s, dtype=torch.float64, generator=g) for s in ((H, nnz), (n, H * Fo), (n, H * Fo)))
        pg, zg, pd, zd = f32(Pv), f32(Z), f64(Pv), f64(Z)
        Y = E.aggregate_heads(pg, zg, meta)
        want = torch.cat([torch.zeros(n, n, dtype=torch.float64).index_put((rows, cols), pd[h]) @ zd[:, h * Fo:(h + 1) * Fo] for h in range(H)], 1)
        _close(Y, want, name + " aggregate_heads")
        got = torch.autograd.grad((Y * dZ.float().to(dev)).sum(), (pg, zg))
        ref = torch.autograd.grad((want * dZ).sum(), (pd, zd))
        _close(got[0], ref[0], name + " aggregate_heads dP"); _close(got[1], ref[1], name + " aggregate_heads dZ")

    conv = L.GATConv(X.shape[1], Fo, heads=H, concat=concat)
    for prm, val in ((conv.weights, Wt), (conv.attn_l, al), (conv.attn_r, ar), (conv.bias, b)):
        prm.data.copy_(val.float())
    conv = conv.to(dev)
    Xg = f32(X)
    Y = conv(Xg, *meta)
    leaves = [f64(t) for t in (X, Wt, al, ar, b)]
    want = G.dense_gat_model(A, *leaves, heads=H, concat=concat)
    what = "%s layer %s " % (name, "concat" if concat else "mean")
    _close(Y, want, what + "Y")
    got = torch.autograd.grad((Y * dY.float().to(dev)).sum(), (Xg, conv.weights, conv.attn_l, conv.attn_r, conv.bias))
    ref = torch.autograd.grad((want * dY).sum(), leaves)
    for g_, r_, k in zip(got, ref, ("dX", "dW", "dattn_l", "dattn_r", "dbias")):
        _close(g_, r_, what + k)
    lonely = np.nonzero(np.diff(rp) == 0)[0]
    if len(lonely):
        assert torch.equal(Y[int(lonely[0])].detach(), conv.bias.detach())       # a node without incoming edges gets the bias only
    T.clear_plan_cache()


# ---- training --------------------------------------------------------------------------------------------------------------------------

def _sbm(dev, n=5000, seed=9):
    rp, col = graphs.community_graph(n, 10, 24, 0.8, seed=seed)
    return rp, col, _meta(dev, rp, col)


def _model(dev, seed=5):
    import tcgnn_layers as L
    torch.manual_seed(seed)
    return [cv.to(dev) for cv in (L.GATConv(32, 8, heads=4), L.GATConv(32, 6, heads=1))]


def _forward(convs, x, meta):
    return convs[1](torch.nn.functional.elu(convs[0](x, *meta)), *meta)


def test_two_identical_gat_training_steps_give_bit_equal_gradients_and_a_prepared_step_builds_nothing(dev, T):
    rp, col, meta = _sbm(dev)
    n = len(rp) - 1
    convs = _model(dev)
    params = [p for cv in convs for p in cv.parameters()]
    x = torch.randn(n, 32, device=dev)
    y = torch.randint(0, 6, (n,), device=dev)
    T.prepare([8, 6], *meta, transpose=True, edge_valued=True, attention=True)
    grads = []
    for _ in range(2):
        for p in params:
            p.grad = None
        torch.nn.functional.cross_entropy(_forward(convs, x, meta), y).backward()
        grads.append([p.grad.clone() for p in params])
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads[0])
    for p, a, b in zip(params, *grads):
        assert torch.equal(a, b), tuple(p.shape)
    # behind prepare(per-head widths, transpose, edge_valued, attention) a step builds nothing: the same bytes stay allocated, and
    # no call synchronises - the transposed CSR edge_colsum reads came with A^T's plan
    def step():
        for p in params:
            p.grad = None
        torch.nn.functional.cross_entropy(_forward(convs, x, meta), y).backward()
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == m0
    torch.cuda.set_sync_debug_mode("error")
    try:
        step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    T.clear_plan_cache()


def test_gat_trains(dev, T):
    """Twenty Adam steps of a two-layer GAT (4 heads of 8, then one head of 6 classes) on a 5 000-node community graph: the loss falls
    (mean of the last five steps below the mean of the first five) and every activation stays finite"""
    rp, col, meta = _sbm(dev)
    n = len(rp) - 1
    g = torch.Generator().manual_seed(1)
    y = torch.from_numpy(np.arange(n) // ((n + 9) // 10) % 6).long()
    x = (torch.randn(n, 32, generator=g) + 0.5 * torch.nn.functional.one_hot(y, 32).float()).to(dev)
    y = y.to(dev)
    convs = _model(dev)
    opt = torch.optim.Adam([p for cv in convs for p in cv.parameters()], lr=0.01)
    losses, top = [], 0.0
    for _ in range(20):
        opt.zero_grad()
        h = convs[0](x, *meta)
        out = convs[1](torch.nn.functional.elu(h), *meta)
        loss = torch.nn.functional.cross_entropy(out, y)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        top = max(top, float(h.detach().abs().max()), float(out.detach().abs().max())) if np.isfinite(losses[-1]) else float("inf")
    print("FIG gat training loss %.4g -> %.4g (first five %.4g, last five %.4g), largest activation %.3g"
          % (losses[0], losses[-1], np.mean(losses[:5]), np.mean(losses[-5:]), top))
    assert np.isfinite(losses).all() and np.isfinite(top)
    assert np.mean(losses[-5:]) < np.mean(losses[:5]), losses
    T.clear_plan_cache()
