"""GATv2 on the MI355X: the three kernels (tcgnn_gatv2_softmax / _backward / tcgnn_gatv2_source_grad) on rows of every length class -
by destination and, on the transposed graph, by source -, at every lane layout, one float off alignment and at degenerate sizes, the
pybind module against the ctypes one, the differentiable operator and GATv2Conv against the dense fp64 model, and training.  The
restatements, the bounds with their derivations and the input sets are tests/gatv2_ref.py's; the softmax and g bounds are
tests/edge_ops_ref.py's and tests/gat_ref.py's, unchanged.  Out-of-range column ids and perm entries are NOT handed to the kernels
here: the clamps are contract, kept by reading (tcgnn_gatv2.inc's header says where they are)."""
import glob
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import gat_ref as G
import gatv2_ref as V
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


def _node_buffer(dev, n, D):
    buf = torch.full((n * D + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[:n * D].view(n, D)


def _untouched(buf, view, E):
    return bool((view[:, E:] == SENTINEL).all()) and bool((buf[view.numel():] == SENTINEL).all())


_TRANSPOSED = {}  # graph key -> (rowptr_t, col_t, perm) on the host, built once


def _transposed(key, rp, col):
    if key not in _TRANSPOSED:
        rp_t, col_t, perm = W.transposed_csr(rp, col[:int(rp[-1])])
        _TRANSPOSED[key] = (rp_t.astype(np.int32), col_t.astype(np.int32), perm.astype(np.int32))
    return _TRANSPOSED[key]


def _gatv2_case(dev, key, rp, col, xl, xr, attn, slope, what, xl_is_xr=False):
    """The three kernels through the C ABI on one graph and one (xl, xr, attn) -> failures.  The edge arrays are handed over NO_ROW
    entries longer than the rows cover and every output lies in a sentinel-filled buffer; every call runs twice (with and without
    d_score in forward), bits compared."""
    import tcgnn_capi as C
    bad = []
    rp = np.ascontiguousarray(rp, dtype=np.int32)
    n, E = len(rp) - 1, int(rp[-1])
    H, F = attn.shape
    HF, Ep = H * F, E + NO_ROW
    trp = _dev(dev, rp)
    colp = np.zeros(Ep, dtype=np.int32)
    colp[:E] = col[:E]
    tcol, txl, tattn = _dev(dev, colp), _dev(dev, xl), _dev(dev, attn)
    txr = txl if xl_is_xr else _dev(dev, xr)
    stream = torch.cuda.current_stream().cuda_stream
    lib = C.lib

    # forward: with the scores, then without
    pbuf, pview = _heads_buffer(dev, None, H, E)
    sbuf, sview = _heads_buffer(dev, None, H, E)
    pbuf2, pview2 = _heads_buffer(dev, None, H, E)
    st = lib.tcgnn_gatv2_softmax(trp.data_ptr(), tcol.data_ptr(), n, Ep, H, F, txl.data_ptr(), txr.data_ptr(), tattn.data_ptr(), slope,
                                 sview.data_ptr(), pview.data_ptr(), stream)
    assert st == 0, lib.tcgnn_last_error()
    st = lib.tcgnn_gatv2_softmax(trp.data_ptr(), tcol.data_ptr(), n, Ep, H, F, txl.data_ptr(), txr.data_ptr(), tattn.data_ptr(), slope,
                                 None, pview2.data_ptr(), stream)
    assert st == 0, lib.tcgnn_last_error()
    if not torch.equal(pbuf, pbuf2):
        bad.append("%s: p differs with and without d_score (or on repetition)" % what)
    if not _untouched(pbuf, pview, E) or not _untouched(sbuf, sview, E):
        bad.append("%s: forward wrote positions no row covers, or guard words" % what)

    # backward by row, twice, and once with g aliasing dp
    dp = V.dp_for(H, E)
    dpbuf, dpview = _heads_buffer(dev, dp, H, E)
    need = lib.tcgnn_gatv2_workspace_bytes(n, Ep, H, F)
    scratch = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    sptr = scratch.data_ptr() + (-scratch.data_ptr()) % 256
    runs = []
    for gv in (None, None, dpview):
        gbuf, gview = (dpbuf, dpview) if gv is not None else _heads_buffer(dev, None, H, E)
        xrbuf, xrview = _node_buffer(dev, n, HF)
        abuf = torch.full((HF + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        st = lib.tcgnn_gatv2_softmax_backward(trp.data_ptr(), tcol.data_ptr(), n, Ep, H, F, txl.data_ptr(), txr.data_ptr(), tattn.data_ptr(), slope,
                                              pview.data_ptr(), dpview.data_ptr(), gview.data_ptr(), xrview.data_ptr(), abuf.data_ptr(), sptr, need, stream)
        assert st == 0, lib.tcgnn_last_error()
        runs.append((gbuf, gview, xrbuf, abuf))
    (gbuf, gview, xrbuf, abuf) = runs[0]
    if not all(torch.equal(a, b) for r in runs[1:] for a, b in zip((gbuf, xrbuf, abuf), (r[0], r[2], r[3]))):
        bad.append("%s: the second backward call, or the one whose g aliases dp, returns other bits" % what)
    if not _untouched(gbuf, gview, E) or not bool((xrbuf[n * HF:] == SENTINEL).all()) or not bool((abuf[HF:] == SENTINEL).all()):
        bad.append("%s: backward wrote positions no row covers, or guard words" % what)
    if E and lib.tcgnn_gatv2_softmax_backward(trp.data_ptr(), tcol.data_ptr(), n, Ep, H, F, txl.data_ptr(), txr.data_ptr(), tattn.data_ptr(), slope,
                                              pview.data_ptr(), dpview.data_ptr(), gview.data_ptr(), xrbuf.data_ptr(), abuf.data_ptr(), sptr, need - 1,
                                              stream) != 5:
        bad.append("%s: a scratch buffer one byte short is not TCGNN_ERR_WORKSPACE" % what)

    # backward by source, over the transposed CSR of tests/walks.py, twice
    rp_t, col_t, perm = _transposed(key, rp, col)
    pad = lambda a: np.concatenate([a, np.zeros(NO_ROW, np.int32)])   # noqa: E731
    trp_t, tcol_t, tperm = _dev(dev, rp_t), _dev(dev, pad(col_t)), _dev(dev, pad(perm))
    outs = []
    for _ in range(2):
        xlbuf, xlview = _node_buffer(dev, n, HF)
        st = lib.tcgnn_gatv2_source_grad(trp_t.data_ptr(), tcol_t.data_ptr(), tperm.data_ptr(), n, Ep, H, F, txl.data_ptr(), txr.data_ptr(),
                                         tattn.data_ptr(), slope, gview.data_ptr(), xlview.data_ptr(), stream)
        assert st == 0, lib.tcgnn_last_error()
        outs.append(xlbuf)
    if not torch.equal(outs[0], outs[1]):
        bad.append("%s: the second source-side call returns other bits" % what)
    if not bool((outs[0][n * HF:] == SENTINEL).all()):
        bad.append("%s: the source-side call wrote guard words" % what)
    torch.cuda.synchronize()

    out = dict(score=sview[:, :E].cpu().numpy(), p=pview[:, :E].cpu().numpy(), g=gview[:, :E].cpu().numpy(),
               d_xr=xrbuf[:n * HF].view(n, HF).cpu().numpy(), d_xl=outs[0][:n * HF].view(n, HF).cpu().numpy(), d_attn=abuf[:HF].view(H, F).cpu().numpy())
    z = V.z_f32(rp, col, xl, xl if xl_is_xr else xr)
    whole, excess = V.shares_of_all_bounds(rp, col, attn, dp, out, z=z, l=V.act_f32(z, slope), c=V.slope_factor_f32(z, attn, slope))
    print("FIG gatv2 %-40s H=%d F=%d slope=%.1f shares of the bounds: " % (what, H, F, slope) + ", ".join("%s %.3g" % kv for kv in whole.items())
          + "; beyond their own rounding: " + ", ".join("%s %.3g" % (k, excess[k]) for k in ("score", "d_xr", "d_xl", "d_attn")))
    for k, v in whole.items():
        if not v <= 1.0:
            bad.append("%s: %s needs %.3g of its bound" % (what, k, v))
    if not all(np.isfinite(a).all() for a in out.values()):
        bad.append("%s: non-finite results" % what)
    return bad, out


ROW_CASES = [(g, H, F, slope, name) for g in ("row_classes", "row_classes_T") for (H, F) in V.ROW_SHAPES for slope in V.SLOPES for name in V.SETS]


@pytest.mark.parametrize("graph,H,F,slope,name", ROW_CASES, ids=["%s-H%d-F%d-slope%.1f-%s" % c for c in ROW_CASES])
def test_gatv2_kernels_on_rows_of_every_length_class(dev, graph, H, F, slope, name):
    """row_classes: the forward and the row-side backward see every length class (0 .. 300 000, 16/17, 64/65, 1024/1025);
    row_classes_T, the same graph transposed: the source-side backward does (gatv2_ref.ATTN_SCALE says why attn is smaller there)"""
    rp, col = V.row_class_graphs()[graph]
    xl, xr, attn = V.x_sets(len(rp) - 1, H, F, attn_scale=V.ATTN_SCALE[graph])[name]
    bad, _ = _gatv2_case(dev, (graph,), rp, col, xl, xr, attn, slope, graph + " / " + name)
    assert not bad, "\n  ".join(bad)


@pytest.mark.parametrize("H,F", V.POWERLAW_SHAPES, ids=["H%d-F%d" % s for s in V.POWERLAW_SHAPES])
def test_gatv2_kernels_at_every_lane_layout(dev, H, F):
    """one lane a head, heads that fill no group, F % 4 != 0 (the dword form), the harness's output layer (1 x 41), the benchmark's
    shapes, F beyond 128 (a head per group, two passes) and H F = 300"""
    rp, col = V.powerlaw()
    xl, xr, attn = V.x_sets(len(rp) - 1, H, F)["normal_x8"]
    bad, _ = _gatv2_case(dev, ("powerlaw",), rp, col, xl, xr, attn, 0.2, "powerlaw 3000")
    assert not bad, "\n  ".join(bad)


def test_one_float_late_and_one_tensor_on_both_sides(dev, T):
    """views of xl, xr, attn and the outputs one float into a larger buffer (off 16 bytes: the dword form) give the bits of the
    aligned call; xl is xr works and equals two copies of it"""
    rp, col = V.powerlaw()
    n, E, (H, F) = len(rp) - 1, len(col), (4, 32)
    trp, tcol = _dev(dev, rp), _dev(dev, col)
    xl, xr, attn = V.x_sets(n, H, F)["normal_x8"]
    dp = _dev(dev, V.dp_for(H, E))

    def late(a):
        buf = torch.empty(a.size + 5, dtype=torch.float32, device=dev)
        view = buf[1:1 + a.size].view(a.shape)
        view.copy_(_dev(dev, a))
        assert view.data_ptr() % 16 == 4
        return view

    def run(txl, txr, tattn, shift):
        mk = (lambda *s: late(np.zeros(s, np.float32))) if shift else (lambda *s: torch.empty(*s, device=dev))
        p, s = T.gatv2_softmax(txl, txr, tattn, trp, tcol, 0.2, out=mk(H, E)), mk(H, E)
        assert torch.equal(T.gatv2_softmax(txl, txr, tattn, trp, tcol, 0.2, score_out=s), p)
        g, d_xr, d_attn = T.gatv2_softmax_backward(p, dp, txl, txr, tattn, trp, tcol, 0.2, out=mk(H, E))
        return p, s, g, d_xr, d_attn, T.gatv2_source_grad(g, txl, txr, tattn, trp, tcol, 0.2)
    aligned = run(_dev(dev, xl), _dev(dev, xr), _dev(dev, attn), False)
    shifted = run(late(xl), late(xr), late(attn), True)
    for name, a, b in zip(("p", "score", "g", "d_xr", "d_attn", "d_xl"), aligned, shifted):
        assert torch.equal(a, b), name
    txl = _dev(dev, xl)
    same, copy = run(txl, txl, _dev(dev, attn), False), run(txl, txl.clone(), _dev(dev, attn), False)
    for name, a, b in zip(("p", "score", "g", "d_xr", "d_attn", "d_xl"), same, copy):
        assert torch.equal(a, b), name
    bad, _ = _gatv2_case(dev, ("powerlaw",), rp, col, xl, None, attn, 0.2, "powerlaw 3000, xl is xr", xl_is_xr=True)
    assert not bad, "\n  ".join(bad)
    T.clear_plan_cache()


def test_gatv2_kernels_at_degenerate_sizes(dev, T):
    H, F = 3, 5
    # E = 1 (one self loop); N = 45, not a multiple of the workgroup's 32 rows
    for n, (rp, col) in ((1, (np.array([0, 1], np.int32), np.array([0], np.int32))), (45, graphs.uniform_graph(45, 4, seed=3, symmetric=False))):
        xl, xr, attn = V.x_sets(n, H, F)["normal_x1"]
        bad, out = _gatv2_case(dev, ("degenerate_n%d" % n,), rp, col, xl, xr, attn, 0.2, "N = %d" % n)
        assert not bad, "\n  ".join(bad)
        if n == 1:
            assert np.all(out["p"] == 1.0) and not out["g"].any() and not out["d_xr"].any() and not out["d_xl"].any() and not out["d_attn"].any()
    # a graph of empty rows only: nothing to normalise, every gradient zero - through the kernels' launchers (E = 0) ...
    n = 37
    rp0, col0 = torch.zeros(n + 1, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
    xl, attn = torch.randn(n, H * F, device=dev), torch.randn(H, F, device=dev)
    empty = torch.zeros(H, 0, device=dev)
    assert T.gatv2_softmax(xl, xl, attn, rp0, col0).shape == (H, 0)
    g, d_xr, d_attn = T.gatv2_softmax_backward(empty, empty, xl, xl, attn, rp0, col0)
    assert g.shape == (H, 0) and d_xr.shape == (n, H * F) and d_attn.shape == (H, F) and not bool(d_xr.any()) and not bool(d_attn.any())
    assert not bool(T.gatv2_source_grad(empty, xl, xl, attn, rp0, col0).any())
    # ... and through the kernels themselves: E > 0 positions exist but no row covers one
    z = np.zeros(n + 1, np.int32)
    xs = V.x_sets(n, H, F)["normal_x1"]
    bad, out = _gatv2_case(dev, ("empty_rows",), z, np.zeros(0, np.int32), *xs, 0.2, "empty rows only")
    assert not bad and not out["d_xr"].any() and not out["d_xl"].any() and not out["d_attn"].any(), bad
    T.clear_plan_cache()


def test_binding_gatv2_functions_equal_the_ctypes_module(dev, T, ext):
    rp, col = V.powerlaw()
    n, E, (H, F) = len(rp) - 1, len(col), (3, 8)
    trp, tcol = _dev(dev, rp), _dev(dev, col)
    xl, xr, attn = (_dev(dev, a) for a in V.x_sets(n, H, F)["normal_x8"])
    dp = _dev(dev, V.dp_for(H, E))
    want = T.gatv2_softmax(xl, xr, attn, trp, tcol, 0.3)
    s_w, s_e = torch.empty_like(want), torch.empty_like(want)
    assert torch.equal(ext.gatv2_softmax(xl, xr, attn, trp, tcol, 0.3), want)
    out = torch.empty_like(want)
    assert ext.gatv2_softmax(xl, xr, attn, trp, tcol, negative_slope=0.3, out=out, score_out=s_e).data_ptr() == out.data_ptr() and torch.equal(out, want)
    T.gatv2_softmax(xl, xr, attn, trp, tcol, 0.3, score_out=s_w)
    assert torch.equal(s_w, s_e)
    g_w, xr_w, a_w = T.gatv2_softmax_backward(want, dp, xl, xr, attn, trp, tcol, 0.3)
    g, d_xr, d_attn = ext.gatv2_softmax_backward(want, dp, xl, xr, attn, trp, tcol, 0.3)
    assert torch.equal(g, g_w) and torch.equal(d_xr, xr_w) and torch.equal(d_attn, a_w) and d_xr.shape == (n, H * F) and d_attn.shape == (H, F)
    alias = dp.clone()
    g2, _, _ = ext.gatv2_softmax_backward(want, alias, xl, xr, attn, trp, tcol, negative_slope=0.3, out=alias)
    assert g2.data_ptr() == alias.data_ptr() and torch.equal(alias, g_w)
    xl_w = T.gatv2_source_grad(g_w, xl, xr, attn, trp, tcol, 0.3)
    assert torch.equal(ext.gatv2_source_grad(g_w, xl, xr, attn, trp, tcol, 0.3), xl_w) and xl_w.shape == (n, H * F)
    for mod in (ext, T):
        with pytest.raises(RuntimeError, match="heads \\* features"):
            mod.gatv2_softmax(xl, xr[:, :-1].contiguous(), attn, trp, tcol)
        with pytest.raises(RuntimeError, match="out must be a contiguous fp32"):
            mod.gatv2_softmax(xl, xr, attn, trp, tcol, 0.2, torch.empty(H, E + 1, device=dev))
        with pytest.raises(RuntimeError, match="dp must be a contiguous fp32"):
            mod.gatv2_softmax_backward(want, dp[:, :-1].contiguous(), xl, xr, attn, trp, tcol)
        with pytest.raises(RuntimeError, match="g must be a contiguous fp32"):
            mod.gatv2_source_grad(g_w[:, :-1].contiguous(), xl, xr, attn, trp, tcol)
    torch.cuda.synchronize()
    ext.clear_plan_cache()
    T.clear_plan_cache()


# ---- the differentiable operator and the layer against the dense fp64 model ---------------------------------------------------------------

def _close(got, want, what, tol=G.GPU_LAYER_TOL):
    got, want = got.detach().double().cpu(), want.detach().double()
    err, top = float((got - want).abs().max()), float(want.abs().max())
    print("FIG %-44s %.3e of the largest entry" % (what, err / max(top, 1e-300)))
    assert got.shape == want.shape and err <= tol * top, "%s: %.3e of the largest entry" % (what, err / max(top, 1e-300))


@pytest.mark.parametrize("share_weights", [False, True], ids=["two_weights", "shared"])
@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
@pytest.mark.parametrize("name", ["layers_n200", "directed_n3000"])
def test_gatv2_operator_and_layer_against_dense_fp64(dev, T, name, concat, share_weights):
    """gat_ref.GPU_LAYER_TOL of the largest entry: the project's condition for chained operators; tests/test_gatv2_cpu.py shows that
    operand rounding alone stays inside half of it on these inputs"""
    import tcgnn_edge_ops as E
    import tcgnn_layers as L
    rp, col, X, Wl, Wr, attn, b, dY = V.gpu_layer_case(name, concat, share_weights)
    if name == "directed_n3000":
        assert not W.is_symmetric(rp, col)
    n, nnz, H, Fo = len(rp) - 1, len(col), V.LAYER_CASE["heads"], V.LAYER_CASE["out"]
    A = G.dense_adjacency(rp, col)
    meta = _meta(dev, rp, col)
    rows, cols = torch.from_numpy(np.repeat(np.arange(n), np.diff(rp))).long(), torch.from_numpy(col).long()
    f32 = lambda t: t.float().to(dev).requires_grad_(True)   # noqa: E731
    f64 = lambda t: t.clone().requires_grad_(True)           # noqa: E731

    if concat:     # the operator on its own: two operands, or one tensor on both sides
        g = torch.Generator().manual_seed(11)
        xl, xr, at, w = (torch.randn(*s, dtype=torch.float64, generator=g) for s in ((n, H * Fo), (n, H * Fo), (H, Fo), (H, nnz)))
        lg, rg, ag, ld, rd, ad = f32(xl), f32(xr), f32(at), f64(xl), f64(xr), f64(at)
        if share_weights:
            rg, rd = lg, ld
        P = E.gatv2_attention(lg, rg, ag, meta[0], meta[1], 0.2)
        want = V.dense_gatv2_attention(A, ld, rd, ad, 0.2)[:, rows, cols]
        _close(P, want, name + " gatv2_attention")
        leaves_g, leaves_d = ((lg, ag), (ld, ad)) if share_weights else ((lg, rg, ag), (ld, rd, ad))
        got = torch.autograd.grad((P * w.float().to(dev)).sum(), leaves_g)
        ref = torch.autograd.grad((want * w).sum(), leaves_d)
        for g_, r_, k in zip(got, ref, ("d_x (both sides)", "d_attn") if share_weights else ("d_xl", "d_xr", "d_attn")):
            _close(g_, r_, name + " gatv2_attention " + k)

    conv = L.GATv2Conv(X.shape[1], Fo, heads=H, concat=concat, share_weights=share_weights)
    for prm, val in ((conv.weights, Wl), (conv.weights_r, Wr), (conv.attn, attn), (conv.bias, b)):
        if prm is not None:
            prm.data.copy_(val.float())
    conv = conv.to(dev)
    Xg = f32(X)
    Y = conv(Xg, *meta)
    leaves = [f64(t) for t in (X, Wl, Wr, attn, b) if t is not None]
    Xd, Wld = leaves[0], leaves[1]
    Wrd = None if share_weights else leaves[2]
    want = V.dense_gatv2_model(A, Xd, Wld, Wrd, leaves[-2], leaves[-1], heads=H, concat=concat)
    what = "%s layer %s %s " % (name, "concat" if concat else "mean", "shared" if share_weights else "two weights")
    _close(Y, want, what + "Y")
    params = [p for p in (conv.weights, conv.weights_r, conv.attn, conv.bias) if p is not None]
    got = torch.autograd.grad((Y * dY.float().to(dev)).sum(), [Xg] + params)
    ref = torch.autograd.grad((want * dY).sum(), leaves)
    for g_, r_, k in zip(got, ref, ("dX", "dWl", "dattn", "dbias") if share_weights else ("dX", "dWl", "dWr", "dattn", "dbias")):
        _close(g_, r_, what + k)
    lonely = np.nonzero(np.diff(rp) == 0)[0]
    if len(lonely):
        assert torch.equal(Y[int(lonely[0])].detach(), conv.bias.detach())       # a node without incoming edges gets the bias only
    T.clear_plan_cache()


# ---- training --------------------------------------------------------------------------------------------------------------------------

def test_three_epochs_of_the_gatv2_model_with_two_heads_on_the_toy_dataset(dev, T, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tc-gnn_atc23_amd"))
    import tcgnn_graph as TG
    import tcgnn_harness as H
    f = np.load(os.path.join(ROOT, "tests", "golden", "dataset_toy.npz"))
    np.savez(os.path.join(tmp_path, "toy.npz"), src_li=f["src_li"], dst_li=f["dst_li"], num_nodes=f["num_nodes"])
    assert H.build_parser().parse_args(["--model", "gatv2", "--heads", "2"]).model == "gatv2"
    ds = TG.TCGNN_dataset(os.path.join(tmp_path, "toy.npz"), 12, 5, load_from_txt=False, seed=0)
    meta = _meta(dev, ds.row_pointers.numpy(), ds.column_index.numpy())
    out = H.time_training("gatv2", meta, ds.x.to(dev), ds.y.to(dev), 12, 16, 5, 2, epochs=3, seed=0, warmup=0, tune=False, heads=2)
    print("FIG gatv2 training on the toy dataset: loss after three epochs %.4f" % out["final_loss"])
    assert np.isfinite(out["final_loss"])
    T.clear_plan_cache()
