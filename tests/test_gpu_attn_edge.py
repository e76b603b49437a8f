"""Fused sparse attention with edge features on the MI355X: tcgnn_attn_edge_forward / _backward / _source_grad through the C ABI on rows of
every length class - by destination and on the transposed graph - at every head layout, with ee = 0 against the calls without edges, one
float off alignment and at degenerate sizes, the pybind module against the ctypes one, operator and layer (edge_dim, beta) against the
dense fp64 model.  Bounds: tests/attn_edge_ref.py."""
import numpy as np
import pytest
import torch

import attn_edge_ref as R
import graphs
from test_gpu_fused_attention import GUARD, INVALID_ARG, SENTINEL, T, _dev, _held, _out, dev, ext  # noqa: F401  (its fixtures, guarded buffers and bars)

pytestmark = pytest.mark.gpu


def _outs(n, E, H, F):
    bufs, views = zip(*[_out(E if name in ("dee", "pg") else n, R.width(name, H, F)) for name in R.NAMES])
    return dict(zip(R.NAMES, bufs)), dict(zip(R.NAMES, views))


def _run(T, trp, tcol, q, k, v, dY, ee, given, H, scale):
    """the three calls through the C ABI, the row side on `given`'s Y and L, the source side on its pg -> ({name: view}, {name: flat buffer})"""
    import tcgnn_capi as C
    (n, D), E, stream = q.shape, tcol.numel(), torch.cuda.current_stream().cuda_stream
    bufs, o = _outs(n, E, H, D // H)
    p, (Y, L, pg) = (lambda t: t.data_ptr()), given
    assert C.lib.tcgnn_attn_edge_forward(p(trp), p(tcol), n, E, p(q), p(k), p(v), p(ee), H, D // H, scale, p(o["Y"]), p(o["L"]), stream) == 0
    assert C.lib.tcgnn_attn_edge_backward(p(trp), p(tcol), n, E, p(q), p(k), p(v), p(ee), p(Y), p(dY), p(L), H, D // H, scale, p(o["dq"]), p(o["delta"]),
                                          p(o["dee"]), p(o["pg"]), stream) == 0
    rp_t, col_t, perm, _ = T.transpose_graph(trp, tcol)
    assert C.lib.tcgnn_attn_edge_source_grad(p(rp_t), p(col_t), p(perm), n, E, p(q), p(dY), p(pg), H, D // H, scale, p(o["dk"]), p(o["dv"]), stream) == 0
    return o, bufs


CASES = [(g, H, F, "normal_x1") for g in "AT" for H, F in R.SHAPES] + [(g, 8, 8, s) for g in "AT" for s in R.SETS[1:]]


@pytest.mark.parametrize("graph,H,F,which", CASES, ids=["%s-%dx%d-%s" % c for c in CASES])
def test_the_three_calls_on_rows_of_every_length_class(T, ext, graph, H, F, which):
    rp, col = R.row_class_graphs()[graph]
    if which == "increasing":
        rp, col = R.sorted_rows(rp, col)
    host = R.inputs(which, rp, col, H, F)
    scale = float(np.float32(F ** -0.5))
    ref = R.attn_edge_f64(rp, col, *host, H, scale)
    trp, tcol = _dev(rp), _dev(col)
    tq, tk, tv, tdY, tee = (_dev(t) for t in host)
    Y, L, _, pg = (_dev(t) for t in ref["given"])
    args = (T, trp, tcol, tq, tk, tv, tdY, tee, (Y, L, pg), H, scale)
    views, bufs = _run(*args)
    _, bufs2 = _run(*args)
    bad = []
    for name in R.NAMES:
        share = R.worst_share(views[name].cpu().numpy(), *ref[name])
        print("FIG attn_edge %s %dx%-3d %-10s %-5s worst share of its bound %.3f" % (graph, H, F, which, name, share))
        if not share <= 1.0 or not torch.equal(bufs[name], bufs2[name]) or not bool((bufs[name][views[name].numel():] == SENTINEL).all()):
            bad.append("%s: exceeds its bound (%.3f), differs on repetition, or sentinels were written" % (name, share))
    for mod in (T, ext):
        got = dict(zip(("Y", "L"), mod.forward_attn_edge(tq, tk, tv, tee, H, trp, tcol)))
        got.update(zip(("dq", "delta", "dee", "pg"), mod.backward_attn_edge(tq, tk, tv, tee, Y, tdY, L, H, trp, tcol)))
        got.update(zip(("dk", "dv"), mod.source_grad_attn_edge(tq, tdY, pg, H, trp, tcol)))
        lean = mod.backward_attn_edge(tq, tk, tv, tee, Y, tdY, L, H, trp, tcol, need_dq=False, need_dee=False, need_pg=False)
        if not all(torch.equal(got[name].view_as(views[name]), views[name]) for name in R.NAMES) or lean[0] is not None or lean[2] is not None \
                or lean[3] is not None or not torch.equal(lean[1], views["delta"]):
            bad.append("%s differs from the C call" % mod.__name__)
        mod.clear_plan_cache()
    assert not bad, bad


@pytest.mark.parametrize("H,F", [(8, 8), (4, 32), (1, 260)])
def test_a_zero_edge_vector_gives_the_bits_of_the_calls_without_edges(T, H, F):
    rp, col = R.row_class_graphs()["A"]
    q, k, v, dY, ee = (_dev(t) for t in R.inputs("normal_x1", rp, col, H, F))
    trp, tcol = _dev(rp), _dev(col)
    ee.zero_()
    Y, L = T.forward_attn(q, k, v, H, trp, tcol)
    dq, delta = T.backward_attn(q, k, v, Y, dY, L, H, trp, tcol)
    Ye, Le = T.forward_attn_edge(q, k, v, ee, H, trp, tcol)
    dqe, deltae, _, _ = T.backward_attn_edge(q, k, v, ee, Y, dY, L, H, trp, tcol)
    assert all(torch.equal(a, b) for a, b in ((Y, Ye), (L, Le), (dq, dqe), (delta, deltae)))
    T.clear_plan_cache()


def test_operands_one_float_off_alignment_take_the_dword_form_and_give_the_same_bits(T):
    rp, col = R.row_class_graphs()["A"]
    H, F = 4, 32
    host = R.inputs("normal_x1", rp, col, H, F)
    Y, L, _, pg = R.attn_edge_f64(rp, col, *host, H, 0.25)["given"]
    aligned = [_dev(t) for t in host + (Y,)]
    off = [torch.empty(t.numel() + 1, device=dev)[1:].view(t.shape).copy_(t) for t in aligned]
    assert all(t.data_ptr() % 16 == 0 for t in aligned) and all(t.data_ptr() % 16 == 4 for t in off)
    L, pg = _dev(L), _dev(pg)
    want, _ = _run(T, _dev(rp), _dev(col), *aligned[:5], (aligned[5], L, pg), H, 0.25)
    got, bufs = _run(T, _dev(rp), _dev(col), *off[:5], (off[5], L, pg), H, 0.25)
    assert all(torch.equal(got[name], want[name]) and bool((bufs[name][got[name].numel():] == SENTINEL).all()) for name in R.NAMES)
    T.clear_plan_cache()


def test_degenerate_sizes_return_ok_and_invalid_arguments_are_refused_before_anything_is_written():
    import tcgnn_capi as C
    stream = torch.cuda.current_stream().cuda_stream
    fwd, bwd, src = C.lib.tcgnn_attn_edge_forward, C.lib.tcgnn_attn_edge_backward, C.lib.tcgnn_attn_edge_source_grad
    n, E, H, F = 10, 30, 3, 5
    rp, col = torch.arange(0, E + 1, 3, dtype=torch.int32, device=dev), torch.zeros(E, dtype=torch.int32, device=dev)
    keep = torch.randn(max(n, E), 2 * H * F, device=dev)   # (alive while its address is in use)
    X = keep.data_ptr()
    bufs, views = _outs(n, E, H, F)
    y, l, delta, dq, dee, pg, dk, dv = (views[name].data_ptr() for name in R.NAMES)
    node = ("Y", "L", "delta", "dq", "dk", "dv")
    assert fwd(None, None, n, 0, X, X, X, X, H, F, 1.0, y, l, stream) == 0 \
        and bwd(None, None, n, 0, X, X, X, X, X, X, X, H, F, 1.0, dq, delta, dee, pg, stream) == 0 \
        and src(None, None, None, n, 0, X, X, X, H, F, 1.0, dk, dv, stream) == 0   # E = 0: the node outputs are zeroed, the edge outputs have no elements
    for name in R.NAMES:
        inside = views[name].view(torch.int32) == 0 if name in node else views[name] == SENTINEL
        assert bool(inside.all()) and bool((bufs[name][views[name].numel():] == SENTINEL).all()), name
        bufs[name].fill_(SENTINEL)
    rp, col = rp.data_ptr(), col.data_ptr()
    assert fwd(rp, col, n, E, X, X, X, X, H, 0, 1.0, y, l, stream) == 0 and bwd(rp, col, n, E, X, X, X, X, X, X, X, H, 0, 1.0, dq, delta, dee, pg, stream) == 0 \
        and src(rp, col, col, n, E, X, X, X, H, 0, 1.0, dk, dv, stream) == 0   # F = 0: only L and delta exist
    for name in R.NAMES:
        inside = views[name].view(torch.int32) == 0 if name in ("L", "delta") else views[name] == SENTINEL
        assert bool(inside.all()) and bool((bufs[name][views[name].numel():] == SENTINEL).all()), name
        bufs[name].fill_(SENTINEL)
    for nn, ee, hh in ((0, 0, H), (0, 5, H), (n, E, 0)):   # N = 0, H = 0: nothing to write
        assert fwd(rp, col, nn, ee, X, X, X, X, hh, F, 1.0, y, l, stream) == 0 \
            and bwd(rp, col, nn, ee, X, X, X, X, X, X, X, hh, F, 1.0, dq, delta, dee, pg, stream) == 0 \
            and src(rp, col, col, nn, ee, X, X, X, hh, F, 1.0, dk, dv, stream) == 0
    nulls = lambda *at: tuple((i, None) for i in at)   # noqa: E731
    # negative sizes, E >= 2^31, H F >= 2^31, more than 65535 column passes (H = 2^21 at F = 5: 2^16 lane groups of 32 heads), null required arrays
    for call, good, at in ((fwd, [rp, col, n, E, X, X, X, X, H, F, 1.0, y, l], ((2, -1), (3, -1), (3, 1 << 31), (8, -1), (9, -1), (8, 1 << 30), (8, 1 << 21)) + nulls(0, 1, 4, 5, 6, 7, 11)),
                           (bwd, [rp, col, n, E, X, X, X, X, X, X, X, H, F, 1.0, dq, delta, dee, pg], ((2, -1), (3, -1), (3, 1 << 31), (11, -1), (12, -1), (11, 1 << 21)) + nulls(0, 1, 4, 5, 6, 7, 8, 9, 10, 15)),
                           (src, [rp, col, col, n, E, X, X, X, H, F, 1.0, dk, dv], ((3, -1), (4, -1), (4, 1 << 31), (8, -1), (9, -1), (8, 1 << 21)) + nulls(0, 1, 2, 5, 6, 7, 11, 12))):
        for i, value in at:
            assert call(*(good[:i] + [value] + good[i + 1:]), stream) == INVALID_ARG, (call.__name__, i, value)
    assert all(bool((buf == SENTINEL).all()) for buf in bufs.values())


@pytest.mark.parametrize("where", ["operator", "layer_concat", "layer_mean", "layer_beta"])
def test_operator_and_layer_with_edge_features_against_the_dense_fp64_model_on_a_directed_graph(T, where):
    import tcgnn_edge_ops as E
    import tcgnn_layers as L
    rp, col = graphs.uniform_graph(500, 6, seed=13, symmetric=False)
    meta = [_dev(a) for a in (rp, col) + tuple(graphs.host_sgt(rp, col)[:3])]
    n, ne, H, F = len(rp) - 1, len(col), 3, 8
    torch.manual_seed(3)
    if where == "operator":
        leaves, dY = [torch.randn(n, H * 7) for _ in range(3)] + [torch.randn(ne, H * 7)], torch.randn(n, H * 7, dtype=torch.float64)
        fn = lambda q, k, v, ee: E.aggregate_attention(q, k, v, H, *meta[:2], edge=ee)   # noqa: E731
        hi = lambda q, k, v, ee: R.dense_f64(rp, col, q, k, v, ee, H)   # noqa: E731
    else:
        concat = where != "layer_mean"
        conv = L.TransformerConv(24, F, heads=H, concat=concat, fused=True, edge_dim=5, beta=where == "layer_beta")
        for b in (conv.bias_q, conv.bias_k, conv.bias_v, conv.bias):
            b.data.normal_()
        # (a softmax does not see a constant added to every score of a row: the gradient of bias_k is 0 and has no largest entry to measure by)
        names, bk = [name for name, _ in conv.named_parameters() if name != "bias_k"], conv.bias_k.data
        leaves = [torch.randn(n, 24), torch.randn(ne, 5)] + [conv.get_parameter(name).data for name in names]
        dY = torch.randn(n, H * F if concat else F, dtype=torch.float64)
        fn = lambda X, ea, *ps: torch.func.functional_call(conv, dict(zip(names, ps), bias_k=bk.to(dev)), (X, *meta), {"edge_attr": ea})   # noqa: E731
        hi = lambda X, ea, *ps: R.layer_f64(rp, col, X, ea, dict(zip(names, ps), bias_k=bk.double()), H, F, concat)   # noqa: E731
    lo64, on_dev = [t.double().requires_grad_(True) for t in leaves], [t.to(dev).requires_grad_(True) for t in leaves]
    Y, want = fn(*on_dev), hi(*lo64)
    _held("edge_" + where, (Y,) + torch.autograd.grad((Y * dY.float().to(dev)).sum(), on_dev), (want,) + torch.autograd.grad((want * dY).sum(), lo64))
    T.clear_plan_cache()
