"""Gated aggregation on the MI355X: tcgnn_gated_sum / tcgnn_gated_source_grad through the C ABI on rows of every length class - by
destination and, on the transposed graph, by source - at every width class, one float off alignment and at degenerate sizes, the pybind
module against the ctypes one, operator and layer against the dense fp64 model, a captured step.  Bounds: tests/gated_ref.py."""
import glob
import importlib.util
import os

import numpy as np
import pytest
import torch

import gated_ref as R
import graphs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, SENTINEL, INVALID_ARG = 4096, -12345.0, 1   # sentinel words behind every output; TCGNN_ERR_INVALID_ARG
NAMES = ("Y", "S", "dq", "dv")
dev = torch.device("cuda:0")


@pytest.fixture(scope="module")
def T():
    import TCGNN
    return TCGNN


@pytest.fixture(scope="module")
def ext():
    spec = importlib.util.spec_from_file_location("TCGNN", glob.glob(os.path.join(ROOT, "integration", "TCGNN*.so"))[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _out(n, D):
    buf = torch.full((n * D + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[:n * D].view(n, D)


def _run(T, trp, tcol, k, q, v, dY, with_sens=True):   # both kernels through the C ABI -> ({name: [n, D] view}, {name: flat buffer})
    import tcgnn_capi as C
    (n, D), E, stream = k.shape, tcol.numel(), torch.cuda.current_stream().cuda_stream
    bufs, views = zip(*[_out(n, D) for _ in NAMES])
    bufs, views = dict(zip(NAMES, bufs)), dict(zip(NAMES, views))
    p = lambda t: t.data_ptr()   # noqa: E731
    assert C.lib.tcgnn_gated_sum(p(trp), p(tcol), n, E, p(k), p(q), p(v), D, p(views["Y"]), p(views["S"]) if with_sens else None, stream) == 0
    rp_t, col_t, perm, _ = T.transpose_graph(trp, tcol)
    assert C.lib.tcgnn_gated_source_grad(p(rp_t), p(col_t), p(perm), n, E, p(k), p(q), p(v), p(dY), D, p(views["dq"]), p(views["dv"]), stream) == 0
    return views, bufs


CASES = [(g, 64, s) for g in "AT" for s in R.SETS] + [(g, D, "normal_x1") for g in "AT" for D in R.WIDTHS if D != 64]


@pytest.mark.parametrize("graph,D,which", CASES, ids=["%s-D%d-%s" % c for c in CASES])
def test_both_kernels_on_rows_of_every_length_class(T, ext, graph, D, which):
    rp, col = R.row_class_graphs()[graph]
    k, q, v, dY = R.inputs(which, len(rp) - 1, D)
    ref = R.gated_f64(rp, col, k, q, v, dY)
    trp, tcol, tk, tdY = _dev(rp), _dev(col), _dev(k), _dev(dY)
    tq, tv = (tk, tk) if which == "aliased" else (_dev(q), _dev(v))
    views, bufs = _run(T, trp, tcol, tk, tq, tv, tdY)
    _, bufs2 = _run(T, trp, tcol, tk, tq, tv, tdY)
    plain, bufs3 = _run(T, trp, tcol, tk, tq, tv, tdY, with_sens=False)
    bad = []
    for name in NAMES:
        share = R.worst_share(views[name].cpu().numpy(), *ref[name])
        print("FIG gated %s D=%-3d %-13s %-2s worst share of its bound %.3f" % (graph, D, which, name, share))
        if not share <= 1.0 or not torch.equal(bufs[name], bufs2[name]) or not bool((bufs[name][views[name].numel():] == SENTINEL).all()):
            bad.append("%s: exceeds its bound (%.3f), differs on repetition, or sentinels were written" % (name, share))
    if not torch.equal(plain["Y"], views["Y"]) or not bool((bufs3["S"] == SENTINEL).all()):
        bad.append("Y without d_S differs, or S was written without being given")
    for mod in (T, ext):
        got = mod.forward_gated(tk, tq, tv, trp, tcol) + mod.source_grad_gated(tk, tq, tv, tdY, trp, tcol)
        Yn, none = mod.forward_gated(tk, tq, tv, trp, tcol, return_sens=False)
        if none is not None or not all(torch.equal(a, views[b]) for a, b in zip(got + (Yn,), NAMES + ("Y",))):
            bad.append("%s differs from the C call" % mod.__name__)
        mod.clear_plan_cache()
    assert not bad, bad


def test_operands_one_float_off_alignment_take_the_dword_form_and_give_the_same_bits(T):
    rp, col = R.row_class_graphs()["A"]
    aligned = [_dev(t) for t in R.inputs("normal_x1", len(rp) - 1, 64)]
    off = [torch.empty(t.numel() + 1, device=dev)[1:].view(t.shape).copy_(t) for t in aligned]
    assert all(t.data_ptr() % 16 == 0 for t in aligned) and all(t.data_ptr() % 16 == 4 for t in off)
    want, _ = _run(T, _dev(rp), _dev(col), *aligned)
    got, bufs = _run(T, _dev(rp), _dev(col), *off)
    assert all(torch.equal(got[name], want[name]) and bool((bufs[name][got[name].numel():] == SENTINEL).all()) for name in NAMES)
    T.clear_plan_cache()


def test_degenerate_sizes_return_ok_and_invalid_arguments_are_refused_before_anything_is_written():
    import tcgnn_capi as C
    stream = torch.cuda.current_stream().cuda_stream
    fwd, src = C.lib.tcgnn_gated_sum, C.lib.tcgnn_gated_source_grad
    n, E, D = 10, 30, 5
    rp, col = torch.arange(0, E + 1, 3, dtype=torch.int32, device=dev), torch.zeros(E, dtype=torch.int32, device=dev)
    keep = torch.randn(n, D, device=dev)   # (alive while its address is in use)
    X = keep.data_ptr()
    outs = [_out(n, D) for _ in NAMES]
    y, s, dq, dv = (view.data_ptr() for _, view in outs)
    assert fwd(None, None, n, 0, X, X, X, D, y, s, stream) == 0 and src(None, None, None, n, 0, X, X, X, X, D, dq, dv, stream) == 0   # E = 0
    for buf, view in outs:
        assert bool((view.view(torch.int32) == 0).all()) and bool((buf[n * D:] == SENTINEL).all())
        buf.fill_(SENTINEL)
    rp, col = rp.data_ptr(), col.data_ptr()
    for nn, ee, dd in ((0, 0, D), (0, 5, D), (n, E, 0)):   # N = 0, D = 0: nothing to write
        assert fwd(rp, col, nn, ee, X, X, X, dd, y, s, stream) == 0 and src(rp, col, col, nn, ee, X, X, X, X, dd, dq, dv, stream) == 0
    for call, good, at in ((fwd, [rp, col, n, E, X, X, X, D, y, s], ((2, -1), (3, -1), (3, 1 << 31), (7, -1), (0, None), (1, None), (4, None), (5, None), (6, None), (8, None))),
                           (src, [rp, col, col, n, E, X, X, X, X, D, dq, dv], ((3, -1), (4, -1), (4, 1 << 31), (9, -1), (0, None), (1, None), (5, None), (6, None), (7, None), (8, None), (10, None), (11, None)))):
        for i, value in at:
            assert call(*(good[:i] + [value] + good[i + 1:]), stream) == INVALID_ARG, (i, value)
    assert all(bool((buf == SENTINEL).all()) for buf, _ in outs)


def _held(what, got, want):   # everything on the path is fp32: DESIGN.md 4.12's bounds - 1e-5 of the largest entry for outputs, 1e-4 for gradients
    for i, (g, w) in enumerate(zip(got, want)):
        rel = float((g.detach().double().cpu() - w.detach()).abs().max()) / float(w.detach().abs().max())
        print("FIG gated %s %d: %.3e of the largest entry" % (what, i, rel))
        assert g.shape == w.shape and rel <= (1e-5 if i == 0 else 1e-4), (what, i, rel)


@pytest.mark.parametrize("where", ["operator", "layer", "layer_on_a_block"])
def test_operator_and_layer_against_the_dense_fp64_model_on_a_directed_graph(T, where):
    import tcgnn_edge_ops as E
    import tcgnn_layers as L
    rp, col = graphs.uniform_graph(500, 6, seed=13, symmetric=False)
    meta = [_dev(rp), _dev(col)] + [torch.empty(0, dtype=torch.int32, device=dev)] * 3
    if where == "layer_on_a_block":
        meta = L.sample_batch_rows(meta, torch.arange(0, 500, 7, device=dev), [4, 4], 11, plan=False).metas[0]
        rp, col = meta[0].cpu().numpy(), meta[1].cpu().numpy()
    n = len(rp) - 1
    torch.manual_seed(3)
    if where == "operator":
        leaves, dY = [torch.randn(n, 41) for _ in range(3)], torch.randn(n, 41, dtype=torch.float64)
        fn = lambda k, q, v: E.aggregate_gated(k, q, v, *meta[:2])   # noqa: E731
        hi = lambda k, q, v: R.dense_f64(rp, col, k, q, v)   # noqa: E731
    else:
        conv = L.ResGatedGraphConv(24, 16)
        conv.bias.data.normal_()
        leaves, dY = [torch.randn(n, 24), conv.weights.data, conv.weights_skip.data, conv.bias.data], torch.randn(n, 16, dtype=torch.float64)
        fn = lambda X, W, Ws, b: torch.func.functional_call(conv, {"weights": W, "weights_skip": Ws, "bias": b}, (X, *meta))   # noqa: E731
        hi = lambda X, W, Ws, b: R.dense_f64(rp, col, *(X @ W).split(16, dim=1)) + X @ Ws + b   # noqa: E731
    lo64, on_dev = [t.double().requires_grad_(True) for t in leaves], [t.to(dev).requires_grad_(True) for t in leaves]
    Y, want = fn(*on_dev), hi(*lo64)
    _held(where, (Y,) + torch.autograd.grad((Y * dY.float().to(dev)).sum(), on_dev), (want,) + torch.autograd.grad((want * dY).sum(), lo64))
    T.clear_plan_cache()


def test_a_prepared_step_replays_from_a_hip_graph_bit_equal_and_free_memory_stays_flat(T):
    import tcgnn_layers as L
    rp, col = graphs.community_graph(3000, 10, 20, 0.8, seed=4)
    meta = [_dev(a) for a in (rp, col) + tuple(graphs.host_sgt(rp, col)[:3])]
    torch.manual_seed(2)
    convs = [L.ResGatedGraphConv(32, 16).to(dev), L.ResGatedGraphConv(16, 6).to(dev)]
    x, y = torch.randn(len(rp) - 1, 32, device=dev).requires_grad_(True), torch.randint(0, 6, (len(rp) - 1,), device=dev)
    T.prepare([], *meta, gated=True)

    def step():
        out = convs[1](torch.relu(convs[0](x, *meta)), *meta)
        return torch.autograd.grad(torch.nn.functional.cross_entropy(out, y), [x] + [p for cv in convs for p in cv.parameters()])

    eager = [g.clone() for g in step()]
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                # allocator warm-up on the side stream, as capture requires
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):   # one stream, no parallel branches
        static = step()
    for _ in range(3):                           # several replays, each against the eager result
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(static, eager))
    T.clear_plan_cache()
