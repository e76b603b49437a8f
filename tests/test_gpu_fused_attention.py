"""Fused sparse attention on the MI355X: tcgnn_attn_forward / _backward / _source_grad through the C ABI on rows of every length class -
by destination and on the transposed graph - at every head layout, one float off alignment and at degenerate sizes, the pybind module
against the ctypes one, operator and layer against the dense fp64 model, a captured step.  Bounds: tests/attn_ref.py."""
import gc
import glob
import importlib.util
import os

import numpy as np
import pytest
import torch

import attn_ref as R
import graphs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, SENTINEL, INVALID_ARG = 4096, -12345.0, 1   # sentinel words behind every output; TCGNN_ERR_INVALID_ARG
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


def _run(T, trp, tcol, q, k, v, dY, given, H, scale, with_lse=True):
    """the three calls through the C ABI, the backward ones on `given` = (Y, L, delta) -> ({name: view}, {name: flat buffer})"""
    import tcgnn_capi as C
    (n, D), E, stream = q.shape, tcol.numel(), torch.cuda.current_stream().cuda_stream
    bufs, views = zip(*[_out(n, H if name in ("L", "delta") else D) for name in R.NAMES])
    bufs, views = dict(zip(R.NAMES, bufs)), dict(zip(R.NAMES, views))
    p, (Y, L, delta) = (lambda t: t.data_ptr()), given
    assert C.lib.tcgnn_attn_forward(p(trp), p(tcol), n, E, p(q), p(k), p(v), H, D // H, scale, p(views["Y"]), p(views["L"]) if with_lse else None, stream) == 0
    assert C.lib.tcgnn_attn_backward(p(trp), p(tcol), n, E, p(q), p(k), p(v), p(Y), p(dY), p(L), H, D // H, scale, p(views["dq"]), p(views["delta"]), stream) == 0
    rp_t, col_t, perm, _ = T.transpose_graph(trp, tcol)
    assert C.lib.tcgnn_attn_source_grad(p(rp_t), p(col_t), p(perm), n, E, p(q), p(k), p(v), p(dY), p(L), p(delta), H, D // H, scale, p(views["dk"]),
                                        p(views["dv"]), stream) == 0
    return views, bufs


CASES = [(g, 8, 8, s) for g in "AT" for s in R.SETS] + [(g, H, F, "normal_x1") for g in "AT" for H, F in R.SHAPES if (H, F) != (8, 8)]


@pytest.mark.parametrize("graph,H,F,which", CASES, ids=["%s-%dx%d-%s" % c for c in CASES])
def test_the_three_calls_on_rows_of_every_length_class(T, ext, graph, H, F, which):
    rp, col = R.row_class_graphs()[graph]
    if which in ("increasing", "decreasing"):
        rp, col = R.sorted_rows(rp, col)
    q, k, v, dY = R.inputs(which, len(rp) - 1, H, F)
    scale = float(np.float32(F ** -0.5))
    ref = R.attn_f64(rp, col, q, k, v, dY, H, scale)
    trp, tcol, tq, tdY = _dev(rp), _dev(col), _dev(q), _dev(dY)
    tk, tv = (tq, tq) if which == "aliased" else (_dev(k), _dev(v))
    given = [_dev(t) for t in ref["given"]]
    args = (T, trp, tcol, tq, tk, tv, tdY, given, H, scale)
    views, bufs = _run(*args)
    _, bufs2 = _run(*args)
    plain, bufs3 = _run(*args, with_lse=False)
    bad = []
    for name in R.NAMES:
        share = R.worst_share(views[name].cpu().numpy(), *ref[name])
        print("FIG attn %s %dx%-3d %-10s %-5s worst share of its bound %.3f" % (graph, H, F, which, name, share))
        if not share <= 1.0 or not torch.equal(bufs[name], bufs2[name]) or not bool((bufs[name][views[name].numel():] == SENTINEL).all()):
            bad.append("%s: exceeds its bound (%.3f), differs on repetition, or sentinels were written" % (name, share))
    if not torch.equal(plain["Y"], views["Y"]) or not bool((bufs3["L"] == SENTINEL).all()):
        bad.append("Y without d_L differs, or L was written without being given")
    Y, L, delta = given
    for mod in (T, ext):
        got = dict(zip(("Y", "L"), mod.forward_attn(tq, tk, tv, H, trp, tcol)))
        got.update(zip(("dq", "delta"), mod.backward_attn(tq, tk, tv, Y, tdY, L, H, trp, tcol)))
        got.update(zip(("dk", "dv"), mod.source_grad_attn(tq, tk, tv, tdY, L, delta, H, trp, tcol)))
        Yn, none = mod.forward_attn(tq, tk, tv, H, trp, tcol, return_lse=False)
        no_dq, d2 = mod.backward_attn(tq, tk, tv, Y, tdY, L, H, trp, tcol, need_dq=False)
        if none is not None or no_dq is not None or not all(torch.equal(got[name], views[name]) for name in R.NAMES) \
                or not torch.equal(Yn, views["Y"]) or not torch.equal(d2, views["delta"]):
            bad.append("%s differs from the C call" % mod.__name__)
        mod.clear_plan_cache()
    assert not bad, bad


def test_operands_one_float_off_alignment_take_the_dword_form_and_give_the_same_bits(T):
    rp, col = R.row_class_graphs()["A"]
    H, F = 4, 32
    host = R.inputs("normal_x1", len(rp) - 1, H, F)
    given = R.attn_f64(rp, col, *host, H, 0.25)["given"]
    aligned = [_dev(t) for t in host + (given[0],)]
    off = [torch.empty(t.numel() + 1, device=dev)[1:].view(t.shape).copy_(t) for t in aligned]
    assert all(t.data_ptr() % 16 == 0 for t in aligned) and all(t.data_ptr() % 16 == 4 for t in off)
    rest = [_dev(t) for t in given[1:]]
    want, _ = _run(T, _dev(rp), _dev(col), *aligned[:4], [aligned[4]] + rest, H, 0.25)
    got, bufs = _run(T, _dev(rp), _dev(col), *off[:4], [off[4]] + rest, H, 0.25)
    assert all(torch.equal(got[name], want[name]) and bool((bufs[name][got[name].numel():] == SENTINEL).all()) for name in R.NAMES)
    T.clear_plan_cache()


def test_degenerate_sizes_return_ok_and_invalid_arguments_are_refused_before_anything_is_written():
    import tcgnn_capi as C
    stream = torch.cuda.current_stream().cuda_stream
    fwd, bwd, src = C.lib.tcgnn_attn_forward, C.lib.tcgnn_attn_backward, C.lib.tcgnn_attn_source_grad
    n, E, H, F = 10, 30, 3, 5
    rp, col = torch.arange(0, E + 1, 3, dtype=torch.int32, device=dev), torch.zeros(E, dtype=torch.int32, device=dev)
    keep = torch.randn(n, H * F, device=dev)   # (alive while its address is in use)
    X = keep.data_ptr()
    outs = dict(zip(R.NAMES, [_out(n, H if name in ("L", "delta") else H * F) for name in R.NAMES]))
    y, l, delta, dq, dk, dv = (outs[name][1].data_ptr() for name in R.NAMES)
    assert fwd(None, None, n, 0, X, X, X, H, F, 1.0, y, l, stream) == 0 and bwd(None, None, n, 0, X, X, X, X, X, X, H, F, 1.0, dq, delta, stream) == 0 \
        and src(None, None, None, n, 0, X, X, X, X, X, X, H, F, 1.0, dk, dv, stream) == 0   # E = 0
    for buf, view in outs.values():
        assert bool((view.view(torch.int32) == 0).all()) and bool((buf[view.numel():] == SENTINEL).all())
        buf.fill_(SENTINEL)
    rp, col = rp.data_ptr(), col.data_ptr()
    assert fwd(rp, col, n, E, X, X, X, H, 0, 1.0, y, l, stream) == 0 and bwd(rp, col, n, E, X, X, X, X, X, X, H, 0, 1.0, dq, delta, stream) == 0 \
        and src(rp, col, col, n, E, X, X, X, X, X, X, H, 0, 1.0, dk, dv, stream) == 0   # F = 0: only L and delta exist
    for name, (buf, view) in outs.items():
        assert bool((buf[view.numel():] == SENTINEL).all()) and bool((view.view(torch.int32) == 0).all() if name in ("L", "delta") else (view == SENTINEL).all())
        buf.fill_(SENTINEL)
    for nn, ee, hh in ((0, 0, H), (0, 5, H), (n, E, 0)):   # N = 0, H = 0: nothing to write
        assert fwd(rp, col, nn, ee, X, X, X, hh, F, 1.0, y, l, stream) == 0 and bwd(rp, col, nn, ee, X, X, X, X, X, X, hh, F, 1.0, dq, delta, stream) == 0 \
            and src(rp, col, col, nn, ee, X, X, X, X, X, X, hh, F, 1.0, dk, dv, stream) == 0
    nulls = lambda *at: tuple((i, None) for i in at)   # noqa: E731
    for call, good, at in ((fwd, [rp, col, n, E, X, X, X, H, F, 1.0, y, l], ((2, -1), (3, -1), (3, 1 << 31), (7, -1), (8, -1), (7, 1 << 30)) + nulls(0, 1, 4, 5, 6, 10)),
                           (bwd, [rp, col, n, E, X, X, X, X, X, X, H, F, 1.0, dq, delta], ((2, -1), (3, -1), (3, 1 << 31), (10, -1), (11, -1)) + nulls(0, 1, 4, 5, 6, 7, 8, 9, 14)),
                           (src, [rp, col, col, n, E, X, X, X, X, X, X, H, F, 1.0, dk, dv], ((3, -1), (4, -1), (4, 1 << 31), (11, -1), (12, -1)) + nulls(0, 1, 5, 6, 7, 8, 9, 10, 14, 15))):
        for i, value in at:
            assert call(*(good[:i] + [value] + good[i + 1:]), stream) == INVALID_ARG, (call.__name__, i, value)
    assert all(bool((buf == SENTINEL).all()) for buf, _ in outs.values())


def _held(what, got, want):   # everything on the path is fp32: DESIGN.md 4.12's bounds - 1e-5 of the largest entry for outputs, 1e-4 for gradients
    for i, (g, w) in enumerate(zip(got, want)):
        rel = float((g.detach().double().cpu() - w.detach()).abs().max()) / float(w.detach().abs().max())
        print("FIG attn %s %d: %.3e of the largest entry" % (what, i, rel))
        assert g.shape == w.shape and rel <= (1e-5 if i == 0 else 1e-4), (what, i, rel)


@pytest.mark.parametrize("where", ["operator", "layer_concat", "layer_mean", "layer_on_a_block"])
def test_operator_and_fused_layer_against_the_dense_fp64_model_on_a_directed_graph(T, where):
    import tcgnn_edge_ops as E
    import tcgnn_layers as L
    rp, col = graphs.uniform_graph(500, 6, seed=13, symmetric=False)
    meta = [_dev(a) for a in (rp, col) + tuple(graphs.host_sgt(rp, col)[:3])]
    if where == "layer_on_a_block":
        meta = L.sample_batch_rows(meta, torch.arange(0, 500, 7, device=dev), [4, 4], 11, plan=False).metas[0]
        rp, col = meta[0].cpu().numpy(), meta[1].cpu().numpy()
    n, H, F = len(rp) - 1, 3, 8
    torch.manual_seed(3)
    if where == "operator":
        leaves, dY = [torch.randn(n, H * 7) for _ in range(3)], torch.randn(n, H * 7, dtype=torch.float64)
        fn = lambda q, k, v: E.aggregate_attention(q, k, v, H, *meta[:2])   # noqa: E731
        hi = lambda q, k, v: R.dense_f64(rp, col, q, k, v, H)   # noqa: E731
    else:
        concat = where != "layer_mean"
        conv = L.TransformerConv(24, F, heads=H, concat=concat, fused=True)
        for b in (conv.bias_q, conv.bias_k, conv.bias_v, conv.bias):
            b.data.normal_()
        # (a softmax does not see a constant added to every score of a row: the gradient of bias_k is 0 and has no largest entry to measure by)
        names, bk = [name for name, _ in conv.named_parameters() if name != "bias_k"], conv.bias_k.data
        leaves, dY = [torch.randn(n, 24)] + [conv.get_parameter(name).data for name in names], torch.randn(n, H * F if concat else F, dtype=torch.float64)
        fn = lambda X, *ps: torch.func.functional_call(conv, dict(zip(names, ps), bias_k=bk.to(dev)), (X, *meta))   # noqa: E731

        def hi(X, *ps):
            w = dict(zip(names, ps), bias_k=bk.double())
            Y = R.dense_f64(rp, col, *(X @ w["weights_" + c] + w["bias_" + c] for c in "qkv"), H)
            return (Y if concat else Y.view(n, H, F).mean(1)) + X @ w["weights_root"] + w["bias"]
    lo64, on_dev = [t.double().requires_grad_(True) for t in leaves], [t.to(dev).requires_grad_(True) for t in leaves]
    Y, want = fn(*on_dev), hi(*lo64)
    _held(where, (Y,) + torch.autograd.grad((Y * dY.float().to(dev)).sum(), on_dev), (want,) + torch.autograd.grad((want * dY).sum(), lo64))
    if where == "layer_concat":   # the composition of the same layer: within its own fp16-image bound (2^-9 of the scale) of the fused path
        conv = conv.to(dev)
        with torch.no_grad():
            fused = conv(leaves[0].to(dev), *meta)
            conv.fused = False
            composed = conv(leaves[0].to(dev), *meta)
        assert float((fused - composed).abs().max()) <= 2.0 ** -9 * float(composed.abs().max())
    T.clear_plan_cache()


def test_a_prepared_fused_step_replays_from_a_hip_graph_bit_equal_and_free_memory_stays_flat(T):
    import tcgnn_layers as L
    rp, col = graphs.community_graph(3000, 10, 20, 0.8, seed=4)
    meta = [_dev(a) for a in (rp, col) + tuple(graphs.host_sgt(rp, col)[:3])]
    torch.manual_seed(2)
    convs = [L.TransformerConv(32, 8, heads=4, fused=True).to(dev), L.TransformerConv(32, 6, fused=True).to(dev)]
    x, y = torch.randn(len(rp) - 1, 32, device=dev).requires_grad_(True), torch.randint(0, 6, (len(rp) - 1,), device=dev)
    T.prepare([], *meta, fused_attention=True)

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
    del graph, static, eager, step, convs
    gc.collect()   # (the captured graph's pool goes back now, not inside a later test's memory check)
