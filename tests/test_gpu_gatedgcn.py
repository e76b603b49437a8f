"""GatedGCN with edge features on the MI355X: tcgnn_gatedgcn_forward / _backward / _source_grad through the C ABI on rows of every length
class - by destination and, on the transposed graph, by source - at every width class, one float off alignment and at degenerate sizes,
the pybind module against the ctypes one, operator and layer against the dense fp64 model, a captured two-layer step.
Reference and bounds: tests/gatedgcn_ref.py; the figures the FIG lines printed on the MI355X: DESIGN.md 4.22."""
import glob
import importlib.util
import os

import numpy as np
import pytest
import torch

import gated_ref as R
import gatedgcn_ref as G
import graphs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, SENTINEL, INVALID_ARG = 4096, -12345.0, 1   # sentinel words behind every output; TCGNN_ERR_INVALID_ARG
NODE_OUT, EDGE_OUT = ("Y", "Den", "dk", "dq", "dv"), ("Z", "G")
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


def _run(T, trp, tcol, t, eps, dZ):   # the three kernels through the C ABI -> ({name: view}, {name: flat buffer}); dZ: a tensor or None
    import tcgnn_capi as C
    (n, D), E, stream = t["k"].shape, tcol.numel(), torch.cuda.current_stream().cuda_stream
    made = {name: _out(E if name in EDGE_OUT else n, D) for name in NODE_OUT + EDGE_OUT}
    bufs, o = {name: m[0] for name, m in made.items()}, {name: m[1] for name, m in made.items()}
    p = lambda x: None if x is None else x.data_ptr()   # noqa: E731
    assert C.lib.tcgnn_gatedgcn_forward(p(trp), p(tcol), n, E, p(t["k"]), p(t["q"]), p(t["v"]), p(t["c"]), D, eps, p(o["Y"]), p(o["Z"]), p(o["Den"]), stream) == 0
    assert C.lib.tcgnn_gatedgcn_backward(p(trp), p(tcol), n, E, p(t["dY"]), p(dZ), p(o["Y"]), p(o["Den"]), p(o["Z"]), p(t["v"]), D, eps, p(o["G"]),
                                         p(o["dk"]), stream) == 0
    rp_t, col_t, perm, _ = T.transpose_graph(trp, tcol)
    assert C.lib.tcgnn_gatedgcn_source_grad(p(rp_t), p(col_t), p(perm), n, E, p(o["G"]), p(o["Z"]), p(t["dY"]), p(o["Den"]), D, eps, p(o["dq"]),
                                            p(o["dv"]), stream) == 0
    return o, bufs


CASES = [(g, 64, s, 1e-6) for g in "AT" for s in (1, 4)] + [(g, D, 1, 1e-6) for g in "AT" for D in R.WIDTHS if D != 64] + [("A", 64, 1, 0.0)]


@pytest.mark.parametrize("graph,D,scale,eps", CASES, ids=["%s-D%d-x%d-eps%g" % c for c in CASES])
def test_the_three_kernels_on_rows_of_every_length_class(T, ext, graph, D, scale, eps):
    rp, col = R.row_class_graphs()[graph]
    host = G.inputs(len(rp) - 1, len(col), D, scale)
    ref = G.gatedgcn_f64(rp, col, host, eps)
    trp, tcol, t = _dev(rp), _dev(col), {name: _dev(a) for name, a in host.items()}
    o, bufs = _run(T, trp, tcol, t, eps, t["dZ"])
    _, bufs2 = _run(T, trp, tcol, t, eps, t["dZ"])
    bad = [] if np.array_equal(o["Z"].cpu().numpy().view(np.int32), ref["Z"].view(np.int32)) else ["Z is not numpy's fp32 sum bit for bit"]
    for name in NODE_OUT + EDGE_OUT:
        if name != "Z":
            share = G.share(o[name].cpu().numpy(), ref[name], G.BOUNDS[name])
            print("FIG gatedgcn %s D=%-3d x%d eps=%g %-3s worst share of its bound %.4f" % (graph, D, scale, eps, name, share))
            if not share <= 1.0:
                bad.append("%s exceeds its bound (%.3f)" % (name, share))
        if not torch.equal(bufs[name], bufs2[name]) or not bool((bufs[name][o[name].numel():] == SENTINEL).all()):
            bad.append("%s differs on repetition, or sentinels were written" % name)
    without, _ = _run(T, trp, tcol, t, eps, None)
    zeros, _ = _run(T, trp, tcol, t, eps, torch.zeros_like(t["dZ"]))
    if not all(torch.equal(without[name].view(torch.int32), zeros[name].view(torch.int32)) for name in ("G", "dk", "dq", "dv")):
        bad.append("dZ = NULL and dZ = 0 differ")
    for mod in (T, ext):
        Y, Z, Den = mod.forward_gatedgcn(t["k"], t["q"], t["v"], t["c"], trp, tcol, eps)
        dc, dk = mod.backward_gatedgcn(t["dY"], t["dZ"], Y, Den, Z, t["v"], trp, tcol, eps)
        dq, dv = mod.source_grad_gatedgcn(dc, Z, t["dY"], Den, trp, tcol, eps)
        dc0, _ = mod.backward_gatedgcn(t["dY"], None, Y, Den, Z, t["v"], trp, tcol, eps)
        pairs = zip((Y, Z, Den, dc, dk, dq, dv, dc0), [o[name] for name in ("Y", "Z", "Den", "G", "dk", "dq", "dv")] + [without["G"]])
        if not all(torch.equal(a, b) for a, b in pairs):
            bad.append("%s differs from the C call" % mod.__name__)
        mod.clear_plan_cache()
    assert not bad, bad


def test_operands_one_float_off_alignment_take_the_dword_form_and_give_the_same_bits(T):
    rp, col = R.row_class_graphs()["A"]
    aligned = {name: _dev(a) for name, a in G.inputs(len(rp) - 1, len(col), 64, 1).items()}
    off = {name: torch.empty(a.numel() + 1, device=dev)[1:].view(a.shape).copy_(a) for name, a in aligned.items()}
    assert all(a.data_ptr() % 16 == 0 for a in aligned.values()) and all(a.data_ptr() % 16 == 4 for a in off.values())
    want, _ = _run(T, _dev(rp), _dev(col), aligned, 1e-6, aligned["dZ"])
    got, bufs = _run(T, _dev(rp), _dev(col), off, 1e-6, off["dZ"])
    assert all(torch.equal(got[name], want[name]) and bool((bufs[name][got[name].numel():] == SENTINEL).all()) for name in NODE_OUT + EDGE_OUT)
    T.clear_plan_cache()


def test_degenerate_sizes_return_ok_and_invalid_arguments_are_refused_before_anything_is_written():
    import tcgnn_capi as C
    stream = torch.cuda.current_stream().cuda_stream
    fwd, bwd, src = C.lib.tcgnn_gatedgcn_forward, C.lib.tcgnn_gatedgcn_backward, C.lib.tcgnn_gatedgcn_source_grad
    n, E, D, eps = 10, 30, 5, 1e-6
    rp, col = torch.arange(0, E + 1, 3, dtype=torch.int32, device=dev), torch.zeros(E, dtype=torch.int32, device=dev)
    keep = torch.randn(n, D, device=dev), torch.randn(E, D, device=dev)   # (alive while their addresses are in use)
    X, M = keep[0].data_ptr(), keep[1].data_ptr()
    outs = {name: _out(E if name in EDGE_OUT else n, D) for name in NODE_OUT + EDGE_OUT}
    y, den, dk, dq, dv, z, g = (outs[name][1].data_ptr() for name in NODE_OUT + EDGE_OUT)
    assert fwd(None, None, n, 0, X, X, X, None, D, eps, y, None, den, stream) == 0 and bwd(None, None, n, 0, X, None, X, X, None, X, D, eps, None, dk, stream) == 0
    assert src(None, None, None, n, 0, None, None, X, X, D, eps, dq, dv, stream) == 0                                                        # E = 0
    for name in NODE_OUT:
        buf, view = outs[name]
        assert bool((view.view(torch.int32) == 0).all()) and bool((buf[n * D:] == SENTINEL).all())
        buf.fill_(SENTINEL)
    rp, col = rp.data_ptr(), col.data_ptr()
    good = ((fwd, [rp, col, n, E, X, X, X, M, D, eps, y, z, den], (2, 3, 8), (0, 1, 4, 5, 6, 7, 10, 11, 12), 9),
            (bwd, [rp, col, n, E, X, M, X, X, M, X, D, eps, g, dk], (2, 3, 10), (0, 1, 4, 6, 7, 8, 9, 12, 13), 11),
            (src, [rp, col, col, n, E, M, M, X, X, D, eps, dq, dv], (3, 4, 9), (0, 1, 2, 5, 6, 7, 8, 11, 12), 10))
    for call, args, sizes, arrays, at_eps in good:
        for nn, ee, dd in ((0, 0, D), (0, 5, D), (n, E, 0)):   # N = 0, D = 0: nothing to write
            a = list(args)
            a[sizes[0]], a[sizes[1]], a[sizes[2]] = nn, ee, dd
            assert call(*a, stream) == 0
        bad = [(i, -1) for i in sizes] + [(sizes[1], 1 << 31), (at_eps, -1.0), (at_eps, float("nan"))] + [(i, None) for i in arrays]
        for i, value in bad:
            assert call(*(args[:i] + [value] + args[i + 1:]), stream) == INVALID_ARG, (call.__name__, i, value)
    assert all(bool((buf == SENTINEL).all()) for buf, _ in outs.values())


def _held(what, got, want, values):   # everything on the path is fp32: `values` results at 1e-5 of the largest entry, the gradients behind them at 1e-4
    for i, (g, w) in enumerate(zip(got, want)):
        rel = float((g.detach().double().cpu() - w.detach()).abs().max()) / float(w.detach().abs().max())
        print("FIG gatedgcn %s %d: %.3e of the largest entry" % (what, i, rel))
        assert g.shape == w.shape and rel <= (G.VALUE_BOUND if i < values else G.GRAD_BOUND), (what, i, rel)


@pytest.mark.parametrize("where", ["operator", "operator_on_a_block", "layer", "layer_on_a_block", "layer_whose_edge_output_is_unused"])
def test_operator_and_layer_against_the_dense_fp64_model_on_a_directed_graph(T, where):
    import tcgnn_edge_ops as E
    import tcgnn_layers as L
    F = torch.nn.functional
    rp, col = graphs.uniform_graph(500, 6, seed=13, symmetric=False)
    meta = [_dev(rp), _dev(col)] + [torch.empty(0, dtype=torch.int32, device=dev)] * 3
    if where.endswith("on_a_block"):
        meta = L.sample_batch_rows(meta, torch.arange(0, 500, 7, device=dev), [4, 4], 11, plan=False).metas[0]
        rp, col = meta[0].cpu().numpy(), meta[1].cpu().numpy()
    n, ne, eps = len(rp) - 1, int(rp[-1]), 1e-6
    torch.manual_seed(3)
    if where.startswith("operator"):
        leaves, width = [torch.randn(n, 41) for _ in range(3)] + [torch.randn(ne, 41)], 41
        fn = lambda k, q, v, c: E.aggregate_gatedgcn(k, q, v, c, *meta[:2], eps)   # noqa: E731
        hi = lambda k, q, v, c: G.dense_f64(rp, col, k, q, v, c, eps)   # noqa: E731
    else:
        conv, width = L.GatedGCNConv(24, 8, 16, eps=eps), 16
        names = ("weights", "bias", "weights_edge", "bias_edge", "bn_nodes.weight", "bn_nodes.bias", "bn_edges.weight", "bn_edges.bias")
        leaves = [torch.randn(n, 24), torch.randn(ne, 8)] + [0.5 * torch.randn_like(conv.get_parameter(name)) + float(name in names[4::2]) for name in names]
        conv.to(dev)
        fn = lambda X, A, *ps: torch.func.functional_call(conv, dict(zip(names, ps)), (X, A, *meta))   # noqa: E731

        def hi(X, A, W, b, We, be, gn, bn, ge, bed):
            Ah, Bh, Dh, Eh = (X @ W + b).split(16, dim=1)
            Y, Z = G.dense_f64(rp, col, Eh, Dh, Bh, A @ We + be, eps)
            return torch.relu(F.batch_norm(Ah + Y, None, None, gn, bn, True)), torch.relu(F.batch_norm(Z, None, None, ge, bed, True))
    dH, dE = torch.randn(n, width, dtype=torch.float64), torch.randn(ne, width, dtype=torch.float64)
    if where == "layer_whose_edge_output_is_unused":
        dE = None   # (the autograd function then hands dZ = None to the row side)
    loss = lambda h, e, to: (h * dH.to(**to)).sum() + (0 if dE is None else (e * dE.to(**to)).sum())   # noqa: E731
    lo64, on_dev = [t.double().requires_grad_(True) for t in leaves], [t.to(dev).requires_grad_(True) for t in leaves]
    got, want = fn(*on_dev), hi(*lo64)
    wrt = slice(None, -2 if dE is None else None)   # (an unused e' leaves bn_edges' two parameters without a gradient)
    _held(where, tuple(got) + torch.autograd.grad(loss(*got, dict(device=dev, dtype=torch.float32)), on_dev[wrt]),
          tuple(want) + torch.autograd.grad(loss(*want, dict(dtype=torch.float64)), lo64[wrt]), 2)
    T.clear_plan_cache()


def test_a_two_layer_step_replays_from_a_hip_graph_bit_equal_and_free_memory_stays_flat(T):
    import tcgnn_layers as L
    rp, col = graphs.community_graph(3000, 10, 20, 0.8, seed=4)
    meta = [_dev(a) for a in (rp, col) + tuple(graphs.host_sgt(rp, col)[:3])]
    torch.manual_seed(2)
    convs = [L.GatedGCNConv(32, 8, 16).to(dev), L.GatedGCNConv(16, 16, 6).to(dev)]   # (the edge features flow: the second layer takes the first one's e')
    x, attr = torch.randn(len(rp) - 1, 32, device=dev).requires_grad_(True), torch.randn(len(col), 8, device=dev).requires_grad_(True)
    y = torch.randint(0, 6, (len(rp) - 1,), device=dev)
    T.prepare([], *meta, gated=True)

    wrt = [x, attr] + list(convs[0].parameters()) + [p for name, p in convs[1].named_parameters() if not name.startswith("bn_edges")]   # (the last e' is unused)

    def step():
        h, e = convs[0](x, attr, *meta)
        out, _ = convs[1](h, e, *meta)
        return torch.autograd.grad(torch.nn.functional.cross_entropy(out, y), wrt)

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
        differ = [(i, tuple(a.shape), float((a - b).abs().max())) for i, (a, b) in enumerate(zip(static, eager)) if not torch.equal(a, b)]
        assert not differ, differ   # (index into wrt, shape, largest difference)
    T.clear_plan_cache()
