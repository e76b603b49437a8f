"""The fused edge-projection operators (forward_uep / backward_uep / source_grad_uep, tcgnn_edge_project_*) against the fp64 model of
tests/edge_project_ref.py: exact on integer-valued inputs, within the derived bounds on normal ones; GINEConv(fuse_edge=True) against
the unfused layer, on the pybind module with the same bits, and from a captured HIP graph; the C ABI's refusals and zero sizes."""
import glob
import importlib.util
import os

import numpy as np
import pytest
import torch

import edge_project_ref as R
import graphs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 1
SENTINEL = -12345.0
SHAPES = [(1, 1), (3, 4), (4, 20), (16, 64), (63, 260), (16, 260), (63, 20)]   # (K, D)


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


def _graph(name):
    """rows: ~2000 nodes, two rows of every length the kernels branch at (tiles of 16, the wavefront-row limit 1024, a long row that is
    no multiple of 16) scattered among 400 short rows, columns drawn with repetition (in-degrees stay below 32); rows_t: its transpose
    as the CSR, so that the SOURCE side walks those row lengths, the long rows on four wavefronts among them; powerlaw: directed;
    many_rows: more chunks of 16 rows than the row-side backward has workgroups (512)."""
    if name == "rows_t":
        rp, col = _graph("rows")
        rows = np.repeat(np.arange(len(rp) - 1, dtype=np.int32), np.diff(rp))
        counts = np.bincount(col, minlength=len(rp) - 1)
        return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), rows[np.argsort(col, kind="stable")]
    if name == "powerlaw":
        return graphs.powerlaw_graph(1500, 8, seed=7, symmetric=False)
    if name == "many_rows":
        return graphs.uniform_graph(9000, 3, seed=3, symmetric=False)
    n, rng = 2000, np.random.default_rng(16)
    lens = [ln for ln in (0, 1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 4099) for _ in range(2)]
    order = rng.permutation(n)
    cols = [np.zeros(0, np.int32)] * n
    for k, ln in enumerate(lens):
        cols[order[k]] = rng.integers(0, n, ln).astype(np.int32)
    for r in order[len(lens):len(lens) + 400]:
        cols[r] = rng.integers(0, n, int(rng.integers(1, 40))).astype(np.int32)
    return np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32), np.concatenate(cols).astype(np.int32)


def _inputs(rp, col, K, D, integers, seed=0):
    rng = np.random.default_rng(seed)
    n, E = len(rp) - 1, len(col)
    if integers:
        draw = lambda lim, *s: rng.integers(-lim, lim + 1, s).astype(np.float32)   # noqa: E731
        return draw(8, n, D), draw(3, E, K), draw(3, K, D), draw(3, D), draw(4, n, D)
    return tuple(rng.standard_normal(s).astype(np.float32) for s in ((n, D), (E, K), (K, D), (D,), (n, D)))


def _put(dev, a, offset=0):
    """a on the device, `offset` floats behind a 16-byte boundary"""
    buf = torch.empty(a.size + offset, dtype=torch.from_numpy(a).dtype, device=dev)
    view = buf[offset:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


def _run(T, dev, rp, col, arrays, act, offset=0):
    X, A, We, be, dY = (_put(dev, a, offset) for a in arrays)
    trp, tcol = _put(dev, rp), _put(dev, col)
    out = lambda: _put(dev, np.full(arrays[0].shape, np.nan, np.float32), offset)   # noqa: E731
    Y = T.forward_uep(X, A, We, be, trp, tcol, act=act, out=out())
    dA, dWe, dbe = T.backward_uep(dY, X, A, We, be, trp, tcol, act=act)
    dX = T.source_grad_uep(dY, X, A, We, be, trp, tcol, act=act, out=out())
    again = (T.forward_uep(X, A, We, be, trp, tcol, act=act),) + T.backward_uep(dY, X, A, We, be, trp, tcol, act=act) + \
            (T.source_grad_uep(dY, X, A, We, be, trp, tcol, act=act),)
    got = (Y, dA, dWe, dbe, dX)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, again)), "a repeated call differs"
    T.clear_plan_cache()
    return [t.cpu() for t in got]


NAMES = ("Y", "dA", "dWe", "dbe", "dX")


def _exact(T, dev, graph, K, D, act, offset=0):
    rp, col = _graph(graph)
    arrays = _inputs(rp, col, K, D, integers=True)
    S, _ = R.forward(rp, col, *arrays[:4], act)
    ref = (S,) + R.backward(rp, col, *arrays, act)[0]
    got = _run(T, dev, rp, col, arrays, act, offset)
    bad = ["%s: %d of %d elements differ" % (w, int((g != torch.from_numpy(r.astype(np.float32))).sum()), g.numel())
           for w, g, r in zip(NAMES, got, ref) if not torch.equal(g, torch.from_numpy(r.astype(np.float32)))]
    assert not bad, bad


@pytest.mark.parametrize("act", ["relu", "identity"])
@pytest.mark.parametrize("K,D", SHAPES)
def test_integer_inputs_give_the_exact_sums_on_rows_of_every_length(dev, T, K, D, act):
    _exact(T, dev, "rows", K, D, act)


@pytest.mark.parametrize("act", ["relu", "identity"])
@pytest.mark.parametrize("K,D", [(16, 64), (63, 260), (63, 20), (4, 20)])
def test_integer_inputs_exact_with_the_source_side_on_rows_of_every_length(dev, T, K, D, act):
    """dX over in-degrees 0, 1, 15 - 17, 31 - 33, 1023 - 1025 and 4099: several trips of the two-tiles-in-flight loop, the four-wavefront
    rows and their LDS combine; 1025 and 4099 leave wavefront 0 an odd tile count (one live tile of two in its last trip), at K = 63 too"""
    _exact(T, dev, "rows_t", K, D, act)


@pytest.mark.parametrize("graph,K,D,offset", [("powerlaw", 16, 64, 0), ("powerlaw", 3, 20, 0), ("many_rows", 16, 20, 0), ("rows", 16, 64, 1),
                                               ("rows", 4, 20, 1), ("rows_t", 16, 64, 1)],
                         ids=["powerlaw", "powerlaw_k3", "more_chunks_than_workgroups", "one_float_off", "one_float_off_k4", "one_float_off_source_rows"])
def test_integer_inputs_exact_on_other_graphs_and_unaligned_operands(dev, T, graph, K, D, offset):
    _exact(T, dev, graph, K, D, "relu", offset)


@pytest.mark.parametrize("graph", ["rows", "powerlaw"])
@pytest.mark.parametrize("K,D", SHAPES)
def test_normal_inputs_stay_within_the_derived_bounds(dev, T, graph, K, D):
    rp, col = _graph(graph)
    arrays = _inputs(rp, col, K, D, integers=False, seed=K + D)
    worst = {}
    for act in ("relu", "identity"):
        S, bound = R.forward(rp, col, *arrays[:4], act)
        got = _run(T, dev, rp, col, arrays, act)
        worst["Y " + act] = float((np.abs(got[0].numpy().astype(np.float64) - S) / bound).max())
        if act == "identity":   # (no mask can flip)
            refs, bounds = R.backward(rp, col, *arrays, act)
            for w, g, r, b in zip(NAMES[1:], got[1:], refs, bounds):
                worst[w] = float((np.abs(g.numpy().astype(np.float64) - r) / b).max())
    print("FIG uep %-8s K=%2d D=%3d worst share of the bound: %s" % (graph, K, D, "  ".join("%s %.3f" % kv for kv in worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst


# ---- the layer ------------------------------------------------------------------------------------------------------------------------

def _layer_graph(name):
    if name == "layers_n200":
        f = np.load(os.path.join(ROOT, "tests", "golden", "layers_n200.npz"))
        return f["rowptr"].astype(np.int32), f["col"].astype(np.int32)
    return graphs.powerlaw_graph(3000, 12, seed=31, symmetric=False)


def _meta(dev, rp, col):
    bp, e2c, e2r, _ = graphs.host_sgt(rp, col)
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (rp, col, bp, e2c, e2r)]


def _layer_pair(dev, seed, *args, **kw):
    import tcgnn_layers as L
    torch.manual_seed(seed)
    plain = L.GINEConv(*args, **kw)
    plain.bias_edge.data.normal_()
    fused = L.GINEConv(*args, fuse_edge=True, **kw)
    fused.load_state_dict(plain.state_dict())
    return plain.to(dev), fused.to(dev)


def _layer_run(conv, meta, X, EA):
    Y = conv(X, *meta, edge_attr=EA)
    return [Y.detach()] + list(torch.autograd.grad(Y.square().sum(), [X, EA] + list(conv.parameters())))


@pytest.mark.parametrize("name", ["layers_n200", "powerlaw_n3000_directed"])
def test_gine_layer_with_fuse_edge_matches_the_unfused_layer(dev, T, name):
    rp, col = _layer_graph(name)
    meta = _meta(dev, rp, col)
    plain, fused = _layer_pair(dev, 3, 24, 16, edge_dim=5, eps=0.25, train_eps=True)
    X = torch.randn(len(rp) - 1, 24, device=dev).requires_grad_(True)
    EA = torch.randn(len(col), 5, device=dev).requires_grad_(True)
    want, got = _layer_run(plain, meta, X, EA), _layer_run(fused, meta, X, EA)
    names = ["Y", "dX", "dedge_attr"] + ["d" + n for n, _ in fused.named_parameters()]
    figs = [(w, float((g - r).abs().max()) / float(r.abs().max()), 1e-5 if w == "Y" else 1e-4) for w, g, r in zip(names, got, want)]
    for w, f, t in figs:
        print("FIG gine fuse_edge %-24s %-14s %.3e of the largest entry (bound %.0e)" % (name, w, f, t))
    assert len(figs) == 8 and all(f <= t for _, f, t in figs), figs
    T.clear_plan_cache()


def test_fuse_edge_is_refused_without_a_usable_edge_dim():
    import tcgnn_layers as L
    for edge_dim in (None, 0, 64):
        with pytest.raises(ValueError):
            L.GINEConv(8, 8, edge_dim=edge_dim, fuse_edge=True)
    assert not L.GINEConv(8, 8, edge_dim=4).fuse_edge


def test_fused_layer_runs_on_the_pybind_module_with_the_same_bits(dev, T, ext):
    import tcgnn_layers as L
    rp, col = _layer_graph("powerlaw_n3000_directed")
    meta = _meta(dev, rp, col)
    _, fused = _layer_pair(dev, 5, 16, 8, edge_dim=4, train_eps=True)
    X = torch.randn(len(rp) - 1, 16, device=dev).requires_grad_(True)
    EA = torch.randn(len(col), 4, device=dev).requires_grad_(True)
    mine = _layer_run(fused, meta, X, EA)
    old = L._backend
    L.set_backend(ext)
    try:
        theirs = _layer_run(fused, meta, X, EA)
    finally:
        L.set_backend(old)
        ext.clear_plan_cache()
    assert all(torch.equal(a, b) for a, b in zip(mine, theirs))
    T.clear_plan_cache()


def test_a_prepared_fused_step_replays_from_a_hip_graph_bit_equal(dev, T):
    rp, col = graphs.community_graph(3000, 10, 20, 0.8, seed=4)
    meta = _meta(dev, rp, col)
    convs = [_layer_pair(dev, 2, 32, 16, edge_dim=8, train_eps=True)[1], _layer_pair(dev, 4, 16, 6, edge_dim=8)[1]]
    params = [p for cv in convs for p in cv.parameters()]
    x = torch.randn(len(rp) - 1, 32, device=dev).requires_grad_(True)
    ea = torch.randn(len(col), 8, device=dev).requires_grad_(True)
    y = torch.randint(0, 6, (len(rp) - 1,), device=dev)
    T.prepare([32, 16], *meta, edge_project=8)   # (the transposed CSR and the scratch of backward_uep's partials)

    def step():
        out = convs[1](torch.relu(convs[0](x, *meta, edge_attr=ea)), *meta, edge_attr=ea)
        return torch.autograd.grad(torch.nn.functional.cross_entropy(out, y), [x, ea] + params)

    eager = [g.clone() for g in step()]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")      # a prepared step never synchronises
    try:
        g = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert all(torch.equal(a, b) for a, b in zip(g, eager))
    del g
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                # allocator and buffer-pool warm-up on the side stream, as capture requires
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):   # one stream, no parallel branches
        static = step()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(static, eager):
            assert torch.equal(a, b), tuple(a.shape)
    del graph, static
    T.clear_plan_cache()


# ---- the C ABI: refusals and zero sizes -----------------------------------------------------------------------------------------------

def _abi(dev):
    n, E, K, D = 10, 30, 4, 8
    t = dict(rp=torch.arange(0, E + 1, 3, dtype=torch.int32, device=dev), col=torch.zeros(E, dtype=torch.int32, device=dev),
             X=torch.randn(n, D, device=dev), A=torch.randn(E, K, device=dev), We=torch.randn(K, D, device=dev), be=torch.randn(D, device=dev),
             ws=torch.empty(1 << 16, dtype=torch.uint8, device=dev))
    for name, size in (("Y", n * D), ("dA", E * K), ("dWe", K * D), ("dbe", D)):
        t[name] = torch.full((size + 64,), SENTINEL, device=dev)
    return n, E, K, D, t


def test_invalid_arguments_are_refused_and_nothing_is_written(dev):
    import tcgnn_capi as C
    stream = torch.cuda.current_stream().cuda_stream
    n, E, K, D, t = _abi(dev)
    p = {k: v.data_ptr() for k, v in t.items()}
    fwd = [p["rp"], p["col"], n, E, p["X"], p["A"], p["We"], p["be"], K, D, 1, p["Y"]]
    bwd = [p["rp"], p["col"], n, E, p["X"], p["A"], p["We"], p["be"], p["X"], K, D, 1, p["dA"], p["dWe"], p["dbe"], p["ws"], t["ws"].numel()]
    src = [p["rp"], p["col"], p["col"], n, E, p["X"], p["A"], p["We"], p["be"], p["X"], K, D, 1, p["Y"]]
    calls = ((C.lib.tcgnn_edge_project_message, fwd, 8, ((2, -1), (3, -1), (9, -1), (10, 2), (0, None), (5, None), (6, None), (11, None))),
             (C.lib.tcgnn_edge_project_backward, bwd, 9, ((2, -1), (3, 1 << 31), (10, -1), (11, 7), (1, None), (8, None), (12, None), (13, None), (14, None))),
             (C.lib.tcgnn_edge_project_source_grad, src, 10, ((3, -1), (4, -1), (11, -1), (12, -1), (2, None), (9, None), (13, None))))
    for fn, good, k_at, bad in calls:
        for at, value in ((k_at, 0), (k_at, 64)) + bad:
            args = list(good)
            args[at] = value
            assert fn(*args, stream) == INVALID_ARG, (fn.__name__, at, value)
    torch.cuda.synchronize()
    assert all(bool((t[k] == SENTINEL).all()) for k in ("Y", "dA", "dWe", "dbe"))
    assert all(fn(*good, stream) == 0 for fn, good, _, _ in calls)


def test_zero_sizes_return_ok_and_zero_what_has_elements(dev):
    import tcgnn_capi as C
    stream = torch.cuda.current_stream().cuda_stream
    n, E, K, D, t = _abi(dev)
    p = {k: v.data_ptr() for k, v in t.items()}
    zrp = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    assert C.lib.tcgnn_edge_project_message(zrp.data_ptr(), None, n, 0, p["X"], None, p["We"], p["be"], K, D, 1, p["Y"], stream) == 0      # E = 0
    assert C.lib.tcgnn_edge_project_message(None, None, 0, 0, None, None, None, None, K, D, 1, None, stream) == 0                         # N = 0
    assert C.lib.tcgnn_edge_project_backward(None, None, 0, E, None, None, None, None, None, K, D, 1, p["dA"], p["dWe"], p["dbe"], None, 0, stream) == 0   # N = 0
    torch.cuda.synchronize()
    for k, size in (("Y", n * D), ("dA", E * K), ("dWe", K * D), ("dbe", D)):
        assert bool((t[k][:size] == 0).all()) and bool((t[k][size:] == SENTINEL).all()), k
    t["Y"].fill_(SENTINEL)
    assert C.lib.tcgnn_edge_project_source_grad(zrp.data_ptr(), None, None, n, 0, None, None, None, None, None, K, D, 0, p["Y"], stream) == 0   # E = 0
    assert C.lib.tcgnn_edge_project_backward(None, None, n, E, None, None, None, None, None, K, 0, 1, p["dA"], None, None, None, 0, stream) == 0   # D = 0
    torch.cuda.synchronize()
    assert bool((t["Y"][:n * D] == 0).all()) and bool((t["Y"][n * D:] == SENTINEL).all()) and bool((t["dA"][:E * K] == 0).all())
