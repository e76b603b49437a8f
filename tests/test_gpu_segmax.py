"""The max aggregation on the MI355X: tcgnn_segment_max / _backward on rows of every length class and at every width class, on the
boundary-shaped graphs and at degenerate sizes, the pybind module against the ctypes one, aggregate_max and SAGEConv against the dense
fp64 model, a captured training step, and training.  The restatements and input sets are tests/segmax_ref.py's.  The forward is held
to the reference BIT FOR BIT (a maximum is exact); the backward to `torch.equal` where the sums are exact (integer dY) and to the fp32
summation bound k 2^-24 sum|terms| otherwise."""
import glob
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import graphs
import segmax_ref as S
import walks as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64        # sentinel words behind Y, arg and dX
NO_ROW = 24       # entries of edgeList that no row covers (behind nodePointer[N])
SENTINEL = -12345
N_ROWS = 2048     # nodes of the row-length graph
INVALID_ARG = 1   # TCGNN_ERR_INVALID_ARG
WIDTHS = (1, 3, 4, 16, 41, 64, 65, 128, 256, 260)


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


def group_lanes(D):
    """lanes that own one neighbour row: the smallest power of two >= ceil(min(D, 256) / 4)"""
    need, g = (min(D, 256) + 3) // 4, 1
    while g < need:
        g *= 2
    return g


_ROW_GRAPHS = {}


def row_length_graph(G):
    """N_ROWS nodes; three rows - the winner planted at the first edge, at the last edge, at the first edge of the last partial step -
    of each length the kernel has a branch at for groups of G lanes (64 / G edges a step, four steps unrolled, kSegWaveRow = 1024, a
    workgroup taking 4 * 64 / G edges a trip), columns drawn with repetition from all nodes but the last, which only the planted
    positions name.  -> (rp, col, planted [(row, position)])"""
    if G not in _ROW_GRAPHS:
        eps = 64 // G
        lens = sorted({0, 1, eps - 1, eps, eps + 1, 4 * eps - 1, 4 * eps + 1, 1023, 1024, 1025, 4099, 70000})
        rng = np.random.default_rng(G)
        rows, planted = [], []
        for ln in lens:
            step = eps if ln <= 1024 else 4 * eps
            for where in (0, ln - 1, (ln - 1) // step * step):
                c = rng.integers(0, N_ROWS - 1, ln).astype(np.int32)
                if ln:
                    c[where] = N_ROWS - 1
                    planted.append((len(rows), where))
                rows.append(c)
        order = rng.permutation(N_ROWS)                     # the listed rows scattered over the graph, every other row empty or short
        lens_all = np.zeros(N_ROWS, dtype=np.int64)
        cols_all = [np.zeros(0, np.int32)] * N_ROWS
        for k, c in enumerate(rows):
            cols_all[order[k]] = c
        for r in order[len(rows):len(rows) + 600]:
            cols_all[r] = rng.integers(0, N_ROWS - 1, int(rng.integers(1, 40))).astype(np.int32)
        for r in range(N_ROWS):
            lens_all[r] = len(cols_all[r])
        rp = np.concatenate([[0], np.cumsum(lens_all)]).astype(np.int32)
        col = np.concatenate(cols_all).astype(np.int32)
        _ROW_GRAPHS[G] = (rp, col, [(int(order[k]), int(rp[order[k]]) + w) for k, w in planted])
    return _ROW_GRAPHS[G]


def _inputs(which, n, D, plant_row=None):
    X = S.input_set(which, n, D, seed=D)
    if plant_row is not None and which in ("ties", "normal"):
        X[plant_row] = 50.0                                # above everything else: the planted position has to win
    return X


_REF = {}   # (graph key, set, D) -> (Y, arg): computed once, shared, never changed


def _ref(key, rp, col, X):
    if key not in _REF:
        _REF[key] = S.segment_max(rp, col, X)
    return _REF[key]


def _guarded(dev, n_elems, dtype):
    buf = torch.full((n_elems + GUARD,), SENTINEL, dtype=dtype, device=dev)
    return buf, buf[:n_elems]


def _forward_case(dev, T, key, rp, col, X, what, ext=None):
    """one graph, one X, every call form -> (failures, Y, arg on the device)"""
    import tcgnn_capi as C
    bad = []
    rp = np.ascontiguousarray(rp, dtype=np.int32)
    n, E, D = len(rp) - 1, int(rp[-1]), X.shape[1]
    colp = np.zeros(E + NO_ROW, dtype=np.int32)
    colp[:E] = col[:E]
    trp, tcol, tX = _dev(dev, rp), _dev(dev, colp), _dev(dev, X)
    stream = torch.cuda.current_stream().cuda_stream
    Yr, argr = _ref(key, rp, col, X)
    outs = []
    for _ in range(2):
        ybuf, y = _guarded(dev, n * D, torch.float32)
        abuf, a = _guarded(dev, n * D, torch.int32)
        st = C.lib.tcgnn_segment_max(trp.data_ptr(), tcol.data_ptr(), n, E + NO_ROW, tX.data_ptr(), D, y.data_ptr(), a.data_ptr(), stream)
        assert st == 0, C.lib.tcgnn_last_error()
        outs.append((ybuf, abuf))
    (ybuf, abuf), (ybuf2, abuf2) = outs
    Y, arg = ybuf[:n * D].view(n, D), abuf[:n * D].view(n, D)
    if not torch.equal(Y.view(torch.int32).cpu(), torch.from_numpy(Yr.view(np.int32))):
        bad.append("%s: Y differs from the reference in %d elements" % (what, int((Y.view(torch.int32).cpu() != torch.from_numpy(Yr.view(np.int32))).sum())))
    if not torch.equal(arg.cpu(), torch.from_numpy(argr)):
        bad.append("%s: arg differs from the reference in %d elements" % (what, int((arg.cpu() != torch.from_numpy(argr)).sum())))
    has = arg >= 0
    if E:
        src = tcol[:E].long()[arg.clamp(min=0).long()]                               # [n, D]: the node the winner names
        picked = tX.view(torch.int32).gather(0, src)                                 # X[col[arg[i, d]], d]
        if not torch.equal(Y.view(torch.int32)[has], picked[has]):
            bad.append("%s: Y is not a copy of X[col[arg]]" % what)
    if bool((Y.view(torch.int32)[~has] != 0).any()):
        bad.append("%s: a row without edges is not +0" % what)
    if not (torch.equal(ybuf.view(torch.int32), ybuf2.view(torch.int32)) and torch.equal(abuf, abuf2)):
        bad.append("%s: the second call returns other bits" % what)
    if not (bool((ybuf[n * D:] == SENTINEL).all()) and bool((abuf[n * D:] == SENTINEL).all())):
        bad.append("%s: guard words written" % what)
    # the module's call (edgeList as long as the rows cover), with and without arg
    Ym, argm = T.forward_max(tX, trp, tcol[:E].contiguous())
    Yn, none = T.forward_max(tX, trp, tcol[:E].contiguous(), return_arg=False)
    if none is not None or not (torch.equal(Ym.view(torch.int32), Y.view(torch.int32)) and torch.equal(argm, arg) and torch.equal(Yn.view(torch.int32), Y.view(torch.int32))):
        bad.append("%s: TCGNN.forward_max differs from the C call" % what)
    if ext is not None:
        Ye, arge = ext.forward_max(tX, trp, tcol[:E].contiguous())
        if not (torch.equal(Ye.view(torch.int32), Y.view(torch.int32)) and torch.equal(arge, arg)):
            bad.append("%s: the pybind module differs from the ctypes one" % what)
    torch.cuda.synchronize()
    return bad, Y, arg


# ---- forward ---------------------------------------------------------------------------------------------------------------------------

WIDTH_CASES = [(D, s) for D in WIDTHS for s in ("ties", "normal")] + [(64, "signed_zero"), (64, "specials")]


@pytest.mark.parametrize("D,which", WIDTH_CASES, ids=["D%d-%s" % c for c in WIDTH_CASES])
def test_forward_on_rows_of_every_length_class_at_every_width(dev, T, ext, D, which):
    G = group_lanes(D)
    rp, col, planted = row_length_graph(G)
    X = _inputs(which, N_ROWS, D, plant_row=N_ROWS - 1)
    bad, Y, arg = _forward_case(dev, T, ("rows", G, which, D), rp, col, X, "row lengths G=%d D=%d %s" % (G, D, which), ext)
    if which in ("ties", "normal"):
        argh = arg.cpu().numpy()
        for r, pos in planted:
            if not (argh[r] == pos).all():
                bad.append("row %d (%d edges): the planted position %d did not win" % (r, rp[r + 1] - rp[r], pos - rp[r]))
    assert not bad, "\n  ".join(bad)


def test_forward_with_rows_off_sixteen_bytes_takes_the_dword_form_and_gives_the_same_bits(dev, T):
    import tcgnn_capi as C
    D = 64
    rp, col, _ = row_length_graph(group_lanes(D))
    n, E = len(rp) - 1, int(rp[-1])
    for which in ("ties", "specials"):
        X = _inputs(which, N_ROWS, D, plant_row=N_ROWS - 1)
        Yr, argr = _ref(("rows", group_lanes(D), which, D), rp, col, X)
        storage = torch.zeros(n * D + 1, dtype=torch.float32, device=dev)
        Xo = storage[1:].view(n, D)
        Xo.copy_(_dev(dev, X))
        assert Xo.data_ptr() % 16 == 4
        trp, tcol = _dev(dev, rp), _dev(dev, col)
        Y, arg = T.forward_max(Xo, trp, tcol)
        assert torch.equal(Y.view(torch.int32).cpu(), torch.from_numpy(Yr.view(np.int32))) and torch.equal(arg.cpu(), torch.from_numpy(argr))
        # backward with arg off sixteen bytes as well
        dY = _dev(dev, np.random.default_rng(2).integers(-8, 9, (n, D)).astype(np.float32))
        a_store = torch.zeros(n * D + 1, dtype=torch.int32, device=dev)
        a_off = a_store[1:].view(n, D)
        a_off.copy_(arg)
        assert torch.equal(T.backward_max(dY, a_off, trp, tcol), T.backward_max(dY, arg, trp, tcol))
    T.clear_plan_cache()


def _structure_graphs():
    out = [(name, rp, col) for name, rp, col in graphs.edge_case_graphs()]
    rp, col = graphs.uniform_graph(48, 3, seed=7)
    out.append(("with_empty_window_n48", *graphs.with_empty_window(rp, col, 16, 32)))
    out.append(("directed_n500", *graphs.uniform_graph(500, 6, seed=13, symmetric=False)))
    out.append(("hub_rows_n2500", *graphs.hub_rows_graph(2500, seed=77)))
    return out


STRUCTURES = {name: (rp, col) for name, rp, col in _structure_graphs()}


@pytest.mark.parametrize("name", list(STRUCTURES))
def test_forward_and_backward_on_structured_graphs(dev, T, ext, name):
    rp, col = STRUCTURES[name]
    n = len(rp) - 1
    bad = []
    for D, which in ((41, "ties"), (64, "normal")):
        X = _inputs(which, n, D)
        b, Y, arg = _forward_case(dev, T, (name, which, D), rp, col, X, "%s D=%d %s" % (name, D, which), ext)
        bad += b
        bad += _backward_case(dev, T, ext, (name, which, D), rp, col, arg, "%s D=%d %s" % (name, D, which))
    assert not bad, "\n  ".join(bad)
    T.clear_plan_cache()
    ext.clear_plan_cache()


# ---- backward --------------------------------------------------------------------------------------------------------------------------

_TRANSPOSED = {}


def _transposed(key, rp, col):
    if key not in _TRANSPOSED:
        rp_t, col_t, perm = W.transposed_csr(rp, col[:int(rp[-1])])
        _TRANSPOSED[key] = tuple(np.ascontiguousarray(a, dtype=np.int32) for a in (rp_t, col_t, perm))
    return _TRANSPOSED[key]


def _backward_case(dev, T, ext, key, rp, col, arg, what):
    """the C call over the host's transposed CSR into guarded buffers, twice; integer dY exactly, random dY within the summation bound;
    the two modules (their own device transpose) bit-equal to it"""
    import tcgnn_capi as C
    bad = []
    rp = np.ascontiguousarray(rp, dtype=np.int32)
    n, E, D = len(rp) - 1, int(rp[-1]), arg.shape[1]
    rp_t, col_t, perm = _transposed(key[0], rp, col)
    pad = lambda a: np.concatenate([a[:E], np.zeros(NO_ROW, np.int32)])   # noqa: E731
    trp_t, tcol_t, tperm = _dev(dev, rp_t), _dev(dev, pad(col_t)), _dev(dev, pad(perm))
    trp, tcol = _dev(dev, rp), _dev(dev, col[:E])
    argh = arg.cpu().numpy()
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(n + D)
    for kind, dY in (("integer", rng.integers(-8, 9, (n, D)).astype(np.float32)), ("random", rng.standard_normal((n, D)).astype(np.float32))):
        dX64, k, sabs = S.segment_max_backward(rp, col, argh, dY)
        tdY = _dev(dev, dY)
        outs = []
        for _ in range(2):
            buf, view = _guarded(dev, n * D, torch.float32)
            st = C.lib.tcgnn_segment_max_backward(trp_t.data_ptr(), tcol_t.data_ptr(), tperm.data_ptr(), n, E + NO_ROW, arg.data_ptr(), tdY.data_ptr(), D,
                                                  view.data_ptr(), stream)
            assert st == 0, C.lib.tcgnn_last_error()
            outs.append(buf)
        got = outs[0][:n * D].view(n, D)
        if bool((got == SENTINEL).any()):
            bad.append("%s: backward left %d elements of dX unwritten" % (what, int((got == SENTINEL).sum())))
        if not bool((outs[0][n * D:] == SENTINEL).all()):
            bad.append("%s: backward wrote guard words" % what)
        if not torch.equal(outs[0], outs[1]):
            bad.append("%s: the second backward call returns other bits" % what)
        gh = got.cpu().numpy().astype(np.float64)
        if kind == "integer":
            if not np.array_equal(gh, dX64):
                bad.append("%s: integer dY: dX differs from the exact sums in %d elements" % (what, int((gh != dX64).sum())))
        else:
            over = np.abs(gh - dX64) > k * 2.0 ** -24 * sabs
            share = float(np.max(np.abs(gh - dX64) / np.maximum(k * 2.0 ** -24 * sabs, 1e-300))) if E else 0.0
            print("FIG segmax backward %-44s largest |dX - dX64| = %.3f of k 2^-24 sum|terms|, most terms %d" % (what, share, int(k.max()) if k.size else 0))
            if over.any():
                bad.append("%s: random dY: %d elements beyond k 2^-24 sum|terms|" % (what, int(over.sum())))
        for mod, label in ((T, "TCGNN"), (ext, "the pybind module")):
            if mod is not None and not torch.equal(mod.backward_max(tdY, arg.contiguous(), trp, tcol), got):
                bad.append("%s: %s.backward_max differs from the C call" % (what, label))
    torch.cuda.synchronize()
    return bad


def test_backward_of_the_ties_forward_on_the_hub_graph_where_thousands_choose_one_source(dev, T, ext):
    rp, col = STRUCTURES["hub_rows_n2500"]
    n = len(rp) - 1
    bad = []
    for D in (3, 64, 260):
        X = _inputs("ties", n, D)
        b, Y, arg = _forward_case(dev, T, ("hub_rows_n2500", "ties", D), rp, col, X, "hub rows D=%d ties" % D)
        _, k, _ = S.segment_max_backward(rp, col, arg.cpu().numpy(), np.ones((n, D), np.float32))
        assert int(k.max()) >= 1000, "no source was chosen a thousand times: the case does not test what it is for"
        bad += b + _backward_case(dev, T, ext, ("hub_rows_n2500", "ties", D), rp, col, arg, "hub rows D=%d ties" % D)
    assert not bad, "\n  ".join(bad)
    T.clear_plan_cache()
    ext.clear_plan_cache()


def test_backward_on_the_row_length_graph(dev, T, ext):
    """the transposed rows of the row-length graph: the planted node is named once per listed row, every other node up to a few hundred times"""
    D = 16
    rp, col, _ = row_length_graph(group_lanes(D))
    X = _inputs("ties", N_ROWS, D, plant_row=N_ROWS - 1)
    b, Y, arg = _forward_case(dev, T, ("rows", group_lanes(D), "ties", D), rp, col, X, "row lengths D=16 ties")
    bad = b + _backward_case(dev, T, ext, ("rows%d" % group_lanes(D), "ties", D), rp, col, arg, "row lengths D=16 ties")
    assert not bad, "\n  ".join(bad)
    T.clear_plan_cache()
    ext.clear_plan_cache()


# ---- degenerate and refused calls ------------------------------------------------------------------------------------------------------

def test_degenerate_sizes_return_ok_and_fill_what_exists(dev, T):
    import tcgnn_capi as C
    stream = torch.cuda.current_stream().cuda_stream
    fwd, bwd = C.lib.tcgnn_segment_max, C.lib.tcgnn_segment_max_backward
    n, D = 37, 5
    rp0 = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    X = torch.randn(n, D, device=dev)
    ybuf, y = _guarded(dev, n * D, torch.float32)
    abuf, a = _guarded(dev, n * D, torch.int32)
    assert fwd(rp0.data_ptr(), None, n, 0, X.data_ptr(), D, y.data_ptr(), a.data_ptr(), stream) == 0          # E = 0
    assert bool((y.view(torch.int32) == 0).all()) and bool((a == -1).all())
    assert bool((ybuf[n * D:] == SENTINEL).all()) and bool((abuf[n * D:] == SENTINEL).all())
    xbuf, dx = _guarded(dev, n * D, torch.float32)
    assert bwd(rp0.data_ptr(), None, None, n, 0, a.data_ptr(), X.data_ptr(), D, dx.data_ptr(), stream) == 0
    assert bool((dx.view(torch.int32) == 0).all()) and bool((xbuf[n * D:] == SENTINEL).all())
    for nn, ee, dd in ((0, 0, D), (0, 5, D), (n, 7, 0)):                                                       # N = 0, D = 0: nothing to write
        ybuf, y = _guarded(dev, 8, torch.float32)
        abuf, a = _guarded(dev, 8, torch.int32)
        assert fwd(rp0.data_ptr(), rp0.data_ptr(), nn, ee, X.data_ptr(), dd, y.data_ptr(), a.data_ptr(), stream) == 0
        assert bwd(rp0.data_ptr(), rp0.data_ptr(), rp0.data_ptr(), nn, ee, a.data_ptr(), X.data_ptr(), dd, y.data_ptr(), stream) == 0
        assert bool((ybuf == SENTINEL).all()) and bool((abuf == SENTINEL).all())
    # the module's calls at those sizes
    col0 = torch.zeros(0, dtype=torch.int32, device=dev)
    Y, arg = T.forward_max(X, rp0, col0)
    assert Y.shape == (n, D) and not bool(Y.any()) and bool((arg == -1).all())
    assert not bool(T.backward_max(X, arg, rp0, col0).any())
    Y, arg = T.forward_max(torch.zeros(n, 0, device=dev), rp0, col0)
    assert Y.shape == (n, 0) and arg.shape == (n, 0)
    # row pointers with a descending pair and an entry beyond the array, column ids out of range: clamped, nothing faults
    E = 100
    wild = torch.tensor([0, 50, 40, 5000], dtype=torch.int32, device=dev)          # rows: [0, 50), empty, [40, 100)
    col = torch.arange(E, dtype=torch.int32, device=dev) % 3
    col[::7] = 1 << 30
    col[3::7] = -5
    X3 = torch.randn(3, 8, device=dev)
    ybuf, y = _guarded(dev, 24, torch.float32)
    abuf, a = _guarded(dev, 24, torch.int32)
    assert fwd(wild.data_ptr(), col.data_ptr(), 3, E, X3.data_ptr(), 8, y.data_ptr(), a.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    a = a.view(3, 8)
    assert bool((a[1] == -1).all()) and bool(((a[0] >= 0) & (a[0] < 50)).all()) and bool(((a[2] >= 40) & (a[2] < 100)).all())
    assert bool((ybuf[24:] == SENTINEL).all()) and bool((abuf[24:] == SENTINEL).all())
    clamped = col.clamp(0, 2).cpu().numpy()
    Yr, argr = S.segment_max(np.array([0, 50, 50, 50]), clamped, X3.cpu().numpy())
    assert torch.equal(a[0].cpu(), torch.from_numpy(argr[0]))


def test_invalid_arguments_are_refused_and_nothing_is_written(dev):
    import tcgnn_capi as C
    stream = torch.cuda.current_stream().cuda_stream
    n, E, D = 10, 30, 4
    rp = torch.arange(0, E + 1, 3, dtype=torch.int32, device=dev)
    col = torch.zeros(E, dtype=torch.int32, device=dev)
    X = torch.randn(n, D, device=dev)
    ybuf, y = _guarded(dev, n * D, torch.float32)
    abuf, a = _guarded(dev, n * D, torch.int32)
    p = lambda t: t.data_ptr()   # noqa: E731
    good = [p(rp), p(col), n, E, p(X), D, p(y), p(a)]
    for at, value in ((2, -1), (3, -1), (3, 1 << 31), (5, -1), (0, None), (1, None), (4, None), (6, None)):
        args = list(good)
        args[at] = value
        assert C.lib.tcgnn_segment_max(*args, stream) == INVALID_ARG, (at, value)
    good = [p(rp), p(col), p(col), n, E, p(a), p(X), D, p(y)]
    for at, value in ((3, -1), (4, -1), (4, 1 << 31), (7, -1), (0, None), (1, None), (2, None), (5, None), (6, None), (8, None)):
        args = list(good)
        args[at] = value
        assert C.lib.tcgnn_segment_max_backward(*args, stream) == INVALID_ARG, (at, value)
    torch.cuda.synchronize()
    assert bool((ybuf == SENTINEL).all()) and bool((abuf == SENTINEL).all())


def test_module_argument_checks(dev, T, ext):
    rp, col = graphs.uniform_graph(50, 4, seed=2)
    trp, tcol = _dev(dev, rp), _dev(dev, col)
    X = torch.randn(50, 8, device=dev)
    for mod in (T, ext):
        with pytest.raises(RuntimeError, match="num_nodes"):
            mod.forward_max(X[:49].contiguous(), trp, tcol)
        with pytest.raises(RuntimeError, match="Float"):
            mod.forward_max(X.double(), trp, tcol)
        with pytest.raises(RuntimeError, match="contiguous"):
            mod.forward_max(X.t().contiguous().t(), trp, tcol)
        Y, arg = mod.forward_max(X, trp, tcol)
        with pytest.raises(RuntimeError, match="arg must have"):
            mod.backward_max(X, arg[:, :4].contiguous(), trp, tcol)
        out = torch.empty_like(X)
        assert mod.forward_max(X, trp, tcol, out=out)[0].data_ptr() == out.data_ptr() and torch.equal(out, Y)
        with pytest.raises(RuntimeError, match="out must be a contiguous fp32"):
            mod.forward_max(X, trp, tcol, out=torch.empty(50, 9, device=dev))
    T.clear_plan_cache()
    ext.clear_plan_cache()


# ---- aggregate_max and SAGEConv against the dense fp64 model ---------------------------------------------------------------------------

def _rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double()
    assert got.shape == want.shape
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)


def _directed500():
    rp, col = graphs.uniform_graph(500, 6, seed=13, symmetric=False)
    assert not W.is_symmetric(rp, col)
    n = len(rp) - 1
    A = torch.zeros(n, n, dtype=torch.float64)
    A.index_put_((torch.from_numpy(np.repeat(np.arange(n), np.diff(rp))), torch.from_numpy(col).long()), torch.ones(len(col), dtype=torch.float64), accumulate=True)
    return rp, col, A


def test_aggregate_max_against_the_dense_fp64_model_on_a_directed_graph(dev, T):
    import tcgnn_edge_ops as E
    rp, col, A = _directed500()
    n = len(rp) - 1
    torch.manual_seed(1)
    X = torch.randn(n, 41)
    dY = torch.randn(n, 41, dtype=torch.float64)
    Xg = X.to(dev).requires_grad_(True)
    Y = E.aggregate_max(Xg, _dev(dev, rp), _dev(dev, col))
    Xd = X.double().requires_grad_(True)
    masked = Xd.unsqueeze(0).expand(n, -1, -1).masked_fill((A == 0).unsqueeze(2), float("-inf"))
    want = torch.where(A.sum(1, keepdim=True) > 0, masked.max(1).values, torch.zeros((), dtype=torch.float64))
    assert torch.equal(Y.detach().cpu().double(), want.detach())                      # a maximum is exact
    got, = torch.autograd.grad((Y * dY.float().to(dev)).sum(), Xg)
    ref, = torch.autograd.grad((want * dY).sum(), Xd)
    print("FIG aggregate_max dX %.3e of the largest entry" % _rel(got, ref))
    assert _rel(got, ref) <= 1e-4
    T.clear_plan_cache()


@pytest.mark.parametrize("dims", [(24, 16), (16, 24)], ids=["narrowing", "widening"])
@pytest.mark.parametrize("aggregator", ["max", "pool", "mean"])
def test_sage_layer_against_the_dense_fp64_model_on_a_directed_graph(dev, T, aggregator, dims):
    """max and pool: the bounds of tests/test_segmax_cpu.py (output 1e-5, gradients 1e-4 of the largest entry) - the aggregation is exact
    and the dense products are fp32.  mean is forward_scaled, whose operand is staged with a 10-bit mantissa (2^-11 = 4.9e-4 per element,
    which no fp32 bound can hold): it is held to 2e-3 of the largest entry, the project's condition for chained operators
    (tests/test_gpu_gat.py, tests/test_gpu_edge_ops.py)."""
    import tcgnn_layers as L
    rp, col, A = _directed500()
    n = len(rp) - 1
    meta = _meta(dev, rp, col)
    torch.manual_seed(3)
    conv = L.SAGEConv(*dims, aggregator=aggregator, directed=True)
    conv.bias.data.normal_()
    if aggregator == "pool":
        conv.bias_pool.data.normal_()
    X = torch.randn(n, dims[0])
    dY = torch.randn(n, dims[1], dtype=torch.float64)
    host = [conv.weights_self, conv.weights, conv.bias] + ([conv.weights_pool, conv.bias_pool] if aggregator == "pool" else [])
    leaves = [t.detach().double().requires_grad_(True) for t in [X] + host]
    conv = conv.to(dev)
    params = [conv.weights_self, conv.weights, conv.bias] + ([conv.weights_pool, conv.bias_pool] if aggregator == "pool" else [])
    Xg = X.to(dev).requires_grad_(True)
    Y = conv(Xg, *meta)
    want = S.dense_sage(A, leaves[0], leaves[1], leaves[2], leaves[3], aggregator, *leaves[4:])
    tol_y, tol_g = S.SAGE_TOL[aggregator]
    got = torch.autograd.grad((Y * dY.float().to(dev)).sum(), [Xg] + params)
    ref = torch.autograd.grad((want * dY).sum(), leaves)
    figs = [("Y", _rel(Y, want), tol_y)] + [(w, _rel(g, r), tol_g) for g, r, w in zip(got, ref, ("dX", "dW_self", "dW_neigh", "dbias", "dW_pool", "dbias_pool"))]
    for w, f, t in figs:
        print("FIG sage %-4s %-9s %-10s %.3e of the largest entry (bound %.0e)" % (aggregator, "%d->%d" % dims, w, f, t))
    assert all(f <= t for _, f, t in figs), figs
    T.clear_plan_cache()


# ---- a captured step, training, the harness --------------------------------------------------------------------------------------------

def test_a_prepared_sage_max_step_replays_from_a_hip_graph_bit_equal_and_allocates_nothing(dev, T):
    import tcgnn_layers as L
    rp, col = graphs.community_graph(3000, 10, 20, 0.8, seed=4)
    n = len(rp) - 1
    meta = _meta(dev, rp, col)
    torch.manual_seed(2)
    convs = [L.SAGEConv(32, 16, aggregator="max").to(dev), L.SAGEConv(16, 6, aggregator="pool").to(dev)]
    params = [p for cv in convs for p in cv.parameters()]
    x = torch.randn(n, 32, device=dev).requires_grad_(True)
    y = torch.randint(0, 6, (n,), device=dev)
    T.prepare([], *meta, max_aggregation=True)

    def step():
        out = convs[1](torch.relu(convs[0](x, *meta)), *meta)
        return torch.autograd.grad(torch.nn.functional.cross_entropy(out, y), [x] + params)

    eager = [g.clone() for g in step()]
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    m0 = torch.cuda.memory_allocated()
    for _ in range(3):
        g = step()
        del g
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0 and torch.cuda.memory_allocated() == m0
    torch.cuda.set_sync_debug_mode("error")      # a prepared step never synchronises
    try:
        g = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert all(torch.equal(a, b) for a, b in zip(g, eager))
    del g
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                # allocator warm-up on the side stream, as capture requires
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):   # one stream, no parallel branches
        static = step()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(static, eager):
        assert torch.equal(a, b), tuple(a.shape)
    del graph, static
    T.clear_plan_cache()


def _toy(tmp_path):
    f = np.load(os.path.join(ROOT, "tests", "golden", "dataset_toy.npz"))
    np.savez(os.path.join(tmp_path, "toy.npz"), src_li=f["src_li"], dst_li=f["dst_li"], num_nodes=f["num_nodes"])


def test_ten_adam_steps_of_a_two_layer_sage_max_net_on_the_toy_dataset_lower_the_loss(dev, T, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tc-gnn_atc23_amd"))
    import tcgnn_graph as TG
    import tcgnn_harness as H
    import tcgnn_layers as L
    _toy(tmp_path)
    ds = TG.TCGNN_dataset(os.path.join(tmp_path, "toy.npz"), 12, 5, load_from_txt=False, seed=0)
    rp, col = ds.row_pointers.numpy(), ds.column_index.numpy()
    meta = _meta(dev, rp, col)
    torch.manual_seed(0)
    model = H.Net(lambda a, b: L.SAGEConv(a, b, aggregator="max"), 12, 16, 5, 2).to(dev)
    g = torch.Generator().manual_seed(1)
    y = torch.randint(0, 5, (ds.num_nodes,), generator=g)
    x = (torch.randn(ds.num_nodes, 12, generator=g) + torch.nn.functional.one_hot(y, 12).float()).to(dev)   # features that tell the label
    y = y.to(dev)
    opt = H.make_adam(model.parameters())
    model.eval()                                                                                             # (no dropout: the same net every step)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = H.node_nll_loss(model(x, meta), y)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("FIG sage max training loss %.4f -> %.4f" % (losses[0], losses[-1]))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    T.clear_plan_cache()


@pytest.mark.parametrize("aggregator", ["mean", "max", "pool"])
def test_harness_prints_its_usual_lines_for_the_sage_model(tmp_path, aggregator):
    _toy(tmp_path)
    env = dict(os.environ, PYTHONWARNINGS="ignore")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tc-gnn_atc23_amd", "tcgnn_harness.py"), "--dataset", "toy", "--graph_dir", str(tmp_path), "--dim", "12",
                        "--hidden", "16", "--classes", "5", "--epochs", "3", "--model", "sage", "--aggregator", aggregator],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout
    assert "model='sage'" in out and "aggregator='%s'" % aggregator in out and "dataset='toy'" in out
    assert re.search(r"^TC_Blocks:\t\d+$", out, re.M) and re.search(r"^Exp_Edges:\t\d+$", out, re.M)
    assert re.search(r"^Prep\. \(ms\):\t\d+\.\d{3}$", out, re.M) and re.search(r"^Train \(ms\):\t\s*\d+\.\d{3}$", out, re.M)
    assert out.index("Prep.") < out.index("Train (ms)")
