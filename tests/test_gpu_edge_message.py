"""Message passing with a feature vector per edge on the MI355X: tcgnn_edge_message / _backward and tcgnn_edge_sum on rows of every
length class at every width class, through perm on transposed and power-law graphs, their memory contract, degenerate sizes and
refusals, the pybind module against the ctypes one, aggregate_ue and GINEConv against the fp64 model, a captured training step, and
training.  The restatements, the input sets and the bound are tests/edge_message_ref.py's.  Y and edge_sum are held to `torch.equal`
where the sums are exact (integer inputs) and to 2^-24 |S| + 2^-149 + 2^-40 sum|terms| otherwise; dM to the reference's BITS on every
set.  EVERY element of every output is compared: no helper here samples or caps what it looks at."""
import glob
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import edge_message_ref as R
import graphs
import walks as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64        # sentinel words behind Y and dM
NO_ROW = 24       # entries of edgeList (rows of Ef, dM) that no row covers (behind nodePointer[N])
SENTINEL = -12345.0
POISON = 1e30     # what the uncovered rows of Ef / M and the node the uncovered column ids name hold
N_ROWS = 2048     # nodes of the row-length graph
INVALID_ARG = 1   # TCGNN_ERR_INVALID_ARG
WIDTHS = (1, 3, 4, 16, 41, 64, 65, 128, 256, 260)
FULL_WIDTHS = (4, 64, 260)
ACT = {"identity": 0, "relu": 1}


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
    """lanes that own one edge: the smallest power of two >= ceil(min(D, 256) / 4)"""
    need, g = (min(D, 256) + 3) // 4, 1
    while g < need:
        g *= 2
    return g


_ROW_GRAPHS = {}


def row_length_graph(G, full):
    """N_ROWS nodes; two rows of each length the kernels have a branch at for groups of G lanes (64 / G edges a step, four steps
    unrolled, rows beyond 1024 edges on the whole workgroup at 4 * 64 / G edges a trip) - and, with `full`, one row of 70 000 edges -
    scattered over the graph among 600 short rows and empty ones; columns drawn with repetition from all nodes but the last, which no
    covered position names (the NO_ROW uncovered ones do).  -> (rp, col)"""
    if (G, full) not in _ROW_GRAPHS:
        eps = 64 // G
        lens = sorted({0, 1, eps - 1, eps, eps + 1, 4 * eps - 1, 4 * eps + 1, 1023, 1024, 1025, 4099})
        lens = [ln for ln in lens for _ in range(2)] + ([70000] if full else [])
        rng = np.random.default_rng(G)
        order = rng.permutation(N_ROWS)
        cols_all = [np.zeros(0, np.int32)] * N_ROWS
        for k, ln in enumerate(lens):
            cols_all[order[k]] = rng.integers(0, N_ROWS - 1, ln).astype(np.int32)
        for r in order[len(lens):len(lens) + 600]:
            cols_all[r] = rng.integers(0, N_ROWS - 1, int(rng.integers(1, 40))).astype(np.int32)
        rp = np.concatenate([[0], np.cumsum([len(c) for c in cols_all])]).astype(np.int32)
        _ROW_GRAPHS[(G, full)] = (rp, np.concatenate(cols_all).astype(np.int32))
    return _ROW_GRAPHS[(G, full)]


_REF = {}   # key -> the reference of one (graph, set, width, act): computed once, shared, never changed


def _ref(key, rp, col, X, Ef, dY, act):
    if key not in _REF:
        E = int(rp[-1])
        Y, S, A = R.edge_message(rp, col, X, Ef, act)
        dM = R.edge_message_backward(rp, col, X, Ef, dY, act, num_edges=E + NO_ROW)
        _REF[key] = (Y, S, A, dM, R.edge_sum(rp, None, dM))
    return _REF[key]


def _guarded(dev, n_elems):
    buf = torch.full((n_elems + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[:n_elems]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _held(what, got, ref32, S, A, exact, bad, figs):
    """got (device, fp32) against the reference: bit-equal where the sums are exact, within the bound otherwise"""
    if exact:
        if not torch.equal(got.cpu(), torch.from_numpy(ref32)):
            bad.append("%s: differs from the exact sums in %d elements" % (what, int((got.cpu() != torch.from_numpy(ref32)).sum())))
    else:
        whole, excess = R.share(got.cpu().numpy(), S, A)
        figs.append((what, whole, excess))
        if not whole <= 1.0:
            bad.append("%s: %.3f of the bound" % (what, whole))


def _case(dev, T, ext, key, rp, col, which, D, act):
    """one graph, one input set, one width, one activation: the three C calls into guarded buffers with NO_ROW uncovered positions,
    twice; then both modules against them"""
    import tcgnn_capi as C
    bad, figs = [], []
    rp = np.ascontiguousarray(rp, dtype=np.int32)
    n, E = len(rp) - 1, int(rp[-1])
    X, Ef, dY = R.input_set(which, n, E, D, seed=D)
    X[n - 1] = POISON                                     # the node only the uncovered column ids name
    Yr, S, A, dMr, (Ysr, Ss, As) = _ref(key, rp, col, X, Ef, dY, act)
    colp = np.full(E + NO_ROW, n - 1, dtype=np.int32)
    colp[:E] = col[:E]
    Efp = np.full((E + NO_ROW, D), POISON, dtype=np.float32)
    Efp[:E] = Ef
    trp, tcol, tX, tEf, tdY = _dev(dev, rp), _dev(dev, colp), _dev(dev, X), _dev(dev, Efp), _dev(dev, dY)
    stream = torch.cuda.current_stream().cuda_stream
    exact = which == "integer"
    what = "%s D=%d %s %s" % (key[0], D, which, act)
    code = ACT[act]
    outs = []
    for _ in range(2):
        ybuf, y = _guarded(dev, n * D)
        mbuf, m = _guarded(dev, (E + NO_ROW) * D)
        sbuf, s = _guarded(dev, n * D)
        assert C.lib.tcgnn_edge_message(trp.data_ptr(), tcol.data_ptr(), n, E + NO_ROW, tX.data_ptr(), tEf.data_ptr(), D, code, y.data_ptr(), stream) == 0, C.lib.tcgnn_last_error()
        assert C.lib.tcgnn_edge_message_backward(trp.data_ptr(), tcol.data_ptr(), n, E + NO_ROW, tX.data_ptr(), tEf.data_ptr(), tdY.data_ptr(), D, code,
                                                 m.data_ptr(), stream) == 0, C.lib.tcgnn_last_error()
        assert C.lib.tcgnn_edge_sum(trp.data_ptr(), None, n, E + NO_ROW, m.data_ptr(), D, s.data_ptr(), stream) == 0, C.lib.tcgnn_last_error()
        outs.append((ybuf, mbuf, sbuf))
    (ybuf, mbuf, sbuf), second = outs
    Y, dM, Ys = ybuf[:n * D].view(n, D), mbuf[:(E + NO_ROW) * D].view(E + NO_ROW, D), sbuf[:n * D].view(n, D)
    if which == "boundary":   # NaNs: where the reference has one the kernel must, everywhere else the bound (R.share checks both)
        _held(what + " Y", Y, Yr, S, A, False, bad, figs)
    else:
        _held(what + " Y", Y, Yr, S, A, exact, bad, figs)
    if not torch.equal(_bits(dM).cpu(), torch.from_numpy(dMr.view(np.int32))):
        bad.append("%s: dM differs from the reference's bits in %d elements" % (what, int((_bits(dM).cpu() != torch.from_numpy(dMr.view(np.int32))).sum())))
    _held(what + " edge_sum(dM)", Ys, Ysr, Ss, As, exact, bad, figs)
    if bool((_bits(Y)[torch.from_numpy(np.diff(rp) == 0).to(dev)] != 0).any()):
        bad.append("%s: a row without edges is not +0" % what)
    for a, b, name in zip((ybuf, mbuf, sbuf), second, ("Y", "dM", "edge_sum")):
        if not torch.equal(_bits(a), _bits(b)):
            bad.append("%s: the second %s call returns other bits" % (what, name))
    if not all(bool((b[k:] == SENTINEL).all()) for b, k in ((ybuf, n * D), (mbuf, (E + NO_ROW) * D), (sbuf, n * D))):
        bad.append("%s: guard words written" % what)
    # the modules' calls (edgeList, Ef and dM as long as the rows cover)
    tcolE, tEfE = tcol[:E].contiguous(), tEf[:E].contiguous()
    for mod, label in ((T, "TCGNN"), (ext, "the pybind module")):
        Ym = mod.forward_ue(tX, tEfE, trp, tcolE, act=act)
        dMm = mod.backward_ue(tdY, tX, tEfE, trp, tcolE, act=act)
        Ysm = mod.edge_sum(dMm, trp)
        if not (torch.equal(_bits(Ym), _bits(Y)) and torch.equal(_bits(dMm), _bits(dM[:E])) and torch.equal(_bits(Ysm), _bits(Ys))):
            bad.append("%s: %s differs from the C calls" % (what, label))
    torch.cuda.synchronize()
    for w, whole, excess in figs:
        print("FIG edge_message %-52s %.3f of the bound, %.3e of the summation's allowance beyond the result's own rounding" % (w, whole, excess))
    return bad


# ---- rows of every length class ----------------------------------------------------------------------------------------------------

SHORT_CASES = [(D, s, "relu") for D in WIDTHS for s in ("integer", "normal", "large")] + [(64, "boundary", "relu")] + \
              [(D, s, "identity") for D in (3, 64, 260) for s in ("integer", "normal")]
FULL_CASES = [(D, s, "relu") for D in FULL_WIDTHS for s in ("integer", "normal", "large")]


@pytest.mark.parametrize("D,which,act", SHORT_CASES, ids=["D%d-%s-%s" % c for c in SHORT_CASES])
def test_rows_of_every_length_class_at_every_width(dev, T, ext, D, which, act):
    G = group_lanes(D)
    rp, col = row_length_graph(G, False)
    bad = _case(dev, T, ext, ("rows G=%d" % G, which, D, act), rp, col, which, D, act)
    assert not bad, "\n  ".join(bad)


@pytest.mark.parametrize("D,which,act", FULL_CASES, ids=["D%d-%s-%s" % c for c in FULL_CASES])
def test_rows_up_to_seventy_thousand_edges(dev, T, ext, D, which, act):
    G = group_lanes(D)
    rp, col = row_length_graph(G, True)
    assert int(np.diff(rp).max()) == 70000
    bad = _case(dev, T, ext, ("rows+hub G=%d" % G, which, D, act), rp, col, which, D, act)
    assert not bad, "\n  ".join(bad)
    T.clear_plan_cache()
    ext.clear_plan_cache()


# ---- edge_sum through perm ------------------------------------------------------------------------------------------------------------

def _perm_graphs():
    return {"rows G=4 transposed": row_length_graph(4, True), "powerlaw_n3000_directed": graphs.powerlaw_graph(3000, 12, seed=31, symmetric=False)}


@pytest.mark.parametrize("name", ["rows G=4 transposed", "powerlaw_n3000_directed"])
@pytest.mark.parametrize("D", [16, 65])
def test_edge_sum_through_perm_over_the_transposed_graph(dev, T, ext, name, D):
    """M in A's order summed by SOURCE node: the rows of A^T, every position through perm.  On the row-length graph's transpose every
    node is named a few hundred times; the C call runs over the host's transposed CSR with NO_ROW uncovered perm entries that name a
    poisoned row of M, the modules over their own device transpose."""
    import tcgnn_capi as C
    rp, col = _perm_graphs()[name]
    rp = np.ascontiguousarray(rp, dtype=np.int32)
    n, E = len(rp) - 1, int(rp[-1])
    rp_t, col_t, perm = (np.ascontiguousarray(a, dtype=np.int32) for a in W.transposed_csr(rp, col[:E]))
    trp, tcol, trp_t = _dev(dev, rp), _dev(dev, col[:E]), _dev(dev, rp_t)
    permp = np.full(E + NO_ROW, E, dtype=np.int32)        # the uncovered entries name row E of M: the poisoned one
    permp[:E] = perm
    tperm = _dev(dev, permp)
    stream = torch.cuda.current_stream().cuda_stream
    bad, figs = [], []
    for which in ("integer", "normal", "large"):
        _, M, _ = R.input_set(which, n, E, D, seed=D + 1)
        Mp = np.full((E + NO_ROW, D), POISON, dtype=np.float32)
        Mp[:E] = M
        tM = _dev(dev, Mp)
        Yr, S, A = R.edge_sum(rp_t, perm, M)
        outs = []
        for _ in range(2):
            buf, y = _guarded(dev, n * D)
            assert C.lib.tcgnn_edge_sum(trp_t.data_ptr(), tperm.data_ptr(), n, E + NO_ROW, tM.data_ptr(), D, y.data_ptr(), stream) == 0, C.lib.tcgnn_last_error()
            outs.append(buf)
        Y = outs[0][:n * D].view(n, D)
        what = "%s D=%d %s edge_sum(perm)" % (name, D, which)
        _held(what, Y, Yr, S, A, which == "integer", bad, figs)
        if not torch.equal(_bits(outs[0]), _bits(outs[1])):
            bad.append(what + ": the second call returns other bits")
        if not bool((outs[0][n * D:] == SENTINEL).all()):
            bad.append(what + ": guard words written")
        for mod, label in ((T, "TCGNN"), (ext, "the pybind module")):
            d_rp_t, _, d_perm, _ = mod.transpose_graph(trp, tcol)
            if not torch.equal(_bits(mod.edge_sum(tM[:E].contiguous(), d_rp_t, d_perm)), _bits(Y)):
                bad.append("%s: %s over its own transpose differs from the C call" % (what, label))
    torch.cuda.synchronize()
    for w, whole, excess in figs:
        print("FIG edge_message %-52s %.3f of the bound, %.3e of the summation's allowance beyond the result's own rounding" % (w, whole, excess))
    assert not bad, "\n  ".join(bad)
    T.clear_plan_cache()
    ext.clear_plan_cache()


# ---- memory ---------------------------------------------------------------------------------------------------------------------------

def _off16(dev, a):
    """a copy of `a` whose first element sits one float behind a 16-byte boundary"""
    store = torch.zeros(a.numel() + 1, dtype=torch.float32, device=dev)
    v = store[1:].view(a.shape)
    v.copy_(a)
    assert v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("D", [64, 260])
def test_operands_one_float_off_sixteen_bytes_give_the_same_bits(dev, T, D):
    """the 16-byte form (every operand aligned) against the dword form, which one misaligned operand is enough to select"""
    rp, col = row_length_graph(group_lanes(D), False)
    n, E = len(rp) - 1, int(rp[-1])
    X, Ef, dY = (_dev(dev, a) for a in R.input_set("normal", n, E, D, seed=3))
    trp, tcol = _dev(dev, rp), _dev(dev, col)
    Y, dM = T.forward_ue(X, Ef, trp, tcol), T.backward_ue(dY, X, Ef, trp, tcol)
    Ys = T.edge_sum(dM, trp)
    assert all(t.data_ptr() % 16 == 0 for t in (X, Ef, dY, Y, dM))
    Xo, Efo, dYo, dMo = (_off16(dev, t) for t in (X, Ef, dY, dM))
    for x, f in ((Xo, Ef), (X, Efo), (Xo, Efo)):
        assert torch.equal(_bits(T.forward_ue(x, f, trp, tcol)), _bits(Y))
    for g, x, f in ((dYo, X, Ef), (dY, Xo, Ef), (dY, X, Efo)):
        assert torch.equal(_bits(T.backward_ue(g, x, f, trp, tcol)), _bits(dM))
    out = _off16(dev, torch.zeros(E, D, device=dev))
    assert T.backward_ue(dY, X, Ef, trp, tcol, out=out).data_ptr() == out.data_ptr() and torch.equal(_bits(out), _bits(dM))
    assert torch.equal(_bits(T.backward_ue(dYo, None, None, trp, tcol, act=None, out=out)), _bits(dY[torch.from_numpy(R.edge_rows(rp)).to(dev)]))
    assert torch.equal(_bits(T.edge_sum(dMo, trp)), _bits(Ys))
    T.clear_plan_cache()


def test_out_is_written_in_place_and_refused_where_it_aliases_or_misfits(dev, T, ext):
    rp, col = graphs.uniform_graph(50, 4, seed=2)
    n, E, D = 50, len(col), 8
    trp, tcol = _dev(dev, rp), _dev(dev, col)
    X, Ef, dY = (_dev(dev, a) for a in R.input_set("normal", n, E, D, seed=1))
    for mod in (T, ext):
        Y, dM = mod.forward_ue(X, Ef, trp, tcol), mod.backward_ue(dY, X, Ef, trp, tcol)
        out = torch.empty_like(X)
        assert mod.forward_ue(X, Ef, trp, tcol, out=out).data_ptr() == out.data_ptr() and torch.equal(out, Y)
        outm = torch.empty_like(Ef)
        assert mod.backward_ue(dY, X, Ef, trp, tcol, out=outm).data_ptr() == outm.data_ptr() and torch.equal(outm, dM)
        assert mod.edge_sum(dM, trp, out=out).data_ptr() == out.data_ptr() and torch.equal(out, mod.edge_sum(dM, trp))
        Xc, Efc = X.clone(), Ef.clone()
        with pytest.raises(RuntimeError, match="share memory"):
            mod.forward_ue(Xc, Ef, trp, tcol, out=Xc)
        with pytest.raises(RuntimeError, match="share memory"):
            mod.backward_ue(dY, X, Efc, trp, tcol, out=Efc)
        assert torch.equal(Xc, X) and torch.equal(Efc, Ef)
        with pytest.raises(RuntimeError, match="out must be a contiguous fp32"):
            mod.forward_ue(X, Ef, trp, tcol, out=torch.empty(n, D + 1, device=dev))
        with pytest.raises(RuntimeError, match="out must be a contiguous fp32"):
            mod.edge_sum(dM, trp, out=torch.empty(n + 1, D, device=dev))
        with pytest.raises(RuntimeError, match="num_edges"):
            mod.forward_ue(X, Ef[:E - 1].contiguous(), trp, tcol)
        with pytest.raises(RuntimeError, match="num_nodes"):
            mod.forward_ue(X[:n - 1].contiguous(), Ef, trp, tcol)
        with pytest.raises(RuntimeError, match="Float"):
            mod.forward_ue(X.double(), Ef, trp, tcol)
        with pytest.raises(ValueError, match="act"):
            mod.forward_ue(X, Ef, trp, tcol, act="tanh")
    T.clear_plan_cache()
    ext.clear_plan_cache()


# ---- degenerate and refused calls ------------------------------------------------------------------------------------------------------

def test_degenerate_sizes_return_ok_and_zero_what_exists(dev, T):
    import tcgnn_capi as C
    stream = torch.cuda.current_stream().cuda_stream
    fwd, bwd, esum = C.lib.tcgnn_edge_message, C.lib.tcgnn_edge_message_backward, C.lib.tcgnn_edge_sum
    n, D = 37, 5
    rp0 = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    X = torch.randn(n, D, device=dev)
    zero = lambda v: bool((_bits(v) == 0).all())   # noqa: E731
    for call in (lambda y: fwd(rp0.data_ptr(), None, n, 0, X.data_ptr(), None, D, 1, y, stream), lambda y: esum(rp0.data_ptr(), None, n, 0, None, D, y, stream)):
        buf, y = _guarded(dev, n * D)                                                                      # E = 0: every row is empty
        assert call(y.data_ptr()) == 0 and zero(y) and bool((buf[n * D:] == SENTINEL).all())
    buf, m = _guarded(dev, 8)
    assert bwd(rp0.data_ptr(), None, n, 0, X.data_ptr(), None, X.data_ptr(), D, 1, m.data_ptr(), stream) == 0   # ... and dM has no element
    assert bool((buf == SENTINEL).all())
    buf, m = _guarded(dev, 6 * D)                                                                          # N = 0: no row covers dM's six rows
    assert bwd(rp0.data_ptr(), rp0.data_ptr(), 0, 6, X.data_ptr(), X.data_ptr(), X.data_ptr(), D, 1, m.data_ptr(), stream) == 0
    assert zero(m) and bool((buf[6 * D:] == SENTINEL).all())
    for nn, ee, dd in ((0, 0, D), (0, 5, D), (n, 7, 0)):                                                   # N = 0, D = 0: Y has no element
        buf, y = _guarded(dev, 8)
        assert fwd(rp0.data_ptr(), rp0.data_ptr(), nn, ee, X.data_ptr(), X.data_ptr(), dd, 1, y.data_ptr(), stream) == 0
        assert esum(rp0.data_ptr(), None, nn, ee, X.data_ptr(), dd, y.data_ptr(), stream) == 0
        if dd == 0:
            assert bwd(rp0.data_ptr(), rp0.data_ptr(), nn, ee, X.data_ptr(), X.data_ptr(), X.data_ptr(), dd, 1, y.data_ptr(), stream) == 0
        assert bool((buf == SENTINEL).all())
    # the module's calls at those sizes
    col0 = torch.zeros(0, dtype=torch.int32, device=dev)
    Ef0 = torch.zeros(0, D, device=dev)
    Y = T.forward_ue(X, Ef0, rp0, col0)
    assert Y.shape == (n, D) and not bool(Y.any())
    assert T.backward_ue(X, X, Ef0, rp0, col0).shape == (0, D)
    assert not bool(T.edge_sum(Ef0, rp0).any())
    assert T.forward_ue(torch.zeros(n, 0, device=dev), torch.zeros(0, 0, device=dev), rp0, col0).shape == (n, 0)
    # positions in front of the first row and behind the last belong to no row: dM is zero there, Y does not see them
    E = 100
    rp = torch.tensor([10, 30, 30, 90], dtype=torch.int32, device=dev)
    col = torch.arange(E, dtype=torch.int32, device=dev) % 3
    X3, Ef, dY3 = torch.rand(3, 8, device=dev) + 1, torch.rand(E, 8, device=dev), torch.randn(3, 8, device=dev)
    Ef[:10], Ef[90:] = POISON, POISON
    buf, m = _guarded(dev, E * 8)
    assert bwd(rp.data_ptr(), col.data_ptr(), 3, E, X3.data_ptr(), Ef.data_ptr(), dY3.data_ptr(), 8, 1, m.data_ptr(), stream) == 0
    m = m.view(E, 8)
    assert zero(m[:10]) and zero(m[90:]) and torch.equal(m[10:30], dY3[0].expand(20, 8)) and torch.equal(m[30:90], dY3[2].expand(60, 8))
    assert bool((buf[E * 8:] == SENTINEL).all())
    buf, y = _guarded(dev, 24)
    assert fwd(rp.data_ptr(), col.data_ptr(), 3, E, X3.data_ptr(), Ef.data_ptr(), 8, 1, y.data_ptr(), stream) == 0
    assert float(y.abs().max()) < 1e3 and zero(y.view(3, 8)[1]) and bool((buf[24:] == SENTINEL).all())
    # row pointers with a descending pair and an entry beyond the array, column ids out of range: clamped as the family clamps them
    wild = torch.tensor([0, 50, 40, 5000], dtype=torch.int32, device=dev)          # rows: [0, 50), empty, [40, 100)
    col[::7] = 1 << 30
    col[3::7] = -5
    Ef = torch.rand(E, 8, device=dev)
    buf, y = _guarded(dev, 24)
    assert fwd(wild.data_ptr(), col.data_ptr(), 3, E, X3.data_ptr(), Ef.data_ptr(), 8, 0, y.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    clamped = col.clamp(0, 2).cpu().numpy()
    Yr, S, A = R.edge_message(np.array([0, 50, 50, 50]), clamped, X3.cpu().numpy(), Ef.cpu().numpy(), "identity")
    assert R.share(y.view(3, 8)[:2].cpu().numpy(), S[:2], A[:2])[0] <= 1.0 and zero(y.view(3, 8)[1]) and bool((buf[24:] == SENTINEL).all())
    Yr, S, A = R.edge_message(np.array([40, 100]), clamped, X3.cpu().numpy(), Ef.cpu().numpy(), "identity")
    assert R.share(y.view(3, 8)[2:].cpu().numpy(), S, A)[0] <= 1.0


def test_invalid_arguments_are_refused_and_nothing_is_written(dev):
    import tcgnn_capi as C
    stream = torch.cuda.current_stream().cuda_stream
    n, E, D = 10, 30, 4
    rp = torch.arange(0, E + 1, 3, dtype=torch.int32, device=dev)
    col = torch.zeros(E, dtype=torch.int32, device=dev)
    X, Ef = torch.randn(n, D, device=dev), torch.randn(E, D, device=dev)
    ybuf, y = _guarded(dev, n * D)
    mbuf, m = _guarded(dev, E * D)
    p = lambda t: t.data_ptr()   # noqa: E731
    good = [p(rp), p(col), n, E, p(X), p(Ef), D, 1, p(y)]
    for at, value in ((2, -1), (3, -1), (3, 1 << 31), (6, -1), (7, 2), (7, -1), (0, None), (1, None), (4, None), (5, None), (8, None)):
        args = list(good)
        args[at] = value
        assert C.lib.tcgnn_edge_message(*args, stream) == INVALID_ARG, (at, value)
    good = [p(rp), p(col), n, E, p(X), p(Ef), p(X), D, 1, p(m)]
    for at, value in ((2, -1), (3, -1), (3, 1 << 31), (7, -1), (8, 5), (8, -1), (0, None), (1, None), (4, None), (5, None), (6, None), (9, None)):
        args = list(good)
        args[at] = value
        assert C.lib.tcgnn_edge_message_backward(*args, stream) == INVALID_ARG, (at, value)
    for at in (0, 6, 9):                                                           # the identity needs neither col, X nor Ef - the rest it does
        args = [p(rp), None, n, E, None, None, p(X), D, 0, p(m)]
        args[at] = None
        assert C.lib.tcgnn_edge_message_backward(*args, stream) == INVALID_ARG, at
    good = [p(rp), None, n, E, p(Ef), D, p(y)]
    for at, value in ((2, -1), (3, -1), (3, 1 << 31), (5, -1), (0, None), (4, None), (6, None)):
        args = list(good)
        args[at] = value
        assert C.lib.tcgnn_edge_sum(*args, stream) == INVALID_ARG, (at, value)
    torch.cuda.synchronize()
    assert bool((ybuf == SENTINEL).all()) and bool((mbuf == SENTINEL).all())
    assert C.lib.tcgnn_edge_message_backward(p(rp), None, n, E, None, None, p(X), D, 0, p(m), stream) == 0
    assert torch.equal(m.view(E, D), X.repeat_interleave(3, dim=0))


# ---- aggregate_ue and GINEConv against the fp64 model ---------------------------------------------------------------------------------

def _rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double()
    assert got.shape == want.shape
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)


def _layer_graph(name):
    if name == "layers_n200":
        f = np.load(os.path.join(ROOT, "tests", "golden", "layers_n200.npz"))
        return f["rowptr"].astype(np.int32), f["col"].astype(np.int32)
    rp, col = graphs.powerlaw_graph(3000, 12, seed=31, symmetric=False)
    assert not W.is_symmetric(rp, col) and (np.diff(rp) == 0).any()
    return rp, col


# Everything here is fp32 arithmetic - no fp16 image, no 10-bit operand: the message is one fp32 rounding (2^-24), the aggregation an
# fp64 sum rounded once (2^-24), the dense products torch's fp32 GEMMs over K <= 41 terms (K 2^-24 of sum |x w| at worst, and the
# largest entry is of the order of that sum).  An output is a chain of two or three such steps, a gradient of up to five, and the
# longest row multiplies a gradient's terms by a few hundred: 1e-5 of the largest entry for an output, 1e-4 for a gradient - the bounds
# of the max aggregation's layer tests (tests/test_gpu_segmax.py), which rest on the same arithmetic.
TOL_Y, TOL_G = R.TOL_Y, R.TOL_G


@pytest.mark.parametrize("name", ["layers_n200", "powerlaw_n3000_directed"])
@pytest.mark.parametrize("act", ["relu", "identity"])
def test_aggregate_ue_against_the_fp64_model(dev, T, name, act):
    import tcgnn_edge_ops as E
    rp, col = _layer_graph(name)
    n, ne, D = len(rp) - 1, len(col), 41
    B, Sel = R.incidence(rp, col, sparse=n > 1000)
    torch.manual_seed(1)
    X, Ef = torch.randn(n, D), torch.randn(ne, D)
    dY = torch.randn(n, D, dtype=torch.float64)
    Xg, Eg = X.to(dev).requires_grad_(True), Ef.to(dev).requires_grad_(True)
    Y = E.aggregate_ue(Xg, Eg, _dev(dev, rp), _dev(dev, col), act)
    Xd, Ed = X.double().requires_grad_(True), Ef.double().requires_grad_(True)
    want = R.dense_aggregate_ue(B, Sel, Xd, Ed, act)
    got = torch.autograd.grad((Y * dY.float().to(dev)).sum(), [Xg, Eg])
    ref = torch.autograd.grad((want * dY).sum(), [Xd, Ed])
    figs = [("Y", _rel(Y, want), TOL_Y)] + [(w, _rel(g, r), TOL_G) for g, r, w in zip(got, ref, ("dX", "dEf"))]
    for w, f, t in figs:
        print("FIG aggregate_ue %-24s %-8s %-4s %.3e of the largest entry (bound %.0e)" % (name, act, w, f, t))
    assert all(f <= t for _, f, t in figs), figs
    Mg = Ef.to(dev).requires_grad_(True)
    Ys = E.edge_sum(Mg, _dev(dev, rp), _dev(dev, col))
    Md = Ef.double().requires_grad_(True)
    assert _rel(Ys, B @ Md) <= TOL_Y
    assert _rel(torch.autograd.grad((Ys * dY.float().to(dev)).sum(), [Mg])[0], torch.autograd.grad(((B @ Md) * dY).sum(), [Md])[0]) <= TOL_G
    T.clear_plan_cache()


@pytest.mark.parametrize("name", ["layers_n200", "powerlaw_n3000_directed"])
@pytest.mark.parametrize("edge_dim", [None, 5], ids=["no_edge_dim", "edge_dim5"])
def test_gine_layer_against_the_fp64_model(dev, T, name, edge_dim):
    import tcgnn_layers as L
    rp, col = _layer_graph(name)
    n, ne = len(rp) - 1, len(col)
    B, Sel = R.incidence(rp, col, sparse=n > 1000)
    meta = _meta(dev, rp, col)
    torch.manual_seed(3)
    conv = L.GINEConv(24, 16, edge_dim=edge_dim, eps=0.25, train_eps=True)
    conv.bias.data.normal_()
    if edge_dim is not None:
        conv.bias_edge.data.normal_()
    X, EA = torch.randn(n, 24), torch.randn(ne, edge_dim or 24)
    dY = torch.randn(n, 16, dtype=torch.float64)
    pick = lambda c: [c.weights, c.bias, c.eps] + ([c.weights_edge, c.bias_edge] if edge_dim is not None else [])   # noqa: E731
    leaves = [t.detach().double().requires_grad_(True) for t in [X, EA] + pick(conv)]
    conv = conv.to(dev)
    Xg, EAg = X.to(dev).requires_grad_(True), EA.to(dev).requires_grad_(True)
    Y = conv(Xg, *meta, edge_attr=EAg)
    want = R.dense_gine(B, Sel, leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], *leaves[5:])
    got = torch.autograd.grad((Y * dY.float().to(dev)).sum(), [Xg, EAg] + pick(conv))
    ref = torch.autograd.grad((want * dY).sum(), leaves)
    figs = [("Y", _rel(Y, want), TOL_Y)] + [(w, _rel(g, r), TOL_G) for g, r, w in zip(got, ref, ("dX", "dedge_attr", "dW", "dbias", "deps", "dW_e", "db_e"))]
    for w, f, t in figs:
        print("FIG gine %-24s %-11s %-10s %.3e of the largest entry (bound %.0e)" % (name, "edge_dim=%s" % edge_dim, w, f, t))
    assert all(f <= t for _, f, t in figs), figs
    T.clear_plan_cache()


def test_layers_run_on_the_pybind_module_with_the_same_bits(dev, T, ext):
    import tcgnn_layers as L
    rp, col = _layer_graph("powerlaw_n3000_directed")
    n, ne = len(rp) - 1, len(col)
    meta = _meta(dev, rp, col)
    torch.manual_seed(5)
    conv = L.GINEConv(16, 8, edge_dim=4, train_eps=True).to(dev)
    X, EA = torch.randn(n, 16, device=dev).requires_grad_(True), torch.randn(ne, 4, device=dev).requires_grad_(True)

    def run():
        Y = conv(X, *meta, edge_attr=EA)
        return [Y.detach()] + list(torch.autograd.grad(Y.square().sum(), [X, EA] + list(conv.parameters())))
    mine = run()
    old = L._backend
    L.set_backend(ext)
    try:
        theirs = run()
    finally:
        L.set_backend(old)
        ext.clear_plan_cache()
    assert all(torch.equal(a, b) for a, b in zip(mine, theirs))
    T.clear_plan_cache()


# ---- a captured step, training ---------------------------------------------------------------------------------------------------------

def test_a_prepared_gine_step_replays_from_a_hip_graph_bit_equal(dev, T):
    import tcgnn_layers as L
    rp, col = graphs.community_graph(3000, 10, 20, 0.8, seed=4)
    n, ne = len(rp) - 1, len(col)
    meta = _meta(dev, rp, col)
    torch.manual_seed(2)
    convs = [L.GINEConv(32, 16, edge_dim=8, train_eps=True).to(dev), L.GINEConv(16, 6, edge_dim=8).to(dev)]
    params = [p for cv in convs for p in cv.parameters()]
    x = torch.randn(n, 32, device=dev).requires_grad_(True)
    ea = torch.randn(ne, 8, device=dev).requires_grad_(True)
    y = torch.randint(0, 6, (n,), device=dev)
    T.prepare([], *meta, max_aggregation=True)    # (the transposed CSR: all the planless calls need)

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


def test_ten_adam_steps_of_a_two_layer_gine_net_on_the_toy_dataset_lower_the_loss(dev, T, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tc-gnn_atc23_amd"))
    import tcgnn_graph as TG
    import tcgnn_harness as H
    import tcgnn_layers as L
    f = np.load(os.path.join(ROOT, "tests", "golden", "dataset_toy.npz"))
    np.savez(os.path.join(tmp_path, "toy.npz"), src_li=f["src_li"], dst_li=f["dst_li"], num_nodes=f["num_nodes"])
    ds = TG.TCGNN_dataset(os.path.join(tmp_path, "toy.npz"), 12, 5, load_from_txt=False, seed=0)
    rp, col = ds.row_pointers.numpy(), ds.column_index.numpy()
    meta = _meta(dev, rp, col)
    g = torch.Generator().manual_seed(1)
    y = torch.randint(0, 5, (ds.num_nodes,), generator=g)
    x = (torch.randn(ds.num_nodes, 12, generator=g) + torch.nn.functional.one_hot(y, 12).float()).to(dev)   # features that tell the label
    edge_attr = torch.randn(len(col), 6, generator=g).to(dev)
    y = y.to(dev)

    class Conv(L.GINEConv):
        def __init__(self, a, b):
            super().__init__(a, b, edge_dim=6, train_eps=True)

        def forward(self, X, *graph):
            return super().forward(X, *graph, edge_attr=edge_attr)

    torch.manual_seed(0)
    model = H.Net(Conv, 12, 16, 5, 2).to(dev)
    opt = H.make_adam(model.parameters())
    model.eval()                                                                                             # (no dropout: the same net every step)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = H.node_nll_loss(model(x, meta), y)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("FIG gine training loss %.4f -> %.4f" % (losses[0], losses[-1]))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    T.clear_plan_cache()
