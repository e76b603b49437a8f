"""Relabelled mini-batch blocks on the MI355X: tcgnn_compact_* against tests/compact_ref.py's numpy restatement (EVERY element of every
output, torch.equal, int32 asserted) on every size class of the mask scan and on sampled graphs of every row-length class, the
properties that need no reference, the memory contract and the refusals, malformed inputs, repetition, the pybind module against the
ctypes one, the existing operators and layers on a compact batch against the same batch uncompacted, and the harness's --batch-size."""
import glob
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import compact_ref as CR
import sample_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
SENTINEL = -12345
BAD_GRAPH, WORKSPACE = 4, 5   # TCGNN_ERR_BAD_GRAPH, TCGNN_ERR_WORKSPACE (include/tcgnn.h)
S, C = CR.SCAN_ROWS, CR.SUMS_PER_PASS


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


def _same(got, want, what):
    assert got.dtype == torch.int32, "%s is %s, not int32" % (what, got.dtype)
    assert torch.equal(got.cpu(), torch.from_numpy(np.ascontiguousarray(want))), "%s differs from the reference" % what


def _check_batch(T, dev, graphs, keep, what):
    """the module's calls on numpy graphs against the reference and the reference-free properties -> (nodes, new_id, blocks) on the device"""
    tg = [(_dev(dev, rp), _dev(dev, col)) for rp, col in graphs]
    tkeep = None if keep is None else _dev(dev, keep)
    before = None if keep is None else tkeep.clone()
    nodes, new_id = T.compact_nodes(tg, tkeep)
    assert keep is None or torch.equal(tkeep, before), "%s: compact_nodes wrote into keep" % what
    blocks = [T.compact_graph(rp, col, nodes, new_id) for rp, col in tg]
    want_nodes, want_id, want_blocks = CR.compact(graphs, keep)
    _same(nodes, want_nodes, what + ": nodes")
    _same(new_id, want_id, what + ": new_id")
    for i, ((rp_b, col_b), (wrp, wcol)) in enumerate(zip(blocks, want_blocks)):
        _same(rp_b, wrp, what + ": nodePointer_b of graph %d" % i)
        _same(col_b, wcol, what + ": edgeList_b of graph %d" % i)
    CR.check_properties(graphs, keep, nodes.cpu().numpy(), new_id.cpu().numpy(), [(a.cpu().numpy(), b.cpu().numpy()) for a, b in blocks])
    return nodes, new_id, blocks


# ---- the mask scan's size classes ----------------------------------------------------------------------------------------------------

SCAN_SIZES = (0, 1, 2, S - 1, S, S + 1, 3 * S + 7, S * C + 1)


def _keep_patterns(n):
    rng = np.random.default_rng(n + 17)
    z = np.zeros(n, np.uint8)
    out = [("none", z.copy()), ("all", np.ones(n, np.uint8))]
    if n:
        first, last, run = z.copy(), z.copy(), z.copy()
        first[0] = 1
        last[n - 1] = 1
        run[S - 4:S + 6] = 1   # (clipped to the array: empty below S - 4 nodes)
        out += [("node 0", first), ("node N - 1", last), ("every other", (np.arange(n) % 2).astype(np.uint8)), ("a run over a block boundary", run)]
    out += [("1 %", (rng.random(n) < 0.01).astype(np.uint8)), ("50 %", (rng.random(n) < 0.5).astype(np.uint8) * 255)]
    return out


@pytest.mark.parametrize("n", SCAN_SIZES, ids=["N%d" % n for n in SCAN_SIZES])
def test_every_size_class_of_the_mask_scan_under_every_keep_pattern(dev, T, n):
    """a graph without edges: the node set is the mask's, so the scan alone decides nodes and new_id"""
    g = [(np.zeros(n + 1, np.int32), np.zeros(0, np.int32))]
    for name, keep in _keep_patterns(n):
        nodes, new_id, blocks = _check_batch(T, dev, g, keep, "N = %d, %s" % (n, name))
        assert nodes.numel() == int((keep != 0).sum()) and blocks[0][0].tolist() == [0] * (nodes.numel() + 1)
    nodes, _, _ = _check_batch(T, dev, g, None, "N = %d, no mask" % n)
    assert nodes.numel() == 0
    # a mask that does not start on a dword boundary takes the byte loads: the same result
    if n:
        keep = _keep_patterns(n)[-1][1]
        padded = _dev(dev, np.concatenate([[9], keep]).astype(np.uint8))
        a = T.compact_nodes([(_dev(dev, g[0][0]), _dev(dev, g[0][1]))], padded[1:])
        assert padded[1:].data_ptr() % 4 == 1
        _same(a[0], CR.compact_nodes(g, keep)[0], "byte-aligned mask: nodes")
        _same(a[1], CR.compact_nodes(g, keep)[1], "byte-aligned mask: new_id")


# ---- graphs --------------------------------------------------------------------------------------------------------------------------

_SAMPLED = {}


def _sampled(dev, T, k, masked):
    """the covered part of sample_ref.row_length_graph() sampled on the device at fan-out k (the sampler has its own tests), as numpy"""
    if (k, masked) not in _SAMPLED:
        rp, col, _ = R.row_length_graph()
        n, E = len(rp) - 1, int(rp[-1])
        mask = (np.random.default_rng(5).random(n) < 0.3).astype(np.uint8) if masked else None
        g = T.sample_neighbors(_dev(dev, rp), _dev(dev, col[:E]), k, 7, None if mask is None else _dev(dev, mask))
        _SAMPLED[(k, masked)] = tuple(t.cpu().numpy() for t in g[:2])
    return _SAMPLED[(k, masked)]


@pytest.mark.parametrize("masked", [False, True], ids=["all-rows", "row-mask"])
@pytest.mark.parametrize("k", [0, 5, 25, 100000], ids=lambda k: "k%d" % k)
def test_one_sampled_graph_of_every_row_length_class(dev, T, k, masked):
    g = _sampled(dev, T, k, masked)
    seeds = np.zeros(len(g[0]) - 1, np.uint8)
    seeds[[0, 5, 2047]] = 1
    nodes, _, _ = _check_batch(T, dev, [g], seeds, "k = %d" % k)
    _check_batch(T, dev, [g], None, "k = %d, no seeds" % k)
    if k == 0:
        assert nodes.tolist() == [0, 5, 2047]
    if k == 100000 and not masked:
        assert len(g[1]) == R.row_length_graph()[0][-1] and np.diff(g[0]).max() == R.LONG_ROW


def test_two_layer_graphs_marked_into_one_mask_and_a_graph_without_edges(dev, T):
    g0, g1 = _sampled(dev, T, 25, False), _sampled(dev, T, 5, True)
    n = len(g0[0]) - 1
    seeds = np.zeros(n, np.uint8)
    seeds[np.random.default_rng(2).integers(0, n, 20)] = 1
    both, _, _ = _check_batch(T, dev, [g0, g1], seeds, "two graphs")
    one, _, _ = _check_batch(T, dev, [g1], seeds, "the smaller graph alone")
    assert one.numel() < both.numel(), "the second graph adds no node: the case checks nothing"
    empty = (np.zeros(n + 1, np.int32), np.zeros(0, np.int32))
    _check_batch(T, dev, [empty, g1], seeds, "a graph without edges beside one with")
    _check_batch(T, dev, [empty], None, "nothing at all")
    # the layered case through tcgnn_layers: sample_layers -> compact_layers
    import tcgnn_layers as L
    rp, col, _ = R.row_length_graph()
    trp, tcol = _dev(dev, rp), _dev(dev, col[:int(rp[-1])])
    tseeds = torch.tensor([3, 77, 1500, 2047], device=dev)
    layers = L.sample_layers((trp, tcol), tseeds, [6, 4], 21)
    batch = L.compact_layers(layers, tseeds, plan=False)
    gs = [(a.cpu().numpy(), b.cpu().numpy()) for a, b, _ in layers]
    keep = np.zeros(n, np.uint8)
    keep[[3, 77, 1500, 2047]] = 1
    want_nodes, want_id, want_blocks = CR.compact(gs, keep)
    _same(batch.nodes, want_nodes, "compact_layers: nodes")
    assert batch.seed_pos.dtype == torch.int64 and batch.seed_pos.tolist() == want_id[[3, 77, 1500, 2047]].tolist()
    assert np.array_equal(want_nodes, np.unique(np.concatenate([[3, 77, 1500, 2047], gs[0][1], gs[1][1]]))), "the kept set is not seeds + sources"
    for m, (wrp, wcol), (_, _, eid), be in zip(batch.metas, want_blocks, layers, batch.eids):
        _same(m[0], wrp, "compact_layers: row pointers")
        _same(m[1], wcol, "compact_layers: columns")
        assert all(t.numel() == 0 for t in m[2:]) and be is eid
    planned = L.sample_batch((trp, tcol), tseeds, [6, 4], 21, plan=True)
    assert torch.equal(planned.nodes, batch.nodes) and torch.equal(planned.seed_pos, batch.seed_pos)
    for m, p in zip(batch.metas, planned.metas):
        assert torch.equal(m[0], p[0]) and torch.equal(m[1], p[1]) and p[2].numel() == (batch.nodes.numel() + 15) // 16 and p[3].numel() == m[1].numel()
    T.clear_plan_cache()


# ---- memory contract -----------------------------------------------------------------------------------------------------------------

def _guarded(dev, n, shift=0):
    """(buffer, view of n entries `shift` entries into it, with GUARD sentinel entries behind)"""
    buf = torch.full((shift + n + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    return buf, buf[shift:shift + n]


def _intact(buf, n, shift=0):
    return bool((buf[:shift] == SENTINEL).all()) and bool((buf[shift + n:] == SENTINEL).all())


def _raw_batch(dev, graphs, keep, expect=0, ws_shift=0, ws_short=0, shift=0, ws=None):
    """One mini-batch through the C calls on guarded outputs of exactly the stated sizes and a workspace of exactly the queried size.
    graphs: numpy (rp, col) pairs; shift: every int32 array starts `shift` entries off its allocation (off sixteen bytes for 1 .. 3).
    expect: the count call's status.  -> (nodes, new_id, blocks) as numpy on success, else None"""
    import tcgnn_capi as Cc
    stream = torch.cuda.current_stream().cuda_stream
    n = len(graphs[0][0]) - 1
    need = Cc._sz(0)
    assert Cc.lib.tcgnn_compact_workspace_bytes(n, Cc.ctypes.byref(need)) == 0
    if ws is None:
        ws = torch.full((need.value + 1024,), 0x5A, dtype=torch.uint8, device=dev)
    base_off = (-ws.data_ptr()) % 256 + 256
    base = ws.data_ptr() + base_off

    def ws_guards_intact():
        return bool((ws[:base_off] == 0x5A).all()) and bool((ws[base_off + need.value:] == 0x5A).all())

    tg = []
    for rp, col in graphs:
        rbuf = torch.zeros(shift + len(rp), dtype=torch.int32, device=dev)
        cbuf = torch.zeros(shift + len(col), dtype=torch.int32, device=dev)
        rbuf[shift:] = _dev(dev, rp)
        cbuf[shift:] = _dev(dev, col)
        tg.append((rbuf[shift:], cbuf[shift:]))
    tkeep = torch.zeros(n, dtype=torch.uint8, device=dev) if keep is None else _dev(dev, keep).clone()
    ibuf, new_id = _guarded(dev, n, shift)
    wsp, wsn = base + ws_shift, need.value - ws_short
    st = Cc.lib.tcgnn_compact_begin(n, wsp, wsn, stream)
    if ws_shift or ws_short:
        kept = Cc._i32(-7)
        sts = [st] + [Cc.lib.tcgnn_compact_mark(rp.data_ptr(), col.data_ptr(), n, col.numel(), tkeep.data_ptr(), wsp, wsn, stream) for rp, col in tg]
        sts.append(Cc.lib.tcgnn_compact_count(tkeep.data_ptr(), n, new_id.data_ptr(), wsp, wsn, Cc.ctypes.byref(kept), stream))
        torch.cuda.synchronize()
        assert all(s == WORKSPACE for s in sts), sts
        assert kept.value == -7 and bool((ibuf == SENTINEL).all()) and bool((ws == 0x5A).all()), "a refused call wrote something"
        assert keep is None and not bool(tkeep.any()), "a refused mark call wrote into the mask"
        return None
    assert st == 0, Cc.lib.tcgnn_last_error()
    for rp, col in tg:
        assert Cc.lib.tcgnn_compact_mark(rp.data_ptr(), col.data_ptr(), n, col.numel(), tkeep.data_ptr(), wsp, wsn, stream) == 0, Cc.lib.tcgnn_last_error()
    kept = Cc._i32(-7)
    st = Cc.lib.tcgnn_compact_count(tkeep.data_ptr(), n, new_id.data_ptr(), wsp, wsn, Cc.ctypes.byref(kept), stream)
    torch.cuda.synchronize()
    assert st == expect, (st, Cc.lib.tcgnn_last_error())
    assert _intact(ibuf, n, shift), "the count call wrote outside new_id"
    assert ws_guards_intact(), "a call wrote outside the workspace"
    if st != 0:
        assert kept.value == -7
        return None
    m = kept.value
    assert not bool((new_id == SENTINEL).any()), "an entry of new_id was not written"
    nbuf, nodes = _guarded(dev, m, shift)
    assert Cc.lib.tcgnn_compact_nodes(new_id.data_ptr(), n, m, nodes.data_ptr(), stream) == 0, Cc.lib.tcgnn_last_error()
    blocks = []
    for rp, col in tg:
        pbuf, rp_b = _guarded(dev, m + 1, shift)
        cbuf, col_b = _guarded(dev, col.numel(), shift)
        st = Cc.lib.tcgnn_compact_graph(rp.data_ptr(), col.data_ptr(), new_id.data_ptr(), nodes.data_ptr(), n, m, col.numel(), rp_b.data_ptr(),
                                        col_b.data_ptr(), stream)
        torch.cuda.synchronize()
        assert st == 0, Cc.lib.tcgnn_last_error()
        assert _intact(pbuf, m + 1, shift) and _intact(cbuf, col.numel(), shift), "compact_graph wrote outside its outputs"
        assert not bool((rp_b == SENTINEL).any()) and not bool((col_b == SENTINEL).any()), "an output entry was not written"
        blocks.append((rp_b.cpu().numpy(), col_b.cpu().numpy()))
    assert _intact(nbuf, m, shift) and not bool((nodes == SENTINEL).any()), "compact_nodes wrote outside nodes or left an entry"
    assert ws_guards_intact()
    return nodes.cpu().numpy(), new_id.cpu().numpy(), blocks


def _equal_ref(got, graphs, keep, what):
    want = CR.compact(graphs, keep)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
    for (a, b), (wa, wb) in zip(got[2], want[2]):
        assert np.array_equal(a, wa) and np.array_equal(b, wb), what
        assert a.dtype == np.int32 and b.dtype == np.int32


@pytest.mark.parametrize("shift", [0, 1, 3], ids=["aligned", "off4", "off12"])
def test_outputs_of_exactly_the_stated_sizes_behind_sentinels(dev, T, shift):
    """shift 1 and 3: every int32 array starts off sixteen bytes, so the kernels take their dword forms - the same outputs"""
    g0, g1 = _sampled(dev, T, 25, False), _sampled(dev, T, 5, True)
    n = len(g0[0]) - 1
    seeds = np.zeros(n, np.uint8)
    seeds[[1, 2, 1024, 2047]] = 1
    _equal_ref(_raw_batch(dev, [g0, g1], seeds, shift=shift), [g0, g1], seeds, "two graphs, shift %d" % shift)
    _equal_ref(_raw_batch(dev, [g1], None, shift=shift), [g1], None, "one graph, no seeds, shift %d" % shift)
    empty = [(np.zeros(n + 1, np.int32), np.zeros(0, np.int32))]
    _equal_ref(_raw_batch(dev, empty, seeds, shift=shift), empty, seeds, "E = 0, shift %d" % shift)
    nothing = [(np.zeros(1, np.int32), np.zeros(0, np.int32))]
    _equal_ref(_raw_batch(dev, nothing, None, shift=shift), nothing, None, "N = 0, shift %d" % shift)


def test_workspaces_that_are_too_small_or_misaligned_are_refused_with_nothing_written(dev, T):
    g = _sampled(dev, T, 5, True)
    for kw in ({"ws_short": 1}, {"ws_shift": 128}, {"ws_shift": 4}):
        assert _raw_batch(dev, [g], None, **kw) is None


def test_malformed_inputs_are_reported_by_the_count_call_and_nothing_is_written_out_of_bounds(dev, T):
    rp, col = _sampled(dev, T, 5, True)
    n, E = len(rp) - 1, len(col)
    assert E > 100

    def with_col(value):
        c = col.copy()
        c[E // 2] = value
        return rp, c

    i = int(np.argmax(np.diff(rp)))
    descending = rp.copy()
    descending[i], descending[i + 1] = descending[i + 1], descending[i]
    short = rp.copy()
    short[-1] -= 1
    cases = (("a column id = N", with_col(n)), ("a column id = -1", with_col(-1)), ("a non-monotone nodePointer", (descending, col)),
             ("nodePointer[N] != E", (short, col)))
    import tcgnn_capi as Cc
    need = Cc._sz(0)
    assert Cc.lib.tcgnn_compact_workspace_bytes(n, Cc.ctypes.byref(need)) == 0
    ws = torch.full((need.value + 1024,), 0x5A, dtype=torch.uint8, device=dev)
    for name, g in cases:
        assert _raw_batch(dev, [g], None, expect=BAD_GRAPH, ws=ws) is None, name
        assert _raw_batch(dev, [(rp, col), g], None, expect=BAD_GRAPH, ws=ws) is None, name + " in the second graph"
        # the count call left the validation word clear: a good batch on the same workspace passes
        _equal_ref(_raw_batch(dev, [(rp, col)], None, ws=ws), [(rp, col)], None, "a good batch behind " + name)
    trp, tcol = _dev(dev, rp), _dev(dev, with_col(n)[1])
    with pytest.raises(RuntimeError, match="bad graph|BAD_GRAPH|column id"):
        T.compact_nodes([(trp, tcol)])


def test_compact_graph_with_a_new_id_that_never_saw_the_graph_stays_in_bounds(dev, T):
    """unspecified-but-safe: ids without a new id become 0, out-of-range ids are not followed, every output entry is written"""
    rp, col = _sampled(dev, T, 25, False)
    n = len(rp) - 1
    trp, tcol = _dev(dev, rp), _dev(dev, col)
    nodes, new_id = T.compact_nodes([(torch.zeros(n + 1, dtype=torch.int32, device=dev), tcol[:0])], _dev(dev, (np.arange(n) % 3 == 0).astype(np.uint8)))
    wild = tcol.clone()
    wild[::7] = 2 ** 31 - 1
    wild[3::7] = -5
    rp_b, col_b = T.compact_graph(trp, wild, nodes, new_id)
    torch.cuda.synchronize()
    want = np.where((wild.cpu().numpy() >= 0) & (wild.cpu().numpy() < n), new_id.cpu().numpy()[np.clip(wild.cpu().numpy(), 0, n - 1)], -1)
    _same(col_b, np.maximum(want, 0).astype(np.int32), "edgeList_b under a foreign new_id")
    _same(rp_b, np.concatenate([rp[nodes.cpu().numpy()], [len(col)]]).astype(np.int32), "nodePointer_b under a foreign new_id")


def test_module_argument_checks(dev, T, ext):
    rp, col = (_dev(dev, a) for a in _sampled(dev, T, 5, True))
    n = rp.numel() - 1
    nodes, new_id = T.compact_nodes([(rp, col)])
    for mod in (T, ext):
        with pytest.raises((RuntimeError, ValueError, TypeError)):
            mod.compact_nodes([])
        with pytest.raises((RuntimeError, TypeError)):
            mod.compact_nodes([(rp.long(), col)])
        with pytest.raises((RuntimeError, TypeError)):
            mod.compact_nodes([(rp.cpu(), col.cpu())])
        with pytest.raises(RuntimeError):
            mod.compact_nodes([(rp, col), (rp[:-1].contiguous(), col)])
        with pytest.raises(RuntimeError):
            mod.compact_nodes([(rp, col)], torch.ones(n - 1, dtype=torch.uint8, device=dev))
        with pytest.raises(RuntimeError):
            mod.compact_nodes([(rp, col)], torch.ones(n, dtype=torch.int32, device=dev))
        with pytest.raises(RuntimeError):
            mod.compact_graph(rp, col, nodes, new_id[:-1].contiguous())
        with pytest.raises(RuntimeError):
            mod.compact_graph(rp, col, nodes.long(), new_id)
        with pytest.raises(RuntimeError):
            mod.compact_graph(rp, col[::2], nodes, new_id)


def test_ten_repetitions_are_bit_identical_and_the_pybind_module_equals_the_ctypes_one(dev, T, ext):
    g0, g1 = _sampled(dev, T, 25, False), _sampled(dev, T, 5, True)
    tg = [(_dev(dev, a), _dev(dev, b)) for a, b in (g0, g1)]
    n = len(g0[0]) - 1
    keep = _dev(dev, (np.random.default_rng(8).random(n) < 0.05).astype(np.uint8))

    def run(mod, k):
        nodes, new_id = mod.compact_nodes(tg, k)
        return [nodes, new_id] + [t for rp, col in tg for t in mod.compact_graph(rp, col, nodes, new_id)]

    first = run(T, keep)
    for _ in range(9):
        assert all(torch.equal(a, b) for a, b in zip(first, run(T, keep)))
    for k in (keep, keep.bool(), None):
        a, b = run(T, k), run(ext, k)
        assert all(torch.equal(x, y) and x.dtype == y.dtype == torch.int32 for x, y in zip(a, b)), "the pybind module differs"


# ---- the existing operators on a compact batch -----------------------------------------------------------------------------------------

_BATCH = []


def _sbm_batch(dev):
    """a 3 000-node seeded SBM, 64 seeds, fan-outs (5, 3): the layer graphs uncompacted and compact, computed once and left unchanged"""
    if not _BATCH:
        import graphs
        import tcgnn_layers as L
        rp, col = graphs.community_graph(3000, 10, 20, 0.8, seed=4)
        trp, tcol = _dev(dev, rp.astype(np.int32)), _dev(dev, col.astype(np.int32))
        seeds = torch.from_numpy(np.sort(np.random.default_rng(1).choice(3000, 64, replace=False))).to(dev)
        layers = L.sample_layers((trp, tcol), seeds, [5, 3], 13)
        batch = L.compact_layers(layers, seeds, plan=False)
        _BATCH.append((trp, tcol, seeds, layers, batch))
    return _BATCH[0]


@pytest.mark.parametrize("D", [16, 64])
def test_existing_operators_give_the_uncompacted_rows_exactly(dev, T, D):
    """The monotone relabelling keeps every row's edges in their order and X[nodes] holds the same numbers, so each operator does the
    same arithmetic per row: torch.equal.  Rows outside `nodes` have no edges: the uncompacted result is zero there."""
    trp, tcol, seeds, layers, batch = _sbm_batch(dev)
    n, nodes = trp.numel() - 1, batch.nodes.long()
    rng = np.random.default_rng(D)
    X = _dev(dev, rng.integers(-8, 9, (n, D)).astype(np.float32))
    Ef_full = _dev(dev, rng.integers(-8, 9, (tcol.numel(), D)).astype(np.float32))
    Xb = X[nodes].contiguous()
    outside = torch.ones(n, dtype=torch.bool, device=dev)
    outside[nodes] = False
    assert 64 < nodes.numel() < n // 2 and bool(outside.any())
    for (rp_s, col_s, eid), meta_b in zip(layers, batch.metas):
        rp_b, col_b = meta_b[0], meta_b[1]
        assert col_b.numel() == col_s.numel() > 0

        def same_rows(full, compact, what):
            assert torch.equal(compact, full[nodes]), "%s: the compact rows differ from rows `nodes` of the uncompacted result" % what
            assert not bool(full[outside].any()), "%s: an uncompacted row outside `nodes` is not zero" % what

        Y, arg = T.forward_max(X, rp_s, col_s)
        Yb, argb = T.forward_max(Xb, rp_b, col_b)
        same_rows(Y, Yb, "forward_max")
        assert torch.equal(argb, arg[nodes]), "forward_max: arg (a CSR position: unchanged by the relabelling)"
        assert bool((arg[outside] == -1).all())
        st, stb = T.forward_stats(X, rp_s, col_s), T.forward_stats(Xb, rp_b, col_b)
        for name in ("mean", "std", "max", "min"):
            same_rows(st[name], stb[name], "forward_stats " + name)
        Ef = Ef_full[eid.long()].contiguous()
        same_rows(T.forward_ue(X, Ef, rp_s, col_s, act="relu"), T.forward_ue(Xb, Ef, rp_b, col_b, act="relu"), "forward_ue")
        dY = _dev(dev, rng.integers(-8, 9, (n, D)).astype(np.float32))
        same_rows(T.backward_max(dY * (~outside).unsqueeze(1), arg, rp_s, col_s), T.backward_max(dY[nodes].contiguous(), argb, rp_b, col_b), "backward_max")
        same_rows(T.edge_sum(Ef, rp_s), T.edge_sum(Ef, rp_b), "edge_sum")
    T.clear_plan_cache()


def test_the_plan_based_spmm_on_a_compact_graph_against_the_oracle(dev, T):
    """forward through compact_layers(plan=True) against the whole-product oracle, with the bound tests/test_gpu_sample.py applies to
    forward on a sampled graph: 1e-3 of max(1, |ref|)"""
    import graphs
    import tcgnn_layers as L
    from oracle import oracle as O
    trp, tcol, seeds, layers, batch = _sbm_batch(dev)
    planned = L.compact_layers(layers, seeds, plan=True)
    rng = np.random.default_rng(3)
    X = rng.integers(-8, 9, (trp.numel() - 1, 64)).astype(np.float32)
    Xb = X[planned.nodes.cpu().numpy()]
    for meta in planned.metas:
        rp_b, col_b = meta[0].cpu().numpy(), meta[1].cpu().numpy()
        bp, e2c, e2r, _ = graphs.host_sgt(rp_b, col_b)
        assert all(torch.equal(t.cpu(), torch.from_numpy(np.ascontiguousarray(w))) for t, w in zip(meta[2:], (bp, e2c, e2r))), "compact_layers' metadata"
        Y = T.forward(_dev(dev, Xb), *meta)[0]
        ref = O.spmm(Xb, rp_b, col_b, bp, e2c, e2r)
        assert np.max(np.abs(Y.cpu().numpy() - ref) / np.maximum(1.0, np.abs(ref))) <= 1e-3
    T.clear_plan_cache()


# ---- layers ----------------------------------------------------------------------------------------------------------------------------

def _integer_(p, lo, hi, gen):
    p.data.copy_(torch.randint(lo, hi + 1, p.shape, generator=gen).to(p.dtype))


def _run_stack(convs, X, metas, rows):
    """layer by layer, eval mode, ReLU between, no log_softmax -> (out[rows], the weight gradients of out[rows].sum(), every layer's input)"""
    for c in convs:
        c.zero_grad()
    h, inputs = X, []
    for i, (c, m) in enumerate(zip(convs, metas)):
        inputs.append(h.detach())
        h = c(h, *m)
        if i + 1 < len(convs):
            h = torch.relu(h)
    out = h[rows]
    out.sum().backward()
    return out.detach(), [p.grad.clone() for c in convs for p in c.parameters()], inputs


def _pad(g, dev):
    return (g[0], g[1]) + tuple(torch.empty(0, dtype=torch.int32, device=dev) for _ in range(3))


def test_a_two_layer_sage_max_stack_is_exact_on_the_compact_batch(dev, T):
    """Weights from {-1, 0, 1}, features from {-2 .. 2}: every partial sum of every product is an integer below 2^24 (asserted on an fp64
    evaluation of the bound below), so fp32 sums are exact in any order and the outputs at seed_pos on the compact batch must
    torch.equal the outputs at the seeds on the uncompacted layer graphs; so must the weight gradients of out[seeds].sum()."""
    import tcgnn_layers as L
    trp, tcol, seeds, layers, batch = _sbm_batch(dev)
    gen = torch.Generator().manual_seed(5)
    convs = [L.SAGEConv(16, 8, aggregator="max", directed=True), L.SAGEConv(8, 4, aggregator="max", directed=True)]
    for c in convs:
        for p in c.parameters():
            _integer_(p, -1, 1, gen)
        c.to(dev).eval()
    X = torch.randint(-2, 3, (trp.numel() - 1, 16), generator=gen).float().to(dev)
    out, grads, inputs = _run_stack(convs, X, [_pad(g, dev) for g in layers], seeds)
    out_b, grads_b, _ = _run_stack(convs, X[batch.nodes.long()].contiguous(), batch.metas, batch.seed_pos)
    # the bound, in fp64: |h| <= max|h|, so a partial sum of h W_self + max(h) W_neigh + b stays within max|h| (|W_self| + |W_neigh|) column sums + |b|
    for c, h in zip(convs, inputs):
        assert torch.equal(h, h.round()), "a layer input is not integer-valued"
        bound = h.abs().double().max() * (c.weights.detach().abs().double().sum(0) + c.weights_self.detach().abs().double().sum(0)).max() + 1
        assert float(bound) < 2 ** 24
    # the gradients: the last layer's upstream gradient is 1 on the 64 seed rows, so its weight gradients sum at most 64 input entries;
    # the first layer's upstream gradient sums a +-1 weight per output (4) for the row itself and for every edge of the last layer
    # graph that chose it - at most (64 + E_last) * 4 - and its weight gradients sum that times an input entry over at most N rows
    g_first = (64 + layers[1][1].numel()) * 4
    assert 64 * float(inputs[1].abs().double().max()) < 2 ** 24 and X.shape[0] * float(inputs[0].abs().double().max()) * g_first < 2 ** 24
    assert torch.equal(out, out.round()) and all(float(g.abs().double().max()) < 2 ** 24 and torch.equal(g, g.round()) for g in grads)
    assert bool(out.any()) and any(bool(g.any()) for g in grads), "all zeros: the case checks nothing"
    assert torch.equal(out_b, out), "SAGE-max outputs at seed_pos differ from the uncompacted outputs at the seeds"
    for g, gb in zip(grads, grads_b):
        assert torch.equal(gb, g), "a SAGE-max weight gradient differs"
    T.clear_plan_cache()


def test_a_two_layer_pna_stack_on_the_compact_batch(dev, T):
    """PNA's std (a square root) and its log-degree scalers make integer arithmetic impossible, and the dense products run over M rows
    on the compact batch and N on the uncompacted graphs (the BLAS may order the sums differently), so this is not bit-exact: the bounds
    are those tests/test_gpu_segstats.py applies to the PNA layer - 1e-5 of the largest entry for the output, 1e-4 for the gradients.
    delta is fixed: pna_delta of a graph depends on its node count."""
    import tcgnn_layers as L
    trp, tcol, seeds, layers, batch = _sbm_batch(dev)
    gen = torch.Generator().manual_seed(6)
    convs = [L.PNAConv(16, 8, delta=1.0), L.PNAConv(8, 4, delta=1.0)]
    for c in convs:
        for p in c.parameters():
            _integer_(p, -1, 1, gen)
        c.to(dev).eval()
    X = torch.randint(-2, 3, (trp.numel() - 1, 16), generator=gen).float().to(dev)
    out, grads, _ = _run_stack(convs, X, [_pad(g, dev) for g in layers], seeds)
    out_b, grads_b, _ = _run_stack(convs, X[batch.nodes.long()].contiguous(), batch.metas, batch.seed_pos)

    def rel(a, b):
        return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp(min=1e-30))

    figs = [("out", rel(out_b, out), 1e-5)] + [("grad %d" % i, rel(gb, g), 1e-4) for i, (g, gb) in enumerate(zip(grads, grads_b))]
    for w, f, t in figs:
        print("FIG pna compact vs uncompacted %-7s %.3e of the largest entry (bound %.0e)" % (w, f, t))
    assert bool(out.any()) and all(bool(g.any()) for g in grads)
    assert all(f <= t for _, f, t in figs), figs
    T.clear_plan_cache()


# ---- harness ---------------------------------------------------------------------------------------------------------------------------

def _harness_args(seen, **kw):
    import tcgnn_harness as H
    args = H.build_parser().parse_args(["--synthetic", "citeseer", "--dim", "16", "--hidden", "16", "--classes", "4", "--epochs", "2", "--model", "sage",
                                        "--aggregator", "max", "--gpu_preprocess", "--fanout", "5,5", "--batch-size", "64"])
    args.batch_hook = lambda epoch, index, seeds: seen.append((epoch, index, seeds.cpu()))
    for k, v in kw.items():
        setattr(args, k, v)
    return args


@pytest.mark.parametrize("model", ["sage", "gcn"])
def test_harness_trains_on_mini_batches_and_reproduces(dev, T, model):
    import tcgnn_harness as H
    kw = {} if model == "sage" else {"model": "gcn", "aggregator": "mean"}
    T.clear_plan_cache()
    T.set_plan_cache_size(4)
    within = []
    try:
        seen = []
        args = _harness_args(seen, **kw)
        hook = args.batch_hook

        def watching(epoch, index, seeds):
            hook(epoch, index, seeds)
            s = T.cache_stats()
            within.append(s["plans"] <= 4 and s["csrs"] <= 8)

        args.batch_hook = watching
        r = H.run(args, quiet=True)
        s = T.cache_stats()
        assert all(within) and s["plans"] <= 4 and s["csrs"] <= 8, s
        n = r["num_nodes"]
        assert r["batches"] == math.ceil(n / 64) and r["batch_size"] == 64 and r["fanout"] == [5, 5]
        assert all(np.isfinite(r[k]) and r[k] >= 0 for k in ("sample_ms", "compact_ms", "plan_ms", "train_ms", "epoch_ms"))
        assert abs(r["epoch_ms"] - (r["sample_ms"] + r["compact_ms"] + r["plan_ms"] + r["train_ms"])) <= 1e-6 * r["epoch_ms"]
        assert np.isfinite(r["final_loss"]) and np.isfinite(r["sampled_loss"])
        assert 64 <= r["mean_block_nodes"] <= n
        assert len(seen) == 2 * r["batches"]
        for epoch in (0, 1):
            ids = torch.cat([sd for e, _, sd in seen if e == epoch])
            assert torch.equal(torch.sort(ids).values, torch.arange(n)), "epoch %d: not every node is a seed exactly once" % epoch
        assert not torch.equal(seen[0][2], seen[r["batches"]][2]), "both epochs draw the same permutation"
        seen2 = []
        r2 = H.run(_harness_args(seen2, **kw), quiet=True)
        assert r2["final_loss"] == r["final_loss"] and r2["sampled_loss"] == r["sampled_loss"], "a second identical run gives another loss"
        assert all(torch.equal(a[2], b[2]) for a, b in zip(seen, seen2))
    finally:
        T.set_plan_cache_size(8)
        T.clear_plan_cache()


def test_harness_refuses_batch_size_without_fanout_and_with_a_captured_epoch(dev):
    import tcgnn_harness as H
    with pytest.raises(ValueError, match="--fanout"):
        H.run(_harness_args([], fanout=None), quiet=True)
    with pytest.raises(ValueError, match="hip_graph"):
        H.run(_harness_args([], hip_graph=True), quiet=True)
    with pytest.raises(ValueError, match=">= 1"):
        H.run(_harness_args([], batch_size=0), quiet=True)
