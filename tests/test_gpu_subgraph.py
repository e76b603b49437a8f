"""Subgraph sampling on the MI355X: tcgnn_random_walk and tcgnn_induce_count / tcgnn_induce on walks and node lists of every size
class over rows of every length class against tests/subgraph_ref.py (EVERY element, torch.equal) and against the library's own
sample_rows + compact_rows_graph; that unlisted / unvisited rows are not read; the memory contract and the reports of the count call;
inputs outside the contract; subgraph_batch / saint_batch field by field against the restatement; an operator on an induced block;
the harness's --sampler saint / cluster."""
import glob
import importlib.util
import os

import numpy as np
import pytest
import torch

import guarded as G
import sample_ref as R
import subgraph_ref as SG

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 1, 2 ** 63 + 5)
LENGTHS = (0, 1, 2, 4, 16)
BAD_GRAPH, WORKSPACE = 4, 5   # TCGNN_ERR_BAD_GRAPH, TCGNN_ERR_WORKSPACE (include/tcgnn.h)


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


def _i32(dev, a):
    return _dev(dev, np.asarray(a, dtype=np.int32))


_ON_DEV = {}
_LISTS = {}
_WANT = {}   # name -> the restated induce of that list, computed once, shared, never changed


def _graph():
    """the row-length graph without the out-of-range entries behind its last row: every column is a node"""
    rp, col, long_row = R.row_length_graph()
    return rp, col[:rp[-1]], long_row


def _graph_dev(dev):
    if "g" not in _ON_DEV:
        rp, col, _ = _graph()
        _ON_DEV["g"] = (_dev(dev, rp), _dev(dev, col))
    return _ON_DEV["g"]


def _new_id(n, nodes):
    new_id = np.full(n, -1, dtype=np.int32)
    new_id[nodes] = np.arange(len(nodes), dtype=np.int32)
    return new_id


def _node_lists():
    """name -> strictly increasing int32 node list over the row-length graph"""
    if not _LISTS:
        rp, col, long_row = _graph()
        n = len(rp) - 1
        d = np.diff(rp.astype(np.int64))
        rng = np.random.default_rng(29)
        boundary = np.array([r for ln in R.ROW_LENGTHS for r in np.nonzero(d == ln)[0][:2]] + [long_row])   # two rows of every class, and the hub
        hub_sources = col[rp[long_row]:rp[long_row + 1]]
        apart, seen = [], set()   # nodes with edges, none of them between two members
        for r in np.nonzero((d > 0) & (d < 40))[0]:
            mine = set(col[rp[r]:rp[r + 1]].tolist())
            if r not in seen and r not in mine and not (mine & set(apart)):
                apart.append(int(r))
                seen |= mine
            if len(apart) == 24:
                break
        _LISTS.update({
            "empty": np.zeros(0, np.int64),
            "one": np.array([int(np.nonzero(d == 1025)[0][0])]),
            "hub": np.array([long_row]),
            "hub+3": np.unique(np.concatenate([[long_row], hub_sources[[0, 7, 4099]]])),
            "boundary": np.unique(boundary),
            "arange": np.arange(n),
            "apart": np.sort(np.array(apart)),
            "M1023": np.sort(rng.choice(n, 1023, replace=False)),
            "M1024": np.sort(rng.choice(n, 1024, replace=False)),
            "M1025": np.sort(rng.choice(n, 1025, replace=False)),
        })
        for key in _LISTS:
            _LISTS[key] = _LISTS[key].astype(np.int32)
        assert len(_LISTS["apart"]) == 24 and len(_LISTS["hub+3"]) >= 3
    return _LISTS


def _want(name):
    if name not in _WANT:
        rp, col, _ = _graph()
        nodes = _node_lists()[name]
        _WANT[name] = SG.induce_subgraph(rp, col, nodes, _new_id(len(rp) - 1, nodes))
    return _WANT[name]


def _equal(got, want, what, names=("nodePointer_b", "edgeList_b", "eid")):
    for g, w, n in zip(got, want, names):
        assert g.dtype == torch.int32 and tuple(g.shape) == tuple(w.shape), "%s: %s has dtype %s, shape %s" % (what, n, g.dtype, tuple(g.shape))
        assert torch.equal(g, torch.from_numpy(w).to(g.device)), "%s: %s differs from the reference" % (what, n)


# ---- random_walk -------------------------------------------------------------------------------------------------------------------------

def _starts(W):
    rp, _, long_row = _graph()
    d = np.diff(rp.astype(np.int64))
    s = np.random.default_rng(W).integers(0, len(rp) - 1, W).astype(np.int32)
    if W:
        s[0] = long_row                              # the hub as a start
    if W > 2:
        s[1] = s[2] = int(np.nonzero(d == 0)[0][0])  # a start on an empty row, twice
    if W > 4:
        s[4] = long_row                              # a repeated start walks on its own
    return s


@pytest.mark.parametrize("W", [0, 1, 63, 64, 65, 3000])
def test_walks_equal_the_reference_in_both_modules(dev, T, ext, W):
    rp, col, _ = _graph()
    trp, tcol = _graph_dev(dev)
    starts = _starts(W)
    tstarts = _i32(dev, starts)
    for length in LENGTHS:
        for seed in SEEDS:
            want = SG.random_walk(rp, col, starts, length, seed)
            for mod in (T, ext):
                got = mod.random_walk(trp, tcol, tstarts, length, seed)
                assert got.dtype == torch.int32 and tuple(got.shape) == (W, length + 1) and got.is_contiguous()
                assert torch.equal(got, _dev(dev, want)), "W = %d, length = %d, seed = %d" % (W, length, seed)
            if W > 2 and length:
                assert (want[1] == starts[1]).all(), "a walk left a row without edges"


def test_every_step_is_an_edge_of_the_graph_or_a_stay(dev, T):
    rp, col, _ = _graph()
    trp, tcol = _graph_dev(dev)
    n = len(rp) - 1
    walks = T.random_walk(trp, tcol, _i32(dev, _starts(3000)), 4, 11).cpu().numpy().astype(np.int64)
    d = np.diff(rp.astype(np.int64))
    edges = np.repeat(np.arange(n, dtype=np.int64), d) * n + col     # key of (row <- source)
    u, v = walks[:, :-1].reshape(-1), walks[:, 1:].reshape(-1)
    stay = (u == v) & (d[u] == 0)
    assert np.all(stay | np.isin(u * n + v, edges))
    assert stay.any() and (~stay).any()


def test_out_of_range_starts_are_carried_through_and_spoiled_pointers_at_unvisited_rows_change_nothing(dev):
    """the C call on a walks array of exactly W (length + 1) entries inside sentinel moats, its inputs inside NaN moats"""
    import tcgnn_capi as C
    rp, col, long_row = _graph()
    n, E = len(rp) - 1, len(col)
    stream = torch.cuda.current_stream().cuda_stream
    starts = _starts(65)
    starts[7], starts[9] = -1, n
    length, seed = 4, 5
    want = SG.random_walk(rp, col, starts, length, seed)
    assert (want[7] == -1).all() and (want[9] == n).all()
    read = np.unique(want[:, :length])                     # rows whose two pointers a walk reads
    read = read[(read >= 0) & (read < n)]
    spoiled = np.full(n + 1, -(2 ** 31), dtype=np.int32)   # every other pointer: far outside [0, E]
    spoiled[1::2] = 2 ** 31 - 1
    spoiled[read], spoiled[read + 1] = rp[read], rp[read + 1]
    assert (spoiled != rp).sum() > n // 2
    cbuf, _ = G.guarded(dev, E, torch.int32, col)
    sbuf, _ = G.guarded(dev, len(starts), torch.int32, starts)
    for pointers in (rp, spoiled):
        pbuf, _ = G.guarded(dev, n + 1, torch.int32, pointers)
        wbuf, w = G.guarded(dev, (len(starts), length + 1), torch.int32, "output")
        st = C.lib.tcgnn_random_walk(G.address(pbuf), G.address(cbuf), G.address(sbuf), len(starts), n, E, length, seed, G.address(wbuf), stream)
        torch.cuda.synchronize()
        assert st == 0, C.lib.tcgnn_last_error()
        assert not G.moat_intact(wbuf, w), "the walk wrote outside walks"
        assert G.unwritten(w) == length + 1   # (the walk that stays on -1: its entries have the bits of the pre-fill)
        assert torch.equal(w, _dev(dev, want))


def test_ten_walks_are_bit_equal(dev, T):
    trp, tcol = _graph_dev(dev)
    starts = _i32(dev, _starts(3000))
    first = T.random_walk(trp, tcol, starts, 4, 2 ** 63 + 5)
    for _ in range(9):
        assert torch.equal(T.random_walk(trp, tcol, starts, 4, 2 ** 63 + 5), first)


# ---- induce_subgraph: every node list, both modules ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["empty", "one", "hub", "hub+3", "boundary", "arange", "apart", "M1023", "M1024", "M1025"])
def test_induce_equals_the_reference_in_both_modules(dev, T, ext, name):
    rp, col, _ = _graph()
    trp, tcol = _graph_dev(dev)
    nodes = _node_lists()[name]
    want = _want(name)
    tnodes, tnew = _i32(dev, nodes), _i32(dev, _new_id(len(rp) - 1, nodes))
    for mod in (T, ext):
        _equal(mod.induce_subgraph(trp, tcol, tnodes, tnew), want, name)
    if name == "arange":
        assert np.array_equal(want[0], rp) and np.array_equal(want[1], col) and np.array_equal(want[2], np.arange(len(col)))
    if name == "apart":
        assert want[0][-1] == 0 and np.diff(rp.astype(np.int64))[nodes].min() > 0, "an edge survived"
    if name == "hub":
        assert want[0][-1] == int((col[rp[nodes[0]]:rp[nodes[0] + 1]] == nodes[0]).sum())


def test_induce_on_shuffled_ids_through_extend_nodes(dev, T, ext):
    rp, col, _ = _graph()
    trp, tcol = _graph_dev(dev)
    n = len(rp) - 1
    ids = np.random.default_rng(7).integers(0, n, 1000).astype(np.int32)
    for mod in (T, ext):
        nodes, new_id = mod.extend_nodes(torch.zeros(n, dtype=torch.uint8, device=dev), _i32(dev, ids))
        assert np.array_equal(nodes.cpu().numpy(), np.unique(ids))
        _equal(mod.induce_subgraph(trp, tcol, nodes, new_id), SG.induce_subgraph(rp, col, np.unique(ids), _new_id(n, np.unique(ids))), "shuffled ids")


def test_induce_on_262145_short_rows_reaches_the_second_level_of_the_scan(dev, T):
    """M = 1 024 * 256 + 1 listed rows: 257 block sums, so the one-workgroup pass over the sums takes a second step with a carry.  The
    list is strictly increasing and M <= N, so the graph has that many nodes: rows of 0 .. 3 edges, three nodes left out"""
    m = 1024 * 256 + 1
    n = m + 3
    rng = np.random.default_rng(30)
    d = np.arange(n, dtype=np.int64) * 7 % 4
    rp = np.concatenate([[0], np.cumsum(d)]).astype(np.int32)
    col = rng.integers(0, n, int(rp[-1])).astype(np.int32)
    nodes = np.delete(np.arange(n), [5, 1024 * 100, n - 2]).astype(np.int32)
    want = SG.induce_subgraph(rp, col, nodes, _new_id(n, nodes))
    _equal(T.induce_subgraph(_dev(dev, rp), _dev(dev, col), _i32(dev, nodes), _i32(dev, _new_id(n, nodes))), want, "262 145 short rows")
    assert 0 < want[0][-1] < len(col)


def test_induce_equals_sample_rows_filtered_and_compacted_by_the_library_itself(dev, T):
    trp, tcol = _graph_dev(dev)
    n = trp.numel() - 1
    for name in ("boundary", "M1025", "hub+3"):
        nodes = _i32(dev, _node_lists()[name])
        new_id = _i32(dev, _new_id(n, _node_lists()[name]))
        rp_s, col_s, eid_s = T.sample_rows(trp, tcol, nodes, None, 0)
        has = new_id[col_s.long()] >= 0
        row = torch.repeat_interleave(torch.arange(nodes.numel(), device=dev), (rp_s[1:] - rp_s[:-1]).long())
        counts = torch.bincount(row[has], minlength=nodes.numel())
        rp_f = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), counts.cumsum(0)]).to(torch.int32)
        rp_b, col_b = T.compact_rows_graph(nodes, rp_f, col_s[has].contiguous(), nodes, new_id)
        got = T.induce_subgraph(trp, tcol, nodes, new_id)
        assert torch.equal(got[0], rp_b) and torch.equal(got[1], col_b) and torch.equal(got[2], eid_s[has]), name


# ---- induce: memory contract ----------------------------------------------------------------------------------------------------------------

def _addr(t):
    return t.data_ptr() if t.numel() else None


def _raw_induce(dev, trp, col, nodes, new_id, expect=0, ws=None, ws_short=0, ws_shift=0, col_shift=0, complete=True):
    """the two C calls on outputs of exactly the stated sizes inside sentinel moats, a workspace of exactly the queried size inside guard
    bytes and an edgeList inside NaN moats, col_shift elements off 16 bytes.  expect: the count call's status.
    -> ((nodePointer_b, edgeList_b, eid) or None, (pbuf, p), ws)"""
    import tcgnn_capi as C
    stream = torch.cuda.current_stream().cuda_stream
    tnodes, tnew = _i32(dev, nodes), _i32(dev, new_id)
    m, n, E = tnodes.numel(), trp.numel() - 1, len(col)
    colbuf, _ = G.guarded(dev, E, torch.int32, np.ascontiguousarray(col, dtype=np.int32), offset_elems=col_shift)
    need = C._sz(0)
    assert C.lib.tcgnn_induce_workspace_bytes(m, C.ctypes.byref(need)) == 0
    ws = ws or G.exact_workspace(dev, need.value)
    assert ws[1].numel() == need.value
    pbuf, p = G.guarded(dev, m + 1, torch.int32, "output")
    kept = C._i64(-7)
    st = C.lib.tcgnn_induce_count(trp.data_ptr(), G.address(colbuf) if E else None, _addr(tnodes), _addr(tnew), m, n, E, G.address(pbuf),
                                  G.address(ws[0]) + ws_shift, need.value - ws_short, C.ctypes.byref(kept), stream)
    torch.cuda.synchronize()
    assert st == expect, (st, C.lib.tcgnn_last_error())
    assert not G.moat_intact(pbuf, p), "the count call wrote outside nodePointer_b"
    assert not G.moat_intact(*ws), "the count call wrote outside its workspace"
    if st != 0:
        assert kept.value == -7
        return None, (pbuf, p), ws
    assert G.unwritten(p) == 0, "an entry of nodePointer_b was not written"
    assert kept.value == int(p[-1])
    cbuf, c = G.guarded(dev, kept.value, torch.int32, "output")
    ebuf, e = G.guarded(dev, kept.value, torch.int32, "output")
    st = C.lib.tcgnn_induce(trp.data_ptr(), G.address(colbuf) if E else None, _addr(tnodes), _addr(tnew), G.address(pbuf), m, n, E, kept.value,
                            G.address(cbuf) if kept.value else None, G.address(ebuf) if kept.value else None, stream)
    torch.cuda.synchronize()
    assert st == 0, C.lib.tcgnn_last_error()
    assert not G.moat_intact(pbuf, p), "the write call wrote nodePointer_b's moat"
    assert not G.moat_intact(cbuf, c) and not G.moat_intact(ebuf, e), "the write call wrote outside its outputs"
    if complete:
        assert G.unwritten(c) == 0 and G.unwritten(e) == 0, "an entry of the outputs was not written"
    return (p, c, e), (pbuf, p), ws


@pytest.mark.parametrize("col_shift", [0, 1, 2, 3])
def test_exact_outputs_and_workspace_with_edgelist_on_and_off_16_bytes(dev, col_shift):
    rp, col, _ = _graph()
    trp, _ = _graph_dev(dev)
    n = len(rp) - 1
    for name in ("empty", "hub+3", "boundary", "M1025", "arange"):
        nodes = _node_lists()[name]
        got, _, _ = _raw_induce(dev, trp, col, nodes, _new_id(n, nodes), col_shift=col_shift)
        _equal(got, _want(name), "the C calls, %s, edgeList %d entries off 16 bytes" % (name, col_shift))


def test_the_c_calls_drop_and_report_nothing_for_uncovered_entries_behind_the_rows(dev):
    rp, col_all, _ = R.row_length_graph()   # (NO_ROW out-of-range ids behind nodePointer[N]: inside edgeList, in no row)
    nodes = _node_lists()["boundary"]
    got, _, _ = _raw_induce(dev, _dev(dev, rp), col_all, nodes, _new_id(len(rp) - 1, nodes))
    _equal(got, _want("boundary"), "uncovered entries")


def test_a_workspace_one_byte_short_or_misaligned_is_refused_with_nothing_written(dev):
    rp, col, _ = _graph()
    trp, _ = _graph_dev(dev)
    nodes = _node_lists()["M1025"]
    for kw in ({"ws_short": 1}, {"ws_shift": 4}, {"ws_shift": 128}):
        _, (pbuf, p), ws = _raw_induce(dev, trp, col, nodes, _new_id(len(rp) - 1, nodes), expect=WORKSPACE, **kw)
        assert G.pristine(pbuf, p), "a refused call wrote nodePointer_b"
        assert G.pristine(*ws), "a refused call wrote its workspace"


def test_bad_listed_rows_are_reported_and_a_good_call_on_the_same_workspace_succeeds(dev):
    rp, col, long_row = _graph()
    trp, _ = _graph_dev(dev)
    n, E = len(rp) - 1, len(col)
    d = np.diff(rp.astype(np.int64))
    good = _node_lists()["boundary"]
    new_id = _new_id(n, good)
    i = int(good[np.nonzero(d[good] == 1024)[0][0]])   # a listed 1 024-edge row
    descending = rp.copy()
    descending[i], descending[i + 1] = descending[i + 1], descending[i]
    beyond = rp.copy()
    beyond[i + 1] = E + 5            # (still ascending at row i)
    wild = rp.copy()
    wild[i], wild[i + 1] = -(2 ** 31), 2 ** 31 - 1
    below, above = good.copy(), good.copy()
    below[0], above[-1] = -1, n
    bad_col = col.copy()
    bad_col[rp[i] + 77] = n
    neg_col = col.copy()
    neg_col[rp[long_row] + 69999] = -1
    cases = (("a listed id of -1", trp, col, below), ("a listed id of N", trp, col, above),
             ("a descending pair at a listed row", _dev(dev, descending), col, good), ("a pointer beyond E at a listed row", _dev(dev, beyond), col, good),
             ("pointers far outside [0, E] at a listed row", _dev(dev, wild), col, good), ("a column of N in a listed row", trp, bad_col, good),
             ("a column of -1 in the listed hub row", trp, neg_col, good))
    for what, p, c, nodes in cases:
        _, _, ws = _raw_induce(dev, p, c, nodes, new_id, expect=BAD_GRAPH)
        got, _, _ = _raw_induce(dev, trp, col, good, new_id, ws=ws)   # the same workspace, now with a good graph
        _equal(got, _want("boundary"), "a good call after " + what)
    # the same faults at rows that are NOT listed go unseen (their pointers and edges are not read): no report
    other = np.array([r for r in _node_lists()["M1023"] if r not in (i - 1, i, i + 1, long_row)], dtype=np.int32)
    want = SG.induce_subgraph(rp, col, other, _new_id(n, other))
    for p, c in ((_dev(dev, wild), col), (trp, bad_col), (trp, neg_col)):
        got, _, _ = _raw_induce(dev, p, c, other, _new_id(n, other))
        _equal(got, want, "faults at unlisted rows")


def test_inputs_outside_the_contract_leave_the_moats_intact(dev):
    rp, col, long_row = _graph()
    trp, _ = _graph_dev(dev)
    n = len(rp) - 1
    good = _node_lists()["boundary"]
    new_id = _new_id(n, good)
    rng = np.random.default_rng(31)
    wild = rng.integers(-(2 ** 31), 2 ** 31 - 1, n).astype(np.int32)
    wild[::3] = rng.integers(0, 3 * len(good), len(wild[::3]))   # many of them >= 0, some beyond M
    foreign = _new_id(n, _node_lists()["M1025"])
    for what, nodes, ids in (("reversed nodes", good[::-1], new_id), ("shuffled nodes", rng.permutation(good), new_id), ("a wild new_id", good, wild),
                             ("another list's new_id", good, foreign)):
        got, _, _ = _raw_induce(dev, trp, col, nodes, ids, complete=False)
        m = len(nodes)
        assert int(got[1].min()) >= 0 and int(got[1].max()) < m, what + ": a new id outside [0, M) was written"
    # reversed and shuffled lists keep every row's own edges (the count and the write agree whatever the order)
    got, _, _ = _raw_induce(dev, trp, col, good[::-1], new_id)
    assert int(got[0][-1]) == int(_want("boundary")[0][-1])


def test_degenerate_sizes(dev, T, ext):
    e = torch.zeros(0, dtype=torch.int32, device=dev)
    one = torch.zeros(1, dtype=torch.int32, device=dev)
    trp, tcol = _graph_dev(dev)
    for mod in (T, ext):
        rp_b, col_b, eid = mod.induce_subgraph(trp, tcol, e, torch.full((trp.numel() - 1,), -1, dtype=torch.int32, device=dev))   # M = 0
        assert rp_b.tolist() == [0] and col_b.numel() == 0 and eid.numel() == 0
        rp_b, col_b, eid = mod.induce_subgraph(one, e, e, e)                                                                        # N = 0
        assert rp_b.tolist() == [0] and col_b.numel() == 0 and eid.numel() == 0
        rp_b, col_b, eid = mod.induce_subgraph(torch.zeros(6, dtype=torch.int32, device=dev), e, _i32(dev, [0, 2, 4]), _i32(dev, [0, -1, 1, -1, 2]))   # E = 0
        assert rp_b.tolist() == [0, 0, 0, 0] and col_b.numel() == 0 and eid.numel() == 0
        assert tuple(mod.random_walk(one, e, e, 3, 0).shape) == (0, 4)                                                             # N = 0, W = 0
        assert mod.random_walk(torch.zeros(6, dtype=torch.int32, device=dev), e, _i32(dev, [4, 0]), 2, 1).tolist() == [[4, 4, 4], [0, 0, 0]]   # E = 0
        with pytest.raises(RuntimeError, match="new_id"):
            mod.induce_subgraph(trp, tcol, e, e)
    with pytest.raises(RuntimeError, match="contiguous"):
        T.induce_subgraph(trp, tcol, torch.arange(8, dtype=torch.int32, device=dev)[::2], torch.zeros(trp.numel() - 1, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError, match="expected scalar type Int"):
        T.random_walk(trp, tcol, torch.zeros(3, dtype=torch.int64, device=dev), 2, 0)
    with pytest.raises(RuntimeError, match="CUDA"):
        T.random_walk(trp, tcol, torch.zeros(3, dtype=torch.int32), 2, 0)   # starts on the CPU


def test_ten_induced_subgraphs_are_bit_equal(dev, T):
    trp, tcol = _graph_dev(dev)
    nodes = _node_lists()["boundary"]
    tnodes, tnew = _i32(dev, nodes), _i32(dev, _new_id(trp.numel() - 1, nodes))
    first = T.induce_subgraph(trp, tcol, tnodes, tnew)
    for _ in range(9):
        assert all(torch.equal(a, b) for a, b in zip(T.induce_subgraph(trp, tcol, tnodes, tnew), first))


# ---- batches --------------------------------------------------------------------------------------------------------------------------------

_SBM = {}


def _sbm(dev):
    if not _SBM:
        import graphs
        rp, col = graphs.community_graph(3000, 10, 20, 0.8, seed=4)
        _SBM["host"] = (rp.astype(np.int32), col.astype(np.int32))
        _SBM["g"] = tuple(_dev(dev, a) for a in _SBM["host"])
    return _SBM["g"], _SBM["host"]


def _batch_equals(batch, ref, layers, plan, what):
    nodes, new_id, seed_pos, (rp_b, col_b), eid = ref
    assert batch.nodes.dtype == torch.int32 and np.array_equal(batch.nodes.cpu().numpy(), nodes), what + ": nodes"
    assert batch.new_id.dtype == torch.int32 and np.array_equal(batch.new_id.cpu().numpy(), new_id), what + ": new_id"
    assert batch.seed_pos.dtype == torch.int64 and np.array_equal(batch.seed_pos.cpu().numpy(), seed_pos), what + ": seed_pos"
    assert len(batch.metas) == len(batch.eids) == layers
    assert all(m is batch.metas[0] for m in batch.metas) and all(e is batch.eids[0] for e in batch.eids), what + ": one graph, one object"
    m = batch.metas[0]
    assert len(m) == 5 and all(t.dtype == torch.int32 for t in m)
    assert np.array_equal(m[0].cpu().numpy(), rp_b) and np.array_equal(m[1].cpu().numpy(), col_b), what + ": the block"
    assert batch.eids[0].dtype == torch.int32 and np.array_equal(batch.eids[0].cpu().numpy(), eid), what + ": eid"
    if plan:
        assert m[2].numel() == (len(nodes) + 15) // 16 and m[3].numel() == len(col_b) == m[4].numel()
    else:
        assert m[2].numel() == m[3].numel() == m[4].numel() == 0


@pytest.mark.parametrize("plan", [False, True], ids=["bare", "plan"])
def test_subgraph_batch_and_saint_batch_equal_the_restatement_field_by_field(dev, T, plan):
    import tcgnn_layers as L
    csr, (rp, col) = _sbm(dev)
    base = np.random.default_rng(1).choice(3000, 64, replace=False)
    for kind, s in (("sorted", np.sort(base)), ("unsorted", base), ("repeated", np.concatenate([base, base[::3], base[:5]]))):
        got = L.subgraph_batch(csr, torch.from_numpy(s).to(dev), plan=plan, layers=3)   # (int64, as the harness's permutation)
        _batch_equals(got, SG.subgraph_batch(rp, col, s), 3, plan, kind + " ids")
    for length, layers in ((2, 2), (4, 1), (0, 2)):
        got = L.saint_batch(csr, torch.from_numpy(base).to(dev), length, 13, plan=plan, layers=layers)
        ref = SG.saint_batch(rp, col, base, length, 13)
        _batch_equals(got, ref, layers, plan, "walks of %d steps" % length)
        assert got.seed_pos.numel() == 64 * (length + 1)
        assert np.array_equal(got.nodes[got.seed_pos[::length + 1]].cpu().numpy(), base), "the roots are not where seed_pos says"
        assert length == 0 or (got.nodes.numel() > 64 and got.metas[0][1].numel() > 0)


def test_forward_max_on_an_induced_block_is_the_masked_full_graph_on_its_rows(dev, T):
    import tcgnn_layers as L
    csr, (rp, col) = _sbm(dev)
    n = len(rp) - 1
    batch = L.saint_batch(csr, torch.from_numpy(np.random.default_rng(2).choice(n, 200, replace=False)).to(dev), 2, 3, plan=False)
    nodes = batch.nodes.cpu().numpy()
    inside = np.zeros(n, dtype=bool)
    inside[nodes] = True
    stays = inside[col]   # the full graph with every column outside the set masked out: all N rows, fewer edges
    row = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
    rp_m = np.concatenate([[0], np.cumsum(np.bincount(row[stays], minlength=n))]).astype(np.int32)
    X = torch.randn(n, 24, generator=torch.Generator().manual_seed(0)).to(dev)
    y_full, arg_full = T.forward_max(X, _dev(dev, rp_m), _dev(dev, col[stays]))
    y_b, arg_b = T.forward_max(X[batch.nodes.long()].contiguous(), batch.metas[0][0], batch.metas[0][1])
    assert torch.equal(y_b, y_full[batch.nodes.long()])
    # and the winners are the same edges of the FULL graph: eid names them
    full_pos = torch.from_numpy(np.nonzero(stays)[0]).to(dev)
    a_b, a_f = arg_b.long(), arg_full[batch.nodes.long()].long()
    assert torch.equal(a_b < 0, a_f < 0)
    assert torch.equal(batch.eids[0].long()[a_b.clamp_min(0)][a_b >= 0], full_pos[a_f.clamp_min(0)][a_f >= 0])


# ---- harness --------------------------------------------------------------------------------------------------------------------------------

def _harness_args(model, *flags):
    import tcgnn_harness as H
    extra = ["--model", "sage", "--aggregator", "max"] if model == "sage" else ["--model", "gcn"]
    return H.build_parser().parse_args(["--synthetic", "citeseer", "--dim", "16", "--hidden", "16", "--classes", "4", "--epochs", "1", "--gpu_preprocess"]
                                       + extra + list(flags))


@pytest.mark.parametrize("sampler,flags,batches", [("saint", ("--batch-size", "64", "--walk-length", "2"), 52), ("cluster", ("--batch-size", "256"), 13)])
@pytest.mark.parametrize("model", ["sage", "gcn"])
def test_harness_trains_on_induced_subgraphs_reproducibly(dev, T, model, sampler, flags, batches):
    import tcgnn_harness as H
    T.clear_plan_cache()
    T.set_plan_cache_size(4)
    try:
        runs = [H.run(_harness_args(model, "--sampler", sampler, *flags), quiet=True) for _ in range(2)]
        normed = H.run(_harness_args(model, "--sampler", sampler, "--saint-norm", "8", *flags), quiet=True) if (model == "sage") == (sampler == "saint") else None
    finally:
        T.set_plan_cache_size(8)
        T.clear_plan_cache()
    a, b = runs
    assert a["batches"] == batches == (3327 + a["batch_size"] - 1) // a["batch_size"] and a["sampler"] == sampler and a["fanout"] is None
    assert np.isfinite(a["final_loss"]) and np.isfinite(a["sampled_loss"])
    assert a["final_loss"] == b["final_loss"] and a["sampled_loss"] == b["sampled_loss"], (a["final_loss"], b["final_loss"])
    assert a["mean_block_nodes"] == b["mean_block_nodes"] and a["mean_block_edges"] == b["mean_block_edges"]
    assert 0 < a["mean_block_nodes"] <= (64 * 3 if sampler == "saint" else 256) and a["mean_block_edges"] >= 0
    assert all(np.isfinite(a[k]) and a[k] >= 0 for k in ("sample_ms", "compact_ms", "plan_ms", "train_ms", "epoch_ms"))
    if normed is not None:
        assert np.isfinite(normed["final_loss"]) and normed["saint_norm"] == 8 and normed["batches"] == batches


def test_harness_refuses_the_subgraph_samplers_without_batch_size_or_with_fanout(dev):
    import tcgnn_harness as H
    with pytest.raises(ValueError, match="--batch-size"):
        H.run(_harness_args("sage", "--sampler", "saint"), quiet=True)
    with pytest.raises(ValueError, match="--fanout"):
        H.run(_harness_args("sage", "--sampler", "cluster", "--batch-size", "64", "--fanout", "5,3"), quiet=True)
    with pytest.raises(ValueError, match="--walk-length"):
        H.run(_harness_args("sage", "--sampler", "saint", "--batch-size", "64", "--walk-length", "-1"), quiet=True)
