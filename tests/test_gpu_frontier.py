"""Seed-list sampling on the MI355X: tcgnn_sample_rows_count / tcgnn_sample_rows on row lists of every size class over rows of every
length class against tests/frontier_ref.py (EVERY element of the three outputs, torch.equal) and against the library's own
sample_neighbors; that unlisted rows are not read; the memory contract and the reports of the count call; tcgnn_compact_mark_ids
(extend_nodes) and tcgnn_compact_rows_graph against the restatement and against compact_graph, in both forms of each kernel and on
inputs outside their contract; sample_batch_rows field by field against sample_batch; the harness's --sampler rows against dense."""
import glob
import importlib.util
import os

import numpy as np
import pytest
import torch

import frontier_ref as FR
import guarded as G
import sample_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FANOUTS = (0, 1, 5, 25, 64, 1000, 100000)
SEEDS = (0, 1, 2 ** 63 + 5)
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


_DENSE = {}   # (k, seed) -> the dense reference sample of the row-length graph, computed once, shared, never changed
_LISTS = {}
_ON_DEV = {}


def _graph():
    rp, col, long_row = R.row_length_graph()
    return rp, col[:rp[-1]], long_row


def _graph_dev(dev):
    if "g" not in _ON_DEV:
        rp, col, _ = _graph()
        _ON_DEV["g"] = (_dev(dev, rp), _dev(dev, col))
    return _ON_DEV["g"]


def _dense(k, seed):
    if (k, seed) not in _DENSE:
        rp, col, _ = _graph()
        _DENSE[(k, seed)] = R.sample_neighbors(rp, col, k, seed)
    return _DENSE[(k, seed)]


def _row_lists():
    """name -> int32 row list over the row-length graph: every size class of the list (the four-slots-per-workgroup edge, the scan's
    1 024-slot workgroups and its second level's 256-sum passes) over rows of every length class"""
    if not _LISTS:
        rp, _, long_row = _graph()
        n = len(rp) - 1
        d = np.diff(rp.astype(np.int64))
        rng = np.random.default_rng(28)
        boundary = np.array([r for ln in R.ROW_LENGTHS for r in np.nonzero(d == ln)[0][:2]] + [long_row])   # two rows of every class, and the hub
        assert len(boundary) == 2 * len(R.ROW_LENGTHS) + 1
        short = np.nonzero(d < 40)[0]            # (empty rows among them)
        b1025 = int(np.nonzero(d == 1025)[0][0])
        _LISTS.update({
            "empty": np.zeros(0, np.int64),
            "one": np.array([b1025]),
            "R3": np.array([long_row, b1025, 0]),
            "R4": np.array([b1025, long_row, int(short[3]), int(np.nonzero(d == 4099)[0][0])]),
            "R5": np.array([int(short[1]), int(np.nonzero(d == 1024)[0][0]), int(short[2]), int(short[1]), long_row]),
            "boundary": boundary,
            "arange": np.arange(n),
            "shuffled-repeats": rng.integers(0, n, 3000),
            "R1023": rng.integers(0, n, 1023),
            "R1024": rng.integers(0, n, 1024),
            "R1025": rng.integers(0, n, 1025),
            "R262145-short": np.resize(rng.permutation(short), 1024 * 256 + 1),
        })
        for key in _LISTS:
            _LISTS[key] = _LISTS[key].astype(np.int32)
        assert len(np.unique(_LISTS["shuffled-repeats"])) < 3000
    return _LISTS


def _equal(got, want, what):
    for g, w, n in zip(got, want, ("rowPointer_s", "edgeList_s", "eid")):
        assert g.dtype == torch.int32 and g.shape == w.shape, "%s: %s has dtype %s, shape %s" % (what, n, g.dtype, tuple(g.shape))
        assert torch.equal(g, torch.from_numpy(w).to(g.device)), "%s: %s differs from the reference" % (what, n)


# ---- sample_rows: every list, every fan-out class, three seeds --------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS, ids=["seed%d" % s for s in SEEDS])
@pytest.mark.parametrize("k", FANOUTS, ids=["k%d" % k for k in FANOUTS])
def test_every_row_list_equals_the_reference(dev, T, k, seed):
    rp, col, _ = _graph()
    trp, tcol = _graph_dev(dev)
    dense = _dense(k, seed)
    for name, rows in _row_lists().items():
        got = T.sample_rows(trp, tcol, _dev(dev, rows), k, seed)
        _equal(got, FR.sample_rows(rp, col, rows, k, seed, dense=dense), "%s, k = %d, seed = %d" % (name, k, seed))
        if name == "arange":
            lib = T.sample_neighbors(trp, tcol, k, seed)
            assert all(torch.equal(a, b) for a, b in zip(got, lib)), "arange(N) differs from the library's own sample_neighbors"


def test_no_fanout_keeps_every_edge_of_the_listed_rows(dev, T):
    rp, col, long_row = _graph()
    trp, tcol = _graph_dev(dev)
    rows = _row_lists()["R5"]
    full = (rp, col, np.arange(len(col), dtype=np.int32))
    for k in (None, R.LONG_ROW, 2 ** 40):
        _equal(T.sample_rows(trp, tcol, _dev(dev, rows), k, 7), FR.sample_rows(rp, col, rows, None, 7, dense=full), "k = %r" % (k,))


def test_the_low_half_of_the_word_decides_between_two_equal_hashes(dev, T):
    rp, col, long_row = _graph()
    trp, tcol = _graph_dev(dev)
    found = R.equal_hash_pair(rp, long_row)
    assert found is not None, "no seed in 0..15 gives the 70 000-edge row two equal hashes"
    seed, k = found
    lo, hi = int(rp[long_row]), int(rp[long_row + 1])
    w = np.sort(R.words(seed, np.arange(lo, hi)))
    assert (w[k - 1] >> np.uint64(32)) == (w[k] >> np.uint64(32)), "the pair does not straddle k"
    rows = np.array([5, long_row, 7], dtype=np.int32)
    got = T.sample_rows(trp, tcol, _dev(dev, rows), k, seed)
    _equal(got, FR.sample_rows(rp, col, rows, k, seed), "k = %d, seed = %d" % (k, seed))
    eid = got[2].cpu().numpy()
    assert int(w[k - 1] & np.uint64(0xFFFFFFFF)) in eid and int(w[k] & np.uint64(0xFFFFFFFF)) not in eid


def test_unlisted_rows_are_not_read(dev, T):
    rp, col, _ = _graph()
    _, tcol = _graph_dev(dev)
    rows = _row_lists()["boundary"]
    touched = np.zeros(len(rp), dtype=bool)
    touched[rows] = True
    touched[rows + 1] = True
    assert (~touched).sum() > 1000
    spoiled = rp.astype(np.int64)
    free = np.nonzero(~touched)[0]
    spoiled[free] = np.where(np.arange(len(free)) % 2 == 0, 2 ** 31 - 1 - np.arange(len(free)), -5 - np.arange(len(free)))   # descending, outside [0, E]
    spoiled = spoiled.astype(np.int32)
    for k, seed in ((25, 1), (1000, 0), (100000, 2)):
        clean = T.sample_rows(_dev(dev, rp), tcol, _dev(dev, rows), k, seed)
        got = T.sample_rows(_dev(dev, spoiled), tcol, _dev(dev, rows), k, seed)   # (no error either: BAD_GRAPH would raise)
        assert all(torch.equal(a, b) for a, b in zip(clean, got)), "the result depends on the pointers of unlisted rows"
        _equal(got, FR.sample_rows(rp, col, rows, k, seed, dense=_dense(k, seed)), "spoiled unlisted pointers, k = %d" % k)


# ---- memory contract -------------------------------------------------------------------------------------------------------------------

def _addr(t):
    return t.data_ptr() if t.numel() else None


def _raw_rows(dev, trp, tcol, rows, n, E, k, seed, expect=0, ws=None, ws_short=0, ws_shift=0):
    """the two C calls on outputs of exactly the stated sizes inside sentinel moats and a workspace of exactly the queried size inside
    guard bytes.  expect: the count call's status.  -> ((rowPointer_s, edgeList_s, eid) or None, (pbuf, p), ws)"""
    import tcgnn_capi as C
    stream = torch.cuda.current_stream().cuda_stream
    trows = _i32(dev, rows)
    nrows = trows.numel()
    need = C._sz(0)
    assert C.lib.tcgnn_sample_rows_workspace_bytes(nrows, C.ctypes.byref(need)) == 0
    ws = ws or G.exact_workspace(dev, need.value)
    assert ws[1].numel() == need.value
    pbuf, p = G.guarded(dev, nrows + 1, torch.int32, "output")
    kept = C._i64(-7)
    st = C.lib.tcgnn_sample_rows_count(trp.data_ptr(), _addr(trows), nrows, n, E, k, G.address(pbuf), G.address(ws[0]) + ws_shift, need.value - ws_short,
                                       C.ctypes.byref(kept), stream)
    torch.cuda.synchronize()
    assert st == expect, (st, C.lib.tcgnn_last_error())
    assert not G.moat_intact(pbuf, p), "the count call wrote outside rowPointer_s"
    assert not G.moat_intact(*ws), "the count call wrote outside its workspace"
    if st != 0:
        assert kept.value == -7
        return None, (pbuf, p), ws
    assert G.unwritten(p) == 0, "an entry of rowPointer_s was not written"
    assert kept.value == int(p[-1])
    cbuf, c = G.guarded(dev, kept.value, torch.int32, "output")
    ebuf, e = G.guarded(dev, kept.value, torch.int32, "output")
    st = C.lib.tcgnn_sample_rows(trp.data_ptr(), tcol.data_ptr(), _addr(trows), G.address(pbuf), nrows, n, E, k, seed % (1 << 64),
                                 G.address(cbuf) if kept.value else None, G.address(ebuf) if kept.value else None, stream)
    torch.cuda.synchronize()
    assert st == 0, C.lib.tcgnn_last_error()
    assert not G.moat_intact(cbuf, c) and not G.moat_intact(ebuf, e), "the select wrote outside its outputs"
    assert G.unwritten(c) == 0 and G.unwritten(e) == 0, "an entry of the outputs was not written"
    return (p, c, e), (pbuf, p), ws


@pytest.mark.parametrize("name", ["empty", "one", "R5", "boundary", "shuffled-repeats", "R1024", "R262145-short"])
def test_outputs_of_exactly_the_stated_sizes_and_a_workspace_of_exactly_the_queried_size(dev, name):
    rp, col, _ = _graph()
    trp, tcol = _graph_dev(dev)
    rows = _row_lists()[name]
    for k, seed in ((5, 0), (1000, 1)):
        got, _, _ = _raw_rows(dev, trp, tcol, rows, len(rp) - 1, len(col), k, seed)
        _equal(got, FR.sample_rows(rp, col, rows, k, seed, dense=_dense(k, seed)), "the C calls, %s, k = %d" % (name, k))


def test_the_c_call_sees_uncovered_entries_behind_the_rows(dev):
    rp, col_all, _ = R.row_length_graph()   # (NO_ROW out-of-range ids behind nodePointer[N])
    rows = _row_lists()["boundary"]
    got, _, _ = _raw_rows(dev, _dev(dev, rp), _dev(dev, col_all), rows, len(rp) - 1, int(rp[-1]), 25, 1)
    _equal(got, FR.sample_rows(rp, col_all, rows, 25, 1, dense=_dense(25, 1)), "uncovered entries")


def test_a_workspace_one_byte_short_or_misaligned_is_refused_with_nothing_written(dev):
    rp, col, _ = _graph()
    trp, tcol = _graph_dev(dev)
    rows = _row_lists()["R1025"]
    for kw in ({"ws_short": 1}, {"ws_shift": 4}, {"ws_shift": 128}):
        _, (pbuf, p), ws = _raw_rows(dev, trp, tcol, rows, len(rp) - 1, len(col), 5, 0, expect=WORKSPACE, **kw)
        assert G.pristine(pbuf, p), "a refused call wrote rowPointer_s"
        assert G.pristine(*ws), "a refused call wrote its workspace"


def test_bad_listed_rows_are_reported_and_a_good_call_on_the_same_workspace_succeeds(dev):
    rp, col, long_row = _graph()
    trp, tcol = _graph_dev(dev)
    n, E = len(rp) - 1, len(col)
    d = np.diff(rp.astype(np.int64))
    good = _row_lists()["R5"]
    i = int(good[1])   # the 1 024-edge row
    assert d[i] == 1024
    descending = rp.copy()
    descending[i], descending[i + 1] = descending[i + 1], descending[i]
    beyond = rp.copy()
    beyond[i + 1] = E + 5            # (still ascending at row i)
    wild = rp.copy()
    wild[i], wild[i + 1] = -(2 ** 31), 2 ** 31 - 1
    below, above = good.copy(), good.copy()
    below[2], above[4] = -1, n
    cases = (("a listed id of -1", trp, below), ("a listed id of N", trp, above), ("a descending pair at a listed row", _dev(dev, descending), good),
             ("a pointer beyond E at a listed row", _dev(dev, beyond), good), ("pointers far outside [0, E] at a listed row", _dev(dev, wild), good))
    want = FR.sample_rows(rp, col, good, 25, 3, dense=_dense(25, 3))
    for what, p, rows in cases:
        _, _, ws = _raw_rows(dev, p, tcol, rows, n, E, 25, 3, expect=BAD_GRAPH)
        got, _, _ = _raw_rows(dev, trp, tcol, good, n, E, 25, 3, ws=ws)   # the same workspace, now with a good list
        _equal(got, want, "a good call after " + what)
    # the same faults at rows that are NOT listed go unseen (they are not read): no report
    other = np.array([r for r in range(n) if r not in (i - 1, i, i + 1)][:40], dtype=np.int32)
    got, _, _ = _raw_rows(dev, _dev(dev, wild), tcol, other, n, E, 25, 3)
    _equal(got, FR.sample_rows(rp, col, other, 25, 3, dense=_dense(25, 3)), "faults at unlisted rows")


def test_a_list_that_keeps_more_than_int32_edges_is_refused_and_nothing_wraps(dev):
    """repeats let E' pass 2^31 - 1 where the dense call's can not: the scan's adds saturate, the count call refuses"""
    import tcgnn_capi as C
    rp, col, long_row = _graph()
    trp, _ = _graph_dev(dev)
    stream = torch.cuda.current_stream().cuda_stream
    fits = (2 ** 31 - 1) // R.LONG_ROW   # the most copies of the hub row whose edges an int32 position can count
    for copies, expect in ((fits, 0), (fits + 1, 1)):   # 1: TCGNN_ERR_INVALID_ARG
        trows = torch.full((copies,), long_row, dtype=torch.int32, device=dev)
        need = C._sz(0)
        assert C.lib.tcgnn_sample_rows_workspace_bytes(copies, C.ctypes.byref(need)) == 0
        ws = G.exact_workspace(dev, need.value)
        pbuf, p = G.guarded(dev, copies + 1, torch.int32, "output")
        kept = C._i64(-7)
        st = C.lib.tcgnn_sample_rows_count(trp.data_ptr(), trows.data_ptr(), copies, len(rp) - 1, len(col), R.LONG_ROW, G.address(pbuf), G.address(ws[0]),
                                           need.value, C.ctypes.byref(kept), stream)
        torch.cuda.synchronize()
        assert st == expect, (st, C.lib.tcgnn_last_error())
        assert not G.moat_intact(pbuf, p) and not G.moat_intact(*ws)
        got = p.cpu().numpy().astype(np.int64)
        exact = np.arange(copies + 1, dtype=np.int64) * R.LONG_ROW
        inside = exact <= 2 ** 31 - 1
        assert np.array_equal(got[inside], exact[inside]), "a pointer below 2^31 is not the exact sum"
        assert np.all(got[~inside] == -(2 ** 31)), "a sum beyond int32 did not saturate to a negative pointer"
        assert kept.value == (copies * R.LONG_ROW if expect == 0 else -7)


def test_degenerate_sizes(dev, T):
    e = torch.zeros(0, dtype=torch.int32, device=dev)
    one = torch.zeros(1, dtype=torch.int32, device=dev)
    rp_s, col_s, eid = T.sample_rows(one, e, e, 5, 1)                                                   # N = 0, R = 0
    assert rp_s.tolist() == [0] and col_s.numel() == 0 and eid.numel() == 0
    rp_s, col_s, eid = T.sample_rows(torch.zeros(6, dtype=torch.int32, device=dev), e, _i32(dev, [4, 0, 4]), 5, 1)   # E = 0
    assert rp_s.tolist() == [0] * 4 and col_s.numel() == 0 and eid.numel() == 0
    loop = (torch.tensor([0, 1], dtype=torch.int32, device=dev), torch.tensor([0], dtype=torch.int32, device=dev))
    for k, kept in ((0, 0), (1, 1), (3, 1), (None, 1)):
        rp_s, col_s, eid = T.sample_rows(*loop, _i32(dev, [0, 0]), k, 9)
        assert rp_s.tolist() == [0, kept, 2 * kept] and col_s.tolist() == [0] * (2 * kept) and eid.tolist() == [0] * (2 * kept)
    with pytest.raises(RuntimeError, match="outside"):
        T.sample_rows(*loop, _i32(dev, [0, 1]), 1, 0)
    with pytest.raises(ValueError):
        T.sample_rows(*loop, _i32(dev, [0]), -1, 0)


def test_ten_repetitions_are_bit_identical_and_the_pybind_module_equals_the_ctypes_one(dev, T, ext):
    trp, tcol = _graph_dev(dev)
    rows = _dev(dev, _row_lists()["shuffled-repeats"])
    first = T.sample_rows(trp, tcol, rows, 25, 2 ** 63 + 5)
    for _ in range(9):
        again = T.sample_rows(trp, tcol, rows, 25, 2 ** 63 + 5)
        assert all(torch.equal(a, b) for a, b in zip(first, again))
    for name, k, seed in (("shuffled-repeats", 25, 2 ** 63 + 5), ("boundary", 5000, 1), ("R5", None, 0), ("arange", 0, 3), ("empty", 5, 1)):
        rows = _dev(dev, _row_lists()[name])
        a = T.sample_rows(trp, tcol, rows, k, seed)
        b = ext.sample_rows(trp, tcol, rows, k, seed)
        assert all(torch.equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b)), "the pybind module differs at %s, k = %r" % (name, k)


def test_module_argument_checks(dev, T, ext):
    trp, tcol = _graph_dev(dev)
    rows = _i32(dev, [1, 2, 3])
    u8 = torch.zeros(trp.numel() - 1, dtype=torch.uint8, device=dev)
    for mod in (T, ext):
        with pytest.raises(RuntimeError):
            mod.sample_rows(trp, tcol, rows.long(), 5, 0)
        with pytest.raises(RuntimeError):
            mod.sample_rows(trp, tcol, rows.cpu(), 5, 0)
        with pytest.raises(RuntimeError):
            mod.sample_rows(trp, tcol, torch.arange(8, dtype=torch.int32, device=dev)[::2], 5, 0)
        with pytest.raises(RuntimeError):
            mod.extend_nodes(u8.bool(), rows)
        with pytest.raises(RuntimeError):
            mod.extend_nodes(u8, rows.long())
        with pytest.raises(RuntimeError):
            mod.extend_nodes(u8, [rows, rows.cpu()])
        with pytest.raises(RuntimeError):
            mod.compact_rows_graph(rows, rows, rows, rows, trp)            # rowPointer_s must hold R + 1 entries
        with pytest.raises(RuntimeError):
            mod.compact_rows_graph(rows, torch.zeros(4, dtype=torch.int32, device=dev), rows.long(), rows, trp)
    assert not bool(u8.any()), "a refused call marked the mask"


# ---- mark_ids / extend_nodes -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", [0, 1, 5, 1023, 4099])
def test_extend_nodes_equals_the_reference_and_the_mask_accumulates_in_both_forms_of_the_kernel(dev, T, ext, count):
    n = 5000
    rng = np.random.default_rng(count)
    first, second = rng.integers(0, n, count).astype(np.int32), rng.integers(0, n, 2 * count + 3).astype(np.int32)
    for mod in (T, ext):
        for off in (0, 1):   # off = 1: the list starts four bytes behind a sixteen-byte boundary - the dword form
            keep_ref = np.zeros(n, dtype=np.uint8)
            keep = torch.zeros(n, dtype=torch.uint8, device=dev)
            a = _dev(dev, np.concatenate([np.zeros(off, np.int32), first]))[off:]
            b = _dev(dev, np.concatenate([np.zeros(off, np.int32), second]))[off:]
            assert count == 0 or (a.data_ptr() % 16 == 4 * off and b.data_ptr() % 16 == 4 * off)
            for ids, ids_ref in ((a, first), ([b, a], [second, first])):
                nodes, new_id = mod.extend_nodes(keep, ids)
                want_nodes, want_new = FR.extend_nodes(keep_ref, ids_ref)
                assert nodes.dtype == torch.int32 and new_id.dtype == torch.int32
                assert torch.equal(nodes.cpu(), torch.from_numpy(want_nodes)) and torch.equal(new_id.cpu(), torch.from_numpy(want_new))
                assert torch.equal(keep.cpu(), torch.from_numpy(keep_ref)), "the mask was not extended in place"


def test_ids_out_of_range_are_reported_by_the_count_call_and_not_followed(dev, T):
    n = 3000
    for bad in (-1, n, 2 ** 31 - 1, -(2 ** 31)):
        buf, keep = G.guarded(dev, n, torch.uint8, "output", align=4)
        keep.zero_()
        with pytest.raises(RuntimeError, match="outside"):
            T.extend_nodes(keep, _i32(dev, [5, bad, 7, 2999, 0]))
        assert not G.moat_intact(buf, keep), "an id out of range was followed"
        assert torch.nonzero(keep).view(-1).tolist() == [0, 5, 7, 2999]
        nodes, _ = T.extend_nodes(keep, _i32(dev, [6]))   # (the report leaves the validation word clear)
        assert nodes.tolist() == [0, 5, 6, 7, 2999]


def test_mark_ids_refuses_a_short_workspace_with_nothing_written(dev):
    import tcgnn_capi as C
    n = 3000
    need = C._sz(0)
    assert C.lib.tcgnn_compact_workspace_bytes(n, C.ctypes.byref(need)) == 0
    ws = G.exact_workspace(dev, need.value)
    buf, keep = G.guarded(dev, n, torch.uint8, "output", align=4)
    ids = _i32(dev, [1, 2, 3])
    st = C.lib.tcgnn_compact_mark_ids(ids.data_ptr(), 3, n, G.address(buf), G.address(ws[0]), need.value - 1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == WORKSPACE and G.pristine(buf, keep) and G.pristine(*ws)


# ---- compact_rows_graph ------------------------------------------------------------------------------------------------------------------

def _raw_block(dev, rows, rp_s, col_s, new_id, m, shift=0, e=None):
    """tcgnn_compact_rows_graph on moated outputs of exactly M + 1 and E' entries; shift = 1 puts both edge arrays four bytes behind a
    sixteen-byte boundary (the dword form).  -> (nodePointer_b, edgeList_b)"""
    import tcgnn_capi as C
    trows, trp_s, tnew = _i32(dev, rows), _i32(dev, rp_s), _i32(dev, new_id)
    e = len(col_s) if e is None else e
    cin_buf, cin = G.guarded(dev, len(col_s), torch.int32, np.asarray(col_s, dtype=np.int32), offset_elems=shift)
    rbuf, r = G.guarded(dev, m + 1, torch.int32, "output", offset_elems=shift)
    obuf, o = G.guarded(dev, e, torch.int32, "output", offset_elems=shift)
    st = C.lib.tcgnn_compact_rows_graph(_addr(trows), trows.numel(), trp_s.data_ptr(), G.address(cin_buf) if e else None, e, _addr(tnew), tnew.numel(), m,
                                        G.address(rbuf), G.address(obuf) if e else None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0, C.lib.tcgnn_last_error()
    assert not G.moat_intact(rbuf, r) and not G.moat_intact(obuf, o), "tcgnn_compact_rows_graph wrote outside its outputs"
    assert G.unwritten(r) == 0, "an entry of nodePointer_b was not written"
    return r, o


_HOPS = {}


def _sampled_hops(dev, T):
    """two hops of the row-list pipeline on the row-length graph from 48 seeds (the hub row among them), restated in numpy: per hop
    (rows, rowPointer_s, edgeList_s), and the final (nodes, new_id)"""
    if not _HOPS:
        rp, col, long_row = _graph()
        seeds = np.random.default_rng(3).choice(len(rp) - 1, 48, replace=False)
        seeds[0] = long_row
        keep = np.zeros(len(rp) - 1, dtype=np.uint8)
        nodes, new_id = FR.extend_nodes(keep, seeds)
        hops = []
        for hop, k in enumerate((3, 5)):
            rows = nodes
            rp_s, col_s, _ = FR.sample_rows(rp, col, rows, k, 60 + hop)
            nodes, new_id = FR.extend_nodes(keep, col_s)
            hops.append((rows, rp_s, col_s))
        _HOPS["h"] = (hops, nodes, new_id)
    return _HOPS["h"]


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "off-16-bytes"])
def test_blocks_equal_the_reference_and_compact_graph_of_the_expanded_graph(dev, T, ext, shift):
    hops, nodes, new_id = _sampled_hops(dev, T)
    n, m = len(new_id), len(nodes)
    tnodes, tnew = _i32(dev, nodes), _i32(dev, new_id)
    for rows, rp_s, col_s in hops:
        want = FR.compact_rows_graph(rows, rp_s, col_s, nodes, new_id)
        r, o = _raw_block(dev, rows, rp_s, col_s, new_id, m, shift=shift)
        assert torch.equal(r.cpu(), torch.from_numpy(want[0])) and torch.equal(o.cpu(), torch.from_numpy(want[1])), "the C call differs from the reference"
        # the same graph written over all N rows, through the existing compact_graph
        full = T.compact_graph(_i32(dev, FR.expand_rows(rows, rp_s, n)), _i32(dev, col_s), tnodes, tnew)
        assert torch.equal(full[0], r) and torch.equal(full[1], o), "the block differs from compact_graph of the expanded graph"
        for mod in (T, ext):
            got = mod.compact_rows_graph(_i32(dev, rows), _i32(dev, rp_s), _i32(dev, col_s), tnodes, tnew)
            assert got[0].dtype == torch.int32 and got[1].dtype == torch.int32
            assert torch.equal(got[0], r) and torch.equal(got[1], o), "the module differs from the C call"


def test_lists_that_are_not_increasing_and_wild_new_ids_stay_in_bounds(dev):
    hops, nodes, new_id = _sampled_hops(dev, None)
    rows, rp_s, col_s = hops[1]
    n, m = len(new_id), len(nodes)
    rng = np.random.default_rng(9)
    wild = rng.integers(-(2 ** 31), 2 ** 31, n).astype(np.int32)
    wild[::3] = rng.integers(0, m, len(wild[::3]))
    bad_rows = rows.copy()
    bad_rows[::5] = [-1, n, 2 ** 31 - 1, -(2 ** 31)] * (len(bad_rows[::5]) // 4) + [-7] * (len(bad_rows[::5]) % 4)
    bad_ptr = rp_s.copy()
    bad_ptr[::2] = rng.integers(-(2 ** 31), 2 ** 31, len(bad_ptr[::2]))
    bad_col = col_s.copy()
    bad_col[::4] = rng.integers(-(2 ** 31), 2 ** 31, len(bad_col[::4]))
    for shift in (0, 1):
        for what, args in (("reversed rows", (rows[::-1].copy(), rp_s, col_s, new_id)), ("shuffled rows", (rng.permutation(rows), rp_s, col_s, new_id)),
                           ("ids out of range among the rows", (bad_rows, rp_s, col_s, new_id)), ("a wild new_id", (rows, rp_s, col_s, wild)),
                           ("wild row pointers", (rows, bad_ptr, col_s, new_id)), ("wild columns", (rows, rp_s, bad_col, new_id)),
                           ("a new_id of minus ones", (rows, rp_s, col_s, np.full(n, -1, np.int32)))):
            r, o = _raw_block(dev, *args, m, shift=shift)   # (the moats are checked inside)
            r, o = r.cpu().numpy(), o.cpu().numpy()
            assert r.min() >= 0 and r.max() <= len(col_s) and r[m] == len(col_s), what
            assert G.unwritten(torch.from_numpy(o)) == 0 and o.min() >= 0 and o.max() < m, what


def test_no_nodes_no_rows_and_no_edges(dev, T):
    e = np.zeros(0, np.int32)
    r, o = _raw_block(dev, e, np.zeros(1, np.int32), e, np.full(10, -1, np.int32), 0)                      # M = 0, R = 0, E' = 0
    assert r.tolist() == [0] and o.numel() == 0
    r, o = _raw_block(dev, e, np.zeros(1, np.int32), e, e, 0)                                             # N = 0 as well
    assert r.tolist() == [0]
    new_id = np.array([-1, 0, -1, 1, 2], np.int32)
    r, o = _raw_block(dev, e, np.zeros(1, np.int32), e, new_id, 3)                                         # R = 0: every row empty
    assert r.tolist() == [0, 0, 0, 0]
    r, o = _raw_block(dev, np.array([1, 4], np.int32), np.zeros(3, np.int32), e, new_id, 3)               # E' = 0
    assert r.tolist() == [0, 0, 0, 0]
    keep = torch.zeros(5, dtype=torch.uint8, device=dev)
    nodes, nid = T.extend_nodes(keep, torch.zeros(0, dtype=torch.int32, device=dev))                      # nothing marked: M = 0
    assert nodes.numel() == 0 and nid.tolist() == [-1] * 5
    rp_b, col_b = T.compact_rows_graph(nodes, torch.zeros(1, dtype=torch.int32, device=dev), nodes, nodes, nid)
    assert rp_b.tolist() == [0] and col_b.numel() == 0
    nodes, nid = T.extend_nodes(torch.zeros(0, dtype=torch.uint8, device=dev), [])                        # N = 0
    assert nodes.numel() == 0 and nid.numel() == 0


# ---- sample_batch_rows --------------------------------------------------------------------------------------------------------------------

_SBM = {}


def _sbm(dev):
    if not _SBM:
        import graphs
        rp, col = graphs.community_graph(3000, 10, 20, 0.8, seed=4)
        _SBM["g"] = (_dev(dev, rp.astype(np.int32)), _dev(dev, col.astype(np.int32)))
    return _SBM["g"]


def _same_batch(a, b, what):
    assert a.nodes.dtype == torch.int32 and torch.equal(a.nodes, b.nodes), what + ": nodes"
    assert a.seed_pos.dtype == torch.int64 and torch.equal(a.seed_pos, b.seed_pos), what + ": seed_pos"
    assert a.new_id.dtype == torch.int32 and torch.equal(a.new_id, b.new_id), what + ": new_id"
    assert len(a.metas) == len(b.metas) == len(a.eids) == len(b.eids)
    for layer, (ma, mb, ea, eb) in enumerate(zip(a.metas, b.metas, a.eids, b.eids)):
        assert len(ma) == len(mb) == 5
        for i, (x, y) in enumerate(zip(ma, mb)):
            assert x.dtype == torch.int32 and x.shape == y.shape and torch.equal(x, y), "%s: layer %d, metadata tensor %d" % (what, layer, i)
        assert ea.dtype == torch.int32 and torch.equal(ea, eb), "%s: layer %d, eid" % (what, layer)


@pytest.mark.parametrize("plan", [False, True], ids=["bare", "plan"])
@pytest.mark.parametrize("fanouts", [(5, 3), (4, 3, 2)], ids=["5-3", "4-3-2"])
def test_sample_batch_rows_equals_sample_batch_field_by_field(dev, T, fanouts, plan):
    import tcgnn_layers as L
    csr = _sbm(dev)
    base = np.random.default_rng(1).choice(3000, 64, replace=False)
    for kind, s in (("sorted", np.sort(base)), ("unsorted", base), ("repeated", np.concatenate([base, base[::3], base[:5]]))):
        seeds = torch.from_numpy(s).to(dev)   # (int64, as the harness's permutation)
        got = L.sample_batch_rows(csr, seeds, list(fanouts), 13, plan=plan)
        want = L.sample_batch(csr, seeds, list(fanouts), 13, plan=plan)
        _same_batch(got, want, "%s seeds, fanouts %s" % (kind, fanouts))
        assert got.nodes.numel() > 64 and all(m[1].numel() > 0 for m in got.metas)
    # and both equal the restatement
    ref = FR.batch_rows(csr[0].cpu().numpy(), csr[1].cpu().numpy(), base, fanouts, 13)
    got = L.sample_batch_rows(csr, torch.from_numpy(base).to(dev), list(fanouts), 13, plan=False)
    assert np.array_equal(got.nodes.cpu().numpy(), ref[0]) and np.array_equal(got.new_id.cpu().numpy(), ref[1])
    for m, (rp_b, col_b), e, e_ref in zip(got.metas, ref[3], got.eids, ref[4]):
        assert np.array_equal(m[0].cpu().numpy(), rp_b) and np.array_equal(m[1].cpu().numpy(), col_b) and np.array_equal(e.cpu().numpy(), e_ref)


def test_sample_batch_rows_with_the_hub_row_among_the_seeds(dev, T):
    import tcgnn_layers as L
    rp, col, long_row = _graph()
    csr = _graph_dev(dev)
    s = np.random.default_rng(3).choice(len(rp) - 1, 48, replace=False)
    s[0] = long_row
    for fanouts in ((5, 3), (1000, 25)):
        seeds = torch.from_numpy(s).to(dev)
        _same_batch(L.sample_batch_rows(csr, seeds, list(fanouts), 5, plan=False), L.sample_batch(csr, seeds, list(fanouts), 5, plan=False),
                    "the row-length graph, fanouts %s" % (fanouts,))


# ---- harness -----------------------------------------------------------------------------------------------------------------------------

def _harness_args(**kw):
    import tcgnn_harness as H
    args = H.build_parser().parse_args(["--synthetic", "citeseer", "--dim", "16", "--hidden", "16", "--classes", "4", "--epochs", "2", "--model", "sage",
                                        "--aggregator", "max", "--gpu_preprocess", "--fanout", "5,3", "--batch-size", "64"])
    for k, v in kw.items():
        setattr(args, k, v)
    return args


@pytest.mark.parametrize("model", ["sage", "gcn"])
def test_harness_sampler_rows_trains_on_the_same_batches_as_dense(dev, T, model):
    import tcgnn_harness as H
    kw = {} if model == "sage" else {"model": "gcn", "aggregator": "mean"}
    T.clear_plan_cache()
    T.set_plan_cache_size(4)
    try:
        dense = H.run(_harness_args(sampler="dense", **kw), quiet=True)
        rows = H.run(_harness_args(sampler="rows", **kw), quiet=True)
    finally:
        T.set_plan_cache_size(8)
        T.clear_plan_cache()
    assert rows["batches"] == dense["batches"] and rows["batch_size"] == 64 and rows["fanout"] == [5, 3]
    assert rows["mean_block_nodes"] == dense["mean_block_nodes"]
    assert np.isfinite(rows["final_loss"]) and rows["final_loss"] == dense["final_loss"], (rows["final_loss"], dense["final_loss"])
    assert rows["sampled_loss"] == dense["sampled_loss"]
    assert all(np.isfinite(rows[k]) and rows[k] >= 0 for k in ("sample_ms", "compact_ms", "plan_ms", "train_ms", "epoch_ms"))


def test_harness_refuses_sampler_rows_without_batch_size(dev):
    import tcgnn_harness as H
    with pytest.raises(ValueError, match="--batch-size"):
        H.run(_harness_args(sampler="rows", batch_size=None), quiet=True)
