"""Seed-list sampling without a GPU: tests/frontier_ref.py's restatement of sample_rows / extend_nodes / compact_rows_graph gives, hop
by hop from the seeds, the same nodes, blocks and eids as the dense pipeline restated (sample_ref + compact_ref); the workspace query
and every refusal of the C calls that precedes a launch; the Python layer's argument checks; the harness's --sampler."""
import ctypes

import numpy as np
import pytest
import torch

import frontier_ref as FR
import sample_ref as R

_GRAPHS = {}


def _graph(name):
    if name not in _GRAPHS:
        if name == "rows":
            rp, col, long_row = R.row_length_graph()
            _GRAPHS[name] = (rp, col[:rp[-1]], long_row)
        else:
            import graphs
            rp, col = graphs.community_graph(3000, 10, 20, 0.8, seed=4)
            _GRAPHS[name] = (rp.astype(np.int32), col.astype(np.int32), None)
    return _GRAPHS[name]


def _seeds(name, kind):
    rp, _, long_row = _graph(name)
    s = np.random.default_rng(3).choice(len(rp) - 1, 48, replace=False)
    if long_row is not None:
        s[0] = long_row   # (the hub row among the seeds)
    if kind == "sorted":
        return np.sort(s)
    if kind == "repeated":
        return np.concatenate([s, s[::3], s[:5]])
    return s


@pytest.mark.parametrize("kind", ["sorted", "unsorted", "repeated"])
@pytest.mark.parametrize("fanouts", [(5, 3), (4, 3, 2)], ids=["5-3", "4-3-2"])
@pytest.mark.parametrize("name", ["rows", "sbm"])
def test_the_row_list_pipeline_equals_the_dense_pipeline(name, fanouts, kind):
    rp, col, _ = _graph(name)
    seeds = _seeds(name, kind)
    a = FR.batch_rows(rp, col, seeds, fanouts, 40)
    b = FR.batch_dense(rp, col, seeds, fanouts, 40)
    for x, y, what in zip(a[:3], b[:3], ("nodes", "new_id", "seed_pos")):
        assert x.dtype == y.dtype and np.array_equal(x, y), what
    assert len(a[3]) == len(b[3]) == len(fanouts)
    for layer, ((rp_a, col_a), (rp_b, col_b), eid_a, eid_b) in enumerate(zip(a[3], b[3], a[4], b[4])):
        assert rp_a.dtype == np.int32 and col_a.dtype == np.int32 and eid_a.dtype == np.int32
        assert np.array_equal(rp_a, rp_b) and np.array_equal(col_a, col_b) and np.array_equal(eid_a, eid_b), "layer %d" % layer
    assert len(a[0]) > len(np.unique(seeds)), "no hop reached a node beyond the seeds"


def test_sample_rows_restated_is_the_listed_rows_of_the_dense_sample_slot_by_slot():
    rp, col, long_row = _graph("rows")
    rows = np.array([long_row, 5, long_row, 0, 2047, 5], dtype=np.int32)   # any order, repeats: every occurrence has its own slot
    rp_s, col_s, eid = FR.sample_rows(rp, col, rows, 7, 2)
    d = np.diff(rp.astype(np.int64))
    assert rp_s[0] == 0 and np.array_equal(np.diff(rp_s), np.minimum(d[rows], 7))
    for i, r in enumerate(rows):
        mine = eid[rp_s[i]:rp_s[i + 1]]
        assert mine.tolist() == R.brute_force_row(2, int(rp[r]), int(d[r]), 7)
        assert np.array_equal(col_s[rp_s[i]:rp_s[i + 1]], col[mine])


def test_extend_nodes_accumulates_and_compact_rows_graph_gives_unlisted_nodes_empty_rows():
    keep = np.zeros(10, dtype=np.uint8)
    nodes, new_id = FR.extend_nodes(keep, np.array([7, 2, 7]))
    assert nodes.tolist() == [2, 7] and new_id.tolist() == [-1, -1, 0, -1, -1, -1, -1, 1, -1, -1]
    rows = nodes
    rp_s, col_s = np.array([0, 2, 3], np.int32), np.array([9, 2, 4], np.int32)   # row 2: columns 9, 2; row 7: column 4
    nodes, new_id = FR.extend_nodes(keep, [col_s, np.zeros(0, np.int32)])
    assert nodes.tolist() == [2, 4, 7, 9] and keep.tolist() == [0, 0, 1, 0, 1, 0, 0, 1, 0, 1]
    rp_b, col_b = FR.compact_rows_graph(rows, rp_s, col_s, nodes, new_id)
    assert rp_b.tolist() == [0, 2, 2, 3, 3] and col_b.tolist() == [3, 0, 1]
    assert FR.expand_rows(rows, rp_s, 10).tolist() == [0, 0, 0, 2, 2, 2, 2, 2, 3, 3, 3]


# ---- the library, loaded on the CPU ---------------------------------------------------------------------------------------------------

INVALID_ARG, WORKSPACE = 1, 5   # TCGNN_ERR_INVALID_ARG, TCGNN_ERR_WORKSPACE (include/tcgnn.h)


@pytest.fixture(scope="module")
def C():
    import tcgnn_capi
    return tcgnn_capi


def test_library_exports_the_calls_and_the_abi_version_is_unchanged(C):
    for name in ("tcgnn_sample_rows_workspace_bytes", "tcgnn_sample_rows_count", "tcgnn_sample_rows", "tcgnn_compact_mark_ids",
                 "tcgnn_compact_rows_graph"):
        assert name in C.SIGNATURES and getattr(C.lib, name) is not None
    assert C.lib.tcgnn_abi_version() == 1


@pytest.mark.parametrize("num_rows", [0, 1, 1023, 1024, 1025, 1024 * 256 + 1])
def test_rows_workspace_query_without_a_device(C, num_rows):
    need = C._sz(0)
    assert C.lib.tcgnn_sample_rows_workspace_bytes(num_rows, ctypes.byref(need)) == 0
    assert need.value == FR.workspace_bytes(num_rows) and need.value % 256 == 0
    # the size follows the list: the same query for a graph of 2.4 M nodes is answered from num_rows alone (there is no such argument)
    assert C.lib.tcgnn_sample_rows_workspace_bytes(-1, ctypes.byref(need)) == INVALID_ARG
    assert C.lib.tcgnn_sample_rows_workspace_bytes(num_rows, None) == INVALID_ARG
    assert b"tcgnn_sample_rows_workspace_bytes" in C.lib.tcgnn_last_error()


def test_every_refusal_that_precedes_a_launch(C):
    """No pointer below is ever dereferenced: the calls return before any launch (there is no device here)."""
    P, WS = 0x10000, 0x20000
    need, cneed = C._sz(0), C._sz(0)
    assert C.lib.tcgnn_sample_rows_workspace_bytes(10, ctypes.byref(need)) == 0
    assert C.lib.tcgnn_compact_workspace_bytes(100, ctypes.byref(cneed)) == 0
    kept = C._i64(-7)

    def count(rp=P, rows=P, r=10, n=100, e=1000, k=5, rp_s=P, ws=WS, nbytes=need.value, out=ctypes.byref(kept)):
        return C.lib.tcgnn_sample_rows_count(rp, rows, r, n, e, k, rp_s, ws, nbytes, out, None)

    def select(rp=P, col=P, rows=P, rp_s=P, r=10, n=100, e=1000, k=5, col_s=P, eid=P):
        return C.lib.tcgnn_sample_rows(rp, col, rows, rp_s, r, n, e, k, 0, col_s, eid, None)

    def mark(ids=P, count=10, n=100, keep=P, ws=WS, nbytes=cneed.value):
        return C.lib.tcgnn_compact_mark_ids(ids, count, n, keep, ws, nbytes, None)

    def graph(rows=P, r=10, rp_s=P, col_s=P, e=30, new_id=P, n=100, m=10, rp_b=P, col_b=P):
        return C.lib.tcgnn_compact_rows_graph(rows, r, rp_s, col_s, e, new_id, n, m, rp_b, col_b, None)

    assert count(rp=None) == INVALID_ARG and count(rows=None) == INVALID_ARG and count(rp_s=None) == INVALID_ARG and count(out=None) == INVALID_ARG
    assert count(r=-1) == INVALID_ARG and count(n=-1) == INVALID_ARG and count(e=-1) == INVALID_ARG and count(k=-1) == INVALID_ARG
    assert count(e=2 ** 31) == INVALID_ARG and b"int32" in C.lib.tcgnn_last_error()
    assert count(ws=None) == WORKSPACE and count(nbytes=need.value - 1) == WORKSPACE and count(ws=WS + 4) == WORKSPACE and count(ws=WS + 128) == WORKSPACE
    assert b"tcgnn_sample_rows_workspace_bytes" in C.lib.tcgnn_last_error()
    assert kept.value == -7
    assert select(rp=None) == INVALID_ARG and select(col=None) == INVALID_ARG and select(rows=None) == INVALID_ARG and select(rp_s=None) == INVALID_ARG
    assert select(col_s=None) == INVALID_ARG and select(eid=None) == INVALID_ARG
    assert select(r=-1) == INVALID_ARG and select(n=-1) == INVALID_ARG and select(e=-1) == INVALID_ARG and select(k=-1) == INVALID_ARG
    assert select(e=2 ** 31) == INVALID_ARG and b"int32" in C.lib.tcgnn_last_error()
    assert mark(ids=None) == INVALID_ARG and mark(keep=None) == INVALID_ARG and mark(count=-1) == INVALID_ARG and mark(n=-1) == INVALID_ARG
    assert mark(ws=None) == WORKSPACE and mark(nbytes=cneed.value - 1) == WORKSPACE and mark(ws=WS + 4) == WORKSPACE
    assert b"tcgnn_compact_workspace_bytes" in C.lib.tcgnn_last_error()
    assert graph(rows=None) == INVALID_ARG and graph(rp_s=None) == INVALID_ARG and graph(col_s=None) == INVALID_ARG and graph(new_id=None) == INVALID_ARG
    assert graph(rp_b=None) == INVALID_ARG and graph(col_b=None) == INVALID_ARG
    assert graph(r=-1) == INVALID_ARG and graph(e=-1) == INVALID_ARG and graph(n=-1) == INVALID_ARG and graph(m=-1) == INVALID_ARG and graph(m=101) == INVALID_ARG
    assert graph(e=2 ** 31) == INVALID_ARG and b"int32" in C.lib.tcgnn_last_error()


# ---- the Python layer's argument checks (they precede every device call) -----------------------------------------------------------------

def test_the_module_refuses_wrong_dtypes_and_devices():
    import TCGNN as T
    i32 = torch.zeros(4, dtype=torch.int32)
    for call in (lambda: T.sample_rows(i32, i32, i32, 5, 0),                                       # CPU tensors: the calls are for the device
                 lambda: T.extend_nodes(torch.zeros(4, dtype=torch.uint8), i32),
                 lambda: T.compact_rows_graph(i32, i32, i32, i32, i32)):
        with pytest.raises(RuntimeError, match="CUDA"):
            call()
    for call in (lambda: T.sample_rows(None, i32, i32, 5, 0), lambda: T.extend_nodes(None, i32),
                 lambda: T.compact_rows_graph([0, 1], i32, i32, i32, i32)):
        with pytest.raises(TypeError):
            call()
    i64, u8 = torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.uint8)
    for call in (lambda: T.sample_rows(i32, i32, i64, 5, 0), lambda: T.sample_rows(i64, i32, i32, 5, 0), lambda: T.sample_rows(i32, i32, u8, 5, 0),
                 lambda: T.extend_nodes(u8, i64), lambda: T.extend_nodes(u8, [i32, i64]),
                 lambda: T.compact_rows_graph(i32, i32, i32, i32, i64), lambda: T.compact_rows_graph(i64, i32, i32, i32, i32)):
        with pytest.raises(RuntimeError, match="expected scalar type Int"):
            call()
    for bad in (torch.zeros(4, dtype=torch.bool), i32):   # (written in place: a bool mask is not taken)
        with pytest.raises(RuntimeError, match="uint8"):
            T.extend_nodes(bad, i32)
    with pytest.raises(ValueError, match="fanout"):
        T.sample_rows(i32, i32, i32, -1, 0)
    for name in ("sample_rows", "extend_nodes", "compact_rows_graph"):
        assert name in T.__all__


def test_sampler_parses_and_rows_is_refused_without_batch_size():
    import tcgnn_harness as H
    p = H.build_parser()
    assert p.parse_args([]).sampler == "dense"
    assert p.parse_args(["--fanout", "5,5", "--batch-size", "64", "--sampler", "rows"]).sampler == "rows"
    with pytest.raises(SystemExit):
        p.parse_args(["--sampler", "sparse"])
    assert H.parse_sampler("dense", None) == "dense" and H.parse_sampler("dense", 64) == "dense" and H.parse_sampler("rows", 64) == "rows"
    with pytest.raises(ValueError, match="--batch-size"):
        H.parse_sampler("rows", None)
    with pytest.raises(ValueError, match="dense"):
        H.parse_sampler("list", 64)
    # time_training refuses before it touches a tensor or the device
    for kw in ({"sampler": "rows"}, {"sampler": "rows", "fanout": "5"}):
        with pytest.raises(ValueError, match="--batch-size"):
            H.time_training("sage", None, None, None, 16, 16, 4, 2, 1, **kw)
