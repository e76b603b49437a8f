"""Relabelled mini-batch blocks without a GPU: the numpy restatement (tests/compact_ref.py) against its own properties and against
numpy.unique, the layered case against sample_ref's layered sampling, and - through tcgnn_capi, which loads the library on the CPU -
the new symbols, the workspace query and every refusal that precedes a launch; the harness's --batch-size checks."""
import ctypes

import numpy as np
import pytest

import compact_ref as CR
import sample_ref as R


def _random_csr(rng, n, rows_with_edges, max_deg, col_hi=None):
    d = np.zeros(n, dtype=np.int64)
    rows = rng.choice(n, size=min(rows_with_edges, n), replace=False)
    d[rows] = rng.integers(1, max_deg + 1, len(rows))
    rp = np.concatenate([[0], np.cumsum(d)]).astype(np.int32)
    col = rng.integers(0, col_hi or n, int(rp[-1])).astype(np.int32)
    return rp, col


# ---- the restatement -----------------------------------------------------------------------------------------------------------------

def test_a_graph_written_out_by_hand():
    #           row 0: -      row 1: 4, 1     row 2: -   row 3: 6     rows 4 .. 7: -
    rp = np.array([0, 0, 2, 2, 3, 3, 3, 3, 3], dtype=np.int32)
    col = np.array([4, 1, 6], dtype=np.int32)
    keep = np.zeros(8, np.uint8)
    keep[7] = 1
    nodes, new_id, [(rp_b, col_b)] = CR.compact([(rp, col)], keep)
    assert nodes.tolist() == [1, 3, 4, 6, 7] and new_id.tolist() == [-1, 0, -1, 1, 2, -1, 3, 4]
    assert rp_b.tolist() == [0, 2, 3, 3, 3, 3] and col_b.tolist() == [2, 0, 3]
    CR.check_properties([(rp, col)], keep, nodes, new_id, [(rp_b, col_b)])
    nodes, new_id, _ = CR.compact([(rp, col)])
    assert nodes.tolist() == [1, 3, 4, 6]


@pytest.mark.parametrize("n,rows,deg,graphs,with_keep", [(1, 1, 1, 1, False), (7, 3, 4, 1, True), (50, 10, 6, 2, True), (300, 40, 9, 3, False),
                                                         (300, 300, 3, 2, True), (64, 0, 1, 1, True), (64, 0, 1, 1, False)])
def test_reference_properties_on_small_graphs(n, rows, deg, graphs, with_keep):
    rng = np.random.default_rng(n * 31 + rows)
    gs = [_random_csr(rng, n, rows, deg) for _ in range(graphs)]
    keep = (rng.random(n) < 0.1).astype(np.uint8) if with_keep else None
    nodes, new_id, blocks = CR.compact(gs, keep)
    CR.check_properties(gs, keep, nodes, new_id, blocks)
    if rows == 0:
        assert len(nodes) == (int(keep.sum()) if with_keep else 0) and all(len(c) == 0 for _, c in blocks)
    if rows == n:
        assert np.array_equal(nodes, np.arange(n)) and all(np.array_equal(b[1], g[1]) for b, g in zip(blocks, gs)), "nothing to drop: the identity"
    # a bool keep, and a keep with other non-zero bytes, say the same
    if with_keep:
        for other in (keep.astype(bool), keep * 7):
            again = CR.compact(gs, other)
            assert np.array_equal(again[0], nodes) and np.array_equal(again[1], new_id)


def test_no_nodes_and_no_edges():
    e = np.zeros(0, np.int32)
    nodes, new_id, [(rp_b, col_b)] = CR.compact([(np.zeros(1, np.int32), e)])
    assert len(nodes) == 0 and len(new_id) == 0 and rp_b.tolist() == [0] and len(col_b) == 0
    nodes, new_id, [(rp_b, col_b)] = CR.compact([(np.zeros(6, np.int32), e)], np.array([0, 1, 0, 0, 1], np.uint8))
    assert nodes.tolist() == [1, 4] and new_id.tolist() == [-1, 0, -1, -1, 1] and rp_b.tolist() == [0, 0, 0] and len(col_b) == 0


def test_the_layered_case_keeps_the_seeds_and_every_hops_sources():
    """sample_ref's layered sampling as tcgnn_layers.sample_layers does it: the last layer's graph holds the seeds' rows, the one before it
    those of the seeds and of that hop's sources.  The kept set of the two graphs is the seeds plus every hop's sources - nothing else."""
    rp, col, _ = R.row_length_graph()
    n, E = len(rp) - 1, int(rp[-1])
    col = col[:E]
    seeds = np.array([3, 77, 1500, 2047])
    m1 = np.zeros(n, np.uint8)
    m1[seeds] = 1
    g1 = R.sample_neighbors(rp, col, 4, 21, m1)
    m0 = m1.copy()
    m0[g1[1]] = 1
    g0 = R.sample_neighbors(rp, col, 6, 22, m0)
    graphs = [(g0[0], g0[1]), (g1[0], g1[1])]
    nodes, new_id, blocks = CR.compact(graphs, m1)
    CR.check_properties(graphs, m1, nodes, new_id, blocks)
    assert np.array_equal(nodes, np.unique(np.concatenate([seeds, g1[1], g0[1]])))
    assert len(nodes) < n / 4, "the batch does not shrink the node set"
    # a sampled graph's eid serves its compact form: the full graph's columns of the kept edges are the compact columns' original ids
    for g, (rp_b, col_b) in zip((g0, g1), blocks):
        assert np.array_equal(nodes[col_b], col[g[2]])


# ---- the library, loaded on the CPU ---------------------------------------------------------------------------------------------------

INVALID_ARG, WORKSPACE = 1, 5   # TCGNN_ERR_INVALID_ARG, TCGNN_ERR_WORKSPACE (include/tcgnn.h)


@pytest.fixture(scope="module")
def C():
    import tcgnn_capi
    return tcgnn_capi


def test_library_exports_the_calls_and_the_abi_version_is_unchanged(C):
    for name in ("tcgnn_compact_workspace_bytes", "tcgnn_compact_begin", "tcgnn_compact_mark", "tcgnn_compact_count", "tcgnn_compact_nodes",
                 "tcgnn_compact_graph"):
        assert name in C.SIGNATURES and getattr(C.lib, name) is not None
    assert C.lib.tcgnn_abi_version() == 1


def test_workspace_query_is_positive_at_zero_and_monotone_in_the_nodes(C):
    sizes = []
    need = C._sz(0)
    for n in (0, 1, CR.SCAN_ROWS, CR.SCAN_ROWS + 1, 232965, 2449029, 2 ** 31 - 1):
        assert C.lib.tcgnn_compact_workspace_bytes(n, ctypes.byref(need)) == 0
        assert need.value % 256 == 0 and need.value > 0
        sizes.append(need.value)
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    assert sizes[5] < 4 * 2449029 // 100   # (the validation words and one partial sum per SCAN_ROWS nodes: far below a word per node)
    assert C.lib.tcgnn_compact_workspace_bytes(-1, ctypes.byref(need)) == INVALID_ARG
    assert C.lib.tcgnn_compact_workspace_bytes(5, None) == INVALID_ARG
    assert b"tcgnn_compact_workspace_bytes" in C.lib.tcgnn_last_error()


def test_every_refusal_that_precedes_a_launch(C):
    """No pointer below is ever dereferenced: the calls return before any launch (there is no device here).  The addresses are
    256-byte aligned numbers."""
    P, WS = 0x10000, 0x20000
    need = C._sz(0)
    assert C.lib.tcgnn_compact_workspace_bytes(100, ctypes.byref(need)) == 0
    kept = C._i32(-7)

    def begin(n=100, ws=WS, nbytes=need.value):
        return C.lib.tcgnn_compact_begin(n, ws, nbytes, None)

    def mark(rp=P, col=P, n=100, e=1000, keep=P, ws=WS, nbytes=need.value):
        return C.lib.tcgnn_compact_mark(rp, col, n, e, keep, ws, nbytes, None)

    def count(keep=P, n=100, new_id=P, ws=WS, nbytes=need.value, out=ctypes.byref(kept)):
        return C.lib.tcgnn_compact_count(keep, n, new_id, ws, nbytes, out, None)

    def nodes(new_id=P, n=100, m=10, out=P):
        return C.lib.tcgnn_compact_nodes(new_id, n, m, out, None)

    def graph(rp=P, col=P, new_id=P, nodes=P, n=100, m=10, e=1000, rp_b=P, col_b=P):
        return C.lib.tcgnn_compact_graph(rp, col, new_id, nodes, n, m, e, rp_b, col_b, None)

    assert begin(n=-1) == INVALID_ARG
    assert mark(rp=None) == INVALID_ARG and mark(col=None) == INVALID_ARG and mark(keep=None) == INVALID_ARG
    assert mark(n=-1) == INVALID_ARG and mark(e=-1) == INVALID_ARG
    assert mark(e=2 ** 31) == INVALID_ARG and b"int32" in C.lib.tcgnn_last_error()
    assert count(keep=None) == INVALID_ARG and count(new_id=None) == INVALID_ARG and count(out=None) == INVALID_ARG and count(n=-1) == INVALID_ARG
    for call in (begin, mark, count):
        assert call(ws=None) == WORKSPACE and call(nbytes=need.value - 1) == WORKSPACE and call(ws=WS + 4) == WORKSPACE and call(ws=WS + 128) == WORKSPACE
        assert b"tcgnn_compact_workspace_bytes" in C.lib.tcgnn_last_error()
    assert kept.value == -7
    assert nodes(new_id=None) == INVALID_ARG and nodes(out=None) == INVALID_ARG and nodes(n=-1) == INVALID_ARG and nodes(m=-1) == INVALID_ARG
    assert nodes(m=101) == INVALID_ARG
    assert graph(rp=None) == INVALID_ARG and graph(col=None) == INVALID_ARG and graph(new_id=None) == INVALID_ARG and graph(nodes=None) == INVALID_ARG
    assert graph(rp_b=None) == INVALID_ARG and graph(col_b=None) == INVALID_ARG
    assert graph(n=-1) == INVALID_ARG and graph(m=-1) == INVALID_ARG and graph(m=101) == INVALID_ARG and graph(e=-1) == INVALID_ARG
    assert graph(e=2 ** 31) == INVALID_ARG and b"int32" in C.lib.tcgnn_last_error()


# ---- the harness's flag ----------------------------------------------------------------------------------------------------------------

def test_batch_size_parses_and_is_refused_without_fanout_with_a_captured_epoch_and_below_one():
    import tcgnn_harness as H
    p = H.build_parser()
    assert p.parse_args([]).batch_size is None
    assert p.parse_args(["--fanout", "5,5", "--batch-size", "64"]).batch_size == 64
    with pytest.raises(SystemExit):
        p.parse_args(["--batch-size", "many"])
    assert H.parse_batch_size(None, None) is None and H.parse_batch_size(None, "5", hip_graph=True) is None
    assert H.parse_batch_size(64, "5,5") == 64 and H.parse_batch_size(1, [5]) == 1
    with pytest.raises(ValueError, match="--fanout"):
        H.parse_batch_size(64, None)
    with pytest.raises(ValueError, match="hip_graph"):
        H.parse_batch_size(64, "5", hip_graph=True)
    for b in (0, -3):
        with pytest.raises(ValueError, match=">= 1"):
            H.parse_batch_size(b, "5")
    # time_training refuses before it touches a tensor or the device
    for kw, match in (({"batch_size": 64}, "--fanout"), ({"batch_size": 64, "fanout": "5", "hip_graph": True}, "hip_graph"),
                      ({"batch_size": 0, "fanout": "5"}, ">= 1")):
        with pytest.raises(ValueError, match=match):
            H.time_training("sage", None, None, None, 16, 16, 4, 2, 1, **kw)


def test_epoch_orders_are_permutations_and_batch_seeds_keep_their_hops_apart():
    import tcgnn_harness as H
    a, b = H.epoch_order(1000, 3, 0), H.epoch_order(1000, 3, 1)
    assert sorted(a.tolist()) == list(range(1000)) and a.tolist() != b.tolist()
    assert a.tolist() == H.epoch_order(1000, 3, 0).tolist() and b.tolist() == H.epoch_order(1000, 2, 2).tolist()
    seeds = {H.batch_seed(s, e, i) + hop for s in (0, 1) for e in range(3) for i in range(50) for hop in range(8)}
    assert len(seeds) == 2 * 3 * 50 * 8
