"""Subgraph sampling without a GPU: tests/subgraph_ref.py's restatement of random_walk and induce_subgraph against pure-Python-integer
walks and a per-edge loop; the pick rule's uniformity; the workspace query and every refusal of the C calls that precedes a launch;
the Python layer's argument checks; saint_node_norm; the harness's parsers, their old answers included."""
import ctypes

import numpy as np
import pytest
import torch

import sample_ref as R
import subgraph_ref as SG

M64 = (1 << 64) - 1


def _graph():
    rp, col, long_row = R.row_length_graph()
    return rp, col[:rp[-1]], long_row


def _h32_int(seed, i):
    """h32 from Python integers alone (no numpy arithmetic), as sample_ref.brute_force_row computes it"""
    def mx(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)
    s = mx((int(seed) % (1 << 64) + 0x9E3779B97F4A7C15) & M64)
    return mx((s + (int(i) + 1) * 0x9E3779B97F4A7C15) & M64) >> 32


def _walk_int(rp, col, start, w, length, seed):
    n, E = len(rp) - 1, len(col)
    walk = [int(start)]
    for t in range(length):
        v = walk[-1]
        if 0 <= v < n:
            lo, hi = min(max(int(rp[v]), 0), E), min(max(int(rp[v + 1]), 0), E)
            if hi - lo > 0:
                v = int(col[lo + ((_h32_int(seed, w * length + t) * (hi - lo)) >> 32)])
        walk.append(v)
    return walk


@pytest.mark.parametrize("seed", [0, 7, 2 ** 63 + 5, -3])
def test_the_restated_walk_equals_a_walk_in_python_integers(seed):
    rp, col, long_row = _graph()
    d = np.diff(rp.astype(np.int64))
    empty = int(np.nonzero(d == 0)[0][0])
    starts = np.concatenate([[long_row, empty, -1, len(rp) - 1, long_row], np.random.default_rng(1).integers(0, len(rp) - 1, 60)]).astype(np.int32)
    for length in (0, 1, 4, 16):
        walks = SG.random_walk(rp, col, starts, length, seed)
        assert walks.dtype == np.int32 and walks.shape == (len(starts), length + 1)
        for w, s in enumerate(starts):
            assert walks[w].tolist() == _walk_int(rp, col, s, w, length, seed), (w, length)
        assert np.all(walks[1] == empty) and np.all(walks[2] == -1) and np.all(walks[3] == len(rp) - 1)   # a stay; carried through unfollowed


def test_the_restated_induce_equals_a_loop_over_every_edge():
    rp, col, long_row = _graph()
    n = len(rp) - 1
    rng = np.random.default_rng(5)
    for nodes in (np.sort(rng.choice(n, 300, replace=False)), np.array([long_row]), np.zeros(0, np.int64), np.arange(n)):
        new_id = np.full(n, -1, np.int32)
        new_id[nodes] = np.arange(len(nodes), dtype=np.int32)
        rp_b, col_b, eid = SG.induce_subgraph(rp, col, nodes, new_id)
        want_rp, want_col, want_eid = [0], [], []
        for v in nodes:
            for e in range(int(rp[v]), int(rp[v + 1])):
                if new_id[col[e]] >= 0:
                    want_col.append(int(new_id[col[e]]))
                    want_eid.append(e)
            want_rp.append(len(want_col))
        assert rp_b.dtype == col_b.dtype == eid.dtype == np.int32
        assert rp_b.tolist() == want_rp and col_b.tolist() == want_col and eid.tolist() == want_eid


def test_induce_over_every_node_returns_the_graph_itself():
    rp, col, _ = _graph()
    n = len(rp) - 1
    rp_b, col_b, eid = SG.induce_subgraph(rp, col, np.arange(n), np.arange(n, dtype=np.int32))
    assert np.array_equal(rp_b, rp) and np.array_equal(col_b, col) and np.array_equal(eid, np.arange(len(col), dtype=np.int32))


def test_subgraph_batch_restated_takes_ids_in_any_order_with_repeats():
    rp, col, long_row = _graph()
    ids = np.array([[long_row, 5], [5, 0], [2047, long_row]])
    nodes, new_id, seed_pos, (rp_b, col_b), eid = SG.subgraph_batch(rp, col, ids)
    assert nodes.tolist() == sorted({long_row, 5, 0, 2047}) and seed_pos.dtype == np.int64 and seed_pos.shape == (6,)
    assert np.array_equal(nodes[seed_pos], ids.reshape(-1)) and len(rp_b) == len(nodes) + 1 and rp_b[-1] == len(col_b) == len(eid)
    assert np.all(np.isin(col[eid], nodes)) and np.array_equal(nodes[col_b], col[eid])
    walks = SG.random_walk(rp, col, np.array([long_row, 5]), 2, 9)
    a, b = SG.saint_batch(rp, col, np.array([long_row, 5]), 2, 9), SG.subgraph_batch(rp, col, walks)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


@pytest.mark.parametrize("seed", [0, 1, 2, 12345])
@pytest.mark.parametrize("d,bound", [(7, 22.46), (64, 103.4)], ids=["d7", "d64"])
def test_the_pick_rule_is_uniform(d, bound, seed):
    """chi-square of j = (h32(seed, i) * d) >> 32 over i = 0 .. 279 999 against the 99.9 % point of chi^2 with d - 1 degrees of freedom"""
    n = 280000
    j = SG.pick(seed, np.arange(n, dtype=np.uint64), np.full(n, d)).astype(np.int64)
    assert j.min() >= 0 and j.max() < d
    seen = np.bincount(j, minlength=d).astype(np.float64)
    chi2 = float(((seen - n / d) ** 2 / (n / d)).sum())
    print("d = %d, seed = %d: chi^2 = %.2f (bound %.2f)" % (d, seed, chi2, bound))
    assert chi2 < bound


# ---- the library, loaded on the CPU ---------------------------------------------------------------------------------------------------

INVALID_ARG, WORKSPACE = 1, 5   # TCGNN_ERR_INVALID_ARG, TCGNN_ERR_WORKSPACE (include/tcgnn.h)


@pytest.fixture(scope="module")
def C():
    import tcgnn_capi
    return tcgnn_capi


def test_library_exports_the_calls_and_the_abi_version_is_unchanged(C):
    for name in ("tcgnn_random_walk", "tcgnn_induce_workspace_bytes", "tcgnn_induce_count", "tcgnn_induce"):
        assert name in C.SIGNATURES and getattr(C.lib, name) is not None
    assert C.lib.tcgnn_abi_version() == 1


@pytest.mark.parametrize("num_kept", [0, 1, 1023, 1024, 1025, 1024 * 256 + 1])
def test_induce_workspace_query_without_a_device(C, num_kept):
    need = C._sz(0)
    assert C.lib.tcgnn_induce_workspace_bytes(num_kept, ctypes.byref(need)) == 0
    assert need.value == SG.workspace_bytes(num_kept) and need.value % 256 == 0
    assert C.lib.tcgnn_induce_workspace_bytes(-1, ctypes.byref(need)) == INVALID_ARG
    assert C.lib.tcgnn_induce_workspace_bytes(num_kept, None) == INVALID_ARG
    assert b"tcgnn_induce_workspace_bytes" in C.lib.tcgnn_last_error()


def test_every_refusal_that_precedes_a_launch(C):
    """No pointer below is ever dereferenced: the calls return before any launch (there is no device here)."""
    P, WS = 0x10000, 0x20000
    need = C._sz(0)
    assert C.lib.tcgnn_induce_workspace_bytes(10, ctypes.byref(need)) == 0
    kept = C._i64(-7)

    def walk(rp=P, col=P, starts=P, w=10, n=100, e=1000, length=2, walks=P):
        return C.lib.tcgnn_random_walk(rp, col, starts, w, n, e, length, 0, walks, None)

    def count(rp=P, col=P, nodes=P, new_id=P, m=10, n=100, e=1000, rp_b=P, ws=WS, nbytes=need.value, out=ctypes.byref(kept)):
        return C.lib.tcgnn_induce_count(rp, col, nodes, new_id, m, n, e, rp_b, ws, nbytes, out, None)

    def induce(rp=P, col=P, nodes=P, new_id=P, rp_b=P, m=10, n=100, e=1000, eb=30, col_b=P, eid=P):
        return C.lib.tcgnn_induce(rp, col, nodes, new_id, rp_b, m, n, e, eb, col_b, eid, None)

    assert walk(rp=None) == INVALID_ARG and walk(col=None) == INVALID_ARG and walk(starts=None) == INVALID_ARG and walk(walks=None) == INVALID_ARG
    assert walk(w=-1) == INVALID_ARG and walk(n=-1) == INVALID_ARG and walk(e=-1) == INVALID_ARG and walk(length=-1) == INVALID_ARG
    assert b"tcgnn_random_walk" in C.lib.tcgnn_last_error()
    assert walk(e=2 ** 31) == INVALID_ARG and b"int32" in C.lib.tcgnn_last_error()
    assert walk(w=2 ** 30, length=1) == INVALID_ARG and b"2^31 - 1" in C.lib.tcgnn_last_error()   # 2^31 entries
    assert walk(w=2 ** 31 - 1, length=1) == INVALID_ARG and walk(w=3, length=2 ** 31 - 1) == INVALID_ARG
    assert count(rp=None) == INVALID_ARG and count(col=None) == INVALID_ARG and count(nodes=None) == INVALID_ARG and count(new_id=None) == INVALID_ARG
    assert count(rp_b=None) == INVALID_ARG and count(out=None) == INVALID_ARG
    assert count(m=-1) == INVALID_ARG and count(n=-1) == INVALID_ARG and count(e=-1) == INVALID_ARG and count(m=101) == INVALID_ARG
    assert count(e=2 ** 31) == INVALID_ARG and b"int32" in C.lib.tcgnn_last_error()
    assert count(ws=None) == WORKSPACE and count(nbytes=need.value - 1) == WORKSPACE and count(ws=WS + 4) == WORKSPACE and count(ws=WS + 128) == WORKSPACE
    assert b"tcgnn_induce_workspace_bytes" in C.lib.tcgnn_last_error()
    assert kept.value == -7
    assert induce(rp=None) == INVALID_ARG and induce(col=None) == INVALID_ARG and induce(nodes=None) == INVALID_ARG and induce(new_id=None) == INVALID_ARG
    assert induce(rp_b=None) == INVALID_ARG and induce(col_b=None) == INVALID_ARG and induce(eid=None) == INVALID_ARG
    assert induce(m=-1) == INVALID_ARG and induce(n=-1) == INVALID_ARG and induce(e=-1) == INVALID_ARG and induce(eb=-1) == INVALID_ARG
    assert induce(m=101) == INVALID_ARG
    assert induce(e=2 ** 31) == INVALID_ARG and b"int32" in C.lib.tcgnn_last_error()
    # nothing to write: answered without a launch (and without a device)
    assert induce(m=0, nodes=None) == 0 and induce(eb=0, col_b=None, eid=None) == 0 and induce(e=0, col=None) == 0
    assert walk(w=0, starts=None, walks=None) == 0


# ---- the Python layer's argument checks (they precede every device call) -----------------------------------------------------------------

def test_the_module_refuses_wrong_dtypes_and_devices():
    import TCGNN as T
    i32 = torch.zeros(4, dtype=torch.int32)
    for call in (lambda: T.random_walk(i32, i32, i32, 2, 0), lambda: T.induce_subgraph(i32, i32, i32, i32)):   # CPU tensors: the calls are for the device
        with pytest.raises(RuntimeError, match="CUDA"):
            call()
    for call in (lambda: T.random_walk(None, i32, i32, 2, 0), lambda: T.random_walk(i32, i32, [0, 1], 2, 0),
                 lambda: T.induce_subgraph(i32, i32, [0, 1], i32), lambda: T.induce_subgraph(i32, i32, i32, None)):
        with pytest.raises(TypeError):
            call()
    i64, u8 = torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.uint8)
    for call in (lambda: T.random_walk(i32, i32, i64, 2, 0), lambda: T.random_walk(i64, i32, i32, 2, 0), lambda: T.random_walk(i32, u8, i32, 2, 0),
                 lambda: T.induce_subgraph(i32, i32, i64, i32), lambda: T.induce_subgraph(i32, i32, i32, i64), lambda: T.induce_subgraph(i32, i64, i32, i32)):
        with pytest.raises(RuntimeError, match="expected scalar type Int"):
            call()
    with pytest.raises(ValueError, match="length"):
        T.random_walk(i32, i32, i32, -1, 0)
    for name in ("random_walk", "induce_subgraph"):
        assert name in T.__all__


def test_saint_node_norm_is_its_formula_zero_counts_included():
    import tcgnn_layers as L
    counts = torch.tensor([0, 1, 3, 0, 8, 2], dtype=torch.float32)
    got = L.saint_node_norm(counts, 8)
    want = torch.tensor([8 / 0.1 / 6, 8 / 1 / 6, 8 / 3 / 6, 8 / 0.1 / 6, 8 / 8 / 6, 8 / 2 / 6], dtype=torch.float64)
    assert got.dtype == torch.float32 and got.shape == (6,)
    assert torch.allclose(got.double(), want, rtol=1e-6, atol=0)
    assert torch.equal(got, L.saint_node_norm(counts.long(), 8))   # integer counts are taken too
    assert torch.isfinite(got).all()


def test_the_harness_parsers_keep_their_answers_and_take_the_new_samplers():
    import tcgnn_harness as H
    p = H.build_parser()
    assert p.parse_args([]).sampler == "dense" and p.parse_args([]).walk_length == 2 and p.parse_args([]).saint_norm == 0
    a = p.parse_args(["--batch-size", "64", "--sampler", "saint", "--walk-length", "3", "--saint-norm", "8"])
    assert (a.sampler, a.batch_size, a.walk_length, a.saint_norm, a.fanout) == ("saint", 64, 3, 8, None)
    assert p.parse_args(["--batch-size", "256", "--sampler", "cluster"]).sampler == "cluster"
    with pytest.raises(SystemExit):
        p.parse_args(["--sampler", "sparse"])
    # old answers
    assert H.parse_sampler("dense", None) == "dense" and H.parse_sampler("dense", 64) == "dense" and H.parse_sampler("rows", 64) == "rows"
    with pytest.raises(ValueError, match="--batch-size"):
        H.parse_sampler("rows", None)
    with pytest.raises(ValueError, match="dense"):
        H.parse_sampler("list", 64)
    assert H.parse_batch_size(None, None) is None and H.parse_batch_size(None, [5]) is None and H.parse_batch_size(64, [5, 5]) == 64
    with pytest.raises(ValueError, match="--fanout"):
        H.parse_batch_size(64, None)
    with pytest.raises(ValueError, match="hip_graph"):
        H.parse_batch_size(64, [5], True)
    with pytest.raises(ValueError, match=">= 1"):
        H.parse_batch_size(0, [5])
    # new ones
    for s in ("saint", "cluster"):
        assert H.parse_sampler(s, 64) == s and H.parse_batch_size(64, None, sampler=s) == 64
        with pytest.raises(ValueError, match="--batch-size"):
            H.parse_sampler(s, None)
        with pytest.raises(ValueError, match="--batch-size"):
            H.parse_batch_size(None, None, sampler=s)
        with pytest.raises(ValueError, match="--fanout"):
            H.parse_batch_size(64, [5, 5], sampler=s)
        with pytest.raises(ValueError, match="hip_graph"):
            H.parse_batch_size(64, None, True, sampler=s)
        with pytest.raises(ValueError, match=">= 1"):
            H.parse_batch_size(0, None, sampler=s)
    assert H.parse_walk_length(0) == 0 and H.parse_walk_length(4) == 4
    with pytest.raises(ValueError, match="--walk-length"):
        H.parse_walk_length(-1)
    # time_training refuses before it touches a tensor or the device
    for kw, match in (({"sampler": "saint"}, "--batch-size"), ({"sampler": "cluster"}, "--batch-size"),
                      ({"sampler": "saint", "batch_size": 64, "fanout": "5"}, "--fanout"), ({"sampler": "cluster", "batch_size": 64, "fanout": "5,5"}, "--fanout"),
                      ({"sampler": "saint", "batch_size": 64, "walk_length": -1}, "--walk-length"),
                      ({"sampler": "dense", "saint_norm": 4}, "--saint-norm"), ({"sampler": "saint", "batch_size": 64, "saint_norm": -1}, "--saint-norm")):
        with pytest.raises(ValueError, match=match):
            H.time_training("sage", None, None, None, 16, 16, 4, 2, 1, **kw)
