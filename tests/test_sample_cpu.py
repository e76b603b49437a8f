"""Seeded neighbour sampling without a GPU: the numpy restatement (tests/sample_ref.py) against a brute force in Python integers, the
pinned hash stream, the uniformity of the selection on fixed inputs, and - through tcgnn_capi, which loads the library on the CPU -
the new symbols, the workspace query and every refusal that precedes a launch."""
import ctypes
import itertools

import numpy as np
import pytest

import sample_ref as R


# ---- the restatement -----------------------------------------------------------------------------------------------------------------

def test_h32_is_pinned():
    """three (seed, e) pairs as literal numbers: no later edit changes the stream silently"""
    assert int(R.h32(0, 0)) == 2802244911
    assert int(R.h32(1, 12345)) == 427416617
    assert int(R.h32(2 ** 63 + 5, 2 ** 31 - 2)) == 567597086
    assert int(R.words(1, 12345)) == (427416617 << 32) | 12345
    assert np.array_equal(R.h32(5, np.arange(3)), [int(R.h32(5, e)) for e in range(3)])


@pytest.mark.parametrize("d", [1, 2, 3, 7, 40])
def test_reference_against_brute_force_on_tiny_rows(d):
    lo = 11
    rp = np.array([0, lo, lo, lo + d, lo + d + 4], dtype=np.int32)   # a row before, an empty row, the row, a row behind
    col = np.arange(100, 100 + lo + d + 4, dtype=np.int32)
    for seed in (0, 1, 2 ** 63 + 5, -3):
        for k in sorted({0, 1, d - 1, d, d + 1}):
            rp_s, col_s, eid = R.sample_neighbors(rp, col, k, seed)
            want = np.concatenate([R.brute_force_row(seed, 0, lo, k), R.brute_force_row(seed, lo, d, k), R.brute_force_row(seed, lo + d, 4, k)]) if k else []
            assert eid.tolist() == [int(e) for e in want]
            assert np.array_equal(np.diff(rp_s), np.minimum(np.diff(rp), k)) and rp_s[0] == 0
            assert np.array_equal(col_s, col[eid]) and eid.dtype == np.int32 and rp_s.dtype == np.int32
            assert np.all(np.diff(eid) > 0)


def test_reference_mask_empty_graph_and_no_fanout():
    rp = np.array([0, 3, 3, 9, 10], dtype=np.int32)
    col = np.arange(10, dtype=np.int32)[::-1].copy()
    mask = np.array([1, 1, 0, 1], dtype=np.uint8)
    rp_s, col_s, eid = R.sample_neighbors(rp, col, 2, 5, mask)
    assert rp_s.tolist() == [0, 2, 2, 2, 3] and eid.tolist() == R.brute_force_row(5, 0, 3, 2) + [9]
    assert np.array_equal(R.sample_neighbors(rp, col, 2, 5, np.ones(4, np.uint8))[2], R.sample_neighbors(rp, col, 2, 5)[2])
    assert R.sample_neighbors(rp, col, 2, 5, np.zeros(4, np.uint8))[0].tolist() == [0] * 5
    rp_s, col_s, eid = R.sample_neighbors(rp, col, None, 5)
    assert np.array_equal(rp_s, rp) and np.array_equal(col_s, col) and np.array_equal(eid, np.arange(10))
    for empty in (np.zeros(1, np.int32), np.zeros(4, np.int32)):
        rp_s, col_s, eid = R.sample_neighbors(empty, np.zeros(0, np.int32), 3, 1)
        assert np.array_equal(rp_s, empty) and len(col_s) == 0 and len(eid) == 0


def test_the_selection_is_uniform_over_subsets_and_over_positions():
    """Conditions on fixed inputs, not measurements.  A row of 8 edges at positions 100..107, k = 3, seeds 0..11 199: the chi-square of
    the 56 subset counts must stay below 93.2 (the 0.999 quantile at 55 degrees of freedom) - this reference gives 49.71.  A row of
    1 000 edges at positions 5 000..5 999, k = 25, seeds 0..3 999: the chi-square of the inclusion counts, scaled by 1 / (1 - k / d),
    must stay below 1 143.9 (the 0.999 quantile at 999 degrees of freedom) - this reference gives 1 070.46."""
    counts = {}
    for seed in range(11200):
        kept = tuple(sorted(np.argsort(R.words(seed, np.arange(100, 108)))[:3].tolist()))
        counts[kept] = counts.get(kept, 0) + 1
    expect = 11200 / 56
    chi2 = sum((counts.get(c, 0) - expect) ** 2 / expect for c in itertools.combinations(range(8), 3))
    print("FIG chi2 of the 56 subsets: %.2f (bound 93.2)" % chi2)
    assert chi2 < 93.2
    inc = np.zeros(1000)
    for seed in range(4000):
        inc[np.argsort(R.words(seed, np.arange(5000, 6000)))[:25]] += 1
    expect = 4000 * 25 / 1000
    chi2 = float(((inc - expect) ** 2 / expect).sum() / (1 - 25 / 1000))
    print("FIG chi2 of the 1000 inclusion counts: %.2f (bound 1143.9)" % chi2)
    assert chi2 < 1143.9


def test_the_long_row_of_the_gpu_graph_has_two_equal_hashes_for_a_seed_below_sixteen():
    rp, col, long_row = R.row_length_graph()
    assert rp[long_row + 1] - rp[long_row] == R.LONG_ROW and len(col) == rp[-1] + R.NO_ROW
    found = R.equal_hash_pair(rp, long_row)
    assert found is not None
    seed, k = found
    w = np.sort(R.words(seed, np.arange(rp[long_row], rp[long_row + 1])))
    assert (w[k - 1] >> np.uint64(32)) == (w[k] >> np.uint64(32)) and w[k - 1] < w[k]


# ---- the library, loaded on the CPU ---------------------------------------------------------------------------------------------------

INVALID_ARG, WORKSPACE = 1, 5   # TCGNN_ERR_INVALID_ARG, TCGNN_ERR_WORKSPACE (include/tcgnn.h)


@pytest.fixture(scope="module")
def C():
    import tcgnn_capi
    return tcgnn_capi


def test_library_exports_the_sampler_and_the_abi_version_is_unchanged(C):
    for name in ("tcgnn_sample_workspace_bytes", "tcgnn_sample_neighbors_count", "tcgnn_sample_neighbors"):
        assert name in C.SIGNATURES and getattr(C.lib, name) is not None
    assert C.lib.tcgnn_abi_version() == 1
    assert C.lib.tcgnn_status_string(INVALID_ARG) == b"invalid argument" and C.lib.tcgnn_status_string(WORKSPACE) == b"workspace missing or too small"


def test_workspace_query_answers_and_grows_with_the_nodes(C):
    sizes = []
    for n in (0, 1, 2048, 232965, 2449029):
        need = C._sz(0)
        assert C.lib.tcgnn_sample_workspace_bytes(n, ctypes.byref(need)) == 0
        assert need.value % 256 == 0 and need.value >= 512
        sizes.append(need.value)
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1] < 4 * 2449030   # (the result words and the scan's partial sums: well below a word per node)
    assert C.lib.tcgnn_sample_workspace_bytes(-1, ctypes.byref(need)) == INVALID_ARG
    assert C.lib.tcgnn_sample_workspace_bytes(5, None) == INVALID_ARG
    assert b"tcgnn_sample_workspace_bytes" in C.lib.tcgnn_last_error()


def test_every_refusal_that_precedes_a_launch(C):
    """No pointer below is ever dereferenced: the calls return before any launch (there is no device here).  The addresses are
    256-byte aligned numbers."""
    P, WS = 0x10000, 0x20000
    kept = C._i64(-7)
    need = C._sz(0)
    assert C.lib.tcgnn_sample_workspace_bytes(100, ctypes.byref(need)) == 0
    ws_err = WORKSPACE

    def count(rp=P, mask=None, n=100, e=1000, k=5, rp_s=P, ws=WS, nbytes=need.value, out=ctypes.byref(kept)):
        return C.lib.tcgnn_sample_neighbors_count(rp, mask, n, e, k, rp_s, ws, nbytes, out, None)

    assert count(rp=None) == INVALID_ARG and count(rp_s=None) == INVALID_ARG and count(out=None) == INVALID_ARG
    assert count(n=-1) == INVALID_ARG and count(e=-1) == INVALID_ARG
    assert count(k=-1) == INVALID_ARG and b"fanout" in C.lib.tcgnn_last_error()
    assert count(e=2 ** 31) == INVALID_ARG and b"int32" in C.lib.tcgnn_last_error()
    assert count(ws=None) == ws_err and count(nbytes=need.value - 1) == ws_err and count(ws=WS + 4) == ws_err and count(ws=WS + 128) == ws_err
    assert kept.value == -7

    def select(rp=P, col=P, mask=None, rp_s=P, n=100, e=1000, k=5, seed=2 ** 64 - 1, col_s=P, eid=P):
        return C.lib.tcgnn_sample_neighbors(rp, col, mask, rp_s, n, e, k, seed, col_s, eid, None)

    assert select(rp=None) == INVALID_ARG and select(rp_s=None) == INVALID_ARG
    assert select(col=None) == INVALID_ARG and select(col_s=None) == INVALID_ARG and select(eid=None) == INVALID_ARG
    assert select(n=-1) == INVALID_ARG and select(e=-1) == INVALID_ARG and select(k=-1) == INVALID_ARG and select(e=2 ** 31) == INVALID_ARG
