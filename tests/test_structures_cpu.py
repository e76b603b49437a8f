"""Pins the catalogue of boundary-shaped graphs (graphs.boundary_graphs / bucketed_boundary_graphs / sync_boundary_graphs) to the
boundaries it is there for, so that it cannot drift away from them, and checks that the ORACLE ALONE stays well inside the
project's bounds on every entry - a quarter of the two accumulation-noise bounds, half of the fp64 bound - so that what
tests/test_gpu_structures.py measures is the kernels.  Plan-free: CSR, host SGT and oracle only, no GPU."""
import numpy as np
import pytest

import graphs
import walks

SMALL = graphs.boundary_graphs()
BUCKETED = graphs.bucketed_boundary_graphs()
SYNC = graphs.sync_boundary_graphs()
ALL = {name: (rp, col) for name, rp, col in SMALL + BUCKETED + SYNC}


def _facts(name):
    rp, col = ALL[name]
    n = len(rp) - 1
    nw = (n + 15) // 16
    bp, e2c, e2r, _ = graphs.host_sgt(rp, col)
    wp = rp[np.minimum(np.arange(nw + 1) * 16, n)]
    return dict(rp=rp, col=col, n=n, nw=nw, bp=bp, e2c=e2c, e2r=e2r, win_edges=np.diff(wp), deg=np.diff(rp), wp=wp)


def _distinct_columns(f, w):
    return len(np.unique(f["col"][f["wp"][w]: f["wp"][w + 1]]))


def test_names_are_unique_and_every_entry_is_valid_input():
    names = [g[0] for g in SMALL + BUCKETED + SYNC]
    assert len(set(names)) == len(names) and len(SMALL) == 14 and len(BUCKETED) == 3 and len(SYNC) == 2
    for name, (rp, col) in ALL.items():
        n = len(rp) - 1
        assert rp.dtype == np.int32 and col.dtype == np.int32 and rp[0] == 0 and rp[-1] == len(col) and np.all(np.diff(rp) >= 0), name
        assert len(col) == 0 or (col.min() >= 0 and col.max() < n), name
        for r in range(0, n, max(1, n // 97)):                     # unique columns inside a row (sorted too, unless the entry says otherwise)
            row = col[rp[r]: rp[r + 1]]
            assert len(np.unique(row)) == len(row), (name, r)
        sorted_rows = bool(np.all((np.diff(col) > 0) | np.isin(np.arange(1, len(col)), rp)))
        assert sorted_rows == (not walks.is_unsorted(name)), name
    # deterministic
    for (a, rp, col), (b, rp2, col2) in zip(SMALL, graphs.boundary_graphs()):
        assert a == b and np.array_equal(rp, rp2) and np.array_equal(col, col2)


def test_block_diag_windows_are_four_full_tiles():
    f = _facts("block_diag_16x32_n4096")
    assert f["n"] % 16 == 0 and np.all(f["win_edges"] == 512) and np.all(f["bp"] == 4)
    assert all(_distinct_columns(f, w) == 32 for w in range(f["nw"]))       # = kCellWords, the flat stream's cell capacity
    assert np.all(f["deg"] == 32)                                               # every mask bit of every tile set
    assert f["col"].max() == f["n"] - 1 and f["col"].min() == 0


def test_range_boundary_columns_sit_on_every_range_size():
    f = _facts("range_boundary_columns_n4585")
    n = f["n"]
    assert n == 3 * 1528 + 1 and n % 16 == 9
    used = set(np.unique(f["col"]).tolist())
    for s in graphs.LDS_RANGE_ROWS:
        for k in range(1, (n - 1) // s + 1):
            assert k * s - 1 in used and k * s in used, (s, k)              # last row of one range, first of the next
    assert 0 in used and n - 1 in used                                          # first record; the last one, next to the sentinel
    assert f["deg"].min() > 0


def test_hub_and_empty_window_entries():
    f = _facts("two_hub_columns_n4101")
    assert f["n"] % 16 == 5 and np.all(f["deg"] == 2) and set(np.unique(f["col"])) == {0, f["n"] - 1} and np.all(f["bp"] == 1)
    f = _facts("one_hub_row_last_n4097")
    assert f["n"] % 16 == 1 and np.all(f["win_edges"][:-1] == 0) and f["win_edges"][-1] == f["n"] and f["bp"][-1] == 513
    assert np.array_equal(f["col"], np.arange(f["n"]))
    f = _facts("middle_rows_only_n4100")
    first, last = np.flatnonzero(f["win_edges"])[[0, -1]]
    assert (first, last) == (100, 119) and np.all(f["win_edges"][100:120] > 0)
    f = _facts("identity_n4103")
    assert f["n"] % 16 == 7 and np.all(f["deg"] == 1) and np.all(f["bp"][:-1] == 2) and f["bp"][-1] == 1
    f = _facts("upper_band200_n4100")
    src = np.repeat(np.arange(f["n"]), f["deg"])
    assert np.all(f["col"] > src) and f["deg"][-1] == 0 and f["deg"][0] == 200 and not walks.is_symmetric(f["rp"], f["col"])
    f = _facts("single_edge_corner_n5000")
    assert len(f["col"]) == 1 and f["col"][0] == f["n"] - 1 and f["deg"][-1] == 1 and np.count_nonzero(f["win_edges"]) == 1


def test_dense_entries():
    f = _facts("complete_n1030")
    assert np.all(f["win_edges"][:-1] == 16480) and f["win_edges"][:-1].min() > 9216      # (two windows' edges: beyond kValSpanHalves = 18 432)
    assert np.all(f["deg"] == f["n"])
    f = _facts("checkerboard_band128_n4100")
    src = np.repeat(np.arange(f["n"]), f["deg"])
    assert np.all((src + f["col"]) % 2 == 0) and f["deg"].max() == 64
    w = 100                                                                                 # an inner window: a column holds the even or the odd rows
    cols = f["col"][f["wp"][w]: f["wp"][w + 1]]; rows = src[f["wp"][w]: f["wp"][w + 1]]
    for c in np.unique(cols)[16:-16]:
        assert sorted((rows[cols == c] % 16).tolist()) == list(range(c % 2, 16, 2))          # mask 0x5555 / 0xaaaa
    for n, edges in ((4095, 65520), (4096, 65536)):
        f = _facts("sixteen_full_rows_n%d" % n)
        assert f["win_edges"][0] == edges and (edges >= 65535) == (n == 4096)                 # either side of the 16-bit edge offsets
        assert not walks.is_symmetric(f["rp"], f["col"])
        assert f["bp"][0] == 512 and f["bp"].max() * f["nw"] <= 4 * f["bp"].sum()            # window 0 is no hub (lds_has_hubs): it is not split


def test_metadata_variants_share_one_graph():
    a, b = _facts("unsorted_rows_n4100"), _facts("short_metadata_n4100")
    assert np.array_equal(a["rp"], b["rp"]) and not np.array_equal(a["col"], b["col"])
    for r in (0, 3, 3000):
        assert np.array_equal(np.sort(a["col"][a["rp"][r]: a["rp"][r + 1]]), b["col"][b["rp"][r]: b["rp"][r + 1]])
    assert walks.windows_handed_over("short_metadata_n4100", b["n"]) * 16 == b["n"] - 4 - 39 * 16 and b["n"] % 16 == 4
    assert b["win_edges"][-graphs.SHORT_METADATA_CUT:].min() > 0          # the windows that are cut off are not empty ones
    assert b["bp"].sum() > 8192                                            # above kSmallMaxTiles: the forced walks are real


def test_bucketed_and_sync_entries_reach_their_walks():
    for name, _, _ in BUCKETED + SYNC:
        f = _facts(name)
        wide = (f["bp"] + 3) // 4                      # >= the plan's wide blocks (32 condensed columns each)
        assert f["nw"] >= 1024 and wide.sum() >= 20 * f["nw"], name        # the bucket table wants 16 per window on average
    f = _facts("one_row_per_column_band1536_n16409")
    w = 500
    cols = f["col"][f["wp"][w]: f["wp"][w + 1]]
    assert f["n"] % 16 == 9 and len(np.unique(cols)) == len(cols)                              # one row per condensed column
    f = _facts("every_other_window_empty_n16500")
    assert np.all(f["win_edges"][1::2] == 0) and np.all(f["win_edges"][0::2] > 0)
    f = _facts("bucket_boundary_columns_n16500")
    used = set(np.unique(f["col"]).tolist()); br = (f["n"] + 7) // 8
    assert all(b * br - 1 in used and b * br in used for b in range(1, 8)) and 0 in used and f["n"] - 1 in used
    f = _facts("communities_empty_xcd_share_n40003")
    nwx = (f["nw"] + 7) // 8
    assert f["nw"] >= 2048 and np.all(f["win_edges"][3 * nwx: 4 * nwx] == 0) and np.all(f["win_edges"][: 3 * nwx] > 0)
    f = _facts("communities_hub_row_and_column_n40003")
    src = np.repeat(np.arange(f["n"]), f["deg"])
    assert np.count_nonzero(f["col"] == 20011) == f["n"] and np.count_nonzero(src == 20011) >= 2501
    wide = (f["bp"] + 3) // 4
    assert wide.max() * f["nw"] <= 8 * wide.sum()                           # windows still "alike" (windows_balanced): the walk's tables get built


@pytest.mark.parametrize("name", [g[0] for g in SMALL + BUCKETED + SYNC])
def test_oracle_alone_stays_inside_its_share_of_the_bounds(name):
    """Accumulation noise (TF32-mode oracle against fp64 on the same rounded operands) at most a quarter of TIGHT and of TOL; operand
    rounding (against the fp64 contract) at most half of 2^-9.  A kernel then has three quarters of the bound to itself."""
    rp, col = ALL[name]
    for D in (16, 64, 128):
        for op, (tight, bar, rounding) in walks.oracle_alone(name, rp, col, D).items():
            assert tight <= walks.NOISE_SHARE * walks.TIGHT, (name, D, op, tight)
            assert bar <= walks.NOISE_SHARE * walks.TOL, (name, D, op, bar)
            assert rounding <= walks.ROUNDING_SHARE * walks.LOOSE, (name, D, op, rounding)
        walks._REFS.clear()
