"""What tests/long_range_graphs.py promises tests/test_gpu_long_ranges.py, checked without a GPU: the boundary records carry edges,
the cells overflow as announced, no window is a hub (a split window keeps the ordinary stream), some rows are empty, and the
oracle alone stays inside its share of the bounds on the new graphs too (as tests/test_structures_cpu.py asserts for its catalogue)."""
import numpy as np
import pytest

import graphs
import long_range_graphs as LG
import walks

ALL = {name: (rp, col) for name, rp, col in LG.catalogue()}


def _cell_columns(rp, col, rows_per_range):
    """[windows, ranges] distinct columns of every (window, range) cell"""
    n = len(rp) - 1
    nw, nr = (n + 15) // 16, (n + rows_per_range - 1) // rows_per_range
    out = np.zeros((nw, nr), np.int64)
    for w in range(nw):
        c = np.unique(col[rp[16 * w]:rp[min(16 * w + 16, n)]])
        out[w] = np.bincount(c // rows_per_range, minlength=nr)
    return out


@pytest.mark.parametrize("name", list(ALL))
def test_no_hub_window_and_some_empty_rows(name):
    rp, col = ALL[name]
    n = len(rp) - 1
    bp, _, _, _ = graphs.host_sgt(rp, col)
    assert int(bp.max()) * len(bp) <= 4 * int(bp.sum()), "a hub window: the plan would split it and keep the ordinary stream"
    deg = np.diff(rp)
    assert all(deg[r] == 0 for r in LG.EMPTY_ROWS if r < n)
    assert (deg > 0).sum() > n // 2


@pytest.mark.parametrize("name", [k for k in ALL if k.startswith("range_arithmetic")])
def test_range_arithmetic_graphs_touch_every_boundary_record(name):
    rp, col = ALL[name]
    n = len(rp) - 1
    used = np.zeros(n, bool); used[col] = True
    for r in range((n + LG.LONG_ROWS - 1) // LG.LONG_ROWS):
        for c in (r * LG.LONG_ROWS, r * LG.LONG_ROWS + LG.LONG_ROWS - 1):
            assert c >= n or used[c], (name, c)
    assert used[n - 1]                                   # the last record of the image, next to the sentinel
    # sizes: one range and sixteen rows; two ranges exactly (the sentinel row opens a range of its own); two and one row; five and
    # forty rows (both buffers wrap twice)
    assert n in (LG.LONG_ROWS + 16, 2 * LG.LONG_ROWS, 2 * LG.LONG_ROWS + 1, 5 * LG.LONG_ROWS + 40)


def test_pool_graphs_overflow_every_cell():
    rp, col = ALL["pool_every_cell_overflows_n4760"]
    cells = _cell_columns(rp, col, LG.LONG_ROWS)
    full = cells
    assert full.min() >= 40 and full.max() <= 60, (full.min(), full.max())
    rp, col = ALL["pool_long_lists_three_ranges_n2856"]
    cells = _cell_columns(rp, col, LG.LONG_ROWS)
    assert cells.shape[1] == 3
    cold_tiles = (np.maximum(cells - 32, 0).sum(1) + 31) // 32     # per window = per wavefront at this size (one window each)
    assert 8 <= np.median(cold_tiles) <= 12, np.median(cold_tiles)


def test_dense_blocks_hold_three_hundred_columns_in_one_range():
    rp, col = ALL["dense_blocks_n4800"]
    cells = _cell_columns(rp, col, LG.LONG_ROWS)
    for w0, nwin, r in ((40, 6, 1), (120, 24, 3)):
        blk = cells[w0:w0 + nwin]
        assert blk[:, r].min() >= 290, blk[:, r].min()
        others = np.delete(blk, r, axis=1)
        assert others.max() <= 64
    assert 24 > 16                                       # the long block cannot sit in one workgroup of sixteen windows


@pytest.mark.parametrize("name", list(ALL))
def test_oracle_alone_stays_inside_its_share_of_the_bounds(name):
    rp, col = ALL[name]
    for D in (64, 128):
        for op, (tight, bar, rounding) in walks.oracle_alone(name, rp, col, D).items():
            if op != "spmm":
                continue
            assert tight <= walks.NOISE_SHARE * walks.TIGHT, (name, D, op, tight)
            assert bar <= walks.NOISE_SHARE * walks.TOL, (name, D, op, bar)
            assert rounding <= walks.ROUNDING_SHARE * walks.LOOSE, (name, D, op, rounding)
        walks._REFS.clear()
