"""Graphs for the long flat walk (952-row LDS ranges, cell stream slot 7 of tcgnn_lds_spmm.inc): tests/test_gpu_long_ranges.py runs them,
tests/test_long_ranges_cpu.py pins what each is there for.  Seeded, a few thousand rows each; built on tests/graphs.py."""
import numpy as np

import graphs

LONG_ROWS = 952          # data rows of one long range (960-row buffers less the eight zero rows)
SHIPPED_ROWS = 760       # the shipped layout of whole 64-column chunks
EMPTY_ROWS = (17, 18, 19, 20, 33)   # rows every graph here leaves without edges


def _finish(src, dst, n):
    """CSR of the directed edges src -> dst with EMPTY_ROWS (those below n) left empty."""
    keep = ~np.isin(src, np.array(EMPTY_ROWS))
    return graphs.csr_from_edges(src[keep], dst[keep], n)


def range_arithmetic_graph(n, seed):
    """A light background, plus edges - from eight rows spread over the graph and from the column's own window - to local rows 0 and
    951 of every 952-row range and to the last record of the image (column n - 1, next to the sentinel row)."""
    rng = np.random.default_rng(seed)
    m = 6 * n
    src, dst = [rng.integers(0, n, size=m)], [rng.integers(0, n, size=m)]
    targets = [c for r in range((n + LONG_ROWS - 1) // LONG_ROWS) for c in (r * LONG_ROWS, r * LONG_ROWS + LONG_ROWS - 1) if c < n] + [n - 1]
    for c in targets:
        rows = np.unique(np.concatenate([rng.integers(0, n, size=8), [min(c, n - 1), 0, n - 1]]))
        src.append(rows); dst.append(np.full(len(rows), c))
    return _finish(np.concatenate(src), np.concatenate(dst), n)


def overflowing_cells_graph(n, cols_per_cell, seed):
    """Every 16-row window holds about cols_per_cell distinct columns in EVERY 952-row range: each cell overflows its one 32-column
    tile, so every wavefront has cold tiles from the first entry on."""
    rng = np.random.default_rng(seed)
    nranges = (n + LONG_ROWS - 1) // LONG_ROWS
    nw = (n + 15) // 16
    src, dst = [], []
    for w in range(nw):
        rows = np.arange(16 * w, min(16 * w + 16, n))
        rows = rows[~np.isin(rows, np.array(EMPTY_ROWS))]
        for r in range(nranges):
            lo, hi = r * LONG_ROWS, min((r + 1) * LONG_ROWS, n)
            k = min(cols_per_cell, hi - lo)
            cols = lo + rng.choice(hi - lo, size=k, replace=False)
            # every chosen column gets one or two edges from the window's rows
            src.append(rng.choice(rows, size=k)); dst.append(cols)
            src.append(rng.choice(rows, size=k // 2)); dst.append(cols[: k // 2])
    return _finish(np.concatenate(src), np.concatenate(dst), n)


def dense_blocks_graph(n, seed, blocks=((40, 6, 1), (120, 24, 3))):
    """A light background and blocks of windows (first window, windows, range) whose every window holds about 300 distinct columns
    of ONE 952-row range: dense entries behind that range's normal entry.  The second block is longer than a workgroup of this size
    holds windows (lds_workgroups: at most sixteen below 2 048 windows), so it straddles two workgroups."""
    rng = np.random.default_rng(seed)
    m = 8 * n
    src, dst = [rng.integers(0, n, size=m)], [rng.integers(0, n, size=m)]
    for w0, nwin, r in blocks:
        lo, hi = r * LONG_ROWS, min((r + 1) * LONG_ROWS, n)
        for w in range(w0, w0 + nwin):
            rows = np.arange(16 * w, 16 * w + 16)
            cols = lo + rng.choice(hi - lo, size=300, replace=False)
            src.append(rng.choice(rows, size=300)); dst.append(cols)
            src.append(rng.choice(rows, size=300)); dst.append(cols)
    return _finish(np.concatenate(src), np.concatenate(dst), n)


def catalogue():
    """[(name, rowptr, col)]"""
    out = []
    for n in (LONG_ROWS + 16, 2 * LONG_ROWS, 2 * LONG_ROWS + 1, 5 * LONG_ROWS + 40):
        out.append(("range_arithmetic_n%d" % n, *range_arithmetic_graph(n, seed=100 + n % 97)))
    out.append(("pool_every_cell_overflows_n4760", *overflowing_cells_graph(5 * LONG_ROWS, 50, seed=7)))
    out.append(("pool_long_lists_three_ranges_n2856", *overflowing_cells_graph(3 * LONG_ROWS, 140, seed=8)))
    out.append(("dense_blocks_n4800", *dense_blocks_graph(4800, seed=9)))
    return out
