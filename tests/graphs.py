"""Seeded synthetic CSR graphs shared by the tests, tools/ and bench.py (no reference data needed)."""
import numpy as np
import scipy.sparse as sp


def csr_from_edges(src, dst, n):
    """COO -> canonical CSR exactly like the reference's dataset.py:94-104 (duplicates merged,
    rows sorted); returns (rowptr int32[n+1], col int32[nnz])."""
    a = sp.coo_matrix((np.ones(len(src), dtype=np.int8), (src, dst)), shape=(n, n)).tocsr()
    a.sum_duplicates()
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32)


def uniform_graph(n, avg_deg, seed, symmetric=True):
    rng = np.random.default_rng(seed)
    m = int(n * avg_deg / (2 if symmetric else 1))
    src = rng.integers(0, n, size=m)
    dst = rng.integers(0, n, size=m)
    if symmetric:
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
    return csr_from_edges(src, dst, n)


def powerlaw_graph(n, avg_deg, seed, alpha=1.8, symmetric=True):
    """Degree-skewed graph: endpoints drawn with probability ~ rank^(-1/alpha)-like weights."""
    rng = np.random.default_rng(seed)
    m = int(n * avg_deg / (2 if symmetric else 1))
    w = (np.arange(1, n + 1, dtype=np.float64)) ** (-1.0 / alpha)
    w /= w.sum()
    perm = rng.permutation(n)
    src = perm[rng.choice(n, size=m, p=w)]
    dst = rng.integers(0, n, size=m)
    if symmetric:
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
    return csr_from_edges(src, dst, n)


def community_graph(n, blocks, avg_deg, p_in, seed):
    """Stochastic block model with consecutively numbered communities: a share p_in of the edges stays inside the endpoint's own
    block (the shape tcgnn_graph.sbm_csr builds at Reddit size: a few column ranges per window are DENSE, the rest sparse)."""
    rng = np.random.default_rng(seed)
    m = int(n * avg_deg / 2)
    src = rng.integers(0, n, size=m)
    size = (n + blocks - 1) // blocks
    inside = rng.random(m) < p_in
    dst_in = np.minimum((src // size) * size + rng.integers(0, size, size=m), n - 1)
    dst = np.where(inside, dst_in, rng.integers(0, n, size=m))
    return csr_from_edges(np.concatenate([src, dst]), np.concatenate([dst, src]), n)


def hub_rows_graph(n, seed, full_rows=24, half_rows=3, background=30000, bg_cols=None):
    """A few rows that are edges to every (or every second) column over a sparse uniform background, symmetrised: inside a hub's
    window a lane's run of edges within its eight tile columns is up to eight long (the edge-valued kernels fetch four values at a
    time), and the hub columns make every other window hold a dense column block."""
    rng = np.random.default_rng(seed)
    half = np.arange(0, n, 2)
    m = n if bg_cols is None else bg_cols   # (bg_cols: the background stays inside the first bg_cols nodes - the column ranges beyond hold hub edges only)
    src = [np.repeat(np.arange(full_rows), n), rng.integers(0, m, background), np.repeat(np.arange(1000, 1000 + half_rows), len(half))]
    dst = [np.tile(np.arange(n), full_rows), rng.integers(0, m, background), np.tile(half, half_rows)]
    s_, d_ = np.concatenate(src), np.concatenate(dst)
    keep = s_ != d_
    s_, d_ = s_[keep], d_[keep]
    return csr_from_edges(np.concatenate([s_, d_]), np.concatenate([d_, s_]), n)


def with_empty_window(rowptr, col, first_row, last_row):
    """Remove every edge of rows [first_row, last_row) (keeps the CSR canonical)."""
    n = len(rowptr) - 1
    a = sp.csr_matrix((np.ones(len(col), dtype=np.int8), col, rowptr), shape=(n, n)).tolil()
    a[first_row:last_row, :] = 0
    a = a.tocsr()
    a.eliminate_zeros()
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32)


def edge_case_graphs():
    """(name, rowptr, col) for the shapes the reference's quirks live at."""
    out = []
    for n, deg in ((1, 1), (15, 4), (16, 5), (17, 3), (32, 6), (40, 4), (1000, 10)):
        rp, c = uniform_graph(n, deg, seed=100 + n, symmetric=n > 1)
        out.append(("uniform_n%d" % n, rp, c))
    rp, c = uniform_graph(48, 3, seed=7)
    rp, c = with_empty_window(rp, c, 16, 32)
    out.append(("empty_middle_window_n48", rp, c))
    rp, c = powerlaw_graph(1000, 12, seed=11)
    out.append(("powerlaw_n1000", rp, c))
    out.append(("no_edges_n20", np.zeros(21, dtype=np.int32), np.zeros(0, dtype=np.int32)))
    return out


SHORT_METADATA_CUT = 40      # windows the `short_metadata` entry's blockPartition is handed over without
LDS_RANGE_ROWS = (504, 632, 760, 1528)   # rows of one LDS-resident column range, per layout (tcgnn_lds_spmm.inc)


def _unsorted_rows(rowptr, col, every=3, seed=21):
    """Every `every`-th row's columns permuted: unique, unsorted - a non-canonical CSR of the same graph."""
    rng = np.random.default_rng(seed)
    col = col.copy()
    for r in range(0, len(rowptr) - 1, every):
        col[rowptr[r]: rowptr[r + 1]] = rng.permutation(col[rowptr[r]: rowptr[r + 1]])
    return col


def boundary_graphs():
    """(name, rowptr, col): deterministic graphs that sit ON a boundary the plan builder or a kernel has a branch for (window, tile,
    cell and LDS-range edges, 16-bit edge offsets, empty and hub windows, E below the limits of the edge-valued paths).  What each is
    there for is pinned by tests/test_structures_cpu.py; tests/test_gpu_structures.py runs every walk over them.  Two entries are
    more than a CSR: `unsorted_rows_*` is not canonical, and `short_metadata_*` is handed to the kernels with its blockPartition cut
    by SHORT_METADATA_CUT windows."""
    out = []
    ar = np.arange
    # every window = exactly 4 full tiles (32 distinct columns: the flat stream's cell capacity), every mask byte 0xff
    n = 4096
    out.append(("block_diag_16x32_n4096", *csr_from_edges(np.repeat(ar(n), 32), (np.repeat(ar(n) // 16, 32) * 32 + np.tile(ar(32), n)) % n, n)))
    # columns on the first / last row of every LDS range size and on the last column; N % 16 = 9
    n = 3 * 1528 + 1
    marks = sorted({k * s + d for s in LDS_RANGE_ROWS for k in range(n // s + 2) for d in (-1, 0) if 0 <= k * s + d < n} | {n - 1})
    r, c = np.repeat(ar(n), len(marks)), np.tile(np.array(marks), n)
    keep = (r * 7 + c) % 3 != 0
    out.append(("range_boundary_columns_n4585", *csr_from_edges(r[keep], c[keep], n)))
    # one-column tiles on the first and the last record of the image
    n = 4101
    out.append(("two_hub_columns_n4101", *csr_from_edges(np.tile(ar(n), 2), np.concatenate([np.zeros(n, np.int64), np.full(n, n - 1)]), n)))
    # every window empty but the ragged last one (N % 16 = 1), which holds every column
    n = 4097
    out.append(("one_hub_row_last_n4097", *csr_from_edges(np.full(n, n - 1), ar(n), n)))
    # empty leading and trailing windows
    n = 4100
    rng = np.random.default_rng(5)
    out.append(("middle_rows_only_n4100", *csr_from_edges(rng.integers(1600, 1920, 40000), rng.integers(0, n, 40000), n)))
    # one edge per row
    n = 4103
    out.append(("identity_n4103", *csr_from_edges(ar(n), ar(n), n)))
    # strictly upper triangular band: asymmetric, last row empty, columns always ahead of the window
    n = 4100
    r = np.repeat(ar(n), 200); c = r + np.tile(ar(1, 201), n)
    out.append(("upper_band200_n4100", *csr_from_edges(r[c < n], c[c < n], n)))
    # 16 480 edges per window, all masks full
    n = 1030
    out.append(("complete_n1030", *csr_from_edges(np.repeat(ar(n), n), np.tile(ar(n), n), n)))
    # mask bytes 0x55 / 0xaa alternating by row
    n = 4100
    r = np.repeat(ar(n), 128); c = r - 64 + np.tile(ar(128), n)
    keep = (c >= 0) & (c < n) & ((r + c) % 2 == 0)
    out.append(("checkerboard_band128_n4100", *csr_from_edges(r[keep], c[keep], n)))
    # E = 1, in the far corner
    n = 5000
    out.append(("single_edge_corner_n5000", *csr_from_edges(np.array([n - 1]), np.array([n - 1]), n)))
    # window 0 holds 65 520 / 65 536 edges: either side of the 16-bit edge offsets of the edge-valued LDS-resident stream.  The
    # background is dense enough (~150 tiles per window against window 0's 512) that window 0 is no hub: a hub window is split
    # over wavefronts, and a plan with split windows keeps the gather walk for edge values before the offsets are ever cut
    for n in (4095, 4096):
        rng = np.random.default_rng(n)
        r = np.concatenate([np.repeat(ar(16), n), rng.integers(0, n, 360000)])
        c = np.concatenate([np.tile(ar(n), 16), rng.integers(0, n, 360000)])
        out.append(("sixteen_full_rows_n%d" % n, *csr_from_edges(r, c, n)))
    rp, col = uniform_graph(4100, 150, seed=21)
    out.append(("unsorted_rows_n4100", rp, _unsorted_rows(rp, col)))
    out.append(("short_metadata_n4100", rp, col))
    return out


def bucketed_boundary_graphs():
    """Entries large and dense enough for the plan's column-bucket table (at least 1 024 windows of 512 distinct columns on
    average: tcgnn_plan_create), which the range-blocked SpMM, the range-major SDDMM and the XCD-sliced fused AGNN walk need."""
    out = []
    ar = np.arange
    # row r -> the columns c = r (mod 16) of a band of 1 536: every condensed column holds ONE row of its window; N % 16 = 9
    n = 16409
    r = np.repeat(ar(n), 96); c = r - 768 + 16 * np.tile(ar(96), n)
    keep = (c >= 0) & (c < n)
    out.append(("one_row_per_column_band1536_n16409", *csr_from_edges(r[keep], c[keep], n)))
    # every other window empty, the rest 100 random columns per row (directed); N % 16 = 4
    n = 16500
    rng = np.random.default_rng(16500)
    rows = ar(n)[(ar(n) // 16) % 2 == 0]
    out.append(("every_other_window_empty_n16500", *csr_from_edges(np.repeat(rows, 100), rng.integers(0, n, 100 * len(rows)), n)))
    # 96 columns around every boundary of the eight column buckets (first and last column of the image included), an eighth per row
    n = 16500
    br = (n + 7) // 8
    marks = np.array(sorted({b * br + d for b in range(9) for d in range(-48, 48) if 0 <= b * br + d < n}))
    r, c = np.repeat(ar(n), len(marks)), np.tile(marks, n)
    keep = (r + c) % 8 == 0
    out.append(("bucket_boundary_columns_n16500", *csr_from_edges(r[keep], c[keep], n)))
    return out


def sync_boundary_graphs():
    """The two entries for the slice-synchronised walk, which needs 2 048 windows and a numbering with locality: the community graph
    test_slice_synchronised_walk... uses, (a) with every row of the fourth XCD's share of the windows emptied, (b) with one hub row
    (every 16th column: 2 501 edges, windows still alike enough for the walk's tables) and one hub column added."""
    rp, col = community_graph(40003, 16, 60, 0.9, seed=31)
    n = len(rp) - 1
    nwx = ((n + 15) // 16 + 7) // 8                      # windows per XCD (build_sync_tables)
    src = np.repeat(np.arange(n), np.diff(rp))
    keep = (src < 3 * nwx * 16) | (src >= 4 * nwx * 16)
    out = [("communities_empty_xcd_share_n40003", *csr_from_edges(src[keep], col[keep], n))]
    hub = 20011
    far = np.arange(0, n, 16)
    s = np.concatenate([src, np.full(len(far), hub), np.arange(n)]); d = np.concatenate([col, far, np.full(n, hub)])
    out.append(("communities_hub_row_and_column_n40003", *csr_from_edges(s, d, n)))
    return out


def host_sgt(rowptr, col, guard=0):
    """Run the product's host SGT through the C ABI (numpy in / numpy out)."""
    import ctypes
    import tcgnn_capi as c
    n = len(rowptr) - 1
    nw = (n + 15) // 16
    bp = np.zeros(nw + guard, dtype=np.int32)
    e2c = np.zeros(len(col), dtype=np.int32)
    e2r = np.zeros(len(col), dtype=np.int32)
    cnt = ctypes.c_int64(0)
    rp = np.ascontiguousarray(rowptr, dtype=np.int32)
    cl = np.ascontiguousarray(col, dtype=np.int32)
    st = c.lib.tcgnn_preprocess(cl.ctypes.data, rp.ctypes.data, n, 16, 8, bp.ctypes.data, nw, e2c.ctypes.data, e2r.ctypes.data,
                                ctypes.byref(cnt), 0)
    c.check(st, "tcgnn_preprocess")
    return bp, e2c, e2r, cnt.value
