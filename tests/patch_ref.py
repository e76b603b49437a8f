"""What tests/test_patch_ref_cpu.py and tests/test_gpu_patch_edges.py share: inputs on which a missing or a doubled patch of the range
guard (wide_patch_kernel, tcgnn_small_fallback.inc) is visible edge by edge, numpy mirrors of the staging rule that decides what is
patched, and the references.  No GPU needed to import.

The data: X = N(0, 1) x 2^14 with |x| < 1 set to 1, and in every DIRTY row ALL D elements N(0, 1) x max|X| x 2^-42.  Such a row is
nonzero in fp32 and (but for a one-in-ten-thousand element beyond four sigma) exactly zero in the fp16 image, whose one scale puts
max|X| into [2^14, 2^15): the MFMA kernels score every edge that touches a dirty row 0, the patch writes the whole value - an edge
the patch skipped misses by its own sum of |terms|, one whose correction was added twice doubles its row of Y.

The mirrors follow tcgnn_stage.inc by name: scale_exp_from_bits, is_tiny, to_half_rna + the fp16 cast (image), range_is_wide with the
cap and the power of guard_sddmm, tcgnn_range_mode.  The dirty rows, the touched edges and the mode a call must report are computed
from them, never assumed."""
import numpy as np
import scipy.sparse as sp

import graphs
import walks as W
from oracle import oracle as O

TIGHT = W.TIGHT
SCORE_BOUND = 4 * TIGHT          # a score against the oracle, relative to the edge's own sum of |terms| (test_a_few_lost_elements_are_patched...)
AGG_BOUND = 256 * TIGHT          # an element of Y / G, relative to its own sum of |terms| (the same test)
DW_BOUND = 1e-5                  # d_w, relative to the sum of |terms| + 1 (the same test)
FP16_MIN_NORMAL = np.float32(6.103515625e-5)
W_ATT = np.float32(0.75)


# ---- the staging rule (tcgnn_stage.inc) ------------------------------------------------------------------------------------------
def bits(x):
    return int(np.float32(x).view(np.uint32))


def scale_exp_from_bits(b):
    """k with absmax * 2^k in [2^14, 2^15); 0 for zero / non-finite data"""
    if b == 0 or b >= 0x7f800000:
        return 0
    return int(np.clip(14 - ((b >> 23) - 127), -126, 126))


def scale_of(X):
    return np.float32(2.0) ** scale_exp_from_bits(bits(np.abs(X).max()))


def is_tiny(X, s):
    """elements that lose bits in the image: nonzero, below fp16's normal range once scaled (decided in fp32, on the source value)"""
    return (X != 0) & (np.abs(X * np.float32(s), dtype=np.float32) < FP16_MIN_NORMAL)


def image(X, s):
    """to_half_rna(x * s) and the cast: 10 mantissa bits, ties away, then fp32 -> fp16 (nearest even, which only subnormals still meet)"""
    return W.round_tf32(X * np.float32(s)).astype(np.float16)


def unscaled_image(X):
    """the image as the MFMA kernels use it, back in X's units (exact: an fp16 value times a power of two)"""
    s = scale_of(X)
    return (image(X, s).astype(np.float32) / s).astype(np.float32)


def header_words(X, D, level):
    s = scale_of(X)
    nz = np.abs(X[(X != 0) & np.isfinite(X)])
    return {"max": bits(np.abs(X).max()), "lo": 0x7f800000 - bits(nz.min()) if nz.size else 0, "cap": 2 * max(D, 1) if level >= 2 else 0,
            "tiny": int(is_tiny(X, s).sum()), "pow": 2, "strict": int(level >= 3)}


def ceil_log2(k):
    return 0 if k <= 1 else int(k - 1).bit_length()


def range_is_wide(h):
    mx, mi = h["max"], h["lo"]
    emax = mx >> 23
    if mi == 0 or mx == 0 or mx >= 0x7f800000 or not emax - ((0x7f800000 - mi) >> 23) > 28:
        return False
    if h["cap"] == 0 or h["tiny"] == 0:
        return False
    return h["pow"] * (emax - 127) >= 29 - ceil_log2(min(h["tiny"], h["cap"]))


def range_mode(X, D, level):
    """what tcgnn_range_mode reports for an SDDMM / fused-AGNN call that staged X: 0 the MFMA path alone, 2 MFMA + patch, 1 plain fp32"""
    h = header_words(X, D, level)
    if not range_is_wide(h):
        return 0
    return 1 if h["strict"] else 2


def dirty_rows(X):
    return np.flatnonzero(is_tiny(X, scale_of(X)).any(axis=1))


def touched_edges(rp, col, rows):
    erow = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    return np.isin(erow, rows) | np.isin(col, rows)


# ---- the data --------------------------------------------------------------------------------------------------------------------
def ordinary_matrix(n, D, salt=0):
    rng = np.random.default_rng(1000 * D + 7 + salt)
    X = (rng.standard_normal((n, D)) * 2.0 ** 14).astype(np.float32)
    X[np.abs(X) < 1.0] = 1.0
    return X, rng


def wide_matrix(n, D, rows, salt=0):
    """the matrix of the module docstring with `rows` dirty; salt: another draw of the same kind (the backward pass's dY)"""
    X, rng = ordinary_matrix(n, D, salt)
    rows = np.asarray(rows)
    keep = np.ones(n, bool); keep[rows] = False
    mx = float(np.abs(X[keep]).max())
    X[rows] = (rng.standard_normal((len(rows), D)) * mx * 2.0 ** -42).astype(np.float32)
    return X


# ---- the graphs ------------------------------------------------------------------------------------------------------------------
CLIQUE_ROWS = np.arange(27, 27 + 3 * 17, 3)      # 17 rows over four windows, none adjacent in numbering


def clique17_graph(n=700):
    """A small symmetric graph whose rows CLIQUE_ROWS are adjacent to each other and to nothing else (no self loops): with all 17
    dirty, every edge of these rows has a dirty row on BOTH sides (the row side of each takes it, the mirror side must not), and
    their rows of Y and G hold nothing but lost terms."""
    rp, col = graphs.uniform_graph(n, 12, seed=17)
    src = np.repeat(np.arange(n), np.diff(rp))
    keep = ~(np.isin(src, CLIQUE_ROWS) | np.isin(col, CLIQUE_ROWS))
    a, b = np.meshgrid(CLIQUE_ROWS, CLIQUE_ROWS, indexing="ij")
    off = a != b
    return graphs.csr_from_edges(np.concatenate([src[keep], a[off]]), np.concatenate([col[keep], b[off]]), n)


def ring_graph(n):
    """every row linked to its two neighbours"""
    r = np.arange(n)
    return graphs.csr_from_edges(np.concatenate([r, r]), np.concatenate([(r + 1) % n, (r - 1) % n]), n)


def finding_rows(n):
    """the dirty rows of the finding: bitmap words apart, the last one behind the windows `short_metadata` hands over"""
    return np.array([n // 7, n // 2, n - 2])


def spread_rows(n, k, seed):
    return np.sort(np.random.default_rng(seed).choice(n, size=k, replace=False))


_GRAPHS = {}


def graph(name):
    """(rowptr, col) of a case's graph, built once"""
    if name not in _GRAPHS:
        if name in ("identity_n4103", "short_metadata_n4100"):
            for g, rp, col in graphs.boundary_graphs():
                if g in ("identity_n4103", "short_metadata_n4100"):
                    _GRAPHS[g] = (rp, col)
        elif name == "uniform_n4000":
            _GRAPHS[name] = graphs.uniform_graph(4000, 100, seed=5)
        elif name == "uniform_n16400":
            _GRAPHS[name] = graphs.uniform_graph(16400, 100, seed=5)
        elif name == "directed_n4000":
            _GRAPHS[name] = graphs.uniform_graph(4000, 100, seed=5, symmetric=False)
        elif name == "hub_rows_n2500":
            _GRAPHS[name] = graphs.hub_rows_graph(2500, seed=77)
        elif name == "clique17_n700":
            _GRAPHS[name] = clique17_graph()
        elif name.startswith("ring_n"):
            _GRAPHS[name] = ring_graph(int(name[6:]))
        else:
            raise KeyError(name)
    return _GRAPHS[name]


def case_rows(name, k):
    """the intended dirty rows of a case: (graph, how many)"""
    n = len(graph(name)[0]) - 1
    if name in ("identity_n4103", "short_metadata_n4100") or name.startswith("ring_n"):
        assert k == 3
        return finding_rows(n)
    if name == "clique17_n700":
        assert k == 17
        return CLIQUE_ROWS
    rows = spread_rows(n, k, seed=100 + k)
    if name == "hub_rows_n2500":           # eight of the rows that are edges to every column among them
        rows = np.sort(np.concatenate([np.arange(8), rows[rows >= 8][: k - 8]]))
    return rows


WIDTHS = (5, 41, 64, 128, 200)             # 5: fewer columns than a group's eight lanes; 41: the tail loop; 200: forward_ef only (sddmm_wide_kernel)
# (graph, D, dirty rows): the width sweep on the finding's two graphs and on the uniform graph - there with 1 and 3 dirty rows and either
# side of kPatchRowDriven = 256; the scan (directed), hub rows, the clique and the two rings at one width each
CASES = [(g, D, 3) for g in ("identity_n4103", "short_metadata_n4100") for D in WIDTHS]
CASES += [("uniform_n4000", D, k) for k in (1, 3, 256, 257) for D in WIDTHS]
CASES += [("directed_n4000", 64, 7), ("hub_rows_n2500", 64, 12), ("clique17_n700", 64, 17), ("ring_n491519", 16, 3), ("ring_n491520", 16, 3)]
# the forced walks: the uniform generator at the smallest size whose plan holds the column-bucket table those walks need (1 024 windows)
WALK_CASE = ("uniform_n16400", 64, 3)


def case_id(c):
    return "%s-D%d-dirty%d" % c


def windows_handed_over(name, n):
    return W.windows_handed_over(name, n)


def covered_rows(name, n):
    return min(n, windows_handed_over(name, n) * 16)


# ---- the references --------------------------------------------------------------------------------------------------------------
def score_refs(name, X, meta=None):
    """(oracle in TF32 mode, fp64 on the rounded operands, sum |a||x|, host metadata); rows behind the windows handed over are zeros,
    the way walks.references leaves them"""
    rp, col = graph(name)
    n = len(rp) - 1
    meta = meta or W.host_meta(rp, col)
    ref = O.sddmm(X, rp, col, *meta, round_mode=O.ROUND_TF32)
    r64, _ = O.sddmm_f64(W.round_tf32(X), rp, col)
    _, s64 = O.sddmm_f64(X, rp, col)
    cut = rp[covered_rows(name, n)]
    for a in (ref, r64, s64):
        a[cut:] = 0
    return ref, r64, s64, meta


def agg_refs(name, X, att, meta):
    """the same three for Y = A(att) X"""
    rp, col = graph(name)
    n = len(rp) - 1
    ref = O.spmm_val(X, rp, col, att, *meta, round_mode=O.ROUND_TF32)
    r64, _ = O.spmm_f64(W.round_tf32(X), rp, col, W.round_tf32(att))
    _, s64 = O.spmm_f64(X, rp, col, att)
    rows = covered_rows(name, n)
    for a in (ref, r64, s64):
        a[rows:] = 0
    return ref, r64, s64


def unpatched_scores(name, X):
    """what the MFMA kernels alone return, emulated: the fp64 product of the emulated images"""
    rp, col = graph(name)
    u, _ = O.sddmm_f64(unscaled_image(X), rp, col)
    u[rp[covered_rows(name, len(rp) - 1)]:] = 0
    return u


def ratio(got, ref, scale):
    """|got - ref| relative to each element's own sum of |terms| (0 where there are none and the two agree)"""
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    out = np.zeros_like(d)
    np.divide(d, scale, out=out, where=scale > 0)
    out[(scale <= 0) & (d > 0)] = np.inf
    return out


def is_symmetric(rp, col):
    n = len(rp) - 1
    a = sp.csr_matrix((np.ones(len(col), dtype=np.int8), col, rp), shape=(n, n))
    return (a != a.T).nnz == 0
