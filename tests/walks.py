"""What tests/test_structures_cpu.py and tests/test_gpu_structures.py share: the data and the cached references of a catalogue
entry (graphs.boundary_graphs), the oracle-alone conditions, and the table of walks - how each is forced and which kernel name
TCGNN.last_kernel must report for it.  No GPU needed to import."""
import numpy as np
import scipy.sparse as sp

import graphs
from oracle import oracle as O

# shares of the bounds the ORACLE ALONE may use up on a catalogue entry (the bounds themselves: test_gpu_parity.TOL / TIGHT / 2^-9)
TOL, TIGHT, LOOSE = 1e-3, 4e-6, 2.0 ** -9
NOISE_SHARE, ROUNDING_SHARE = 0.25, 0.5


def round_tf32(x):
    """cvt.rna.tf32 on an array: round to 10 mantissa bits, ties away from zero (what oracle_round_tf32 does element by element)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x1000) & 0xffffe000).astype(np.uint32).view(np.float32)


def is_short(name):
    return name.startswith("short_metadata")


def is_unsorted(name):
    return name.startswith("unsorted_rows")


def is_symmetric(rp, col):
    n = len(rp) - 1
    a = sp.csr_matrix((np.ones(len(col), dtype=np.int8), col, rp), shape=(n, n))
    return (a != a.T).nnz == 0


def windows_handed_over(name, n):
    nw = (n + 15) // 16
    return nw - graphs.SHORT_METADATA_CUT if is_short(name) else nw


def case_data(n, nnz, D):
    """Standard-normal features and edge values, the data the oracle-alone conditions were measured with."""
    rng = np.random.default_rng(D)
    X = rng.standard_normal((n, D)).astype(np.float32)
    att = rng.standard_normal(nnz).astype(np.float32)
    return X, att


def host_meta(rp, col):
    n, nnz = len(rp) - 1, len(col)
    bp = np.zeros((n + 15) // 16, np.int32); e2c = np.zeros(nnz, np.int32); e2r = np.zeros(nnz, np.int32)
    O.preprocess(col, rp, n, 16, 8, bp, e2c, e2r)
    return bp, e2c, e2r


_REFS = {}


def references(name, rp, col, D, ops=("spmm", "spmm_val", "sddmm")):
    """{op: (ref_tf32, ref64, scale64)} for the entry's own data (case_data), cached per (name, D).  `short_metadata`: rows (and the
    scores of edges) of the windows that are not handed over are zeros, as zeros_like leaves them."""
    key = (name, D)
    have = _REFS.setdefault(key, {})
    n, nnz = len(rp) - 1, len(col)
    X, att = case_data(n, nnz, D)
    if "meta" not in have:
        have["meta"] = host_meta(rp, col)
    bp, e2c, e2r = have["meta"]
    rows = windows_handed_over(name, n) * 16
    for op in ops:
        if op in have:
            continue
        if op == "spmm":
            ref = O.spmm(X, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32); r64, s64 = O.spmm_f64(X, rp, col)
        elif op == "spmm_val":
            ref = O.spmm_val(X, rp, col, att, bp, e2c, e2r, round_mode=O.ROUND_TF32) if nnz else np.zeros((n, D), np.float32)
            r64, s64 = O.spmm_f64(X, rp, col, att) if nnz else (np.zeros((n, D)), np.zeros((n, D)))
        else:
            ref = O.sddmm(X, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32); r64, s64 = O.sddmm_f64(X, rp, col)
        if rows < n:
            cut = slice(rp[rows], None) if op == "sddmm" else slice(rows, None)
            ref[cut] = 0; r64[cut] = 0; s64[cut] = 0
        have[op] = (ref, r64, s64)
    return {op: have[op] for op in ops}, (X, att), (bp, e2c, e2r)


def oracle_alone(name, rp, col, D):
    """{op: (noise_tight, noise_bar, rounding)}: the TF32-mode oracle's distance from an fp64 evaluation on the SAME rounded operands
    (accumulation noise - what two correct implementations may differ by) relative to sum|a||x| + 1 and to max(1, |ref|), and its
    distance from the fp64 contract on the unrounded operands (operand rounding, shared by kernels and oracle) relative to
    sum|a||x| + 1."""
    refs, (X, att), _ = references(name, rp, col, D)
    Xr, attr = round_tf32(X), round_tf32(att)
    n, nnz = len(rp) - 1, len(col)
    rows = windows_handed_over(name, n) * 16
    out = {}
    for op, (ref, r64, s64) in refs.items():
        if nnz == 0:
            out[op] = (0.0, 0.0, 0.0)
            continue
        if op == "spmm":
            rr, _ = O.spmm_f64(Xr, rp, col)
        elif op == "spmm_val":
            rr, _ = O.spmm_f64(Xr, rp, col, attr)
        else:
            rr, _ = O.sddmm_f64(Xr, rp, col)
        if rows < n:
            rr[slice(rp[rows], None) if op == "sddmm" else slice(rows, None)] = 0
        out[op] = (float((np.abs(ref - rr) / (s64 + 1.0)).max()), float((np.abs(ref - rr) / np.maximum(1.0, np.abs(rr))).max()),
                   float((np.abs(ref - r64) / (s64 + 1.0)).max()))
    return out


def transposed_csr(rp, col):
    """(rowptr, col, perm) of A^T: perm[k] = the position in A's CSR order of A^T's k-th edge."""
    n = len(rp) - 1
    a = sp.csr_matrix((np.arange(1, len(col) + 1, dtype=np.int64), col, rp), shape=(n, n)).T.tocsr()
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), (a.data - 1).astype(np.int64)


# ---- the range-major walks cut the fp16 image into column ranges of TCGNN_RANGE_KB; mirrors of x16_pitch and of range_count
# (x16_pitch: tcgnn_stage.inc; range_count: tcgnn_device.hip, the one loop route_sddmm, the SpMM dispatcher and launch_agnn_range_major pick the number of ranges with), so that a test can
# force eight of them and say so
def image_bytes(n, D):
    row = (D + 15) // 16 * 16 * 2
    if row > 128:
        pitch = (row + 127) // 128 * 128
    else:
        pitch = 32
        while pitch < row:
            pitch <<= 1
    return (n + 1) * pitch


def range_kb_for_eight(n, D):
    """TCGNN_RANGE_KB that cuts the image into eight ranges or more (a multiple of eight: what the XCD-affinity branch wants)."""
    return str(max(1, image_bytes(n, D) // 1024 // 8))


def expected_ranges(n, D, column_buckets, range_kb):
    nranges, limit = 1, int(range_kb) << 10
    while nranges < column_buckets and image_bytes(n, D) // nranges > limit:
        nranges <<= 1
    return nranges


# ---- forcing a walk, and judging what it returned (tests/test_gpu_structures.py; kept here for the GPU tests that force walks through ctypes)
KNOBS = ("TCGNN_LDS_FLAT", "TCGNN_LDS_DENSE_COLS", "TCGNN_SDDMM_XCD", "TCGNN_RM_IDENT", "TCGNN_AGNN_SLICED", "TCGNN_AGNN_ROT", "TCGNN_RANGE_KB",
         "TCGNN_LDS_HOT_COLS", "TCGNN_SYNC", "TCGNN_PATCH_ROWS")


def forced(T, monkeypatch, mode, env, body, ctx):
    """body() under one walk: an empty plan cache (the stream knobs are read when a stream is built), the knobs, the mode.
    ctx: {"n", "D"} for knobs whose value is a function of them, "capfd" (may be None: nothing is read back) - and ctx["stream"]
    receives what the plan said it built, (tiles per cell seen, most dense entries seen), or None."""
    import re
    import sys
    import tcgnn_capi as c
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v(ctx["n"], ctx["D"]) if callable(v) else v)
    streams = "TCGNN_LDS_FLAT" in env and ctx.get("capfd") is not None       # (the plan says what it built on stderr: tiles per cell, dense entries)
    if streams:
        monkeypatch.setenv("TCGNN_VERBOSE", "1")
        sys.stdout.write(ctx["capfd"].readouterr().out)
    ctx["stream"] = None
    T.clear_plan_cache()
    try:
        c.check(c.lib.tcgnn_set_spmm_mode(mode), "tcgnn_set_spmm_mode")
        return body()
    finally:
        c.lib.tcgnn_set_spmm_mode(0)
        T.clear_plan_cache()
        for k in env:
            monkeypatch.delenv(k, raising=False)
        if streams:
            monkeypatch.delenv("TCGNN_VERBOSE", raising=False)
            out, err = ctx["capfd"].readouterr()
            sys.stdout.write(out)
            found = re.findall(r"flat: (\d+) tile\(s\) per cell, \d+ entries \((\d+) dense\)", err)
            ctx["stream"] = ({int(t) for t, _ in found}, max([int(d) for _, d in found] or [0]))


def judge(name, got, ref, r64, s64, what, zero=None, zero_value=0.0):
    """-> list of failures (empty: fine).  The project's bounds; the non-canonical entry as test_non_canonical_rows_take_the_fallback_kernels
    judges such a plan (absolute, against the TF32-mode oracle)."""
    from test_gpu_parity import assert_parity
    bad = []
    if not np.isfinite(got).all():
        bad.append("%s: %d non-finite elements" % (what, int((~np.isfinite(got)).sum())))
        return bad
    fig = (float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()), float((np.abs(got - ref) / (s64 + 1.0)).max()),
           float((np.abs(got - r64) / (s64 + 1.0)).max())) if got.size else (0.0, 0.0, 0.0)
    print("FIG %-34s bar %.2e tight %.2e fp64 %.2e" % (what, *fig))
    if is_unsorted(name):
        lim = 1e-3 if what.startswith("forward ") or what.startswith("epilogues") else 1e-4
        if got.size and np.abs(got - ref).max() >= lim:
            bad.append("%s: %.3e from the oracle (non-canonical plan: %.0e)" % (what, np.abs(got - ref).max(), lim))
    else:
        try:
            assert_parity(got, ref, r64, s64, what)
        except AssertionError as e:
            bad.append(str(e) or "%s: beyond 2^-9 of the fp64 contract (%.3e)" % (what, fig[2]))
    if zero is not None and zero.any():
        z = got[zero]
        want = np.broadcast_to(np.asarray(zero_value, dtype=np.float32), z.shape)
        if not np.array_equal(z, want):
            bad.append("%s: %d elements of rows without edges differ from the empty sum's value" % (what, int((z != want).sum())))
    return bad


def zero_rows(name, rp):
    """rows whose sum is empty: no edges, or beyond the windows handed over (`short_metadata`)"""
    n = len(rp) - 1
    z = np.diff(rp) == 0
    z[windows_handed_over(name, n) * 16:] = True
    return z


# ---- the walks: name -> (spmm mode, test knobs, what last_kernel must report).  A knob's value may be a function of (N, D).  The knobs are read when a stream is built or per
# call (tcgnn_device.hip "run-time switches"), so a walk starts from an empty plan cache.
def _is(name):
    return lambda k: k == name


def _starts(prefix):
    return lambda k: k.startswith(prefix)


def _has(part):
    return lambda k: part in k


FORWARD_WALKS = {
    "auto": (0, {}, None),
    "per_window": (1, {}, _is("spmm_kernel")),
    "range_blocked": (2, {"TCGNN_RANGE_KB": range_kb_for_eight}, _is("spmm_blocked_kernel")),
    "lds_ordinary": (3, {"TCGNN_LDS_FLAT": "0"}, _starts("spmm_lds_kernel")),
    "lds_flat1": (3, {"TCGNN_LDS_FLAT": "1"}, _starts("spmm_lds_flat_kernel")),
    "lds_flat2": (3, {"TCGNN_LDS_FLAT": "2"}, _starts("spmm_lds_flat_kernel")),
    "lds_flat1_dense": (3, {"TCGNN_LDS_FLAT": "1", "TCGNN_LDS_DENSE_COLS": "1"}, _starts("spmm_lds_flat_kernel")),
    "single_launch_fp32": (4, {}, _is("spmm_small_kernel")),
    "slice_synchronised": (5, {}, _is("spmm_sync_kernel")),
}
# (walks whose mode has no way to another kernel on a plan with windows: no entry of the exception table may name them; every LDS
#  walk must at least stay on an LDS-resident kernel)
STRICT_FORWARD = {"per_window", "single_launch_fp32"}
LDS_FORWARD = {"lds_ordinary", "lds_flat1", "lds_flat2", "lds_flat1_dense"}

AGNN_WALKS = {
    "auto": (0, {}, None),
    "per_window": (1, {}, _is("spmm_kernel")),
    "range_blocked": (2, {"TCGNN_RANGE_KB": range_kb_for_eight}, _is("spmm_blocked_kernel")),
    # (one tile per cell forced, as every edge-valued LDS test does: the stream is cut from single-edge tiles, build_val_stream)
    "lds_val": (3, {"TCGNN_LDS_FLAT": "1"}, _has("spmm_lds_val_kernel")),
    "lds_val_dense": (3, {"TCGNN_LDS_FLAT": "1", "TCGNN_LDS_DENSE_COLS": "1"}, _has("spmm_lds_val_kernel")),
    "slice_synchronised": (5, {}, _is("spmm_sync_kernel")),
}


def _sddmm_name(suffix=""):
    return lambda k, D: k == ("sddmm_kernel" + suffix if (D + 31) // 32 <= 4 else "sddmm_wide_kernel")


def _sddmm_narrow(suffix=""):
    """the range-major and slice-synchronised walks exist up to 128 columns (ks <= 4) only"""
    return lambda k, D: (D + 31) // 32 <= 4 and k == "sddmm_kernel" + suffix


# (the range-major walk, mode 2, in eight ranges or more - test_sddmm_range_major_walk_with_xcd_affinity... forces it the same way;
#  the kernel's name does not tell the range-major walk from the per-window one: the test computes the range count as well)
_RM = {"TCGNN_RANGE_KB": range_kb_for_eight}
SDDMM_WALKS = {
    "auto": (0, {}, _sddmm_name()),
    "xcd0": (2, dict(_RM, TCGNN_SDDMM_XCD="0"), _sddmm_narrow()),
    "xcd1": (2, dict(_RM, TCGNN_SDDMM_XCD="1"), _sddmm_narrow()),
    "xcd2": (2, dict(_RM, TCGNN_SDDMM_XCD="2"), _sddmm_narrow()),
    "ident0": (2, dict(_RM, TCGNN_RM_IDENT="0"), _sddmm_narrow()),
    "ident1": (2, dict(_RM, TCGNN_RM_IDENT="1"), _sddmm_narrow()),
    "slice_synchronised": (5, {}, _sddmm_narrow(" (slice-synchronised)")),
}

# (TCGNN_SYNC=0: on a graph with locality and 2 048 windows the automatic mode takes the slice-synchronised walk before it looks at
#  TCGNN_AGNN_SLICED - sync_chosen - so the walks that force the other forms switch that one off)
_SLICED = "agnn_kernel (XCD-sliced) + agnn_slice_sum_kernel"
FUSED_WALKS = {
    "auto": (0, {}, None),
    "sliced0": (0, {"TCGNN_AGNN_SLICED": "0", "TCGNN_SYNC": "0"}, _is("agnn_kernel")),
    # (1: the automatic rule between the three forms, which no catalogue graph is large enough to send away from the per-window walk
    #  by itself - values only, no name to demand)
    "sliced1": (0, {"TCGNN_AGNN_SLICED": "1", "TCGNN_SYNC": "0"}, None),
    "sliced2": (0, {"TCGNN_AGNN_SLICED": "2", "TCGNN_SYNC": "0"}, _is(_SLICED)),
    "sliced16": (0, {"TCGNN_AGNN_SLICED": "16", "TCGNN_SYNC": "0"}, _is(_SLICED)),
    "sliced2_rot0": (0, {"TCGNN_AGNN_SLICED": "2", "TCGNN_AGNN_ROT": "0", "TCGNN_SYNC": "0"}, _is(_SLICED)),
    "sliced2_rot1": (0, {"TCGNN_AGNN_SLICED": "2", "TCGNN_AGNN_ROT": "1", "TCGNN_SYNC": "0"}, _is(_SLICED)),
    "range_major": (2, {"TCGNN_RANGE_KB": range_kb_for_eight, "TCGNN_SYNC": "0"}, _is("agnn_kernel")),
    "slice_synchronised": (5, {}, _is("agnn_kernel (slice-synchronised)")),
}
