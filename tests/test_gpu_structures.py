"""The walk x structure matrix: every walk of every operator, forced the way the other GPU tests force them, on the catalogue of
boundary-shaped graphs (tests/graphs.py; pinned to its boundaries by tests/test_structures_cpu.py), against the whole-product
oracle.  Needs an MI355X: `pytest -m gpu`.

What each entry is there for:

  block_diag_16x32_n4096          every window exactly 4 full tiles, every mask byte 0xff, cells at the flat stream's 32-column cap
  range_boundary_columns_n4585    columns on the first / last row of every LDS range size (504 / 632 / 760 / 1528) and on the last
                                  record of the image, next to the sentinel; N % 16 = 9
  two_hub_columns_n4101           one-column tiles on record 0 and record Nc - 1
  one_hub_row_last_n4097          every window empty but the ragged last one (N % 16 = 1), which holds every column: hub splitting
                                  with nearly every (workgroup, range) pair empty
  middle_rows_only_n4100          empty leading and trailing windows
  identity_n4103                  one edge per row
  upper_band200_n4100             strictly asymmetric, last row empty, columns always ahead of the window
  complete_n1030                  16 480 edges per window, all masks full, every column a multi-edge column: at one tile per cell nearly
                                  all of it is cold remainder (spmm_cold_planar_kernel / spmm_cold_val_kernel)
  checkerboard_band128_n4100      mask bytes 0x55 / 0xaa alternating by row
  single_edge_corner_n5000        E = 1: below the E >= 4 / E >= 8 limits of the edge-valued and fused paths
  sixteen_full_rows_n4095 / 4096  window 0 holds 65 520 / 65 536 edges: either side of the 16-bit edge offsets of the edge-valued stream
                                  (over a background dense enough that window 0 is not split as a hub).  4095 runs the LDS-resident
                                  edge-valued walk through val_permute_kernel's UN-STAGED path (a pair of windows beyond 18 432
                                  stream edges); 4096 is refused by val_index16_kernel and takes the gather walk
  unsorted_rows_n4100             a non-canonical plan at a size where the forced walks are real
  short_metadata_n4100            blockPartition 40 windows short: nw_eff * 16 < N (memset + epi_fill_kernel) under every walk
  one_row_per_column_band1536_n16409, every_other_window_empty_n16500, bucket_boundary_columns_n16500
                                  large enough for the plan's column-bucket table (>= 1 024 windows of >= 512 distinct columns),
                                  which the range-blocked SpMM, the range-major SDDMM and the XCD-sliced fused walk need: columns on
                                  every bucket boundary, empty windows inside a persistent wavefront's group, one-row columns
  communities_empty_xcd_share_n40003, communities_hub_row_and_column_n40003
                                  the slice-synchronised walk (>= 2 048 windows, locality) with one XCD's share of the windows
                                  empty / with a hub row and a hub column

Every call is judged on VALUES (test_gpu_parity.assert_parity with the project's bounds, finite everywhere, exact zeros in rows without
edges), on the KERNEL THAT RAN (TCGNN.last_kernel against the name the walk must report; EXCEPTIONS lists the (walk, graph) pairs
that legitimately report another one, each with its plan condition - a pair in the table that DOES run the forced kernel fails
too) and on DETERMINISM (a second call returns the same bits).  The last test demands that every walk ran its own kernel on at
least half of the graphs it was run on and prints the counts.

The walks that need a bucket table (range-blocked SpMM, range-major SDDMM and fused pair, XCD-sliced fused pair) are forced on every
graph with TCGNN_RANGE_KB set to an eighth of the image, as test_sddmm_range_major_walk_with_xcd_affinity... forces them: eight ranges
or more, a multiple of eight, at every width.  On the 14 entries of about 4 k nodes the plan has no bucket table (257 - 313 windows;
tcgnn_plan_create builds it from 4 windows per CU, 1 024, on) and EXCEPTIONS says so; their half is counted over the five larger
entries, and the range-major SDDMM / fused walks, whose kernel carries the per-window walk's name, count as run only where the plan
holds a bucket table and the range count computed from the image size is a multiple of eight.  The slice-synchronised walk is run on
the two 40 k entries.  The flat walks also read the plan's verbose line: tiles per cell as forced, dense entries counted."""
import sys

import numpy as np
import pytest
import torch

import graphs
import walks as W
from oracle import oracle as O
from test_gpu_parity import assert_parity, to_dev

pytestmark = pytest.mark.gpu

SMALL = graphs.boundary_graphs()
BUCKETED = graphs.bucketed_boundary_graphs()
SYNC = graphs.sync_boundary_graphs()
GRAPHS = {name: (rp, col) for name, rp, col in SMALL + BUCKETED + SYNC}
SMALL_NAMES, BUCKETED_NAMES, SYNC_NAMES = ([g[0] for g in s] for s in (SMALL, BUCKETED, SYNC))
KNOBS = W.KNOBS
NEEDS_BUCKETS = {("forward", "range_blocked"), ("forward_AGNN", "range_blocked"), ("forward_ef", "xcd0"), ("forward_ef", "xcd1"), ("forward_ef", "xcd2"),
                 ("forward_ef", "ident0"), ("forward_ef", "ident1"), ("agnn_fused", "sliced2"), ("agnn_fused", "sliced16"), ("agnn_fused", "sliced2_rot0"),
                 ("agnn_fused", "sliced2_rot1"), ("agnn_fused", "range_major")}
# walks whose kernel carries the per-window walk's name: that they ran is shown by the bucket table and the computed range count
SAME_NAME = {("forward_ef", w) for w in ("xcd0", "xcd1", "xcd2", "ident0", "ident1")} | {("agnn_fused", "range_major")}
WALKS = {"forward": W.FORWARD_WALKS, "forward_AGNN": W.AGNN_WALKS, "forward_ef": W.SDDMM_WALKS, "agnn_fused": W.FUSED_WALKS}

# (operator, walk, graph) -> the plan condition that sends the call to another kernel.  Checked both ways: a pair that is not here and
# reports another kernel fails, and so does a pair that is here and reports the forced one.
_HUBS = "hub windows are split over wavefronts (lds_has_hubs: the longest window beyond 4x the mean), which keeps the ordinary cell stream"
_HUB_GRAPHS = ("one_hub_row_last_n4097", "middle_rows_only_n4100", "communities_hub_row_and_column_n40003")
_CSR = "spmm_val_csr_kernel (non-canonical plan, or E < 4) runs before any walk is chosen and reports no kernel"
EXCEPTIONS = {}
for _g in _HUB_GRAPHS:
    for _w in ("lds_flat1", "lds_flat2", "lds_flat1_dense"):
        EXCEPTIONS[("forward", _w, _g)] = _HUBS
    for _w in ("lds_val", "lds_val_dense"):
        EXCEPTIONS[("forward_AGNN", _w, _g)] = _HUBS + " - and the edge-valued stream wants a flat one (build_val_stream: nsplit == 0)"
for _w in ("per_window", "lds_val", "lds_val_dense"):
    EXCEPTIONS[("forward_AGNN", _w, "single_edge_corner_n5000")] = _CSR + ": E = 1"
    EXCEPTIONS[("forward_AGNN", _w, "unsorted_rows_n4100")] = _CSR + ": canonical == 0"
for _w in ("lds_val", "lds_val_dense"):
    # a refusal that is a correct result from another kernel: window 0 holds 65 536 edges, val_index16_kernel raises `bad`, the plan
    # settles on the gather walks (val_choice = 0) - and sixteen_full_rows_n4095, 65 520 edges, runs the LDS-resident walk
    EXCEPTIONS[("forward_AGNN", _w, "sixteen_full_rows_n4096")] = "a window of 65 535 edges or more is beyond the stream's 16-bit edge offsets: gather walk"
EXCEPTIONS[("forward_ef", "auto", "unsorted_rows_n4100")] = "sddmm_csr_kernel (canonical == 0) reports no kernel"
_NO_BUCKETS = "column_buckets == 0: tcgnn_plan_create builds the bucket table from 4 windows per CU (1 024) on, this plan has 257 - 313: per-window walk"
# widths the LDS-resident edge-valued walk does not cover on any graph (val_lds_width_ok: whole 64-column chunks or a three-plane remainder)
def _val_lds_width(D):
    return ((D + 15) // 16 * 16) % 64 in (0, 48)

# what a documented refusal must say: (operator, graph) -> a piece of the RuntimeError's text
REFUSALS = {("agnn_fused", "single_edge_corner_n5000"): "E >= 8", ("agnn_fused", "unsorted_rows_n4100"): "canonical"}

RAN = {}        # (operator, walk) -> {(graph, D): the forced kernel ran}
STREAMS = {}    # (operator, walk) -> {graph: (tiles per cell seen, most dense entries seen)} from the plan's verbose lines
_CTX = {}       # the running test's capfd


def _widths(name, op):
    base = (16, 41, 64, 128)
    if op == "agnn_fused":
        return base
    if op == "forward_ef":
        return base + (160,)
    if name in ("block_diag_16x32_n4096", "range_boundary_columns_n4585") and op in ("forward", "epilogues"):
        return base + (1, 201)       # one padded plane; 13 planes = three 64-column passes + a one-plane remainder with D % 4 != 0
    return base


def _walks_for(name, op):
    out = []
    for walk in WALKS[op]:
        if walk == "slice_synchronised" and name not in SYNC_NAMES:
            continue
        out.append(walk)
    return out


for _op, _walk in NEEDS_BUCKETS:
    for _g in SMALL_NAMES:
        EXCEPTIONS.setdefault((_op, _walk, _g), _NO_BUCKETS)


CASES = [(name, D, op) for name in GRAPHS for op in ("forward", "epilogues", "forward_AGNN", "forward_ef", "agnn_fused")
         for D in _widths(name, op)]
CASES.sort(key=lambda c: (list(GRAPHS).index(c[0]), c[1]))      # (graph, D) together: the references are cached for one pair at a time


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def T():
    import TCGNN
    return TCGNN


_META = {}


def _meta(dev, name):
    """The five metadata tensors on the device, as the host SGT wrote them (`short_metadata`: blockPartition cut)."""
    if name not in _META:
        _META.clear()
        rp, col = GRAPHS[name]
        bp, e2c, e2r, _ = graphs.host_sgt(rp, col)
        bp = bp[: W.windows_handed_over(name, len(rp) - 1)]
        _META[name] = tuple(to_dev(dev, rp, col, bp, e2c, e2r))
    return _META[name]


_CACHE = {"key": None}


def _cached(name, D, what, make):
    if _CACHE["key"] != (name, D):
        _CACHE.clear(); _CACHE["key"] = (name, D); W._REFS.clear()
    if what not in _CACHE:
        _CACHE[what] = make()
    return _CACHE[what]


def _refs(name, D, op):
    rp, col = GRAPHS[name]
    r, data, meta = W.references(name, rp, col, D, ops=(op,))
    return r[op], data, meta


def _zero_rows(name):
    return W.zero_rows(name, GRAPHS[name][0])


_judge = W.judge


def _kernel_check(op, walk, name, D, kernel, pred, failures, covered=True):
    """The forced walk ran - or the pair is in EXCEPTIONS, and then it did not."""
    if pred is None:
        return
    ran = bool(pred(kernel))
    if (op, walk) in SAME_NAME:          # (mode 2 with a bucket table, in eight ranges or more - a multiple of eight, as the XCD branch wants)
        n = len(GRAPHS[name][0]) - 1
        nr = W.expected_ranges(n, D, _CTX["buckets"], W.range_kb_for_eight(n, D))
        ran = ran and _CTX["buckets"] > 0 and nr >= 8 and nr % 8 == 0
    print("OBS %s | %s | %s | D=%d | %s | %s" % (op, walk, name, D, kernel, "ran" if ran else "OTHER"))
    if not covered:                       # a width the walk covers on no graph
        if ran:
            failures.append("%s/%s D=%d reports %r at a width outside the walk's range" % (op, walk, D, kernel))
        return
    RAN.setdefault((op, walk), {})[(name, D)] = ran
    why = EXCEPTIONS.get((op, walk, name))
    if why is None and not ran:
        failures.append("%s/%s: last_kernel is %r, not the forced kernel, and EXCEPTIONS has no entry for the pair" % (op, walk, kernel))
    if why is not None and ran:
        failures.append("%s/%s: EXCEPTIONS says %r, but the forced kernel ran (%r)" % (op, walk, why, kernel))


def _forced(T, monkeypatch, mode, env, body):
    """body() under one walk (walks.forced: an empty plan cache, the knobs, the mode); _CTX["stream"] receives what the plan built."""
    return W.forced(T, monkeypatch, mode, env, body, _CTX)


def _stream_check(op, walk, name, kernel_ran, env, failures):
    """A flat walk that ran built streams of the forced number of tiles per cell; the dense entries it saw are kept for the report."""
    if "TCGNN_LDS_FLAT" not in env or env["TCGNN_LDS_FLAT"] == "0" or not kernel_ran:
        return
    tpcs, dense = _CTX["stream"] or (set(), 0)
    if tpcs != {int(env["TCGNN_LDS_FLAT"])}:
        failures.append("%s/%s: the plan reports flat streams of %s tile(s) per cell, forced %s" % (op, walk, sorted(tpcs), env["TCGNN_LDS_FLAT"]))
    seen = STREAMS.setdefault((op, walk), {})
    seen[name] = max(seen.get(name, 0), dense)


def _run_forward(dev, T, monkeypatch, name, D):
    (ref, r64, s64), (X, _), _ = _refs(name, D, "spmm")
    meta = _meta(dev, name)
    tX = _cached(name, D, "tX", lambda: to_dev(dev, X)[0])
    zero = _zero_rows(name)
    failures = []
    for walk in _walks_for(name, "forward"):
        mode, env, pred = W.FORWARD_WALKS[walk]

        def body():
            Y = T.forward(tX, *meta)[0]
            k = T.last_kernel(*meta)
            return Y, k, T.forward(tX, *meta)[0]
        try:
            Y, kernel, again = _forced(T, monkeypatch, mode, env, body)
        except RuntimeError as e:
            failures.append("%s: %s" % (walk, e))
            continue
        bad = _judge(name, Y.cpu().numpy(), ref, r64, s64, "forward %s (%s)" % (walk, kernel), zero)
        if not torch.equal(Y, again):
            bad.append("forward %s: the second call returns other bits" % walk)
        _kernel_check("forward", walk, name, D, kernel, pred, bad)
        _stream_check("forward", walk, name, pred is not None and pred(kernel), env, bad)
        if walk in W.LDS_FORWARD and not kernel.startswith("spmm_lds"):
            bad.append("forward %s: mode 3 left the LDS-resident kernels (%r)" % (walk, kernel))
        if walk == "auto":
            print("OBS forward | auto | %s | D=%d | %s | chosen" % (name, D, kernel))
        failures += bad
    return failures


def _run_epilogues(dev, T, monkeypatch, name, D):
    """forward_fused (ReLU, gate), forward_scaled and transpose=True on the walk the automatic mode chooses and on mode 3."""
    rp, col = GRAPHS[name]
    n = len(rp) - 1
    (ref, r64, s64), (X, _), (bp, e2c, e2r) = _refs(name, D, "spmm")
    meta = _meta(dev, name)
    tX = _cached(name, D, "tX", lambda: to_dev(dev, X)[0])
    zero = _zero_rows(name)
    rows = W.windows_handed_over(name, n) * 16
    rng = np.random.default_rng(1000 + D)
    r = rng.uniform(0.1, 1.0, n).astype(np.float32); c = rng.uniform(0.1, 1.0, n).astype(np.float32); b = rng.standard_normal(D).astype(np.float32)
    tr, tc, tb = to_dev(dev, r, c, b)

    def scaled_refs():
        Xc = (c[:, None] * X).astype(np.float32)
        a = O.spmm(Xc, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32); a64, as64 = O.spmm_f64(Xc, rp, col)
        a[rows:] = 0; a64[rows:] = 0; as64[rows:] = 0
        pre = (a * r[:, None] + b).astype(np.float32)
        pre64 = a64 * r[:, None].astype(np.float64) + b.astype(np.float64)
        return np.maximum(pre, 0), np.maximum(pre64, 0), as64 * r[:, None].astype(np.float64) + np.abs(b).astype(np.float64)
    sref, s64ref, sscale = _cached(name, D, "scaled", scaled_refs)
    directed = (not W.is_short(name)) and (not W.is_unsorted(name)) and not W.is_symmetric(rp, col)
    if directed:
        def t_refs():
            trp, tcol, _ = W.transposed_csr(rp, col)
            tb_, te2c, te2r = W.host_meta(trp, tcol)
            a64, as64 = O.spmm_f64(X, trp, tcol)
            return O.spmm(X, trp, tcol, tb_, te2c, te2r, round_mode=O.ROUND_TF32), a64, as64, np.diff(trp) == 0
        tref, t64, ts64, tzero = _cached(name, D, "transposed", t_refs)
    failures = []
    for walk in ("auto", "lds_default"):
        mode, env = (0, {}) if walk == "auto" else (3, {})

        def body():
            Y = T.forward(tX, *meta)[0]
            k0 = T.last_kernel(*meta)
            out = {"relu": T.forward_fused(tX, *meta, relu=True)[0], "k_relu": T.last_kernel(*meta),
                   "gate": T.forward_fused(tX, *meta, gate=Y)[0], "Y": Y, "k0": k0,
                   "scaled": T.forward_scaled(tX, *meta, row_scale=tr, col_scale=tc, bias=tb, relu=True)[0], "k_scaled": T.last_kernel(*meta)}
            out["scaled2"] = T.forward_scaled(tX, *meta, row_scale=tr, col_scale=tc, bias=tb, relu=True)[0]
            if directed:
                out["t"] = T.forward(tX, *meta, transpose=True)[0]
                out["k_t"] = T.last_kernel(*meta, transpose=True)
            return out
        try:
            out = _forced(T, monkeypatch, mode, env, body)
        except RuntimeError as e:
            failures.append("epilogues %s: %s" % (walk, e))
            continue
        tag = "epilogues %s" % walk
        failures += _judge(name, out["relu"].cpu().numpy(), np.maximum(ref, 0), np.maximum(r64, 0), s64, "%s relu (%s)" % (tag, out["k_relu"]), zero)
        # the gate is the kernel's own output: the reference is the oracle on X * (Y > 0) with that very mask
        Xg = (X * (out["Y"].cpu().numpy() > 0)).astype(np.float32)
        g = O.spmm(Xg, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32); g64, gs64 = O.spmm_f64(Xg, rp, col)
        g[rows:] = 0; g64[rows:] = 0; gs64[rows:] = 0
        failures += _judge(name, out["gate"].cpu().numpy(), g, g64, gs64, "%s gate" % tag, zero)
        failures += _judge(name, out["scaled"].cpu().numpy(), sref, s64ref, sscale, "%s scaled (%s)" % (tag, out["k_scaled"]), zero, np.maximum(b, 0))
        if not torch.equal(out["scaled"], out["scaled2"]):
            failures.append("%s scaled: the second call returns other bits" % tag)
        if walk == "lds_default":
            for k in ("k0", "k_relu", "k_scaled"):
                if not out[k].startswith("spmm_lds"):
                    failures.append("%s: mode 3 left the LDS-resident kernels at %s (%r)" % (tag, k, out[k]))
        if directed:
            failures += _judge(name, out["t"].cpu().numpy(), tref, t64, ts64, "%s transposed (%s)" % (tag, out["k_t"]), tzero)
            if walk == "lds_default" and not out["k_t"].startswith("spmm_lds"):
                failures.append("%s transposed: mode 3 left the LDS-resident kernels (%r)" % (tag, out["k_t"]))
    return failures


def _run_agnn(dev, T, monkeypatch, name, D):
    (ref, r64, s64), (X, att), _ = _refs(name, D, "spmm_val")
    meta = _meta(dev, name)
    tX = _cached(name, D, "tX", lambda: to_dev(dev, X)[0])
    tatt = _cached(name, D, "tatt", lambda: to_dev(dev, att)[0].view(1, -1))
    zero = _zero_rows(name)
    failures = []
    for walk in _walks_for(name, "forward_AGNN"):
        mode, env, pred = W.AGNN_WALKS[walk]

        def body():
            if mode == 3:                 # (the stream is built before the first call, which would otherwise still take a gather walk)
                T.prepare([D], *meta, edge_valued=True)
            Y = T.forward_AGNN(tX, meta[0], meta[1], tatt, *meta[2:])[0]
            k = T.last_kernel(*meta)
            return Y, k, T.forward_AGNN(tX, meta[0], meta[1], tatt, *meta[2:])[0]
        try:
            Y, kernel, again = _forced(T, monkeypatch, mode, env, body)
        except RuntimeError as e:
            failures.append("forward_AGNN %s: %s" % (walk, e))
            continue
        bad = _judge(name, Y.cpu().numpy(), ref, r64, s64, "forward_AGNN %s (%s)" % (walk, kernel), zero)
        if not torch.equal(Y, again):
            bad.append("forward_AGNN %s: the second call returns other bits" % walk)
        _kernel_check("forward_AGNN", walk, name, D, kernel, pred, bad, covered=not walk.startswith("lds_val") or _val_lds_width(D))
        _stream_check("forward_AGNN", walk, name, pred is not None and pred(kernel), env, bad)
        if walk == "auto":
            print("OBS forward_AGNN | auto | %s | D=%d | %s | chosen" % (name, D, kernel))
        failures += bad
    return failures


def _run_sddmm(dev, T, monkeypatch, name, D):
    (ref, r64, s64), (X, _), _ = _refs(name, D, "sddmm")
    rp, col = GRAPHS[name]
    meta = _meta(dev, name)
    tX = _cached(name, D, "tX", lambda: to_dev(dev, X)[0])
    failures, first = [], None
    if len(col) == 0:
        return failures
    for walk in _walks_for(name, "forward_ef"):
        mode, env, pred = W.SDDMM_WALKS[walk]

        def body():
            ef = T.forward_ef(tX, *meta)[0]
            k = T.last_kernel(*meta)
            return ef, k, T.forward_ef(tX, *meta)[0]
        try:
            ef, kernel, again = _forced(T, monkeypatch, mode, env, body)
        except RuntimeError as e:
            failures.append("forward_ef %s: %s" % (walk, e))
            continue
        bad = _judge(name, ef.cpu().numpy(), ref, r64, s64, "forward_ef %s (%s)" % (walk, kernel))
        if not torch.equal(ef, again):
            bad.append("forward_ef %s: the second call returns other bits" % walk)
        # every edge is scored once, from the same two rounded rows, whatever the walk: the same bits
        if first is None:
            first = ef
        elif not torch.equal(ef, first):
            bad.append("forward_ef %s: scores differ in bits from the automatic walk's" % walk)
        # (beyond 128 columns - ks = 5 - there is neither a range-major nor a slice-synchronised SDDMM: sddmm_wide_kernel, per window)
        _kernel_check("forward_ef", walk, name, D, kernel, (lambda k: pred(k, D)), bad, covered=walk == "auto" or D <= 128)
        if walk != "auto" and D > 128 and kernel != ("" if W.is_unsorted(name) else "sddmm_wide_kernel"):   # ("": sddmm_csr_kernel)
            bad.append("forward_ef %s D=%d: %r" % (walk, D, kernel))
        failures += bad
    return failures


def _run_fused(dev, T, monkeypatch, name, D):
    rp, col = GRAPHS[name]
    n, nnz = len(rp) - 1, len(col)
    _, (X, _), (bp, e2c, e2r) = _refs(name, D, "sddmm")
    meta = _meta(dev, name)
    H = (X / np.sqrt(D)).astype(np.float32)
    dY = np.random.default_rng(2000 + D).standard_normal((n, D)).astype(np.float32)
    tH, tdY = to_dev(dev, H, dY)
    wv = np.float32(0.7)
    tw = torch.tensor([wv], device=dev)
    rows = min(W.windows_handed_over(name, n) * 16, n)
    zero = _zero_rows(name)
    refs = {}

    def refs_for(ef_np):
        key = ef_np.tobytes()
        if key not in refs:
            att = (wv * ef_np).astype(np.float32)
            e = O.sddmm(H, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32); e64, es64 = O.sddmm_f64(H, rp, col)
            y = O.spmm_val(H, rp, col, att, bp, e2c, e2r, round_mode=O.ROUND_TF32); y64, ys64 = O.spmm_f64(H, rp, col, att)
            g = O.spmm_val(dY, rp, col, att, bp, e2c, e2r, round_mode=O.ROUND_TF32); g64, gs64 = O.spmm_f64(dY, rp, col, att)
            d_att = O.sddmm(dY, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32).astype(np.float64)
            for a in (y, y64, ys64, g, g64, gs64):
                a[rows:] = 0
            for a in (e, e64, es64, d_att):
                a[rp[rows]:] = 0
            refs.clear()
            refs[key] = ((e, e64, es64), (y, y64, ys64), (g, g64, gs64), float((d_att * col).sum()), float((np.abs(d_att) * col).sum()) + 1.0)
        return refs[key]
    failures = []
    for walk in _walks_for(name, "agnn_fused"):
        mode, env, pred = W.FUSED_WALKS[walk]

        def body():
            Y, ef, efmax = T.agnn_fused_forward(tH, meta[0], meta[1], tw, *meta[2:])
            kf = T.last_kernel(*meta)
            G, dw = T.agnn_fused_backward(tdY, meta[0], meta[1], tw, ef, efmax, *meta[2:])
            kb = T.last_kernel(*meta)
            G2, dw2 = T.agnn_fused_backward(tdY, meta[0], meta[1], tw, ef, efmax, *meta[2:])
            Y2 = T.agnn_fused_forward(tH, meta[0], meta[1], tw, *meta[2:])[0]
            return Y, ef, G, dw, kf, kb, torch.equal(G, G2) and torch.equal(dw, dw2) and torch.equal(Y, Y2)
        refusal = REFUSALS.get(("agnn_fused", name))
        try:
            Y, ef, G, dw, kf, kb, same = _forced(T, monkeypatch, mode, env, body)
        except RuntimeError as e:
            if refusal is None or refusal not in str(e):
                failures.append("agnn_fused %s: %s" % (walk, e))
            continue
        if refusal is not None:
            failures.append("agnn_fused %s: REFUSALS expects an error naming %r, the call went through (%r)" % (walk, refusal, kf))
        (e, e64, es64), (y, y64, ys64), (g, g64, gs64), want, term_scale = refs_for(ef.cpu().numpy())
        bad = _judge(name, ef.cpu().numpy(), e, e64, es64, "agnn_fused %s scores (%s)" % (walk, kf))
        bad += _judge(name, Y.cpu().numpy(), y, y64, ys64, "agnn_fused %s Y (%s)" % (walk, kf), zero)
        bad += _judge(name, G.cpu().numpy(), g, g64, gs64, "agnn_fused %s G (%s)" % (walk, kb), zero)
        if not abs(float(dw) - want) <= 1e-6 * term_scale:
            bad.append("agnn_fused %s: d_w %.6e, want %.6e (terms %.3e)" % (walk, float(dw), want, term_scale))
        if not same:
            bad.append("agnn_fused %s: a second call returns other bits" % walk)
        _kernel_check("agnn_fused", walk, name, D, kf, pred, bad)
        if pred is not None and not pred(kb) == pred(kf):
            bad.append("agnn_fused %s: forward took %r, backward %r" % (walk, kf, kb))
        if walk == "auto":
            print("OBS agnn_fused | auto | %s | D=%d | %s / %s | chosen" % (name, D, kf, kb))
        failures += bad
    return failures


RUNNERS = {"forward": _run_forward, "epilogues": _run_epilogues, "forward_AGNN": _run_agnn, "forward_ef": _run_sddmm, "agnn_fused": _run_fused}


@pytest.mark.parametrize("name,D,op", CASES, ids=["%s-D%d-%s" % c for c in CASES])
def test_every_walk_on_boundary_shaped_graphs(dev, T, monkeypatch, capfd, name, D, op):
    info = T.plan_info(*_meta(dev, name))
    rp, col = GRAPHS[name]
    n = len(rp) - 1
    assert info["num_windows"] == W.windows_handed_over(name, n) and info["canonical"] == (0 if W.is_unsorted(name) else 1)
    assert (info["column_buckets"] > 0) == (name not in SMALL_NAMES), info      # what NEEDS_BUCKETS rests on
    _CTX.update(capfd=capfd, n=n, D=D, buckets=info["column_buckets"])
    failures = RUNNERS[op](dev, T, monkeypatch, name, D)
    sys.stdout.write(capfd.readouterr().out)
    assert not failures, "%s D=%d %s:\n  " % (name, D, op) + "\n  ".join(failures)


def test_every_exception_names_a_pair_that_was_run():
    for (op, walk, name), why in EXCEPTIONS.items():
        assert op in WALKS and walk in WALKS[op] and name in GRAPHS and walk in _walks_for(name, op) and why, (op, walk, name)
        assert not (op == "forward" and walk in W.STRICT_FORWARD), "modes 1 and 4 have no way to another kernel: %s" % ((op, walk, name),)
    # the conditions the table states, from the CSR and the host SGT: hub windows (lds_has_hubs), E < 4, unsorted rows, 65 535 edges
    for name, (rp, col) in GRAPHS.items():
        n = len(rp) - 1
        bp = graphs.host_sgt(rp, col)[0][: W.windows_handed_over(name, n)]
        hubs = int(bp.max()) * len(bp) > 4 * max(int(bp.sum()), 1)
        assert hubs == (name in _HUB_GRAPHS), (name, hubs)
        csr = len(col) < 4 or W.is_unsorted(name)
        assert csr == (("forward_AGNN", "per_window", name) in EXCEPTIONS), name
        too_long = int(np.diff(rp[np.minimum(np.arange(len(bp) + 1) * 16, n)]).max()) >= 65535
        assert (too_long and not hubs and not csr) == (EXCEPTIONS.get(("forward_AGNN", "lds_val", name), "").startswith("a window of 65 535")), name


def test_every_walk_ran_its_own_kernel_on_half_of_its_graphs():
    """Runs behind the matrix, in the same process: per walk, on how many graphs the forced kernel ran (at every width the walk
    covers), so that EXCEPTIONS cannot swallow a walk.  The share is taken over the graphs whose plan can hold the walk at all - for
    the walks that need the column-bucket table, the five entries with 1 024 windows or more; for the slice-synchronised walk the two
    it is run on - and the count over everything it was run on is printed beside it."""
    assert RAN, "the matrix (test_every_walk_on_boundary_shaped_graphs) has to run before this test, in the same process"
    short = []
    for (op, walk), seen in sorted(RAN.items()):
        by_graph = {}
        for (name, D), ran in seen.items():
            by_graph[name] = by_graph.get(name, True) and ran
        eligible = [g for g in by_graph if not ((op, walk) in NEEDS_BUCKETS and g in SMALL_NAMES)]
        ok, total = sum(by_graph[g] for g in eligible), len(eligible)
        print("WALK %-12s %-20s forced kernel ran on %2d of %2d graphs that can hold it (%2d of the %2d it was run on)" % (
            op, walk, ok, total, sum(by_graph.values()), len(by_graph)))
        if 2 * ok < total or ok == 0:
            short.append((op, walk, ok, total))
    assert not short, short
    # the streams the flat walks built: dense entries on a quarter of the graphs at least where they were forced (TCGNN_LDS_DENSE_COLS=1
    # makes every cell that overflows its tiles a dense entry; cells of 32 columns or fewer - identity, the hub columns - have none)
    for (op, walk), seen in sorted(STREAMS.items()):
        with_dense = sum(1 for d in seen.values() if d > 0)
        print("STREAM %-12s %-16s flat streams on %2d graphs, dense entries on %2d" % (op, walk, len(seen), with_dense))
        if walk.endswith("_dense"):
            assert 4 * with_dense >= len(seen), (op, walk, seen)
