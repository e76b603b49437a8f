"""The range guard's patch (wide_patch_kernel, tcgnn_small_fallback.inc) edge by edge.  Needs an MI355X: `pytest -m gpu`.

At the default guard level the MFMA kernels of SDDMM and of the fused AGNN pair run on the fp16 image and the patch, one launch behind
them, recomputes in fp32 every edge that touches a DIRTY row of X (a row with elements the image loses).  The inputs of
tests/patch_ref.py make each such edge visible on its own: a dirty row is zero in the image, so an edge the patch skipped keeps the
score 0 and misses by its whole sum of |terms|, and a correction added twice doubles a dirty row's row of Y
(tests/test_patch_ref_cpu.py shows, without a GPU, that these inputs carry every bound used here).

Operators: forward_ef (patch mode 0), agnn_fused_forward (mode 1), agnn_fused_backward (mode 2: dY built like X; ef and ef_absmax saved
from a forward on ordinary X, so that the backward's own patch is what is judged).  Guard level 2 is the subject, level 1 the
unpatched control, level 3 the dense fp32 way (wide_dense_body).  Every case asserts:

  * range_mode reports what the numpy mirror of the staging rule predicts (2 / 0 / 1), and the mirror's dirty rows are the intended ones;
  * every score is within 4 x TIGHT of the TF32-mode oracle relative to the edge's own sum of |terms| - the touched edges of covered
    rows judged on their own - and at level 1 at least 99 % of those touched edges are NOT (the control: the input discriminates on
    this GPU as it does in the emulation);
  * every untouched edge is bit-equal to the level-1 call, element by element; every edge of a row behind the windows the plan was
    given is exactly 0 at levels 2 and 3;
  * Y and G are within 256 x TIGHT of the oracle's edge-valued SpMM per element, relative to the element's own sum of |terms| - the
    dirty rows' own rows of Y, and in the 17-row clique every row of G, consist of nothing but patched terms - with exact zeros behind
    the windows; rows of G with no dirty neighbour are bit-equal to the level-1 call;
  * d_w within 1e-5 of the sum of |terms| + 1 (rows behind the windows excluded); int(ef_absmax[0]) is the bits of max |ef|;
  * the same call twice returns bit-equal scores (Y, G and d_w collect atomics in no fixed order: judged by their bounds, both calls);
  * on the uniform graph with 3 and 256 dirty rows the scan (TCGNN_PATCH_ROWS=0) returns the row-driven branch's scores bit for bit.

Graphs: the two catalogue entries of the r11 finding (identity_n4103; short_metadata_n4100, whose dirty row N - 2 lies behind the
windows handed over), the symmetric uniform 4 000 x 100 graph with 1 / 3 / 256 / 257 dirty rows (kPatchRowDriven = 256: row-driven up
to it, the scan beyond), its directed form (the scan), hub rows, the clique of patch_ref.clique17_graph, and two rings either side of
the 15 360-word LDS bitmap (kPatchBitmapWords).  Widths 5 / 41 / 64 / 128, and 200 for forward_ef (sddmm_wide_kernel).

The forced walks (xcd1 for the SDDMM; sliced2 and range_major for the fused pair, through walks.forced) run on the same uniform
generator at 16 400 nodes: those walks need the plan's column-bucket table, which tcgnn_plan_create builds from 1 024 windows on - on
the 250 windows of the 4 000-node graph every one of them is the per-window walk under another name, and TCGNN_AGNN_SLICED=2 reports
"agnn_kernel" there.  A last_kernel that is not the table's (tests/walks.py), a plan without buckets, or a range count that is no
multiple of eight is a failure."""
import sys

import numpy as np
import pytest
import torch

import patch_ref as P
import walks as W
from test_gpu_parity import to_dev

pytestmark = pytest.mark.gpu

OPS = ("sddmm", "fused_forward", "fused_backward")
CASES = [(c, op) for c in P.CASES for op in OPS if op == "sddmm" or c[1] <= 128]
FORCED = [("sddmm", "xcd1"), ("fused_forward", "sliced2"), ("fused_backward", "sliced2"), ("fused_forward", "range_major"), ("fused_backward", "range_major")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def T():
    import TCGNN
    return TCGNN


_CASE = {"key": None}


def _shared(case, what, make):
    """per case, built once and left unchanged: the graph's metadata, the matrices, the references"""
    if _CASE["key"] != case:
        _CASE.clear(); _CASE["key"] = case
    if what not in _CASE:
        _CASE[what] = make()
    return _CASE[what]


def _setup(dev, case):
    name, D, k = case
    rp, col = P.graph(name)
    n = len(rp) - 1
    host = _shared(case, "host", lambda: W.host_meta(rp, col))
    meta = _shared(case, "meta", lambda: tuple(to_dev(dev, rp, col, host[0][: P.windows_handed_over(name, n)], host[1], host[2])))
    rows = P.case_rows(name, k)
    covered_rows = P.covered_rows(name, n)
    return {"name": name, "D": D, "k": k, "rp": rp, "col": col, "n": n, "host": host, "meta": meta, "rows": rows,
            "covered_rows": covered_rows, "covered": np.arange(len(col)) < rp[covered_rows],
            "touched": _shared(case, "touched", lambda: P.touched_edges(rp, col, rows)),
            "erow": _shared(case, "erow", lambda: np.repeat(np.arange(n), np.diff(rp)))}


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _at_level(T, level, body):
    T.set_range_guard(level)
    out = body()
    return out, T.range_mode()[0]


class Findings(list):
    def need(self, ok, text, *args):
        if not ok:
            self.append(text % args)


def _judge_scores(c, bad, what, X, ef2, ef2b, ef1, ef3, refs):
    """the scores of one operator at levels 2 (twice), 1 and 3 -> the largest ratios"""
    ref, _, s64, _ = refs
    cov, touched = c["covered"], c["touched"]
    judged = touched & cov
    r2, r3, r1 = P.ratio(ef2, ref, s64), P.ratio(ef3, ref, s64), P.ratio(ef1, ref, s64)
    bad.need(np.isfinite(ef2).all() and np.isfinite(ef3).all(), "%s: non-finite scores", what)
    bad.need(judged.sum() >= c["k"], "%s: %d touched edges of covered rows", what, judged.sum())
    over = judged & (r2 > P.SCORE_BOUND)
    bad.need(not over.any(), "%s level 2: %d of %d touched edges beyond 4 x TIGHT (worst %.3e, first edges %s)", what, over.sum(), judged.sum(),
             r2[judged].max(), np.flatnonzero(over)[:6])
    bad.need(r2.max() <= P.SCORE_BOUND, "%s level 2: %.3e from the oracle somewhere", what, r2.max())
    bad.need(r3.max() <= P.SCORE_BOUND, "%s level 3: %.3e from the oracle", what, r3.max())
    bad.need((r1[judged] > P.SCORE_BOUND).sum() >= 0.99 * judged.sum(), "%s level 1 (control): only %d of %d touched edges miss unpatched", what,
             (r1[judged] > P.SCORE_BOUND).sum(), judged.sum())
    diff = np.ascontiguousarray(ef2).view(np.uint32) != np.ascontiguousarray(ef1).view(np.uint32)
    bad.need(not (diff & ~touched).any(), "%s: %d untouched edges differ from the level-1 call", what, (diff & ~touched).sum())
    for lv, ef in ((2, ef2), (3, ef3)):
        bad.need(not ef[~cov].any(), "%s level %d: %d nonzero scores in rows behind the windows", what, lv, np.count_nonzero(ef[~cov]))
    nd = int((np.ascontiguousarray(ef2).view(np.uint32) != np.ascontiguousarray(ef2b).view(np.uint32)).sum())
    bad.need(nd == 0, "%s: a second call differs in %d scores (by up to %.3e of max |ef|)", what, nd, np.abs(ef2 - ef2b).max() / max(np.abs(ef2).max(), 1e-30))
    return r2[judged].max(), r2.max(), r3.max()


def _judge_agg(c, bad, what, got, ref3):
    ref, _, s64 = ref3
    r = P.ratio(got, ref, s64)
    bad.need(np.isfinite(got).all(), "%s: non-finite elements", what)
    over = r > P.AGG_BOUND
    bad.need(not over.any(), "%s: %d elements beyond 256 x TIGHT (worst %.3e, rows %s)", what, over.sum(), r.max(), np.flatnonzero(over.any(axis=1))[:6])
    bad.need(not got[c["covered_rows"]:].any(), "%s: %d nonzero elements in rows behind the windows", what, np.count_nonzero(got[c["covered_rows"]:]))
    return r.max()


def _modes(bad, what, X, D, got):
    want = [P.range_mode(X, D, lv) for lv in (2, 1, 3)]
    bad.need(want == [2, 0, 1], "%s: the mirror predicts %s", what, want)
    bad.need(list(got) == want, "%s: range_mode reports %s at levels 2 / 1 / 3, the mirror predicts %s", what, list(got), want)


def _scan_too(c):
    return c["name"] == "uniform_n4000" and c["k"] in (3, 256)


def _run_sddmm(dev, T, monkeypatch, case, bad, name_pred=None):
    c = _setup(dev, case)
    D, meta = c["D"], c["meta"]
    X = _shared(case, "X", lambda: P.wide_matrix(c["n"], D, c["rows"]))
    bad.need(np.array_equal(P.dirty_rows(X), np.sort(c["rows"])), "the mirror finds dirty rows %s", P.dirty_rows(X)[:8])
    refs = _shared(case, "score_refs", lambda: P.score_refs(c["name"], X, c["host"]))
    tX = to_dev(dev, X)[0]

    def call():
        return T.forward_ef(tX, *meta)[0].cpu().numpy()
    ef2, m2 = _at_level(T, 2, call)
    kernel = T.last_kernel(*meta)
    ef2b, _ = _at_level(T, 2, call)
    scan = None
    if _scan_too(c):
        monkeypatch.setenv("TCGNN_PATCH_ROWS", "0")
        try:
            scan, _ = _at_level(T, 2, call)
        finally:
            monkeypatch.delenv("TCGNN_PATCH_ROWS")
    ef1, m1 = _at_level(T, 1, call)
    ef3, m3 = _at_level(T, 3, call)
    _modes(bad, "forward_ef", X, D, (m2, m1, m3))
    pred = name_pred or (lambda k: W.SDDMM_WALKS["auto"][2](k, D))
    bad.need(pred(kernel), "forward_ef: last_kernel is %r", kernel)
    fig = _judge_scores(c, bad, "forward_ef", X, ef2, ef2b, ef1, ef3, refs)
    if scan is not None:
        bad.need(_bits_equal(scan, ef2), "forward_ef: the scan differs from the row-driven branch in %d scores", (scan != ef2).sum())
    print("FIG %-32s forward_ef     (%s) touched %.2e all %.2e level3 %.2e" % (P.case_id(case), kernel, *fig))


def _run_fused_forward(dev, T, monkeypatch, case, bad, name_pred=None):
    c = _setup(dev, case)
    D, meta = c["D"], c["meta"]
    X = _shared(case, "X", lambda: P.wide_matrix(c["n"], D, c["rows"]))
    refs = _shared(case, "score_refs", lambda: P.score_refs(c["name"], X, c["host"]))
    tX = to_dev(dev, X)[0]
    tw = torch.tensor([P.W_ATT], device=dev)

    def call():
        Y, ef, efm = T.agnn_fused_forward(tX, meta[0], meta[1], tw, *meta[2:])
        return Y.cpu().numpy(), ef.cpu().numpy(), int(efm[0].item())
    (Y2, ef2, mx2), m2 = _at_level(T, 2, call)
    kernel = T.last_kernel(*meta)
    (Y2b, ef2b, _), _ = _at_level(T, 2, call)
    scan = None
    if _scan_too(c):
        monkeypatch.setenv("TCGNN_PATCH_ROWS", "0")
        try:
            scan, _ = _at_level(T, 2, call)
        finally:
            monkeypatch.delenv("TCGNN_PATCH_ROWS")
    (Y1, ef1, _), m1 = _at_level(T, 1, call)
    (Y3, ef3, mx3), m3 = _at_level(T, 3, call)
    _modes(bad, "fused forward", X, D, (m2, m1, m3))
    if name_pred is not None:
        bad.need(name_pred(kernel), "fused forward: last_kernel is %r", kernel)
    fig = _judge_scores(c, bad, "fused forward", X, ef2, ef2b, ef1, ef3, refs)
    for lv, ef, mx in ((2, ef2, mx2), (3, ef3, mx3)):
        bad.need(mx == int(np.abs(ef).max().view(np.int32)), "fused forward level %d: ef_absmax[0] = %#x, max |ef| = %#x", lv, mx, int(np.abs(ef).max().view(np.int32)))
    refY = P.agg_refs(c["name"], X, (P.W_ATT * ef2).astype(np.float32), c["host"])
    figY = [_judge_agg(c, bad, "Y level 2" + tag, Y, refY) for tag, Y in (("", Y2), (" (second call)", Y2b))]
    figY.append(_judge_agg(c, bad, "Y level 3", Y3, P.agg_refs(c["name"], X, (P.W_ATT * ef3).astype(np.float32), c["host"])))
    # the control: a dirty row's own row of Y consists of patched terms only - unpatched, it is nowhere near
    own = [r for r in c["rows"] if r < c["covered_rows"] and c["rp"][r + 1] > c["rp"][r]]
    bad.need(len(own) > 0 and all(P.ratio(Y1[r], refY[0][r], refY[2][r]).max() > P.AGG_BOUND for r in own), "Y level 1 (control): a dirty row's row of Y passes unpatched")
    if scan is not None:
        bad.need(_bits_equal(scan[1], ef2), "fused forward: the scan differs from the row-driven branch in %d scores", (scan[1] != ef2).sum())
        _judge_agg(c, bad, "Y level 2 (scan)", scan[0], refY)
    print("FIG %-32s fused forward  (%s) touched %.2e all %.2e level3 %.2e Y %.2e / %.2e level3 %.2e" % (P.case_id(case), kernel, *fig, *figY))


def _run_fused_backward(dev, T, monkeypatch, case, bad, name_pred=None):
    c = _setup(dev, case)
    D, meta, rp, col = c["D"], c["meta"], c["rp"], c["col"]
    X0 = P.ordinary_matrix(c["n"], D)[0]
    dY = _shared(case, "dY", lambda: P.wide_matrix(c["n"], D, c["rows"], salt=1))
    bad.need(np.array_equal(P.dirty_rows(dY), np.sort(c["rows"])), "the mirror finds dirty rows %s in dY", P.dirty_rows(dY)[:8])
    tX0, tdY = to_dev(dev, X0, dY)
    tw = torch.tensor([P.W_ATT], device=dev)
    (Y0, ef, efm), m0 = _at_level(T, 2, lambda: T.agnn_fused_forward(tX0, meta[0], meta[1], tw, *meta[2:]))
    bad.need(m0 == 0 == P.range_mode(X0, D, 2), "the forward call on ordinary X reports range_mode %d", m0)
    att = (P.W_ATT * ef.cpu().numpy()).astype(np.float32)

    def call():
        G, dw = T.agnn_fused_backward(tdY, meta[0], meta[1], tw, ef, efm, *meta[2:])
        return G.cpu().numpy(), float(dw)
    (G2, dw2), m2 = _at_level(T, 2, call)
    kernel = T.last_kernel(*meta)
    (G2b, dw2b), _ = _at_level(T, 2, call)
    (G1, _), m1 = _at_level(T, 1, call)
    (G3, dw3), m3 = _at_level(T, 3, call)
    _modes(bad, "fused backward", dY, D, (m2, m1, m3))
    if name_pred is not None:
        bad.need(name_pred(kernel), "fused backward: last_kernel is %r", kernel)
    refG = P.agg_refs(c["name"], dY, att, c["host"])
    figG = [_judge_agg(c, bad, "G " + tag, G, refG) for tag, G in (("level 2", G2), ("level 2 (second call)", G2b), ("level 3", G3))]
    # rows of G none of whose neighbours is dirty get no correction: the MFMA kernel's bits
    dirty_col = np.isin(col, c["rows"])
    clean = np.ones(c["n"], bool); clean[c["erow"][dirty_col]] = False
    bad.need(_bits_equal(G2[clean], G1[clean]), "G: %d rows without a dirty neighbour differ from the level-1 call", (G2[clean] != G1[clean]).any(axis=1).sum())
    if c["name"] == "clique17_n700":       # nothing but lost terms: the control misses every one of these rows, the patch none
        bad.need(all(P.ratio(G1[r], refG[0][r], refG[2][r]).max() > P.AGG_BOUND for r in c["rows"]), "G level 1 (control): a clique row passes unpatched")
    d_att, _, d_s64, _ = _shared(case, "dY_score_refs", lambda: P.score_refs(c["name"], dY, c["host"]))
    want, scale = float((d_att.astype(np.float64) * col).sum()), float((d_s64 * col).sum()) + 1.0
    figw = []
    for tag, dw in (("level 2", dw2), ("level 2 (second call)", dw2b), ("level 3", dw3)):
        figw.append(abs(dw - want) / scale)
        bad.need(figw[-1] <= P.DW_BOUND, "d_w %s: %.9e, want %.9e (%.3e of the terms)", tag, dw, want, figw[-1])
    print("FIG %-32s fused backward (%s) G %.2e / %.2e level3 %.2e d_w %.2e / %.2e level3 %.2e" % (P.case_id(case), kernel, *figG, *figw))


RUNNERS = {"sddmm": _run_sddmm, "fused_forward": _run_fused_forward, "fused_backward": _run_fused_backward}


def _guarded(T, body):
    try:
        return body()
    finally:
        T.set_range_guard(2)      # the default level, whatever happened
        T.clear_plan_cache()


@pytest.mark.parametrize("case,op", CASES, ids=["%s-%s" % (P.case_id(c), op) for c, op in CASES])
def test_patch_edge_by_edge(dev, T, monkeypatch, case, op):
    c = _setup(dev, case)
    info = T.plan_info(*c["meta"])
    assert info["num_windows"] == P.windows_handed_over(c["name"], c["n"]) and info["canonical"] == 1
    bad = Findings()
    _guarded(T, lambda: RUNNERS[op](dev, T, monkeypatch, case, bad))
    assert not bad, "%s %s:\n  " % (P.case_id(case), op) + "\n  ".join(bad)


@pytest.mark.parametrize("op,walk", FORCED, ids=["%s-%s" % f for f in FORCED])
def test_patch_behind_the_forced_walks(dev, T, monkeypatch, op, walk):
    case = P.WALK_CASE
    c = _setup(dev, case)
    n, D = c["n"], c["D"]
    mode, env, pred = (W.SDDMM_WALKS if op == "sddmm" else W.FUSED_WALKS)[walk]
    name_pred = (lambda k: pred(k, D)) if op == "sddmm" else pred
    bad = Findings()
    buckets = T.plan_info(*c["meta"])["column_buckets"]
    nr = W.expected_ranges(n, D, buckets, W.range_kb_for_eight(n, D))
    bad.need(buckets > 0, "the plan holds no column-bucket table: %s is the per-window walk under another name", walk)
    if walk != "sliced2":          # (the range-major walks carry the per-window kernel's name: the range count shows that they ran)
        bad.need(nr >= 8 and nr % 8 == 0, "%s: %d column ranges", walk, nr)
    ctx = {"n": n, "D": D, "capfd": None}
    _guarded(T, lambda: W.forced(T, monkeypatch, mode, env, lambda: RUNNERS[op](dev, T, monkeypatch, case, bad, name_pred), ctx))
    sys.stdout.flush()
    assert not bad, "%s %s under %s:\n  " % (P.case_id(case), op, walk) + "\n  ".join(bad)
