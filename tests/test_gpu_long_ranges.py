"""The long flat walk - 952-row LDS ranges, cell stream slot 7, spmm_lds_flat_long_kernel - forced with TCGNN_LDS_LONG=1 on the graphs of
tests/long_range_graphs.py, against the whole-product oracle.  Needs an MI355X: `pytest -m gpu`.

Every case runs in mode 3 with one tile per cell forced (TCGNN_LDS_FLAT=1, as the other flat-walk tests force it: the long stream exists
only as such a stream) and must hold assert_parity's three bounds, leave exact zeros in rows without edges and return the same bits from
a second call.

WHICH walk ran: TCGNN.last_kernel reports the kernel family, "spmm_lds_flat_kernel", for either range length (tests/test_gpu_scaled_spmm.py
pins that exact string on the headline graph, which takes the long walk), so the range length is read from the plan itself: its verbose
line "cell stream 7 (8 windows per wavefront, 952-row ranges)" - or, with TCGNN_LDS_LONG=0, "cell stream 4 (... 760-row ranges)" - and,
at D = 64, plan_info's range count.

  range arithmetic  N = 952 + 16, 2 x 952 (the sentinel row alone behind the last range), 2 x 952 + 1, 5 x 952 + 40 (both buffers wrap
                    twice); edges on local rows 0 and 951 of every range and on the last record of the image
  the pool          every cell of every window overflows its tile (about 50 columns): every wavefront of a pool group has a cold tile
                    waiting from the first entry on, and only its turn - one entry in eight - lets it gather; and three ranges with about
                    ten cold tiles per wavefront: most of the list goes to the loop behind the walk
  dense entries     blocks of windows with 300 columns in one range (TCGNN_LDS_DENSE_COLS lowered as the other tests lower it), one
                    block longer than a workgroup holds windows
  widths and forms  D = 128 (two long chunks), 96 and 41 (a long chunk beside a remainder pass on a shipped stream), 16 and 32 (no whole
                    64-column chunk: the shipped layouts, whatever the knob says), forward_fused with ReLU and with a gate,
                    forward_scaled (the _epi_ twin), transpose=True, and a wide-range matrix (the range guard's fallback inside the kernel)
  knob = 0          the same graphs on the shipped 760-row stream"""
import re
import sys

import numpy as np
import pytest
import torch

import long_range_graphs as LG
import walks as W
from oracle import oracle as O
from test_gpu_parity import to_dev

pytestmark = pytest.mark.gpu

GRAPHS = {name: (rp, col) for name, rp, col in LG.catalogue()}
LONG = {"TCGNN_LDS_FLAT": "1", "TCGNN_LDS_LONG": "1"}
SHIPPED = {"TCGNN_LDS_FLAT": "1", "TCGNN_LDS_LONG": "0"}
DENSE = {"TCGNN_LDS_DENSE_COLS": "64"}
POOL, LISTS, BLOCKS = "pool_every_cell_overflows_n4760", "pool_long_lists_three_ranges_n2856", "dense_blocks_n4800"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def T():
    import TCGNN
    return TCGNN


_META = {}


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_on_the_device(T):
    """the tests behind this file find the device as the tests before it left it: no tensor of this file alive, no cached plan, no cached block"""
    yield
    _META.clear()
    W._REFS.clear()
    T.clear_plan_cache()
    torch.cuda.empty_cache()


def _meta(dev, name):
    if name not in _META:
        _META.clear()
        rp, col = GRAPHS[name]
        bp, e2c, e2r = W.host_meta(rp, col)
        _META[name] = tuple(to_dev(dev, rp, col, bp, e2c, e2r))
    return _META[name]


def _streams(err):
    """{slot: (rows per range, cold tiles multiplied inside the kernel)} from the plan's verbose lines"""
    out = {}
    for slot, rows in re.findall(r"cell stream (\d+) \(\d+ windows per wavefront, (\d+)-row ranges\)", err):
        out[int(slot)] = int(rows)
    return out


def _run(T, monkeypatch, capfd, env, body):
    """body() in mode 3 under the knobs, from an empty plan cache -> (its result, the streams the plan built, stderr)"""
    monkeypatch.setenv("TCGNN_VERBOSE", "1")
    sys.stdout.write(capfd.readouterr().out)
    try:
        res = W.forced(T, monkeypatch, 3, env, body, {"n": 0, "D": 0, "capfd": None})
    finally:
        monkeypatch.delenv("TCGNN_VERBOSE", raising=False)
    out, err = capfd.readouterr()
    sys.stdout.write(out)
    return res, _streams(err), err


def _forward_case(dev, T, monkeypatch, capfd, name, D, env, want_slot):
    rp, col = GRAPHS[name]
    n = len(rp) - 1
    refs, (X, _), _ = W.references(name, rp, col, D, ops=("spmm",))
    meta = _meta(dev, name)
    tX = to_dev(dev, X)[0]

    def body():
        Y = T.forward(tX, *meta)[0]
        return Y, T.last_kernel(*meta), T.forward(tX, *meta)[0], T.plan_info(*meta)["lds_ranges"]
    (Y, kernel, again, ranges), streams, err = _run(T, monkeypatch, capfd, env, body)
    bad = W.judge(name, Y.cpu().numpy(), *refs["spmm"], "forward %s D=%d (%s)" % (name, D, kernel), W.zero_rows(name, rp))
    if not torch.equal(Y, again):
        bad.append("the second call returns other bits")
    if kernel != "spmm_lds_flat_kernel":
        bad.append("last_kernel is %r" % kernel)
    rows = {7: LG.LONG_ROWS, 4: LG.SHIPPED_ROWS}[want_slot]
    if streams.get(want_slot) != rows or (11 - want_slot) in streams:
        bad.append("the plan built the streams %r, wanted slot %d (%d-row ranges) and not slot %d: %s" % (streams, want_slot, rows, 11 - want_slot, err[-600:]))
    if D == 64 and ranges != (n + rows - 1) // rows:
        bad.append("plan_info counts %d ranges, %d-row ranges make %d" % (ranges, rows, (n + rows - 1) // rows))
    W._REFS.clear()
    assert not bad, "\n".join(bad)
    return err


@pytest.mark.parametrize("name", [k for k in GRAPHS if k.startswith("range_arithmetic")])
def test_range_arithmetic(dev, T, monkeypatch, capfd, name):
    _forward_case(dev, T, monkeypatch, capfd, name, 64, LONG, 7)


@pytest.mark.parametrize("name", [POOL, LISTS])
def test_the_shared_pool_of_cold_tiles(dev, T, monkeypatch, capfd, name):
    # (no dense entries: a cell of three tiles or more would otherwise turn its pair into a dense one, and nothing would be cold)
    err = _forward_case(dev, T, monkeypatch, capfd, name, 64, dict(LONG, TCGNN_LDS_DENSE_COLS="100000000"), 7)
    m = re.search(r"(\d+) tiles \+ (\d+) cold gather tiles", err)
    assert m and "multiplied inside the kernel" in err, err[-800:]
    nw = (len(GRAPHS[name][0]) - 1 + 15) // 16
    per_wave = int(m.group(2)) / nw                      # (one window per wavefront at this size)
    assert per_wave >= (8 if name == LISTS else 2), per_wave


def test_dense_entries_on_long_ranges(dev, T, monkeypatch, capfd):
    err = _forward_case(dev, T, monkeypatch, capfd, BLOCKS, 64, dict(LONG, **DENSE), 7)
    dense = [int(x) for x in re.findall(r"entries \((\d+) dense\)", err)]
    # (six windows in one workgroup; twenty-four in two or more: dense entries in at least three workgroups)
    assert dense and dense[0] >= 3, err[-800:]


@pytest.mark.parametrize("name", list(GRAPHS))
def test_knob_zero_keeps_the_shipped_stream(dev, T, monkeypatch, capfd, name):
    _forward_case(dev, T, monkeypatch, capfd, name, 64, dict(SHIPPED, **(DENSE if name == BLOCKS else {})), 4)


@pytest.mark.parametrize("name,D", [(POOL, 128), (POOL, 96), (POOL, 41), (BLOCKS, 128), ("range_arithmetic_n4800", 96)])
def test_widths_with_a_long_chunk(dev, T, monkeypatch, capfd, name, D):
    """two long chunks; a long chunk beside a remainder pass of two planes (4-window layout, slot 1) or of three planes (Reddit's 41
    classes: one more pair of 32-column chunks of the SAME long stream, the fourth plane all zeros)"""
    _forward_case(dev, T, monkeypatch, capfd, name, D, dict(LONG, **(DENSE if name == BLOCKS else {})), 7)


@pytest.mark.parametrize("D", [16, 32])
def test_narrow_widths_fall_back_to_the_shipped_layouts(dev, T, monkeypatch, capfd, D):
    name = POOL
    rp, col = GRAPHS[name]
    refs, (X, _), _ = W.references(name, rp, col, D, ops=("spmm",))
    meta = _meta(dev, name)
    tX = to_dev(dev, X)[0]

    def body():
        Y = T.forward(tX, *meta)[0]
        return Y, T.last_kernel(*meta), T.forward(tX, *meta)[0]
    (Y, kernel, again), streams, err = _run(T, monkeypatch, capfd, LONG, body)
    bad = W.judge(name, Y.cpu().numpy(), *refs["spmm"], "forward D=%d (%s)" % (D, kernel), W.zero_rows(name, rp))
    W._REFS.clear()
    assert not bad, "\n".join(bad)
    assert torch.equal(Y, again)
    assert kernel.startswith("spmm_lds_flat_kernel"), kernel
    assert 7 not in streams and 4 not in streams and streams, (streams, err[-600:])     # (4-window layout: slot 2 / slot 1)


def test_fused_scaled_and_transposed_forms(dev, T, monkeypatch, capfd):
    name, D = POOL, 64
    rp, col = GRAPHS[name]
    n = len(rp) - 1
    refs, (X, _), (bp, e2c, e2r) = W.references(name, rp, col, D, ops=("spmm",))
    ref, r64, s64 = refs["spmm"]
    meta = _meta(dev, name)
    zero = W.zero_rows(name, rp)
    rng = np.random.default_rng(77)
    gate = rng.standard_normal((n, D)).astype(np.float32)
    r = rng.uniform(0.1, 1.0, n).astype(np.float32); c = rng.uniform(0.1, 1.0, n).astype(np.float32); b = rng.standard_normal(D).astype(np.float32)
    tX, tg, tr, tc, tb = to_dev(dev, X, gate, r, c, b)
    Xg = (X * (gate > 0)).astype(np.float32)
    Xc = (c[:, None] * X).astype(np.float32)
    trp, tcol, _ = W.transposed_csr(rp, col)
    tmeta = W.host_meta(trp, tcol)

    def body():
        out = {}
        for what, call in (("relu", lambda: T.forward_fused(tX, *meta, relu=True)[0]), ("gate", lambda: T.forward_fused(tX, *meta, gate=tg)[0]),
                           ("scaled", lambda: T.forward_scaled(tX, *meta, row_scale=tr, col_scale=tc, bias=tb, relu=True)[0]),
                           ("transpose", lambda: T.forward(tX, *meta, transpose=True)[0])):
            y = call()
            k = T.last_kernel(*meta, transpose=what == "transpose")
            out[what] = (y, k, call())
        return out
    out, streams, err = _run(T, monkeypatch, capfd, LONG, body)
    bad = []
    for what, (y, k, again) in out.items():
        if not torch.equal(y, again):
            bad.append("%s: the second call returns other bits" % what)
        if k != "spmm_lds_flat_kernel":
            bad.append("%s: last_kernel is %r" % (what, k))
    assert streams.get(7) == LG.LONG_ROWS and 4 not in streams, (streams, err[-600:])
    assert len(re.findall(r"cell stream 7 \(", err)) == 2, "A and A^T each build a long stream"
    bad += W.judge(name, out["relu"][0].cpu().numpy(), np.maximum(ref, 0), np.maximum(r64, 0), s64, "forward_fused relu", zero)
    g = O.spmm(Xg, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32); g64, gs64 = O.spmm_f64(Xg, rp, col)
    bad += W.judge(name, out["gate"][0].cpu().numpy(), g, g64, gs64, "forward_fused gate", zero)
    a = O.spmm(Xc, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32); a64, as64 = O.spmm_f64(Xc, rp, col)
    pre = (a * r[:, None] + b).astype(np.float32); pre64 = a64 * r[:, None].astype(np.float64) + b.astype(np.float64)
    bad += W.judge(name, out["scaled"][0].cpu().numpy(), np.maximum(pre, 0), np.maximum(pre64, 0), as64 * r[:, None].astype(np.float64) + np.abs(b).astype(np.float64),
                   "forward_scaled", zero, np.maximum(b, 0))
    t = O.spmm(X, trp, tcol, *tmeta, round_mode=O.ROUND_TF32); t64, ts64 = O.spmm_f64(X, trp, tcol)
    bad += W.judge(name, out["transpose"][0].cpu().numpy(), t, t64, ts64, "forward transpose=True", np.diff(trp) == 0)
    W._REFS.clear()
    assert not bad, "\n".join(bad)


def test_wide_range_matrix_takes_the_fallback_inside_the_long_kernel(dev, T, monkeypatch, capfd):
    """include/tcgnn.h "Operand range": one row of 3e7 over 1e-3 data is "wide" - the kernel returns into the fp32 walk at its top
    (lds_own_fallback: a single launch, binary A, whole rows).  Judged against fp64 on the unrounded operands, relative to
    sum |a||x| + 1, at the 2^-9 the fp32-MFMA walk's 10-bit operands allow."""
    name, D = "range_arithmetic_n4800", 64
    rp, col = GRAPHS[name]
    n = len(rp) - 1
    rng = np.random.default_rng(9)
    X = (rng.standard_normal((n, D)) * 1e-3).astype(np.float32)
    X[777] = 3e7 * (1.0 + rng.random(D).astype(np.float32))
    r64, s64 = O.spmm_f64(X, rp, col)
    meta = _meta(dev, name)
    tX = to_dev(dev, X)[0]

    def body():
        Y = T.forward(tX, *meta)[0]
        return Y, T.last_kernel(*meta), T.forward(tX, *meta)[0]
    (Y, kernel, again), streams, err = _run(T, monkeypatch, capfd, LONG, body)
    assert kernel == "spmm_lds_flat_kernel" and streams.get(7) == LG.LONG_ROWS, (kernel, streams)
    got = Y.cpu().numpy()
    assert np.isfinite(got).all()
    assert (np.abs(got - r64) / (s64 + 1.0)).max() <= 2.0 ** -9
    assert torch.equal(Y, again)
    assert not got[W.zero_rows(name, rp)].any()
