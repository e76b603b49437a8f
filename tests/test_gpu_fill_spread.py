"""The long flat walk's two fill schedules - TCGNN_LDS_FILL_SPREAD=1 (default: a normal entry's range fill goes out one LDS-DMA
instruction per filling wavefront in front of its tile steps) against =0 (the whole fill in one burst at the entry's top) - on the
952-row stream, forced with TCGNN_LDS_LONG=1 as tests/test_gpu_long_ranges.py forces it.  Needs an MI355X: `pytest -m gpu`.

The products and their order are the same under both schedules - only when the bytes land in LDS changes - so every case asks for
BIT-FOR-BIT equal results from the two on ONE plan (the knob is read per launch), and for the project's SpMM bounds against the oracle
(walks.judge: assert_parity's three bounds, exact zeros in rows without edges).  That the 952-row stream ran is read from the plan's
verbose line "cell stream 7 (8 windows per wavefront, 952-row ranges)".

  range arithmetic   the four graphs of long_range_graphs.py: every boundary record of the range list, several ranges and a short last one;
                     a workgroup of such a graph holds one window per wavefront, so all sixteen have an empty last slot, all sixteen
                     fill, and every one leaves the tile walk at the `break` in front of the empty slot
  light fillers      14 592 windows = 128 workgroups x 114: a workgroup deals 7 windows to most wavefronts and 8 to two or three, so the
                     light ones (at least twelve) take the fills and the full ones issue none
  all full           16 384 windows = 128 workgroups x 128 window slots: no wavefront has an empty slot, all sixteen fill and none breaks out
  widths             D = 128 (two long chunks), 96 (long chunk + a remainder on a shipped layout), 41 (a plane beyond the matrix)
  dense entries      the dense-blocks graph: normal entries spread, dense entries burst, the buffer parity across the phase change
  skipped fills      one range only (no entry names a range to fetch: the prologue's fill alone), and two ranges (workgroups of one or
                     two entries)
  forms              forward_scaled (the _epi_ twin) and forward_fused with ReLU once each; a wide-range matrix, which leaves the kernel
                     at its top for the fp32 fallback under either schedule"""
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

LONG = {"TCGNN_LDS_FLAT": "1", "TCGNN_LDS_LONG": "1"}
DENSE = {"TCGNN_LDS_DENSE_COLS": "64"}
KNOB = "TCGNN_LDS_FILL_SPREAD"
BLOCKS = "dense_blocks_n4800"


def _sparse_graph(n, seed):
    """three edges per row to columns all over the graph (every range of every workgroup holds a few), EMPTY_ROWS left empty"""
    rng = np.random.default_rng(seed)
    m = 3 * n
    return LG._finish(rng.integers(0, n, size=m), rng.integers(0, n, size=m), n)


def _catalogue():
    out = {name: (rp, col) for name, rp, col in LG.catalogue() if name.startswith("range_arithmetic") or name == BLOCKS}
    out["single_range_n900"] = LG.range_arithmetic_graph(900, seed=41)
    out["two_ranges_n1200"] = LG.range_arithmetic_graph(1200, seed=42)
    return out


class _Graphs(dict):
    """(the two graphs of Reddit's size are built when their test runs, not when the file is collected)"""
    BIG = {"light_fillers_n233472": (16 * 128 * 114, 43), "all_full_n262144": (16 * 128 * 128, 44)}

    def __missing__(self, name):
        self[name] = _sparse_graph(*self.BIG[name])
        return self[name]


GRAPHS = _Graphs(_catalogue())
SMALL = [k for k in GRAPHS if k.startswith("range_arithmetic")]


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
    yield
    _META.clear()
    W._REFS.clear()
    T.clear_plan_cache()
    torch.cuda.empty_cache()


def _meta(dev, name):
    if name not in _META:
        _META.clear()
        rp, col = GRAPHS[name]
        _META[name] = tuple(to_dev(dev, rp, col, *W.host_meta(rp, col)))
    return _META[name]


def _both(T, monkeypatch, capfd, env, call):
    """call() under the burst and under the spread schedule on one plan, mode 3 -> (Y burst, Y spread, Y spread again, stderr)"""
    monkeypatch.setenv("TCGNN_VERBOSE", "1")
    sys.stdout.write(capfd.readouterr().out)

    def body():
        monkeypatch.setenv(KNOB, "0")
        burst = call()
        monkeypatch.setenv(KNOB, "1")
        spread = call()
        monkeypatch.delenv(KNOB)
        return burst, spread, call()
    try:
        res = W.forced(T, monkeypatch, 3, env, body, {"n": 0, "D": 0, "capfd": None})
    finally:
        monkeypatch.delenv("TCGNN_VERBOSE", raising=False)
        monkeypatch.delenv(KNOB, raising=False)
    out, err = capfd.readouterr()
    sys.stdout.write(out)
    return (*res, err)


def _long_stream_ran(err):
    rows = {int(s): int(r) for s, r in re.findall(r"cell stream (\d+) \(\d+ windows per wavefront, (\d+)-row ranges\)", err)}
    assert rows.get(7) == LG.LONG_ROWS and 4 not in rows, (rows, err[-600:])


def _case(dev, T, monkeypatch, capfd, name, D, env=LONG):
    rp, col = GRAPHS[name]
    refs, (X, _), _ = W.references(name, rp, col, D, ops=("spmm",))
    meta = _meta(dev, name)
    tX = to_dev(dev, X)[0]
    burst, spread, default, err = _both(T, monkeypatch, capfd, env, lambda: T.forward(tX, *meta)[0])
    _long_stream_ran(err)
    bad = W.judge(name, spread.cpu().numpy(), *refs["spmm"], "forward %s D=%d spread" % (name, D), W.zero_rows(name, rp))
    bad += W.judge(name, burst.cpu().numpy(), *refs["spmm"], "forward %s D=%d burst" % (name, D), W.zero_rows(name, rp))
    if not torch.equal(burst, spread):
        bad.append("the spread schedule returns other bits than the burst: %d elements" % int((burst != spread).sum()))
    if not torch.equal(spread, default):
        bad.append("the default is not the spread schedule's result")
    W._REFS.clear()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", SMALL)
def test_range_arithmetic(dev, T, monkeypatch, capfd, name):
    _case(dev, T, monkeypatch, capfd, name, 64)


@pytest.mark.parametrize("name", ["light_fillers_n233472", "all_full_n262144"])
def test_who_fills(dev, T, monkeypatch, capfd, name):
    _case(dev, T, monkeypatch, capfd, name, 64)


@pytest.mark.parametrize("D", [128, 96, 41])
def test_widths(dev, T, monkeypatch, capfd, D):
    _case(dev, T, monkeypatch, capfd, "range_arithmetic_n4800", D)


def test_dense_entries_keep_the_burst(dev, T, monkeypatch, capfd):
    _case(dev, T, monkeypatch, capfd, BLOCKS, 64, dict(LONG, **DENSE))


@pytest.mark.parametrize("name", ["single_range_n900", "two_ranges_n1200"])
def test_entries_without_a_fill(dev, T, monkeypatch, capfd, name):
    _case(dev, T, monkeypatch, capfd, name, 64)


def test_scaled_and_relu_forms(dev, T, monkeypatch, capfd):
    name, D = "range_arithmetic_n4800", 64
    rp, col = GRAPHS[name]
    n = len(rp) - 1
    refs, (X, _), (bp, e2c, e2r) = W.references(name, rp, col, D, ops=("spmm",))
    ref, r64, s64 = refs["spmm"]
    meta = _meta(dev, name)
    zero = W.zero_rows(name, rp)
    rng = np.random.default_rng(78)
    r = rng.uniform(0.1, 1.0, n).astype(np.float32); c = rng.uniform(0.1, 1.0, n).astype(np.float32); b = rng.standard_normal(D).astype(np.float32)
    tX, tr, tc, tb = to_dev(dev, X, r, c, b)
    Xc = (c[:, None] * X).astype(np.float32)
    bad = []
    burst, spread, _, err = _both(T, monkeypatch, capfd, LONG, lambda: T.forward_fused(tX, *meta, relu=True)[0])
    _long_stream_ran(err)
    bad += W.judge(name, spread.cpu().numpy(), np.maximum(ref, 0), np.maximum(r64, 0), s64, "forward_fused relu spread", zero)
    if not torch.equal(burst, spread):
        bad.append("relu: the spread schedule returns other bits than the burst")
    burst, spread, _, err = _both(T, monkeypatch, capfd, LONG, lambda: T.forward_scaled(tX, *meta, row_scale=tr, col_scale=tc, bias=tb, relu=True)[0])
    _long_stream_ran(err)
    a = O.spmm(Xc, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32); a64, as64 = O.spmm_f64(Xc, rp, col)
    pre = (a * r[:, None] + b).astype(np.float32); pre64 = a64 * r[:, None].astype(np.float64) + b.astype(np.float64)
    bad += W.judge(name, spread.cpu().numpy(), np.maximum(pre, 0), np.maximum(pre64, 0), as64 * r[:, None].astype(np.float64) + np.abs(b).astype(np.float64),
                   "forward_scaled spread", zero, np.maximum(b, 0))
    if not torch.equal(burst, spread):
        bad.append("scaled: the spread schedule returns other bits than the burst")
    W._REFS.clear()
    assert not bad, "\n".join(bad)


def test_wide_range_matrix_takes_the_fallback_under_either_schedule(dev, T, monkeypatch, capfd):
    """one row of 3e7 over 1e-3 data is "wide": the kernel returns into the fp32 walk at its top; fp64 on the unrounded operands,
    relative to sum |a||x| + 1, at the 2^-9 of that walk's 10-bit operands (as tests/test_gpu_long_ranges.py judges it)"""
    name, D = "range_arithmetic_n4800", 64
    rp, col = GRAPHS[name]
    n = len(rp) - 1
    rng = np.random.default_rng(10)
    X = (rng.standard_normal((n, D)) * 1e-3).astype(np.float32)
    X[777] = 3e7 * (1.0 + rng.random(D).astype(np.float32))
    r64, s64 = O.spmm_f64(X, rp, col)
    meta = _meta(dev, name)
    tX = to_dev(dev, X)[0]
    burst, spread, _, err = _both(T, monkeypatch, capfd, LONG, lambda: T.forward(tX, *meta)[0])
    _long_stream_ran(err)
    got = spread.cpu().numpy()
    assert np.isfinite(got).all()
    assert (np.abs(got - r64) / (s64 + 1.0)).max() <= 2.0 ** -9
    assert torch.equal(burst, spread)
    assert not got[W.zero_rows(name, rp)].any()
