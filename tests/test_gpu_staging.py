"""The staging pass's choice of converter never shows in the result.  Needs an MI355X: `pytest -m gpu`.

Every hot-path call stages X as a scaled fp16 image first, and which kernel writes that image depends on the width and on where X
lies in memory (tcgnn_stage.inc, launch_convert_rows / launch_convert_planar):

  row-major image (per-window walk)      16-byte loads where D % 4 == 0 and X is 16-byte aligned, scalar loads otherwise
  planar image (LDS-resident walks)      D = 16   the rows kernel (whole aligned float4 rows, no padding columns)
                                         D = 20   a chunk per thread with 16-byte loads
                                         D = 41   the tiled kernel (no float4 in a row; 64 rows of X fit 48 KB of LDS) - a column-scaled
                                                  operand has no tiled kernel: scalar chunks
                                         D = 201  a chunk per thread with scalar loads (201 x 256 B exceeds 48 KB)

Handing X over one float late turns every vector path off.  On two catalogue graphs - uniform_n40 (fewer than 64 rows: one tiled
workgroup, a partial last block everywhere) and range_boundary_columns_n4585 (N % 16 = 9, which the LDS-resident walk accepts) - for
`forward`, the gated fused call and `forward_scaled` with a column scale, on the per-window walk and on lds_flat1 (forced as
tests/walks.py forces them), at the four widths:

  Y of the late call is bit-equal to Y of the aligned call, and TCGNN.range_mode says the same;
  on the per-window walk Y is also bit-equal to tcgnn_spmm_staged on the image tcgnn_stage_absmax + tcgnn_stage_rows build from the
  operand the call rounds (X; X where the gate lets it through; col_scale * X) - from the aligned and from the late copy.

What this pins and what it does not: at D = 16 and 20 the aligned and the late call go through DIFFERENT converters (rows kernel or
vector chunks against scalar chunks / the tiled kernel).  At D = 41 and 201 no row holds a float4, so both calls take the same
converter and only the abs-max pass differs between them (16-byte against scalar loads; scalar for both under a column scale); on the per-window walk the staged image is the
third reference at every width, on the planar walk those two widths pin the abs-max pass alone.

Where last_kernel shows that lds_flat1 was not taken at D = 201 (thirteen planes: three 64-column passes and a one-plane remainder), the
case prints an OBS line and is skipped; at every other width, and on the per-window walk always, another kernel is a failure."""
import ctypes

import numpy as np
import pytest
import torch

import graphs
import walks as W
from test_gpu_parity import to_dev

pytestmark = pytest.mark.gpu

_EDGE = {n: (rp, c) for n, rp, c in graphs.edge_case_graphs()}
_BOUNDARY = {n: (rp, c) for n, rp, c in graphs.boundary_graphs()}
GRAPHS = {"uniform_n40": _EDGE["uniform_n40"], "range_boundary_columns_n4585": _BOUNDARY["range_boundary_columns_n4585"]}
OPS = ("forward", "gated", "scaled")
WALKS = ("per_window", "lds_flat1")
WIDTHS = (16, 20, 41, 201)
CASES = [(name, op, walk, D) for name in GRAPHS for walk in WALKS for D in WIDTHS for op in OPS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def T():
    import TCGNN
    return TCGNN


_META, _DATA = {}, {}


def _meta(dev, name):
    if name not in _META:
        rp, col = GRAPHS[name]
        bp, e2c, e2r, _ = graphs.host_sgt(rp, col)
        _META[name] = tuple(to_dev(dev, rp, col, bp, e2c, e2r))
    return _META[name]


def _late(t):
    """a contiguous copy of t that starts one float behind a 16-byte boundary"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    off = ((-buf.data_ptr()) % 16) // 4 + 1
    out = buf[off: off + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


def _data(dev, name, D):
    """X aligned and one float late, the gate, the column scale and the fp32 operands the gated / scaled calls round - computed once"""
    if (name, D) not in _DATA:
        n = len(GRAPHS[name][0]) - 1
        rng = np.random.default_rng(1000 * D + n)
        X, gate = (rng.standard_normal((n, D)).astype(np.float32) for _ in range(2))
        cs = rng.uniform(0.25, 4.0, n).astype(np.float32)
        tX, tgate, tcs = to_dev(dev, X, gate, cs)
        assert tX.data_ptr() % 16 == 0 and tgate.data_ptr() % 16 == 0
        operand = {"forward": tX, "gated": torch.where(tgate > 0, tX, torch.zeros_like(tX)), "scaled": tcs[:, None] * tX}
        _DATA[(name, D)] = (tX, _late(tX), tgate, tcs, operand)
    return _DATA[(name, D)]


def _staged(c, dev, meta, operand, D):
    """tcgnn_spmm_staged on a plan of its own, from the row-major image tcgnn_stage_absmax + tcgnn_stage_rows build from `operand`"""
    n, nnz = meta[0].numel() - 1, meta[1].numel()
    st = torch.cuda.current_stream(dev).cuda_stream
    pitch = int(c.lib.tcgnn_x16_pitch(D))
    nbytes = 256 + (n + 1) * pitch * 2
    buf = torch.zeros(nbytes + 256, dtype=torch.uint8, device=dev)
    off = (-buf.data_ptr()) % 256
    image = buf[off: off + nbytes]
    c.check(c.lib.tcgnn_stage_absmax(operand.data_ptr(), n * D, image.data_ptr(), st), "tcgnn_stage_absmax")
    c.check(c.lib.tcgnn_stage_rows(operand.data_ptr(), n, D, image.data_ptr(), image.data_ptr() + 256, st), "tcgnn_stage_rows")
    plan = c._vp()
    c.check(c.lib.tcgnn_plan_create(*[t.data_ptr() for t in meta], n, nnz, meta[2].numel(), st, ctypes.byref(plan)), "tcgnn_plan_create")
    try:
        Y = torch.empty(n, D, device=dev)
        c.check(c.lib.tcgnn_spmm_staged(plan, image.data_ptr(), Y.data_ptr(), D, st), "tcgnn_spmm_staged")
        kernel = c.lib.tcgnn_plan_last_kernel(plan).decode()
        torch.cuda.synchronize(dev)
    finally:
        c.lib.tcgnn_plan_destroy(plan)
    return Y, kernel


@pytest.mark.parametrize("name,op,walk,D", CASES, ids=["%s-%s-%s-D%d" % c for c in CASES])
def test_the_choice_of_converter_never_shows_in_the_result(dev, T, monkeypatch, name, op, walk, D):
    import tcgnn_capi as c
    meta = _meta(dev, name)
    tX, tX_late, tgate, tcs, operand = _data(dev, name, D)
    mode, env, pred = W.FORWARD_WALKS[walk]

    def call(x):
        if op == "forward":
            Y = T.forward(x, *meta)[0]
        elif op == "gated":
            Y = T.forward_fused(x, *meta, gate=tgate)[0]
        else:
            Y = T.forward_scaled(x, *meta, col_scale=tcs)[0]
        return Y, T.last_kernel(*meta), T.range_mode(dev)

    def body():
        out = [call(tX), call(tX_late)]
        if walk == "per_window":
            out += [_staged(c, dev, meta, operand[op], D), _staged(c, dev, meta, _late(operand[op]), D)]
        return out

    n = len(GRAPHS[name][0]) - 1
    out = W.forced(T, monkeypatch, mode, env, body, {"n": n, "D": D, "capfd": None})
    (Y, kernel, rm), (Y_late, kernel_late, rm_late) = out[:2]
    print("OBS %s | %s | %s | D=%d | %s | %s | range_mode %s %s" % (op, walk, name, D, kernel, kernel_late, rm, rm_late))
    if not (pred(kernel) and pred(kernel_late)):
        assert walk == "lds_flat1" and D == 201, "last_kernel is %r / %r: the forced walk was not taken" % (kernel, kernel_late)
        print("OBS %s | %s | %s | D=%d: the forced walk was not taken (%r)" % (op, walk, name, D, kernel))
        pytest.skip("last_kernel is %r: the forced walk was not taken at this width" % kernel)
    assert torch.isfinite(Y).all()
    assert torch.equal(Y, Y_late), "X one float late changes Y: %d elements differ" % int((Y != Y_late).sum())
    assert rm == rm_late, "range_mode %s with X aligned, %s with X one float late" % (rm, rm_late)
    for (Ys, ks), what in zip(out[2:], ("the aligned operand", "the operand one float late")):
        assert pred(ks), "tcgnn_spmm_staged ran %r" % ks
        assert torch.equal(Y, Ys), "tcgnn_spmm_staged on the image staged from %s differs from the call in %d elements" % (what, int((Y != Ys).sum()))
