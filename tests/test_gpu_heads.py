"""tcgnn_spmm_heads / TCGNN.forward_heads on the GPU: the multi-head edge-valued SpMM - spmm_heads_kernel where the library's fused
walk covers (heads, F), head by head inside the library elsewhere - against the project's oracle head by head (tests/heads_ref.py),
judged by walks.judge with the project's three bounds unchanged.  Needs an MI355X: `pytest -m gpu`.

Graphs: the smallest shapes at which this kernel can go wrong - edge_case_graphs() (an empty middle window among them), hub rows (runs
of more than four edges inside eight columns: the second value DMA), E = 1 and 4 <= E < 8 (the CSR way; the clamped value read), the
unsorted-rows entry (a non-canonical plan), short_metadata (windows that are not handed over), and one graph whose windows take four
wavefronts (the fixed-order combine).  (heads, F): heads_ref.SHAPES."""
import glob
import importlib.util
import os

import numpy as np
import pytest
import torch

import gat_ref as G
import graphs
import heads_ref as HR
import test_gpu_memory_contract as MC
import test_gpu_structures as S
import walks as W
from test_gpu_parity import to_dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPHS = {name: (rp, col) for name, rp, col in graphs.edge_case_graphs()}
GRAPHS["hub_rows_n2500"] = graphs.hub_rows_graph(2500, seed=77)
GRAPHS["dense_n3000_deg150"] = graphs.uniform_graph(3000, 150, seed=2)              # four wavefronts per window
GRAPHS["five_edges_n40"] = graphs.csr_from_edges(np.array([0, 3, 3, 17, 39]), np.array([5, 3, 30, 17, 0]), 40)   # 4 <= E < 8
for _n in ("single_edge_corner_n5000", "unsorted_rows_n4100", "short_metadata_n4100"):
    GRAPHS[_n] = S.GRAPHS[_n]
SHAPES = sorted(HR.SHAPES)
FUSED_KERNEL = "spmm_heads_kernel"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def T():
    import TCGNN
    return TCGNN


@pytest.fixture(scope="module")
def ext():
    found = glob.glob(os.path.join(ROOT, "integration", "TCGNN*.so"))
    assert found, "integration/TCGNN*.so is not built"
    spec = importlib.util.spec_from_file_location("TCGNN", found[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_META, _REFS = {}, {}


def _meta(dev, name):
    """the five metadata tensors on the device as the host SGT wrote them (`short_metadata`: blockPartition cut)"""
    if name not in _META:
        rp, col = GRAPHS[name]
        bp, e2c, e2r, _ = graphs.host_sgt(rp, col)
        _META[name] = tuple(to_dev(dev, rp, col, bp[: W.windows_handed_over(name, len(rp) - 1)], e2c, e2r))
    return _META[name]


def _case(name, H, F):
    """(Z, P, forward reference, (transposed reference, rows of A^T without edges)), computed once per (name, H, F) and left unchanged"""
    key = (name, H, F)
    if key not in _REFS:
        if len(_REFS) > 8:
            _REFS.clear()
        rp, col = GRAPHS[name]
        n = len(rp) - 1
        rows = min(W.windows_handed_over(name, n) * 16, n)
        Z, P = HR.heads_data(name, n, len(col), H, F)
        _REFS[key] = (Z, P, HR.heads_reference(rp, col, Z, P, rows), HR.transposed_reference(rp, col, Z, P, rows))
    return _REFS[key]


def _fused_expected(name, H, F):
    """what include/tcgnn.h says of the route: the fused walk for these widths on a canonical plan with E >= 4 (and windows)"""
    return H > 1 and F in (8, 16, 24, 32) and not W.is_unsorted(name) and len(GRAPHS[name][1]) >= 4


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_forward_heads_matches_the_oracle_head_by_head(dev, T, name, shape):
    """forward_heads and forward_heads(transpose=True) inside the project's bounds of the per-head oracle, rows without edges exact
    zeros, the same bits on repetition, the kernel the header promises, one head bit-equal to forward_AGNN"""
    H, F = shape
    rp, col = GRAPHS[name]
    n = len(rp) - 1
    Z, P, ref, (tref, tzero) = _case(name, H, F)
    m = _meta(dev, name)
    tZ, tP = to_dev(dev, Z, P)
    bad = []
    Y = T.forward_heads(tZ, m[0], m[1], tP, *m[2:], H)[0]
    kernel = T.last_kernel(*m)
    assert Y.shape == (n, H * F) and Y.dtype == torch.float32
    bad += W.judge(name, Y.cpu().numpy(), *ref, "forward_heads %dx%d (%s)" % (H, F, kernel), W.zero_rows(name, rp))
    if not torch.equal(T.forward_heads(tZ, m[0], m[1], tP, *m[2:], H)[0], Y):
        bad.append("forward_heads: the second call returns other bits")
    if _fused_expected(name, H, F) and kernel != FUSED_KERNEL:
        bad.append("forward_heads %dx%d ran %r, not %s" % (H, F, kernel, FUSED_KERNEL))
    if H > 1 and not _fused_expected(name, H, F) and kernel == FUSED_KERNEL:
        bad.append("forward_heads %dx%d ran the fused kernel on a shape it does not cover" % (H, F))
    if H == 1 and not torch.equal(Y, T.forward_AGNN(tZ, m[0], m[1], tP, *m[2:])[0]):
        bad.append("one head is not forward_AGNN bit for bit")
    Yt = T.forward_heads(tZ, m[0], m[1], tP, *m[2:], H, transpose=True)[0]
    tz = tzero.copy()
    tz[min(W.windows_handed_over(name, n) * 16, n):] = True
    # (A^T's rows are sorted whatever A's are: the transposed plan of the unsorted entry is canonical and is judged as such)
    bad += W.judge("A^T of " + name if W.is_unsorted(name) else name, Yt.cpu().numpy(), *tref,
                   "forward_heads(transpose) %dx%d (%s)" % (H, F, T.last_kernel(*m, transpose=True)), tz)
    if not torch.equal(T.forward_heads(tZ, m[0], m[1], tP, *m[2:], H, transpose=True)[0], Yt):
        bad.append("forward_heads(transpose): the second call returns other bits")
    if H == 1 and not torch.equal(Yt, T.forward_AGNN(tZ, m[0], m[1], tP, *m[2:], transpose=True)[0]):
        bad.append("one head, transposed, is not forward_AGNN(transpose=True) bit for bit")
    assert not bad, "%s %dx%d:\n  " % (name, H, F) + "\n  ".join(bad)


def test_aggregate_heads_is_one_timed_call_of_the_named_kernel(dev, T):
    import tcgnn_edge_ops as E
    name = "dense_n3000_deg150"
    m = _meta(dev, name)
    for (H, F), want_kernel, want_calls in (((8, 8), FUSED_KERNEL, 1), ((3, 12), "spmm_kernel", 3)):
        Z, P, ref, _ = _case(name, H, F)
        tZ, tP = to_dev(dev, Z, P)
        T.kernel_timing(*m, max_calls=64)
        Y = E.aggregate_heads(tP, tZ, m)
        times = T.kernel_timing(*m)
        T.kernel_timing(*m, max_calls=0)
        print("OBS aggregate_heads %dx%d: %d timed call(s), %s" % (H, F, len(times), T.last_kernel(*m)))
        assert T.last_kernel(*m) == want_kernel and len(times) == want_calls, (H, F, T.last_kernel(*m), len(times))
        assert not W.judge(name, Y.cpu().numpy(), *ref, "aggregate_heads %dx%d" % (H, F), W.zero_rows(name, GRAPHS[name][0]))


def test_fused_heads_and_eight_single_calls_share_the_reference(dev, T):
    """(8, 8) through the fused walk and as eight forward_AGNN calls: both inside the bounds of the same reference - one scale for all of
    Z and of P against one per head, another summation order: not bit-equal, and not expected to be.  The distance is printed."""
    name, (H, F) = "dense_n3000_deg150", (8, 8)
    rp, _ = GRAPHS[name]
    Z, P, ref, _ = _case(name, H, F)
    m = _meta(dev, name)
    tZ, tP = to_dev(dev, Z, P)
    Y = T.forward_heads(tZ, m[0], m[1], tP, *m[2:], H)[0]
    single = torch.cat([T.forward_AGNN(tZ[:, h * F:(h + 1) * F].contiguous(), m[0], m[1], tP[h].view(1, -1), *m[2:])[0] for h in range(H)], 1)
    bad = W.judge(name, Y.cpu().numpy(), *ref, "fused 8x8", W.zero_rows(name, rp)) + W.judge(name, single.cpu().numpy(), *ref, "eight single calls", W.zero_rows(name, rp))
    print("FIG fused 8x8 against eight forward_AGNN calls: %.3e of sum|a||x| + 1" % float((np.abs(Y.cpu().numpy() - single.cpu().numpy()) / (ref[2] + 1.0)).max()))
    assert not bad, "\n".join(bad)


def test_range_guard_takes_the_whole_call(dev, T):
    name, H, F, Z, P = HR.wide_case()
    rp, col = GRAPHS[name]
    m = _meta(dev, name)
    tZ, tP = to_dev(dev, Z, P)
    Y = T.forward_heads(tZ, m[0], m[1], tP, *m[2:], H)[0]
    assert T.range_mode()[1] == 1 and T.last_kernel(*m) == FUSED_KERNEL          # wide: the fp32 way behind the kernel did the work
    bad = W.judge(name, Y.cpu().numpy(), *HR.heads_reference(rp, col, Z, P), "forward_heads, one head x 2^24 (fp32 way)", W.zero_rows(name, rp))
    # a head of all zeros: exact zeros in its columns, on the MFMA path
    Z, P, _, _ = _case(name, H, F)
    P = P.copy()
    P[1] = 0
    tZ, tP = to_dev(dev, Z, P)
    Y = T.forward_heads(tZ, m[0], m[1], tP, *m[2:], H)[0]
    assert T.range_mode()[1] == 0
    bad += W.judge(name, Y.cpu().numpy(), *HR.heads_reference(rp, col, Z, P), "forward_heads, one head of zeros", W.zero_rows(name, rp))
    if bool((Y[:, F:2 * F] != 0).any()):
        bad.append("the columns of the all-zero head are not exact zeros")
    assert not bad, "\n".join(bad)


CONTRACT = [(name, shape) for name in ("uniform_n40", "range_boundary_columns_n4585") for shape in ((3, 8), (9, 16))]


@pytest.mark.parametrize("name,shape", CONTRACT, ids=["%s-%dx%d" % (n, *s) for n, s in CONTRACT])
def test_heads_call_keeps_the_memory_contract(dev, T, monkeypatch, name, shape):
    """Through ctypes with guarded buffers (test_gpu_memory_contract.Case): Y between moats, pre-filled with NaN; a workspace of exactly
    tcgnn_spmm_heads_workspace_bytes between moats, one byte less refused with nothing written; X and the edge values between NaN moats,
    unchanged, and one float late the same bits; Y one float late, bad H or F, a null array: refused, everything untouched."""
    H, F = shape
    cs = MC.Case(dev, T, monkeypatch, name, H * F)
    lib, n = cs.lib, cs.n
    Z, P = HR.heads_data(name, n, cs.nnz, H, F)
    ref = HR.heads_reference(cs.rp, cs.col, Z, P)
    tZ, tP = to_dev(dev, Z, P)
    plan = cs.plan()
    try:
        need = int(lib.tcgnn_spmm_heads_workspace_bytes(plan, H, F))
        assert need > 0
        what = "tcgnn_spmm_heads %dx%d" % (H, F)
        call = lambda h, f, null=(): (lambda p, ws, nb: (plan, None if "X" in null else p["X"], None if "val" in null else p["val"],   # noqa: E731
                                                         None if "Y" in null else p["Y"], h, f, ws, nb, cs.stream))
        outs, ins = {"Y": ((n, H * F), MC.F32)}, {"X": Z, "val": P}
        out = cs.call(what, lib.tcgnn_spmm_heads, call(H, F), outs, ins, need)
        kernel = cs.kernel(plan)
        if out is not None:
            Y = out["Y"]
            what += " (%s)" % kernel
            if kernel != FUSED_KERNEL:
                cs.fail.append("%s: not the fused kernel" % what)
            if cs.written(what, "Y", Y):
                cs.judge(what, Y, ref, cs.zero)
            cs.same(what, Y, T.forward_heads(tZ, cs.meta[0], cs.meta[1], tP, *cs.meta[2:], H)[0])
            for late in (("X",), ("val",), ("X", "val")):
                w2 = "%s with %s one float late" % (what, " + ".join(late))
                o = cs.call(w2, lib.tcgnn_spmm_heads, call(H, F), outs, ins, need, offsets=late)
                cs.same(w2, o and o["Y"], Y, "the aligned call")
            cs.call(what + " with Y one float late", lib.tcgnn_spmm_heads, call(H, F), outs, ins, need, offsets=("Y",), expect=MC.INVALID_ARG)
            for h, f in ((0, F), (H, 0), (-1, F)):
                cs.call("%s with H = %d, F = %d" % (what, h, f), lib.tcgnn_spmm_heads, call(h, f), outs, ins, need, expect=MC.INVALID_ARG)
            for null in ("X", "val", "Y"):
                cs.call("%s with %s null" % (what, null), lib.tcgnn_spmm_heads, call(H, F, (null,)), outs, ins, need, expect=MC.INVALID_ARG)
    finally:
        cs.destroy(plan)
    cs.end_of_walk("tcgnn_spmm_heads")
    MC._finish(cs, "%s %dx%d tcgnn_spmm_heads" % (name, H, F))
    T.clear_plan_cache()


def test_binding_forward_heads_equals_the_ctypes_module(dev, T, ext):
    rp, col = graphs.powerlaw_graph(3000, 12, seed=31, symmetric=False)
    n, E = len(rp) - 1, len(col)
    bp, e2c, e2r, _ = graphs.host_sgt(rp, col)
    m = to_dev(dev, rp, col, bp, e2c, e2r)
    g = torch.Generator(device=dev).manual_seed(6)
    for H, F in ((8, 8), (5, 24), (3, 12), (1, 16)):
        X, P = torch.randn(n, H * F, device=dev, generator=g), torch.randn(H, E, device=dev, generator=g)
        for transpose in (False, True):
            want = T.forward_heads(X, m[0], m[1], P, *m[2:], H, transpose=transpose)[0]
            got = ext.forward_heads(X, m[0], m[1], P, *m[2:], H, transpose=transpose)[0]
            assert torch.equal(got, want), (H, F, transpose)
    with pytest.raises(RuntimeError, match="heads"):
        ext.forward_heads(X, m[0], m[1], P, *m[2:], 3)
    with pytest.raises(RuntimeError, match="heads"):
        T.forward_heads(X, m[0], m[1], P, *m[2:], 3)
    with pytest.raises(RuntimeError, match="edgeAttention must be"):
        T.forward_heads(X, m[0], m[1], P[:, :-1].contiguous(), *m[2:], 1)
    with pytest.raises(RuntimeError, match="edgeAttention must be"):
        ext.forward_heads(X, m[0], m[1], P[:, :-1].contiguous(), *m[2:], 1)
    torch.cuda.synchronize()
    ext.clear_plan_cache()
    T.clear_plan_cache()


@pytest.mark.parametrize("shape", [(8, 8), (5, 24)], ids=["8x8", "5x24"])
@pytest.mark.parametrize("name", ["layers_n200", "directed_n3000"])
def test_aggregate_heads_gradients_against_dense_fp64(dev, T, name, shape):
    """values, dP and dZ of aggregate_heads against the dense fp64 products head by head (gat_ref.dense_adjacency's matrix), at the
    constant the layer test uses (gat_ref.GPU_LAYER_TOL of the largest entry); directed_n3000 is not symmetric"""
    import tcgnn_edge_ops as E
    H, F = shape
    rp, col = G.golden_graph() if name == "layers_n200" else graphs.powerlaw_graph(3000, 12, seed=31, symmetric=False)
    if name == "directed_n3000":
        assert not W.is_symmetric(rp, col)
    n, nnz = len(rp) - 1, len(col)
    bp, e2c, e2r, _ = graphs.host_sgt(rp, col)
    meta = to_dev(dev, rp, col, bp, e2c, e2r)
    rows, cols = torch.from_numpy(np.repeat(np.arange(n), np.diff(rp))).long(), torch.from_numpy(col).long()
    g = torch.Generator().manual_seed(100 * H + F)
    Pv, Z, dY = (torch.randn(*s, dtype=torch.float64, generator=g) for s in ((H, nnz), (n, H * F), (n, H * F)))
    pg, zg = (t.float().to(dev).requires_grad_(True) for t in (Pv, Z))
    pd, zd = (t.clone().requires_grad_(True) for t in (Pv, Z))
    Y = E.aggregate_heads(pg, zg, meta)
    assert T.last_kernel(*meta) == FUSED_KERNEL
    want = torch.cat([torch.zeros(n, n, dtype=torch.float64).index_put((rows, cols), pd[h]) @ zd[:, h * F:(h + 1) * F] for h in range(H)], 1)
    got = torch.autograd.grad((Y * dY.float().to(dev)).sum(), (pg, zg))
    assert T.last_kernel(*meta, transpose=True) == FUSED_KERNEL
    ref = torch.autograd.grad((want * dY).sum(), (pd, zd))
    for a, b, what in ((Y, want, "Y"), (got[0], ref[0], "dP"), (got[1], ref[1], "dZ")):
        a, b = a.detach().double().cpu(), b.detach()
        err, top = float((a - b).abs().max()), float(b.abs().max())
        print("FIG %s %dx%d aggregate_heads %-2s %.3e of the largest entry" % (name, H, F, what, err / top))
        assert a.shape == b.shape and err <= G.GPU_LAYER_TOL * top, (what, err / top)
    T.clear_plan_cache()
