"""tcgnn_sddmm_heads / TCGNN.forward_ef_heads on the GPU: the multi-head SDDMM - sddmm_kernel's multi-head form ("sddmm_heads_kernel")
where the library's fused walk covers (heads, F), head by head inside the library elsewhere - against the per-head reference of
tests/sddmm_heads_ref.py, judged by test_gpu_parity.assert_parity with the project's three bounds unchanged; then sddmm_heads,
edge_softmax_heads, aggregate_heads' dP and TransformerConv against a dense fp64 model.  Needs an MI355X: `pytest -m gpu`."""
import ctypes
import glob
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import gat_ref as G
import graphs
import sddmm_heads_ref as HR
import test_gpu_memory_contract as MC
import test_gpu_structures as S
import walks as W
from test_gpu_parity import assert_parity, to_dev
from test_sddmm_heads_cpu import dense_transformer_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPHS = HR.gpu_graphs()
SHAPES = sorted(HR.SHAPES)
FUSED = "sddmm_heads_kernel"


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


_META = {}


def _meta(dev, name):
    """the five metadata tensors on the device as the host SGT wrote them (`short_metadata`: blockPartition cut)"""
    if name not in _META:
        rp, col = GRAPHS[name]
        bp, e2c, e2r, _ = graphs.host_sgt(rp, col)
        _META[name] = tuple(to_dev(dev, rp, col, bp[: W.windows_handed_over(name, len(rp) - 1)], e2c, e2r))
    return _META[name]


def _judge(name, got, refs, what, bad, bar=True):
    """the three bounds, on every graph - the non-canonical entry too (test_gpu_edge_ops._judge)"""
    ref, r64, s64 = refs
    if not np.isfinite(got).all():
        bad.append("%s: non-finite scores" % what)
        return
    fig = (float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()), float((np.abs(got - ref) / (s64 + 1.0)).max()),
           float((np.abs(got - r64) / (s64 + 1.0)).max())) if got.size else (0.0, 0.0, 0.0)
    print("FIG %-64s bar %.2e tight %.2e fp64 %.2e (shares %.2f %.2f %.2f)" % (what, *fig, fig[0] / W.TOL, fig[1] / W.TIGHT, fig[2] / W.LOOSE))
    try:
        assert_parity(got, ref, r64, s64, what, unit_scale=bar)
    except AssertionError as e:
        bad.append(str(e) or "%s: beyond 2^-9 of the fp64 contract (%.3e)" % (what, fig[2]))


def _fused_expected(name, rp, col, H, F):
    n = len(rp) - 1
    return HR.fused_expected(H, F, not W.is_unsorted(name), len(col), W.windows_handed_over(name, n))


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_forward_ef_heads_matches_the_reference_head_by_head(dev, T, ext, name, shape):
    """inside the three bounds of the per-head reference, finite, zero behind a short blockPartition, the same bits from a second call
    and from the pybind module, the fused kernel exactly where the header promises it, one head bit-equal to forward_ef2"""
    H, F = shape
    rp, col = GRAPHS[name]
    n, nnz = len(rp) - 1, len(col)
    X, Z = HR.heads_data(name, n, H, F)
    rows = HR.rows_handed_over(name, n)
    ref = HR.heads_reference(rp, col, X, Z, H, rows)
    m = _meta(dev, name)
    tX, tZ = to_dev(dev, X, Z)
    bad = []
    ef = T.forward_ef_heads(tX, tZ, *m, H)[0]
    kernel = T.last_kernel(*m)
    assert ef.shape == (H, nnz) and ef.dtype == torch.float32
    _judge(name, ef.cpu().numpy().astype(np.float64), ref, "forward_ef_heads %s %dx%d (%s)" % (name, H, F, kernel), bad)
    if bool((ef[:, int(rp[rows]):] != 0).any()):
        bad.append("scores of the windows that were not handed over are not zero")
    if not torch.equal(T.forward_ef_heads(tX, tZ, *m, H)[0], ef):
        bad.append("the second call returns other bits")
    if not torch.equal(ext.forward_ef_heads(tX, tZ, *m, H)[0], ef):
        bad.append("the pybind module differs in bits from the ctypes one")
    fused = _fused_expected(name, rp, col, H, F)
    if fused and kernel != FUSED:
        bad.append("ran %r, not %s" % (kernel, FUSED))
    if not fused and kernel.startswith(FUSED):
        bad.append("ran the fused kernel on a shape or plan it does not cover")
    if H > 1 and F > 128 and not W.is_unsorted(name) and nnz >= 4 and kernel != "sddmm_wide_kernel":
        bad.append("heads of %d columns ran %r, not sddmm_wide_kernel" % (F, kernel))
    if H == 1 and not torch.equal(ef[0], T.forward_ef2(tX, tZ, *m)[0]):
        bad.append("one head is not forward_ef2 bit for bit")
    ext.clear_plan_cache()
    assert not bad, "%s %dx%d:\n  " % (name, H, F) + "\n  ".join(bad)


# ---- every SDDMM walk, on the catalogue of boundary-shaped graphs --------------------------------------------------------------------------

WALK_SHAPES = ((8, 8), (4, 32))
WALK_CASES = [(name, shape) for name in S.GRAPHS for shape in WALK_SHAPES]


def _kernel_ran(walk, name, D, kernel, pred, fused, failures):
    """test_gpu_edge_ops._kernel_ran for forward_ef_heads, under test_gpu_structures' exception table (the entries of forward_ef): the
    fused kernel reports the single-head kernel's name with `sddmm_heads_kernel` in place of `sddmm_kernel`"""
    if not fused:          # (a non-canonical plan, fewer than four edges: the CSR launch, whatever is forced)
        if kernel.startswith(FUSED):
            failures.append("forward_ef_heads/%s: the fused kernel ran on a plan it does not cover" % walk)
        return
    if not kernel.startswith(FUSED):
        failures.append("forward_ef_heads/%s: last_kernel is %r, not the fused kernel" % (walk, kernel))
        return
    ran = bool(pred(kernel.replace(FUSED, "sddmm_kernel", 1), D))
    if ("forward_ef", walk) in S.SAME_NAME:
        n = len(S.GRAPHS[name][0]) - 1
        nr = W.expected_ranges(n, D, S._CTX["buckets"], W.range_kb_for_eight(n, D))
        ran = ran and S._CTX["buckets"] > 0 and nr >= 8 and nr % 8 == 0
    print("OBS forward_ef_heads | %s | %s | D=%d | %s | %s" % (walk, name, D, kernel, "ran" if ran else "OTHER"))
    why = S.EXCEPTIONS.get(("forward_ef", walk, name))
    if why is None and not ran:
        failures.append("forward_ef_heads/%s: last_kernel is %r, not the forced kernel, and EXCEPTIONS has no entry for the pair" % (walk, kernel))
    if why is not None and ran:
        failures.append("forward_ef_heads/%s: EXCEPTIONS says %r, but the forced kernel ran (%r)" % (walk, why, kernel))


@pytest.mark.parametrize("name,shape", WALK_CASES, ids=["%s-%dx%d" % (n, *s) for n, s in WALK_CASES])
def test_forward_ef_heads_on_every_sddmm_walk(dev, T, monkeypatch, capfd, name, shape):
    """walks.SDDMM_WALKS forced as tests/test_gpu_edge_ops.py forces them: inside the bounds, bit-equal across walks and on repetition,
    the forced kernel.  (The entries at the staging cap - windows of full tiles, 65 520 / 65 536 edges in one window - are where a
    per-head flush could lose or repeat a run.)"""
    H, F = shape
    D = H * F
    rp, col = S.GRAPHS[name]
    n, nnz = len(rp) - 1, len(col)
    meta = S._meta(dev, name)
    info = T.plan_info(*meta)
    S._CTX.update(capfd=capfd, n=n, D=D, buckets=info["column_buckets"])
    X, Z = HR.heads_data(name, n, H, F)
    ref = HR.heads_reference(rp, col, X, Z, H, HR.rows_handed_over(name, n))
    fused = _fused_expected(name, rp, col, H, F)
    tX, tZ = to_dev(dev, X, Z)
    failures, first = [], None
    for walk in S._walks_for(name, "forward_ef"):
        mode, env, pred = W.SDDMM_WALKS[walk]

        def body():
            ef = T.forward_ef_heads(tX, tZ, *meta, H)[0]
            return dict(ef=ef, kernel=T.last_kernel(*meta), again=T.forward_ef_heads(tX, tZ, *meta, H)[0])
        try:
            o = S._forced(T, monkeypatch, mode, env, body)
        except RuntimeError as e:
            failures.append("forward_ef_heads %s: %s" % (walk, e))
            continue
        bad = []
        _judge(name, o["ef"].cpu().numpy().astype(np.float64), ref, "forward_ef_heads %s %s %dx%d (%s)" % (name, walk, H, F, o["kernel"]), bad)
        if not torch.equal(o["ef"], o["again"]):
            bad.append("forward_ef_heads %s: the second call returns other bits" % walk)
        if first is None:
            first = o["ef"]
        elif not torch.equal(o["ef"], first):
            bad.append("forward_ef_heads %s: scores differ in bits from the automatic walk's" % walk)
        _kernel_ran(walk, name, D, o["kernel"], pred, fused, bad)
        failures += bad
    T.clear_plan_cache()
    sys.stdout.write(capfd.readouterr().out)
    assert not failures, "%s %dx%d:\n  " % (name, H, F) + "\n  ".join(failures)


# ---- head isolation: what catches a wrong lane mask ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(3, 8), (8, 8), (4, 16), (4, 32), (2, 64)], ids=lambda s: "%dx%d" % s)
def test_a_head_touches_its_own_row_of_scores_only(dev, T, shape):
    """head h of Z x 2^-10 scales ef[h] by exactly 2^-10 and leaves every other head's bits (h: not the head that holds max|Z|, so the
    one scale of Z stays; the head's elements are kept at 2^-12 or more so that none leaves fp16's normal range); a head of zeros in X
    gives exact zeros in its row and nothing else"""
    H, F = shape
    name = "hub_rows_n2500"
    rp, col = GRAPHS[name]
    n = len(rp) - 1
    m = _meta(dev, name)
    X, Z = HR.heads_data(name, n, H, F)
    top = int(np.argmax(np.abs(Z).max(0))) // F
    h = (top + 1) % H
    cols = slice(h * F, (h + 1) * F)
    Z[:, cols] = np.where(np.abs(Z[:, cols]) < 2.0 ** -12, np.float32(2.0 ** -12), Z[:, cols])
    Zs = Z.copy()
    Zs[:, cols] *= np.float32(2.0 ** -10)
    X0 = X.copy()
    X0[:, cols] = 0
    tX, tZ, tZs, tX0 = to_dev(dev, X, Z, Zs, X0)
    ef = T.forward_ef_heads(tX, tZ, *m, H)[0]
    assert T.last_kernel(*m) == FUSED
    scaled = T.forward_ef_heads(tX, tZs, *m, H)[0]
    zeroed = T.forward_ef_heads(tX0, tZ, *m, H)[0]
    others = [k for k in range(H) if k != h]
    assert torch.equal(scaled[h], ef[h] * 2.0 ** -10), "head %d of Z x 2^-10 does not scale its scores by exactly 2^-10" % h
    assert torch.equal(scaled[others], ef[others]), "scaling head %d of Z moved another head's scores" % h
    assert not bool((zeroed[h] != 0).any()), "a head of zeros in X does not give exact zeros"
    assert torch.equal(zeroed[others], ef[others]), "zeroing head %d of X moved another head's scores" % h
    assert bool((ef[h] != 0).any())


# ---- the range guard at its default level (2) ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", HR.WIDE_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("which", ["X", "Z"])
def test_range_guard_takes_the_whole_call(dev, T, which, shape):
    """one row of X, then of Z, x 2^30 at (4, 8) - fused - and at (3, 12) - head by head: the operand's header says wide
    (tcgnn_range_mode on the header the operand was staged under: Z's at the workspace's start, X's behind it) and the ONE fp32
    launch behind the MFMA kernels did the work"""
    import tcgnn_capi as c
    name, (H, F) = HR.WIDE[0], shape
    rp, col, X, Z, ref = HR.wide_case(which, shape)
    m = _meta(dev, name)
    tX, tZ = to_dev(dev, X, Z)
    ef = T.forward_ef_heads(tX, tZ, *m, H)[0]
    assert T.last_kernel(*m) == (FUSED if F == 8 else "sddmm_kernel")
    plan = T._plan_of(m)
    need = int(c.lib.tcgnn_sddmm_heads_workspace_bytes(plan, H, F))
    ws = T._buffer("workspace", None, dev)[0] + (need // 2 if which == "X" else 0)
    a, b = c._i32(0), c._i32(0)
    c.check(c.lib.tcgnn_range_mode(ws, torch.cuda.current_stream(dev).cuda_stream, ctypes.byref(a), ctypes.byref(b)), "tcgnn_range_mode")
    assert a.value != 0, "the header of %s does not say wide" % which
    bad = []
    _judge(name, ef.cpu().numpy().astype(np.float64), ref, "forward_ef_heads %dx%d range guard, a row of %s x 2^30" % (H, F, which), bad, bar=False)
    assert not bad, "\n".join(bad)
    T.clear_plan_cache()


# ---- the memory contract, through ctypes with guarded buffers ------------------------------------------------------------------------------

CONTRACT = [(name, shape) for name in ("uniform_n40", "range_boundary_columns_n4585") for shape in ((3, 8), (4, 32))]


@pytest.mark.parametrize("name,shape", CONTRACT, ids=["%s-%dx%d" % (n, *s) for n, s in CONTRACT])
def test_sddmm_heads_call_keeps_the_memory_contract(dev, T, monkeypatch, name, shape):
    """ef between moats, pre-filled with NaN, fully written; a workspace of exactly tcgnn_sddmm_heads_workspace_bytes between moats, one
    byte less refused with nothing written; X and Z between NaN moats, unchanged, and one float late - ef too - the same bits; bad H
    or F, a null array: refused, everything untouched"""
    H, F = shape
    cs = MC.Case(dev, T, monkeypatch, name, H * F)
    lib, n = cs.lib, cs.n
    X, Z = HR.heads_data(name, n, H, F)
    ref = HR.heads_reference(cs.rp, cs.col, X, Z, H)
    tX, tZ = to_dev(dev, X, Z)
    plan = cs.plan()
    try:
        need = int(lib.tcgnn_sddmm_heads_workspace_bytes(plan, H, F))
        assert need > 0
        what = "tcgnn_sddmm_heads %dx%d" % (H, F)
        call = lambda h, f, null=(): (lambda p, ws, nb: (plan, None if "X" in null else p["X"], None if "Z" in null else p["Z"],   # noqa: E731
                                                         None if "ef" in null else p["ef"], h, f, ws, nb, cs.stream))
        outs, ins = {"ef": ((H, cs.nnz), MC.F32)}, {"X": X, "Z": Z}
        out = cs.call(what, lib.tcgnn_sddmm_heads, call(H, F), outs, ins, need)
        kernel = cs.kernel(plan)
        if out is not None:
            ef = out["ef"]
            what += " (%s)" % kernel
            if kernel != FUSED:
                cs.fail.append("%s: not the fused kernel" % what)
            if cs.written(what, "ef", ef):
                _judge(name, ef.cpu().numpy().astype(np.float64), ref, what, cs.fail)
            cs.same(what, ef, T.forward_ef_heads(tX, tZ, *cs.meta, H)[0])
            for late in (("X",), ("Z",), ("ef",), ("X", "Z", "ef")):
                w2 = "%s with %s one float late" % (what, " + ".join(late))
                o = cs.call(w2, lib.tcgnn_sddmm_heads, call(H, F), outs, ins, need, offsets=late)
                cs.same(w2, o and o["ef"], ef, "the aligned call")
            for h, f in ((0, F), (H, 0), (-1, F)):
                cs.call("%s with H = %d, F = %d" % (what, h, f), lib.tcgnn_sddmm_heads, call(h, f), outs, ins, need, expect=MC.INVALID_ARG)
            for null in ("X", "Z", "ef"):
                cs.call("%s with %s null" % (what, null), lib.tcgnn_sddmm_heads, call(H, F, (null,)), outs, ins, need, expect=MC.INVALID_ARG)
    finally:
        cs.destroy(plan)
    cs.end_of_walk("tcgnn_sddmm_heads")
    MC._finish(cs, "%s %dx%d tcgnn_sddmm_heads" % (name, H, F))
    T.clear_plan_cache()


# ---- the differentiable operators and the layer against dense fp64 -------------------------------------------------------------------------

def _directed500():
    rp, col = graphs.powerlaw_graph(500, 8, seed=41, symmetric=False)
    assert not W.is_symmetric(rp, col)
    return rp, col


def _dev_meta(dev, rp, col):
    bp, e2c, e2r, _ = graphs.host_sgt(rp, col)
    return tuple(to_dev(dev, rp, col, bp, e2c, e2r))


def _close(got, want, what):
    got, want = got.detach().double().cpu(), want.detach()
    err, top = float((got - want).abs().max()), float(want.abs().max())
    print("FIG %-44s %.3e of the largest entry" % (what, err / max(top, 1e-300)))
    assert got.shape == want.shape and err <= G.GPU_LAYER_TOL * top, "%s: %.3e of the largest entry" % (what, err / max(top, 1e-300))


def test_sddmm_heads_and_edge_softmax_heads_against_dense_fp64(dev, T):
    import tcgnn_edge_ops as E
    rp, col = _directed500()
    n, nnz = len(rp) - 1, len(col)
    meta = _dev_meta(dev, rp, col)
    A = G.dense_adjacency(rp, col)
    rows, cols = torch.from_numpy(np.repeat(np.arange(n), np.diff(rp))).long(), torch.from_numpy(col).long()
    H, F = 3, 8
    g = torch.Generator().manual_seed(5)
    Xd, Zd = (torch.randn(n, H * F, dtype=torch.float64, generator=g).requires_grad_(True) for _ in range(2))
    w = torch.randn(H, nnz, dtype=torch.float64, generator=g)
    Xg, Zg = (t.detach().float().to(dev).requires_grad_(True) for t in (Xd, Zd))
    beta = torch.tensor([F ** -0.5], device=dev)
    Sg = E.sddmm_heads(Xg, Zg, meta, H)
    assert T.last_kernel(*meta) == FUSED
    Pg = E.edge_softmax_heads(Sg, meta[0], beta)
    got = torch.autograd.grad((Pg * w.float().to(dev)).sum(), (Xg, Zg))
    Sd, Pd = [], []
    for h in range(H):
        c = slice(h * F, (h + 1) * F)
        full = Xd[:, c] @ Zd[:, c].t()
        Sd.append(full[rows, cols])
        soft = torch.softmax((full * F ** -0.5).masked_fill(A == 0, float("-inf")).masked_fill(A.sum(1, keepdim=True) == 0, 0.0), dim=1)
        Pd.append(soft[rows, cols])
    Sd, Pd = torch.stack(Sd), torch.stack(Pd)
    want = torch.autograd.grad((Pd * w).sum(), (Xd, Zd))
    _close(Sg, Sd, "sddmm_heads 3x8")
    _close(Pg, Pd, "edge_softmax_heads 3x8")
    _close(got[0], want[0], "sddmm_heads 3x8 dX")
    _close(got[1], want[1], "sddmm_heads 3x8 dZ")
    T.clear_plan_cache()


@pytest.mark.parametrize("root_weight", [True, False], ids=["root", "noroot"])
@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
def test_transformer_layer_against_the_dense_fp64_model(dev, T, concat, root_weight):
    import tcgnn_layers as L
    rp, col = _directed500()
    n = len(rp) - 1
    meta = _dev_meta(dev, rp, col)
    A = G.dense_adjacency(rp, col)
    H, F, inp = 3, 8, 24
    torch.manual_seed(7)
    layer = L.TransformerConv(inp, F, heads=H, concat=concat, root_weight=root_weight)
    for b in (layer.bias_q, layer.bias_k, layer.bias_v, layer.bias):
        b.data.normal_(std=0.1)
    X = torch.randn(n, inp)
    dY = torch.randn(n, H * F if concat else F, dtype=torch.float64)
    import copy
    dense = copy.deepcopy(layer).double()
    Xd = X.double().requires_grad_(True)
    want = dense_transformer_model(A, Xd, dense, H)
    ref = torch.autograd.grad((want * dY).sum(), [Xd] + list(dense.parameters()))
    layer = layer.to(dev)
    Xg = X.to(dev).requires_grad_(True)
    Y = layer(Xg, *meta)
    got = torch.autograd.grad((Y * dY.float().to(dev)).sum(), [Xg] + list(layer.parameters()))
    _close(Y, want, "TransformerConv Y")
    # (d bias_k is zero in exact arithmetic - the softmax drops a shift of every key - and is judged on the scale of d bias_q)
    names = ["X"] + [k for k, _ in layer.named_parameters()]
    scale = dict(zip(names, ref))
    for g_, r_, k in zip(got, ref, names):
        if k == "bias_k":
            err = float((g_.detach().double().cpu() - r_).abs().max())
            print("FIG TransformerConv dbias_k %.3e of the largest entry of dbias_q" % (err / float(scale["bias_q"].abs().max())))
            assert err <= G.GPU_LAYER_TOL * float(scale["bias_q"].abs().max())
        else:
            _close(g_, r_, "TransformerConv d%s" % k)
    T.clear_plan_cache()


@pytest.mark.parametrize("shape", [(8, 8), (5, 24)], ids=["8x8", "5x24"])
def test_aggregate_heads_dP_against_dense_fp64(dev, T, shape):
    import tcgnn_edge_ops as E
    H, F = shape
    rp, col = _directed500()
    n, nnz = len(rp) - 1, len(col)
    meta = _dev_meta(dev, rp, col)
    g = torch.Generator().manual_seed(100 * H + F)
    Pv, Z, dY = (torch.randn(*s, dtype=torch.float64, generator=g) for s in ((H, nnz), (n, H * F), (n, H * F)))
    pg = Pv.float().to(dev).requires_grad_(True)
    Y = E.aggregate_heads(pg, Z.float().to(dev), meta)
    T.kernel_timing(*meta, max_calls=64)
    dP, = torch.autograd.grad((Y * dY.float().to(dev)).sum(), (pg,))
    times = T.kernel_timing(*meta)
    T.kernel_timing(*meta, max_calls=0)
    kernel = T.last_kernel(*meta)
    print("OBS aggregate_heads %dx%d dP: %d timed call(s), %s" % (H, F, len(times), kernel))
    assert (kernel == FUSED and len(times) == 1) if F == 8 else (kernel == "sddmm_kernel" and len(times) == H)
    _close(dP, torch.from_numpy(HR.dense_heads_f64(rp, col, dY.numpy(), Z.numpy(), H)), "aggregate_heads %dx%d dP" % (H, F))
    T.clear_plan_cache()


# ---- a captured step ---------------------------------------------------------------------------------------------------------------------

def test_a_prepared_transformer_step_replays_from_a_hip_graph_bit_equal_and_allocates_nothing(dev, T):
    import tcgnn_layers as L
    rp, col = graphs.community_graph(3000, 10, 20, 0.8, seed=4)
    n = len(rp) - 1
    meta = _dev_meta(dev, rp, col)
    torch.manual_seed(2)
    convs = [L.TransformerConv(32, 8, heads=4).to(dev), L.TransformerConv(32, 6, heads=1).to(dev)]
    params = [p for cv in convs for p in cv.parameters()]
    x = torch.randn(n, 32, device=dev)
    y = torch.randint(0, 6, (n,), device=dev)

    def step():
        for p in params:
            p.grad = None
        loss = torch.nn.functional.cross_entropy(convs[1](torch.relu(convs[0](x, *meta)), *meta), y)
        loss.backward()
        return loss

    T.prepare([8, 6], *meta, transpose=True, edge_valued=True, attention=True, heads=4)
    for _ in range(2):
        step()
        torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == m0
    torch.cuda.set_sync_debug_mode("error")          # a prepared step never synchronises
    try:
        step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                    # (the buffers are per stream: the side stream warms its own, as capture requires)
        for _ in range(3):
            step()
        eager_loss = step().detach().clone()
        eager_grads = [p.grad.clone() for p in params]
        for p in params:
            p.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):   # one stream, no parallel branches
            static_loss = torch.nn.functional.cross_entropy(convs[1](torch.relu(convs[0](x, *meta)), *meta), y)
            static_loss.backward()
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_loss, eager_loss)
    for p, g in zip(params, eager_grads):
        assert p.grad is not None and torch.equal(p.grad, g)
    del graph
    T.clear_plan_cache()
