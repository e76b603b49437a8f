"""The C ABI's memory contract (include/tcgnn.h "Alignment", "Workspace size", "Y is fully overwritten"): WHERE the plan-based entry
points write and what they read beyond their operands, on every walk, through ctypes with guarded buffers (tests/guarded.py; what the
helper catches is shown on CPU tensors by tests/test_guarded_cpu.py).  Needs an MI355X: `pytest -m gpu`.

The other GPU files judge values through the TCGNN module, whose outputs are torch.empty blocks (rounded up to 512 bytes, recycled -
an element that is not written often still holds the previous, correct answer) and whose workspace is 25 % larger than asked for.
Here every call gets

  outputs      of exactly the contract's size between SENTINEL moats, pre-filled with NaN: finite afterwards = fully overwritten;
  a workspace  of exactly tcgnn_workspace_bytes(plan, D) bytes (tcgnn_sddmm2_workspace_bytes for tcgnn_sddmm2; for the LDS-resident
               edge-valued walk asked after tcgnn_plan_prepare_val), 256-byte aligned and no more, between moats, pre-filled with 0xff
               (NaN as fp16 and fp32: an image column that is read without having been staged shows in the values);
  inputs       between quiet-NaN moats, compared bit for bit with their snapshots afterwards, like the five metadata arrays.

and is judged on: status 0; the output finite everywhere, exact zeros (max(bias, 0) for the scaled call) in rows without edges, inside
the project's bounds against the oracle (walks.judge = what tests/test_gpu_structures.py uses), bit-equal to the same call on the same
walk through the TCGNN module with ordinary torch allocations; every moat intact; every operand unchanged.  Before it, the same call
with a workspace ONE BYTE short must return TCGNN_ERR_WORKSPACE and leave outputs and workspace untouched, bit for bit.

Offset operands (the audit table): every array the header lets start at any 4-byte boundary is handed over one float late -
alone and together with the others - at D = 64, 128 and 100 on one small and one 4 k graph per operator, on the walks that stage X in
each of its layouts; the results are bit-equal to the aligned call's.  The [N, D] outputs, which the header wants 16-byte aligned, are
handed over one float late too: TCGNN_ERR_INVALID_ARG, everything untouched.

Walks are forced as tests/test_gpu_structures.py forces them (walks.forced and the walk tables).  That file judges WHICH kernel ran;
here the kernel's name only has to be the one the module's call reports.  The walks that need a bucket table run on
bucket_boundary_columns_n16500 only (on the 4 k graphs they are the per-window kernel again), the slice-synchronised walk on
communities_hub_row_and_column_n40003 only.

A call that returns TCGNN_ERR_HIP ends the whole session (pytest.exit): after a GPU fault nothing more is started."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import guarded as G
import test_gpu_structures as S
import walks as W
from oracle import oracle as O
from test_gpu_parity import TIGHT, to_dev

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, HIP_ERROR, WORKSPACE, UNSUPPORTED = 0, 1, 2, 5, 6
F32, I32 = torch.float32, torch.int32

EDGE_NAMES = ("uniform_n1", "uniform_n15", "uniform_n16", "uniform_n17", "uniform_n32", "uniform_n40", "empty_middle_window_n48")
BOUNDARY_NAMES = ("range_boundary_columns_n4585", "one_hub_row_last_n4097", "complete_n1030", "single_edge_corner_n5000", "sixteen_full_rows_n4095",
                  "unsorted_rows_n4100", "short_metadata_n4100", "upper_band200_n4100")
BUCKET_NAME, SYNC_NAME = "bucket_boundary_columns_n16500", "communities_hub_row_and_column_n40003"
_EDGE = {n: (rp, c) for n, rp, c in S.graphs.edge_case_graphs()}
GRAPHS = {n: _EDGE[n] for n in EDGE_NAMES}
GRAPHS.update({n: S.GRAPHS[n] for n in BOUNDARY_NAMES + (BUCKET_NAME, SYNC_NAME)})
OPS = ("forward", "epilogues", "forward_AGNN", "forward_ef", "agnn_fused")
WALKS = S.WALKS
# one small and one 4 k graph, the three widths: where operands are handed over one float late
OFFSET_GRAPHS, OFFSET_WIDTHS = ("uniform_n40", "range_boundary_columns_n4585"), (64, 128, 100)
# ... on the walks that stage X row-major, planar, or not at all (the single-launch kernel reads fp32 X)
OFFSET_WALKS = {"forward": ("auto", "per_window", "lds_ordinary", "lds_flat1", "single_launch_fp32"), "epilogues": ("auto", "lds_default"),
                "forward_AGNN": ("auto", "per_window", "lds_val"), "forward_ef": ("auto",), "agnn_fused": ("auto", "sliced0")}


def _widths(name, op):
    if name in (BUCKET_NAME, SYNC_NAME):
        return (41, 64, 128)
    base = (1, 7, 16, 41, 64, 100, 128)
    if op == "forward_ef":
        return base + (160,)                       # sddmm_wide_kernel
    if op == "forward" and name in BOUNDARY_NAMES[:2]:
        return base + (201,)                       # 13 planes: three 64-column passes and a one-plane remainder with D % 4 != 0
    return base


def _walks_for(name, op):
    if op == "epilogues":
        return {SYNC_NAME: ("slice_synchronised",), BUCKET_NAME: ("range_blocked",)}.get(name, ("auto", "lds_default"))
    if name == SYNC_NAME:
        return ("slice_synchronised",)
    needs = [w for w in WALKS[op] if (op, w) in S.NEEDS_BUCKETS]
    if name == BUCKET_NAME:
        return tuple(needs)
    return tuple(w for w in WALKS[op] if w != "slice_synchronised" and w not in needs)


def _walk(op, walk):
    """-> (mode, knobs)"""
    if op == "epilogues":
        return {"auto": (0, {}), "lds_default": (3, {}), "range_blocked": W.FORWARD_WALKS["range_blocked"][:2],
                "slice_synchronised": W.FORWARD_WALKS["slice_synchronised"][:2]}[walk]
    return WALKS[op][walk][:2]


CASES = [(name, D, op) for name in GRAPHS for op in OPS for D in _widths(name, op)]
CASES.sort(key=lambda c: (list(GRAPHS).index(c[0]), c[1]))      # (graph, D) together: the references are cached for one pair at a time


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def T():
    import TCGNN
    return TCGNN


_META, _CACHE = {}, {"key": None}


def _meta(dev, name):
    """(the five metadata tensors on the device as the host SGT wrote them - `short_metadata`: blockPartition cut -, their snapshots)"""
    if name not in _META:
        _META.clear()
        rp, col = GRAPHS[name]
        bp, e2c, e2r, _ = S.graphs.host_sgt(rp, col)
        bp = bp[: W.windows_handed_over(name, len(rp) - 1)]
        meta = tuple(to_dev(dev, rp, col, bp, e2c, e2r))
        _META[name] = (meta, tuple(G.snapshot(t) for t in meta))
    return _META[name]


def _cached(name, D, what, make):
    if _CACHE["key"] != (name, D):
        _CACHE.clear(); _CACHE["key"] = (name, D); W._REFS.clear()
    if what not in _CACHE:
        _CACHE[what] = make()
    return _CACHE[what]


class Case:
    """One (graph, D) under test: its data, its guarded inputs, the list of failures, and the guarded call."""

    def __init__(self, dev, T, monkeypatch, name, D):
        import tcgnn_capi as c
        self.c, self.lib, self.dev, self.T, self.mp, self.name, self.D = c, c.lib, dev, T, monkeypatch, name, D
        self.rp, self.col = GRAPHS[name]
        self.n, self.nnz = len(self.rp) - 1, len(self.col)
        self.meta, self.meta_snap = _meta(dev, name)
        _cached(name, D, "entered", lambda: True)            # (leaves the previous pair's references and tensors behind BEFORE this pair's are made)
        self.rows = min(W.windows_handed_over(name, self.n) * 16, self.n)     # rows inside the windows handed over
        self.zero = W.zero_rows(name, self.rp)
        self.stream = torch.cuda.current_stream(dev).cuda_stream
        self.fail, self.ins = [], {}
        self.ctx = {"n": self.n, "D": D, "capfd": None}
        self.offsets = name in OFFSET_GRAPHS and D in OFFSET_WIDTHS

    # ---- plans
    def plan(self):
        h = self.c._vp()
        m = self.meta
        self.c.check(self.lib.tcgnn_plan_create(*[t.data_ptr() for t in m], self.n, self.nnz, m[2].numel(), self.stream, ctypes.byref(h)), "tcgnn_plan_create")
        return h

    def destroy(self, h):
        torch.cuda.synchronize(self.dev)
        self.lib.tcgnn_plan_destroy(h)

    def kernel(self, h):
        return self.lib.tcgnn_plan_last_kernel(h).decode()

    def forced(self, op, walk, body):
        mode, env = _walk(op, walk)
        try:
            return W.forced(self.T, self.mp, mode, env, body, self.ctx)
        except RuntimeError as e:
            if "HIP" in str(e) or "hip" in str(e):
                pytest.exit("%s %s/%s: %s - a GPU fault: nothing more is run" % (self.name, op, walk, e), returncode=3)
            self.fail.append("%s %s: %s" % (op, walk, e))
            return None

    # ---- guarded buffers
    def inp(self, label, array, offset=0):
        """the guarded input `label` (made once per case and offset): (buf, view, snapshot)"""
        key = (label, offset)
        if key not in self.ins:
            t = torch.as_tensor(array)
            buf, view = G.guarded(self.dev, tuple(t.shape), t.dtype, t, offset_elems=offset)
            self.ins[key] = (buf, view, G.snapshot(view))
        return self.ins[key]

    def status(self, st, what):
        if st == HIP_ERROR:
            pytest.exit("%s D=%d %s: TCGNN_ERR_HIP (%s) - a GPU fault: nothing more is run" % (self.name, self.D, what, self.lib.tcgnn_last_error().decode("utf-8", "replace")),
                        returncode=3)
        return st

    def call(self, what, fn, build, outs, ins, need, offsets=(), expect=OK):
        """One guarded call.  fn: the entry point; build(p, ws, nb) -> its arguments, p[label] = the address of the guarded array `label`;
        outs: {label: (shape, dtype)}; ins: {label: values}; need: the workspace's exact size (None: the call takes none); offsets: the
        labels handed over one element late; expect: the status the call must return - anything but OK: with everything left untouched.
        -> {label: view} of the outputs, None unless the call returned OK."""
        dev = self.dev
        ob = {l: G.guarded(dev, shp, dt, "output", offset_elems=1 if l in offsets else 0) for l, (shp, dt) in outs.items()}
        ib = {l: self.inp(l, a, 1 if l in offsets else 0) for l, a in ins.items()}
        wsb, ws = G.exact_workspace(dev, need or 0)
        p = {l: G.address(b) for l, (b, _) in ob.items()}
        p.update({l: G.address(b) for l, (b, _, _) in ib.items()})
        wsp = G.address(wsb) if need is not None else None

        def untouched():
            return [l for l, (b, v) in ob.items() if not G.pristine(b, v)] + ([] if G.pristine(wsb, ws) else ["the workspace"])
        if need and expect == OK:
            st = self.status(fn(*build(p, wsp, need - 1)), what)
            if st != WORKSPACE:
                self.fail.append("%s with a workspace one byte short of %d: status %d, not TCGNN_ERR_WORKSPACE" % (what, need, st))
            elif untouched():
                self.fail.append("%s, refused for its workspace one byte short, had already written %s" % (what, ", ".join(untouched())))
            if st == OK:      # (the call ran: fresh outputs for the judged one)
                ob = {l: G.guarded(dev, shp, dt, "output", offset_elems=1 if l in offsets else 0) for l, (shp, dt) in outs.items()}
                p.update({l: G.address(b) for l, (b, _) in ob.items()})
        st = self.status(fn(*build(p, wsp, need or 0)), what)
        if st != expect:
            self.fail.append("%s: status %d (%s), expected %d" % (what, st, self.lib.tcgnn_last_error().decode("utf-8", "replace") if st else "ok", expect))
            return None
        if expect != OK:
            if untouched():
                self.fail.append("%s, refused with status %d, had already written %s" % (what, st, ", ".join(untouched())))
            return None
        for l, (b, v) in list(ob.items()) + [("the workspace", (wsb, ws))]:
            bad = G.moat_intact(b, v)
            if bad:
                self.fail.append("%s: %d moat elements of %s changed, at offsets %s .. (array of %d)" % (what, len(bad), l, bad[:4], v.numel()))
        for l, (b, v, snap) in ib.items():
            if not G.unchanged(v, snap):
                self.fail.append("%s: the operand %s was written" % (what, l))
        return {l: v for l, (_, v) in ob.items()}

    def written(self, what, label, view):
        k = G.unwritten(view)
        if k:
            self.fail.append("%s: %d of %d elements of %s were not written" % (what, k, view.numel(), label))
        return k == 0

    def same(self, what, got, want, against="the TCGNN module's call with torch allocations"):
        if got is None or want is None:
            return
        if got.shape != want.shape or not G.unchanged(got, want.to(got.dtype) if want.dtype != got.dtype else want):
            diff = int((got.reshape(-1).view(I32) != want.reshape(-1).view(I32)).sum()) if got.shape == want.shape else -1
            self.fail.append("%s: %d elements differ in bits from %s" % (what, diff, against))

    def end_of_walk(self, what):
        for t, snap, l in zip(self.meta, self.meta_snap, ("nodePointer", "edgeList", "blockPartition", "edgeToColumn", "edgeToRow")):
            if not G.unchanged(t, snap):
                self.fail.append("%s: the metadata array %s was written" % (what, l))

    def end_of_case(self):
        for (l, off), (b, v, snap) in self.ins.items():
            bad = G.moat_intact(b, v)
            if bad or not G.unchanged(v, snap):
                self.fail.append("the operand %s (offset %d): %d moat elements changed (%s ..), values %s" % (l, off, len(bad), bad[:4], "unchanged" if G.unchanged(v, snap) else "CHANGED"))

    def ws_bytes(self, plan, D=None):
        return int(self.lib.tcgnn_workspace_bytes(plan, self.D if D is None else D))

    def judge(self, what, view, ref, zero=None, zero_value=0.0):
        self.fail += W.judge(self.name, view.cpu().numpy(), *ref, what, zero, zero_value)


def _variants(labels_alone, everything):
    """offset variants: each group alone, then all together"""
    out = [tuple(g) for g in labels_alone]
    if tuple(everything) not in out:
        out.append(tuple(everything))
    return out


# ------------------------------------------------------------------------------------------------------------------ operators

def _run_forward(cs):
    name, D, T, lib = cs.name, cs.D, cs.T, cs.lib
    ref, (X, _), _ = W.references(name, cs.rp, cs.col, D, ops=("spmm",))
    tX = _cached(name, D, "tX", lambda: to_dev(cs.dev, X)[0])
    for walk in _walks_for(name, "forward"):
        def body():
            plan = cs.plan()
            try:
                what = "tcgnn_spmm %s" % walk
                build = lambda p, ws, nb: (plan, p["X"], p["Y"], D, ws, nb, cs.stream)   # noqa: E731
                out = cs.call(what, lib.tcgnn_spmm, build, {"Y": ((cs.n, D), F32)}, {"X": X}, cs.ws_bytes(plan))
                kernel = cs.kernel(plan)
                if out is None:
                    return
                Y = out["Y"]
                what += " (%s)" % kernel
                if cs.written(what, "Y", Y):
                    cs.judge("forward %s (%s)" % (walk, kernel), Y, ref["spmm"], cs.zero)
                cs.same(what, Y, T.forward(tX, *cs.meta)[0])
                if T.last_kernel(*cs.meta) != kernel:
                    cs.fail.append("%s: the module's call ran %r" % (what, T.last_kernel(*cs.meta)))
                if walk == "auto":    # Y one float late: refused before anything is enqueued
                    cs.call(what + " with Y one float late", lib.tcgnn_spmm, build, {"Y": ((cs.n, D), F32)}, {"X": X}, cs.ws_bytes(plan), offsets=("Y",), expect=INVALID_ARG)
                if cs.offsets and walk in OFFSET_WALKS["forward"]:
                    o = cs.call(what + " with X one float late", lib.tcgnn_spmm, build, {"Y": ((cs.n, D), F32)}, {"X": X}, cs.ws_bytes(plan), offsets=("X",))
                    cs.same(what + " with X one float late", o and o["Y"], Y, "the aligned call")
            finally:
                cs.destroy(plan)
        cs.forced("forward", walk, body)
        cs.end_of_walk("tcgnn_spmm %s" % walk)


def _run_epilogues(cs):
    """tcgnn_spmm_fused (ReLU; gate) and tcgnn_spmm_scaled (all four operands, ReLU) on the automatic walk and on mode 3."""
    name, D, T, lib, n = cs.name, cs.D, cs.T, cs.lib, cs.n
    ref, (X, _), (bp, e2c, e2r) = W.references(name, cs.rp, cs.col, D, ops=("spmm",))
    base, r64, s64 = ref["spmm"]
    rng = np.random.default_rng(1000 + D)
    r = rng.uniform(0.1, 1.0, n).astype(np.float32); cscale = rng.uniform(0.1, 1.0, n).astype(np.float32); b = rng.standard_normal(D).astype(np.float32)
    gate = rng.standard_normal((n, D)).astype(np.float32)            # a fixed mask: half of the elements pass
    rows = cs.rows

    def refs():
        Xg = (X * (gate > 0)).astype(np.float32)
        g = O.spmm(Xg, cs.rp, cs.col, bp, e2c, e2r, round_mode=O.ROUND_TF32); g64, gs64 = O.spmm_f64(Xg, cs.rp, cs.col)
        Xc = (cscale[:, None] * Xg).astype(np.float32)
        a = O.spmm(Xc, cs.rp, cs.col, bp, e2c, e2r, round_mode=O.ROUND_TF32); a64, as64 = O.spmm_f64(Xc, cs.rp, cs.col)
        for z in (g, g64, gs64, a, a64, as64):
            z[rows:] = 0
        pre = (a * r[:, None] + b).astype(np.float32)
        pre64 = a64 * r[:, None].astype(np.float64) + b.astype(np.float64)
        return (g, g64, gs64), (np.maximum(pre, 0), np.maximum(pre64, 0), as64 * r[:, None].astype(np.float64) + np.abs(b).astype(np.float64))
    gate_ref, scaled_ref = _cached(name, D, "epilogue refs", refs)
    tX = _cached(name, D, "tX", lambda: to_dev(cs.dev, X)[0])
    tr, tc, tb, tg = _cached(name, D, "epilogue tensors", lambda: to_dev(cs.dev, r, cscale, b, gate))
    Y_shape = {"Y": ((n, D), F32)}
    for walk in _walks_for(name, "epilogues"):
        def body():
            plan = cs.plan()
            try:
                need = lambda: cs.ws_bytes(plan)   # noqa: E731
                fused = lambda relu, gated: (lambda p, ws, nb: (plan, p["X"], p["gate"] if gated else None, p["Y"], D, relu, ws, nb, cs.stream))   # noqa: E731
                what = "tcgnn_spmm_fused(relu) %s" % walk
                out = cs.call(what, lib.tcgnn_spmm_fused, fused(1, False), Y_shape, {"X": X}, need())
                if out is not None and cs.written(what, "Y", out["Y"]):
                    cs.judge("epilogues %s relu (%s)" % (walk, cs.kernel(plan)), out["Y"], (np.maximum(base, 0), np.maximum(r64, 0), s64), cs.zero)
                    cs.same(what, out["Y"], T.forward_fused(tX, *cs.meta, relu=True)[0])
                what = "tcgnn_spmm_fused(gate) %s" % walk
                out = cs.call(what, lib.tcgnn_spmm_fused, fused(0, True), Y_shape, {"X": X, "gate": gate}, need())
                if out is not None and cs.written(what, "Y", out["Y"]):
                    cs.judge("epilogues %s gate (%s)" % (walk, cs.kernel(plan)), out["Y"], gate_ref, cs.zero)
                    cs.same(what, out["Y"], T.forward_fused(tX, *cs.meta, gate=tg)[0])
                what = "tcgnn_spmm_scaled %s" % walk
                scaled = lambda p, ws, nb: (plan, p["X"], p["col_scale"], p["gate"], p["row_scale"], p["bias"], p["Y"], D, 1, ws, nb, cs.stream)   # noqa: E731
                ins = {"X": X, "col_scale": cscale, "gate": gate, "row_scale": r, "bias": b}
                out = cs.call(what, lib.tcgnn_spmm_scaled, scaled, Y_shape, ins, need())
                if out is None:
                    return
                Y = out["Y"]
                if cs.written(what, "Y", Y):
                    cs.judge("epilogues %s scaled (%s)" % (walk, cs.kernel(plan)), Y, scaled_ref, cs.zero, np.maximum(b, 0))
                cs.same(what, Y, T.forward_scaled(tX, *cs.meta, row_scale=tr, col_scale=tc, bias=tb, relu=True, gate=tg)[0])
                if walk in ("auto", "range_blocked", "slice_synchronised"):
                    cs.call(what + " with Y one float late", lib.tcgnn_spmm_scaled, scaled, Y_shape, ins, need(), offsets=("Y",), expect=INVALID_ARG)
                if cs.offsets and walk in OFFSET_WALKS["epilogues"]:
                    for late in _variants((("X",), ("gate",), ("row_scale", "col_scale", "bias")), tuple(ins)):
                        w2 = "%s with %s one float late" % (what, " + ".join(late))
                        o = cs.call(w2, lib.tcgnn_spmm_scaled, scaled, Y_shape, ins, need(), offsets=late)
                        cs.same(w2, o and o["Y"], Y, "the aligned call")
            finally:
                cs.destroy(plan)
        cs.forced("epilogues", walk, body)
        cs.end_of_walk("epilogues %s" % walk)


def _run_agnn(cs):
    name, D, T, lib = cs.name, cs.D, cs.T, cs.lib
    ref, (X, att), _ = W.references(name, cs.rp, cs.col, D, ops=("spmm_val",))
    tX = _cached(name, D, "tX", lambda: to_dev(cs.dev, X)[0])
    tatt = _cached(name, D, "tatt", lambda: to_dev(cs.dev, att)[0].view(1, -1))
    m = cs.meta
    for walk in _walks_for(name, "forward_AGNN"):
        def body():
            plan = cs.plan()
            try:
                # the stream of the LDS-resident edge-valued walk is built BEFORE the workspace is sized, as the header prescribes (on both
                # plans: the first call would otherwise still take a gather walk, or not, by the size of the workspace it was given)
                cs.c.check(lib.tcgnn_plan_prepare_val(plan, D, cs.stream), "tcgnn_plan_prepare_val")
                T.prepare([D], *m, edge_valued=True)
                what = "tcgnn_spmm_val %s" % walk
                build = lambda p, ws, nb: (plan, p["X"], p["val"], p["Y"], D, ws, nb, cs.stream)   # noqa: E731
                ins, Y_shape = {"X": X, "val": att}, {"Y": ((cs.n, D), F32)}
                out = cs.call(what, lib.tcgnn_spmm_val, build, Y_shape, ins, cs.ws_bytes(plan))
                kernel = cs.kernel(plan)
                if out is None:
                    return
                Y = out["Y"]
                what += " (%s)" % kernel
                if cs.written(what, "Y", Y):
                    cs.judge("forward_AGNN %s (%s)" % (walk, kernel), Y, ref["spmm_val"], cs.zero)
                cs.same(what, Y, T.forward_AGNN(tX, m[0], m[1], tatt, *m[2:])[0])
                if T.last_kernel(*m) != kernel:
                    cs.fail.append("%s: the module's call ran %r" % (what, T.last_kernel(*m)))
                if walk == "auto":
                    cs.call(what + " with Y one float late", lib.tcgnn_spmm_val, build, Y_shape, ins, cs.ws_bytes(plan), offsets=("Y",), expect=INVALID_ARG)
                if cs.offsets and walk in OFFSET_WALKS["forward_AGNN"]:
                    for late in _variants((("X",), ("val",)), ("X", "val")):
                        w2 = "%s with %s one float late" % (what, " + ".join(late))
                        o = cs.call(w2, lib.tcgnn_spmm_val, build, Y_shape, ins, cs.ws_bytes(plan), offsets=late)
                        cs.same(w2, o and o["Y"], Y, "the aligned call")
            finally:
                cs.destroy(plan)
        cs.forced("forward_AGNN", walk, body)
        cs.end_of_walk("tcgnn_spmm_val %s" % walk)


def _run_sddmm(cs):
    """tcgnn_sddmm, and tcgnn_sddmm2 with the same matrix as two separately guarded operands: its scores are tcgnn_sddmm's bit for bit."""
    name, D, T, lib = cs.name, cs.D, cs.T, cs.lib
    if cs.nnz == 0:
        return
    ref, (X, _), _ = W.references(name, cs.rp, cs.col, D, ops=("sddmm",))
    tX = _cached(name, D, "tX", lambda: to_dev(cs.dev, X)[0])
    ef_shape = {"ef": ((cs.nnz,), F32)}
    for walk in _walks_for(name, "forward_ef"):
        def body():
            plan = cs.plan()
            try:
                what = "tcgnn_sddmm %s" % walk
                build = lambda p, ws, nb: (plan, p["X"], p["ef"], D, ws, nb, cs.stream)   # noqa: E731
                out = cs.call(what, lib.tcgnn_sddmm, build, ef_shape, {"X": X}, cs.ws_bytes(plan))
                kernel = cs.kernel(plan)
                if out is None:
                    return
                ef = out["ef"]
                what += " (%s)" % kernel
                if cs.written(what, "ef", ef):
                    cs.judge("forward_ef %s (%s)" % (walk, kernel), ef, ref["sddmm"])
                cs.same(what, ef, T.forward_ef(tX, *cs.meta)[0])
                w2 = "tcgnn_sddmm2(X, X) %s" % walk
                build2 = lambda p, ws, nb: (plan, p["X"], p["Z"], p["ef"], D, ws, nb, cs.stream)   # noqa: E731
                need2 = int(lib.tcgnn_sddmm2_workspace_bytes(plan, D))
                o2 = cs.call(w2, lib.tcgnn_sddmm2, build2, ef_shape, {"X": X, "Z": X}, need2)
                if o2 is not None and cs.written(w2, "ef", o2["ef"]):
                    cs.same(w2, o2["ef"], ef, "tcgnn_sddmm's scores")
                if cs.offsets and walk in OFFSET_WALKS["forward_ef"]:
                    for late in _variants((("X",), ("ef",)), ("X", "ef")):
                        w3 = "%s with %s one float late" % (what, " + ".join(late))
                        o = cs.call(w3, lib.tcgnn_sddmm, build, ef_shape, {"X": X}, cs.ws_bytes(plan), offsets=late)
                        cs.same(w3, o and o["ef"], ef, "the aligned call")
                    for late in _variants((("X",), ("Z",)), ("X", "Z", "ef")):
                        w3 = "%s with %s one float late" % (w2, " + ".join(late))
                        o = cs.call(w3, lib.tcgnn_sddmm2, build2, ef_shape, {"X": X, "Z": X}, need2, offsets=late)
                        cs.same(w3, o and o["ef"], ef, "the aligned call")
            finally:
                cs.destroy(plan)
        cs.forced("forward_ef", walk, body)
        cs.end_of_walk("tcgnn_sddmm %s" % walk)


def _run_fused(cs):
    name, D, T, lib, n, nnz = cs.name, cs.D, cs.T, cs.lib, cs.n, cs.nnz
    _, (X, _), (bp, e2c, e2r) = W.references(name, cs.rp, cs.col, D, ops=("sddmm",))
    H = (X / np.sqrt(D)).astype(np.float32)
    dY = np.random.default_rng(2000 + D).standard_normal((n, D)).astype(np.float32)
    wv = np.array([0.7], np.float32)
    tH, tdY, tw = _cached(name, D, "fused tensors", lambda: to_dev(cs.dev, H, dY, wv))
    rows, m = cs.rows, cs.meta
    e_cut = int(cs.rp[rows])
    refusal = nnz < 8 or W.is_unsorted(name)      # (the fused pair wants E >= 8 and a canonical plan: TCGNN_ERR_UNSUPPORTED, nothing written)

    def refs_for(ef_np):
        att = (wv[0] * ef_np).astype(np.float32)
        e = O.sddmm(H, cs.rp, cs.col, bp, e2c, e2r, round_mode=O.ROUND_TF32); e64, es64 = O.sddmm_f64(H, cs.rp, cs.col)
        y = O.spmm_val(H, cs.rp, cs.col, att, bp, e2c, e2r, round_mode=O.ROUND_TF32); y64, ys64 = O.spmm_f64(H, cs.rp, cs.col, att)
        g = O.spmm_val(dY, cs.rp, cs.col, att, bp, e2c, e2r, round_mode=O.ROUND_TF32); g64, gs64 = O.spmm_f64(dY, cs.rp, cs.col, att)
        d_att = O.sddmm(dY, cs.rp, cs.col, bp, e2c, e2r, round_mode=O.ROUND_TF32).astype(np.float64)
        for a in (y, y64, ys64, g, g64, gs64):
            a[rows:] = 0
        for a in (e, e64, es64, d_att):
            a[e_cut:] = 0
        return (e, e64, es64), (y, y64, ys64), (g, g64, gs64), float((d_att * cs.col).sum()), float((np.abs(d_att) * cs.col).sum()) + 1.0
    fwd_outs = {"ef": ((nnz,), F32), "ef_absmax": ((1 + n,), I32), "Y": ((n, D), F32)}
    bwd_outs = {"G": ((n, D), F32), "dw": ((1,), F32)}
    for walk in _walks_for(name, "agnn_fused"):
        def body():
            plan = cs.plan()
            try:
                need = lambda: cs.ws_bytes(plan)   # noqa: E731
                what = "tcgnn_agnn_pair_forward %s" % walk
                fwd = lambda words: (lambda p, ws, nb: (plan, p["H"], p["w"], p["ef"], p["ef_absmax"], words, p["Y"], D, ws, nb, cs.stream))   # noqa: E731
                ins = {"H": H, "w": wv}
                if refusal:
                    cs.call(what, lib.tcgnn_agnn_pair_forward, fwd(1 + n), fwd_outs, ins, need(), expect=UNSUPPORTED)
                    return
                out = cs.call(what, lib.tcgnn_agnn_pair_forward, fwd(1 + n), fwd_outs, ins, need())
                kf = cs.kernel(plan)
                if out is None:
                    return
                what += " (%s)" % kf
                ef, efm, Y = out["ef"], out["ef_absmax"], out["Y"]
                # (a row beyond the windows handed over has no exponent: words 1 + rows .. stay as they were)
                ok = cs.written(what, "ef", ef) & cs.written(what, "Y", Y) & cs.written(what, "ef_absmax[: 1 + rows]", efm[: 1 + rows])
                Ym, efm_m_ef, efm_m = T.agnn_fused_forward(tH, m[0], m[1], tw, *m[2:])
                cs.same(what + " Y", Y, Ym); cs.same(what + " ef", ef, efm_m_ef); cs.same(what + " ef_absmax", efm[: 1 + rows], efm_m[: 1 + rows])
                if not ok:
                    return
                (e, e64, es64), yref, gref, want, term_scale = _cached(name, D, "fused refs " + str(hash(ef.cpu().numpy().tobytes())), lambda: refs_for(ef.cpu().numpy()))
                cs.judge("agnn_fused %s scores (%s)" % (walk, kf), ef, (e, e64, es64))
                cs.judge("agnn_fused %s Y (%s)" % (walk, kf), Y, yref, cs.zero)
                # d_ef_absmax with N words: one short of what the call writes
                if walk == "auto":
                    short = dict(fwd_outs, ef_absmax=((n,), I32))
                    cs.call(what + " with N words of ef_absmax", lib.tcgnn_agnn_pair_forward, fwd(n), short, ins, need(), expect=INVALID_ARG)
                    cs.call(what + " with Y one float late", lib.tcgnn_agnn_pair_forward, fwd(1 + n), fwd_outs, ins, need(), offsets=("Y",), expect=INVALID_ARG)
                # ---- backward, from the saved scores as operands of their own
                ef_np, efm_np = ef.cpu().numpy().copy(), efm.cpu().numpy().copy()
                wb = "tcgnn_agnn_pair_backward %s" % walk
                bwd = lambda words: (lambda p, ws, nb: (plan, p["dY"], p["w"], p["ef saved"], p["ef_absmax saved"], words, p["G"], p["dw"], D, ws, nb, cs.stream))   # noqa: E731
                cs.ins = {k: v for k, v in cs.ins.items() if "saved" not in k[0]}      # (this walk's own scores)
                bins = {"dY": dY, "w": wv, "ef saved": ef_np, "ef_absmax saved": efm_np}
                ob = cs.call(wb, lib.tcgnn_agnn_pair_backward, bwd(1 + n), bwd_outs, bins, need())
                kb = cs.kernel(plan)
                if ob is None:
                    return
                wb += " (%s)" % kb
                Gm, dwm = T.agnn_fused_backward(tdY, m[0], m[1], tw, efm_m_ef, efm_m, *m[2:])
                cs.same(wb + " G", ob["G"], Gm); cs.same(wb + " d_w", ob["dw"], dwm)
                if cs.written(wb, "G", ob["G"]) & cs.written(wb, "dw", ob["dw"]):
                    cs.judge("agnn_fused %s G (%s)" % (walk, kb), ob["G"], gref, cs.zero)
                    if not abs(float(ob["dw"]) - want) <= 1e-6 * term_scale:
                        cs.fail.append("%s: d_w %.6e, want %.6e (terms %.3e)" % (wb, float(ob["dw"]), want, term_scale))
                if walk == "auto":
                    cs.call(wb + " with N words of ef_absmax", lib.tcgnn_agnn_pair_backward, bwd(n), bwd_outs, bins, need(), expect=INVALID_ARG)
                    cs.call(wb + " with G one float late", lib.tcgnn_agnn_pair_backward, bwd(1 + n), bwd_outs, bins, need(), offsets=("G",), expect=INVALID_ARG)
                if cs.offsets and walk in OFFSET_WALKS["agnn_fused"]:
                    for late in _variants((("H",), ("w",), ("ef", "ef_absmax")), ("H", "w", "ef", "ef_absmax")):
                        w2 = "%s with %s one float late" % (what, " + ".join(late))
                        o = cs.call(w2, lib.tcgnn_agnn_pair_forward, fwd(1 + n), fwd_outs, ins, need(), offsets=late)
                        if o is not None:
                            cs.same(w2 + " Y", o["Y"], Y, "the aligned call"); cs.same(w2 + " ef", o["ef"], ef, "the aligned call")
                            cs.same(w2 + " ef_absmax", o["ef_absmax"][: 1 + rows], efm[: 1 + rows], "the aligned call")
                    for late in _variants((("dY",), ("ef saved", "ef_absmax saved"), ("dw",)), ("dY", "w", "ef saved", "ef_absmax saved", "dw")):
                        w2 = "%s with %s one float late" % (wb, " + ".join(late))
                        o = cs.call(w2, lib.tcgnn_agnn_pair_backward, bwd(1 + n), bwd_outs, bins, need(), offsets=late)
                        if o is not None:
                            cs.same(w2 + " G", o["G"], ob["G"], "the aligned call"); cs.same(w2 + " d_w", o["dw"], ob["dw"], "the aligned call")
            finally:
                cs.destroy(plan)
        cs.forced("agnn_fused", walk, body)
        cs.end_of_walk("agnn pair %s" % walk)


RUNNERS = {"forward": _run_forward, "epilogues": _run_epilogues, "forward_AGNN": _run_agnn, "forward_ef": _run_sddmm, "agnn_fused": _run_fused}


def _finish(cs, what):
    cs.end_of_case()
    assert not cs.fail, "%s:\n  " % what + "\n  ".join(cs.fail)


@pytest.mark.parametrize("name,D,op", CASES, ids=["%s-D%d-%s" % c for c in CASES])
def test_every_walk_keeps_the_memory_contract(dev, T, monkeypatch, name, D, op):
    cs = Case(dev, T, monkeypatch, name, D)
    RUNNERS[op](cs)
    _finish(cs, "%s D=%d %s" % (name, D, op))


# ------------------------------------------------------------------------------------------------------------------ the rest of the ABI

GEMM_GRAPHS = ("uniform_n17", "uniform_n40", "range_boundary_columns_n4585", "short_metadata_n4100")


@pytest.mark.parametrize("dims", [(64, 41), (41, 7)], ids=["64x41", "41x7"])
@pytest.mark.parametrize("name", GEMM_GRAPHS)
def test_dense_update_keeps_the_memory_contract(dev, T, monkeypatch, name, dims):
    """tcgnn_spmm_gemm: Y is [N, D_out] - the memset of a plan with fewer windows than rows, the LDS-resident kernel's zeroed Y and every
    store are sized by D_out, the workspace by D_in.  Value: the oracle's aggregate times W in fp64, at the distance
    test_dense_update_fused_behind_the_aggregation allows (2 TIGHT of (sum|a||x| + 1) |W| + 1)."""
    din, dout = dims
    cs = Case(dev, T, monkeypatch, name, din)
    lib = cs.lib
    ref, (X, _), _ = W.references(name, cs.rp, cs.col, din, ops=("spmm",))
    Wm = (np.random.default_rng(din * 131 + dout).standard_normal((din, dout)) / np.sqrt(din)).astype(np.float32)
    agg, _, s64 = ref["spmm"]
    want = agg.astype(np.float64) @ Wm.astype(np.float64)
    bound = (s64 + 1.0) @ np.abs(Wm.astype(np.float64)) + 1.0
    tX, tW = to_dev(dev, X, Wm)
    for walk in ("auto", "per_window", "lds_ordinary", "lds_flat1"):
        def body():
            plan = cs.plan()
            try:
                what = "tcgnn_spmm_gemm %s" % walk
                build = lambda p, ws, nb: (plan, p["X"], p["W"], p["Y"], din, dout, 0, ws, nb, cs.stream)   # noqa: E731
                outs, ins = {"Y": ((cs.n, dout), F32)}, {"X": X, "W": Wm}
                out = cs.call(what, lib.tcgnn_spmm_gemm, build, outs, ins, cs.ws_bytes(plan))
                if out is None:
                    return
                Y = out["Y"]
                what += " (%s)" % cs.kernel(plan)
                if cs.written(what, "Y", Y):
                    got = Y.cpu().numpy().astype(np.float64)
                    fig = float((np.abs(got - want) / bound).max())
                    print("FIG %-40s %.2e of the bound's scale" % (what, fig))
                    if not fig <= 2 * TIGHT:
                        cs.fail.append("%s: %.3e of (sum|a||x| + 1) |W| + 1 from the oracle's aggregate times W" % (what, fig))
                    if cs.zero.any() and not bool((Y[torch.from_numpy(cs.zero).to(dev)] == 0).all()):
                        cs.fail.append("%s: rows without edges are not exact zeros" % what)
                cs.same(what, Y, T.forward_gemm(tX, tW, *cs.meta)[0])
                if walk == "auto":
                    cs.call(what + " with Y one float late", lib.tcgnn_spmm_gemm, build, outs, ins, cs.ws_bytes(plan), offsets=("Y",), expect=INVALID_ARG)
                if name in OFFSET_GRAPHS:
                    for late in _variants((("X",), ("W",)), ("X", "W")):
                        w2 = "%s with %s one float late" % (what, " + ".join(late))
                        o = cs.call(w2, lib.tcgnn_spmm_gemm, build, outs, ins, cs.ws_bytes(plan), offsets=late)
                        cs.same(w2, o and o["Y"], Y, "the aligned call")
            finally:
                cs.destroy(plan)
        cs.forced("forward", walk, body)
        cs.end_of_walk("tcgnn_spmm_gemm %s" % walk)
    _finish(cs, "%s %dx%d tcgnn_spmm_gemm" % (name, din, dout))


@pytest.mark.parametrize("D", [41, 64, 128])
def test_transposed_plan_with_permuted_edge_values(dev, T, monkeypatch, D):
    """upper_band200_n4100 (directed): A^T's plan from the host transpose, tcgnn_permute_edge_values into a buffer of exactly E floats,
    tcgnn_spmm_val on it - against the oracle on A^T and bit-equal to forward_AGNN(transpose=True)."""
    name = "upper_band200_n4100"
    rp, col = GRAPHS[name]
    n, nnz = len(rp) - 1, len(col)
    trp, tcol, perm = W.transposed_csr(rp, col)
    tbp, te2c, te2r = W.host_meta(trp, tcol)
    X, att = W.case_data(n, nnz, D)
    att_t = att[perm]
    ref = (O.spmm_val(X, trp, tcol, att_t, tbp, te2c, te2r, round_mode=O.ROUND_TF32),) + O.spmm_f64(X, trp, tcol, att_t)
    cs = Case(dev, T, monkeypatch, name, D)
    lib = cs.lib
    meta_t = tuple(to_dev(dev, trp, tcol, tbp, te2c, te2r))
    snap_t = tuple(G.snapshot(t) for t in meta_t)
    tX, tatt = to_dev(dev, X, att)
    m = cs.meta
    for walk in ("auto", "per_window", "lds_val"):
        def body():
            plan = cs.c._vp()
            cs.c.check(lib.tcgnn_plan_create(*[t.data_ptr() for t in meta_t], n, nnz, meta_t[2].numel(), cs.stream, ctypes.byref(plan)), "tcgnn_plan_create")
            try:
                what = "tcgnn_permute_edge_values"
                out = cs.call(what, lib.tcgnn_permute_edge_values, lambda p, ws, nb: (p["val"], p["perm"], nnz, p["out"], cs.stream),
                              {"out": ((nnz,), F32)}, {"val": att, "perm": perm.astype(np.int32)}, None)
                if out is None or not cs.written(what, "out", out["out"]):
                    return
                cs.same(what, out["out"], torch.from_numpy(att_t).to(dev), "val[perm]")
                if walk == "auto":
                    for late in _variants((("val",), ("perm",), ("out",)), ("val", "perm", "out")):
                        o = cs.call("%s with %s one element late" % (what, " + ".join(late)), lib.tcgnn_permute_edge_values,
                                    lambda p, ws, nb: (p["val"], p["perm"], nnz, p["out"], cs.stream), {"out": ((nnz,), F32)}, {"val": att, "perm": perm.astype(np.int32)}, None,
                                    offsets=late)
                        cs.same(what + " (offset)", o and o["out"], out["out"], "the aligned call")
                cs.c.check(lib.tcgnn_plan_prepare_val(plan, D, cs.stream), "tcgnn_plan_prepare_val")
                T.prepare([D], *m, edge_valued=True, transpose=True)
                what = "tcgnn_spmm_val on A^T %s" % walk
                need = int(lib.tcgnn_workspace_bytes(plan, D))
                o = cs.call(what, lib.tcgnn_spmm_val, lambda p, ws, nb: (plan, p["X"], p["val_t"], p["Y"], D, ws, nb, cs.stream), {"Y": ((n, D), F32)},
                            {"X": X, "val_t": att_t}, need)
                if o is None:
                    return
                what += " (%s)" % cs.kernel(plan)
                if cs.written(what, "Y", o["Y"]):
                    cs.judge(what, o["Y"], ref, np.diff(trp) == 0)
                cs.same(what, o["Y"], T.forward_AGNN(tX, m[0], m[1], tatt.view(1, -1), *m[2:], transpose=True)[0])
            finally:
                cs.destroy(plan)
        cs.forced("forward_AGNN", walk, body)
        cs.end_of_walk(walk)
        for t, s, l in zip(meta_t, snap_t, ("nodePointer_t", "edgeList_t", "blockPartition_t", "edgeToColumn_t", "edgeToRow_t")):
            if not G.unchanged(t, s):
                cs.fail.append("%s: the metadata array %s was written" % (walk, l))
    _finish(cs, "%s D=%d transposed plan" % (name, D))


SGT_GRAPHS = EDGE_NAMES + ("range_boundary_columns_n4585",)


@pytest.mark.parametrize("name", SGT_GRAPHS)
def test_device_sgt_and_transpose_on_exact_scratch(dev, T, monkeypatch, name):
    """tcgnn_preprocess_gpu_ws and tcgnn_transpose_ws with scratch of exactly ..._workspace_bytes (256-byte aligned, between moats) and
    guarded outputs of bp_len, E, E and N + 1, E, E elements: equal to the host SGT and to walks.transposed_csr, moats intact, one byte
    less of scratch refused with the outputs untouched.  (test_device_sgt_with_edge_arrays_longer_than_the_csr pins that edge arrays
    LONGER than the CSR keep their tail, test_device_sgt_on_caller_scratch_allocates_nothing that the scratch of the size asked for
    is enough at 200 k nodes and that 256 bytes less are refused - both on torch allocations, without moats; not repeated here.)"""
    cs = Case(dev, T, monkeypatch, name, 16)
    lib, n, nnz = cs.lib, cs.n, cs.nnz
    nw = (n + 15) // 16
    bp_h, e2c_h, e2r_h, total = S.graphs.host_sgt(cs.rp, cs.col)
    need = ctypes.c_size_t(0)
    cs.c.check(lib.tcgnn_preprocess_gpu_workspace_bytes(n, nnz, 16, ctypes.byref(need)), "tcgnn_preprocess_gpu_workspace_bytes")
    got = ctypes.c_int64(-1)
    ins = {"edgeList": cs.col.astype(np.int32), "nodePointer": cs.rp.astype(np.int32)}
    out = cs.call("tcgnn_preprocess_gpu_ws", lib.tcgnn_preprocess_gpu_ws,
                  lambda p, ws, nb: (p["edgeList"], p["nodePointer"], n, nnz, 16, 8, p["blockPartition"], nw, p["edgeToColumn"], p["edgeToRow"], ws, nb, ctypes.byref(got), cs.stream),
                  {"blockPartition": ((nw,), I32), "edgeToColumn": ((nnz,), I32), "edgeToRow": ((nnz,), I32)}, ins, int(need.value))
    if out is not None:
        for l, want in (("blockPartition", bp_h), ("edgeToColumn", e2c_h), ("edgeToRow", e2r_h)):
            cs.same("tcgnn_preprocess_gpu_ws " + l, out[l], torch.from_numpy(want).to(dev), "the host SGT")
        if got.value != total:
            cs.fail.append("tcgnn_preprocess_gpu_ws: TC_Blocks %d, host %d" % (got.value, total))
    cs.c.check(lib.tcgnn_transpose_workspace_bytes(n, nnz, ctypes.byref(need)), "tcgnn_transpose_workspace_bytes")
    sym = ctypes.c_int32(-1)
    out = cs.call("tcgnn_transpose_ws", lib.tcgnn_transpose_ws,
                  lambda p, ws, nb: (p["nodePointer"], p["edgeList"], n, nnz, p["nodePointer_t"], p["edgeList_t"], p["perm"], ws, nb, ctypes.byref(sym), cs.stream),
                  {"nodePointer_t": ((n + 1,), I32), "edgeList_t": ((nnz,), I32), "perm": ((nnz,), I32)}, ins, int(need.value))
    if out is not None:
        trp, tcol, perm = W.transposed_csr(cs.rp, cs.col)
        for l, want in (("nodePointer_t", trp), ("edgeList_t", tcol), ("perm", perm.astype(np.int32))):
            cs.same("tcgnn_transpose_ws " + l, out[l], torch.from_numpy(want).to(dev), "walks.transposed_csr")
        if sym.value != int(W.is_symmetric(cs.rp, cs.col)):
            cs.fail.append("tcgnn_transpose_ws: symmetric = %d" % sym.value)
    _finish(cs, "%s device SGT and transpose" % name)


@pytest.mark.parametrize("D", [41, 64, 100])
@pytest.mark.parametrize("name", OFFSET_GRAPHS)
def test_caller_staged_images_keep_the_memory_contract(dev, T, monkeypatch, name, D):
    """tcgnn_stage_absmax / tcgnn_stage_rows / tcgnn_spmm_staged and the planar pair: an image of exactly the header's size (256 bytes
    + (N + 1) rows of tcgnn_x16_pitch(D) halves; 256 + ceil(D / 16) planes of N + 1 32-byte records), 256-byte aligned between moats;
    Y bit-equal to tcgnn_spmm on the same walk (mode 1; mode 3 for the planar image), the image read-only to the SpMM, X one float
    late gives the same image, a destination or a Y that is not aligned as the header asks is refused."""
    cs = Case(dev, T, monkeypatch, name, D)
    lib, n = cs.lib, cs.n
    _, (X, _), _ = W.references(name, cs.rp, cs.col, D, ops=("spmm",))
    tX = to_dev(dev, X)[0]
    pitch = int(lib.tcgnn_x16_pitch(D))
    planes = (D + 15) // 16
    for walk, layout in (("per_window", "rows"), ("lds_flat1", "planar"), ("lds_ordinary", "planar")):
        def body():
            plan = cs.plan()
            try:
                if layout == "planar" and not lib.tcgnn_spmm_staged_layout(plan, D, cs.stream):
                    print("OBS %s D=%d %s: tcgnn_spmm_staged_layout says row-major" % (name, D, walk))
                    return
                nbytes = 256 + ((n + 1) * pitch * 2 if layout == "rows" else planes * (n + 1) * 32)
                for late in ((), ("X",)):
                    imb, image = G.exact_workspace(dev, nbytes)
                    image.zero_()                                      # (the header's other words, the sentinel record and all padding are zero)
                    img = G.address(imb)
                    xb, xv, xs = cs.inp("X", X, 1 if late else 0)
                    cs.c.check(lib.tcgnn_stage_absmax(G.address(xb), n * D, img, cs.stream), "tcgnn_stage_absmax")
                    if layout == "rows":
                        st = lib.tcgnn_stage_rows(G.address(xb), n, D, img, img + 256, cs.stream)
                    else:
                        st = lib.tcgnn_stage_rows_planar(G.address(xb), n, D, img, img + 256, n + 1, cs.stream)
                    cs.status(st, "tcgnn_stage_rows")
                    what = "staged %s image%s, %s" % (layout, " (X one float late)" if late else "", walk)
                    if st != OK:
                        cs.fail.append("%s: staging returned %d" % (what, st))
                        return
                    if G.moat_intact(imb, image) or not G.unchanged(xv, xs):
                        cs.fail.append("%s: staging wrote outside the image (%s) or into X" % (what, G.moat_intact(imb, image)[:4]))
                    if not late:
                        first = G.snapshot(image)
                    elif not G.unchanged(image, first):
                        cs.fail.append("%s: the image differs from the one staged from the aligned X" % what)
                    fn = lib.tcgnn_spmm_staged if layout == "rows" else lib.tcgnn_spmm_staged_planar
                    snap = G.snapshot(image)
                    out = cs.call(what, fn, lambda p, ws, nb: (plan, img, p["Y"], D, cs.stream), {"Y": ((n, D), F32)}, {}, None)
                    if out is not None and cs.written(what, "Y", out["Y"]):
                        cs.same(what, out["Y"], T.forward(tX, *cs.meta)[0], "tcgnn_spmm on the same walk")
                    if not G.unchanged(image, snap) or G.moat_intact(imb, image):
                        cs.fail.append("%s: the SpMM wrote into the staged image or around it" % what)
                    if not late:
                        cs.call(what + " with Y one float late", fn, lambda p, ws, nb: (plan, img, p["Y"], D, cs.stream), {"Y": ((n, D), F32)}, {}, None,
                                offsets=("Y",), expect=INVALID_ARG)
                        bad_dst = lib.tcgnn_stage_rows(G.address(xb), n, D, img, img + 256 + 4, cs.stream) if layout == "rows" else \
                            lib.tcgnn_stage_rows_planar(G.address(xb), n, D, img, img + 256 + 16, n + 1, cs.stream)
                        if bad_dst != INVALID_ARG or not G.unchanged(image, snap):
                            cs.fail.append("%s: a destination off its alignment returned %d" % (what, bad_dst))
            finally:
                cs.destroy(plan)
        cs.forced("forward", walk, body)
        cs.end_of_walk("staged %s" % walk)
    _finish(cs, "%s D=%d staged images" % (name, D))


def test_the_matrix_covers_what_it_claims():
    """the catalogue entries exist, every operator has a case on every graph at every width, and the offset cases are among them"""
    assert set(GRAPHS) == set(EDGE_NAMES + BOUNDARY_NAMES + (BUCKET_NAME, SYNC_NAME)) and len(GRAPHS) == 17
    assert sorted({len(GRAPHS[n][0]) - 1 for n in EDGE_NAMES}) == [1, 15, 16, 17, 32, 40, 48]
    seen = {(n, op): {D for nn, D, o in CASES if nn == n and o == op} for n in GRAPHS for op in OPS}
    for (n, op), ds in seen.items():
        assert ds == set(_widths(n, op)) and _walks_for(n, op), (n, op)
        if n in OFFSET_GRAPHS:
            assert set(OFFSET_WIDTHS) <= ds and set(OFFSET_WALKS[op]) <= set(_walks_for(n, op)), (n, op)
    assert 201 in seen[(BOUNDARY_NAMES[0], "forward")] and 201 in seen[(BOUNDARY_NAMES[1], "forward")] and 160 in seen[("complete_n1030", "forward_ef")]
    assert _walks_for(SYNC_NAME, "forward") == ("slice_synchronised",) and "range_blocked" in _walks_for(BUCKET_NAME, "forward")
    print("CASES %d matrix cases" % len(CASES))
    sys.stdout.flush()
