"""The one-pass staging of the planar image never shows in the result.  Needs an MI355X: `pytest -m gpu`.

Where X lies in whole aligned float4 rows and D is a multiple of 16, a call on an LDS-resident walk stages its planar fp16 image with
stage_fused_kernel + stage_settle_kernel (tcgnn_stage.inc): one pass over X that converts with the scale exponent the plan remembers
from the last call of its kind, and a short second launch that checks the guess - a HIT - or converts again with the true scale - a
MISS.  Either way the workspace must hold, bit for bit, what memset + abs-max + convert leave there.

Every call here goes through the C ABI (tcgnn_spmm, tcgnn_spmm_fused with a gate, tcgnn_spmm_scaled with a column scale) on a
workspace of exactly tcgnn_workspace_bytes between two moats, pre-filled with 0xff, and is repeated with tcgnn_set_stage_onepass(0) on
a second such workspace.  Compared, as bits: Y, the twelve header words, the bytes of the planar image, and tcgnn_range_mode.  The walk
is lds_flat1, forced as tests/walks.py forces it; another kernel in last_kernel is a failure.

Graphs (tests/graphs.py): uniform_n40 (fewer float4 than one workgroup's stride: one workgroup, partial round only) and
range_boundary_columns_n4585 (N % 16 = 9).  Widths: D = 16 (the second graph: 18 340 float4, five workgroups of one partial round
each - a slot reduction over several workgroups) and D = 64 (eighteen workgroups, four planes).

  scale sequence      X, X, 8 X, 8 X, X with one element raised across the next power of two, all-zero X, X on one plan: the plan's
                      counters must read miss, hit, miss, hit, miss after the first five
  interleaved kinds   plain, gated (the gate zeroes the largest element, 64 times the rest) and column-scaled calls in turn on one
                      plan: each kind has its own table entry, so from the second round on every call hits
  range guard         one 1e12 among O(1) values; one 1e-5 among 1e4's (the cases tcgnn_stage.inc's comments name), each on a miss
                      and on a hit; an X with Inf, an X with NaN
  hint poisoning      max |X| = 3e38 leaves the guess -113; the O(1) matrix after it is first converted to garbage (zeros) and must
                      still come out right"""
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
WIDTHS = (16, 64)
CASES = [(name, D) for name in GRAPHS for D in WIDTHS]
IDS = ["%s-D%d" % c for c in CASES]
HIP_ERROR = 2
MOAT = 4096
HDR_WORDS = 12


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


def _data(dev, name, D):
    """standard-normal X, a gate that lets half of the elements through, a column scale - made once per (graph, D)"""
    if (name, D) not in _DATA:
        n = len(GRAPHS[name][0]) - 1
        rng = np.random.default_rng(1000 * D + n)
        X, gate = (rng.standard_normal((n, D)).astype(np.float32) for _ in range(2))
        cs = rng.uniform(0.25, 4.0, n).astype(np.float32)
        _DATA[(name, D)] = tuple(to_dev(dev, X, gate, cs))
    return _DATA[(name, D)]


def _bits(t):
    return t.contiguous().view(torch.int32)


class Workspace:
    """exactly `need` bytes, 256-byte aligned, between two moats"""

    def __init__(self, dev, need):
        self.need = need
        self.buf = torch.empty(need + 2 * MOAT + 256, dtype=torch.uint8, device=dev)
        off = (-(self.buf.data_ptr() + MOAT)) % 256 + MOAT
        self.off = off
        self.ws = self.buf[off: off + need]
        assert self.ws.data_ptr() % 256 == 0

    def arm(self):
        self.buf.fill_(0xa5)
        self.ws.fill_(0xff)

    def moats_intact(self):
        return bool((self.buf[: self.off] == 0xa5).all()) and bool((self.buf[self.off + self.need:] == 0xa5).all())


class Plan:
    """one plan of a graph under lds_flat1, two workspaces, and the compared call"""

    def __init__(self, c, dev, name, D):
        self.c, self.lib, self.dev, self.name, self.D = c, c.lib, dev, name, D
        self.meta = _meta(dev, name)
        self.n, self.nnz = self.meta[0].numel() - 1, self.meta[1].numel()
        self.stream = torch.cuda.current_stream(dev).cuda_stream
        self.h = c._vp()
        self.ok(self.lib.tcgnn_plan_create(*[t.data_ptr() for t in self.meta], self.n, self.nnz, self.meta[2].numel(), self.stream, ctypes.byref(self.h)), "tcgnn_plan_create")
        self.ok(self.lib.tcgnn_plan_prepare(self.h, D, self.stream), "tcgnn_plan_prepare")
        need = int(self.lib.tcgnn_workspace_bytes(self.h, D))
        self.image_bytes = (D // 16) * (self.n + 1) * 32
        # the header, the image, the dirty-row bitmap and behind it the 256 x 16 bytes of slots all lie inside what the header prescribes
        assert need >= 256 + self.image_bytes + (self.n + 1 + 31) // 32 * 4 + 256 * 16
        self.one, self.two = Workspace(dev, need), Workspace(dev, need)

    def ok(self, st, what):
        if st == HIP_ERROR:
            pytest.exit("%s D=%d %s: TCGNN_ERR_HIP (%s) - a GPU fault: nothing more is run" % (self.name, self.D, what, self.lib.tcgnn_last_error().decode("utf-8", "replace")),
                        returncode=3)
        self.c.check(st, what)

    def destroy(self):
        torch.cuda.synchronize(self.dev)
        self.lib.tcgnn_plan_destroy(self.h)

    def stats(self):
        h, m = self.c._i64(0), self.c._i64(0)
        self.ok(self.lib.tcgnn_plan_stage_stats(self.h, self.stream, ctypes.byref(h), ctypes.byref(m)), "tcgnn_plan_stage_stats")
        return h.value, m.value

    def _once(self, w, kind, X, gate, cs):
        w.arm()
        Y = torch.empty(self.n, self.D, device=self.dev)
        p, nb, D, st = w.ws.data_ptr(), w.need, self.D, self.stream
        if kind == "plain":
            self.ok(self.lib.tcgnn_spmm(self.h, X.data_ptr(), Y.data_ptr(), D, p, nb, st), "tcgnn_spmm")
        elif kind == "gated":
            self.ok(self.lib.tcgnn_spmm_fused(self.h, X.data_ptr(), gate.data_ptr(), Y.data_ptr(), D, 0, p, nb, st), "tcgnn_spmm_fused")
        else:
            self.ok(self.lib.tcgnn_spmm_scaled(self.h, X.data_ptr(), cs.data_ptr(), None, None, None, Y.data_ptr(), D, 0, p, nb, st), "tcgnn_spmm_scaled")
        kernel = self.lib.tcgnn_plan_last_kernel(self.h).decode()
        a, b = self.c._i32(0), self.c._i32(0)
        self.ok(self.lib.tcgnn_range_mode(p, st, ctypes.byref(a), ctypes.byref(b)), "tcgnn_range_mode")
        torch.cuda.synchronize(self.dev)
        assert W.FORWARD_WALKS["lds_flat1"][2](kernel), "last_kernel is %r: the forced walk was not taken" % kernel
        assert w.moats_intact(), "%s wrote outside its workspace of %d bytes" % (kind, nb)
        hdr = w.ws[: 4 * HDR_WORDS].clone().view(torch.int32)
        image = w.ws[256: 256 + self.image_bytes].clone()
        return Y, hdr, image, (a.value, b.value)

    def compare(self, what, kind, X, gate=None, cs=None):
        """the call with the one-pass staging and with the two-pass staging; -> ("hit" | "miss", range mode) of the first"""
        assert X.data_ptr() % 16 == 0 and (gate is None or gate.data_ptr() % 16 == 0)
        try:
            h0, m0 = self.stats()
            self.ok(self.lib.tcgnn_set_stage_onepass(1), "tcgnn_set_stage_onepass")
            Y1, hdr1, im1, rm1 = self._once(self.one, kind, X, gate, cs)
            h1, m1 = self.stats()
            self.ok(self.lib.tcgnn_set_stage_onepass(0), "tcgnn_set_stage_onepass")
            Y2, hdr2, im2, rm2 = self._once(self.two, kind, X, gate, cs)
            assert self.stats() == (h1, m1), "%s: a two-pass call moved the one-pass counters" % what
        finally:
            self.lib.tcgnn_set_stage_onepass(1)
        assert (h1 - h0) + (m1 - m0) == 1, "%s: the one-pass staging did not take this call (hits %d -> %d, misses %d -> %d)" % (what, h0, h1, m0, m1)
        went = "hit" if h1 > h0 else "miss"
        print("OBS %s | %s D=%d | %s | %s | header %s | range_mode %s" % (what, self.name, self.D, kind, went, [hex(v & 0xffffffff) for v in hdr1.tolist()], rm1))
        assert torch.equal(hdr1, hdr2), "%s (%s): header words %s, two-pass %s" % (what, went, hdr1.tolist(), hdr2.tolist())
        assert torch.equal(im1, im2), "%s (%s): %d image bytes differ from the two-pass image" % (what, went, int((im1 != im2).sum()))
        assert torch.equal(_bits(Y1), _bits(Y2)), "%s (%s): %d elements of Y differ from the two-pass call" % (what, went, int((_bits(Y1) != _bits(Y2)).sum()))
        assert rm1 == rm2, "%s (%s): range_mode %s, two-pass %s" % (what, went, rm1, rm2)
        return went, rm1


def _with_plan(dev, T, monkeypatch, name, D, body):
    import tcgnn_capi as c
    mode, env, _ = W.FORWARD_WALKS["lds_flat1"]

    def run():
        plan = Plan(c, dev, name, D)
        try:
            return body(plan)
        finally:
            plan.destroy()
    return W.forced(T, monkeypatch, mode, env, run, {"n": len(GRAPHS[name][0]) - 1, "D": D, "capfd": None})


def _largest(X):
    i = int(torch.argmax(X.abs()))
    return i // X.shape[1], i % X.shape[1]


@pytest.mark.parametrize("name,D", CASES, ids=IDS)
def test_a_scale_sequence_hits_and_misses_as_the_exponent_moves(dev, T, monkeypatch, name, D):
    X = _data(dev, name, D)[0]
    r, c = _largest(X)
    top = float(X[r, c].abs())
    raised = X.clone()
    raised[r, c] = float(2.0 ** (np.floor(np.log2(top)) + 1))       # the smallest value of the next binade: the exponent moves by one
    assert np.floor(np.log2(float(raised.abs().max()))) == np.floor(np.log2(top)) + 1

    def body(p):
        seq = [("X", X), ("X again", X), ("8 X", 8 * X), ("8 X again", 8 * X), ("one element across the power of two", raised),
               ("all-zero X", torch.zeros_like(X)), ("X after zeros", X)]
        return [p.compare(what, "plain", x)[0] for what, x in seq]
    went = _with_plan(dev, T, monkeypatch, name, D, body)
    assert went[:5] == ["miss", "hit", "miss", "hit", "miss"], went


@pytest.mark.parametrize("name,D", CASES, ids=IDS)
def test_call_kinds_keep_their_own_guess(dev, T, monkeypatch, name, D):
    X0, gate0, cs = _data(dev, name, D)
    X, gate = X0.clone(), gate0.clone()
    r, c = _largest(X)
    X[r, c] = 64.0 * X[r, c]            # plain: the scale of 64 max; gated: the gate zeroes it, so the scale of what is left
    gate[r, c] = -1.0

    def body(p):
        out = []
        for rnd in range(3):
            out.append([p.compare("round %d" % rnd, kind, X, gate if kind == "gated" else None, cs if kind == "scaled" else None)[0] for kind in ("plain", "gated", "scaled")])
        return out
    went = _with_plan(dev, T, monkeypatch, name, D, body)
    assert went[0] == ["miss"] * 3 and went[1] == ["hit"] * 3 and went[2] == ["hit"] * 3, went


@pytest.mark.parametrize("name,D", CASES, ids=IDS)
def test_the_range_guard_decides_as_on_the_two_pass_path(dev, T, monkeypatch, name, D):
    X = _data(dev, name, D)[0]
    n = X.shape[0]
    huge = X.clone(); huge[n // 2, D - 1] = 1e12                      # one 1e12 among O(1) values: everything else loses bits
    stray = (1e4 * (1.0 + X.abs())).contiguous(); stray[n - 1, 0] = 1e-5   # one 1e-5 among 1e4's: one lost element
    inf = X.clone(); inf[0, 0] = float("inf")
    nan = X.clone(); nan[n - 1, D - 1] = float("nan")

    def body(p):
        out = {}
        for what, x in (("one 1e12", huge), ("one 1e-5", stray)):
            out[what] = [p.compare("%s, call %d" % (what, k), "plain", x) for k in range(2)]
        for what, x in (("Inf", inf), ("NaN", nan)):
            p.compare(what, "plain", x)
            p.compare(what + " again", "plain", x)
        return out
    out = _with_plan(dev, T, monkeypatch, name, D, body)
    for what, pair in out.items():
        assert [w for w, _ in pair] == ["miss", "hit"], (what, pair)
        assert pair[0][1] == pair[1][1], (what, pair)
    # (the bound of the binary SpMM: 2^40 with many lost elements is wide; 2^15 with one lost element is not)
    assert out["one 1e12"][0][1][0] == 1 and out["one 1e-5"][0][1][0] == 0, out


@pytest.mark.parametrize("name,D", CASES, ids=IDS)
def test_a_poisoned_guess_costs_a_miss_and_nothing_else(dev, T, monkeypatch, name, D):
    X = _data(dev, name, D)[0]
    big = X.clone(); big[0, 0] = 3e38                                 # exponent 127: the guess becomes 14 - 127 = -113

    def body(p):
        return [p.compare(what, "plain", x)[0] for what, x in (("max 3e38", big), ("O(1) after 3e38", X), ("O(1) again", X))]
    went = _with_plan(dev, T, monkeypatch, name, D, body)
    assert went == ["miss", "miss", "hit"], went
