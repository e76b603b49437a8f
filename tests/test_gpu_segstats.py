"""The one-gather aggregation on the MI355X: tcgnn_segment_stats / _backward on rows of every length class at every width class, every
nullable form, the dword form, the boundary-shaped graphs and degenerate sizes, the shipped tcgnn_segment_max as a cross-check, the
pybind module against the ctypes one, aggregate_stats and PNAConv against the dense fp64 model, and a captured training step.  The
restatements, input sets and bounds are tests/stats_ref.py's; the row-length graph and the buffer helpers tests/test_gpu_segmax.py's.
Extrema and args are held to the reference BIT FOR BIT; mean and std to the helper's per-element bounds; the backward to `torch.equal`
where the sums are exact (integer operands) and to the summation bound k 2^-24 sum|terms| otherwise."""
import numpy as np
import pytest
import torch

import graphs
import stats_ref as R
import test_gpu_segmax as M

pytestmark = pytest.mark.gpu

GUARD, NO_ROW, SENTINEL, N_ROWS, INVALID_ARG = M.GUARD, M.NO_ROW, M.SENTINEL, M.N_ROWS, M.INVALID_ARG
WIDTHS = (1, 3, 4, 41, 64, 65, 256, 260)
VALUES, ARGS = ("mean", "std", "max", "min"), ("argmax", "argmin")
ORDER = ("mean", "std", "max", "argmax", "min", "argmin")       # the C entry's output arguments


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def T():
    import TCGNN
    return TCGNN


ext = M.ext
_dev = M._dev


def _inputs(which, n, D, plant_row=None):
    """the set's X; on `ties` and `normal` the planted node holds +50 in the even columns (it has to win the maximum there) and -50 in
    the odd ones (the minimum)"""
    X = R.input_set(which, n, D, seed=D)
    if plant_row is not None and which in ("ties", "normal"):
        X[plant_row, 0::2] = 50.0
        X[plant_row, 1::2] = -50.0
    return X


_REF = {}   # (graph key, set, D) -> stats_ref.segment_stats: computed once, shared, never changed


def _ref(key, rp, col, X):
    if key not in _REF:
        _REF[key] = R.segment_stats(rp, col, X)
    return _REF[key]


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _c_forward(dev, trp, tcol, n, E, tX, D, names, eps=1e-5):
    """one C call with the outputs in `names` given (the others null) -> {name: (guarded buffer, view)}"""
    import tcgnn_capi as C
    out = {k: M._guarded(dev, n * D, torch.int32 if k in ARGS else torch.float32) for k in names}
    st = C.lib.tcgnn_segment_stats(trp.data_ptr(), tcol.data_ptr(), n, E, tX.data_ptr(), D, eps, *[out[k][1].data_ptr() if k in out else None for k in ORDER],
                                   torch.cuda.current_stream().cuda_stream)
    assert st == 0, C.lib.tcgnn_last_error()
    return out


def _forward_case(dev, T, key, rp, col, X, what, ext=None, moments=True):
    """one graph, one X: the full C call (moments null with moments=False) into guarded buffers, twice, against the reference; the two
    modules against it -> (failures, {name: [n, D] device tensor})"""
    bad = []
    rp = np.ascontiguousarray(rp, dtype=np.int32)
    n, E, D = len(rp) - 1, int(rp[-1]), X.shape[1]
    colp = np.zeros(E + NO_ROW, dtype=np.int32)
    colp[:E] = col[:E]
    trp, tcol, tX = _dev(dev, rp), _dev(dev, colp), _dev(dev, X)
    r = _ref(key, rp, col, X)
    names = [k for k in ORDER if moments or k not in ("mean", "std")]
    first, second = (_c_forward(dev, trp, tcol, n, E + NO_ROW, tX, D, names) for _ in range(2))
    got = {k: first[k][0][:n * D].view(n, D) for k in names}
    for k in names:
        if not torch.equal(_bits(first[k][0]), _bits(second[k][0])):
            bad.append("%s: %s: the second call returns other bits" % (what, k))
        if not bool((first[k][0][n * D:] == SENTINEL).all()):
            bad.append("%s: %s: guard words written" % (what, k))
    for k in ("max", "min", "argmax", "argmin"):
        want = torch.from_numpy(r[k].view(np.int32))
        if not torch.equal(_bits(got[k]).cpu(), want):
            bad.append("%s: %s differs from the reference in %d elements" % (what, k, int((_bits(got[k]).cpu() != want).sum())))
    empty = torch.from_numpy(r["k"] == 0).to(dev)
    for k in names:
        if bool((_bits(got[k])[empty] != (-1 if k in ARGS else 0)).any()):
            bad.append("%s: %s of a row without edges is not %s" % (what, k, "-1" if k in ARGS else "+0"))
    if moments:
        for k in ("mean", "std"):
            err = np.abs(got[k].cpu().numpy().astype(np.float64) - r[k])
            bound = r[k + "_bound"]
            has = bound > 0
            share = float((err[has] / bound[has]).max()) if has.any() else 0.0
            print("FIG segstats %-4s %-40s largest error %.3f of the bound" % (k, what, share))
            if not (err <= bound).all():
                bad.append("%s: %s beyond the bound in %d elements (largest %.3f of it)" % (what, k, int((err > bound).sum()), share))
        asked = VALUES
    else:
        asked = ("max", "min")
    # the modules' calls (edgeList as long as the rows cover)
    for mod, label in ((T, "TCGNN"), (ext, "the pybind module")):
        if mod is None:
            continue
        res = mod.forward_stats(tX, trp, tcol[:E].contiguous(), aggregators=asked)
        if sorted(res) != sorted(names) or not all(torch.equal(_bits(res[k]), _bits(got[k])) for k in names):
            bad.append("%s: %s.forward_stats differs from the C call" % (what, label))
    torch.cuda.synchronize()
    return bad, got


# ---- forward ---------------------------------------------------------------------------------------------------------------------------

WIDTH_CASES = [(D, s) for D in WIDTHS for s in ("ties", "normal", "offset", "constant")] + [(D, s) for D in (3, 64, 260) for s in ("signed_zero", "specials")]


@pytest.mark.parametrize("D,which", WIDTH_CASES, ids=["D%d-%s" % c for c in WIDTH_CASES])
def test_forward_on_rows_of_every_length_class_at_every_width(dev, T, ext, D, which):
    G = M.group_lanes(D)
    rp, col, planted = M.row_length_graph(G)
    X = _inputs(which, N_ROWS, D, plant_row=N_ROWS - 1)
    what = "row lengths G=%d D=%d %s" % (G, D, which)
    bad, got = _forward_case(dev, T, ("rows", G, which, D), rp, col, X, what, ext, moments=which != "specials")
    if which in ("ties", "normal"):
        amax, amin = got["argmax"].cpu().numpy(), got["argmin"].cpu().numpy()
        for r, pos in planted:
            if not ((amax[r, 0::2] == pos).all() and (amin[r, 1::2] == pos).all()):
                bad.append("row %d (%d edges): the planted position %d did not win" % (r, rp[r + 1] - rp[r], pos - rp[r]))
    if which == "constant":
        std = got["std"][torch.from_numpy(np.diff(rp) > 0).to(dev)].cpu().numpy().astype(np.float64)
        if not (np.abs(std - np.sqrt(1e-5)) <= 2.0 ** -23 * np.sqrt(1e-5) * 1.0001).all():       # (the bound with var = 0)
            bad.append("constant columns: std is not fp32(sqrt(eps))")
    assert not bad, "\n  ".join(bad)


@pytest.mark.parametrize("which", ["ties", "normal"])
def test_extrema_equal_the_shipped_segment_max(dev, T, which):
    D = 64
    rp, col, _ = M.row_length_graph(M.group_lanes(D))
    X = _inputs(which, N_ROWS, D, plant_row=N_ROWS - 1)
    trp, tcol, tX = _dev(dev, rp), _dev(dev, col), _dev(dev, X)
    res = T.forward_stats(tX, trp, tcol, aggregators=("max", "min"))
    Y, arg = T.forward_max(tX, trp, tcol)
    assert torch.equal(_bits(res["max"]), _bits(Y)) and torch.equal(res["argmax"], arg)
    Yn, argn = T.forward_max(-tX, trp, tcol)
    assert torch.equal(res["argmin"], argn)
    if which == "normal":                                     # (no zeros on rows with edges: the negation keeps every bit but the sign)
        assert torch.equal(_bits(-res["min"])[argn >= 0], _bits(Yn)[argn >= 0])
    T.clear_plan_cache()


FORMS = [("mean", "std"), ("max", "argmax", "min", "argmin"), ("mean", "std", "max", "min"), ("mean",), ("std",), ("max",), ("min",), ("min", "argmin"),
         ("std", "max", "argmax")]


@pytest.mark.parametrize("D", [41, 64])
def test_each_nullable_form_writes_what_the_full_call_writes(dev, D):
    rp, col, _ = M.row_length_graph(M.group_lanes(D))
    n, E = len(rp) - 1, int(rp[-1])
    trp, tcol, tX = _dev(dev, rp), _dev(dev, col), _dev(dev, _inputs("normal", N_ROWS, D, plant_row=N_ROWS - 1))
    full = _c_forward(dev, trp, tcol, n, E, tX, D, ORDER)
    for names in FORMS:
        part = _c_forward(dev, trp, tcol, n, E, tX, D, names)
        for k in names:
            assert torch.equal(_bits(part[k][0]), _bits(full[k][0])), (names, k)


def test_rows_off_sixteen_bytes_take_the_dword_form_and_give_the_same_bits(dev, T):
    D = 64
    rp, col, _ = M.row_length_graph(M.group_lanes(D))
    n = len(rp) - 1
    trp, tcol = _dev(dev, rp), _dev(dev, col)
    for which in ("normal", "specials"):
        tX = _dev(dev, _inputs(which, N_ROWS, D, plant_row=N_ROWS - 1))
        storage = torch.zeros(n * D + 1, dtype=torch.float32, device=dev)
        Xo = storage[1:].view(n, D)
        Xo.copy_(tX)
        assert Xo.data_ptr() % 16 == 4
        a, b = T.forward_stats(tX, trp, tcol), T.forward_stats(Xo, trp, tcol)
        assert all(torch.equal(_bits(a[k]), _bits(b[k])) for k in ORDER)
    T.clear_plan_cache()


# ---- backward --------------------------------------------------------------------------------------------------------------------------

GROUPS = (("a",), ("b",), ("max",), ("min",), ("a", "b", "max", "min"))


def _backward_case(dev, T, ext, key, rp, col, got, what, off16=False):
    """the C call over the host's transposed CSR into guarded buffers, twice: every group alone and all together, integer operands
    exactly and random ones within the summation bound; then the two modules (their own device transpose, a and b formed from the
    gradients of mean and std by the documented fp32 operations) bit-equal to the C call"""
    import tcgnn_capi as C
    bad = []
    rp = np.ascontiguousarray(rp, dtype=np.int32)
    n, E = len(rp) - 1, int(rp[-1])
    D = got["argmax"].shape[1]
    rp_t, col_t, perm = M._transposed(key, rp, col)
    pad = lambda a: np.concatenate([a[:E], np.zeros(NO_ROW, np.int32)])   # noqa: E731
    trp_t, tcol_t, tperm = _dev(dev, rp_t), _dev(dev, pad(col_t)), _dev(dev, pad(perm))
    stream = torch.cuda.current_stream().cuda_stream
    argh = {k: got[k].cpu().numpy() for k in ARGS}
    rng = np.random.default_rng(n + D)

    def place(a):       # on the device; with off16 at an address 4 bytes past a 16-byte boundary
        t = _dev(dev, a)
        if not off16:
            return t
        store = torch.zeros(t.numel() + 1, dtype=t.dtype, device=dev)
        store[1:].copy_(t.reshape(-1))
        assert store[1:].data_ptr() % 16 == 4
        return store[1:].view(t.shape)

    for kind in ("integer", "random"):
        draw = (lambda: rng.integers(-8, 9, (n, D)).astype(np.float32)) if kind == "integer" else (lambda: rng.standard_normal((n, D)).astype(np.float32))
        h = {k: draw() for k in ("Z", "a", "b", "dmax", "dmin")}
        t = {k: place(v) for k, v in h.items()}
        targ = {k: place(v) for k, v in argh.items()}
        for groups in GROUPS:
            dZ64, k, sabs = R.segment_stats_backward(rp, col, h["Z"], h["a"] if "a" in groups else None, h["b"] if "b" in groups else None,
                                                     argh["argmax"] if "max" in groups else None, h["dmax"], argh["argmin"] if "min" in groups else None, h["dmin"])
            p = lambda name, on: t[name].data_ptr() if on else None   # noqa: E731
            outs = []
            for _ in range(2):
                buf, view = M._guarded(dev, n * D, torch.float32)
                st = C.lib.tcgnn_segment_stats_backward(trp_t.data_ptr(), tcol_t.data_ptr(), tperm.data_ptr(), n, E + NO_ROW, p("Z", "b" in groups),
                                                        p("a", "a" in groups), p("b", "b" in groups), targ["argmax"].data_ptr() if "max" in groups else None,
                                                        p("dmax", "max" in groups), targ["argmin"].data_ptr() if "min" in groups else None,
                                                        p("dmin", "min" in groups), D, view.data_ptr(), stream)
                assert st == 0, C.lib.tcgnn_last_error()
                outs.append(buf)
            tag = "%s: %s %s" % (what, "+".join(groups), kind)
            res = outs[0][:n * D].view(n, D)
            if bool((res == SENTINEL).any()):
                bad.append("%s: %d elements of dZ unwritten" % (tag, int((res == SENTINEL).sum())))
            if not bool((outs[0][n * D:] == SENTINEL).all()):
                bad.append("%s: guard words written" % tag)
            if not torch.equal(outs[0], outs[1]):
                bad.append("%s: the second call returns other bits" % tag)
            gh = res.cpu().numpy().astype(np.float64)
            if kind == "integer":
                if not np.array_equal(gh, dZ64):
                    bad.append("%s: dZ differs from the exact sums in %d elements" % (tag, int((gh != dZ64).sum())))
            else:
                bound = k * 2.0 ** -24 * sabs
                share = float(np.max(np.abs(gh - dZ64) / np.maximum(bound, 1e-300))) if E else 0.0
                if len(groups) == 4:
                    print("FIG segstats backward %-40s largest |dZ - dZ64| = %.3f of k 2^-24 sum|terms|, most terms %d" % (what, share, int(k.max()) if k.size else 0))
                if (np.abs(gh - dZ64) > bound).any():
                    bad.append("%s: %d elements beyond k 2^-24 sum|terms|" % (tag, int((np.abs(gh - dZ64) > bound).sum())))
    # the modules: a and b from the gradients, as TCGNN.backward_stats documents them
    if not off16:
        trp, tcol = _dev(dev, rp), _dev(dev, col[:E])
        grads = {a: _dev(dev, rng.standard_normal((n, D)).astype(np.float32)) for a in VALUES}
        saved = dict(got, Z=t["Z"])
        has = (trp[1:] > trp[:-1]).unsqueeze(1)
        inv_k = has.float() / (trp[1:] - trp[:-1]).clamp(min=1).float().unsqueeze(1)
        b = (grads["std"] * inv_k) / torch.where(has, got["std"], 1.0)
        a = grads["mean"] * inv_k - b * got["mean"]
        buf, view = M._guarded(dev, n * D, torch.float32)
        st = C.lib.tcgnn_segment_stats_backward(trp_t.data_ptr(), tcol_t.data_ptr(), tperm.data_ptr(), n, E, t["Z"].data_ptr(), a.data_ptr(), b.data_ptr(),
                                                got["argmax"].data_ptr(), grads["max"].data_ptr(), got["argmin"].data_ptr(), grads["min"].data_ptr(), D,
                                                view.data_ptr(), stream)
        assert st == 0, C.lib.tcgnn_last_error()
        for mod, label in ((T, "TCGNN"), (ext, "the pybind module")):
            if mod is not None and not torch.equal(mod.backward_stats(grads, saved, trp, tcol), view.view(n, D)):
                bad.append("%s: %s.backward_stats differs from the C call" % (what, label))
            if mod is not None:
                only = mod.backward_stats({"max": grads["max"], "mean": None}, saved, trp, tcol)
                if not torch.equal(only, mod.backward_max(grads["max"], got["argmax"], trp, tcol)):
                    bad.append("%s: %s.backward_stats of the maximum alone differs from backward_max" % (what, label))
    torch.cuda.synchronize()
    return bad


@pytest.mark.parametrize("name", list(M.STRUCTURES))
def test_forward_and_backward_on_structured_graphs(dev, T, ext, name):
    rp, col = M.STRUCTURES[name]
    n = len(rp) - 1
    bad = []
    for D, which in ((41, "ties"), (64, "normal")):
        X = _inputs(which, n, D)
        what = "%s D=%d %s" % (name, D, which)
        b, got = _forward_case(dev, T, (name, which, D), rp, col, X, what, ext)
        bad += b + _backward_case(dev, T, ext, name, rp, col, got, what)
    assert not bad, "\n  ".join(bad)
    T.clear_plan_cache()
    ext.clear_plan_cache()


def test_backward_of_the_ties_forward_on_the_hub_graph_where_thousands_choose_one_source(dev, T, ext):
    rp, col = M.STRUCTURES["hub_rows_n2500"]
    n = len(rp) - 1
    bad = []
    for D in (3, 64):
        X = _inputs("ties", n, D)
        b, got = _forward_case(dev, T, ("hub_rows_n2500", "ties", D), rp, col, X, "hub rows D=%d ties" % D)
        _, k, _ = R.segment_stats_backward(rp, col, argmax=got["argmax"].cpu().numpy(), dmax=np.ones((n, D), np.float32))
        assert int(k.max()) >= 1000, "no source was chosen a thousand times: the case does not test what it is for"
        bad += b + _backward_case(dev, T, ext, "hub_rows_n2500", rp, col, got, "hub rows D=%d ties" % D)
    assert not bad, "\n  ".join(bad)
    T.clear_plan_cache()
    ext.clear_plan_cache()


@pytest.mark.parametrize("D", [64, 260])
def test_backward_with_every_gathered_array_off_sixteen_bytes(dev, T, ext, D):
    """(D = 260: two column blocks, aligned and not)"""
    name = "directed_n500"
    rp, col = M.STRUCTURES[name]
    X = _inputs("ties", len(rp) - 1, D)
    b, got = _forward_case(dev, T, (name, "ties", D), rp, col, X, "directed_n500 D=%d ties" % D)
    bad = b + _backward_case(dev, T, ext, name, rp, col, got, "directed_n500 D=%d ties" % D)
    bad += _backward_case(dev, T, None, name, rp, col, got, "directed_n500 D=%d ties, operands off 16 bytes" % D, off16=True)
    assert not bad, "\n  ".join(bad)
    T.clear_plan_cache()
    ext.clear_plan_cache()


def test_backward_on_the_row_length_graph(dev, T, ext):
    """the transposed rows of the row-length graph: the planted node is named once per listed row, every other node up to a few hundred times"""
    D = 4
    G = M.group_lanes(D)
    rp, col, _ = M.row_length_graph(G)
    X = _inputs("ties", N_ROWS, D, plant_row=N_ROWS - 1)
    b, got = _forward_case(dev, T, ("rows", G, "ties", D), rp, col, X, "row lengths D=4 ties")
    bad = b + _backward_case(dev, T, ext, "rows%d" % G, rp, col, got, "row lengths D=4 ties")
    assert not bad, "\n  ".join(bad)
    T.clear_plan_cache()
    ext.clear_plan_cache()


# ---- degenerate and refused calls ------------------------------------------------------------------------------------------------------

def test_degenerate_sizes_return_ok_and_fill_what_exists(dev, T):
    import tcgnn_capi as C
    stream = torch.cuda.current_stream().cuda_stream
    fwd, bwd = C.lib.tcgnn_segment_stats, C.lib.tcgnn_segment_stats_backward
    n, D = 37, 5
    rp0 = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    X = torch.randn(n, D, device=dev)
    out = {k: M._guarded(dev, n * D, torch.int32 if k in ARGS else torch.float32) for k in ORDER}
    assert fwd(rp0.data_ptr(), None, n, 0, X.data_ptr(), D, 1e-5, *[out[k][1].data_ptr() for k in ORDER], stream) == 0          # E = 0
    for k in ORDER:
        assert bool((_bits(out[k][1]) == (-1 if k in ARGS else 0)).all()) and bool((out[k][0][n * D:] == SENTINEL).all()), k
    part = {k: M._guarded(dev, n * D, torch.int32 if k in ARGS else torch.float32) for k in ("std", "min")}
    assert fwd(rp0.data_ptr(), None, n, 0, X.data_ptr(), D, 1e-5, None, part["std"][1].data_ptr(), None, None, part["min"][1].data_ptr(), None, stream) == 0
    assert not bool(part["std"][1].any()) and not bool(part["min"][1].any())
    xbuf, dz = M._guarded(dev, n * D, torch.float32)
    a = out["argmax"][1]
    assert bwd(rp0.data_ptr(), None, None, n, 0, X.data_ptr(), X.data_ptr(), X.data_ptr(), a.data_ptr(), X.data_ptr(), a.data_ptr(), X.data_ptr(), D, dz.data_ptr(),
               stream) == 0
    assert bool((dz.view(torch.int32) == 0).all()) and bool((xbuf[n * D:] == SENTINEL).all())
    for nn, ee, dd in ((0, 0, D), (0, 5, D), (n, 7, 0)):                                                       # N = 0, D = 0: nothing to write
        small = {k: M._guarded(dev, 8, torch.int32 if k in ARGS else torch.float32) for k in ORDER}
        assert fwd(rp0.data_ptr(), rp0.data_ptr(), nn, ee, X.data_ptr(), dd, 1e-5, *[small[k][1].data_ptr() for k in ORDER], stream) == 0
        assert bwd(rp0.data_ptr(), rp0.data_ptr(), rp0.data_ptr(), nn, ee, X.data_ptr(), X.data_ptr(), X.data_ptr(), a.data_ptr(), X.data_ptr(), a.data_ptr(),
                   X.data_ptr(), dd, small["mean"][1].data_ptr(), stream) == 0
        assert all(bool((small[k][0] == SENTINEL).all()) for k in ORDER)
    # every group null on a graph with edges: dZ is zeroed
    rp, col = graphs.uniform_graph(50, 4, seed=2)
    rp_t, col_t, perm = (np.ascontiguousarray(x, dtype=np.int32) for x in M.W.transposed_csr(rp, col))
    zbuf, dz = M._guarded(dev, 50 * D, torch.float32)
    assert bwd(_dev(dev, rp_t).data_ptr(), _dev(dev, col_t).data_ptr(), _dev(dev, perm).data_ptr(), 50, len(col), *[None] * 7, D, dz.data_ptr(), stream) == 0
    assert bool((dz.view(torch.int32) == 0).all()) and bool((zbuf[50 * D:] == SENTINEL).all())
    # the module's calls at those sizes
    col0 = torch.zeros(0, dtype=torch.int32, device=dev)
    res = T.forward_stats(X, rp0, col0)
    assert all(res[k].shape == (n, D) for k in ORDER) and all(not bool(res[k].any()) for k in VALUES) and bool((res["argmax"] == -1).all())
    assert not bool(T.backward_stats({k: X for k in VALUES}, dict(res, Z=X), rp0, col0).any())
    res = T.forward_stats(torch.zeros(n, 0, device=dev), rp0, col0, aggregators=("std",))
    assert list(res) == ["std"] and res["std"].shape == (n, 0)


def test_invalid_arguments_are_refused_and_nothing_is_written(dev):
    import tcgnn_capi as C
    stream = torch.cuda.current_stream().cuda_stream
    n, E, D = 10, 30, 4
    rp = torch.arange(0, E + 1, 3, dtype=torch.int32, device=dev)
    col = torch.zeros(E, dtype=torch.int32, device=dev)
    X = torch.randn(n, D, device=dev)
    out = {k: M._guarded(dev, n * D, torch.int32 if k in ARGS else torch.float32) for k in ORDER}
    p = lambda t: t.data_ptr()   # noqa: E731
    good = [p(rp), p(col), n, E, p(X), D, 1e-5] + [p(out[k][1]) for k in ORDER]
    for at, value in ((2, -1), (3, -1), (3, 1 << 31), (5, -1), (0, None), (1, None), (4, None), (9, None), (11, None)):   # sizes, inputs, max / min without their arg's value
        args = list(good)
        args[at] = value
        assert C.lib.tcgnn_segment_stats(*args, stream) == INVALID_ARG, (at, value)
    assert C.lib.tcgnn_segment_stats(*good[:7], *[None] * 6, stream) == INVALID_ARG
    dz = out["mean"][1]
    a = out["argmax"][1]
    good = [p(rp), p(col), p(col), n, E, p(X), p(X), p(X), p(a), p(X), p(a), p(X), D, p(dz)]
    for at, value in ((3, -1), (4, -1), (4, 1 << 31), (12, -1), (0, None), (1, None), (2, None), (13, None), (5, None), (7, None), (8, None), (9, None),
                      (10, None), (11, None)):
        args = list(good)
        args[at] = value
        assert C.lib.tcgnn_segment_stats_backward(*args, stream) == INVALID_ARG, (at, value)
    torch.cuda.synchronize()
    assert all(bool((out[k][0] == SENTINEL).all()) for k in ORDER)


def test_module_argument_checks(dev, T, ext):
    rp, col = graphs.uniform_graph(50, 4, seed=2)
    trp, tcol = _dev(dev, rp), _dev(dev, col)
    X = torch.randn(50, 8, device=dev)
    for mod in (T, ext):
        with pytest.raises(RuntimeError, match="num_nodes"):
            mod.forward_stats(X[:49].contiguous(), trp, tcol)
        with pytest.raises(RuntimeError, match="Float"):
            mod.forward_stats(X.double(), trp, tcol)
        with pytest.raises(ValueError, match="aggregators"):
            mod.forward_stats(X, trp, tcol, aggregators=("mean", "median"))
        res = mod.forward_stats(X, trp, tcol, aggregators=("min", "mean"), return_arg=False)
        assert sorted(res) == ["mean", "min"]
        full = mod.forward_stats(X, trp, tcol)
        with pytest.raises(RuntimeError, match="shape and device of Z"):
            mod.backward_stats({"max": X[:, :4].contiguous()}, dict(full, Z=X), trp, tcol)
        with pytest.raises(ValueError, match="grads"):
            mod.backward_stats({"median": X}, dict(full, Z=X), trp, tcol)
        out = torch.empty_like(X)
        assert mod.backward_stats({"mean": X}, dict(full, Z=X), trp, tcol, out=out).data_ptr() == out.data_ptr()
    T.clear_plan_cache()
    ext.clear_plan_cache()


# ---- aggregate_stats and PNAConv against the dense fp64 model --------------------------------------------------------------------------

def test_aggregate_stats_against_the_dense_fp64_model_on_a_directed_graph(dev, T):
    import tcgnn_edge_ops as E
    rp, col, A = M._directed500()
    n, D = len(rp) - 1, 23
    torch.manual_seed(1)
    Z = torch.randn(n, D)
    dY = [torch.randn(n, D, dtype=torch.float64) for _ in VALUES]
    Zg = Z.to(dev).requires_grad_(True)
    got = E.aggregate_stats(Zg, _dev(dev, rp), _dev(dev, col))
    Zd = Z.double().requires_grad_(True)
    eye = torch.eye(D, dtype=torch.float64)
    zero = torch.zeros(D, dtype=torch.float64)
    want = [R.dense_pna(A, Zd, eye, torch.zeros(D, D, dtype=torch.float64), zero, torch.cat([torch.zeros(D, D, dtype=torch.float64), eye]), zero,
                        aggregators=(a,), scalers=("identity",)) for a in VALUES]
    assert torch.equal(got[2].detach().cpu().double(), want[2].detach()) and torch.equal(got[3].detach().cpu().double(), want[3].detach())   # extrema are exact
    figs = [(a, M._rel(g, w), 1e-5) for a, g, w in zip(VALUES, got, want)]
    gz, = torch.autograd.grad(sum((g * d.float().to(dev)).sum() for g, d in zip(got, dY)), Zg)
    rz, = torch.autograd.grad(sum((w * d).sum() for w, d in zip(want, dY)), Zd, retain_graph=True)
    figs.append(("dZ", M._rel(gz, rz), 1e-4))
    for w, f, t in figs:
        print("FIG aggregate_stats %-4s %.3e of the largest entry (bound %.0e)" % (w, f, t))
    assert all(f <= t for _, f, t in figs), figs
    only, = E.aggregate_stats(Zg, _dev(dev, rp), _dev(dev, col), aggregators=("std",))      # std alone: the mean it needs is computed beside it
    assert torch.equal(only, got[1])
    g1, = torch.autograd.grad((only * dY[1].float().to(dev)).sum(), Zg)
    r1, = torch.autograd.grad((want[1] * dY[1]).sum(), Zd)
    assert M._rel(g1, r1) <= 1e-4
    T.clear_plan_cache()


@pytest.mark.parametrize("dims", [(24, 16), (16, 24)], ids=["narrowing", "widening"])
def test_pna_layer_against_the_dense_fp64_model_on_a_directed_graph(dev, T, dims):
    """the bounds of tests/test_segstats_cpu.py: output 1e-5, gradients 1e-4 of the largest entry - the aggregation is fp32-exact or
    better and the dense products are fp32"""
    import tcgnn_layers as L
    rp, col, A = M._directed500()
    n = len(rp) - 1
    meta = M._meta(dev, rp, col)
    torch.manual_seed(3)
    conv = L.PNAConv(*dims)
    conv.bias_pre.data.normal_()
    conv.bias_post.data.normal_()
    names = ["weights_src", "weights_dst", "bias_pre", "weights_post", "bias_post"]
    X = torch.randn(n, dims[0])
    dY = torch.randn(n, dims[1], dtype=torch.float64)
    leaves = [X.double().requires_grad_(True)] + [getattr(conv, k).detach().double().requires_grad_(True) for k in names]
    conv = conv.to(dev)
    params = [getattr(conv, k) for k in names]
    Xg = X.to(dev).requires_grad_(True)
    Y = conv(Xg, *meta)
    want = R.dense_pna(A, *leaves)
    got = torch.autograd.grad((Y * dY.float().to(dev)).sum(), [Xg] + params)
    ref = torch.autograd.grad((want * dY).sum(), leaves)
    figs = [("Y", M._rel(Y, want), R.LAYER_TOL_Y)] + [(w, M._rel(g, r), R.LAYER_TOL_G) for g, r, w in zip(got, ref, ["dX"] + ["d" + k for k in names])]
    for w, f, t in figs:
        print("FIG pna %-9s %-13s %.3e of the largest entry (bound %.0e)" % ("%d->%d" % dims, w, f, t))
    assert all(f <= t for _, f, t in figs), figs
    T.clear_plan_cache()


def test_a_prepared_pna_step_replays_from_a_hip_graph_bit_equal(dev, T):
    import tcgnn_layers as L
    rp, col = graphs.community_graph(3000, 10, 20, 0.8, seed=4)
    n = len(rp) - 1
    meta = M._meta(dev, rp, col)
    torch.manual_seed(2)
    convs = [L.PNAConv(32, 16).to(dev), L.PNAConv(16, 6).to(dev)]
    params = [p for cv in convs for p in cv.parameters()]
    x = torch.randn(n, 32, device=dev).requires_grad_(True)
    y = torch.randint(0, 6, (n,), device=dev)
    T.prepare([], *meta, max_aggregation=True)

    def step():
        out = convs[1](torch.relu(convs[0](x, *meta)), *meta)
        return torch.autograd.grad(torch.nn.functional.cross_entropy(out, y), [x] + params)

    eager = [g.clone() for g in step()]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")      # a prepared step never synchronises
    try:
        g = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert all(torch.equal(a, b) for a, b in zip(g, eager))
    del g
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                # allocator warm-up on the side stream, as capture requires
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):   # one stream, no parallel branches
        static = step()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(static, eager):
        assert torch.equal(a, b), tuple(a.shape)
    del graph, static
    T.clear_plan_cache()
