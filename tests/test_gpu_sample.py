"""Seeded neighbour sampling on the MI355X: tcgnn_sample_neighbors_count / tcgnn_sample_neighbors on rows of every length class at
every fan-out class against tests/sample_ref.py's numpy restatement (EVERY element of the three outputs, torch.equal), the
structural properties checked without the reference, the tie that only the low half of the word decides, masks, the memory
contract and the refusals, degenerate sizes, repetition, the pybind module against the ctypes one, the existing operators on a
sampled graph, a sampled training step, the plan cache over resampled epochs, and the harness's --fanout."""
import glob
import importlib.util
import os

import numpy as np
import pytest
import torch

import edge_message_ref as EM
import sample_ref as R
import segmax_ref as SM
import stats_ref as ST

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
SENTINEL = -12345
FANOUTS = (0, 1, 2, 5, 25, 64, 1000, 5000, 100000)
SEEDS = (0, 1, 2 ** 63 + 5)
BAD_GRAPH, WORKSPACE = 4, 5   # TCGNN_ERR_BAD_GRAPH, TCGNN_ERR_WORKSPACE (include/tcgnn.h)


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


def _dev(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


_REF = {}   # (graph, k, seed, mask) -> the reference, computed once, shared, never changed


def _ref(key, rp, col, k, seed, mask=None):
    if key not in _REF:
        _REF[key] = R.sample_neighbors(rp, col, k, seed, mask)
    return _REF[key]


def _structure(rp, col, k, mask, got):
    """the properties that need no reference"""
    rp_s, col_s, eid = (t.cpu().numpy() for t in got)
    d = np.diff(rp.astype(np.int64))
    want = np.minimum(d, d.max() + 1 if k is None else k) * (1 if mask is None else (np.asarray(mask) != 0))
    assert rp_s[0] == 0 and np.array_equal(np.diff(rp_s), want), "row counts are not min(d, k) * mask"
    assert len(eid) == rp_s[-1] == len(col_s)
    assert np.all(np.diff(eid.astype(np.int64)) > 0), "eid is not strictly increasing"
    assert np.array_equal(col_s, col[eid]), "edgeList_s is not edgeList[eid]"
    rows = np.repeat(np.arange(len(d)), np.diff(rp_s))
    assert np.all((eid >= rp[rows]) & (eid < rp[rows + 1])), "a kept edge lies outside its row"


def _equal(got, want, what):
    for g, w, n in zip(got, want, ("nodePointer_s", "edgeList_s", "eid")):
        assert g.dtype == torch.int32 and torch.equal(g.cpu(), torch.from_numpy(w)), "%s: %s differs from the reference" % (what, n)


# ---- rows of every length class ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS, ids=["seed%d" % s for s in SEEDS])
@pytest.mark.parametrize("k", FANOUTS, ids=["k%d" % k for k in FANOUTS])
def test_rows_of_every_length_class_equal_the_reference(dev, T, k, seed):
    rp, col, _ = R.row_length_graph()
    E = int(rp[-1])
    trp, tcol = _dev(dev, rp), _dev(dev, col)
    # the module's call takes the covered part; the C call below it sees the NO_ROW out-of-range ids behind nodePointer[N]
    got = T.sample_neighbors(trp, tcol[:E].contiguous(), k, seed)
    _structure(rp, col, k, None, got)
    _equal(got, _ref(("rows", k, seed), rp, col, k, seed), "k = %d, seed = %d" % (k, seed))
    raw = _raw_call(dev, trp, tcol, None, len(rp) - 1, len(col), k, seed, expect=0, n_out=int(got[0][-1]), num_edges_arg=E)
    _equal(raw, [g.cpu().numpy() for g in got], "the C call with uncovered entries behind the rows")


def test_no_fanout_and_a_fanout_beyond_the_largest_degree_copy_the_graph(dev, T):
    rp, col, _ = R.row_length_graph()
    E = int(rp[-1])
    trp, tcol = _dev(dev, rp), _dev(dev, col[:E])
    for k in (None, R.LONG_ROW, 2 ** 40):
        rp_s, col_s, eid = T.sample_neighbors(trp, tcol, k, 7)
        assert torch.equal(rp_s, trp) and torch.equal(col_s, tcol) and torch.equal(eid.cpu(), torch.arange(E, dtype=torch.int32))
        assert col_s.data_ptr() != tcol.data_ptr()


def test_the_low_half_of_the_word_decides_between_two_equal_hashes(dev, T):
    rp, col, long_row = R.row_length_graph()
    found = R.equal_hash_pair(rp, long_row)
    assert found is not None, "no seed in 0..15 gives the 70 000-edge row two equal hashes"
    seed, k = found
    lo, hi = int(rp[long_row]), int(rp[long_row + 1])
    w = np.sort(R.words(seed, np.arange(lo, hi)))
    assert (w[k - 1] >> np.uint64(32)) == (w[k] >> np.uint64(32)), "the pair does not straddle k"
    E = int(rp[-1])
    got = T.sample_neighbors(_dev(dev, rp), _dev(dev, col[:E]), k, seed)
    want = _ref(("rows", k, seed), rp, col, k, seed)
    _equal(got, want, "k = %d, seed = %d" % (k, seed))
    eid = got[2].cpu().numpy()
    assert int(w[k - 1] & np.uint64(0xFFFFFFFF)) in eid and int(w[k] & np.uint64(0xFFFFFFFF)) not in eid


# ---- masks -------------------------------------------------------------------------------------------------------------------------

def test_masks(dev, T):
    rp, col, _ = R.row_length_graph()
    n, E = len(rp) - 1, int(rp[-1])
    trp, tcol = _dev(dev, rp), _dev(dev, col[:E])
    k, seed = 25, 4
    plain = T.sample_neighbors(trp, tcol, k, seed)
    ones = T.sample_neighbors(trp, tcol, k, seed, torch.ones(n, dtype=torch.uint8, device=dev))
    assert all(torch.equal(a, b) for a, b in zip(plain, ones))
    zeros = T.sample_neighbors(trp, tcol, k, seed, torch.zeros(n, dtype=torch.uint8, device=dev))
    assert zeros[1].numel() == 0 and zeros[2].numel() == 0 and not bool(zeros[0].any())
    mask = (np.random.default_rng(5).random(n) < 0.5).astype(np.uint8)
    mask[np.argmax(np.diff(rp))] = 1
    for kk in (25, 5000):
        got8 = T.sample_neighbors(trp, tcol, kk, seed, _dev(dev, mask))
        gotb = T.sample_neighbors(trp, tcol, kk, seed, _dev(dev, mask.astype(bool)))
        _structure(rp, col, kk, mask, got8)
        _equal(got8, _ref(("rows-mask", kk, seed), rp, col, kk, seed, mask), "random mask, k = %d" % kk)
        assert all(torch.equal(a, b) for a, b in zip(got8, gotb)), "a bool mask and a uint8 mask disagree"
    with pytest.raises(RuntimeError):
        T.sample_neighbors(trp, tcol, k, seed, torch.ones(n - 1, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError):
        T.sample_neighbors(trp, tcol, k, seed, torch.ones(n, dtype=torch.int32, device=dev))


# ---- memory contract ---------------------------------------------------------------------------------------------------------------

def _guarded(dev, n):
    buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    return buf, buf[:n]


def _raw_call(dev, trp, tcol, tmask, n, col_len, k, seed, expect, n_out=None, num_edges_arg=None, ws_shift=0, ws_short=0):
    """the two C calls on guarded outputs, a workspace of exactly the queried size and outputs of exactly E' entries.
    expect: the count call's status.  -> (rp_s, col_s, eid) on success"""
    import tcgnn_capi as C
    stream = torch.cuda.current_stream().cuda_stream
    E = col_len if num_edges_arg is None else num_edges_arg
    need = C._sz(0)
    assert C.lib.tcgnn_sample_workspace_bytes(n, C.ctypes.byref(need)) == 0
    ws = torch.empty(need.value + 512, dtype=torch.uint8, device=dev)
    base = ws.data_ptr() + (-ws.data_ptr()) % 256
    pbuf, p = _guarded(dev, n + 1)
    kept = C._i64(-7)
    st = C.lib.tcgnn_sample_neighbors_count(trp.data_ptr(), tmask.data_ptr() if tmask is not None else None, n, E, k, p.data_ptr(), base + ws_shift,
                                            need.value - ws_short, C.ctypes.byref(kept), stream)
    torch.cuda.synchronize()
    assert st == expect, (st, C.lib.tcgnn_last_error())
    assert bool((pbuf[n + 1:] == SENTINEL).all()), "the count call wrote behind nodePointer_s"
    if st != 0:
        assert kept.value == -7
        return pbuf
    if n_out is not None:
        assert kept.value == n_out
    cbuf, c = _guarded(dev, kept.value)
    ebuf, e = _guarded(dev, kept.value)
    st = C.lib.tcgnn_sample_neighbors(trp.data_ptr(), tcol.data_ptr(), tmask.data_ptr() if tmask is not None else None, p.data_ptr(), n, E, k,
                                      seed % (1 << 64), c.data_ptr(), e.data_ptr(), stream)
    torch.cuda.synchronize()
    assert st == 0, C.lib.tcgnn_last_error()
    assert bool((cbuf[kept.value:] == SENTINEL).all()) and bool((ebuf[kept.value:] == SENTINEL).all()), "guard words written"
    assert not bool((e == SENTINEL).any()), "an entry of eid was not written"
    return p, c, e


def test_workspaces_that_are_too_small_or_misaligned_are_refused(dev):
    rp, col, _ = R.row_length_graph()
    n = len(rp) - 1
    trp, tcol = _dev(dev, rp), _dev(dev, col)
    ws_err = WORKSPACE
    for kw in ({"ws_short": 1}, {"ws_shift": 4}, {"ws_shift": 128}):
        out = _raw_call(dev, trp, tcol, None, n, len(col), 5, 0, expect=ws_err, num_edges_arg=int(rp[-1]), **kw)
        assert bool((out == SENTINEL).all()), "a refused call wrote nodePointer_s"


def test_bad_row_pointers_are_reported_and_nothing_is_written_out_of_bounds(dev):
    rp, col, _ = R.row_length_graph()
    n, E = len(rp) - 1, int(rp[-1])
    bad_graph = BAD_GRAPH
    tcol = _dev(dev, col)
    shifted = rp.copy()
    shifted[0] = 1
    descending = rp.copy()
    i = int(np.argmax(np.diff(rp)))
    descending[i], descending[i + 1] = descending[i + 1], descending[i]
    wild = rp.copy()
    wild[5], wild[6] = -(2 ** 31), 2 ** 31 - 1   # (monotone no more, and far outside [0, E])
    short = rp.copy()
    short[-1] -= 1
    for name, p in (("nodePointer[0] = 1", shifted), ("a descending pair", descending), ("pointers outside [0, E]", wild), ("nodePointer[N] != E", short)):
        _raw_call(dev, _dev(dev, p), tcol, None, n, len(col), 25, 3, expect=bad_graph, num_edges_arg=E)


def test_degenerate_sizes(dev, T):
    e = torch.zeros(0, dtype=torch.int32, device=dev)
    rp_s, col_s, eid = T.sample_neighbors(torch.zeros(1, dtype=torch.int32, device=dev), e, 5, 1)             # N = 0
    assert rp_s.tolist() == [0] and col_s.numel() == 0 and eid.numel() == 0
    rp_s, col_s, eid = T.sample_neighbors(torch.zeros(6, dtype=torch.int32, device=dev), e, 5, 1)             # E = 0
    assert rp_s.tolist() == [0] * 6 and col_s.numel() == 0 and eid.numel() == 0
    loop = (torch.tensor([0, 1], dtype=torch.int32, device=dev), torch.tensor([0], dtype=torch.int32, device=dev))
    for k, kept in ((0, 0), (1, 1), (3, 1), (None, 1)):
        rp_s, col_s, eid = T.sample_neighbors(*loop, k, 9)
        assert rp_s.tolist() == [0, kept] and col_s.tolist() == [0] * kept and eid.tolist() == [0] * kept
    _raw_call(dev, loop[0], loop[1], None, 1, 1, 1, 0, expect=0, n_out=1)
    with pytest.raises(ValueError):
        T.sample_neighbors(*loop, -1, 0)


def test_ten_repetitions_are_bit_identical_and_the_pybind_module_equals_the_ctypes_one(dev, T, ext):
    rp, col, _ = R.row_length_graph()
    E = int(rp[-1])
    trp, tcol = _dev(dev, rp), _dev(dev, col[:E])
    mask = _dev(dev, (np.random.default_rng(8).random(len(rp) - 1) < 0.7).astype(np.uint8))
    first = T.sample_neighbors(trp, tcol, 25, 2 ** 63 + 5, mask)
    for _ in range(9):
        again = T.sample_neighbors(trp, tcol, 25, 2 ** 63 + 5, mask)
        assert all(torch.equal(a, b) for a, b in zip(first, again))
    for k, seed, m in ((25, 2 ** 63 + 5, mask), (5000, 1, None), (None, 0, None), (0, 3, mask.bool())):
        a = T.sample_neighbors(trp, tcol, k, seed, m)
        b = ext.sample_neighbors(trp, tcol, k, seed, m)
        assert all(torch.equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b)), "the pybind module differs at k = %r" % (k,)


# ---- the existing operators on a sampled graph -------------------------------------------------------------------------------------

_POWER = []


def _power_law():
    """an R-MAT graph of 2 048 nodes (tcgnn_graph.rmat_csr), its k = 8 sample by the reference, features"""
    if not _POWER:
        import tcgnn_graph as G
        rp, col = (t.numpy().astype(np.int32) for t in G.rmat_csr(2048, 40000, seed=3, device="cpu")[:2])
        rp_s, col_s, eid = R.sample_neighbors(rp, col, 8, 11)
        rng = np.random.default_rng(0)
        X = rng.integers(-8, 9, (len(rp) - 1, 64)).astype(np.float32)       # (small integers: sums are exact in fp32 and in fp16 staging)
        Ef = rng.integers(-8, 9, (len(col), 64)).astype(np.float32)
        _POWER.append((rp, col, rp_s, col_s, eid, X, Ef))
    return _POWER[0]


def test_existing_operators_on_the_sampled_power_law_graph(dev, T):
    import graphs
    import tcgnn_layers as L
    from oracle import oracle as O
    rp, col, rp_s, col_s, eid, X, Ef = _power_law()
    assert np.diff(rp).max() > 100 and np.diff(rp_s).max() == 8
    trp, tcol, tX, tEf = _dev(dev, rp), _dev(dev, col), _dev(dev, X), _dev(dev, Ef)
    meta_s, teid = L.sample_meta((trp, tcol), 8, 11, plan=True)
    _equal((meta_s[0], meta_s[1], teid), (rp_s, col_s, eid), "sample_meta")
    bare, _ = L.sample_meta((trp, tcol), 8, 11, plan=False)
    assert torch.equal(bare[0], meta_s[0]) and torch.equal(bare[1], meta_s[1]) and all(t.numel() == 0 for t in bare[2:])
    bp, e2c, e2r, _ = graphs.host_sgt(rp_s, col_s)
    assert all(torch.equal(t.cpu(), torch.from_numpy(np.ascontiguousarray(w))) for t, w in zip(meta_s[2:], (bp, e2c, e2r))), "sample_meta's metadata"
    # forward_max: the winner's bits and position
    Y, arg = T.forward_max(tX, meta_s[0], meta_s[1])
    Yr, argr = SM.segment_max(rp_s, col_s, X)
    assert torch.equal(Y.cpu(), torch.from_numpy(Yr)) and torch.equal(arg.cpu(), torch.from_numpy(argr))
    # forward_stats: within the reference's own bounds
    st = T.forward_stats(tX, meta_s[0], meta_s[1])
    sr = ST.segment_stats(rp_s, col_s, X)
    assert torch.equal(st["max"].cpu(), torch.from_numpy(sr["max"])) and torch.equal(st["min"].cpu(), torch.from_numpy(sr["min"]))
    for name in ("mean", "std"):
        err = np.abs(st[name].cpu().numpy().astype(np.float64) - sr[name])
        assert np.all(err <= sr[name + "_bound"]), "%s misses its bound by %.3e" % (name, float((err - sr[name + "_bound"]).max()))
    # forward_ue with the kept edges' features: integer inputs, exact sums
    Yue = T.forward_ue(tX, tEf[teid.long()].contiguous(), meta_s[0], meta_s[1], act="relu")
    Yue_r, S, A = EM.edge_message(rp_s, col_s, X, Ef[eid], "relu")
    assert torch.equal(Yue.cpu(), torch.from_numpy(Yue_r))
    # the plan-based SpMM through sample_meta(plan=True) against the oracle on the reference's sampled CSR
    Ysp = T.forward(tX, *meta_s)[0]
    ref = O.spmm(X, rp_s, col_s, bp, e2c, e2r)
    assert np.max(np.abs(Ysp.cpu().numpy() - ref) / np.maximum(1.0, np.abs(ref))) <= 1e-3


def test_a_sampled_sage_max_step_trains_and_resampled_epochs_stay_within_the_plan_cache(dev, T):
    import tcgnn_layers as L
    rp, col, *_, X, _ = _power_law()
    trp, tcol, tX = _dev(dev, rp), _dev(dev, col), _dev(dev, X)
    torch.manual_seed(0)
    y = torch.randint(0, 4, (len(rp) - 1,), device=dev)
    T.clear_plan_cache()
    T.set_plan_cache_size(3)
    try:
        for agg, plan in (("max", False), ("mean", True)):
            conv = L.SAGEConv(64, 4, aggregator=agg, directed=True).to(dev)
            opt = torch.optim.Adam(conv.parameters(), lr=0.01)
            losses = []
            for epoch in range(8):
                meta_s, _ = L.sample_meta((trp, tcol), 8, 100 + epoch, plan=plan)
                opt.zero_grad()
                loss = torch.nn.functional.cross_entropy(conv(tX, *meta_s), y)
                loss.backward()
                opt.step()
                losses.append(float(loss.detach()))
                s = T.cache_stats()
                assert s["plans"] <= 3 and s["csrs"] <= 6, s
            assert all(np.isfinite(losses)) and all(torch.isfinite(p.grad).all() for p in conv.parameters())
    finally:
        T.set_plan_cache_size(8)
        T.clear_plan_cache()


def test_sample_layers_follows_the_frontier(dev, T):
    import tcgnn_layers as L
    rp, col, *_ = _power_law()
    n = len(rp) - 1
    trp, tcol = _dev(dev, rp), _dev(dev, col)
    seeds = torch.tensor([3, 77, 1500], device=dev)
    g0, g1 = L.sample_layers((trp, tcol), seeds, [6, 4], 21)
    m1 = np.zeros(n, np.uint8)
    m1[[3, 77, 1500]] = 1
    w1 = R.sample_neighbors(rp, col, 4, 21, m1)
    _equal(g1, w1, "the seeds' hop")
    m0 = m1.copy()
    m0[w1[1]] = 1
    _equal(g0, R.sample_neighbors(rp, col, 6, 22, m0), "the hop behind it")


# ---- harness -----------------------------------------------------------------------------------------------------------------------

def _harness_args(**kw):
    import tcgnn_harness as H
    args = H.build_parser().parse_args(["--synthetic", "citeseer", "--dim", "16", "--hidden", "16", "--classes", "4", "--epochs", "3", "--model", "sage",
                                        "--aggregator", "max", "--gpu_preprocess", "--fanout", "5"])
    for k, v in kw.items():
        setattr(args, k, v)
    return args


def test_harness_trains_sage_max_on_sampled_graphs(dev):
    import tcgnn_harness as H
    r = H.run(_harness_args(), quiet=True)
    assert all(k in r and np.isfinite(r[k]) and r[k] >= 0 for k in ("sample_ms", "plan_ms", "train_ms"))
    assert np.isfinite(r["final_loss"]) and np.isfinite(r["sampled_loss"]) and r["fanout"] == [5, 5]
    r2 = H.run(_harness_args(fanout="5,3", model="gcn", aggregator="mean"), quiet=True)
    assert np.isfinite(r2["final_loss"]) and r2["fanout"] == [5, 3] and r2["plan_ms"] > 0


def test_harness_refuses_fanout_with_a_captured_epoch(dev):
    import tcgnn_harness as H
    with pytest.raises(ValueError, match="hip_graph"):
        H.run(_harness_args(hip_graph=True), quiet=True)
