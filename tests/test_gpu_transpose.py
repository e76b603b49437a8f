"""The transposed aggregation on the MI355X: tcgnn_transpose_ws (A^T's CSR and the edge permutation, built on the device), the
transpose=True keyword of the TCGNN operators (A^T's plan cached beside A's; A's own on a symmetric graph), the pybind module's
keyword and the layers' directed=True backward pass.

The contract: a transposed call is bit-identical to the same call on A^T's metadata built on the host (scipy + host SGT), on
every walk; the layers' gradients on a directed graph are those of A^T (DGL port, dense fp64)."""
import glob
import importlib.util
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import graphs
from minibatch_ref import AGNN_DW_TOL, DIRECTED_GRAD_TOL, GCN_DX_NORM_TOL
from oracle import oracle as O
from test_gpu_parity import CASES, ROOT, _sampled_oracle_checks, assert_parity, meta_for, to_dev

pytestmark = pytest.mark.gpu

WIDTHS = (1, 7, 16, 41, 64, 128, 200)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def T():
    import TCGNN
    return TCGNN


def _host_transpose(rp, col):
    """(rp_t, col_t, perm) by a stable sort of the column ids: entry eT of A^T is the eT-th (column, CSR position) pair"""
    n = len(rp) - 1
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))
    perm = np.argsort(col, kind="stable").astype(np.int32)
    rp_t = np.zeros(n + 1, dtype=np.int32)
    rp_t[1:] = np.cumsum(np.bincount(col, minlength=n))
    return rp_t, rows[perm].astype(np.int32), perm


def _directed(name):
    return {"directed_uniform_n3000": lambda: graphs.uniform_graph(3000, 10, seed=21, symmetric=False),
            "directed_powerlaw_n12000": lambda: graphs.powerlaw_graph(12000, 40, seed=22, symmetric=False),
            "directed_uniform_n17": lambda: graphs.uniform_graph(17, 3, seed=23, symmetric=False)}[name]()


DIRECTED = ("directed_uniform_n3000", "directed_powerlaw_n12000", "directed_uniform_n17")


def _non_canonical():
    """unsorted rows with duplicate entries (the host SGT and the plans take them)"""
    rng = np.random.default_rng(5)
    n = 300
    rows = np.sort(rng.integers(0, n, 2400))
    cols = rng.integers(0, n, 2400)
    cols[::7] = cols[1::7][: len(cols[::7])]          # duplicates inside rows
    rp = np.zeros(n + 1, dtype=np.int32)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=n))
    col = cols.astype(np.int32)
    for r in range(n):                                 # shuffle each row
        seg = col[rp[r]:rp[r + 1]]
        rng.shuffle(seg)
    return rp, col


GRAPHS = [(name, rp, c) for name, rp, c in CASES] + [(name, *_directed(name)) for name in DIRECTED] + [("non_canonical_n300", *_non_canonical())]


@pytest.mark.parametrize("case", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_transpose_graph_equals_scipy(dev, T, case):
    name, rp, col = case
    n = len(rp) - 1
    trp, tcol = to_dev(dev, rp, col)
    rp_t, col_t, perm, sym = T.transpose_graph(trp, tcol)
    rp_t, col_t, perm = (t.cpu().numpy() for t in (rp_t, col_t, perm))
    want_rp, want_col, want_perm = _host_transpose(rp, col)
    assert np.array_equal(rp_t, want_rp) and np.array_equal(col_t, want_col) and np.array_equal(perm, want_perm), name
    if name != "non_canonical_n300":
        at = sp.csr_matrix((np.ones(len(col)), col, rp), shape=(n, n)).T.tocsr()
        assert np.array_equal(rp_t, at.indptr) and np.array_equal(col_t, at.indices), name
    assert np.array_equal(np.sort(perm), np.arange(len(col)))
    rows = np.repeat(np.arange(n), np.diff(rp))
    rows_t = np.repeat(np.arange(n), np.diff(rp_t))
    assert np.array_equal(col_t, rows[perm]) and np.array_equal(col[perm], rows_t)
    assert sym == (np.array_equal(rp_t, rp) and np.array_equal(col_t, col)), name
    if name.startswith("directed_") or name == "non_canonical_n300":
        assert not sym
    if name == "citeseer_shape":
        assert sym


def test_transpose_rejects_malformed_graphs_without_a_fault(dev, T):
    rp, col = graphs.uniform_graph(200, 6, seed=3, symmetric=False)
    n = len(rp) - 1
    bad = []
    c = col.copy(); c[17] = n; bad.append((rp, c))                 # an id at N (the forward path takes it, a transpose cannot)
    c = col.copy(); c[5] = -1; bad.append((rp, c))
    r = rp.copy(); r[0] = 1; bad.append((r, col))
    r = rp.copy(); r[50] = r[52] + 3; bad.append((r, col))        # not monotone
    r = rp.copy(); r[-1] = len(col) - 1; bad.append((r, col))     # nodePointer[N] != E
    for r_, c_ in bad:
        with pytest.raises(RuntimeError, match="graph metadata inconsistent"):
            T.transpose_graph(*to_dev(dev, r_, c_))
    torch.cuda.synchronize()
    got = T.transpose_graph(*to_dev(dev, rp, col))             # the library is still good
    assert np.array_equal(got[0].cpu().numpy(), _host_transpose(rp, col)[0])


def _meta_t(dev, rp, col):
    rp_t, col_t, perm = _host_transpose(rp, col)
    return rp_t, col_t, perm, meta_for(dev, rp_t, col_t)


BIT_CASES = [g for g in GRAPHS if g[0] in ("uniform_n40", "empty_middle_window_n48", "powerlaw_n1000", "no_edges_n20", "hub_rows_n2500",
                                          "non_canonical_n300") + DIRECTED]


@pytest.mark.parametrize("case", BIT_CASES, ids=[g[0] for g in BIT_CASES])
def test_transposed_spmm_is_bit_identical_to_the_host_built_transpose_on_every_walk(dev, T, case):
    import tcgnn_capi as capi
    name, rp, col = case
    n = len(rp) - 1
    _, meta = meta_for(dev, rp, col)
    rp_t, col_t, perm, ((bp_t, e2c_t, e2r_t), meta_t) = _meta_t(dev, rp, col)
    rng = np.random.default_rng(n + 3)
    widths = (16, 64, 128) if n > 5000 else WIDTHS
    try:
        for mode in range(6):
            capi.check(capi.lib.tcgnn_set_spmm_mode(mode), "tcgnn_set_spmm_mode")
            for D in widths:
                X = torch.from_numpy((rng.standard_normal((n, D)) * float(rng.choice([0.01, 1.0, 300.0]))).astype(np.float32)).to(dev)
                try:
                    want = T.forward(X, *meta_t)[0]
                except RuntimeError:   # a forced walk this plan cannot take: the transposed call refuses it the same way
                    with pytest.raises(RuntimeError):
                        T.forward(X, *meta, transpose=True)
                    continue
                got = T.forward(X, *meta, transpose=True)[0]
                what = "%s mode %d D=%d" % (name, mode, D)
                assert T.last_kernel(*meta, transpose=True) == T.last_kernel(*meta_t), what
                assert torch.equal(got, want), what
                att = torch.from_numpy(rng.standard_normal(len(col)).astype(np.float32)).to(dev)
                want = T.forward_AGNN(X, meta_t[0], meta_t[1], att[torch.from_numpy(perm).to(dev).long()].view(1, -1), *meta_t[2:])[0]
                got = T.forward_AGNN(X, meta[0], meta[1], att.view(1, -1), *meta[2:], transpose=True)[0]
                assert torch.equal(got, want), "edge-valued " + what
    finally:
        capi.lib.tcgnn_set_spmm_mode(0)
    # and against the oracle's A^T X (TF32-mode and fp64)
    for D in (16, 41, 64):
        Xh = rng.standard_normal((n, D)).astype(np.float32)
        got = T.forward(to_dev(dev, Xh)[0], *meta, transpose=True)[0].cpu().numpy()
        Y64, absY = O.spmm_f64(Xh, rp_t, col_t)
        assert_parity(got, O.spmm(Xh, rp_t, col_t, bp_t, e2c_t, e2r_t, round_mode=O.ROUND_TF32), Y64, absY, "%s A^T X D=%d" % (name, D))
    T.clear_plan_cache()


@pytest.mark.parametrize("case", [g for g in BIT_CASES if g[0] in ("powerlaw_n1000", "directed_uniform_n3000", "directed_powerlaw_n12000")],
                         ids=lambda g: g[0])
def test_transposed_scaled_and_fused_calls_are_bit_identical_to_their_compositions(dev, T, case):
    name, rp, col = case
    n = len(rp) - 1
    _, meta = meta_for(dev, rp, col)
    _, _, _, (_, meta_t) = _meta_t(dev, rp, col)
    rng = np.random.default_rng(n)
    for D in (16, 64, 128):
        X = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)).to(dev)
        gate = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)).to(dev)
        r = torch.from_numpy(rng.uniform(0.05, 2.0, n).astype(np.float32)).to(dev)
        c = torch.from_numpy(rng.uniform(0.05, 2.0, n).astype(np.float32)).to(dev)
        b = torch.from_numpy(rng.standard_normal(D).astype(np.float32)).to(dev)
        for kw in (dict(row_scale=r, col_scale=c, bias=b, relu=True), dict(row_scale=c, col_scale=r, gate=gate), dict(col_scale=c)):
            got = T.forward_scaled(X, *meta, transpose=True, **kw)[0]
            assert torch.equal(got, T.forward_scaled(X, *meta_t, **kw)[0]), "%s D=%d scaled" % (name, D)
            Xp = X * (kw["gate"] > 0) if "gate" in kw else X
            Y = T.forward((kw["col_scale"][:, None] * Xp).contiguous(), *meta_t)[0]
            if kw.get("row_scale") is not None:
                Y = Y * kw["row_scale"][:, None]
            if kw.get("bias") is not None:
                Y = Y + kw["bias"]
            assert torch.equal(got, torch.relu(Y) if kw.get("relu") else Y), "%s D=%d scaled composition" % (name, D)
        got = T.forward_fused(X, *meta, relu=True, transpose=True)[0]
        assert torch.equal(got, torch.relu(T.forward(X, *meta_t)[0]))
        got = T.forward_fused(X, *meta, gate=gate, transpose=True)[0]
        assert torch.equal(got, T.forward((X * (gate > 0)).contiguous(), *meta_t)[0])
    T.clear_plan_cache()


def test_symmetric_graph_reuses_its_plan(dev, T):
    rp, col = graphs.uniform_graph(5000, 12, seed=9)
    _, meta = meta_for(dev, rp, col)
    n, E = len(rp) - 1, len(col)
    rng = np.random.default_rng(0)
    info = T.plan_info(*meta)
    info_t = T.plan_info(*meta, transpose=True)
    assert info_t["symmetric"] and info_t["shares_plan"] and info_t["transpose_bytes"] == 4 * E
    assert {k: info_t[k] for k in info} == info
    rp_t, col_t, perm, sym = T.transpose_graph(meta[0], meta[1])
    assert sym and rp_t is meta[0] and col_t is meta[1]
    for D in (16, 64, 128):
        X = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)).to(dev)
        assert torch.equal(T.forward(X, *meta, transpose=True)[0], T.forward(X, *meta)[0])
        att = torch.from_numpy(rng.standard_normal(E).astype(np.float32)).to(dev)
        got = T.forward_AGNN(X, meta[0], meta[1], att.view(1, -1), *meta[2:], transpose=True)[0]
        assert torch.equal(got, T.forward_AGNN(X, meta[0], meta[1], att[perm.long()].view(1, -1), *meta[2:])[0])
    T.clear_plan_cache()


def test_eviction_takes_everything_a_graph_owns_and_nothing_a_live_one_needs(dev, T):
    """Five small graphs (four directed, one symmetric) through two cache slots, twice, on a side stream: every call past the
    second evicts a plan that has a transposed part, degree scales and a transposed CSR.  The second round computes the first's
    bits, the counts stay within the limit after every call, and clearing gives back every byte."""
    T.clear_plan_cache()
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    gs = [graphs.uniform_graph(200 + 50 * k, 6, seed=70 + k, symmetric=k == 4) for k in range(5)]
    data = []
    for k, (rp, col) in enumerate(gs):
        gen = torch.Generator().manual_seed(k)
        data.append((meta_for(dev, rp, col)[1], torch.randn(len(rp) - 1, 16, generator=gen).to(dev), torch.randn(3, len(col), generator=gen).to(dev)))
    m1 = torch.cuda.memory_allocated()
    T.set_plan_cache_size(2)

    def within_the_limit():
        s = T.cache_stats()
        assert s["plans"] <= 2 and s["transposed"] <= 2 and s["csrs"] <= 2, s   # (every graph here has a plan: no planless CSR entry)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    rounds = []
    try:
        with torch.cuda.stream(side):
            for rnd in range(2):
                outs = []
                for meta, X, val in data:
                    outs.append(T.forward(X, *meta, transpose=True)[0])
                    within_the_limit()
                    outs.append(T.forward_AGNN(X, meta[0], meta[1], val[:1], *meta[2:], transpose=True)[0])
                    within_the_limit()
                    outs.extend(T.degree_scales(meta[0], meta[1], "both"))
                    within_the_limit()
                    outs.append(T.edge_colsum(val, meta[0], meta[1]))
                    within_the_limit()
                rounds.append(outs)
        side.synchronize()
        assert T.cache_stats()["plans"] == 2 and T.cache_stats()["buffers"] >= 2    # (the side stream's workspace and value buffer)
        assert len(rounds[0]) == len(rounds[1]) == 25
        for a, b in zip(*rounds):
            assert a is not b and torch.equal(a, b)
    finally:
        T.set_plan_cache_size(8)
        T.clear_plan_cache()
    assert T.cache_stats() == dict(plans=0, csrs=0, transposed=0, retired=0, buffers=0, buffer_bytes=0)
    del rounds, outs, a, b
    assert torch.cuda.memory_allocated() == m1
    del data, meta, X, val
    assert torch.cuda.memory_allocated() == m0


def _directed_community_graph(n=3000, blocks=6, avg_deg=12, seed=6):
    import tcgnn_graph as G
    rp, col = G.sbm_csr(n, n * avg_deg, seed=seed, blocks=blocks, p_in=0.8, directed=True)
    return rp.numpy(), col.numpy()


def _gcn_pair(dev, rp, col, in_dim, hidden, classes, directed=True, seed=0):
    import tcgnn_layers as L
    from oracle import dgl_gcn_cpu as B
    torch.manual_seed(seed)
    cpu = B.GCN(in_dim, hidden, classes)
    convs = [L.GCNConv(in_dim, hidden, norm="both", bias=True, directed=directed),
             L.GCNConv(hidden, classes, norm="both", bias=True, directed=directed)]
    for conv, layer in zip(convs, cpu.layers):
        with torch.no_grad():
            layer.bias.copy_(torch.randn(layer.bias.shape) * 0.1)
            conv.weights.copy_(layer.weight)
            conv.bias.copy_(layer.bias)
    return [cv.to(dev) for cv in convs], cpu, B.CpuGraph(rp, col, threads=2, symmetric=False)


def _logits(convs, x, meta):
    return convs[1](convs[0](x, *meta, fuse_relu=True), *meta)


def _rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().double()
    return ((a - b).abs() / b.abs().clamp(min=1.0)).max().item()


def _norm_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).norm() / b.norm()).item()


def _dense_input_gradient(rp, col, x, y, cpu, mask):
    """d loss / d x of the port's two layers in fp64 with a dense A, the hidden ReLU taken as the given 0/1 mask"""
    n = len(rp) - 1
    A = torch.from_numpy(sp.csr_matrix((np.ones(len(col)), col, rp), shape=(n, n)).toarray())
    r = torch.from_numpy(np.maximum(np.diff(rp), 1).astype(np.float64)) ** -0.5                   # in-degree: row length
    c = torch.from_numpy(np.maximum(np.bincount(col, minlength=n), 1).astype(np.float64)) ** -0.5  # out-degree: column count
    (W1, b1), (W2, b2) = [(lay.weight.detach().double(), lay.bias.detach().double()) for lay in cpu.layers]
    x64 = x.double().requires_grad_(True)
    h = (r[:, None] * (A @ (c[:, None] * (x64 @ W1))) + b1) * mask
    z = r[:, None] * (A @ (c[:, None] * (h @ W2))) + b2
    torch.nn.functional.cross_entropy(z, y).backward()
    return x64.grad


def test_directed_normalised_gcn_matches_the_dgl_port(dev, T):
    """Logits, weight and bias gradients against the port within 1e-3 (as the symmetric test in test_gpu_scaled_spmm.py).  The input
    gradient is not averaged over nodes: where the 10-bit-operand forward and the port's fp32 forward put a hidden pre-activation on
    different sides of zero, the two ReLU masks differ and so does that element's gradient.  So it is checked (a) element-wise in norm
    against a dense fp64 evaluation of the port's formula that takes the GPU's own mask, tightly, and (b) against the port in norm,
    loosely; and the undirected layer (backward through A) is shown to get it wrong."""
    rp, col = _directed_community_graph()
    _, meta = meta_for(dev, rp, col)
    n = len(rp) - 1
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(n, 32, generator=gen)
    y = torch.randint(0, 7, (n,), generator=torch.Generator().manual_seed(2))
    convs, cpu, graph = _gcn_pair(dev, rp, col, 32, 16, 7)
    xc = x.clone().requires_grad_(True)
    ref = cpu(graph, xc)
    torch.nn.functional.cross_entropy(ref, y).backward()
    xg = x.to(dev).requires_grad_(True)
    hidden = convs[0](xg, *meta, fuse_relu=True)
    got = convs[1](hidden, *meta)
    torch.nn.functional.cross_entropy(got, y.to(dev)).backward()
    ref64 = _dense_input_gradient(rp, col, x, y, cpu, (hidden > 0).detach().cpu().double())
    # the undirected layer (backward through A) on the same weights: the same forward pass, the wrong gradient
    convs_a, _, _ = _gcn_pair(dev, rp, col, 32, 16, 7, directed=False)
    xa = x.to(dev).requires_grad_(True)
    torch.nn.functional.cross_entropy(_logits(convs_a, xa, meta), y.to(dev)).backward()
    errs = {"logits": _rel_err(got, ref), "input grad vs fp64": _norm_err(xg.grad, ref64), "input grad vs port": _norm_err(xg.grad, xc.grad),
            "undirected input grad vs fp64": _norm_err(xa.grad, ref64)}
    for i, (conv, layer) in enumerate(zip(convs, cpu.layers)):
        errs["layer %d weight grad" % i] = _rel_err(conv.weights.grad, layer.weight.grad)
        errs["layer %d bias grad" % i] = _rel_err(conv.bias.grad, layer.bias.grad)
    bounds = {"input grad vs fp64": GCN_DX_NORM_TOL, "input grad vs port": 5e-2}
    for k, e in errs.items():
        if k.startswith("undirected"):
            assert e > 0.2, errs
        else:
            assert e <= bounds.get(k, 1e-3), (k, errs)
    T.clear_plan_cache()


def test_directed_normalised_gcn_trains_like_the_dgl_port(dev, T):
    """20 Adam epochs from the same weights, as test_gpu_scaled_spmm.py::test_normalised_gcn_trains_like_the_dgl_port, on a directed
    community graph: final losses within 2 % of each other."""
    rp, col = _directed_community_graph(seed=7)
    _, meta = meta_for(dev, rp, col)
    n = len(rp) - 1
    size = (n + 5) // 6
    labels = torch.arange(n) // size
    x = torch.randn(n, 32, generator=torch.Generator().manual_seed(3)) + torch.nn.functional.one_hot(labels, 32).float() * 0.5
    convs, cpu, graph = _gcn_pair(dev, rp, col, 32, 16, 6)
    opt_g = torch.optim.Adam([p for cv in convs for p in cv.parameters()], lr=1e-2)
    opt_c = torch.optim.Adam(cpu.parameters(), lr=1e-2)
    xd, yd = x.to(dev), labels.to(dev)
    losses_g, losses_c = [], []
    for _ in range(20):
        opt_g.zero_grad(); opt_c.zero_grad()
        lg = torch.nn.functional.cross_entropy(_logits(convs, xd, meta), yd)
        lc = torch.nn.functional.cross_entropy(cpu(graph, x), labels)
        lg.backward(); lc.backward()
        opt_g.step(); opt_c.step()
        losses_g.append(float(lg)); losses_c.append(float(lc))
    assert losses_g[-1] < 0.8 * losses_g[0], losses_g
    assert abs(losses_g[-1] - losses_c[-1]) <= 0.02 * losses_c[-1], (losses_g[-1], losses_c[-1])
    T.clear_plan_cache()


def test_directed_sag_gin_agnn_match_a_dense_fp64_evaluation(dev, T):
    import tcgnn_layers as L
    rp, col = graphs.powerlaw_graph(600, 10, seed=8, symmetric=False)
    _, meta = meta_for(dev, rp, col)
    n, E = len(rp) - 1, len(col)
    A = torch.from_numpy(sp.csr_matrix((np.ones(E), col, rp), shape=(n, n)).toarray())
    torch.manual_seed(4)
    x = torch.randn(n, 24, dtype=torch.float64)
    dy = torch.randn(n, 12, dtype=torch.float64)

    def run(module_out, dense_out, params_g, params_d):
        (module_out * dy.float().to(dev)).sum().backward()
        (dense_out * dy).sum().backward()
        for pg, pd in zip(params_g, params_d):
            scale = pd.grad.abs().max().item()
            assert ((pg.grad.detach().cpu().double() - pd.grad).abs().max().item()) <= DIRECTED_GRAD_TOL * max(1.0, scale)   # (10-bit operands)

    xg, xd = x.float().to(dev).requires_grad_(True), x.clone().requires_grad_(True)
    sag = L.SAG(*meta, directed=True)
    run(sag(xg[:, :12].contiguous()), A @ xd[:, :12], [xg], [xd])

    gin = L.GINConv(24, 12, directed=True)
    with torch.no_grad():
        gin.weights.mul_(0.2)
    Wd = gin.weights.detach().double().clone().requires_grad_(True)
    gin = gin.to(dev)
    xg, xd = x.float().to(dev).requires_grad_(True), x.clone().requires_grad_(True)
    run(gin(xg, *meta), (A @ xd) @ Wd, [xg, gin.weights], [xd, Wd])

    agnn = L.AGNNConv(24, 12, directed=True)
    with torch.no_grad():
        agnn.attention_w.fill_(0.3)
    Wd = agnn.weights.detach().double().clone().requires_grad_(True)
    agnn = agnn.to(dev)
    xg, xd = x.float().to(dev).requires_grad_(True), x.clone().requires_grad_(True)
    rows = torch.from_numpy(np.repeat(np.arange(n), np.diff(rp))).long()
    colt = torch.from_numpy(col).long()
    H = xd @ Wd
    att = 0.3 * (H[rows] * H[colt]).sum(1).detach()               # (the layer does not propagate through the scores)
    Aatt = torch.zeros(n, n, dtype=torch.float64).index_put_((rows, colt), att, accumulate=True)
    run(agnn(xg, *meta), Aatt @ H, [xg, agnn.weights], [xd, Wd])
    dyh = dy
    d_w = ((dyh[rows] * dyh[colt]).sum(1) * colt.double()).sum().item()
    bound = ((dyh[rows] * dyh[colt]).sum(1).abs() * colt.double()).sum().item()
    assert abs(float(agnn.attention_w.grad) - d_w) <= AGNN_DW_TOL * bound
    T.clear_plan_cache()


def _directed_model(dev, n):
    import tcgnn_layers as L
    torch.manual_seed(5)
    convs = [L.GCNConv(32, 16, norm="both", bias=True, directed=True), L.AGNNConv(16, 6, directed=True)]
    return [cv.to(dev) for cv in convs]


def _step(convs, x, y, meta):
    for cv in convs:
        for p in cv.parameters():
            p.grad = None
    loss = torch.nn.functional.cross_entropy(convs[1](convs[0](x, *meta, fuse_relu=True), *meta), y)
    loss.backward()
    return loss


def test_directed_training_step_allocates_nothing_does_not_synchronise_and_replays_bit_equal(dev, T):
    rp, col = _directed_community_graph(seed=9)
    _, meta = meta_for(dev, rp, col)
    n = len(rp) - 1
    convs = _directed_model(dev, n)
    params = [p for cv in convs for p in cv.parameters()]
    x = torch.randn(n, 32, device=dev)
    y = torch.randint(0, 6, (n,), device=dev)
    T.prepare([16, 6], *meta, transpose=True, edge_valued=True)
    _step(convs, x, y, meta)
    torch.cuda.synchronize()
    _step(convs, x, y, meta)
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    _step(convs, x, y, meta)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == m0   # (the loss and the gradients replace the previous step's: nothing accumulates)
    torch.cuda.set_sync_debug_mode("error")
    try:
        _step(convs, x, y, meta)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            _step(convs, x, y, meta)
        eager_loss = _step(convs, x, y, meta).detach().clone()
        eager_grads = [p.grad.clone() for p in params]
        for p in params:
            p.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            static_loss = torch.nn.functional.cross_entropy(convs[1](convs[0](x, *meta, fuse_relu=True), *meta), y)
            static_loss.backward()
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_loss, eager_loss)
    for p, g in zip(params, eager_grads):
        assert torch.equal(p.grad, g)
    del graph
    T.clear_plan_cache()


def test_transposed_spmm_at_full_size_on_the_production_walk(dev, T):
    """A directed Reddit-shaped graph with communities: A^T X at D = 64 bit-equal to forward on A^T's metadata built by the device SGT
    (same walk), and that call against the oracle on sampled windows of the A^T graph."""
    import tcgnn_graph as G
    n, nnz, _, _ = G.SHAPES["reddit"]
    rp, col = G.sbm_reddit_csr(n, nnz, seed=0, device=dev, directed=True)
    E = col.numel()
    nw = (n + 15) // 16

    def translate(rp_, col_):
        bp = torch.zeros(nw, dtype=torch.int32, device=dev); e2c = torch.zeros(E, dtype=torch.int32, device=dev); e2r = torch.zeros(E, dtype=torch.int32, device=dev)
        T.preprocess_gpu(col_, rp_, n, 16, 8, bp, e2c, e2r)
        return (rp_, col_, bp, e2c, e2r)
    meta = translate(rp, col)
    rp_t, col_t, perm, sym = T.transpose_graph(rp, col)
    assert not sym
    meta_t = translate(rp_t.clone(), col_t.clone())
    T.prepare([64], *meta, transpose=True)
    X = torch.randn(n, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    got = T.forward(X, *meta, transpose=True)[0]
    want = T.forward(X, *meta_t)[0]
    assert T.last_kernel(*meta, transpose=True) == T.last_kernel(*meta_t)
    assert torch.equal(got, want)
    T.clear_plan_cache()
    _sampled_oracle_checks(dev, T, n, E, meta_t, 64, nwin=128)
    T.clear_plan_cache()


@pytest.fixture(scope="module")
def ext():
    found = glob.glob(os.path.join(ROOT, "integration", "TCGNN*.so"))
    assert found, "integration/TCGNN*.so is not built"
    spec = importlib.util.spec_from_file_location("TCGNN", found[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_binding_transposed_calls_equal_the_ctypes_module(dev, T, ext):
    for rp, col in (graphs.powerlaw_graph(3000, 12, seed=31, symmetric=False), graphs.uniform_graph(2000, 8, seed=32)):
        _, meta = meta_for(dev, rp, col)
        n, E = len(rp) - 1, len(col)
        rng = np.random.default_rng(n)
        for D in (16, 64):
            X = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)).to(dev)
            att = torch.from_numpy(rng.standard_normal(E).astype(np.float32)).to(dev).view(1, -1)
            r = torch.from_numpy(rng.uniform(0.1, 1.0, n).astype(np.float32)).to(dev)
            assert torch.equal(ext.forward(X, *meta, transpose=True)[0], T.forward(X, *meta, transpose=True)[0])
            assert torch.equal(ext.backward(X, *meta, transpose=True)[0], T.forward(X, *meta, transpose=True)[0])
            assert torch.equal(ext.forward_AGNN(X, meta[0], meta[1], att, *meta[2:], transpose=True)[0],
                               T.forward_AGNN(X, meta[0], meta[1], att, *meta[2:], transpose=True)[0])
            assert torch.equal(ext.forward_scaled(X, *meta, row_scale=r, col_scale=r, relu=True, transpose=True)[0],
                               T.forward_scaled(X, *meta, row_scale=r, col_scale=r, relu=True, transpose=True)[0])
            assert torch.equal(ext.forward(X, *meta)[0], T.forward(X, *meta)[0])
    ext.clear_plan_cache()
    T.clear_plan_cache()
