"""tcgnn_spmm_scaled / TCGNN.forward_scaled / GCNConv(norm=..., bias=...) on the MI355X: the GCN layer's degree normalisation and
bias fused into the SpMM kernels (column scale while X is staged, row scale / bias / ReLU where the final kernel stores Y).

The contract is bit-identity with the unfused fp32 composition forward(c * X') -> * r -> + b -> relu on every walk; the rest checks
the composition itself against the oracle and the normalised layer against the DGL port in oracle/dgl_gcn_cpu.py."""
import numpy as np
import pytest
import torch

import graphs
from oracle import oracle as O
from test_gpu_parity import CASES, assert_parity, meta_for, to_dev

pytestmark = pytest.mark.gpu

WIDTHS = (1, 7, 16, 41, 64, 128, 200)
VARIANTS = ("r", "c", "rc", "rcb", "rcb_relu", "c_gate")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def T():
    import TCGNN
    return TCGNN


def _mixed(rng, shape, dev):
    """magnitudes mixed the way test_three_kernels_match_oracle mixes them (0.01 / 1 / 300)"""
    mag = float(rng.choice([0.01, 1.0, 300.0]))
    return torch.from_numpy((rng.standard_normal(shape) * mag).astype(np.float32)).to(dev)


def _composition(T, meta, X, r=None, c=None, b=None, relu=False, gate=None):
    Xp = X * (gate > 0) if gate is not None else X
    if c is not None:
        Xp = c[:, None] * Xp
    Y = T.forward(Xp.contiguous(), *meta)[0]
    if r is not None:
        Y = Y * r[:, None]
    if b is not None:
        Y = Y + b
    return torch.relu(Y) if relu else Y


def _variant(v, rng, n, D, dev, Y0):
    r = torch.from_numpy(rng.uniform(0.05, 2.0, n).astype(np.float32)).to(dev) if "r" in v else None
    c = torch.from_numpy(rng.uniform(0.05, 2.0, n).astype(np.float32)).to(dev) if "c" in v else None
    b = torch.from_numpy(rng.standard_normal(D).astype(np.float32)).to(dev) if "b" in v else None
    gate = Y0 if "gate" in v else None
    return dict(row_scale=r, col_scale=c, bias=b, relu=v.endswith("relu"), gate=gate)


def _check_identity(T, meta, X, kw, what):
    want = _composition(T, meta, X, kw["row_scale"], kw["col_scale"], kw["bias"], kw["relu"], kw["gate"])
    walk = T.last_kernel(*meta)
    got = T.forward_scaled(X, *meta, **kw)[0]
    assert T.last_kernel(*meta) == walk, "%s: the scaled call took %s, the composition %s" % (what, T.last_kernel(*meta), walk)
    assert torch.equal(got, want), "%s: max |diff| %.3e" % (what, (got - want).abs().max().item())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_scaled_spmm_is_bit_identical_to_the_composition_on_every_walk(dev, T, case):
    import tcgnn_capi as capi
    name, rp, col = case
    n = len(rp) - 1
    _, meta = meta_for(dev, rp, col)
    rng = np.random.default_rng(n + 7)
    widths = (16, 64, 128) if n > 5000 else WIDTHS
    try:
        for mode in range(6):
            capi.check(capi.lib.tcgnn_set_spmm_mode(mode), "tcgnn_set_spmm_mode")
            for D in widths:
                X = _mixed(rng, (n, D), dev)
                try:
                    Y0 = T.forward(X, *meta)[0]
                except RuntimeError:
                    # a forced walk this plan cannot take: the scaled call refuses it the same way
                    with pytest.raises(RuntimeError):
                        T.forward_scaled(X, *meta, row_scale=torch.ones(n, device=dev))
                    continue
                for v in VARIANTS:
                    _check_identity(T, meta, X, _variant(v, rng, n, D, dev, Y0), "%s mode %d D=%d %s" % (name, mode, D, v))
    finally:
        capi.lib.tcgnn_set_spmm_mode(0)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ("uniform_n17", "empty_middle_window_n48", "powerlaw_n1000", "citeseer_shape",
                                                                 "hub_rows_n2500", "no_edges_n20")], ids=lambda c: c[0])
@pytest.mark.parametrize("D", [16, 41, 64])
def test_scaled_spmm_matches_the_oracle(dev, T, case, D):
    """c * X meets the 10-bit operand rounding like any input of forward(); r is one fp32 multiply behind it."""
    name, rp, col = case
    n = len(rp) - 1
    (bp, e2c, e2r), meta = meta_for(dev, rp, col)
    rng = np.random.default_rng(D + n)
    X = rng.standard_normal((n, D)).astype(np.float32)
    r = rng.uniform(0.1, 1.0, n).astype(np.float32)
    c = rng.uniform(0.1, 1.0, n).astype(np.float32)
    tX, tr, tc = to_dev(dev, X, r, c)
    got = T.forward_scaled(tX, *meta, row_scale=tr, col_scale=tc)[0].cpu().numpy()
    Xc = (c[:, None] * X).astype(np.float32)
    ref = (O.spmm(Xc, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32) * r[:, None]).astype(np.float32)
    r64, a64 = O.spmm_f64(Xc, rp, col)
    assert_parity(got, ref, r64 * r[:, None].astype(np.float64), a64 * r[:, None].astype(np.float64), "%s D=%d" % (name, D))


def _full_size(dev, T, shape, generator):
    import tcgnn_graph as G
    n, nnz, _, _ = G.SHAPES[shape]
    rp, col = G.GENERATORS[generator](n, nnz, seed=0, device=dev)
    E = col.numel()
    nw = (n + 15) // 16
    bp = torch.zeros(nw, dtype=torch.int32, device=dev); e2c = torch.zeros(E, dtype=torch.int32, device=dev); e2r = torch.zeros(E, dtype=torch.int32, device=dev)
    T.preprocess_gpu(col, rp, n, 16, 8, bp, e2c, e2r)
    return n, (rp, col, bp, e2c, e2r)


def _sampled_rows_fp64(meta, X, r, c, b, rows):
    """the normalised aggregation of a few rows in fp64 on the host (r * sum_j c_j x_j + b)"""
    rp = meta[0].cpu().numpy(); col = meta[1].cpu().numpy()
    Xh = X.double().cpu().numpy(); rh = r.double().cpu().numpy(); ch = c.double().cpu().numpy(); bh = b.double().cpu().numpy()
    out, scale = [], []
    for i in rows:
        nb = col[rp[i]:rp[i + 1]]
        terms = ch[nb, None] * Xh[nb]
        out.append(rh[i] * terms.sum(0) + bh)
        scale.append(rh[i] * np.abs(terms).sum(0) + np.abs(bh))
    return np.array(out), np.array(scale)


@pytest.mark.parametrize("shape,generator,D,walk", [("reddit", "sbm_reddit", 64, "spmm_lds_flat_kernel"),
                                                     ("ogbn-products", "sbm", 128, "spmm_sync_kernel")])
def test_production_walks_at_full_size(dev, T, shape, generator, D, walk):
    n, meta = _full_size(dev, T, shape, generator)
    r, c = T.degree_scales(meta[0], meta[1], "both")
    g = torch.Generator(device=dev).manual_seed(5)
    X = torch.randn(n, D, device=dev, generator=g)
    b = torch.randn(D, device=dev, generator=g)
    T.prepare([D], *meta)
    Y0 = T.forward(X, *meta)[0]
    assert T.last_kernel(*meta) == walk
    for kw in (dict(row_scale=r, col_scale=c, bias=b, relu=True), dict(row_scale=r, col_scale=c), dict(col_scale=r, row_scale=c, gate=Y0)):
        _check_identity(T, meta, X, dict(dict(row_scale=None, col_scale=None, bias=None, relu=False, gate=None), **kw), "%s D=%d" % (shape, D))
        assert T.last_kernel(*meta) == walk
    Y = T.forward_scaled(X, *meta, row_scale=r, col_scale=c, bias=b)[0]
    rows = np.random.default_rng(1).choice(n, 256, replace=False)
    ref, scale = _sampled_rows_fp64(meta, X, r, c, b, rows)
    err = np.abs(Y[torch.from_numpy(rows).to(dev)].double().cpu().numpy() - ref) / (scale + 1.0)
    assert err.max() <= 2.0 ** -9, err.max()
    T.clear_plan_cache()


def test_range_guard_decides_on_the_scaled_operand(dev, T):
    """include/tcgnn.h "Operand range": a 3e7 row over 1e-3 data is "wide".  (a) X is wide but c * X is not (that row's c is
    1e-7): the MFMA walk runs; (b) X is ordinary but c * X is wide (one c of 3e10): the fp32 fallback runs.  Both bit-identical
    to the composition, which makes the same decision on the same matrix."""
    import tcgnn_capi as capi
    rp, col = graphs.uniform_graph(4109, 100, seed=31)
    _, meta = meta_for(dev, rp, col)
    n = len(rp) - 1
    rng = np.random.default_rng(9)
    try:
        for mode in (0, 1, 3, 4):
            capi.check(capi.lib.tcgnn_set_spmm_mode(mode), "tcgnn_set_spmm_mode")
            for D in (64, 80):
                X = (rng.standard_normal((n, D)) * 1e-3).astype(np.float32)
                X[777] = 3e7 * (1.0 + rng.random(D).astype(np.float32))
                tX = torch.from_numpy(X).to(dev)
                c = torch.ones(n, device=dev); c[777] = 1e-7
                r = torch.from_numpy(rng.uniform(0.5, 1.0, n).astype(np.float32)).to(dev)
                if mode != 4:
                    T.forward(tX, *meta)
                    assert T.range_mode()[0] == 1
                kw = dict(row_scale=r, col_scale=c, bias=None, relu=True, gate=None)
                _check_identity(T, meta, tX, kw, "narrowed mode %d D=%d" % (mode, D))
                if mode != 4:
                    assert T.range_mode()[0] == 0, "mode %d: c * X is not wide" % mode
                X2 = torch.from_numpy((rng.standard_normal((n, D)) * 1e-3).astype(np.float32)).to(dev)
                c2 = torch.ones(n, device=dev); c2[777] = 3e10
                kw = dict(row_scale=r, col_scale=c2, bias=torch.ones(D, device=dev), relu=False, gate=None)
                _check_identity(T, meta, X2, kw, "widened mode %d D=%d" % (mode, D))
                if mode != 4:
                    assert T.range_mode()[0] == 1, "mode %d: c * X is wide" % mode
    finally:
        capi.lib.tcgnn_set_spmm_mode(0)
        T.clear_plan_cache()


def _gcn_pair(dev, rp, col, in_dim, hidden, classes, seed=0):
    import tcgnn_layers as L
    from oracle import dgl_gcn_cpu as B
    torch.manual_seed(seed)
    cpu = B.GCN(in_dim, hidden, classes)
    convs = [L.GCNConv(in_dim, hidden, norm="both", bias=True), L.GCNConv(hidden, classes, norm="both", bias=True)]
    for conv, layer in zip(convs, cpu.layers):
        with torch.no_grad():
            layer.bias.copy_(torch.randn(layer.bias.shape) * 0.1)   # (nonzero: the bias gradient and its place in the sum are exercised)
            conv.weights.copy_(layer.weight)
            conv.bias.copy_(layer.bias)
    convs = [cv.to(dev) for cv in convs]
    return convs, cpu, B.CpuGraph(rp, col, threads=2, symmetric=True)


def _gpu_logits(convs, x, meta):
    h = convs[0](x, *meta, fuse_relu=True)
    return convs[1](h, *meta)


def test_normalised_gcn_layer_matches_the_dgl_port(dev, T):
    rp, col = graphs.uniform_graph(2000, 8, seed=4)
    _, meta = meta_for(dev, rp, col)
    n = len(rp) - 1
    convs, cpu, graph = _gcn_pair(dev, rp, col, 32, 16, 7)
    x = torch.randn(n, 32, generator=torch.Generator().manual_seed(1))
    y = torch.randint(0, 7, (n,), generator=torch.Generator().manual_seed(2))
    ref = cpu(graph, x)
    torch.nn.functional.cross_entropy(ref, y).backward()
    got = _gpu_logits(convs, x.to(dev), meta)
    torch.nn.functional.cross_entropy(got, y.to(dev)).backward()

    def close(a, b, what):
        a, b = a.detach().cpu().double(), b.detach().double()
        err = ((a - b).abs() / b.abs().clamp(min=1.0)).max().item()
        assert err <= 1e-3, "%s: %.3e" % (what, err)
    close(got, ref, "logits")
    for i, (conv, layer) in enumerate(zip(convs, cpu.layers)):
        close(conv.weights.grad, layer.weight.grad, "layer %d weight grad" % i)
        close(conv.bias.grad, layer.bias.grad, "layer %d bias grad" % i)


@pytest.mark.parametrize("norm", ["right", "left"])
def test_right_and_left_norms_against_a_dense_fp64_layer(dev, T, norm):
    import tcgnn_layers as L
    rp, col = graphs.powerlaw_graph(600, 10, seed=8)
    _, meta = meta_for(dev, rp, col)
    n = len(rp) - 1
    A = np.zeros((n, n))
    for i in range(n):
        A[i, col[rp[i]:rp[i + 1]]] = 1.0
    deg_in = np.maximum(A.sum(1), 1.0); deg_out = np.maximum(A.sum(0), 1.0)
    torch.manual_seed(3)
    conv = L.GCNConv(24, 12, norm=norm, bias=True)
    conv.reset_parameters()   # (O(1) activations: the 1e-3 bar is stated for them - unscaled weights make X W ~ 5 and the bar relative to that)
    with torch.no_grad():
        conv.bias.normal_()
    conv = conv.to(dev)
    x = torch.randn(n, 24)
    got = conv(x.to(dev), *meta).detach().cpu().double().numpy()
    H = x.double().numpy() @ conv.weights.detach().cpu().double().numpy()
    An = A / deg_in[:, None] if norm == "right" else A / deg_out[None, :]
    ref = An @ H + conv.bias.detach().cpu().double().numpy()
    assert (np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max() <= 1e-3


def test_eager_calls_allocate_nothing_once_the_scales_are_cached(dev, T):
    """Once a graph's scales are cached, a forward_scaled call and a normalised layer call allocate nothing that outlives them (the
    output is the only allocation: deleting it returns memory_allocated() to where it was), and the scales are the same tensors."""
    rp, col = graphs.community_graph(3000, 6, 12, 0.8, seed=5)
    _, meta = meta_for(dev, rp, col)
    n = len(rp) - 1
    x = torch.randn(n, 16, device=dev)
    convs, _, _ = _gcn_pair(dev, rp, col, 16, 16, 6)
    r, c = T.degree_scales(meta[0], meta[1], "both")
    with torch.no_grad():
        T.forward_scaled(x, *meta, row_scale=r, col_scale=c)
        convs[0](x, *meta, fuse_relu=True)
        torch.cuda.synchronize()
        m0 = torch.cuda.memory_allocated()
        out = T.forward_scaled(x, *meta, row_scale=r, col_scale=c, bias=convs[0].bias, relu=True)[0]
        del out
        assert torch.cuda.memory_allocated() == m0
        out = convs[0](x, *meta, fuse_relu=True)
        del out
        assert torch.cuda.memory_allocated() == m0
    r2, c2 = T.degree_scales(meta[0], meta[1], "both")
    assert r2 is r and c2 is c
    T.clear_plan_cache()
    r3, _ = T.degree_scales(meta[0], meta[1], "both")
    assert r3 is not r and torch.equal(r3, r)   # (evicted with the plan, recomputed to the same values)
    T.clear_plan_cache()


def test_the_layer_step_does_not_synchronise(dev, T):
    """What a HIP-graph capture cannot contain: a forward + backward step of the normalised GCN, eager, under torch's sync
    debug mode set to raise - also with the scale cache empty (degree_scales computes without reading anything back)."""
    rp, col = graphs.community_graph(3000, 6, 12, 0.8, seed=5)
    _, meta = meta_for(dev, rp, col)
    n = len(rp) - 1
    convs, _, _ = _gcn_pair(dev, rp, col, 32, 16, 6)
    x = torch.randn(n, 32, device=dev)
    y = torch.randint(0, 6, (n,), device=dev)
    T.prepare([16, 6], *meta)
    torch.nn.functional.cross_entropy(_gpu_logits(convs, x, meta), y).backward()   # (the plan and workspace exist from here on)
    torch.cuda.synchronize()
    T.drop_scales(meta[0], meta[1])
    stats = T.cache_stats()
    assert stats["plans"] >= 1 and stats["buffers"] >= 1   # (the plan and the workspace stay; only the scales are computed again)
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.nn.functional.cross_entropy(_gpu_logits(convs, x, meta), y).backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    T.clear_plan_cache()


def test_normalised_gcn_trains_like_the_dgl_port(dev, T):
    """20 Adam epochs (lr 1e-2) from the same initial weights on a labelled community graph.  Bound on the final loss: 2 %
    relative.  Each forward / backward aggregation rounds its operands to a 10-bit mantissa (<= 2^-11 relative per element,
    ~1e-4 after averaging over a row) where the port computes in fp32; Adam's normalised steps of size lr move every weight by the
    same amount in both runs as long as the gradient signs agree, so the two trajectories separate only through the few weights
    whose gradients are near zero - measured differences are far below 2 %, which is still tight enough to catch a wrong gradient
    (a missing scale or bias term moves the final loss by tens of percent)."""
    rp, col = graphs.community_graph(3000, 6, 12, 0.8, seed=6)
    _, meta = meta_for(dev, rp, col)
    n = len(rp) - 1
    size = (n + 5) // 6
    labels = torch.arange(n) // size
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(n, 32, generator=gen) + torch.nn.functional.one_hot(labels, 32).float() * 0.5
    convs, cpu, graph = _gcn_pair(dev, rp, col, 32, 16, 6)
    opt_g = torch.optim.Adam([p for cv in convs for p in cv.parameters()], lr=1e-2)
    opt_c = torch.optim.Adam(cpu.parameters(), lr=1e-2)
    xd, yd = x.to(dev), labels.to(dev)
    losses_g, losses_c = [], []
    for _ in range(20):
        opt_g.zero_grad(); opt_c.zero_grad()
        lg = torch.nn.functional.cross_entropy(_gpu_logits(convs, xd, meta), yd)
        lc = torch.nn.functional.cross_entropy(cpu(graph, x), labels)
        lg.backward(); lc.backward()
        opt_g.step(); opt_c.step()
        losses_g.append(float(lg)); losses_c.append(float(lc))
    assert losses_g[-1] < 0.8 * losses_g[0], losses_g
    assert abs(losses_g[-1] - losses_c[-1]) <= 0.02 * losses_c[-1], (losses_g[-1], losses_c[-1])


def test_training_step_captured_in_a_hip_graph_replays_bit_equal(dev, T):
    """A forward + backward step of the normalised GCN (norm='both', bias, fused ReLU) captured with torch.cuda.graph after warm-up
    on the side stream the capture runs on (the workspace, the scales and every width's walk exist before the capture begins)
    replays to the same loss and gradients, bit for bit, as the same step run eagerly."""
    rp, col = graphs.community_graph(3000, 6, 12, 0.8, seed=5)
    _, meta = meta_for(dev, rp, col)
    n = len(rp) - 1
    convs, _, _ = _gcn_pair(dev, rp, col, 32, 16, 6)
    params = [p for cv in convs for p in cv.parameters()]
    x = torch.randn(n, 32, device=dev)
    y = torch.randint(0, 6, (n,), device=dev)
    T.prepare([16, 6], *meta)

    def step():
        for p in params:
            p.grad = None
        loss = torch.nn.functional.cross_entropy(_gpu_logits(convs, x, meta), y)
        loss.backward()
        return loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
        eager_loss = step().detach().clone()
        eager_grads = [p.grad.clone() for p in params]
        for p in params:
            p.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            static_loss = torch.nn.functional.cross_entropy(_gpu_logits(convs, x, meta), y)
            static_loss.backward()
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_loss, eager_loss)
    for p, g in zip(params, eager_grads):
        assert torch.equal(p.grad, g)
    T.clear_plan_cache()
