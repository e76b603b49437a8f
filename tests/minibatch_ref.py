"""What tests/test_minibatch_cpu.py and tests/test_gpu_minibatch.py share: the catalogue of mini-batch blocks (each from the numpy
restatements frontier_ref / subgraph_ref and, on the device, from the tcgnn_layers call that builds the same batch), the table of
layer configurations with their dense fp64 models, the bounds and how a share of a bound is measured.  No GPU needed to import.

The dense models are the ones the per-layer tests use (gat_ref, gatv2_ref, stats_ref, edge_message_ref, segmax_ref, edge_ops_ref,
sddmm_heads_ref); the GCN / GIN / AGNN expressions, which tests/test_gpu_transpose.py and tests/test_gpu_scaled_spmm.py write inline,
are stated here once as functions with the operand-rounding switch gat_ref.dense_gat_model has.

Bounds.  Every bound is the one the layer's own GPU test applies: gat_ref.GPU_LAYER_TOL, stats_ref.LAYER_TOL_Y / _G,
edge_message_ref.TOL_Y / TOL_G, segmax_ref.SAGE_TOL, walks.TOL (the 1e-3 bar of tests/test_gpu_scaled_spmm.py) and the three
constants below, which tests/test_gpu_transpose.py imports from here.  The one bound no test states is the VALUE of the binary GCN /
GIN / reference-AGNN layers (tests/test_gpu_transpose.py judges their gradients only): the forward pass is the same SpMM on A that
the backward pass runs on A^T, over operands rounded the same way, so it is held to the gradients' bound."""
import types
import zlib

import numpy as np

import edge_message_ref as EM
import edge_ops_ref as EO
import frontier_ref as FR
import gat_ref as G
import gatv2_ref as V
import graphs
import sddmm_heads_ref as HR
import segmax_ref as SM
import stats_ref as ST
import subgraph_ref as SG
import walks

DIRECTED_GRAD_TOL = 5e-3     # tests/test_gpu_transpose.py: SAG / GIN / AGNN gradients, of max(1, largest entry) (10-bit operands)
AGNN_DW_TOL = 2e-3           # ... the reference's d attention_w, of sum |sddmm(dY)[e]| col[e]
GCN_DX_NORM_TOL = 3e-3       # ... the normalised GCN's input gradient against dense fp64, in norm
GCN_TOL = walks.TOL          # tests/test_gpu_scaled_spmm.py: logits and parameter gradients, element-wise of max(1, |ref|)

INP, OUT, HEADS = G.LAYER_CASE["inp"], G.LAYER_CASE["out"], G.LAYER_CASE["heads"]
EDGE_DIM = 5
SAMPLE_SEED = 13


# ---- the catalogue -----------------------------------------------------------------------------------------------------------------------

_FULL = []


def full_graph():
    """(rowptr, col) of the graph every entry is drawn from: a six-community graph with the rows of window 6 emptied (isolated seeds)"""
    if not _FULL:
        rp, col = graphs.community_graph(1500, 6, 14, 0.8, seed=4)
        _FULL.append(graphs.with_empty_window(rp, col, 96, 112))
    return _FULL[0]


_SEEDS48 = np.sort(np.random.default_rng(3).choice(1500, 48, replace=False))
_ROOTS40 = np.sort(np.random.default_rng(3).choice(1500, 40, replace=False))


class Entry:
    """One mini-batch.  host(): (nodes, new_id, seed_pos, [(nodePointer_b, edgeList_b)], [eid]) from the numpy restatements, one pair per
    layer graph (input layer first), computed once.  device(L, csr): the CompactBatch of the same batch through tcgnn_layers, plan=True."""

    def __init__(self, name, kind, ids, fanouts=None, walk_length=None):
        self.name, self.kind, self.ids, self.fanouts, self.walk_length = name, kind, np.asarray(ids), fanouts, walk_length
        self._host = None

    def host(self):
        if self._host is None:
            rp, col = full_graph()
            if self.kind == "rows":
                self._host = FR.batch_rows(rp, col, self.ids, self.fanouts, SAMPLE_SEED)
            else:
                if self.kind == "cluster":
                    nodes, new_id, pos, block, eid = SG.subgraph_batch(rp, col, self.ids)
                else:
                    nodes, new_id, pos, block, eid = SG.saint_batch(rp, col, self.ids, self.walk_length, SAMPLE_SEED)
                self._host = (nodes, new_id, pos, [block], [eid])
        return self._host

    def device(self, L, csr):
        import torch
        dev = csr[0].device
        if self.kind == "rows":
            return L.sample_batch_rows(csr, torch.from_numpy(self.ids.astype(np.int64)).to(dev), list(self.fanouts), SAMPLE_SEED, plan=True)
        ids = torch.from_numpy(self.ids.astype(np.int32)).to(dev)
        if self.kind == "cluster":
            return L.subgraph_batch(csr, ids, plan=True)
        return L.saint_batch(csr, ids, self.walk_length, SAMPLE_SEED, plan=True)


CATALOGUE = [
    Entry("fanout_4_3", "rows", _SEEDS48, fanouts=(4, 3)),
    Entry("fanout_5_3_2", "rows", _SEEDS48, fanouts=(5, 3, 2)),
    Entry("few_2_2", "rows", _SEEDS48[:3], fanouts=(2, 2)),
    Entry("one_1_1", "rows", _SEEDS48[:1], fanouts=(1, 1)),
    Entry("isolated_seed", "rows", [100], fanouts=(3, 3)),
    Entry("cluster_310", "cluster", np.arange(1000, 1310)),
    Entry("saint_40x2", "saint", _ROOTS40, walk_length=2),
]
ENTRIES = {e.name: e for e in CATALOGUE}

# what every entry is in the catalogue for, pinned by tests/test_minibatch_cpu.py: M, and per layer graph (input layer first) the edges,
# the rows with edges, the 16-row windows without any and whether the block is symmetric
FACTS = {
    "fanout_4_3": dict(M=653, E=[712, 144], rows=[178, 48], empty_windows=[1, 11], symmetric=[False, False]),
    "fanout_5_3_2": dict(M=1204, E=[2205, 408, 96], rows=[441, 136, 48], empty_windows=[0, 12, 40], symmetric=[False, False, False]),
    "few_2_2": dict(M=24, E=[18, 6], rows=[9, 3], empty_windows=[0, 1], symmetric=[False, False]),
    "one_1_1": dict(M=4, E=[2, 1], rows=[2, 1], empty_windows=[0, 0], symmetric=[False, False]),
    "isolated_seed": dict(M=1, E=[0, 0], rows=[0, 0], empty_windows=[1, 1], symmetric=[True, True]),
    # the subgraph a SYMMETRIC graph induces on a node set is symmetric: the range lies clear of the emptied rows, so this block is.  It is
    # in the catalogue for its shape (square, every row used, the longest rows); the wrong-matrix condition names it as an exception
    "cluster_310": dict(M=310, E=[3078], rows=[308], empty_windows=[0], symmetric=[True]),
    # (the walks visit nodes of the emptied window, whose rows are empty and whose columns are not: the block is not symmetric)
    "saint_40x2": dict(M=110, E=[228], rows=[108], empty_windows=[0], symmetric=[False]),
}
# blocks on which a layer that back-propagates through A instead of A^T can not be told apart: no edges, and A = A^T
INSENSITIVE = ("isolated_seed", "cluster_310")


def block_facts(nodes, blocks):
    M = len(nodes)
    out = dict(M=M, E=[], rows=[], empty_windows=[], symmetric=[])
    for rp_b, col_b in blocks:
        d = np.diff(rp_b)
        used = np.zeros((M + 15) // 16, dtype=bool)
        used[np.nonzero(d)[0] // 16] = True
        out["E"].append(len(col_b)); out["rows"].append(int((d > 0).sum())); out["empty_windows"].append(int((~used).sum()))
        out["symmetric"].append(bool(walks.is_symmetric(rp_b, col_b)))
    return out


# ---- dense fp64 models that the per-layer tests write inline ------------------------------------------------------------------------------

def _aggregate(A, Z, rounded):
    """A @ Z; rounded: Z as the kernels stage it (10 mantissa bits, walks.round_tf32) and, on the way back, dY alike"""
    if not rounded:
        return A @ Z
    return G._make_round_grad().apply(A @ (Z + (G._round_tf32_t(Z) - Z).detach()))


def dense_gcn(A, X, W, bias=None, norm="none", round_operands=False):
    """GCNConv: Y = r * (A (c * (X W))) + b with DGL's 'both' scales (in-degree = row sums, out-degree = column sums, clamped to 1) or
    none (the binary layer of tests/test_gpu_transpose.py)"""
    H = X @ W
    if norm == "both":
        r, c = A.sum(1).clamp(min=1) ** -0.5, A.sum(0).clamp(min=1) ** -0.5
        Y = r.unsqueeze(1) * _aggregate(A, c.unsqueeze(1) * H, round_operands)
    else:
        Y = _aggregate(A, H, round_operands)
    return Y + bias if bias is not None else Y


def dense_gin(A, X, W, round_operands=False):
    return _aggregate(A, X, round_operands) @ W


def dense_agnn(A, rp, col, X, W, w, round_operands=False):
    """the reference's AGNN layer: att = w <h_i, h_j> on the edges, NOT differentiated (the layer does not propagate through the scores)"""
    import torch
    rows, cols = torch.from_numpy(G._edge_rows(rp)).long(), torch.from_numpy(np.asarray(col)).long()
    H = X @ W
    Hs = G._round_tf32_t(H) if round_operands else H.detach()
    att = float(w.detach()) * (Hs[rows] * Hs[cols]).sum(1)
    if round_operands:
        att = G._round_tf32_t(att)
    Aatt = torch.zeros_like(A).index_put_((rows, cols), att, accumulate=True)
    return _aggregate(Aatt, H, round_operands)


def agnn_reference_dw(rp, col, dY):
    """(d attention_w, the scale it is judged on) of the reference's backward: <sddmm(dY), column ids>"""
    import torch
    rows, cols = torch.from_numpy(G._edge_rows(rp)).long(), torch.from_numpy(np.asarray(col)).long()
    s = (dY[rows] * dY[cols]).sum(1)
    return float((s * cols.double()).sum()), float((s.abs() * cols.double()).sum())


# ---- the wrong matrix ----------------------------------------------------------------------------------------------------------------------

def wrong_matrix_mode(A):
    """A torch function mode under which every product P @ Z whose left operand is an M x M matrix on A's support (A itself, a matrix
    of attention values) keeps its value and back-propagates to Z through P instead of P^T: the dense gradient of a layer whose
    backward aggregation takes the wrong matrix."""
    import torch
    from torch.overrides import TorchFunctionMode
    M = A.shape[0]
    off = A == 0

    class Wrong(torch.autograd.Function):
        @staticmethod
        def forward(ctx, P, Z):
            ctx.save_for_backward(P, Z)
            return P @ Z

        @staticmethod
        def backward(ctx, g):
            P, Z = ctx.saved_tensors
            return g @ Z.t(), P @ g

    class Mode(TorchFunctionMode):
        def __torch_function__(self, func, types, args=(), kwargs=None):
            if func in (torch.matmul, torch.Tensor.matmul, torch.Tensor.__matmul__, torch.mm, torch.Tensor.mm) and len(args) == 2:
                P, Z = args
                if (isinstance(P, torch.Tensor) and isinstance(Z, torch.Tensor) and P.dim() == 2 and Z.dim() == 2 and tuple(P.shape) == (M, M)
                        and Z.shape[0] == M and not bool(P.detach()[off].any())):
                    return Wrong.apply(P, Z)
            return func(*args, **(kwargs or {}))
    return Mode()


# ---- the layer table ----------------------------------------------------------------------------------------------------------------------

def _glorot(a, b):
    return (2.0 / (a + b)) ** 0.5


class Layer:
    """One layer configuration.  make(L): the module; attrs: its parameters in leaf order, each (attribute, shape, scale of the
    standard-normal leaf or, for a constant, ("fill", value)); dense(ctx, leaves, round_operands): the dense fp64 model on
    ctx = block_context(rp, col), leaves = [X, (edge_attr,) parameters ...]; checks: {"Y" | "grad" | leaf name: (metric, bound)};
    empty(module, X): the value rows without edges must hold exactly; plan_based: the layer aggregates through a plan (and A^T's);
    rounds: the dense model has the operand-rounding switch; data_scale: the scale of X and of dY (standard normal x data_scale)."""

    def __init__(self, name, make, attrs, dense, checks, empty, plan_based, rounds=False, out=OUT, wrong="mode", data_scale=1.0):
        self.name, self.make, self.attrs, self.dense, self.checks, self.empty = name, make, attrs, dense, checks, empty
        self.plan_based, self.rounds, self.out, self.wrong, self.data_scale = plan_based, rounds, out, wrong, data_scale

    def leaf_names(self):
        return ["X"] + (["edge_attr"] if self.name == "gine" else []) + [a for a, _, _ in self.attrs]

    def leaves(self, entry, M, eid=None):
        """(leaves, dY): seeded fp64 tensors; GINE's edge_attr rows are those of the full graph's edges the block kept (edge_attr[eid])"""
        import torch
        g = torch.Generator().manual_seed(zlib.crc32(("%s/%s" % (entry, self.name)).encode()))
        rnd = lambda *shape: torch.randn(*shape, dtype=torch.float64, generator=g)   # noqa: E731
        out = [rnd(M, INP) * self.data_scale]
        if self.name == "gine":
            full = rnd(len(full_graph()[1]), EDGE_DIM)
            out.append(full[torch.from_numpy(np.asarray(eid, dtype=np.int64))].clone())
        for _, shape, scale in self.attrs:
            out.append(torch.full(shape, float(scale[1]), dtype=torch.float64) if isinstance(scale, tuple) else rnd(*shape) * scale)
        return out, rnd(M, self.out) * self.data_scale

    def assign(self, module, leaves):
        """copies the parameter leaves into the module (fp32) -> its parameters in leaf order"""
        params = []
        for (attr, _, _), leaf in zip(self.attrs, leaves[len(leaves) - len(self.attrs):]):
            p = getattr(module, attr)
            p.data.copy_(leaf.float().reshape(p.shape))
            params.append(p)
        return params

    def check(self, leaf):
        """(metric, bound) of "Y" or of the gradient of a leaf"""
        return self.checks.get(leaf, self.checks["Y" if leaf == "Y" else "grad"])


def block_context(rp, col):
    ctx = types.SimpleNamespace(rp=np.asarray(rp), col=np.asarray(col), A=G.dense_adjacency(rp, col))
    ctx.B, ctx.Sel = EM.incidence(rp, col)
    return ctx


def _dense_transformer(ctx, lv, round_operands=False):
    layer = types.SimpleNamespace(weights_q=lv[1], bias_q=lv[2], weights_k=lv[3], bias_k=lv[4], weights_v=lv[5], bias_v=lv[6], weights_root=lv[7],
                                  bias=lv[8], concat=True)
    return HR.dense_transformer_model(ctx.A, lv[0], layer, HEADS)


def _zeros(module, X):
    import torch
    return torch.zeros(X.shape[0], OUT, dtype=X.dtype, device=X.device)


def _bias_rows(attr="bias"):
    return lambda module, X: getattr(module, attr).detach().unsqueeze(0).expand(X.shape[0], -1)


def _self_rows(weight, bias, rows=None):
    def value(module, X):
        import torch
        W = getattr(module, weight).detach()
        return torch.mm(X.detach(), W if rows is None else W[:rows]) + getattr(module, bias).detach()
    return value


WIDE = HEADS * OUT
_LARGEST = "largest"     # |got - want| against bound x the largest entry of want (gat_ref, stats_ref, edge_message_ref, segmax_ref)
_UNIT = "unit"           # ... against bound x max(1, the largest entry)  (tests/test_gpu_transpose.py)
_BAR = "bar"             # |got - want| / max(1, |want|) element by element  (tests/test_gpu_scaled_spmm.py)
_NORM = "norm"           # |got - want|_2 / |want|_2  (tests/test_gpu_transpose.py, the input gradient)
_ATT = [("Y", (_LARGEST, G.GPU_LAYER_TOL)), ("grad", (_LARGEST, G.GPU_LAYER_TOL))]
_BINARY = dict([("Y", (_UNIT, DIRECTED_GRAD_TOL)), ("grad", (_UNIT, DIRECTED_GRAD_TOL))])


def _sage(aggregator):
    tol_y, tol_g = SM.SAGE_TOL[aggregator]
    attrs = [("weights_self", (INP, OUT), _glorot(INP, OUT)), ("weights", (INP, OUT), _glorot(INP, OUT)), ("bias", (OUT,), 0.1)]
    if aggregator == "pool":
        attrs += [("weights_pool", (INP, INP), _glorot(INP, INP)), ("bias_pool", (INP,), 0.1)]
    return Layer("sage_" + aggregator, lambda L: L.SAGEConv(INP, OUT, aggregator=aggregator, directed=True), attrs,
                 lambda ctx, lv, round_operands=False: SM.dense_sage(ctx.A, lv[0], lv[1], lv[2], lv[3], aggregator, *lv[4:]),
                 {"Y": (_LARGEST, tol_y), "grad": (_LARGEST, tol_g)}, _self_rows("weights_self", "bias"), plan_based=aggregator == "mean",
                 wrong="mode" if aggregator == "mean" else "reversed")


LAYERS = [
    # (data_scale: the 1e-3 bar is absolute below 1 and stated for activations and gradients of O(1).  With standard-normal X and dY the
    #  layer's values reach 3.5 and its weight gradient, a sum over the block's rows, 40: operand rounding ALONE then uses 0.95 and 5.1 of
    #  the bar.  A fifth of each keeps both of O(1) - 0.9 and 1.7 at most - and the rounding within 0.42 of the bar)
    Layer("gcn_both_bias", lambda L: L.GCNConv(INP, OUT, norm="both", bias=True, directed=True),
          [("weights", (INP, OUT), _glorot(INP, OUT)), ("bias", (OUT,), 0.1)],
          lambda ctx, lv, round_operands=False: dense_gcn(ctx.A, lv[0], lv[1], lv[2], "both", round_operands),
          {"Y": (_BAR, GCN_TOL), "grad": (_BAR, GCN_TOL), "X": (_NORM, GCN_DX_NORM_TOL)}, _bias_rows(), plan_based=True, rounds=True, data_scale=0.2),
    Layer("gcn", lambda L: L.GCNConv(INP, OUT, directed=True), [("weights", (INP, OUT), _glorot(INP, OUT))],
          lambda ctx, lv, round_operands=False: dense_gcn(ctx.A, lv[0], lv[1], None, "none", round_operands), _BINARY, _zeros, plan_based=True, rounds=True),
    Layer("gin", lambda L: L.GINConv(INP, OUT, directed=True), [("weights", (INP, OUT), _glorot(INP, OUT))],
          lambda ctx, lv, round_operands=False: dense_gin(ctx.A, lv[0], lv[1], round_operands), _BINARY, _zeros, plan_based=True, rounds=True),
    # (attention_w: the constants tests/test_gpu_transpose.py and tests/test_gpu_edge_ops.py set; the reference layer's d attention_w is
    #  not a gradient of the model - agnn_reference_dw - and is judged apart)
    Layer("agnn", lambda L: L.AGNNConv(INP, OUT, directed=True), [("weights", (INP, OUT), _glorot(INP, OUT)), ("attention_w", (1, 1), ("fill", 0.3))],
          lambda ctx, lv, round_operands=False: dense_agnn(ctx.A, ctx.rp, ctx.col, lv[0], lv[1], lv[2], round_operands), _BINARY, _zeros, plan_based=True,
          rounds=True),
    Layer("agnn_softmax", lambda L: L.AGNNConv(INP, OUT, directed=True, attention="softmax"),
          [("weights", (INP, OUT), _glorot(INP, OUT)), ("attention_w", (1, 1), ("fill", 1.7))],
          lambda ctx, lv, round_operands=False: EO.dense_attention_model(ctx.A, lv[0], lv[1], lv[2]), dict(_ATT), _zeros, plan_based=True),
    Layer("gat", lambda L: L.GATConv(INP, OUT, heads=HEADS),
          [("weights", (INP, WIDE), _glorot(INP, WIDE)), ("attn_l", (1, HEADS, OUT), 0.5), ("attn_r", (1, HEADS, OUT), 0.5), ("bias", (WIDE,), 0.1)],
          lambda ctx, lv, round_operands=False: G.dense_gat_model(ctx.A, *lv, heads=HEADS, round_operands=round_operands), dict(_ATT), _bias_rows(),
          plan_based=True, rounds=True, out=WIDE),
    Layer("gatv2", lambda L: L.GATv2Conv(INP, OUT, heads=HEADS),
          [("weights", (INP, WIDE), _glorot(INP, WIDE)), ("weights_r", (INP, WIDE), _glorot(INP, WIDE)), ("attn", (1, HEADS, OUT), 0.5),
           ("bias", (WIDE,), 0.1)],
          lambda ctx, lv, round_operands=False: V.dense_gatv2_model(ctx.A, *lv, heads=HEADS, round_operands=round_operands), dict(_ATT), _bias_rows(),
          plan_based=True, rounds=True, out=WIDE),
    # (d bias_k is zero in exact arithmetic - the softmax drops a shift of every key - and is judged on the scale of d bias_q, as
    #  tests/test_gpu_sddmm_heads.py judges it)
    Layer("transformer", lambda L: L.TransformerConv(INP, OUT, heads=HEADS),
          [(k + n, s, c) for n in ("q", "k", "v") for k, s, c in (("weights_", (INP, WIDE), _glorot(INP, WIDE)), ("bias_", (WIDE,), 0.1))] +
          [("weights_root", (INP, WIDE), _glorot(INP, WIDE)), ("bias", (WIDE,), 0.1)],
          _dense_transformer, dict(_ATT), _self_rows("weights_root", "bias"), plan_based=True, out=WIDE),
    _sage("mean"), _sage("max"), _sage("pool"),
    Layer("pna", lambda L: L.PNAConv(INP, OUT, delta=1.0),
          [("weights_src", (INP, OUT), _glorot(INP, OUT)), ("weights_dst", (INP, OUT), _glorot(INP, OUT)), ("bias_pre", (OUT,), 0.1),
           ("weights_post", (INP + 12 * OUT, OUT), _glorot(INP + 12 * OUT, OUT)), ("bias_post", (OUT,), 0.1)],
          lambda ctx, lv, round_operands=False: ST.dense_pna(ctx.A, *lv, delta=1.0),
          {"Y": (_LARGEST, ST.LAYER_TOL_Y), "grad": (_LARGEST, ST.LAYER_TOL_G)}, _self_rows("weights_post", "bias_post", rows=INP), plan_based=False,
          wrong="reversed"),
    Layer("gine", lambda L: L.GINEConv(INP, OUT, edge_dim=EDGE_DIM),
          [("weights", (INP, OUT), _glorot(INP, OUT)), ("bias", (OUT,), 0.1), ("weights_edge", (EDGE_DIM, INP), _glorot(EDGE_DIM, INP)),
           ("bias_edge", (INP,), 0.1)],
          lambda ctx, lv, round_operands=False: EM.dense_gine(ctx.B, ctx.Sel, lv[0], lv[1], lv[2], lv[3], 0.0, lv[4], lv[5]),
          {"Y": (_LARGEST, EM.TOL_Y), "grad": (_LARGEST, EM.TOL_G)}, _self_rows("weights", "bias"), plan_based=False, wrong="reversed"),
]
LAYER = {c.name: c for c in LAYERS}


def reversed_context(ctx):
    """the block with every edge reversed (A^T), for the layers whose dense model has no matrix product to swap - the gather-based
    extrema, PNA, GINE: their input gradient on the reversed block stands in for the wrong-matrix one"""
    rp_t, col_t, perm = walks.transposed_csr(ctx.rp, ctx.col)
    return block_context(rp_t, col_t), perm


# ---- shares of a bound ---------------------------------------------------------------------------------------------------------------------

def share(metric, bound, got, want, top=None):
    """the share of its bound that `got` uses against `want` (fp64 torch tensors of one shape): <= 1 passes.  top: the largest entry the
    'largest' metric judges on, where that is not want's own.  A bound of zero (want is all zeros) is met by zeros only."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    if got.numel() == 0:
        return 0.0
    d = (got - want).abs()
    if metric == _BAR:
        return float((d / want.abs().clamp(min=1.0)).max()) / bound
    if metric == _NORM:
        err, limit = float(d.norm()), bound * float(want.norm())
    else:
        top = float(want.abs().max()) if top is None else top
        err, limit = float(d.max()), bound * (max(1.0, top) if metric == _UNIT else top)
    if limit == 0.0:
        return 0.0 if err == 0.0 else float("inf")
    return err / limit


def gradients(Y, dY, leaves):
    """the gradients of (Y * dY).sum() for every leaf, zeros where the output does not depend on one"""
    import torch
    got = torch.autograd.grad((Y * dY).sum(), leaves, allow_unused=True)
    return [torch.zeros_like(t) if g is None else g for g, t in zip(got, leaves)]


def shares(layer, names, got, want):
    """{name: share of its bound} for "Y" and every leaf's gradient; got / want: {name: tensor}"""
    out = {}
    for k in names:
        metric, bound = layer.check(k)
        top = float(want["bias_q"].abs().max()) if (layer.name == "transformer" and k == "bias_k") else None
        out[k] = share(metric, bound, got[k], want[k], top)
    return out
