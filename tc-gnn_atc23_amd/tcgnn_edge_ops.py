"""Differentiable edge operators over the TCGNN operator API - what an attention layer with a softmax over every node's incoming
edges is composed of (DGL's AGNNConv / edge_softmax; no counterpart in the reference's gnn_conv.py, whose AGNN layer aggregates with
unnormalised scores and does not propagate through them).  Every gradient is exact, on directed graphs as well:

    sddmm(X, Z, meta)             ef[e] = <X[row e], Z[col e]>            bwd: dX = A_val(d_ef) Z,  dZ = A_val(d_ef)^T X
    edge_softmax(s, rowptr, beta) p = softmax over each CSR row of beta s  bwd: g = p (dp - sum_row p dp); ds = beta g; dbeta = <s, g>
    aggregate(P, H, meta)         Y = A_val(P) H                           bwd: dP = sddmm(dY, H),  dH = A_val(P)^T dY
    gat_attention(el, er, rowptr, col, slope)  P[h] = softmax by row of leaky_relu(el[col e, h] + er[row e, h])   (multi-head GAT)
                                  bwd: g as above per head; ds = g lrelu'(raw); d_er = row sums of ds; d_el = column sums of ds
    gatv2_attention(xl, xr, attn, rowptr, col, slope)  P[h] = softmax by row of <attn[h], leaky_relu(xl[col e, head h] + xr[row e, head h])>   (GATv2)
                                  bwd: g as above per head; d_xr, d_attn by row and d_xl over A^T, from the backend's two GATv2 backward calls
    aggregate_heads(P, Z, meta)   Y[:, head h] = A_val(P[h]) Z[:, head h], all heads in one call   bwd: dP = sddmm_heads(dY, Z), dZ through A^T, one call each
    sddmm_heads(X, Z, meta, H)    ef[h, e] = <X[row e, head h], Z[col e, head h]>, [H, E], one call  bwd: dX = A_val(d_ef) Z, dZ = A_val(d_ef)^T X per head, one call each
    edge_softmax_heads(S, rowptr, beta)  edge_softmax of every row of S [H, E] (head by head on the one-head operator, one [H, E] result)
    aggregate_max(X, rowptr, col) Y[i, d] = max over row i of X[col e, d] (0 for an empty row)     bwd: dX[j, d] = sum of dY[i, d] over the edges that won (i, d)
    aggregate_stats(Z, rowptr, col, aggregators)  mean / std / max / min over row i of Z[col e, d], one gather for all (PNA)     bwd: one walk over A^T for all of them
    aggregate_ue(X, Ef, rowptr, col, act)  Y[i, d] = sum over row i of act(X[col e, d] + Ef[e, d]), Ef [E, D] (u_add_e; GINE)   bwd: dM = dY[row e] masked, once; dEf = dM, dX = sum of dM by source over A^T
    edge_sum(M, rowptr, col)      Y[i, d] = sum over row i of M[e, d], M [E, D] (copy_e)                        bwd: dM[e] = dY[row e]

`meta` is the five metadata tensors every operator of the API takes (row_pointers, column_index, blockPartition, edgeToColumn,
edgeToRow).  aggregate ALWAYS back-propagates through the transposed matrix, also on a structurally symmetric graph: softmax
weights are not symmetric (the backend then permutes the values over A's own plan).

The operators come from tcgnn_layers.backend(): forward_ef2, edge_softmax, edge_softmax_backward, forward_AGNN(transpose=),
forward_heads(transpose=), forward_ef_heads, forward_max, backward_max, forward_stats, backward_stats, forward_ue, backward_ue, edge_sum (with transpose_graph) and the gat_* / gatv2_* calls.  A backend without them is an error - there is no composed fallback in this module (a
stand-in backend installed with tcgnn_layers.set_backend is given forward_heads and forward_ef_heads there, by their per-head definitions, if it has none).
"""
import torch

import tcgnn_layers as _L


class _SDDMM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, Z, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow):
        ctx.meta = (row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow)
        X, Z = X.contiguous(), Z.contiguous()
        ctx.save_for_backward(X, Z)
        return _L.backend().forward_ef2(X, Z, *ctx.meta)[0]

    @staticmethod
    def backward(ctx, d_ef):
        X, Z = ctx.saved_tensors
        rp, col, bp, e2c, e2r = ctx.meta
        b = _L.backend()
        att = d_ef.contiguous().view(1, -1)
        d_x = b.forward_AGNN(Z, rp, col, att, bp, e2c, e2r)[0] if ctx.needs_input_grad[0] else None
        d_z = b.forward_AGNN(X, rp, col, att, bp, e2c, e2r, transpose=True)[0] if ctx.needs_input_grad[1] else None
        return (d_x, d_z) + (None,) * 5


class _EdgeSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, score, row_pointers, beta):
        score = score.contiguous()
        b1 = beta.detach().reshape(1).contiguous() if beta is not None else None
        p = _L.backend().edge_softmax(score, row_pointers, b1)
        ctx.rowptr = row_pointers
        ctx.has_beta = beta is not None
        ctx.beta_shape = beta.shape if beta is not None else None
        # (the scores - E floats - are kept only where d_beta = sum s g can be asked for)
        ctx.want_beta = ctx.has_beta and beta.requires_grad
        ctx.save_for_backward(*([p] + ([b1] if ctx.has_beta else []) + ([score] if ctx.want_beta else [])))
        return p

    @staticmethod
    def backward(ctx, d_p):
        saved = list(ctx.saved_tensors)
        p = saved.pop(0)
        b1 = saved.pop(0) if ctx.has_beta else None
        score = saved.pop(0) if ctx.want_beta else None
        want_beta = ctx.want_beta and ctx.needs_input_grad[2]
        d_s, d_beta = _L.backend().edge_softmax_backward(p, d_p.contiguous(), ctx.rowptr, beta=b1, score=score if want_beta else None,
                                                         need_dbeta=want_beta)
        return (d_s if ctx.needs_input_grad[0] else None, None, d_beta.reshape(ctx.beta_shape).to(d_s.dtype) if want_beta else None)


class _Aggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, P, H, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow):
        ctx.meta = (row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow)
        P, H = P.contiguous(), H.contiguous()
        ctx.save_for_backward(P, H)
        return _L.backend().forward_AGNN(H, row_pointers, column_index, P.view(1, -1), blockPartition, edgeToColumn, edgeToRow)[0]

    @staticmethod
    def backward(ctx, d_y):
        P, H = ctx.saved_tensors
        rp, col, bp, e2c, e2r = ctx.meta
        b = _L.backend()
        d_y = d_y.contiguous()
        d_p = b.forward_ef2(d_y, H, *ctx.meta)[0] if ctx.needs_input_grad[0] else None
        d_h = b.forward_AGNN(d_y, rp, col, P.view(1, -1), bp, e2c, e2r, transpose=True)[0] if ctx.needs_input_grad[1] else None
        return (d_p, d_h) + (None,) * 5


class _GATAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, el, er, row_pointers, column_index, negative_slope):
        el, er = el.contiguous(), er.contiguous()
        p = _L.backend().gat_softmax(el, er, row_pointers, column_index, negative_slope)
        ctx.graph = (row_pointers, column_index)
        ctx.slope = negative_slope
        ctx.save_for_backward(p, el, er)
        return p

    @staticmethod
    def backward(ctx, d_p):
        p, el, er = ctx.saved_tensors
        b = _L.backend()
        d_p = d_p.contiguous()
        ds, d_er = b.gat_softmax_backward(p, d_p, el, er, *ctx.graph, ctx.slope)
        d_el = b.edge_colsum(ds, *ctx.graph) if ctx.needs_input_grad[0] else None
        return d_el, (d_er if ctx.needs_input_grad[1] else None), None, None, None


class _GATv2Attention(torch.autograd.Function):
    """P = gatv2_softmax(xl, xr, attn); (g, d_xr, d_attn) = gatv2_softmax_backward, d_xl = gatv2_source_grad(g) over A^T.  shared: xl and xr
    are ONE tensor (a layer with share_weights), given once - its gradient is the sum of both sides."""

    @staticmethod
    def forward(ctx, xl, xr, attn, row_pointers, column_index, negative_slope, shared):
        xl = xl.contiguous()
        xr = xl if shared else xr.contiguous()
        attn = attn.contiguous()
        p = _L.backend().gatv2_softmax(xl, xr, attn, row_pointers, column_index, negative_slope)
        ctx.graph = (row_pointers, column_index)
        ctx.slope, ctx.shared = negative_slope, shared
        ctx.save_for_backward(*((p, xl, attn) if shared else (p, xl, attn, xr)))
        return p

    @staticmethod
    def backward(ctx, d_p):
        p, xl, attn = ctx.saved_tensors[:3]
        xr = xl if ctx.shared else ctx.saved_tensors[3]
        b = _L.backend()
        g, d_xr, d_attn = b.gatv2_softmax_backward(p, d_p.contiguous(), xl, xr, attn, *ctx.graph, ctx.slope)
        d_xl = b.gatv2_source_grad(g, xl, xr, attn, *ctx.graph, ctx.slope) if ctx.needs_input_grad[0] else None
        if ctx.shared:
            return (d_xl + d_xr if d_xl is not None else None), None, (d_attn if ctx.needs_input_grad[2] else None), None, None, None, None
        return d_xl, (d_xr if ctx.needs_input_grad[1] else None), (d_attn if ctx.needs_input_grad[2] else None), None, None, None, None


class _AggregateHeads(torch.autograd.Function):
    """Y = forward_heads(Z, P): one call for all heads, and one over A^T for dZ.  dP [heads, E] is ONE forward_ef_heads(dY, Z) call, the
    multi-head SDDMM (a stand-in backend without it was given the per-head definition by tcgnn_layers.set_backend)."""

    @staticmethod
    def forward(ctx, P, Z, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow):
        ctx.meta = (row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow)
        P, Z = P.contiguous(), Z.contiguous()
        ctx.save_for_backward(P, Z)
        rp, col, bp, e2c, e2r = ctx.meta
        return _L.backend().forward_heads(Z, rp, col, P, bp, e2c, e2r, P.shape[0])[0]

    @staticmethod
    def backward(ctx, d_y):
        P, Z = ctx.saved_tensors
        b = _L.backend()
        H = P.shape[0]
        d_y = d_y.contiguous()
        d_p = d_z = None
        if ctx.needs_input_grad[0]:
            d_p = b.forward_ef_heads(d_y, Z, *ctx.meta, H)[0]
        if ctx.needs_input_grad[1]:
            rp, col, bp, e2c, e2r = ctx.meta
            d_z = b.forward_heads(d_y, rp, col, P, bp, e2c, e2r, H, transpose=True)[0]
        return (d_p, d_z) + (None,) * 5


def _into(row, result):
    """`result` is `row` where the backend wrote through out= (TCGNN, the binding); a stand-in that returns a tensor of its own is copied"""
    if result.data_ptr() != row.data_ptr():
        row.copy_(result)


class _SDDMMHeads(torch.autograd.Function):
    """ef = forward_ef_heads(X, Z): one call for all heads; dX = forward_heads(Z, d_ef) and dZ = forward_heads(X, d_ef) over A^T, one call each."""

    @staticmethod
    def forward(ctx, X, Z, heads, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow):
        ctx.meta = (row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow)
        ctx.heads = heads
        X, Z = X.contiguous(), Z.contiguous()
        ctx.save_for_backward(X, Z)
        return _L.backend().forward_ef_heads(X, Z, *ctx.meta, heads)[0]

    @staticmethod
    def backward(ctx, d_ef):
        X, Z = ctx.saved_tensors
        rp, col, bp, e2c, e2r = ctx.meta
        b = _L.backend()
        d_ef = d_ef.contiguous()
        d_x = b.forward_heads(Z, rp, col, d_ef, bp, e2c, e2r, ctx.heads)[0] if ctx.needs_input_grad[0] else None
        d_z = b.forward_heads(X, rp, col, d_ef, bp, e2c, e2r, ctx.heads, transpose=True)[0] if ctx.needs_input_grad[1] else None
        return (d_x, d_z) + (None,) * 6


class _EdgeSoftmaxHeads(torch.autograd.Function):
    """edge_softmax of every head's row of S [H, E] with one beta (a constant: no d_beta), written into one [H, E] tensor through out="""

    @staticmethod
    def forward(ctx, S, row_pointers, beta):
        S = S.contiguous()
        b1 = beta.detach().reshape(1).contiguous() if beta is not None else None
        b = _L.backend()
        P = torch.empty_like(S)
        for h in range(S.shape[0]):
            _into(P[h], b.edge_softmax(S[h], row_pointers, b1, out=P[h]))
        ctx.rowptr = row_pointers
        ctx.has_beta = b1 is not None
        ctx.save_for_backward(*([P] + ([b1] if ctx.has_beta else [])))
        return P

    @staticmethod
    def backward(ctx, d_p):
        P = ctx.saved_tensors[0]
        b1 = ctx.saved_tensors[1] if ctx.has_beta else None
        b = _L.backend()
        d_p = d_p.contiguous()
        d_s = torch.empty_like(P)
        for h in range(P.shape[0]):
            _into(d_s[h], b.edge_softmax_backward(P[h], d_p[h], ctx.rowptr, beta=b1, out=d_s[h])[0])
        return d_s, None, None


class _AggregateMax(torch.autograd.Function):
    """Y = forward_max(X); the winning CSR positions (int32 [N, D]) are what is saved - X is not needed again."""

    @staticmethod
    def forward(ctx, X, row_pointers, column_index):
        Y, arg = _L.backend().forward_max(X.contiguous(), row_pointers, column_index)
        ctx.graph = (row_pointers, column_index)
        ctx.save_for_backward(arg)
        return Y

    @staticmethod
    def backward(ctx, d_y):
        arg, = ctx.saved_tensors
        d_x = _L.backend().backward_max(d_y.contiguous(), arg, *ctx.graph) if ctx.needs_input_grad[0] else None
        return d_x, None, None


def aggregate_max(X, row_pointers, column_index):
    """Y[i, d] = the maximum of X[col e, d] over the edges e of CSR row i (a node's incoming edges); a row without edges gives 0.
    Exact (fp32 in, the winner's bits out); among equal values the first edge of the row wins, and only it receives the gradient:
    dX[j, d] = the sum of dY[i, d] over the edges (i <- j) that won element (i, d) - a fixed-order walk over A^T, no atomics."""
    return _AggregateMax.apply(X, row_pointers, column_index)


class _AggregateStats(torch.autograd.Function):
    """forward_stats(Z) of the named aggregators; saved: Z, mean and std (where std is asked for) and the args - nothing of size E."""

    @staticmethod
    def forward(ctx, Z, row_pointers, column_index, names, eps):
        Z = Z.contiguous()
        # (the gradient of std needs the mean: one more output of the same walk)
        asked = names + (("mean",) if "std" in names and "mean" not in names else ())
        r = _L.backend().forward_stats(Z, row_pointers, column_index, aggregators=asked, eps=eps)
        ctx.graph, ctx.names = (row_pointers, column_index), names
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(Z, *(r.get(k) if k in ("argmax", "argmin") or "std" in names else None for k in ("mean", "std", "argmax", "argmin")))
        return tuple(r[a] for a in names)

    @staticmethod
    def backward(ctx, *d):
        if not ctx.needs_input_grad[0]:
            return (None,) * 5
        Z, mean, std, argmax, argmin = ctx.saved_tensors
        grads = {a: g.contiguous() for a, g in zip(ctx.names, d) if g is not None}
        saved = {"Z": Z, "mean": mean, "std": std, "argmax": argmax, "argmin": argmin}
        return (_L.backend().backward_stats(grads, saved, *ctx.graph),) + (None,) * 4


def aggregate_stats(Z, row_pointers, column_index, aggregators=("mean", "std", "max", "min"), eps=1e-5):
    """PNA's aggregators over the edges of every CSR row (a node's incoming edges) from one gather of the neighbour rows: a tuple of
    [N, D] tensors in the order of `aggregators` (among 'mean', 'std', 'max', 'min'; std = sqrt(max(var, 0) + eps), population
    variance).  A row without edges gives 0 in every one.  max and min are exact and send their gradient to the first edge that
    holds the value; the backward is one fixed-order walk over A^T for all of them (the backend's backward_stats), no atomics."""
    names = (aggregators,) if isinstance(aggregators, str) else tuple(aggregators)
    if not names or len(set(names)) != len(names) or any(a not in ("mean", "std", "max", "min") for a in names):
        raise ValueError("aggregators must be distinct names among mean, std, max, min, got %r" % (aggregators,))
    return _AggregateStats.apply(Z, row_pointers, column_index, names, float(eps))


class _AggregateUE(torch.autograd.Function):
    """Y = forward_ue(X, Ef); backward: dM = backward_ue(dY) ONCE - it is dEf, and dX = edge_sum(dM) over A^T through perm.  Saved: X
    and Ef under ReLU (the mask is recomputed from them); nothing under the identity."""

    @staticmethod
    def forward(ctx, X, Ef, row_pointers, column_index, act):
        X, Ef = X.contiguous(), Ef.contiguous()
        ctx.graph, ctx.act = (row_pointers, column_index), act
        if act == "relu":
            ctx.save_for_backward(X, Ef)
        return _L.backend().forward_ue(X, Ef, row_pointers, column_index, act=act)

    @staticmethod
    def backward(ctx, d_y):
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return (None,) * 5
        X, Ef = ctx.saved_tensors if ctx.act == "relu" else (None, None)
        b = _L.backend()
        d_m = b.backward_ue(d_y.contiguous(), X, Ef, *ctx.graph, act=ctx.act)
        d_x = None
        if ctx.needs_input_grad[0]:
            rp_t, _, perm, _ = b.transpose_graph(*ctx.graph)
            d_x = b.edge_sum(d_m, rp_t, perm)
        return d_x, (d_m if ctx.needs_input_grad[1] else None), None, None, None


def aggregate_ue(X, Ef, row_pointers, column_index, act="relu"):
    """Y[i, d] = the sum over the edges e of CSR row i of act(X[col e, d] + Ef[e, d]): message passing with a feature vector per edge
    (DGL's u_add_e / sum; act 'relu': GINEConv's message, 'identity' or None: the plain sum).  X: [N, D], Ef: [E, D] in CSR position
    order.  One fused walk, no [E, D] tensor going forward; going back the per-edge gradient dM [E, D] is made once - it IS dEf - and
    dX is its sum by source node, one row-granular read of dM over A^T.  fp64 sums in a fixed order, no atomics; exact on any graph."""
    if act not in ("relu", "identity", None):
        raise ValueError("act must be 'relu', 'identity' or None, got %r" % (act,))
    if X.dim() != 2 or Ef.dim() != 2 or Ef.shape[0] != column_index.numel() or Ef.shape[1] != X.shape[1]:
        raise RuntimeError("X must be [N, D] and Ef [E, D] = [%d, %d], got %s and %s" % (column_index.numel(), X.shape[-1], tuple(X.shape), tuple(Ef.shape)))
    return _AggregateUE.apply(X, Ef, row_pointers, column_index, "relu" if act == "relu" else "identity")


class _EdgeSum(torch.autograd.Function):
    """Y = edge_sum(M) by destination node; dM[e] = dY[row e]: backward_ue without an activation."""

    @staticmethod
    def forward(ctx, M, row_pointers, column_index):
        ctx.graph = (row_pointers, column_index)
        return _L.backend().edge_sum(M.contiguous(), row_pointers)

    @staticmethod
    def backward(ctx, d_y):
        d_m = _L.backend().backward_ue(d_y.contiguous(), None, None, *ctx.graph, act=None) if ctx.needs_input_grad[0] else None
        return d_m, None, None


def edge_sum(M, row_pointers, column_index):
    """Y[i, d] = the sum of M[e, d] over the edges e of CSR row i (DGL's copy_e / sum): per-edge rows [E, D] in CSR position order summed
    into their destination nodes, fp64 in a fixed order; a row without edges gives 0.  bwd: dM[e] = dY[row e]."""
    if M.dim() != 2 or M.shape[0] != column_index.numel():
        raise RuntimeError("M must be [E, D] with E = %d, got %s" % (column_index.numel(), tuple(M.shape)))
    return _EdgeSum.apply(M, row_pointers, column_index)


def gat_attention(el, er, row_pointers, column_index, negative_slope=0.2):
    """P[h, e] = softmax over every CSR row of leaky_relu(el[col e, h] + er[row e, h]): GAT's attention, [heads, E] (head-major: P[h] is
    what aggregate takes).  el / er: [N, heads].  bwd: (ds, d_er) from the backend's gat_softmax_backward, d_el = edge_colsum(ds)."""
    return _GATAttention.apply(el, er, row_pointers, column_index, float(negative_slope))


def gatv2_attention(xl, xr, attn, row_pointers, column_index, negative_slope=0.2):
    """P[h, e] = softmax over every CSR row of sum_f attn[h, f] leaky_relu(xl[col e, hF + f] + xr[row e, hF + f]): GATv2's attention,
    [heads, E] head-major (what aggregate_heads takes).  xl / xr: [N, heads * F], attn: [heads, F].  One fused kernel forward (no
    [E, heads * F] tensor), two backward: (g, d_xr, d_attn) by row, d_xl over A^T - exact on any graph.  When xl and xr are the same
    tensor its gradient is the sum of both sides."""
    if attn.dim() != 2 or xl.dim() != 2 or xl.shape != xr.shape or xl.shape[1] != attn.shape[0] * attn.shape[1]:
        raise RuntimeError("xl and xr must be [N, heads * F] and attn [heads, F], got %s, %s and %s" % (tuple(xl.shape), tuple(xr.shape), tuple(attn.shape)))
    shared = xl is xr
    return _GATv2Attention.apply(xl, None if shared else xr, attn, row_pointers, column_index, float(negative_slope), shared)


def aggregate_heads(P, Z, meta):
    """Y[:, hF:(h+1)F] = A_val(P[h]) Z[:, hF:(h+1)F] for P [heads, E] and Z [N, heads * F]: the multi-head aggregation, one
    forward_heads call of the backend (the library's multi-head edge-valued SpMM: one gather feeds every head where its fused walk
    covers the shape).  dZ is one forward_heads call over A^T, dP one forward_ef_heads call (the multi-head SDDMM); both exact."""
    if P.dim() != 2 or Z.dim() != 2 or P.shape[0] < 1 or Z.shape[1] % P.shape[0]:
        raise RuntimeError("P must be [heads, E] and Z [N, heads * F], got %s and %s" % (tuple(P.shape), tuple(Z.shape)))
    return _AggregateHeads.apply(P, Z, *meta)


def sddmm_heads(X, Z, meta, heads):
    """ef[h, e] = <X[row e, hF:(h+1)F], Z[col e, hF:(h+1)F]> for X, Z [N, heads * F]: the scores of multi-head dot-product attention,
    [heads, E] head-major, one forward_ef_heads call of the backend (the library's multi-head SDDMM: one gather feeds every head's
    dot product where its fused walk covers the shape).  dX and dZ are one forward_heads call each (dZ over A^T); both exact."""
    heads = int(heads)
    if X.dim() != 2 or X.shape != Z.shape or heads < 1 or X.shape[1] % heads:
        raise RuntimeError("X and Z must both be [N, heads * F], got %s and %s for %d heads" % (tuple(X.shape), tuple(Z.shape), heads))
    return _SDDMMHeads.apply(X, Z, heads, *meta)


def edge_softmax_heads(S, row_pointers, beta=None):
    """softmax of beta * S[h] over every CSR row, for every head h of S [heads, E]; beta: a one-element CONSTANT tensor (a scale such
    as 1 / sqrt(F): it gets no gradient) or None = 1.  Head by head on the one-head operator, into one [heads, E] tensor."""
    if S.dim() != 2:
        raise RuntimeError("S must be [heads, E], got %s" % (tuple(S.shape),))
    return _EdgeSoftmaxHeads.apply(S, row_pointers, beta)


def sddmm(X, Z, meta):
    """ef[e] = <X[row e], Z[col e]> for every CSR edge, differentiable in both operands."""
    return _SDDMM.apply(X, Z, *meta)


def edge_softmax(score, row_pointers, beta=None):
    """softmax of beta * score over every CSR row (a node's incoming edges); beta: a one-element tensor (a Parameter) or None = 1."""
    return _EdgeSoftmax.apply(score, row_pointers, beta)


def aggregate(P, H, meta):
    """Y = A_val(P) H with A_val[row e, col e] = P[e], differentiable in the edge values and in H."""
    return _Aggregate.apply(P, H, *meta)
