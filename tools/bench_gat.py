#!/usr/bin/env python3
"""Multi-head GAT attention: one JSON line per measurement.
Graphs: sbm_reddit, R-MAT at the Reddit shape, and an SBM graph at the ogbn-products shape; (heads, features per head) = (8, 8) and
(4, 32).  Times are HIP-event medians of 30 calls after 5 warm-up calls (the composition: 10 after 2; epochs: tcgnn_harness.time_training):
  gat_softmax     the fused forward, the fused backward (ds and d_er) and edge_colsum (d_el), each against the torch composition on the same
                  box - row ids from repeat_interleave (built outside the timed region), two row gathers (H one-dimensional gathers each
                  where torch's row gather does not agree with them: checked per call) and leaky_relu into an [H, E] score array, H calls of TCGNN.edge_softmax; backward: H calls of TCGNN.edge_softmax_backward, the leaky_relu mask, index_add_
                  over the rows for d_er; index_add_ over the SOURCE nodes for d_el - and the forward against the HBM roofline B / 8 TB/s,
                  B = 4 (N + 1) + 4 E + 8 N H + 4 H E
  aggregate       aggregate_heads (ONE multi-head edge-valued SpMM, forward; forward + backward) against ONE binary forward at width H F;
                  heads_walk names the kernel the multi-head call ran
  sddmm           forward_ef_heads (ONE multi-head SDDMM) against the loop it replaces - H forward_ef2 calls on contiguous copies of the
                  heads' column blocks, stacked - and aggregate_heads' dP alone (backward with respect to the edge values only);
                  sddmm_walk names the kernel the multi-head call ran.  (forward_ef_heads_ms is null on a tree from before the call
                  existed: the tool is run on the parent commit's tree as well, for the A/B figures of DESIGN.md 4.11)
  epoch           a GAT epoch and a TransformerConv epoch, 2 layers, hidden = H F
    python tools/bench_gat.py [--epochs K] [--skip-epochs] [--skip-attention] [--graphs a,b] [--configs 8x8,4x32,2x64]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tc-gnn_atc23_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import TCGNN  # noqa: E402
import tcgnn_edge_ops as E_ops  # noqa: E402
import tcgnn_graph as G  # noqa: E402
import tcgnn_harness as H  # noqa: E402

PEAK_BYTES_PER_MS = 8e12 / 1e3
CONFIGS = ((8, 8), (4, 32))
SLOPE = 0.2


def emit(**kw):
    print(json.dumps(kw), flush=True)


def translate(rp, col, n, dev):
    E = col.numel()
    bp = torch.zeros((n + 15) // 16, dtype=torch.int32, device=dev); e2c = torch.zeros(E, dtype=torch.int32, device=dev); e2r = torch.zeros(E, dtype=torch.int32, device=dev)
    TCGNN.preprocess_gpu(col, rp, n, 16, 8, bp, e2c, e2r)
    return (rp, col, bp, e2c, e2r)


def median_ms(fn, reps=30, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2]


def gather_rows(x, idx):
    """x[idx] for x [N, H]: torch's row gather"""
    return x[idx]


def gather_per_head(x, idx):
    """the same as H one-dimensional gathers (what the composition falls back to where the row gather does not agree with them)"""
    xt = x.t().contiguous()
    return torch.stack([xt[h][idx] for h in range(xt.shape[0])], dim=1)


def torch_forward(el, er, rp, rows, cols, gather=gather_rows):
    s = F.leaky_relu(gather(el, cols) + gather(er, rows), SLOPE).t().contiguous()          # [H, E]: written and read again
    return torch.stack([TCGNN.edge_softmax(s[h], rp) for h in range(s.shape[0])])


def torch_backward(p, dp, el, er, rp, rows, cols, gather=gather_rows):
    raw = (gather(el, cols) + gather(er, rows)).t()
    g = torch.stack([TCGNN.edge_softmax_backward(p[h], dp[h], rp)[0] for h in range(p.shape[0])])
    ds = torch.where(raw > 0, g, g * SLOPE)
    return ds, torch.zeros_like(er).index_add_(0, rows, ds.t())


def torch_colsum(ds, cols, n):
    return torch.zeros(n, ds.shape[0], device=ds.device).index_add_(0, cols, ds.t())


def attention_times(graph, n, rp, col, heads, dev):
    E = col.numel()
    g = torch.Generator(device=dev).manual_seed(heads)
    el, er = torch.randn(n, heads, device=dev, generator=g), torch.randn(n, heads, device=dev, generator=g)
    dp = torch.randn(heads, E, device=dev, generator=g)
    p, ds = torch.empty(heads, E, device=dev), torch.empty(heads, E, device=dev)
    TCGNN.edge_colsum(dp, rp, col)   # (the transposed CSR: built once per graph, outside the timed region)
    t_f = median_ms(lambda: TCGNN.gat_softmax(el, er, rp, col, SLOPE, out=p))
    t_b = median_ms(lambda: TCGNN.gat_softmax_backward(p, dp, el, er, rp, col, SLOPE, out=ds))
    t_c = median_ms(lambda: TCGNN.edge_colsum(ds, rp, col))
    lens = (rp[1:] - rp[:-1]).long()
    rows, cols = torch.repeat_interleave(torch.arange(n, device=dev), lens), col.long()
    # the composition's row gather x[idx] of an [N, H] matrix is checked against H one-dimensional gathers first: where they disagree
    # (on the torch build this was written with: H = 4 - 16-byte rows - with 1e8 indices) the composition is timed, and
    # compared, with the one-dimensional gathers; the line records which
    rows_ok = all(torch.equal(gather_rows(x, i), gather_per_head(x, i)) for x, i in ((el, cols), (er, rows)))
    gather = gather_rows if rows_ok else gather_per_head
    t_cf = median_ms(lambda: torch_forward(el, er, rp, rows, cols, gather), reps=10, warmup=2)
    t_cb = median_ms(lambda: torch_backward(p, dp, el, er, rp, rows, cols, gather), reps=10, warmup=2)
    t_cc = median_ms(lambda: torch_colsum(ds, cols, n), reps=5, warmup=1)
    err = float((torch_forward(el, er, rp, rows, cols, gather) - p).abs().max())
    ds_t, der_t = torch_backward(p, dp, el, er, rp, rows, cols, gather)
    _, der = TCGNN.gat_softmax_backward(p, dp, el, er, rp, col, SLOPE, out=ds)
    err_b = max(float((ds_t - ds).abs().max()), float((der_t - der).abs().max()))
    err_c = float((torch_colsum(ds, cols, n) - TCGNN.edge_colsum(ds, rp, col)).abs().max())
    bf = 4 * (n + 1) + 4 * E + 8 * n * heads + 4 * heads * E
    bb = 4 * (n + 1) + 4 * E + 12 * n * heads + 12 * heads * E
    bc = 4 * (n + 1) + 4 * E + 4 * n * heads + 4 * heads * E
    emit(graph=graph, what="gat_softmax", heads=heads, forward_ms=t_f, backward_ms=t_b, colsum_ms=t_c, torch_forward_ms=t_cf, torch_backward_ms=t_cb,
         torch_colsum_ms=t_cc, torch_row_gather_agrees_with_per_head_gathers=rows_ok, index_bytes_of_the_composition=(rows.numel() + cols.numel()) * 8, roofline_forward_ms=bf / PEAK_BYTES_PER_MS,
         roofline_backward_ms=bb / PEAK_BYTES_PER_MS, roofline_colsum_ms=bc / PEAK_BYTES_PER_MS, forward_GBps=bf / t_f / 1e6,
         backward_GBps=bb / t_b / 1e6, colsum_GBps=bc / t_c / 1e6, longest_row=int(lens.max()), max_abs_difference_from_torch=err,
         max_abs_backward_difference_from_torch=err_b, max_abs_colsum_difference_from_torch=err_c)


def aggregate_times(graph, n, meta, heads, feat, dev):
    E = meta[1].numel()
    g = torch.Generator(device=dev).manual_seed(feat)
    P = torch.rand(heads, E, device=dev, generator=g)
    Z = torch.randn(n, heads * feat, device=dev, generator=g)
    dY = torch.randn(n, heads * feat, device=dev, generator=g)
    with torch.no_grad():
        t_h = median_ms(lambda: E_ops.aggregate_heads(P, Z, meta))
        walk_h = TCGNN.last_kernel(*meta)
        t_1 = median_ms(lambda: TCGNN.forward(Z, *meta))
        walk_1 = TCGNN.last_kernel(*meta)

    def both():
        p, z = P.detach().requires_grad_(True), Z.detach().requires_grad_(True)
        torch.autograd.grad(E_ops.aggregate_heads(p, z, meta), (p, z), dY)
    t_hb = median_ms(both, reps=10, warmup=3)
    emit(graph=graph, what="aggregate", heads=heads, features=feat, aggregate_heads_ms=t_h, binary_forward_ms=t_1, ratio=t_h / t_1,
         aggregate_heads_forward_backward_ms=t_hb, binary_walk=walk_1, heads_walk=walk_h)


def sddmm_times(graph, n, meta, heads, feat, dev):
    E = meta[1].numel()
    g = torch.Generator(device=dev).manual_seed(feat + 1)
    X = torch.randn(n, heads * feat, device=dev, generator=g)
    Z = torch.randn(n, heads * feat, device=dev, generator=g)
    P = torch.rand(heads, E, device=dev, generator=g)

    def per_head():
        return torch.stack([TCGNN.forward_ef2(X[:, h * feat:(h + 1) * feat].contiguous(), Z[:, h * feat:(h + 1) * feat].contiguous(), *meta)[0] for h in range(heads)])
    fused = getattr(TCGNN, "forward_ef_heads", None)
    with torch.no_grad():
        t_loop = median_ms(per_head)
        walk_1 = TCGNN.last_kernel(*meta)
        t_heads = median_ms(lambda: fused(X, Z, *meta, heads)) if fused else None
        walk_h = TCGNN.last_kernel(*meta) if fused else None
        diff = float((fused(X, Z, *meta, heads)[0] - per_head()).abs().max()) if fused else None

    def dp_only():
        p = P.detach().requires_grad_(True)
        torch.autograd.grad(E_ops.aggregate_heads(p, Z, meta), (p,), X)
    with torch.no_grad():
        t_fwd = median_ms(lambda: E_ops.aggregate_heads(P, Z, meta), reps=10, warmup=3)
    t_dp = median_ms(dp_only, reps=10, warmup=3) - t_fwd
    emit(graph=graph, what="sddmm", heads=heads, features=feat, forward_ef_heads_ms=t_heads, per_head_forward_ef2_ms=t_loop, aggregate_heads_dP_ms=t_dp,
         sddmm_walk=walk_h, per_head_walk=walk_1, max_abs_difference_from_the_per_head_loop=diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--skip-epochs", action="store_true")
    ap.add_argument("--skip-attention", action="store_true", help="leave out the gat_softmax measurements and their torch compositions")
    ap.add_argument("--graphs", type=str, default="sbm_reddit,rmat_reddit,sbm_products")
    ap.add_argument("--configs", type=str, default=",".join("%dx%d" % c for c in CONFIGS), help="heads x features per head, e.g. 8x8,4x32,2x64")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    table = {"sbm_reddit": ("reddit", "sbm_reddit"), "rmat_reddit": ("reddit", "rmat"), "sbm_products": ("ogbn-products", "sbm")}
    for graph in args.graphs.split(","):
        shape, gen = table[graph]
        n, nnz, in_dim, classes = G.SHAPES[shape]
        rp, col = G.GENERATORS[gen](n, nnz, seed=0, device=dev)
        emit(graph=graph, what="graph", num_nodes=n, num_edges=col.numel())
        meta = translate(rp, col, n, dev)
        for heads, feat in [tuple(int(v) for v in c.split("x")) for c in args.configs.split(",")]:
            TCGNN.prepare([feat, heads * feat], *meta, transpose=True, edge_valued=True, attention=True)
            TCGNN.prepare([feat], *meta, transpose=True, edge_valued=True, heads=heads)
            if not args.skip_attention:
                with torch.no_grad():
                    attention_times(graph, n, rp, col, heads, dev)
                torch.cuda.empty_cache()
            aggregate_times(graph, n, meta, heads, feat, dev)
            torch.cuda.empty_cache()
            sddmm_times(graph, n, meta, heads, feat, dev)
            torch.cuda.empty_cache()
            if not args.skip_epochs:
                x = torch.randn(n, in_dim, device=dev)
                y = torch.randint(0, classes, (n,), device=dev)
                r = H.time_training("gat", meta, x, y, in_dim, heads * feat, classes, 2, args.epochs, heads=heads)
                emit(graph=graph, what="epoch", model="gat", heads=heads, features=feat, hidden=heads * feat, train_ms=r["train_ms"], final_loss=r["final_loss"])
                if hasattr(TCGNN, "forward_ef_heads"):
                    r = H.time_training("transformer", meta, x, y, in_dim, heads * feat, classes, 2, args.epochs, heads=heads)
                    emit(graph=graph, what="epoch", model="transformer", heads=heads, features=feat, hidden=heads * feat, train_ms=r["train_ms"], final_loss=r["final_loss"])
                del x, y
                torch.cuda.empty_cache()
        TCGNN.clear_plan_cache()
        del meta, rp, col
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
