#!/usr/bin/env python3
"""GATv2 attention: one JSON line per measurement.
Graphs: sbm_reddit, R-MAT at the Reddit shape, and an SBM graph at the ogbn-products shape; (heads, features per head) = (8, 8) and
(4, 32).  Times are HIP-event medians of 20 calls after 3 warm-up calls (the composition: 3 after 1):
  gatv2_softmax   the fused forward (tcgnn_gatv2_softmax) and the fused backward as its two calls - by row (g, d_xr, d_attn) and by source
                  (d_xl over A^T) - each with the gather bound E H F 4 bytes over the measured time (what the neighbour rows alone would
                  cost at that rate; HBM's 8 TB/s for comparison), against, in the same run,
  composition     torch: xl[col] + xr[row] - an [E, H F] tensor -, leaky_relu, the dot product with attn, edge_softmax_heads; forward
                  alone, and forward + autograd backward with respect to xl, xr and attn.  Where it runs out of memory the line says so.
  gat             gat_softmax / gat_softmax_backward + edge_colsum at the same head count: the additive scores, whose per-edge work is
                  two 4 H-byte gathers instead of one 4 H F-byte row.
    python tools/bench_gatv2.py [--graphs a,b] [--configs 8x8,4x32] [--skip-composition]"""
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

PEAK_BYTES_PER_MS = 8e12 / 1e3
CONFIGS = ((8, 8), (4, 32))
SLOPE = 0.2


def emit(**kw):
    print(json.dumps(kw), flush=True)


def median_ms(fn, reps=20, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2]


def composition(xl, xr, attn, rp, rows, cols):
    H, Fh = attn.shape
    z = F.leaky_relu(xl[cols] + xr[rows], SLOPE)                                     # [E, H F]: written and read again
    s = (z.view(-1, H, Fh) * attn).sum(-1).t().contiguous()                           # [H, E]
    return E_ops.edge_softmax_heads(s, rp)


def times(graph, n, rp, col, heads, feat, dev, skip_composition):
    E, HF = col.numel(), heads * feat
    g = torch.Generator(device=dev).manual_seed(HF)
    xl, xr = torch.randn(n, HF, device=dev, generator=g), torch.randn(n, HF, device=dev, generator=g)
    attn = torch.randn(heads, feat, device=dev, generator=g) / feat ** 0.5
    dp = torch.randn(heads, E, device=dev, generator=g)
    p, gg = torch.empty(heads, E, device=dev), torch.empty(heads, E, device=dev)
    TCGNN.transpose_graph(rp, col)   # (the transposed CSR: built once per graph, outside the timed region)
    with torch.no_grad():
        t_f = median_ms(lambda: TCGNN.gatv2_softmax(xl, xr, attn, rp, col, SLOPE, out=p))
        t_r = median_ms(lambda: TCGNN.gatv2_softmax_backward(p, dp, xl, xr, attn, rp, col, SLOPE, out=gg))
        t_s = median_ms(lambda: TCGNN.gatv2_source_grad(gg, xl, xr, attn, rp, col, SLOPE))
        _, d_xr, d_attn = TCGNN.gatv2_softmax_backward(p, dp, xl, xr, attn, rp, col, SLOPE, out=gg)
        d_xl = TCGNN.gatv2_source_grad(gg, xl, xr, attn, rp, col, SLOPE)
    gather = E * HF * 4
    line = dict(graph=graph, what="gatv2_softmax", heads=heads, features=feat, forward_ms=t_f, backward_row_ms=t_r, backward_source_ms=t_s,
                backward_ms=t_r + t_s, gather_bytes=gather, forward_gather_GBps=gather / t_f / 1e6, backward_row_gather_GBps=gather / t_r / 1e6,
                backward_source_gather_GBps=gather / t_s / 1e6, gather_at_hbm_peak_ms=gather / PEAK_BYTES_PER_MS,
                longest_row=int((rp[1:] - rp[:-1]).max()))
    if not skip_composition:
        lens = (rp[1:] - rp[:-1]).long()
        rows, cols = torch.repeat_interleave(torch.arange(n, device=dev), lens), col.long()
        try:
            with torch.no_grad():
                t_cf = median_ms(lambda: composition(xl, xr, attn, rp, rows, cols), reps=3, warmup=1)
                err = float((composition(xl, xr, attn, rp, rows, cols) - p).abs().max())

            def both():
                leaves = [t.detach().requires_grad_(True) for t in (xl, xr, attn)]
                return torch.autograd.grad(composition(*leaves, rp, rows, cols), leaves, dp)
            t_cfb = median_ms(both, reps=3, warmup=1)
            ref = both()
            top = lambda t: max(float(t.abs().max()), 1e-30)   # noqa: E731
            err_b = max(float((a - b).abs().max()) / top(b) for a, b in zip((d_xl, d_xr, d_attn), ref))
            del ref
            line.update(torch_forward_ms=t_cf, torch_forward_backward_ms=t_cfb, fused_forward_backward_ms=t_f + t_r + t_s,
                        forward_speedup=t_cf / t_f, forward_backward_speedup=t_cfb / (t_f + t_r + t_s), max_abs_difference_from_torch=err,
                        max_backward_difference_from_torch_of_the_largest_entry=err_b, composition_out_of_memory=False)
        except torch.OutOfMemoryError:
            line.update(composition_out_of_memory=True)
        del rows, cols
        torch.cuda.empty_cache()
    emit(**line)
    # the additive scores at the same head count
    el, er = torch.randn(n, heads, device=dev, generator=g), torch.randn(n, heads, device=dev, generator=g)
    with torch.no_grad():
        t_gf = median_ms(lambda: TCGNN.gat_softmax(el, er, rp, col, SLOPE, out=p))
        t_gb = median_ms(lambda: TCGNN.gat_softmax_backward(p, dp, el, er, rp, col, SLOPE, out=gg))
        t_gc = median_ms(lambda: TCGNN.edge_colsum(gg, rp, col))
    emit(graph=graph, what="gat", heads=heads, gat_forward_ms=t_gf, gat_backward_ms=t_gb + t_gc, gatv2_over_gat_forward=t_f / t_gf,
         gatv2_over_gat_backward=(t_r + t_s) / (t_gb + t_gc))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=str, default="sbm_reddit,rmat_reddit,sbm_products")
    ap.add_argument("--configs", type=str, default=",".join("%dx%d" % c for c in CONFIGS), help="heads x features per head, e.g. 8x8,4x32")
    ap.add_argument("--skip-composition", action="store_true", help="leave out the torch composition (an [E, H F] tensor, several times over)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    table = {"sbm_reddit": ("reddit", "sbm_reddit"), "rmat_reddit": ("reddit", "rmat"), "sbm_products": ("ogbn-products", "sbm")}
    for graph in args.graphs.split(","):
        shape, gen = table[graph]
        n, nnz, _, _ = G.SHAPES[shape]
        rp, col = G.GENERATORS[gen](n, nnz, seed=0, device=dev)
        emit(graph=graph, what="graph", num_nodes=n, num_edges=col.numel())
        for heads, feat in [tuple(int(v) for v in c.split("x")) for c in args.configs.split(",")]:
            times(graph, n, rp, col, heads, feat, dev, args.skip_composition)
            torch.cuda.empty_cache()
        TCGNN.clear_plan_cache()
        del rp, col
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
