#!/usr/bin/env python3
"""Fused sparse attention (forward_attn / backward_attn / source_grad_attn; TransformerConv(fused=True)) against the three-operator
composition (sddmm_heads, edge_softmax_heads, aggregate_heads): one JSON line per case.
Cases: sbm_reddit, an SBM graph at the ogbn-products shape and R-MAT at the Reddit shape, each at heads x F = 8 x 8 and 4 x 32.
Both paths run on the same q, k, v in ALTERNATING samples of one run, after --warmup calls of each and with everything either needs
prepared outside the timed region (prepare: the plans, A^T's, the workspaces; the transposed CSR).  Times are HIP-event medians with
[min, max]; a comparison counts only where the two intervals are disjoint (intervals_disjoint):
  forward              aggregate_attention / the composition, no gradients kept
  step                 forward + backward with gradients for q, k and v
  the three calls      forward_attn, backward_attn, source_grad_attn on their own (--reps samples each)
  peak bytes           of torch's allocator over one step, above what was allocated before it
    python tools/bench_fused_attention.py [--cases sbm_reddit:8x8,rmat_reddit:4x32]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tc-gnn_atc23_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import TCGNN  # noqa: E402
import tcgnn_edge_ops as E_ops  # noqa: E402
import tcgnn_graph as G  # noqa: E402
from bench_gated import emit, measure, peak_bytes, stats, timed  # noqa: E402

CASES = "sbm_reddit:8x8,sbm_reddit:4x32,sbm_products:8x8,sbm_products:4x32,rmat_reddit:8x8,rmat_reddit:4x32"
GRAPHS = {"sbm_reddit": ("reddit", "sbm_reddit"), "rmat_reddit": ("reddit", "rmat"), "sbm_products": ("ogbn-products", "sbm")}


def alternating(a, b, reps, warmup):
    for _ in range(warmup):
        a()
        b()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(a))
        tb.append(timed(b))
    return stats(ta), stats(tb)


def case(graph, meta, H, F, dev, args):
    rp, col = meta[:2]
    n, E, scale = rp.numel() - 1, col.numel(), F ** -0.5
    g = torch.Generator(device=dev).manual_seed(H * 1000 + F)
    q, k, v, dY = (torch.randn(n, H * F, device=dev, generator=g) for _ in range(4))
    beta = torch.tensor([scale], dtype=torch.float32, device=dev)
    TCGNN.prepare([F], *meta, edge_valued=True, transpose=True, attention=True, heads=H)
    TCGNN.prepare([], *meta, fused_attention=True)

    def fused_fwd(a=q, b=k, c=v):
        return E_ops.aggregate_attention(a, b, c, H, rp, col, scale)

    def composed_fwd(a=q, b=k, c=v):
        return E_ops.aggregate_heads(E_ops.edge_softmax_heads(E_ops.sddmm_heads(a, b, meta, H), rp, beta), c, meta)

    def step(fwd):
        leaves = [t.detach().requires_grad_(True) for t in (q, k, v)]
        return torch.autograd.grad(fwd(*leaves), leaves, dY)

    line = dict(graph=graph, what="fused_attention", heads=H, F=F, num_edges=E, longest_row=int((rp[1:] - rp[:-1]).max()), gather_bytes=2 * E * H * F * 4)
    with torch.no_grad():
        Y, L = TCGNN.forward_attn(q, k, v, H, rp, col, scale)
        _, delta = TCGNN.backward_attn(q, k, v, Y, dY, L, H, rp, col, scale)
        line["forward_attn"] = measure(lambda: TCGNN.forward_attn(q, k, v, H, rp, col, scale, out=Y), args.reps, args.warmup)
        line["backward_attn"] = measure(lambda: TCGNN.backward_attn(q, k, v, Y, dY, L, H, rp, col, scale), args.reps, args.warmup)
        line["source_grad_attn"] = measure(lambda: TCGNN.source_grad_attn(q, k, v, dY, L, delta, H, rp, col, scale), args.reps, args.warmup)
        line["max_abs_difference_from_composition"] = float((composed_fwd() - Y).abs().max())
        line["fused_forward"], line["composed_forward"] = alternating(fused_fwd, composed_fwd, args.reps, args.warmup)
    ours, theirs = step(fused_fwd), step(composed_fwd)
    line["max_gradient_difference_of_the_largest_entry"] = max(float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30) for a, b in zip(ours, theirs))
    del ours, theirs
    line["fused_step_peak_bytes"], line["composed_step_peak_bytes"] = peak_bytes(lambda: step(fused_fwd)), peak_bytes(lambda: step(composed_fwd))
    line["fused_step"], line["composed_step"] = alternating(lambda: step(fused_fwd), lambda: step(composed_fwd), args.reps, args.warmup)
    for what in ("forward", "step"):
        f, c = line["fused_" + what], line["composed_" + what]
        line[what + "_speedup"] = c["median_ms"] / f["median_ms"]
        line[what + "_intervals_disjoint"] = f["max_ms"] < c["min_ms"] or c["max_ms"] < f["min_ms"]
    emit(**line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=str, default=CASES, help="graph:HxF, comma separated; graphs: " + ", ".join(GRAPHS))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cases = [(c.split(":")[0],) + tuple(int(x) for x in c.split(":")[1].split("x")) for c in args.cases.split(",")]
    for graph in dict.fromkeys(c[0] for c in cases):
        shape, gen = GRAPHS[graph]
        n, nnz, _, _ = G.SHAPES[shape]
        rp, col = G.GENERATORS[gen](n, nnz, seed=0, device=dev)
        E = col.numel()
        bp, e2c, e2r = torch.zeros((n + 15) // 16, dtype=torch.int32, device=dev), torch.zeros(E, dtype=torch.int32, device=dev), torch.zeros(E, dtype=torch.int32, device=dev)
        fd = os.dup(1)
        os.dup2(2, 1)   # (the SGT's two report lines go to stderr: stdout is JSON lines only)
        TCGNN.preprocess_gpu(col, rp, n, 16, 8, bp, e2c, e2r)
        sys.stdout.flush()
        os.dup2(fd, 1)
        emit(graph=graph, what="graph", num_nodes=n, num_edges=E)
        for _, H, F in [c for c in cases if c[0] == graph]:
            case(graph, (rp, col, bp, e2c, e2r), H, F, dev, args)
            torch.cuda.empty_cache()
        TCGNN.clear_plan_cache()
        del rp, col, bp, e2c, e2r
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
