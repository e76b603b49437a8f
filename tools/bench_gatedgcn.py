#!/usr/bin/env python3
"""GatedGCN with edge features (forward_gatedgcn / backward_gatedgcn / source_grad_gatedgcn; GatedGCNConv): one JSON line per case.
A case is graph:D:scale - the graph's shape shrunk to N * scale nodes and nnz * scale^2 edges.  The operator's inherent [E, D] tensors (c, Z,
dZ, G) are 29 GB EACH on the Reddit shape at D = 64 and the torch composition holds several more, so the default cases are sbm_reddit at
full size and D = 16 (7.3 GB each) and sbm_reddit, R-MAT and the products SBM at scale 0.5 and D = 64 (about 7.3 - 7.9 GB each): both sides fit.
Times are HIP-event medians with [min, max] of --reps calls after --warmup calls:
  forward_gatedgcn, backward_gatedgcn (with dZ and without), source_grad_gatedgcn     the three calls (the transposed CSR is built outside)
  fused step     aggregate_gatedgcn forward + backward, gradients for k, q, v and c, a loss on Y and Z, against, in ALTERNATING samples of one run,
  composition    torch: Z = k[row] + q[col] + c, sigmoid, index_add_ of eta * v[col] and of eta, the quotient, and its autograd backward.
                 Peak bytes of torch's allocator for both.  Where the composition runs out of memory the line says so.
  forward_gated, forward_ue at the same D: each moves two rows per edge where forward_gatedgcn moves four (two gathered, one streamed in, one out).
    python tools/bench_gatedgcn.py [--cases sbm_reddit:16:1,rmat_reddit:64:0.5] [--skip-composition]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tc-gnn_atc23_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import TCGNN  # noqa: E402
import tcgnn_edge_ops as E_ops  # noqa: E402
import tcgnn_graph as G  # noqa: E402
from bench_gated import GRAPHS, emit, measure, peak_bytes, stats, timed  # noqa: E402

CASES = "sbm_reddit:16:1,sbm_reddit:64:0.5,rmat_reddit:64:0.5,sbm_products:64:0.5"
EPS = 1e-6


def composition(k, q, v, c, rows, cols):
    Z = k[rows] + q[cols] + c
    eta = torch.sigmoid(Z)
    num = torch.zeros_like(k).index_add_(0, rows, eta * v[cols])
    return num / (torch.zeros_like(k).index_add_(0, rows, eta) + EPS), Z


def case(graph, scale, n, rp, col, D, dev, args):
    E = col.numel()
    g = torch.Generator(device=dev).manual_seed(D)
    k, q, v, dY = (torch.randn(n, D, device=dev, generator=g) for _ in range(4))
    c, dZ = (torch.randn(E, D, device=dev, generator=g) for _ in range(2))
    TCGNN.transpose_graph(rp, col)   # (built once per graph, outside the timed region)
    row_bytes = E * D * 4
    with torch.no_grad():
        fwd = measure(lambda: TCGNN.forward_gatedgcn(k, q, v, c, rp, col, EPS), args.reps, args.warmup)
        Y, Z, Den = TCGNN.forward_gatedgcn(k, q, v, c, rp, col, EPS)
        bwd = measure(lambda: TCGNN.backward_gatedgcn(dY, dZ, Y, Den, Z, v, rp, col, EPS), args.reps, args.warmup)
        bwd0 = measure(lambda: TCGNN.backward_gatedgcn(dY, None, Y, Den, Z, v, rp, col, EPS), args.reps, args.warmup)
        Gm, _ = TCGNN.backward_gatedgcn(dY, dZ, Y, Den, Z, v, rp, col, EPS)
        src = measure(lambda: TCGNN.source_grad_gatedgcn(Gm, Z, dY, Den, rp, col, EPS), args.reps, args.warmup)
        del Gm
        f_gated = measure(lambda: TCGNN.forward_gated(k, q, v, rp, col, return_sens=False, out=Y), args.reps, args.warmup)
        f_ue = measure(lambda: TCGNN.forward_ue(k, c, rp, col, act="identity", out=Y), args.reps, args.warmup)
    line = dict(graph=graph, what="gatedgcn", D=D, scale=scale, num_nodes=n, num_edges=E, longest_row=int((rp[1:] - rp[:-1]).max()), edge_tensor_bytes=row_bytes,
                forward_gatedgcn=fwd, backward_gatedgcn=bwd, backward_gatedgcn_without_dZ=bwd0, source_grad_gatedgcn=src,
                forward_GBps_over_four_rows_per_edge=4 * row_bytes / fwd["median_ms"] / 1e6, forward_gated_without_S=f_gated, forward_ue=f_ue,
                forward_over_forward_gated=fwd["median_ms"] / f_gated["median_ms"], forward_over_forward_ue=fwd["median_ms"] / f_ue["median_ms"])
    del Z, Den

    def step(fn):
        leaves = [t.detach().requires_grad_(True) for t in (k, q, v, c)]
        return torch.autograd.grad(fn(*leaves), leaves, (dY, dZ))

    fused = lambda: step(lambda *t: E_ops.aggregate_gatedgcn(*t, rp, col, EPS))   # noqa: E731
    line["fused_step_peak_bytes"] = peak_bytes(fused)
    if args.skip_composition:
        line["fused_step"] = measure(fused, args.reps, args.warmup)
    else:
        rows = torch.repeat_interleave(torch.arange(n, device=dev), (rp[1:] - rp[:-1]).long())
        cols = col.long()
        torch_step = lambda: step(lambda *t: composition(*t, rows, cols))   # noqa: E731
        try:
            line["torch_step_peak_bytes"] = peak_bytes(torch_step)
            ours, theirs = fused(), torch_step()
            line["max_gradient_difference_from_torch_of_the_largest_entry"] = max(
                float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30) for a, b in zip(ours, theirs))
            del ours, theirs
            tf, tt = [], []
            for _ in range(args.torch_reps):   # alternating samples of one run
                tf.append(timed(fused))
                tt.append(timed(torch_step))
            line.update(fused_step=stats(tf), torch_step=stats(tt), composition_out_of_memory=False)
            line["step_speedup"] = line["torch_step"]["median_ms"] / line["fused_step"]["median_ms"]
            line["intervals_disjoint"] = line["fused_step"]["max_ms"] < line["torch_step"]["min_ms"]
        except torch.OutOfMemoryError:
            line.update(composition_out_of_memory=True, fused_step=measure(fused, args.reps, args.warmup))
    emit(**line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=str, default=CASES, help="graph:D:scale, comma separated; graphs: " + ", ".join(GRAPHS))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-reps", type=int, default=5, help="samples of the composition and of the fused step it alternates with")
    ap.add_argument("--skip-composition", action="store_true", help="leave out the torch composition (many [E, D] tensors at once)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for text in args.cases.split(","):
        graph, D, scale = text.split(":")
        shape, gen = GRAPHS[graph]
        n, nnz, _, _ = G.SHAPES[shape]
        n, nnz = int(n * float(scale)), int(nnz * float(scale) ** 2)
        rp, col = G.GENERATORS[gen](n, nnz, seed=0, device=dev)
        case(graph, float(scale), n, rp, col, int(D), dev, args)
        TCGNN.clear_plan_cache()
        del rp, col
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
