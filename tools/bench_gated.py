#!/usr/bin/env python3
"""Gated aggregation (forward_gated / source_grad_gated; ResGatedGraphConv): one JSON line per measurement.
Cases: sbm_reddit, R-MAT at the Reddit shape and an SBM graph at the ogbn-products shape at D = 64; sbm_reddit also at D = 16 and 128.
Times are HIP-event medians with [min, max] of --reps calls after --warmup calls:
  forward_gated        tcgnn_gated_sum with S, and without it
  source_grad_gated    tcgnn_gated_source_grad over A^T (the transposed CSR is built outside the timed region)
  fused step           aggregate_gated forward + backward with gradients for k, q and v, against, in ALTERNATING samples of the same run,
  composition          torch: sigmoid(k[row] + q[col]) * v[col] - [E, D] tensors - summed by row with index_add_, and its autograd
                       backward; forward alone as well.  Peak bytes of torch's allocator for both.  Where it runs out of memory the
                       line says so.
  forward_ue           tcgnn_edge_message (identity) at the same D: a yardstick that also moves two rows per edge (one gathered, one streamed).
The gather bound of a walk is 2 E D 4 bytes (two neighbour rows per edge) over the measured time.
    python tools/bench_gated.py [--cases sbm_reddit:64,rmat_reddit:64] [--skip-composition]"""
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

CASES = "sbm_reddit:64,rmat_reddit:64,sbm_products:64,sbm_reddit:16,sbm_reddit:128"
GRAPHS = {"sbm_reddit": ("reddit", "sbm_reddit"), "rmat_reddit": ("reddit", "rmat"), "sbm_products": ("ogbn-products", "sbm")}


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(samples):
    t = sorted(samples)
    return {"median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1]}


def measure(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return stats([timed(fn) for _ in range(reps)])


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def composition(k, q, v, rows, cols):
    msg = torch.sigmoid(k[rows] + q[cols]) * v[cols]
    return torch.zeros_like(k).index_add_(0, rows, msg)


def case(graph, n, rp, col, D, dev, args):
    E = col.numel()
    g = torch.Generator(device=dev).manual_seed(D)
    k, q, v, dY = (torch.randn(n, D, device=dev, generator=g) for _ in range(4))
    TCGNN.transpose_graph(rp, col)   # (the transposed CSR: built once per graph, outside the timed region)
    gather = 2 * E * D * 4
    with torch.no_grad():
        Y = torch.empty_like(k)
        f_s = measure(lambda: TCGNN.forward_gated(k, q, v, rp, col, out=Y), args.reps, args.warmup)
        f_n = measure(lambda: TCGNN.forward_gated(k, q, v, rp, col, return_sens=False, out=Y), args.reps, args.warmup)
        s_g = measure(lambda: TCGNN.source_grad_gated(k, q, v, dY, rp, col), args.reps, args.warmup)
    line = dict(graph=graph, what="gated", D=D, num_edges=E, longest_row=int((rp[1:] - rp[:-1]).max()), gather_bytes=gather,
                forward_gated=f_s, forward_gated_without_S=f_n, source_grad_gated=s_g,
                forward_gather_GBps=gather / f_s["median_ms"] / 1e6, source_gather_GBps=gather / s_g["median_ms"] / 1e6)

    def fused():
        leaves = [t.detach().requires_grad_(True) for t in (k, q, v)]
        return torch.autograd.grad(E_ops.aggregate_gated(*leaves, rp, col), leaves, dY)
    line["fused_step_peak_bytes"] = peak_bytes(fused)
    if args.skip_composition:
        line["fused_step"] = measure(fused, args.reps, args.warmup)
    else:
        rows = torch.repeat_interleave(torch.arange(n, device=dev), (rp[1:] - rp[:-1]).long())
        cols = col.long()

        def torch_step():
            leaves = [t.detach().requires_grad_(True) for t in (k, q, v)]
            return torch.autograd.grad(composition(*leaves, rows, cols), leaves, dY)
        try:
            line["torch_step_peak_bytes"] = peak_bytes(torch_step)
            with torch.no_grad():
                line["torch_forward"] = measure(lambda: composition(k, q, v, rows, cols), args.torch_reps, 1)
                line["max_abs_difference_from_torch"] = float((composition(k, q, v, rows, cols) - Y).abs().max())
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
        del rows, cols
        torch.cuda.empty_cache()
    # the yardstick: u_add_e moves a gathered row and a streamed row per edge
    try:
        Ef = torch.randn(E, D, device=dev, generator=g)
        with torch.no_grad():
            line["forward_ue"] = measure(lambda: TCGNN.forward_ue(k, Ef, rp, col, act="identity", out=Y), args.reps, args.warmup)
        line["forward_gated_over_forward_ue"] = f_s["median_ms"] / line["forward_ue"]["median_ms"]
        del Ef
    except torch.OutOfMemoryError:
        line["forward_ue"] = "out of memory"
    emit(**line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=str, default=CASES, help="graph:D, comma separated; graphs: " + ", ".join(GRAPHS))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=5, help="samples of the composition and of the fused step it alternates with")
    ap.add_argument("--skip-composition", action="store_true", help="leave out the torch composition ([E, D] tensors, several at once)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cases = [(c.split(":")[0], int(c.split(":")[1])) for c in args.cases.split(",")]
    for graph in dict.fromkeys(c[0] for c in cases):
        shape, gen = GRAPHS[graph]
        n, nnz, _, _ = G.SHAPES[shape]
        rp, col = G.GENERATORS[gen](n, nnz, seed=0, device=dev)
        emit(graph=graph, what="graph", num_nodes=n, num_edges=col.numel())
        for _, D in [c for c in cases if c[0] == graph]:
            case(graph, n, rp, col, D, dev, args)
            torch.cuda.empty_cache()
        TCGNN.clear_plan_cache()
        del rp, col
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
