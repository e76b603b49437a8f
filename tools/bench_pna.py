#!/usr/bin/env python3
"""One-gather aggregation (forward_stats / backward_stats) against the calls it replaces, and PNA epochs beside SAGE-max epochs.

Per graph and width, HIP events, median of --reps calls after --warmup, one child process per graph:
    forward_stats all / extrema / moments  tcgnn_segment_stats with all four aggregators, with max + min only, with mean + std only
    forward_max, 2 x forward_max           tcgnn_segment_max on X, and on X then -X (what max + min cost before)
    four calls                             forward_scaled (mean) + forward on X * X (second moment) + forward_max(X) + forward_max(-X)
    torch fwd                              X[col] (E x D floats) + torch.segment_reduce x 4 (mean, a second mean for the variance, max, min)
    backward_stats, 2 x backward_max       tcgnn_segment_stats_backward with every group against two tcgnn_segment_max_backward calls
    torch bwd                              autograd of the torch composition
    gather bound                           E rows of 4 D bytes at 16 TB/s and at 8 TB/s
    PNA epoch, SAGE epoch max              tcgnn_harness.time_training (two layers, hidden 64)
GRAPHS: name:generator:D[,D...] separated by spaces; default the four of DESIGN.md 4.14.  The torch lines run fewer repetitions."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tc-gnn_atc23_amd")):
    sys.path.insert(0, p)

DEFAULT = ["reddit:sbm_reddit:64,128", "ogbn-products:sbm:128", "reddit:rmat:64"]


def median_ms(fn, reps, warmup):
    import numpy as np
    import torch
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def one_graph(spec, args):
    import torch
    import TCGNN
    import tcgnn_graph as G
    import tcgnn_harness as H
    dev = torch.device("cuda:0")
    shape, gen, dims = spec.split(":")
    n, nnz, in_dim, classes = G.SHAPES[shape]
    rp, col = G.GENERATORS[gen](n, nnz, seed=0, device=dev)
    E, nw = col.numel(), (n + 15) // 16
    bp = torch.zeros(nw, dtype=torch.int32, device=dev); e2c = torch.zeros(E, dtype=torch.int32, device=dev); e2r = torch.zeros(E, dtype=torch.int32, device=dev)
    TCGNN.preprocess_gpu(col, rp, n, 16, 8, bp, e2c, e2r)
    meta = (rp, col, bp, e2c, e2r)
    lens = rp[1:] - rp[:-1]
    print("%s / %s: N = %d, E = %d, longest row %d (build %s)" % (shape, gen, n, E, int(lens.max()), __import__("tcgnn_capi").build_id()), flush=True)
    TCGNN.prepare([], *meta, max_aggregation=True)
    r_scale, _ = TCGNN.degree_scales(rp, col, "right")
    g = torch.Generator(device=dev).manual_seed(0)
    ms = lambda fn: median_ms(fn, args.reps, args.warmup)   # noqa: E731
    for D in (int(d) for d in dims.split(",")):
        X = torch.randn(n, D, device=dev, generator=g)
        d = {a: torch.randn(n, D, device=dev, generator=g) for a in TCGNN.STATS_AGGREGATORS}
        TCGNN.prepare([D], *meta, max_aggregation=True)
        full = TCGNN.forward_stats(X, rp, col)
        saved = dict(full, Z=X)
        negX, sqX, dX = -X, X * X, torch.empty_like(X)
        t_all = ms(lambda: TCGNN.forward_stats(X, rp, col))
        t_ext = ms(lambda: TCGNN.forward_stats(X, rp, col, aggregators=("max", "min")))
        t_mom = ms(lambda: TCGNN.forward_stats(X, rp, col, aggregators=("mean", "std")))
        t_max = ms(lambda: TCGNN.forward_max(X, rp, col))
        t_max2 = ms(lambda: (TCGNN.forward_max(X, rp, col), TCGNN.forward_max(negX, rp, col)))
        t_four = ms(lambda: (TCGNN.forward_scaled(X, *meta, row_scale=r_scale), TCGNN.forward(sqX, *meta), TCGNN.forward_max(X, rp, col),
                             TCGNN.forward_max(negX, rp, col)))
        t_bwd = ms(lambda: TCGNN.backward_stats(d, saved, rp, col, out=dX))
        t_bwd_ext = ms(lambda: TCGNN.backward_stats({"max": d["max"], "min": d["min"]}, saved, rp, col, out=dX))
        t_bmax2 = ms(lambda: (TCGNN.backward_max(d["max"], full["argmax"], rp, col, out=dX), TCGNN.backward_max(d["min"], full["argmin"], rp, col, out=dX)))
        gb = 4.0 * D * E / 1e9
        print("  D=%3d  forward_stats all %.3f ms  extrema %.3f ms  moments %.3f ms | forward_max %.3f ms  2 x forward_max %.3f ms  four calls %.3f ms"
              " | gather %.1f GB: %.3f ms at 16 TB/s, %.3f ms at 8 TB/s" % (D, t_all, t_ext, t_mom, t_max, t_max2, t_four, gb, gb / 16.0, gb / 8.0), flush=True)
        line = "  D=%3d  backward_stats all %.3f ms  extrema %.3f ms | 2 x backward_max %.3f ms" % (D, t_bwd, t_bwd_ext, t_bmax2)
        if not args.skip_torch:
            try:
                lengths, coll = lens.long(), col.long()
                Xg = X.clone().requires_grad_(True)

                def compose():
                    M = Xg[coll]
                    mean = torch.segment_reduce(M, "mean", lengths=lengths, unsafe=True)
                    var = torch.segment_reduce(M * M, "mean", lengths=lengths, unsafe=True) - mean * mean
                    return (mean, torch.sqrt(torch.relu(var) + 1e-5), torch.segment_reduce(M, "max", lengths=lengths, unsafe=True),
                            torch.segment_reduce(M, "min", lengths=lengths, unsafe=True))
                few = max(3, args.reps // 3)
                t_tf = median_ms(lambda: compose(), few, 2)
                outs = compose()
                t_tb = median_ms(lambda: torch.autograd.grad(outs, Xg, [d[a] for a in TCGNN.STATS_AGGREGATORS], retain_graph=True), few, 2)
                has = lens.view(-1, 1) > 0
                same = bool(torch.equal(torch.where(has, outs[2].detach(), torch.zeros_like(X)), full["max"])
                            and torch.equal(torch.where(has, outs[3].detach(), torch.zeros_like(X)), full["min"]))
                line += " | torch fwd %.3f ms  bwd %.3f ms (extrema equal: %s)" % (t_tf, t_tb, same)
                del outs, Xg
            except RuntimeError as e:   # (E x D floats several times over: out of memory on the largest shapes)
                line += " | torch composition: %s" % str(e).splitlines()[0][:80]
            torch.cuda.empty_cache()
        print(line, flush=True)
        del X, d, full, saved, negX, sqX, dX
    if not args.skip_epochs:
        gen_ = torch.Generator().manual_seed(0)
        x = torch.randn(n, in_dim, generator=gen_).to(dev)
        y = torch.randint(0, classes, (n,), generator=gen_).to(dev)
        r = H.time_training("pna", meta, x, y, in_dim, 64, classes, 2, 10, warmup=3)
        print("  PNA epoch       (%d -> 64 -> %d): %.3f ms" % (in_dim, classes, r["train_ms"]), flush=True)
        r = H.time_training("sage", meta, x, y, in_dim, 64, classes, 2, 10, warmup=3, aggregator="max")
        print("  SAGE epoch max  (%d -> 64 -> %d): %.3f ms" % (in_dim, classes, r["train_ms"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("graphs", nargs="*", default=DEFAULT)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--skip-epochs", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        one_graph(args.graphs[0], args)
        return
    for spec in args.graphs:   # a fresh process per graph: no allocator state or cached plan carries over
        flags = ["--reps", str(args.reps), "--warmup", str(args.warmup)] + (["--skip-torch"] if args.skip_torch else []) + (["--skip-epochs"] if args.skip_epochs else [])
        r = subprocess.run([sys.executable, os.path.abspath(__file__), spec, "--child", *flags], timeout=900)
        if r.returncode:
            sys.exit(r.returncode)


if __name__ == "__main__":
    main()
