#!/usr/bin/env python3
"""Max aggregation (forward_max / backward_max) against the torch composition it replaces, and GraphSAGE epochs by aggregator.

Per graph and width, HIP events, median of --reps calls after --warmup:
    forward_max, backward_max              tcgnn_segment_max / _backward
    torch fwd, torch bwd                   X[col] (E x D floats) + torch.segment_reduce(..., "max"), and its autograd backward
    forward                                the binary SpMM on the same graph, for scale
    gather bound                           E rows of 4 D bytes at 16 TB/s (scattered lines from L2) and at 8 TB/s (beyond it), DESIGN.md 4
    SAGE epoch mean / max / pool           tcgnn_harness.time_training (two layers, hidden 64)
--xcd-ab runs the operator part twice in child processes, TCGNN_SEGMAX_XCD_MAP=0 and =1 (the row-to-workgroup mapping is read when the
library loads).  GRAPHS: name:generator:D[,D...] separated by spaces; default the four of DESIGN.md 4.12."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("graphs", nargs="*", default=DEFAULT)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--skip-epochs", action="store_true")
    ap.add_argument("--xcd-ab", action="store_true")
    args = ap.parse_args()
    if args.xcd_ab:
        for setting in ("0", "1"):
            print("---- TCGNN_SEGMAX_XCD_MAP=%s" % setting, flush=True)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), *args.graphs, "--reps", str(args.reps), "--warmup", str(args.warmup), "--skip-torch",
                                "--skip-epochs"], env=dict(os.environ, TCGNN_SEGMAX_XCD_MAP=setting), timeout=900)
            if r.returncode:
                sys.exit(r.returncode)
        return
    import torch
    import TCGNN
    import tcgnn_graph as G
    import tcgnn_harness as H
    dev = torch.device("cuda:0")
    print("build %s, XCD mapping %s" % (__import__("tcgnn_capi").build_id(), os.environ.get("TCGNN_SEGMAX_XCD_MAP", "1 (default)")))
    for spec in args.graphs:
        shape, gen, dims = spec.split(":")
        n, nnz, in_dim, classes = G.SHAPES[shape]
        rp, col = G.GENERATORS[gen](n, nnz, seed=0, device=dev)
        E, nw = col.numel(), (n + 15) // 16
        bp = torch.zeros(nw, dtype=torch.int32, device=dev); e2c = torch.zeros(E, dtype=torch.int32, device=dev); e2r = torch.zeros(E, dtype=torch.int32, device=dev)
        TCGNN.preprocess_gpu(col, rp, n, 16, 8, bp, e2c, e2r)
        meta = (rp, col, bp, e2c, e2r)
        lens = (rp[1:] - rp[:-1])
        print("%s / %s: N = %d, E = %d, longest row %d" % (shape, gen, n, E, int(lens.max())), flush=True)
        TCGNN.prepare([], *meta, max_aggregation=True)
        g = torch.Generator(device=dev).manual_seed(0)
        for D in (int(d) for d in dims.split(",")):
            X = torch.randn(n, D, device=dev, generator=g)
            dY = torch.randn(n, D, device=dev, generator=g)
            Y, arg = TCGNN.forward_max(X, rp, col)
            dX = torch.empty_like(X)
            t_f = median_ms(lambda: TCGNN.forward_max(X, rp, col, out=Y), args.reps, args.warmup)
            t_b = median_ms(lambda: TCGNN.backward_max(dY, arg, rp, col, out=dX), args.reps, args.warmup)
            t_s = median_ms(lambda: TCGNN.forward(X, *meta), args.reps, args.warmup)
            gb = 4.0 * D * E / 1e9
            line = "  D=%3d  forward_max %.3f ms  backward_max %.3f ms  forward (SpMM) %.3f ms | gather %.1f GB: %.3f ms at 16 TB/s, %.3f ms at 8 TB/s" % (
                D, t_f, t_b, t_s, gb, gb / 16.0, gb / 8.0)
            if not args.skip_torch:
                try:
                    lengths = lens.long()
                    coll = col.long()
                    Xg = X.clone().requires_grad_(True)

                    def compose():
                        return torch.segment_reduce(Xg[coll], "max", lengths=lengths, unsafe=True)
                    t_tf = median_ms(lambda: compose(), max(3, args.reps // 3), 2)
                    out = compose()
                    t_tb = median_ms(lambda: torch.autograd.grad(out, Xg, dY, retain_graph=True), max(3, args.reps // 3), 2)
                    same = bool(torch.equal(torch.where(lens.view(-1, 1) > 0, out.detach(), torch.zeros_like(Y)), Y))
                    line += " | torch fwd %.3f ms  bwd %.3f ms (Y equal: %s)" % (t_tf, t_tb, same)
                    del out, Xg
                except RuntimeError as e:   # (E x D floats, twice over in backward: out of memory on the largest shapes)
                    line += " | torch composition: %s" % str(e).splitlines()[0][:80]
                torch.cuda.empty_cache()
            print(line, flush=True)
            del X, dY, Y, arg, dX
        if not args.skip_epochs:
            gen_ = torch.Generator().manual_seed(0)
            x = torch.randn(n, in_dim, generator=gen_).to(dev)
            y = torch.randint(0, classes, (n,), generator=gen_).to(dev)
            for agg in ("mean", "max", "pool"):
                r = H.time_training("sage", meta, x, y, in_dim, 64, classes, 2, 10, warmup=3, aggregator=agg)
                print("  SAGE epoch %-4s (%d -> 64 -> %d): %.3f ms" % (agg, in_dim, classes, r["train_ms"]), flush=True)
            del x, y
        TCGNN.clear_plan_cache()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
