#!/usr/bin/env python3
"""Message passing with a feature vector per edge (forward_ue / backward_ue / edge_sum) against the torch composition it replaces, and a
GINE epoch.

Per graph and width, HIP events, median of --reps calls after --warmup (the torch composition: 3 after 1), all in one run:
    forward_ue, backward_ue          tcgnn_edge_message / _backward with ReLU
    edge_sum(perm)                   tcgnn_edge_sum over the transposed graph: dM summed by source node (the gradient with respect to X)
    aggregate_ue fwd+bwd             the autograd Function, gradients for X and Ef: the three calls above
    torch fwd, torch fwd+bwd         relu(X[col] + Ef) - E x D floats - then torch.segment_reduce(..., "sum"), and its autograd
    forward_max                      tcgnn_segment_max on the same rows: the same gather of X without the stream of Ef
    rate                             the bytes the operator must move over the time: forward 4 E D of Ef streamed + 4 E D of X gathered + 4 E
                                     ids + 4 N D written; backward the same read plus 4 N D of dY and 4 E D of dM written
    GINE epoch                       tcgnn_harness.time_training("gine"): two layers D -> D -> classes on random D-wide inputs (a GINE
                                     layer aggregates at its INPUT width: the datasets' own widths would make Ef' hundreds of GB)
GRAPHS: name:generator:D[,D...] separated by spaces; default the three of DESIGN.md 4.15."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tc-gnn_atc23_amd")):
    sys.path.insert(0, p)

DEFAULT = ["reddit:sbm_reddit:16,64", "reddit:rmat:16,64", "ogbn-products:sbm:16,64"]


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--edge-dim", type=int, default=16)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--skip-epochs", action="store_true")
    args = ap.parse_args()
    import torch
    import TCGNN
    import tcgnn_edge_ops as EO
    import tcgnn_graph as G
    import tcgnn_harness as H
    dev = torch.device("cuda:0")
    print("build %s, XCD mapping %s" % (__import__("tcgnn_capi").build_id(), os.environ.get("TCGNN_SEGMAX_XCD_MAP", "1 (default)")))
    misses = []
    for spec in args.graphs:
        shape, gen, dims = spec.split(":")
        n, nnz, _, classes = G.SHAPES[shape]
        rp, col = G.GENERATORS[gen](n, nnz, seed=0, device=dev)
        E, nw = col.numel(), (n + 15) // 16
        bp = torch.zeros(nw, dtype=torch.int32, device=dev); e2c = torch.zeros(E, dtype=torch.int32, device=dev); e2r = torch.zeros(E, dtype=torch.int32, device=dev)
        TCGNN.preprocess_gpu(col, rp, n, 16, 8, bp, e2c, e2r)
        meta = (rp, col, bp, e2c, e2r)
        lens = (rp[1:] - rp[:-1])
        print("%s / %s: N = %d, E = %d, longest row %d" % (shape, gen, n, E, int(lens.max())), flush=True)
        TCGNN.prepare([], *meta, max_aggregation=True)
        rp_t, _, perm, _ = TCGNN.transpose_graph(rp, col)
        g = torch.Generator(device=dev).manual_seed(0)
        for D in (int(d) for d in dims.split(",")):
            tag = "%s/%s D=%d" % (shape, gen, D)
            X = torch.randn(n, D, device=dev, generator=g)
            dY = torch.randn(n, D, device=dev, generator=g)
            Ef = torch.randn(E, D, device=dev, generator=g)
            Y, dM, dX = torch.empty_like(X), torch.empty_like(Ef), torch.empty_like(X)
            t_f = median_ms(lambda: TCGNN.forward_ue(X, Ef, rp, col, out=Y), args.reps, args.warmup)
            t_b = median_ms(lambda: TCGNN.backward_ue(dY, X, Ef, rp, col, out=dM), args.reps, args.warmup)
            t_s = median_ms(lambda: TCGNN.edge_sum(dM, rp_t, perm, out=dX), args.reps, args.warmup)
            t_m = median_ms(lambda: TCGNN.forward_max(X, rp, col, return_arg=False, out=dX), args.reps, args.warmup)
            del dM
            Xg, Eg = X.clone().requires_grad_(True), Ef.clone().requires_grad_(True)

            def fused():
                return torch.autograd.grad(EO.aggregate_ue(Xg, Eg, rp, col, "relu"), [Xg, Eg], dY)
            t_fb = median_ms(fused, args.reps, args.warmup)
            fwd_gb = (8.0 * E * D + 4.0 * E + 4.0 * n * D) / 1e9
            bwd_gb = (12.0 * E * D + 4.0 * E + 4.0 * n * D) / 1e9
            sum_gb = (4.0 * E * D + 4.0 * E + 4.0 * n * D) / 1e9   # (dM's rows gathered through perm, perm itself, dX written)
            print("  D=%3d  forward_ue %.3f ms (%.1f GB, %.2f TB/s)  backward_ue %.3f ms (%.1f GB, %.2f TB/s)  edge_sum(perm) %.3f ms (%.1f GB, %.2f TB/s)"
                  "  aggregate_ue fwd+bwd %.3f ms | forward_max %.3f ms" % (D, t_f, fwd_gb, fwd_gb / t_f, t_b, bwd_gb, bwd_gb / t_b, t_s, sum_gb, sum_gb / t_s,
                                                                             t_fb, t_m), flush=True)
            if not args.skip_torch:
                try:
                    lengths, coll = lens.long(), col.long()

                    def compose():
                        return torch.segment_reduce(torch.relu(Xg[coll] + Eg), "sum", lengths=lengths, unsafe=True)
                    t_tf = median_ms(lambda: compose(), 3, 1)
                    t_tfb = median_ms(lambda: torch.autograd.grad(compose(), [Xg, Eg], dY), 3, 1)
                    out = compose().detach()
                    err = float((out - Y).abs().max() / out.abs().max())
                    del out
                    line = "         torch fwd %.3f ms  fwd+bwd %.3f ms (largest |difference| %.1e of the largest entry): fused forward %.1fx, forward + backward %.1fx" % (
                        t_tf, t_tfb, err, t_tf / t_f, t_tfb / t_fb)
                    for what, ours, theirs in (("forward", t_f, t_tf), ("forward + backward", t_fb, t_tfb)):
                        if ours >= theirs:
                            misses.append("%s %s: fused %.3f ms against torch %.3f ms" % (tag, what, ours, theirs))
                except RuntimeError as e:   # (E x D floats several times over: out of memory on the largest shapes)
                    line = "         torch composition: %s" % str(e).splitlines()[0][:100]
                torch.cuda.empty_cache()
                print(line, flush=True)
            del X, dY, Ef, Y, dX, Xg, Eg
            torch.cuda.empty_cache()
            if not args.skip_epochs:
                gen_ = torch.Generator().manual_seed(0)
                x = torch.randn(n, D, generator=gen_).to(dev)
                y = torch.randint(0, classes, (n,), generator=gen_).to(dev)
                try:
                    r = H.time_training("gine", meta, x, y, D, D, classes, 2, 5, warmup=2, edge_dim=args.edge_dim)
                    print("         GINE epoch (%d -> %d -> %d, edge_dim %d, edge_attr drawn on the device from seed 0): %.3f ms" % (D, D, classes, args.edge_dim, r["train_ms"]),
                          flush=True)
                except RuntimeError as e:
                    print("         GINE epoch: %s" % str(e).splitlines()[0][:100], flush=True)
                del x, y
                torch.cuda.empty_cache()
        del rp_t, perm
        TCGNN.clear_plan_cache()
        torch.cuda.empty_cache()
    print("misses against the torch composition: %s" % ("; ".join(misses) if misses else "none"))


if __name__ == "__main__":
    main()
