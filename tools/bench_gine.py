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
    fused projection                 forward_uep / backward_uep / source_grad_uep (tcgnn_edge_project_*, edge_attr [E, edge_dim]) and the
                                     layer's aggregation forward + backward, fused (aggregate_uep) against unfused (edge_attr We + be by torch,
                                     then aggregate_ue) in ALTERNATING samples: median [min, max] of --reps each, and the peak bytes torch
                                     allocated during one such step; likewise the GINE epoch with and without --fuse-edge, --epoch-samples
                                     alternating samples a side; the last line names either as a miss where the fused interval is not
                                     wholly below the unfused one
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


def alternating_ms(fns, reps, warmup):
    """[(median, min, max)] of each fn, sampled in turn: a, b, a, b, ..."""
    import numpy as np
    import torch
    for _ in range(warmup):
        for fn in fns:
            fn()
    times = [[] for _ in fns]
    for _ in range(reps):
        for fn, ts in zip(fns, times):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ts.append(a.elapsed_time(b))
    return [(float(np.median(ts)), min(ts), max(ts)) for ts in times]


def peak_gb(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("graphs", nargs="*", default=DEFAULT)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--edge-dim", type=int, default=16)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--skip-epochs", action="store_true")
    ap.add_argument("--epoch-samples", type=int, default=3, help="alternating GINE epoch samples per side")
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
            del Ef, Eg
            torch.cuda.empty_cache()
            K = args.edge_dim
            A = torch.randn(E, K, device=dev, generator=g).requires_grad_(True)
            We = (torch.randn(K, D, device=dev, generator=g) / K ** 0.5).requires_grad_(True)
            be = torch.randn(D, device=dev, generator=g).requires_grad_(True)
            TCGNN.prepare([D], *meta, edge_project=K)
            Ad, Wd, bd = A.detach(), We.detach(), be.detach()
            t_pf = median_ms(lambda: TCGNN.forward_uep(X, Ad, Wd, bd, rp, col, out=Y), args.reps, args.warmup)
            t_pb = median_ms(lambda: TCGNN.backward_uep(dY, X, Ad, Wd, bd, rp, col), args.reps, args.warmup)
            t_ps = median_ms(lambda: TCGNN.source_grad_uep(dY, X, Ad, Wd, bd, rp, col, out=dX), args.reps, args.warmup)
            print("         fused projection (edge_dim %d): forward_uep %.3f ms  backward_uep %.3f ms  source_grad_uep %.3f ms" % (K, t_pf, t_pb, t_ps), flush=True)
            try:
                def step_fused():
                    return torch.autograd.grad(EO.aggregate_uep(Xg, A, We, be, rp, col, "relu"), [Xg, A, We, be], dY)

                def step_unfused():
                    return torch.autograd.grad(EO.aggregate_ue(Xg, A @ We + be, rp, col, "relu"), [Xg, A, We, be], dY)
                (f_med, f_lo, f_hi), (u_med, u_lo, u_hi) = alternating_ms([step_fused, step_unfused], args.reps, args.warmup)
                print("         aggregation fwd+bwd: fused %.3f ms [%.3f, %.3f]  unfused %.3f ms [%.3f, %.3f]  peak allocated: fused %.2f GB, unfused %.2f GB"
                      % (f_med, f_lo, f_hi, u_med, u_lo, u_hi, peak_gb(step_fused), peak_gb(step_unfused)), flush=True)
                if f_hi >= u_lo:   # (not faster with disjoint intervals)
                    misses.append("%s aggregation fwd+bwd: fused [%.3f, %.3f] ms not below unfused [%.3f, %.3f] ms" % (tag, f_lo, f_hi, u_lo, u_hi))
            except RuntimeError as e:
                print("         aggregation fwd+bwd: %s" % str(e).splitlines()[0][:100], flush=True)
            del X, dY, Y, dX, Xg, A, We, be, Ad, Wd, bd
            torch.cuda.empty_cache()
            if not args.skip_epochs:
                gen_ = torch.Generator().manual_seed(0)
                x = torch.randn(n, D, generator=gen_).to(dev)
                y = torch.randint(0, classes, (n,), generator=gen_).to(dev)
                epochs = {False: [], True: []}
                for fuse in (False, True) * args.epoch_samples:   # (alternating samples, each the mean of five epochs)
                    try:
                        r = H.time_training("gine", meta, x, y, D, D, classes, 2, 5, warmup=2, edge_dim=args.edge_dim, fuse_edge=fuse)
                        epochs[fuse].append(r["train_ms"])
                        print("         GINE epoch%s (%d -> %d -> %d, edge_dim %d, edge_attr drawn on the device from seed 0): %.3f ms"
                              % (" --fuse-edge" if fuse else "", D, D, classes, args.edge_dim, r["train_ms"]), flush=True)
                    except RuntimeError as e:
                        print("         GINE epoch%s: %s" % (" --fuse-edge" if fuse else "", str(e).splitlines()[0][:100]), flush=True)
                    torch.cuda.empty_cache()
                if epochs[True] and epochs[False] and max(epochs[True]) >= min(epochs[False]):   # (not faster with disjoint intervals)
                    misses.append("%s GINE epoch: fused [%.3f, %.3f] ms not below unfused [%.3f, %.3f] ms"
                                  % (tag, min(epochs[True]), max(epochs[True]), min(epochs[False]), max(epochs[False])))
                del x, y
                torch.cuda.empty_cache()
        del rp_t, perm
        TCGNN.clear_plan_cache()
        torch.cuda.empty_cache()
    print("misses (against the torch composition; fused against unfused): %s" % ("; ".join(misses) if misses else "none"))


if __name__ == "__main__":
    main()
