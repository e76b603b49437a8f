#!/usr/bin/env python3
"""Seeded neighbour sampling (TCGNN.sample_neighbors) against the torch composition it replaces, the planless operators on the sampled
graph against the full graph, and training epochs with and without --fanout.

Per graph and fan-out, HIP events (a host clock for the count call, which synchronises), median of --reps calls after --warmup:
    count, select                   tcgnn_sample_neighbors_count / tcgnn_sample_neighbors on preallocated outputs
    sample_neighbors                the module's call: both, the output allocations and the one synchronisation
    torch composition               per-edge random keys, ONE sort by (row, key), rank below k, mask, restore CSR order (nonzero) - the
                                    figure to beat; other keys, so another sample: only the time is compared
    forward_max / _stats / _ue      D = 64, on the sampled graph and on the full one
    epochs                          tcgnn_harness.time_training, SAGE-max, PNA and GINE, without a fan-out and with 25: sample / plan / train
GRAPHS: name:generator separated by spaces; default sbm_reddit, the R-MAT Reddit shape and the products SBM.  The last line names every
miss: a selection that loses to the torch composition, an operator or an epoch that gets slower on the sampled graph."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tc-gnn_atc23_amd")):
    sys.path.insert(0, p)

DEFAULT = ["reddit:sbm_reddit", "reddit:rmat", "ogbn-products:sbm"]


def median_ms(fn, reps, warmup, host=False):
    import numpy as np
    import torch
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        if host:
            torch.cuda.synchronize()
            t = time.perf_counter(); fn(); torch.cuda.synchronize()
            times.append((time.perf_counter() - t) * 1e3)
        else:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            times.append(a.elapsed_time(b))
    return float(np.median(times))


def torch_sample(rp, rows, k, gen):
    """the composition: (rp_s, eid) of a uniform k-subset per row"""
    import torch
    E = rows.numel()
    key = torch.rand(E, device=rows.device, generator=gen, dtype=torch.float64)
    order = torch.argsort(rows.double() + key)                 # one sort by (row, key): rows are integers, keys in [0, 1)
    rank = torch.arange(E, device=rows.device) - rp[:-1].long()[rows[order]]
    keep = torch.zeros(E, dtype=torch.bool, device=rows.device)
    keep[order[rank < k]] = True
    eid = keep.nonzero().view(-1)                              # (CSR order restored)
    rp_s = torch.zeros_like(rp)
    rp_s[1:] = torch.cumsum(torch.clamp(rp[1:] - rp[:-1], max=k), 0)
    return rp_s, eid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("graphs", nargs="*", default=DEFAULT)
    ap.add_argument("--fanouts", type=str, default="10,25")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--skip-epochs", action="store_true")
    args = ap.parse_args()
    import torch
    import TCGNN
    import tcgnn_capi as C
    import tcgnn_graph as G
    import tcgnn_harness as H
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    print("build %s" % C.build_id())
    misses = []
    for spec in args.graphs:
        shape, gen = spec.split(":")
        n, nnz, in_dim, classes = G.SHAPES[shape]
        rp, col = G.GENERATORS[gen](n, nnz, seed=0, device=dev)
        E = col.numel()
        lens = rp[1:] - rp[:-1]
        print("%s / %s: N = %d, E = %d, longest row %d" % (shape, gen, n, E, int(lens.max())), flush=True)
        g = torch.Generator(device=dev).manual_seed(0)
        X = torch.randn(n, 64, device=dev, generator=g)
        Ef = torch.randn(E, 64, device=dev, generator=g)
        full = {"forward_max": median_ms(lambda: TCGNN.forward_max(X, rp, col), args.reps, args.warmup),
                "forward_stats": median_ms(lambda: TCGNN.forward_stats(X, rp, col), args.reps, args.warmup),
                "forward_ue": median_ms(lambda: TCGNN.forward_ue(X, Ef, rp, col), args.reps, args.warmup)}
        print("  full graph, D = 64: " + "  ".join("%s %.3f ms" % kv for kv in full.items()), flush=True)
        need = C._sz(0)
        C.check(C.lib.tcgnn_sample_workspace_bytes(n, C.ctypes.byref(need)), "tcgnn_sample_workspace_bytes")
        ws = torch.empty(need.value + 256, dtype=torch.uint8, device=dev)
        wsp = ws.data_ptr() + (-ws.data_ptr()) % 256
        rows = torch.repeat_interleave(torch.arange(n, device=dev), lens.long()) if not args.skip_torch else None
        for k in (int(t) for t in args.fanouts.split(",")):
            rp_s = torch.empty(n + 1, dtype=torch.int32, device=dev)
            kept = C._i64(0)

            def count():
                C.check(C.lib.tcgnn_sample_neighbors_count(rp.data_ptr(), None, n, E, k, rp_s.data_ptr(), wsp, need.value, C.ctypes.byref(kept), stream), "count")
            t_count = median_ms(count, args.reps, args.warmup, host=True)
            col_s = torch.empty(kept.value, dtype=torch.int32, device=dev)
            eid = torch.empty(kept.value, dtype=torch.int32, device=dev)
            t_sel = median_ms(lambda: C.check(C.lib.tcgnn_sample_neighbors(rp.data_ptr(), col.data_ptr(), None, rp_s.data_ptr(), n, E, k, 7, col_s.data_ptr(),
                                                                           eid.data_ptr(), stream), "select"), args.reps, args.warmup)
            t_mod = median_ms(lambda: TCGNN.sample_neighbors(rp, col, k, 7), args.reps, args.warmup, host=True)
            line = "  fanout %3d: E' = %d (%.1f %%)  count %.3f ms  select %.3f ms  sample_neighbors %.3f ms" % (k, kept.value, 100.0 * kept.value / E, t_count, t_sel, t_mod)
            if not args.skip_torch:
                try:
                    gt = torch.Generator(device=dev).manual_seed(k)
                    t_torch = median_ms(lambda: torch_sample(rp, rows, k, gt), max(3, args.reps // 4), 1, host=True)
                    line += " | torch composition %.3f ms" % t_torch
                    if t_torch < t_mod:
                        misses.append("%s/%s fanout %d: sample_neighbors %.3f ms loses to the torch composition %.3f ms" % (shape, gen, k, t_mod, t_torch))
                except RuntimeError as e:
                    line += " | torch composition: %s" % str(e).splitlines()[0][:80]
                torch.cuda.empty_cache()
            print(line, flush=True)
            Efs = Ef[eid.long()].contiguous()
            part = {"forward_max": median_ms(lambda: TCGNN.forward_max(X, rp_s, col_s), args.reps, args.warmup),
                    "forward_stats": median_ms(lambda: TCGNN.forward_stats(X, rp_s, col_s), args.reps, args.warmup),
                    "forward_ue": median_ms(lambda: TCGNN.forward_ue(X, Efs, rp_s, col_s), args.reps, args.warmup)}
            print("    sampled graph, D = 64: " + "  ".join("%s %.3f ms (full / sampled %.1f)" % (name, t, full[name] / t) for name, t in part.items()), flush=True)
            misses += ["%s/%s fanout %d: %s slower on the sampled graph (%.3f ms against %.3f ms)" % (shape, gen, k, name, t, full[name])
                       for name, t in part.items() if t > full[name]]
            del Efs, col_s, eid
        del X, Ef, rows
        torch.cuda.empty_cache()
        if not args.skip_epochs:
            nw = (n + 15) // 16
            bp = torch.zeros(nw, dtype=torch.int32, device=dev); e2c = torch.zeros(E, dtype=torch.int32, device=dev); e2r = torch.zeros(E, dtype=torch.int32, device=dev)
            TCGNN.preprocess_gpu(col, rp, n, 16, 8, bp, e2c, e2r)
            meta = (rp, col, bp, e2c, e2r)
            gen_ = torch.Generator().manual_seed(0)
            x = torch.randn(n, in_dim, generator=gen_).to(dev)
            y = torch.randint(0, classes, (n,), generator=gen_).to(dev)
            for model, kw in (("sage", {"aggregator": "max"}), ("pna", {}), ("gine", {})):
                # (GINE projects edge_attr to the layer's input width: [E, in_dim] floats - 64 input features there, as tools/bench_gine.py)
                xin = x[:, :64].contiguous() if model == "gine" else x
                in_dim = xin.shape[1]
                base = H.time_training(model, meta, xin, y, in_dim, 64, classes, 2, 5, warmup=2, **kw)
                samp = H.time_training(model, meta, xin, y, in_dim, 64, classes, 2, 5, warmup=2, fanout=[25, 25], **kw)
                print("  %-4s epoch (%d -> 64 -> %d): full %.3f ms (loss %.4f) | fanout 25: sample %.3f + plan %.3f + train %.3f = %.3f ms (full-graph loss %.4f)" % (
                    model, in_dim, classes, base["train_ms"], base["final_loss"], samp["sample_ms"], samp["plan_ms"], samp["train_ms"], samp["epoch_ms"],
                    samp["final_loss"]), flush=True)
                if samp["epoch_ms"] > base["train_ms"]:
                    misses.append("%s/%s %s epoch: %.3f ms with fanout 25 against %.3f ms" % (shape, gen, model, samp["epoch_ms"], base["train_ms"]))
            del x, y
        TCGNN.clear_plan_cache()
        torch.cuda.empty_cache()
    print("misses: " + ("; ".join(misses) if misses else "none"))


if __name__ == "__main__":
    main()
