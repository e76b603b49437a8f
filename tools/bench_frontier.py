#!/usr/bin/env python3
"""Seed-list sampling (TCGNN.sample_rows / extend_nodes / compact_rows_graph, tcgnn_layers.sample_batch_rows, --sampler rows) against the
dense path it stands beside (sample_layers + compact_layers: one wavefront per row of the graph behind a frontier mask).

Per graph, one mini-batch of --batch seeds with fan-outs --fanouts (input layer first).  Both paths' CompactBatch are compared element
by element before anything is timed.  Median (min .. max) of --reps after --warmup, a host clock around device synchronisations:
  1. the two halves     sample_layers | compact_layers against sample_layers_rows | compact_layers_rows - what the harness times as
                        sample_ms and compact_ms - and the rows path's calls one by one;
  2. one training step  SAGE-max, hidden 64: sample / compact / plan / train with either sampler;
  3. an epoch           tcgnn_harness.time_training(batch_size=..., sampler=...) for SAGE-max: ceil(N / batch) steps, split into its parts.
GRAPHS: name:generator separated by spaces; default sbm_reddit, the R-MAT Reddit shape and the products SBM.  A win counts when the
rows path's slowest repetition is faster than the dense path's fastest; the last line names every graph where it is not."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tc-gnn_atc23_amd")):
    sys.path.insert(0, p)

DEFAULT = ["reddit:sbm_reddit", "reddit:rmat", "ogbn-products:sbm"]


def timed(fn, reps, warmup):
    """(median, min, max) ms of fn between device synchronisations"""
    import numpy as np
    import torch
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter(); fn(); torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return float(np.median(times)), float(min(times)), float(max(times))


def fmt(t):
    return "%.3f (%.3f .. %.3f)" % t


def same_batch(a, b):
    import torch
    ok = torch.equal(a.nodes, b.nodes) and torch.equal(a.seed_pos, b.seed_pos) and torch.equal(a.new_id, b.new_id) and len(a.metas) == len(b.metas)
    for ma, mb, ea, eb in zip(a.metas, b.metas, a.eids, b.eids):
        ok = ok and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(ma, mb)) and torch.equal(ea, eb)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("graphs", nargs="*", default=DEFAULT)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--fanouts", type=str, default="25,10")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-epochs", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import TCGNN
    import tcgnn_capi as C
    import tcgnn_graph as G
    import tcgnn_harness as H
    import tcgnn_layers as L
    dev = torch.device("cuda:0")
    fanouts = [int(t) for t in args.fanouts.split(",")]
    print("build %s" % C.build_id())
    misses = []
    for spec in args.graphs:
        shape, gen = spec.split(":")
        n, nnz, in_dim, classes = G.SHAPES[shape]
        rp, col = G.GENERATORS[gen](n, nnz, seed=0, device=dev)
        csr = (rp, col)
        print("%s / %s: N = %d, E = %d, batch %d, fan-outs %s" % (shape, gen, n, col.numel(), args.batch, fanouts), flush=True)
        seeds = H.epoch_order(n, 0, 0)[:args.batch].to(dev)
        dense, rows = L.sample_batch(csr, seeds, fanouts, 5, plan=False), L.sample_batch_rows(csr, seeds, fanouts, 5, plan=False)
        assert same_batch(rows, dense), "sample_batch_rows and sample_batch disagree"
        M = rows.nodes.numel()
        hops, nodes, new_id = L.sample_layers_rows(csr, seeds, fanouts, 5)
        print("  equal batches: True; M = %d (M / N = %.4f); row lists %s; E' per layer %s"
              % (M, M / n, [h[0].numel() for h in hops], [h[2].numel() for h in hops]))

        # ---- 1. the two halves, and the rows path's calls
        graphs = L.sample_layers(csr, seeds, fanouts, 5)
        t_ds = timed(lambda: L.sample_layers(csr, seeds, fanouts, 5), args.reps, args.warmup)
        t_dc = timed(lambda: L.compact_layers(graphs, seeds, plan=False), args.reps, args.warmup)
        t_rs = timed(lambda: L.sample_layers_rows(csr, seeds, fanouts, 5), args.reps, args.warmup)
        t_rc = timed(lambda: L.compact_layers_rows(hops, nodes, new_id, seeds, plan=False), args.reps, args.warmup)
        print("  sample : dense sample_layers %s ms | rows sample_layers_rows %s ms" % (fmt(t_ds), fmt(t_rs)))
        print("  compact: dense compact_layers %s ms | rows compact_layers_rows %s ms" % (fmt(t_dc), fmt(t_rc)))
        print("  both   : dense %.3f ms | rows %.3f ms (medians)" % (t_ds[0] + t_dc[0], t_rs[0] + t_rc[0]))
        keep = torch.zeros(n, dtype=torch.uint8, device=dev)
        mask0 = torch.zeros(n, dtype=torch.uint8, device=dev).index_fill_(0, hops[0][0].long(), 1)   # hops[0]: the widest list
        t_one = timed(lambda: TCGNN.sample_rows(rp, col, hops[0][0], fanouts[0], 5 + len(fanouts) - 1), args.reps, args.warmup)
        t_dense_one = timed(lambda: TCGNN.sample_neighbors(rp, col, fanouts[0], 5 + len(fanouts) - 1, mask0), args.reps, args.warmup)
        t_ext = timed(lambda: TCGNN.extend_nodes(keep, hops[0][2]), args.reps, args.warmup)
        t_blk = timed(lambda: TCGNN.compact_rows_graph(hops[0][0], hops[0][1], hops[0][2], nodes, new_id), args.reps, args.warmup)
        print("    calls on the widest hop (%d rows, E' = %d): sample_rows %s ms (sample_neighbors behind the same rows' mask %s ms)  extend_nodes %s ms  "
              "compact_rows_graph %s ms" % (hops[0][0].numel(), hops[0][2].numel(), fmt(t_one), fmt(t_dense_one), fmt(t_ext), fmt(t_blk)), flush=True)
        del keep, mask0
        if t_rs[2] >= t_ds[1]:
            misses.append("%s/%s (M / N = %.2f): rows sample %s ms is not outside dense %s ms" % (shape, gen, M / n, fmt(t_rs), fmt(t_ds)))

        gen_ = torch.Generator().manual_seed(0)
        x = torch.randn(n, in_dim, generator=gen_).to(dev)
        y = torch.randint(0, classes, (n,), generator=gen_).to(dev)

        # ---- 2. one SAGE-max training step with either sampler
        if not args.skip_steps:
            torch.manual_seed(0)
            net = H.Net(lambda a, b, **kw: L.SAGEConv(a, b, aggregator="max", **kw), in_dim, 64, classes, len(fanouts), directed=True).to(dev)
            opt = H.make_adam(net.parameters())

            def step(sampler):
                ms, t = {}, None

                def lap(key):
                    nonlocal t
                    torch.cuda.synchronize()
                    now = time.perf_counter()
                    if key:
                        ms[key] = (now - t) * 1e3
                    t = now

                lap(None)
                if sampler == "rows":
                    drawn = L.sample_layers_rows(csr, seeds, fanouts, 5)
                    lap("sample")
                    batch = L.compact_layers_rows(*drawn, seeds, plan=False)
                else:
                    drawn = L.sample_layers(csr, seeds, fanouts, 5)
                    lap("sample")
                    batch = L.compact_layers(drawn, seeds, plan=False)
                xb = x[batch.nodes.long()]
                lap("compact")
                for m in batch.metas:
                    TCGNN.transpose_graph(m[0], m[1])
                lap("plan")
                net.train()
                opt.zero_grad()
                loss = H.node_nll_loss(net(xb, batch.metas)[batch.seed_pos], y[seeds])
                loss.backward()
                opt.step()
                lap("train")
                return ms

            for sampler in ("dense", "rows"):
                for _ in range(args.warmup):
                    step(sampler)
                runs = [step(sampler) for _ in range(args.reps)]
                med = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
                total = [sum(r.values()) for r in runs]
                print("  sage-max step, sampler %-5s: sample %.3f + compact %.3f + plan %.3f + train %.3f = %.3f ms (%.3f .. %.3f)"
                      % (sampler, med["sample"], med["compact"], med["plan"], med["train"], float(np.median(total)), min(total), max(total)), flush=True)
                TCGNN.clear_plan_cache()
            del net, opt
            torch.cuda.empty_cache()

        # ---- 3. an epoch of mini-batches with either sampler
        if not args.skip_epochs:
            E = col.numel()
            bp = torch.zeros((n + 15) // 16, dtype=torch.int32, device=dev); e2c = torch.zeros(E, dtype=torch.int32, device=dev); e2r = torch.zeros(E, dtype=torch.int32, device=dev)
            TCGNN.preprocess_gpu(col, rp, n, 16, 8, bp, e2c, e2r)
            meta = (rp, col, bp, e2c, e2r)
            out = {}
            for sampler in ("dense", "rows"):
                mb = out[sampler] = H.time_training("sage", meta, x, y, in_dim, 64, classes, len(fanouts), 1, warmup=3, aggregator="max", fanout=fanouts,
                                                    batch_size=args.batch, sampler=sampler)
                print("  sage --batch-size %d --sampler %-5s epoch: %d steps, mean M %.0f (%.4f N): sample %.1f + compact %.1f + plan %.1f + train %.1f = %.1f ms "
                      "(full-graph loss %.6f)" % (args.batch, sampler, mb["batches"], mb["mean_block_nodes"], mb["mean_block_nodes"] / n, mb["sample_ms"],
                                                 mb["compact_ms"], mb["plan_ms"], mb["train_ms"], mb["epoch_ms"], mb["final_loss"]), flush=True)
            print("    equal losses: %s" % (out["dense"]["final_loss"] == out["rows"]["final_loss"]))
            del bp, e2c, e2r, meta
        del x, y
        TCGNN.clear_plan_cache()
        torch.cuda.empty_cache()
    print("misses: " + ("; ".join(misses) if misses else "none"))


if __name__ == "__main__":
    main()
