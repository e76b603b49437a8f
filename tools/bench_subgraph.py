#!/usr/bin/env python3
"""Subgraph sampling (TCGNN.random_walk / induce_subgraph, tcgnn_layers.subgraph_batch / saint_batch, --sampler saint / cluster) against
what a user would compose from torch and from the library's older calls.

Per graph, median (min .. max) of --reps after --warmup, a host clock around device synchronisations, all contenders in one run, every
result compared element by element before anything is timed:
  1. induce_subgraph  on three node sets - the nodes that walks of --walk-length steps from 1 024 and from 3 000 roots visit, and one
                      contiguous range of N / 50 ids - against
                        (a) torch: repeat_interleave of the row ids, new_id[col] >= 0, a cumsum, two masked gathers;
                        (b) sample_rows(fanout=None) + the same filter in torch + compact_rows_graph;
  2. random_walk      against a torch walk (per step a randint scaled by the degree and two gathers; other draws, so only shapes and
                      edge membership are compared);
  3. epochs           one SAGE-max step and a --batch-size epoch for --sampler saint and cluster beside --sampler rows (fan-outs
                      25, 10): reported, not judged - the batches differ in kind.
GRAPHS: name:generator separated by spaces; default sbm_reddit, the R-MAT Reddit shape and the products SBM.  A win counts when
induce_subgraph's slowest repetition is faster than a baseline's fastest; the last line names every case where it is not."""
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


def torch_filter(rp_s, col_s, eid_s, new_id, M):
    """the edges of a row-list graph whose column has a new id: (row pointers, new ids, positions)"""
    import torch
    d = (rp_s[1:] - rp_s[:-1]).long()
    row = torch.repeat_interleave(torch.arange(M, device=rp_s.device), d)
    ids = new_id[col_s.long()]
    has = ids >= 0
    counts = torch.bincount(row[has], minlength=M)
    rp_b = torch.cat([counts.new_zeros(1), counts.cumsum(0)]).to(torch.int32)
    return rp_b, ids[has], eid_s[has]


def torch_induce(rp, col, nodes, new_id):
    """baseline (a): nothing but torch"""
    import torch
    v = nodes.long()
    lo = rp[v].long()
    d = rp[v + 1].long() - lo
    start = d.cumsum(0) - d
    row = torch.repeat_interleave(torch.arange(v.numel(), device=rp.device), d)
    pos = torch.arange(row.numel(), device=rp.device) + (lo - start)[row]
    ids = new_id[col[pos].long()]
    has = ids >= 0
    counts = torch.bincount(row[has], minlength=v.numel())
    rp_b = torch.cat([counts.new_zeros(1), counts.cumsum(0)]).to(torch.int32)
    return rp_b, ids[has], pos[has].to(torch.int32)


def library_induce(T, rp, col, nodes, new_id):
    """baseline (b): the library's older calls around the torch filter"""
    rp_s, col_s, eid_s = T.sample_rows(rp, col, nodes, None, 0)
    rp_f, _, eid = torch_filter(rp_s, col_s, eid_s, new_id, nodes.numel())
    keep = new_id[col_s.long()] >= 0
    rp_b, col_b = T.compact_rows_graph(nodes, rp_f, col_s[keep].contiguous(), nodes, new_id)
    return rp_b, col_b, eid


def torch_walk(rp, col, starts, length, gen):
    import torch
    v = starts.long()
    out = [v]
    for _ in range(length):
        lo = rp[v].long()
        d = rp[v + 1].long() - lo
        j = (torch.randint(0, 1 << 31, v.shape, device=v.device, generator=gen) * d) >> 31
        v = torch.where(d > 0, col[(lo + j).clamp_max(col.numel() - 1)].long(), v)
        out.append(v)
    return torch.stack(out, 1).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("graphs", nargs="*", default=DEFAULT)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--walk-length", dest="walk_length", type=int, default=2)
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
        print("%s / %s: N = %d, E = %d" % (shape, gen, n, col.numel()), flush=True)
        order = H.epoch_order(n, 0, 0).to(dev)

        # ---- 1. induce_subgraph on three node sets
        sets = []
        for roots in (1024, 3000):
            walks = TCGNN.random_walk(rp, col, order[:roots].to(torch.int32), args.walk_length, 5)
            sets.append(("%d roots, walks of %d" % (roots, args.walk_length), walks.reshape(-1)))
        sets.append(("a range of N / 50 ids", torch.arange(n // 3, n // 3 + n // 50, dtype=torch.int32, device=dev)))
        for what, ids in sets:
            nodes, new_id = TCGNN.extend_nodes(torch.zeros(n, dtype=torch.uint8, device=dev), ids)
            ours = TCGNN.induce_subgraph(rp, col, nodes, new_id)
            for name, other in (("torch", torch_induce(rp, col, nodes, new_id)), ("library", library_induce(TCGNN, rp, col, nodes, new_id))):
                assert all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(ours, other)), "induce_subgraph and the %s composition disagree" % name
            rows_edges = int((rp[nodes.long() + 1] - rp[nodes.long()]).sum())
            t_us = timed(lambda: TCGNN.induce_subgraph(rp, col, nodes, new_id), args.reps, args.warmup)
            t_a = timed(lambda: torch_induce(rp, col, nodes, new_id), args.reps, args.warmup)
            t_b = timed(lambda: library_induce(TCGNN, rp, col, nodes, new_id), args.reps, args.warmup)
            print("  induce, %s: M = %d, %d edges in the listed rows, E_b = %d (equal results: True)\n"
                  "    induce_subgraph %s ms | (a) torch %s ms | (b) sample_rows + filter + compact_rows_graph %s ms"
                  % (what, nodes.numel(), rows_edges, ours[1].numel(), fmt(t_us), fmt(t_a), fmt(t_b)), flush=True)
            for name, t in (("(a) torch", t_a), ("(b) library", t_b)):
                if t_us[2] >= t[1]:
                    misses.append("%s/%s, %s: induce_subgraph %s ms is not outside %s %s ms" % (shape, gen, what, fmt(t_us), name, fmt(t)))

        # ---- 2. random_walk against a torch walk
        for roots in (1024, 3000):
            starts = order[:roots].to(torch.int32)
            g = torch.Generator(device=dev).manual_seed(0)
            ours, theirs = TCGNN.random_walk(rp, col, starts, args.walk_length, 5), torch_walk(rp, col, starts, args.walk_length, g)
            assert ours.shape == theirs.shape and torch.equal(ours[:, 0], theirs[:, 0])
            t_us = timed(lambda: TCGNN.random_walk(rp, col, starts, args.walk_length, 5), args.reps, args.warmup)
            t_t = timed(lambda: torch_walk(rp, col, starts, args.walk_length, g), args.reps, args.warmup)
            print("  walk, %d roots, %d steps: random_walk %s ms | torch %s ms" % (roots, args.walk_length, fmt(t_us), fmt(t_t)), flush=True)
            if t_us[2] >= t_t[1]:
                misses.append("%s/%s, %d walks: random_walk %s ms is not outside torch %s ms" % (shape, gen, roots, fmt(t_us), fmt(t_t)))

        gen_ = torch.Generator().manual_seed(0)
        x = torch.randn(n, in_dim, generator=gen_).to(dev)
        y = torch.randint(0, classes, (n,), generator=gen_).to(dev)

        # ---- 3. one SAGE-max step on a saint batch, in its parts
        if not args.skip_steps:
            torch.manual_seed(0)
            net = H.Net(lambda a, b, **kw: L.SAGEConv(a, b, aggregator="max", **kw), in_dim, 64, classes, len(fanouts), directed=True).to(dev)
            opt = H.make_adam(net.parameters())
            roots = order[:args.batch].to(torch.int32)

            def step():
                ms, t = {}, None

                def lap(key):
                    nonlocal t
                    torch.cuda.synchronize()
                    now = time.perf_counter()
                    if key:
                        ms[key] = (now - t) * 1e3
                    t = now

                lap(None)
                ids = TCGNN.random_walk(rp, col, roots, args.walk_length, 5).reshape(-1)
                lap("sample")
                batch = L.subgraph_batch(csr, ids, plan=False, layers=len(fanouts))
                at = batch.nodes.long()
                xb, yb = x[at], y[at]
                lap("compact")
                TCGNN.transpose_graph(batch.metas[0][0], batch.metas[0][1])
                lap("plan")
                net.train()
                opt.zero_grad()
                loss = H.node_nll_loss(net(xb, batch.metas), yb)
                loss.backward()
                opt.step()
                lap("train")
                return ms, batch.nodes.numel(), batch.metas[0][1].numel()

            for _ in range(args.warmup):
                step()
            runs = [step() for _ in range(args.reps)]
            med = {k: float(np.median([r[0][k] for r in runs])) for k in runs[0][0]}
            total = [sum(r[0].values()) for r in runs]
            print("  sage-max step, saint batch of %d roots (M = %d, E_b = %d): sample %.3f + compact %.3f + plan %.3f + train %.3f = %.3f ms (%.3f .. %.3f)"
                  % (args.batch, runs[0][1], runs[0][2], med["sample"], med["compact"], med["plan"], med["train"], float(np.median(total)), min(total),
                     max(total)), flush=True)
            TCGNN.clear_plan_cache()
            del net, opt
            torch.cuda.empty_cache()

        # ---- 4. an epoch of mini-batches with each sampler
        if not args.skip_epochs:
            E = col.numel()
            bp = torch.zeros((n + 15) // 16, dtype=torch.int32, device=dev); e2c = torch.zeros(E, dtype=torch.int32, device=dev); e2r = torch.zeros(E, dtype=torch.int32, device=dev)
            TCGNN.preprocess_gpu(col, rp, n, 16, 8, bp, e2c, e2r)
            meta = (rp, col, bp, e2c, e2r)
            for sampler, kw in (("rows", {"fanout": fanouts}), ("saint", {"walk_length": args.walk_length}), ("cluster", {})):
                mb = H.time_training("sage", meta, x, y, in_dim, 64, classes, len(fanouts), 1, warmup=3, aggregator="max", batch_size=args.batch,
                                     sampler=sampler, **kw)
                print("  sage --batch-size %d --sampler %-7s epoch: %d steps, mean M %.0f (%.4f N)%s: sample %.1f + compact %.1f + plan %.1f + train %.1f = %.1f ms "
                      "(full-graph loss %.6f)" % (args.batch, sampler, mb["batches"], mb["mean_block_nodes"], mb["mean_block_nodes"] / n,
                                                 ", mean E_b %.0f" % mb["mean_block_edges"] if "mean_block_edges" in mb else "", mb["sample_ms"],
                                                 mb["compact_ms"], mb["plan_ms"], mb["train_ms"], mb["epoch_ms"], mb["final_loss"]), flush=True)
            del bp, e2c, e2r, meta
        del x, y
        TCGNN.clear_plan_cache()
        torch.cuda.empty_cache()
    print("misses: " + ("; ".join(misses) if misses else "none"))


if __name__ == "__main__":
    main()
