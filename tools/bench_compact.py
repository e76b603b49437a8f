#!/usr/bin/env python3
"""Relabelled mini-batch blocks (TCGNN.compact_nodes / compact_graph, tcgnn_layers.sample_batch, --batch-size) against what they replace.

Per graph, one mini-batch of --batch seeds with fan-outs --fanouts (input layer first); median of --reps after --warmup:
  1. compaction       compact_nodes + compact_graph of both layer graphs (the module's calls: mark, count, nodes, relabel, the output
                      allocations and the one synchronisation; a host clock around a device synchronisation) against the torch composition
                      torch.unique(cat(seeds, columns of every layer), return_inverse=True) + the pointer gather.  Both results are
                      compared element by element before anything is timed; the C calls alone are timed with HIP events.
  2. one training step  SAGE-max, PNA and GCN, hidden 64: on the compact batch (sample / compact / plan / train) against the same batch
                      uncompacted - sample_layers, the model over all N nodes, the loss on the seeds (sample / plan / train).
  3. an epoch         tcgnn_harness.time_training(batch_size=...) for SAGE-max: one epoch of ceil(N / batch) steps, split into its parts;
                      beside it --fanout 25 full-node-set epochs.  Different training regimes: where the step counts can be made equal
                      (at most --equal-steps batches per epoch) the fan-out regime runs as many epochs as the mini-batch epoch has steps and
                      both full-graph losses are printed; no speed-up is claimed across regimes.
GRAPHS: name:generator separated by spaces; default sbm_reddit, the R-MAT Reddit shape and the products SBM.  The last line names every
miss: a compaction that loses to the torch composition, a compact step slower than the uncompacted one."""
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


def torch_compact(seeds, layers):
    """the composition: (nodes, [(rp_b, col_b)]) by one sort of everything that names a node"""
    import torch
    named = torch.cat([seeds.int()] + [g[1] for g in layers])
    nodes, inverse = torch.unique(named, return_inverse=True)
    out, at = [], seeds.numel()
    for rp, col, _ in layers:
        col_b = inverse[at:at + col.numel()].int()
        at += col.numel()
        out.append((torch.cat([rp[nodes.long()], rp[-1:]]), col_b))
    return nodes, out


class Laps:
    """host clock between device synchronisations, summed per key"""

    def __init__(self):
        self.ms = {}
        self.t = None

    def start(self):
        import torch
        torch.cuda.synchronize()
        self.t = time.perf_counter()

    def lap(self, key):
        import torch
        torch.cuda.synchronize()
        now = time.perf_counter()
        self.ms[key] = self.ms.get(key, 0.0) + (now - self.t) * 1e3
        self.t = now


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("graphs", nargs="*", default=DEFAULT)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--fanouts", type=str, default="25,10")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--models", type=str, default="sage,pna,gcn")
    ap.add_argument("--equal-steps", type=int, default=300, help="largest number of batches per epoch at which part 3 runs as many fan-out epochs")
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
    stream = torch.cuda.current_stream().cuda_stream
    fanouts = [int(t) for t in args.fanouts.split(",")]
    print("build %s" % C.build_id())
    misses = []
    for spec in args.graphs:
        shape, gen = spec.split(":")
        n, nnz, in_dim, classes = G.SHAPES[shape]
        rp, col = G.GENERATORS[gen](n, nnz, seed=0, device=dev)
        E = col.numel()
        print("%s / %s: N = %d, E = %d, batch %d, fan-outs %s" % (shape, gen, n, E, args.batch, fanouts), flush=True)
        seeds = H.epoch_order(n, 0, 0)[:args.batch].to(dev)
        t_sample = median_ms(lambda: L.sample_layers((rp, col), seeds, fanouts, 5), args.reps, args.warmup, host=True)
        layers = L.sample_layers((rp, col), seeds, fanouts, 5)
        pairs = [(g[0], g[1]) for g in layers]
        keep = torch.zeros(n, dtype=torch.uint8, device=dev).index_fill_(0, seeds, 1)

        # ---- 1. compaction against the torch composition
        def ours():
            nodes, new_id = TCGNN.compact_nodes(pairs, keep)
            return nodes, [TCGNN.compact_graph(a, b, nodes, new_id) for a, b in pairs]

        nodes, blocks = ours()
        t_nodes, t_blocks = torch_compact(seeds, layers)
        same = torch.equal(nodes, t_nodes) and all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(blocks, t_blocks))
        assert same, "the library's compaction and the torch composition disagree"
        M = nodes.numel()
        t_ours = median_ms(ours, args.reps, args.warmup, host=True)
        t_torch = median_ms(lambda: torch_compact(seeds, layers), args.reps, args.warmup, host=True)
        # the C calls alone on preallocated outputs, HIP events (the count call by a host clock: it synchronises)
        need = C._sz(0)
        C.check(C.lib.tcgnn_compact_workspace_bytes(n, C.ctypes.byref(need)), "tcgnn_compact_workspace_bytes")
        ws = torch.empty(need.value + 256, dtype=torch.uint8, device=dev)
        wsp = ws.data_ptr() + (-ws.data_ptr()) % 256
        mask, new_id, kept = keep.clone(), torch.empty(n, dtype=torch.int32, device=dev), C._i32(0)
        C.check(C.lib.tcgnn_compact_begin(n, wsp, need.value, stream), "begin")

        def mark():
            for a, b in pairs:
                C.check(C.lib.tcgnn_compact_mark(a.data_ptr(), b.data_ptr(), n, b.numel(), mask.data_ptr(), wsp, need.value, stream), "mark")

        def relabel():
            for (a, b), (a_b, b_b) in zip(pairs, blocks):
                C.check(C.lib.tcgnn_compact_graph(a.data_ptr(), b.data_ptr(), new_id.data_ptr(), nodes.data_ptr(), n, M, b.numel(), a_b.data_ptr(), b_b.data_ptr(),
                                                  stream), "graph")

        t_mark = median_ms(mark, args.reps, args.warmup)
        t_count = median_ms(lambda: C.check(C.lib.tcgnn_compact_count(mask.data_ptr(), n, new_id.data_ptr(), wsp, need.value, C.ctypes.byref(kept), stream),
                                            "count"), args.reps, args.warmup, host=True)
        assert kept.value == M
        t_list = median_ms(lambda: C.check(C.lib.tcgnn_compact_nodes(new_id.data_ptr(), n, M, nodes.data_ptr(), stream), "nodes"), args.reps, args.warmup)
        t_rel = median_ms(relabel, args.reps, args.warmup)
        print("  sample_layers %.3f ms; E' per layer %s; M = %d (M / N = %.4f)" % (t_sample, [g[1].numel() for g in layers], M, M / n))
        print("  compaction: compact_nodes + %d x compact_graph %.3f ms | torch composition (unique over %d ids + pointer gather) %.3f ms | equal outputs: %s"
              % (len(pairs), t_ours, seeds.numel() + sum(g[1].numel() for g in layers), t_torch, same))
        print("    C calls: mark (both layers) %.3f ms  count %.3f ms  nodes %.3f ms  relabel (both layers) %.3f ms" % (t_mark, t_count, t_list, t_rel), flush=True)
        if t_ours > t_torch:
            misses.append("%s/%s compaction %.3f ms loses to the torch composition %.3f ms" % (shape, gen, t_ours, t_torch))
        del ws, mask, new_id, blocks, t_blocks

        gen_ = torch.Generator().manual_seed(0)
        x = torch.randn(n, in_dim, generator=gen_).to(dev)
        y = torch.randint(0, classes, (n,), generator=gen_).to(dev)

        # ---- 2. one training step on the compact batch against the same batch uncompacted
        for model in ([] if args.skip_steps else args.models.split(",")):
            if model == "sage":
                net = H.Net(lambda a, b, **kw: L.SAGEConv(a, b, aggregator="max", **kw), in_dim, 64, classes, len(fanouts), directed=True)
            elif model == "pna":
                net = H.Net(L.PNAConv, in_dim, 64, classes, len(fanouts))
            else:
                net = H.Net(L.GCNConv, in_dim, 64, classes, len(fanouts), directed=True)
            torch.manual_seed(0)
            net = net.to(dev)
            opt = H.make_adam(net.parameters())
            planned = model == "gcn"
            pad = tuple(torch.empty(0, dtype=torch.int32, device=dev) for _ in range(3))

            def step(compact, laps):
                laps.start()
                graphs = L.sample_layers((rp, col), seeds, fanouts, 5)
                laps.lap("sample")
                if compact:
                    batch = L.compact_layers(graphs, seeds, plan=False)
                    metas, xb, rows = batch.metas, x[batch.nodes.long()], batch.seed_pos
                    laps.lap("compact")
                else:
                    metas, xb, rows = [(g[0], g[1]) + pad for g in graphs], x, seeds
                if planned:
                    metas = [L.csr_meta(m[0], m[1]) for m in metas]
                laps.lap("plan")
                net.train()
                opt.zero_grad()
                loss = H.node_nll_loss(net(xb, metas)[rows], y[seeds])
                loss.backward()
                opt.step()
                laps.lap("train")

            res = {}
            for compact in (False, True):
                for _ in range(args.warmup):
                    step(compact, Laps())
                runs = []
                for _ in range(args.reps):
                    laps = Laps()
                    step(compact, laps)
                    runs.append(laps.ms)
                res[compact] = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
                res[compact]["step"] = float(np.median([sum(r.values()) for r in runs]))
                TCGNN.clear_plan_cache()
            u, c = res[False], res[True]
            print("  %-4s step (%d -> 64 -> %d): uncompacted sample %.3f + plan %.3f + train %.3f = %.3f ms | compact sample %.3f + compact %.3f + plan %.3f + train %.3f = %.3f ms"
                  % (model, in_dim, classes, u["sample"], u["plan"], u["train"], u["step"], c["sample"], c["compact"], c["plan"], c["train"], c["step"]), flush=True)
            if c["step"] > u["step"]:
                misses.append("%s/%s %s step: compact %.3f ms against uncompacted %.3f ms" % (shape, gen, model, c["step"], u["step"]))
            del net, opt
            torch.cuda.empty_cache()

        # ---- 3. an epoch of mini-batches beside full-node-set fan-out epochs (different regimes)
        if not args.skip_epochs:
            nw = (n + 15) // 16
            bp = torch.zeros(nw, dtype=torch.int32, device=dev); e2c = torch.zeros(E, dtype=torch.int32, device=dev); e2r = torch.zeros(E, dtype=torch.int32, device=dev)
            TCGNN.preprocess_gpu(col, rp, n, 16, 8, bp, e2c, e2r)
            meta = (rp, col, bp, e2c, e2r)
            mb = H.time_training("sage", meta, x, y, in_dim, 64, classes, len(fanouts), 1, warmup=3, aggregator="max", fanout=fanouts, batch_size=args.batch)
            print("  sage --batch-size %d epoch: %d steps, mean M %.0f (%.4f N): sample %.1f + compact %.1f + plan %.1f + train %.1f = %.1f ms (full-graph loss %.4f)"
                  % (args.batch, mb["batches"], mb["mean_block_nodes"], mb["mean_block_nodes"] / n, mb["sample_ms"], mb["compact_ms"], mb["plan_ms"], mb["train_ms"],
                     mb["epoch_ms"], mb["final_loss"]), flush=True)
            equal = mb["batches"] <= args.equal_steps
            fo = H.time_training("sage", meta, x, y, in_dim, 64, classes, len(fanouts), mb["batches"] if equal else 5, warmup=3, aggregator="max", fanout=[25] * len(fanouts))
            print("  sage --fanout 25 full-node-set epoch (one step each): sample %.3f + plan %.3f + train %.3f = %.3f ms; full-graph loss after %d steps %.4f%s"
                  % (fo["sample_ms"], fo["plan_ms"], fo["train_ms"], fo["epoch_ms"], 3 + (mb["batches"] if equal else 5), fo["final_loss"],
                     " (the mini-batch epoch above: %d steps)" % (3 + mb["batches"]) if equal else " - step counts differ, the losses are not comparable"), flush=True)
            del bp, e2c, e2r, meta
        del x, y
        TCGNN.clear_plan_cache()
        torch.cuda.empty_cache()
    print("misses: " + ("; ".join(misses) if misses else "none"))


if __name__ == "__main__":
    main()
