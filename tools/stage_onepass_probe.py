#!/usr/bin/env python3
"""The one-pass staging (tcgnn_stage.inc: stage_fused_kernel + stage_settle_kernel) where the benchmark does not look.
On the Reddit shape (`sbm_reddit`), median of HIP-event times over whole calls of TCGNN.forward:

  hit path / miss path   the same X every call (the guess of the scale always holds) against X and 8 X in turn (it never does),
                         each with the one-pass staging and with tcgnn_set_stage_onepass(0), at D = 64 and D = 16; the plan's
                         hit / miss counters beside them

and, with --train, the harness's GCN and AGNN training (hidden 64): per model, eager and captured in a HIP graph, the hit and miss
counts of epochs 31 - 60 after the dry epochs (two trainings from the same seed, 30 and 60 timed epochs: their difference), and the
epoch time with the one-pass staging on and off.
    python tools/stage_onepass_probe.py [--train] [--reps K]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tc-gnn_atc23_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import TCGNN  # noqa: E402
import tcgnn_graph as G  # noqa: E402
import tcgnn_harness as H  # noqa: E402


def graph(shape, gen, dev):
    n, nnz, in_dim, classes = G.SHAPES[shape]
    rp, col = G.GENERATORS[gen](n, nnz, seed=0, device=dev)
    E = col.numel()
    nw = (n + 15) // 16
    bp = torch.zeros(nw, dtype=torch.int32, device=dev); e2c = torch.zeros(E, dtype=torch.int32, device=dev); e2r = torch.zeros(E, dtype=torch.int32, device=dev)
    TCGNN.preprocess_gpu(col, rp, n, 16, 8, bp, e2c, e2r)
    return n, in_dim, classes, (rp, col, bp, e2c, e2r)


def median_ms(fns, reps, warmup=6):
    """fns: called in turn, one timed call per event pair"""
    for k in range(warmup):
        fns[k % len(fns)]()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for k, (a, b) in enumerate(ev):
        a.record(); fns[k % len(fns)](); b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2]


def calls(meta, n, dev, reps):
    with torch.no_grad():
        for D in (64, 16):
            g = torch.Generator(device=dev).manual_seed(0)
            X = torch.randn(n, D, device=dev, generator=g)
            X8 = 8 * X
            TCGNN.prepare([D], *meta)
            same, turn = [lambda: TCGNN.forward(X, *meta)], [lambda: TCGNN.forward(X, *meta), lambda: TCGNN.forward(X8, *meta)]
            row = {}
            for on in (1, 0, 1, 0):      # each setting twice, alternating: a drift of the box shows as a difference between the two
                TCGNN.set_stage_onepass(on)
                for what, fns in (("same X", same), ("X, 8 X in turn", turn)):
                    h0, m0 = TCGNN.stage_stats(*meta)
                    ms = median_ms(fns, reps)
                    h1, m1 = TCGNN.stage_stats(*meta)
                    row.setdefault((on, what), []).append((ms, h1 - h0, m1 - m0))
            TCGNN.set_stage_onepass(1)
            print("D=%-3d %s" % (D, TCGNN.last_kernel(*meta)))
            for (on, what), v in row.items():
                print("   one-pass %d  %-16s  call %s ms   hits %s  misses %s" % (on, what, " ".join("%.4f" % r[0] for r in v), [r[1] for r in v], [r[2] for r in v]))


def training(meta, n, in_dim, classes, dev, epochs):
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(n, in_dim, device=dev, generator=gen)
    y = torch.randint(0, classes, (n,), device=dev, generator=gen)
    for model in ("gcn", "agnn"):
        for hip_graph in (False, True):
            out = {}
            for on in (1, 0):
                TCGNN.set_stage_onepass(on)
                for ep in (epochs, 2 * epochs):
                    h0, m0 = TCGNN.stage_stats(*meta)
                    r = H.time_training(model, meta, x, y, in_dim, 64, classes, 2, ep, seed=0, warmup=9, hip_graph=hip_graph)
                    h1, m1 = TCGNN.stage_stats(*meta)
                    out[(on, ep)] = (r["train_ms"], h1 - h0, m1 - m0, r["final_loss"])
            TCGNN.set_stage_onepass(1)
            a, b = out[(1, epochs)], out[(1, 2 * epochs)]
            hits, misses = b[1] - a[1], b[2] - a[2]
            print("%-5s %-9s hidden 64: epochs %d - %d staged one-pass calls: %d hits, %d misses (%.0f %% hit); all epochs of the longer run, dry ones included: %d hits, %d misses" %
                  (model, "hip_graph" if hip_graph else "eager", epochs + 1, 2 * epochs, hits, misses, 100.0 * hits / max(hits + misses, 1), b[1], b[2]))
            print("      epoch ms (%d / %d timed epochs): one-pass %.3f / %.3f   two-pass %.3f / %.3f   final loss %.6g / %.6g (two-pass counters moved by %d)" %
                  (epochs, 2 * epochs, a[0], b[0], out[(0, epochs)][0], out[(0, 2 * epochs)][0], b[3], out[(0, 2 * epochs)][3], out[(0, 2 * epochs)][1] + out[(0, 2 * epochs)][2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--epochs", type=int, default=30)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, in_dim, classes, meta = graph("reddit", "sbm_reddit", dev)
    calls(meta, n, dev, args.reps)
    if args.train:
        training(meta, n, in_dim, classes, dev, args.epochs)


if __name__ == "__main__":
    main()
