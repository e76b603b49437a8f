#!/usr/bin/env python3
"""Edge softmax, the two-operand SDDMM and the softmax-AGNN layer: one JSON line per measurement.
Graphs: sbm_reddit, R-MAT at the Reddit shape, and an SBM graph at the ogbn-products shape.  Times are HIP-event medians of 30 calls
after 5 warm-up calls (epochs: tcgnn_harness.time_training):
  edge_softmax   forward and backward (with d_beta) against the torch composition on the same box - row ids from repeat_interleave,
                 scatter_reduce amax, exp, index_add_ and a divide - and against the roofline B / 8 TB/s,
                 B = 4 (N + 1) + 8 E forward, 4 (N + 1) + 16 E backward with d_beta
  sddmm2         forward_ef2(X, Z) against forward_ef(X), the same kernel, at D = 64 and 128
  epoch          the AGNN epoch, hidden 64, 2 layers, attention = softmax against reference
    python tools/bench_attention.py [--epochs K] [--skip-epochs] [--graphs a,b]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tc-gnn_atc23_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import TCGNN  # noqa: E402
import tcgnn_graph as G  # noqa: E402
import tcgnn_harness as H  # noqa: E402

PEAK_BYTES_PER_MS = 8e12 / 1e3


def emit(**kw):
    print(json.dumps(kw), flush=True)


def translate(rp, col, n, dev):
    E = col.numel()
    bp = torch.zeros((n + 15) // 16, dtype=torch.int32, device=dev); e2c = torch.zeros(E, dtype=torch.int32, device=dev); e2r = torch.zeros(E, dtype=torch.int32, device=dev)
    TCGNN.preprocess_gpu(col, rp, n, 16, 8, bp, e2c, e2r)
    return (rp, col, bp, e2c, e2r)


def median_ms(fn, reps=30, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2]


def torch_softmax(s, rows, n, beta):
    x = beta * s
    m = torch.full((n,), -float("inf"), device=s.device).scatter_reduce(0, rows, x, "amax")
    ex = torch.exp(x - m[rows])
    return ex / torch.zeros(n, device=s.device).index_add_(0, rows, ex)[rows]


def torch_softmax_backward(p, dp, s, rows, n, beta):
    g = p * (dp - torch.zeros(n, device=p.device).index_add_(0, rows, p * dp)[rows])
    return beta * g, (s * g).sum()


def softmax_times(graph, n, rp, E, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    s, dp = torch.randn(E, device=dev, generator=g), torch.randn(E, device=dev, generator=g)
    beta = torch.tensor([0.9], device=dev)
    p, ds = torch.empty_like(s), torch.empty_like(s)
    TCGNN.edge_softmax(s, rp, beta, out=p)
    t_f = median_ms(lambda: TCGNN.edge_softmax(s, rp, beta, out=p))
    t_b = median_ms(lambda: TCGNN.edge_softmax_backward(p, dp, rp, beta=beta, score=s, need_dbeta=True, out=ds))
    t_b0 = median_ms(lambda: TCGNN.edge_softmax_backward(p, dp, rp, beta=beta, out=ds))
    # the composition: the row ids are built once outside the timed region (4 E bytes more that it has to keep), as a layer would
    lens = (rp[1:] - rp[:-1]).long()
    rows = torch.repeat_interleave(torch.arange(n, device=dev), lens)
    t_rows = median_ms(lambda: torch.repeat_interleave(torch.arange(n, device=dev), lens), reps=5, warmup=1)
    t_cf = median_ms(lambda: torch_softmax(s, rows, n, beta), reps=10, warmup=2)
    t_cb = median_ms(lambda: torch_softmax_backward(p, dp, s, rows, n, beta), reps=10, warmup=2)
    err = float((torch_softmax(s, rows, n, beta) - p).abs().max())
    bf, bb, bb0 = 4 * (n + 1) + 8 * E, 4 * (n + 1) + 16 * E, 4 * (n + 1) + 12 * E
    emit(graph=graph, what="edge_softmax", forward_ms=t_f, backward_dbeta_ms=t_b, backward_ms=t_b0, torch_forward_ms=t_cf, torch_backward_ms=t_cb,
         torch_row_ids_ms=t_rows, row_id_bytes=rows.numel() * rows.element_size(), roofline_forward_ms=bf / PEAK_BYTES_PER_MS,
         roofline_backward_dbeta_ms=bb / PEAK_BYTES_PER_MS, forward_GBps=bf / t_f / 1e6, backward_dbeta_GBps=bb / t_b / 1e6, backward_GBps=bb0 / t_b0 / 1e6,
         longest_row=int(lens.max()), max_abs_difference_from_torch=err)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--skip-epochs", action="store_true")
    ap.add_argument("--graphs", type=str, default="sbm_reddit,rmat_reddit,sbm_products")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    table = {"sbm_reddit": ("reddit", "sbm_reddit"), "rmat_reddit": ("reddit", "rmat"), "sbm_products": ("ogbn-products", "sbm")}
    for graph in args.graphs.split(","):
        shape, gen = table[graph]
        n, nnz, in_dim, classes = G.SHAPES[shape]
        rp, col = G.GENERATORS[gen](n, nnz, seed=0, device=dev)
        E = col.numel()
        emit(graph=graph, what="graph", num_nodes=n, num_edges=E)
        with torch.no_grad():
            softmax_times(graph, n, rp, E, dev)
            torch.cuda.empty_cache()
            meta = translate(rp, col, n, dev)
            for D in (64, 128):
                TCGNN.prepare([D], *meta, attention=True)
                g = torch.Generator(device=dev).manual_seed(D)
                X, Z = torch.randn(n, D, device=dev, generator=g), torch.randn(n, D, device=dev, generator=g)
                t = {"forward_ef_ms": [], "forward_ef2_ms": []}
                for _ in range(3):   # (in turn, the best median of each: the first timed call after a pause runs on cold clocks)
                    t["forward_ef_ms"].append(median_ms(lambda: TCGNN.forward_ef(X, *meta)))
                    t["forward_ef2_ms"].append(median_ms(lambda: TCGNN.forward_ef2(X, Z, *meta)))
                emit(graph=graph, what="sddmm2", D=D, walk=TCGNN.last_kernel(*meta), **{k: min(v) for k, v in t.items()})
                del X, Z
        if not args.skip_epochs:
            x = torch.randn(n, in_dim, device=dev)
            y = torch.randint(0, classes, (n,), device=dev)
            for attention in ("reference", "softmax"):
                r = H.time_training("agnn", meta, x, y, in_dim, 64, classes, 2, args.epochs, attention=attention)
                emit(graph=graph, what="epoch", attention=attention, train_ms=r["train_ms"], final_loss=r["final_loss"])
            del x, y
        TCGNN.clear_plan_cache()
        del meta, rp, col
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
