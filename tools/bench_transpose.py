#!/usr/bin/env python3
"""The transposed aggregation (tcgnn_transpose_ws, transpose=True, the layers' directed=True): one JSON line per measurement.
Graphs: the Reddit shape directed (SBM with communities and R-MAT) and the symmetric sbm_reddit graph.  Times are HIP-event
medians (build steps: median of 3; calls: of 30 after 5 warm-up calls; whole calls):
  transpose_kernels   tcgnn_transpose_ws alone, on preallocated outputs and scratch (its one read-back included)
  device_sgt          tcgnn_preprocess_gpu_ws on the same graph (the target the transpose is held against)
  transposed_build    transpose + device SGT of A^T + tcgnn_plan_create (what the first transpose=True call of a graph pays)
  spmm D              forward(X, transpose=True) / forward(X, meta_T) / forward(X)
  permute             tcgnn_permute_edge_values, and forward_AGNN(transpose=True) against forward_AGNN on A
  epoch               GCN epoch, hidden 64, norm='both', 2 layers, directed=True / False on the directed graph, eager and replayed
  memory              plan_bytes of A^T's plan and the arrays the transposed entry owns
    python tools/bench_transpose.py [--epochs K] [--skip-epochs]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tc-gnn_atc23_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import TCGNN  # noqa: E402
import tcgnn_capi as C  # noqa: E402
import tcgnn_graph as G  # noqa: E402
import tcgnn_harness as H  # noqa: E402


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


def build_times(graph, n, rp, col, dev):
    E = col.numel()
    stream = torch.cuda.current_stream(dev).cuda_stream
    rp_t = torch.empty(n + 1, dtype=torch.int32, device=dev); col_t = torch.empty(E, dtype=torch.int32, device=dev)
    perm = torch.empty(E, dtype=torch.int32, device=dev)
    need = C._sz(0)
    C.check(C.lib.tcgnn_transpose_workspace_bytes(n, E, C.ctypes.byref(need)), "tcgnn_transpose_workspace_bytes")
    ws = torch.empty(need.value + 256, dtype=torch.uint8, device=dev)
    ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
    sym = C._i32(0)
    fn = lambda: C.check(C.lib.tcgnn_transpose_ws(rp.data_ptr(), col.data_ptr(), n, E, rp_t.data_ptr(), col_t.data_ptr(), perm.data_ptr(),  # noqa: E731
                                                  ptr, need.value, C.ctypes.byref(sym), stream), "tcgnn_transpose_ws")
    emit(graph=graph, what="transpose_kernels", ms=median_ms(fn, reps=3, warmup=1), workspace_bytes=need.value, symmetric=bool(sym.value))
    del ws
    bp = torch.zeros((n + 15) // 16, dtype=torch.int32, device=dev); e2c = torch.empty(E, dtype=torch.int32, device=dev); e2r = torch.empty(E, dtype=torch.int32, device=dev)
    C.check(C.lib.tcgnn_preprocess_gpu_workspace_bytes(n, E, 16, C.ctypes.byref(need)), "sgt bytes")
    ws = torch.empty(need.value + 256, dtype=torch.uint8, device=dev)
    ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
    tc = C._i64(0)
    fn = lambda: C.check(C.lib.tcgnn_preprocess_gpu_ws(col.data_ptr(), rp.data_ptr(), n, E, 16, 8, bp.data_ptr(), bp.numel(), e2c.data_ptr(),  # noqa: E731
                                                       e2r.data_ptr(), ptr, need.value, C.ctypes.byref(tc), stream), "sgt")
    emit(graph=graph, what="device_sgt", ms=median_ms(fn, reps=3, warmup=1))
    del ws


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--skip-epochs", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, nnz, in_dim, classes = G.SHAPES["reddit"]
    for graph, gen, directed in (("sbm_reddit_directed", "sbm_reddit", True), ("rmat_directed", "rmat", True), ("sbm_reddit", "sbm_reddit", False)):
        rp, col = G.GENERATORS[gen](n, nnz, seed=0, device=dev, directed=directed)
        E = col.numel()
        emit(graph=graph, what="graph", num_nodes=n, num_edges=E)
        build_times(graph, n, rp, col, dev)
        meta = translate(rp, col, n, dev)
        times = []
        for _ in range(3):
            TCGNN.clear_plan_cache()
            TCGNN.plan_info(*meta)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); TCGNN.plan_info(*meta, transpose=True); b.record(); b.synchronize()
            times.append(a.elapsed_time(b))
        info = TCGNN.plan_info(*meta, transpose=True)
        emit(graph=graph, what="transposed_build", ms=sorted(times)[1], plan_bytes=info["plan_bytes"] if not info["shares_plan"] else 0,
             transpose_bytes=info["transpose_bytes"], symmetric=info["symmetric"])
        rp_t, col_t, perm, sym = TCGNN.transpose_graph(rp, col)
        meta_t = meta if sym else translate(rp_t.clone(), col_t.clone(), n, dev)
        with torch.no_grad():
            for D in (64, 128):
                TCGNN.prepare([D], *meta, transpose=True, edge_valued=D == 64)
                TCGNN.prepare([D], *meta_t)
                X = torch.randn(n, D, device=dev, generator=torch.Generator(device=dev).manual_seed(D))
                # (three rounds in turn, the best median of each: the first timed call of a width after a pause runs on cold clocks)
                t = {"transpose_ms": [], "host_built_transpose_ms": [], "forward_ms": []}
                for _ in range(3):
                    t["forward_ms"].append(median_ms(lambda: TCGNN.forward(X, *meta)))
                    t["transpose_ms"].append(median_ms(lambda: TCGNN.forward(X, *meta, transpose=True)))
                    t["host_built_transpose_ms"].append(median_ms(lambda: TCGNN.forward(X, *meta_t)))
                emit(graph=graph, what="spmm", D=D, walk=TCGNN.last_kernel(*meta, transpose=True), **{k: min(v) for k, v in t.items()})
            X = torch.randn(n, 64, device=dev)
            att = torch.randn(1, E, device=dev)
            out = torch.empty(E, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            t_p = median_ms(lambda: C.lib.tcgnn_permute_edge_values(att.data_ptr(), perm.data_ptr(), E, out.data_ptr(), stream))
            t_vt = median_ms(lambda: TCGNN.forward_AGNN(X, meta[0], meta[1], att, *meta[2:], transpose=True))
            t_v = median_ms(lambda: TCGNN.forward_AGNN(X, meta[0], meta[1], att, *meta[2:]))
            emit(graph=graph, what="edge_valued", D=64, permute_ms=t_p, permute_GBps=E * 12 / t_p / 1e6, transpose_ms=t_vt, forward_AGNN_ms=t_v)
        if directed and gen == "sbm_reddit" and not args.skip_epochs:
            x = torch.randn(n, in_dim, device=dev)
            y = torch.randint(0, classes, (n,), device=dev)
            for d in (True, False):
                for hg in (False, True):
                    r = H.time_training("gcn", meta, x, y, in_dim, 64, classes, 2, args.epochs, hip_graph=hg, norm="both", bias=True, directed=d)
                    emit(graph=graph, what="epoch", directed=d, hip_graph=hg, train_ms=r["train_ms"], final_loss=r["final_loss"])
        TCGNN.clear_plan_cache()
        del meta, meta_t, rp, col, rp_t, col_t, perm
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
