"""The REAL multi-GPU path (HipShardOps: HIP kernels + both exchanges) with world_size 2 on the one GPU of the test box, and
the 64-bit addressing of a papers100M-sized shard (BASELINE.json configs[4]).  Needs an MI355X: `pytest -m gpu`.

RCCL refuses two ranks on one device, so the two processes rendezvous over gloo (127.0.0.1) and the gathers are host-staged
(tcgnn_shard.all_gather_rows); everything else - local SGT, tcgnn_plan_create_sharded with num_cols > num_rows and a
row offset, the three kernels on the shard, the fp16-on-the-wire exchange (one-word all-reduce of the absmax bit pattern +
all-gather of the image slices into a strided view), autograd through the exchange and one whole sharded GCN step - is the
code an 8-GPU run executes.  Each rank checks its results against the UNSHARDED HIP kernels on the whole graph and the oracle.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import graphs
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TIGHT = 4e-6


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, out_dir):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tc-gnn_atc23_amd"), os.path.join(root, "tests")):
        sys.path.insert(0, p)
    import TCGNN
    import tcgnn_capi as c
    import tcgnn_shard as S
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ok, notes, planar_seen = {}, [], []
    try:
        for gname, (rp, col) in (("powerlaw_n6000", graphs.powerlaw_graph(6000, 60, seed=5)), ("uniform_n20000", graphs.uniform_graph(20000, 48, seed=6))):
            n = len(rp) - 1
            bp, e2c, e2r, _ = graphs.host_sgt(rp, col)
            meta = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (rp, col, bp, e2c, e2r)]
            shard = S.RowShard(rp, col, device=dev)                      # HipShardOps: the product path
            assert isinstance(shard.ops, S.HipShardOps) and shard.world == 2
            b0, b1 = shard.layout.bounds[rank], shard.layout.bounds[rank + 1]
            e0, e1 = int(rp[b0]), int(rp[b1])
            for D in (64, 41):
                rng = np.random.default_rng(100 + D)
                X = (rng.standard_normal((n, D)) * 3.0).astype(np.float32)
                att = rng.standard_normal(len(col)).astype(np.float32)
                tX = torch.from_numpy(X).to(dev)
                x_local = tX[b0:b1].contiguous()
                Yfull = TCGNN.forward(tX, *meta)[0]
                Y64, absY = O.spmm_f64(X, rp, col)
                scale = torch.from_numpy(absY[b0:b1]).to(dev) + 1.0
                tag = "%s D=%d " % (gname, D)
                Yl = shard.spmm(x_local)                                 # fp32 all-gather + local SpMM
                ok[tag + "spmm vs unsharded HIP"] = bool(((Yl - Yfull[b0:b1]).abs() / scale).max().item() <= TIGHT)
                ok[tag + "spmm vs fp64"] = bool(((Yl.double().cpu() - torch.from_numpy(Y64[b0:b1])).abs() / scale.cpu()).max().item() <= 2.0 ** -9)
                try:                                                     # fp16 on the wire: bit-identical on the same walk
                    for mode in (1, 2):
                        c.check(c.lib.tcgnn_set_spmm_mode(mode), "tcgnn_set_spmm_mode")
                        a = shard.spmm(x_local)
                        b = shard.spmm(x_local, wire="fp16")
                        ok[tag + "fp16 wire == fp32 wire (mode %d)" % mode] = bool(torch.equal(a, b))
                        # r05: the exchange in column chunks (ring of two buffers, side stream) equals the whole-matrix one on the same walk
                        for ch, wr in ((16, "fp32"), (32, "fp32"), (64, "auto"), (32, "fp16")):
                            ok[tag + "chunked exchange %d cols / %s (mode %d)" % (ch, wr, mode)] = bool(torch.equal(a, shard.spmm_chunked(x_local, chunk=ch, wire=wr)))
                    # r06: with the LDS-resident kernel forced the fp16 exchange stages the image PLANAR - one
                    # all-gather per 16-column plane - and the shard keeps the fast kernel: bit for bit the fp32-gather call on that kernel
                    c.check(c.lib.tcgnn_set_spmm_mode(3), "tcgnn_set_spmm_mode")
                    planar = bool(c.lib.tcgnn_spmm_staged_layout(shard.ops.plan, D, torch.cuda.current_stream(dev).cuda_stream))
                    a = shard.spmm(x_local)
                    ka = c.lib.tcgnn_plan_last_kernel(shard.ops.plan).decode()
                    b = shard.spmm(x_local, wire="fp16")
                    kb = c.lib.tcgnn_plan_last_kernel(shard.ops.plan).decode()
                    notes.append(tag + "mode 3: planar %s, kernels %s / %s" % (planar, ka, kb))
                    if planar:
                        ok[tag + "planar fp16 wire == fp32 wire on the LDS-resident kernel"] = bool(torch.equal(a, b)) and ka.startswith("spmm_lds") and kb.startswith("spmm_lds")
                        ok[tag + "planar chunked exchange"] = bool(torch.equal(a[:, :min(D, 64)].contiguous(), shard.spmm_chunked(x_local[:, :min(D, 64)].contiguous(), chunk=64, wire="fp16"))) if D >= 64 else True
                    else:
                        ok[tag + "row-major fallback of the staged call (mode 3)"] = bool(((a - b).abs() / scale).max().item() <= TIGHT)
                    planar_seen.append(planar)
                finally:
                    c.lib.tcgnn_set_spmm_mode(0)
                Yo = shard.spmm_overlapped(x_local)                      # gather on a side stream under the own-block product
                ok[tag + "overlapped exchange"] = bool(((Yo - Yl).abs() / scale).max().item() <= TIGHT)
                Yv = shard.spmm_val(x_local, torch.from_numpy(att[e0:e1]).to(dev))
                Yvfull = TCGNN.forward_AGNN(tX, meta[0], meta[1], torch.from_numpy(att).to(dev).view(1, -1), *meta[2:])[0]
                _, absYv = O.spmm_f64(X, rp, col, att)
                ok[tag + "spmm_val"] = bool(((Yv - Yvfull[b0:b1]).abs() / (torch.from_numpy(absYv[b0:b1]).to(dev) + 1.0)).max().item() <= TIGHT)
                ef = shard.sddmm(x_local)
                effull = TCGNN.forward_ef(tX, *meta)[0]
                _, absef = O.sddmm_f64(X, rp, col)
                ok[tag + "sddmm"] = bool(ef.numel() == e1 - e0 and ((ef - effull[e0:e1]).abs() / (torch.from_numpy(absef[e0:e1]).to(dev) + 1.0)).max().item() <= TIGHT)
            # autograd through the exchange (A, not A^T: the reference's convention) against the unsharded kernels
            D = 32
            rng = np.random.default_rng(7)
            X = rng.standard_normal((n, D)).astype(np.float32); G = rng.standard_normal((n, D)).astype(np.float32)
            xl = torch.from_numpy(X[b0:b1]).to(dev).requires_grad_(True)
            (shard.aggregate(xl) * torch.from_numpy(G[b0:b1]).to(dev)).sum().backward()
            ref = TCGNN.forward(torch.from_numpy(G).to(dev), *meta)[0][b0:b1]
            ok[gname + " backward through the exchange"] = bool(((xl.grad - ref).abs() / (ref.abs() + 10.0)).max().item() <= 1e-5)
            shard.ops.close()

        ok["the planar staged image was exercised"] = any(planar_seen)
        # one whole sharded GCN training step on the HIP kernels vs the same step on the undivided graph (dense A, autograd)
        rp, col = graphs.powerlaw_graph(500, 12, seed=9)
        n, in_dim, hidden, classes = 500, 20, 16, 5
        rng = np.random.default_rng(1)
        X = (rng.standard_normal((n, in_dim)) * 0.1).astype(np.float32)
        y = rng.integers(0, classes, size=n)
        shard = S.RowShard(rp, col, device=dev)
        b0, b1 = shard.layout.bounds[rank], shard.layout.bounds[rank + 1]
        model = S.ShardedGCN(in_dim, hidden, classes, num_layers=2, dropout=0.0, seed=3).to(dev)
        model.weights[0].data.mul_(0.1); model.weights[1].data.mul_(0.1)
        w0 = [w.detach().clone() for w in model.weights]
        opt = torch.optim.SGD(model.parameters(), lr=0.5)
        loss = S.sharded_train_step(model, shard, torch.from_numpy(X[b0:b1]).to(dev), torch.from_numpy(y[b0:b1]).to(dev), opt, n)
        A = np.zeros((n, n), np.float32)
        for r in range(n):
            A[r, col[rp[r]:rp[r + 1]]] = 1.0
        At = torch.from_numpy(A).to(dev)
        W = [w.clone().requires_grad_(True) for w in w0]
        h = torch.relu(At @ (torch.from_numpy(X).to(dev) @ W[0]))
        logp = torch.log_softmax(At @ (h @ W[1]), dim=1)
        ref_loss = -logp.gather(1, torch.from_numpy(y).to(dev).view(-1, 1)).mean()
        ref_loss.backward()
        ok["gcn step loss"] = abs(float(loss) - float(ref_loss)) < 2e-3 * max(1.0, abs(float(ref_loss)))   # 10-bit operands in the kernels
        for k in range(2):
            ok["gcn step w%d" % k] = bool(torch.allclose(model.weights[k].detach(), w0[k] - 0.5 * W[k].grad, rtol=2e-2, atol=2e-4))
        notes.append("loss %.6f ref %.6f" % (float(loss), float(ref_loss)))
        shard.ops.close()
    except Exception as exc:   # report, do not hang the other rank in a collective
        import traceback
        ok["exception"] = False
        notes.append(traceback.format_exc())
        raise
    finally:
        with open(os.path.join(out_dir, "rank%d.txt" % rank), "w") as f:
            f.write(repr(ok) + "\n" + "\n".join(notes))
        np.save(os.path.join(out_dir, "rank%d.npy" % rank), np.array([int(v) for v in ok.values()] or [0]))
        dist.destroy_process_group()


def test_two_ranks_on_the_real_hip_shard_path(tmp_path):
    assert torch.cuda.is_available()
    port = _free_port()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        flags = np.load(os.path.join(tmp_path, "rank%d.npy" % r))
        assert flags.size > 20 and flags.all(), open(os.path.join(tmp_path, "rank%d.txt" % r)).read()


def test_shard_whose_feature_matrix_needs_64_bit_addresses():
    """One rank's shard of a papers100M-sized run: A is 4096 x 34 000 000 and X is [34 000 000, 128] - num_cols * D = 4.35e9
    elements, beyond 32-bit element AND byte offsets (the reference's `unsigned` address math overflows there,
    TCGNN_kernel.cu:420).  Edges point below and above every 2^32 boundary; SpMM, edge-valued SpMM and SDDMM (A's rows sit at
    row_offset inside X) are checked against float64 gathers on the device."""
    import tcgnn_capi as c
    import tcgnn_shard as S
    dev = torch.device("cuda:0")
    rows, num_cols, D, deg = 4096, 34_000_000, 128, 48
    H = num_cols // 2                                   # world of 2 blocks of 17 M rows; this is rank 1's shard
    layout = S.ShardLayout([0, H, 2 * H])
    assert layout.num_cols == num_cols and num_cols * D > 2 ** 32
    rng = np.random.default_rng(0)
    # neighbours: around every overflow boundary of the element offset (2^32 / D rows) and the byte offset (2^32 / (4 D), / (2 D)), plus uniform
    special = np.array([2 ** 32 // D, 2 ** 32 // (4 * D), 2 ** 32 // (2 * D), 2 ** 31 // D, num_cols - 1, 0], dtype=np.int64)
    lrp = np.zeros(rows + 1, np.int32); cols = []
    for r in range(rows):
        cset = set(rng.integers(0, num_cols, size=deg - 8).tolist())
        cset.update((special[rng.integers(0, len(special), size=8)] + rng.integers(-2, 3, size=8)).clip(0, num_cols - 1).tolist())
        cc = np.array(sorted(cset), dtype=np.int64)
        cols.append(cc); lrp[r + 1] = lrp[r] + len(cc)
    lcol = np.concatenate(cols).astype(np.int32)
    ops = S.HipShardOps(lrp, lcol, layout, 1, dev)      # rank 1: row_off = H
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(num_cols, D, device=dev, generator=g)               # 17.4 GB
    tcol = torch.from_numpy(lcol).to(dev).long()
    erow = torch.repeat_interleave(torch.arange(rows, device=dev), torch.from_numpy(np.diff(lrp)).to(dev).long())
    Xn = X[tcol].double()                                               # [E, D] neighbour rows
    ref = torch.zeros(rows, D, dtype=torch.float64, device=dev).index_add_(0, erow, Xn)
    scale = torch.zeros(rows, D, dtype=torch.float64, device=dev).index_add_(0, erow, Xn.abs()) + 1.0
    att = torch.randn(tcol.numel(), device=dev, generator=g)
    refv = torch.zeros(rows, D, dtype=torch.float64, device=dev).index_add_(0, erow, Xn * att.double()[:, None])
    scalev = torch.zeros(rows, D, dtype=torch.float64, device=dev).index_add_(0, erow, (Xn * att.double()[:, None]).abs()) + 1.0
    Xr = X[H + erow].double()                                           # A's row r is X's row row_off + r
    refe = (Xr * Xn).sum(1); scalee = (Xr * Xn).abs().sum(1) + 1.0
    del Xr
    err = {}
    err["spmm (auto: single-launch fp32 kernel)"] = ((ops.spmm(X).double() - ref).abs() / scale).max().item()
    try:
        c.check(c.lib.tcgnn_set_spmm_mode(1), "tcgnn_set_spmm_mode")
        a = ops.spmm(X)                                                 # the fp16 gather walk over an 8.7 GB image
        err["spmm (per-window gather walk)"] = ((a.double() - ref).abs() / scale).max().item()
        err["spmm_val"] = ((ops.spmm_val(X, att).double() - refv).abs() / scalev).max().item() / 2
        err["sddmm"] = ((ops.sddmm(X).double() - refe).abs() / scalee).max().item() / 2
        # the pre-staged fp16 image (what crosses the fabric with wire="fp16"; a world of one process would only copy its own
        # block, so the image is built over all rows directly): same kernel, same bits
        pitch = c.lib.tcgnn_x16_pitch(D)
        image = torch.zeros(256 + (num_cols + 1) * pitch * 2 + 256, dtype=torch.uint8, device=dev)
        off = (-image.data_ptr()) % 256
        image = image[off: off + 256 + (num_cols + 1) * pitch * 2]
        word = image[:4].view(torch.int32)
        st = torch.cuda.current_stream(dev).cuda_stream
        c.check(c.lib.tcgnn_stage_absmax(X.data_ptr(), num_cols * D, word.data_ptr(), st), "absmax")
        c.check(c.lib.tcgnn_stage_rows(X.data_ptr(), num_cols, D, word.data_ptr(), image[256:].data_ptr(), st), "rows")
        b = torch.empty(rows, D, device=dev)
        c.check(c.lib.tcgnn_spmm_staged(ops.plan, image.data_ptr(), b.data_ptr(), D, st), "staged")
        err["staged image == workspace image"] = 0.0 if torch.equal(a, b) else 1.0
        del image
        # the fused AGNN pair gathers through the same descriptor
        w = torch.tensor([0.5], device=dev)
        ws, nb = ops._workspace(D)
        ef = torch.empty(tcol.numel(), device=dev); efm = torch.zeros(1 + rows, dtype=torch.int32, device=dev); Yf = torch.empty(rows, D, device=dev)   # (max |ef| + one scale exponent per row: include/tcgnn.h)
        if c.lib.tcgnn_agnn_supported(ops.plan, D):
            # (a buffer sized for r04's one word is refused, not overrun)
            assert c.lib.tcgnn_agnn_pair_forward(ops.plan, X.data_ptr(), w.data_ptr(), ef.data_ptr(), efm.data_ptr(), 1, Yf.data_ptr(), D, ws, nb, st) == 1   # TCGNN_ERR_INVALID_ARG
            c.check(c.lib.tcgnn_agnn_pair_forward(ops.plan, X.data_ptr(), w.data_ptr(), ef.data_ptr(), efm.data_ptr(), efm.numel(), Yf.data_ptr(), D, ws, nb, st), "agnn_pair_forward")
            err["fused agnn ef"] = ((ef.double() - refe).abs() / scalee).max().item() / 2
    finally:
        c.lib.tcgnn_set_spmm_mode(0)
    bad = {k: v for k, v in err.items() if not v <= 2.0 ** -9}
    assert not bad, (bad, err)
    ops.close()


@pytest.mark.parametrize("D", [64, 128])
def test_row_shard_on_the_xcd_sliced_and_xcd_affine_walks(D, monkeypatch):
    """r03: a rank's rectangular shard (A is rows x num_cols, its rows sit at row_offset inside X) on the walks that slice the COLUMNS
    by XCD - the edge-valued SpMM on the fused kernel's sliced walk (score half off) and the range-major SDDMM with XCD affinity -
    forced here, against float64 gathers and against the same shard on the per-window walks."""
    import tcgnn_capi as c
    import tcgnn_shard as S
    dev = torch.device("cuda:0")
    rows, H, deg = 40_003, 40_003, 40
    layout = S.ShardLayout([0, H, 2 * H])
    num_cols = layout.num_cols
    rng = np.random.default_rng(5)
    cols = np.sort(rng.integers(0, num_cols, size=(rows, deg)), axis=1)
    keep = np.ones_like(cols, dtype=bool); keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
    lrp = np.zeros(rows + 1, np.int32); lrp[1:] = np.cumsum(keep.sum(1))
    lcol = cols[keep].astype(np.int32)
    ops = S.HipShardOps(lrp, lcol, layout, 1, dev)      # rank 1: row_off = H
    g = torch.Generator(device=dev).manual_seed(D)
    X = torch.randn(num_cols, D, device=dev, generator=g)
    att = torch.randn(lcol.size, device=dev, generator=g)
    tcol = torch.from_numpy(lcol).to(dev).long()
    erow = torch.repeat_interleave(torch.arange(rows, device=dev), torch.from_numpy(np.diff(lrp)).to(dev).long())
    Xn = X[tcol].double()
    refv = torch.zeros(rows, D, dtype=torch.float64, device=dev).index_add_(0, erow, att.double()[:, None] * Xn)
    scalev = torch.zeros(rows, D, dtype=torch.float64, device=dev).index_add_(0, erow, (att.double()[:, None] * Xn).abs()) + 1.0
    Xr = X[ops.row_off + erow].double()                                 # (blocks are padded to a common height: row_off = rank * layout.H)
    refe = (Xr * Xn).sum(1); scalee = (Xr * Xn).abs().sum(1) + 1.0
    name = lambda: c.lib.tcgnn_plan_last_kernel(ops.plan).decode()
    try:
        monkeypatch.setenv("TCGNN_AGNN_SLICED", "0"); monkeypatch.setenv("TCGNN_SDDMM_XCD", "0")
        yv0, ef0 = ops.spmm_val(X, att), ops.sddmm(X)
        monkeypatch.setenv("TCGNN_AGNN_SLICED", "2")
        yv1 = ops.spmm_val(X, att); kv = name()
        c.check(c.lib.tcgnn_set_spmm_mode(2), "tcgnn_set_spmm_mode")
        monkeypatch.setenv("TCGNN_SDDMM_XCD", "2"); monkeypatch.setenv("TCGNN_RANGE_KB", "256")
        ef1 = ops.sddmm(X)
    finally:
        c.lib.tcgnn_set_spmm_mode(0)
    assert "values only" in kv, kv
    for y in (yv0, yv1):
        assert ((y.double() - refv).abs() / scalev).max().item() <= 2.0 ** -9
    assert ((yv1 - yv0).abs().double() / scalev).max().item() <= 1e-5
    assert ((ef0.double() - refe).abs() / scalee).max().item() <= 2.0 ** -9
    assert torch.equal(ef0, ef1)
    ops.close()


@pytest.mark.parametrize("D", [64, 128])
def test_row_shard_on_the_slice_synchronised_walk(D, monkeypatch, capfd):
    """r06: a rank's rectangular shard of a graph with communities (rows H .. 2H of 2H nodes, 16 communities, 90 % of the edges inside)
    on the slice-synchronised range walk - its tables are built for shards too (the columns are global, the SDDMM's window rows sit at
    row_offset inside X), so the automatic mode may take it there: forced (mode 5) against float64 gathers and the per-window walk;
    the scores bit for bit."""
    import tcgnn_capi as c
    import tcgnn_shard as S
    dev = torch.device("cuda:0")
    H = 40_000
    rp, col = graphs.community_graph(2 * H, 16, 50, 0.9, seed=13)
    layout = S.ShardLayout([0, H, 2 * H])
    lrp, lcol = S.local_csr(rp, col, layout, 1)
    rows = len(lrp) - 1
    monkeypatch.setenv("TCGNN_VERBOSE", "1")
    ops = S.HipShardOps(lrp, lcol, layout, 1, dev)      # rank 1: row_off = H
    assert "sync walk:" in capfd.readouterr().err
    g = torch.Generator(device=dev).manual_seed(D)
    X = torch.randn(layout.num_cols, D, device=dev, generator=g) / D ** 0.5
    att = torch.randn(lcol.size, device=dev, generator=g)
    tcol = torch.from_numpy(np.ascontiguousarray(lcol)).to(dev).long()
    erow = torch.repeat_interleave(torch.arange(rows, device=dev), torch.from_numpy(np.diff(lrp)).to(dev).long())
    Xn = X[tcol].double()
    ref = torch.zeros(rows, D, dtype=torch.float64, device=dev).index_add_(0, erow, Xn)
    scale = torch.zeros(rows, D, dtype=torch.float64, device=dev).index_add_(0, erow, Xn.abs()) + 1.0
    refv = torch.zeros(rows, D, dtype=torch.float64, device=dev).index_add_(0, erow, att.double()[:, None] * Xn)
    scalev = torch.zeros(rows, D, dtype=torch.float64, device=dev).index_add_(0, erow, (att.double()[:, None] * Xn).abs()) + 1.0
    Xr = X[ops.row_off + erow].double()
    refe = (Xr * Xn).sum(1); scalee = (Xr * Xn).abs().sum(1) + 1.0
    name = lambda: c.lib.tcgnn_plan_last_kernel(ops.plan).decode()
    out = {}
    try:
        for mode in (1, 5):
            c.check(c.lib.tcgnn_set_spmm_mode(mode), "tcgnn_set_spmm_mode")
            y = ops.spmm(X); k1 = name()
            yv = ops.spmm_val(X, att); k2 = name()
            ef = ops.sddmm(X); k3 = name()
            out[mode] = (y, yv, ef, (k1, k2, k3))
    finally:
        c.lib.tcgnn_set_spmm_mode(0)
    assert out[5][3] == ("spmm_sync_kernel", "spmm_sync_kernel", "sddmm_kernel (slice-synchronised)"), out[5][3]
    for mode in (1, 5):
        assert ((out[mode][0].double() - ref).abs() / scale).max().item() <= 2.0 ** -9
        assert ((out[mode][1].double() - refv).abs() / scalev).max().item() <= 2.0 ** -9
        assert ((out[mode][2].double() - refe).abs() / scalee).max().item() <= 2.0 ** -9
    assert ((out[5][0] - out[1][0]).abs().double() / scale).max().item() <= 1e-5
    assert torch.equal(out[5][2], out[1][2])
    ops.close()


def _rccl_worker(rank, world, port, out_dir):
    """World of ONE under backend "nccl" (= RCCL): every collective of the N-rank step executes - all_gather_into_tensor of the
    fp32 row blocks, the one-word int32 all_reduce(MAX), all_gather_into_tensor of the fp16 image slices into the strided view,
    the flat all_reduce of the weight gradients and of the loss - and must leave the results of the collective-free path."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tc-gnn_atc23_amd"), os.path.join(root, "tests")):
        sys.path.insert(0, p)
    import tcgnn_capi as c
    import tcgnn_shard as S
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    ok, notes = {}, []
    try:
        rp, col = graphs.uniform_graph(20000, 48, seed=6)
        n = len(rp) - 1
        plain = S.RowShard(rp, col, device=dev, always_collective=False)
        coll = S.RowShard(rp, col, device=dev, always_collective=True)
        assert dist.get_backend() == "nccl" and coll.world == 1
        for D in (64, 41, 16):
            X = torch.randn(n, D, device=dev, generator=torch.Generator(device=dev).manual_seed(D))
            for mode in (0, 1, 2):
                try:
                    c.check(c.lib.tcgnn_set_spmm_mode(mode), "tcgnn_set_spmm_mode")
                    a = plain.spmm(X)
                    ok["D=%d mode %d fp32 all-gather under RCCL" % (D, mode)] = bool(torch.equal(a, coll.spmm(X)))
                    if mode:   # (the staged image is row-major: gather walks)
                        ok["D=%d mode %d fp16 image all-gather + int32 all-reduce(MAX) under RCCL" % (D, mode)] = bool(torch.equal(plain.spmm(X, wire="fp16"), coll.spmm(X, wire="fp16")))
                finally:
                    c.lib.tcgnn_set_spmm_mode(0)
            ok["D=%d sddmm" % D] = bool(torch.equal(plain.sddmm(X), coll.sddmm(X)))
            a = plain.spmm(X)
            ok["D=%d overlapped exchange (side-stream all-gather under RCCL)" % D] = bool(((coll.spmm_overlapped(X) - a).abs().max() <= 1e-4 * (a.abs().max() + 1.0)).item())
            try:   # the chunked exchange's collectives on the side stream under RCCL (fp16 image slices from 64 columns up, fp32 below)
                c.check(c.lib.tcgnn_set_spmm_mode(1), "tcgnn_set_spmm_mode")
                a1 = plain.spmm(X)
                ok["D=%d chunked exchange under RCCL" % D] = bool(torch.equal(a1, coll.spmm_chunked(X, chunk=64)) and torch.equal(a1, coll.spmm_chunked(X, chunk=16, wire="fp32")))
            finally:
                c.lib.tcgnn_set_spmm_mode(0)
        # one whole training step with the gradient / loss all-reduces issued
        in_dim, hidden, classes = 20, 16, 5
        Xf = torch.randn(n, in_dim, device=dev) * 0.1
        y = torch.randint(0, classes, (n,), device=dev)
        losses = []
        for sh in (plain, coll):
            model = S.ShardedGCN(in_dim, hidden, classes, num_layers=2, dropout=0.0, seed=3).to(dev)
            opt = torch.optim.SGD(model.parameters(), lr=0.5)
            losses.append((float(S.sharded_train_step(model, sh, Xf, y, opt, n)), [w.detach().clone() for w in model.weights]))
        ok["training step: loss"] = losses[0][0] == losses[1][0]
        ok["training step: weights"] = all(torch.equal(a, b) for a, b in zip(losses[0][1], losses[1][1]))
        dist.barrier()
        plain.ops.close(); coll.ops.close()
    except Exception:
        import traceback
        ok["exception"] = False
        notes.append(traceback.format_exc())
        raise
    finally:
        with open(os.path.join(out_dir, "rccl_rank%d.txt" % rank), "w") as f:
            f.write(repr(ok) + "\n" + "\n".join(notes))
        np.save(os.path.join(out_dir, "rccl_rank%d.npy" % rank), np.array([int(v) for v in ok.values()] or [0]))
        dist.destroy_process_group()


def test_rccl_world_of_one_executes_every_collective_of_the_n_gpu_step(tmp_path):
    assert torch.cuda.is_available()
    mp.spawn(_rccl_worker, args=(1, _free_port(), str(tmp_path)), nprocs=1, join=True)
    flags = np.load(os.path.join(tmp_path, "rccl_rank0.npy"))
    assert flags.size >= 15 and flags.all(), open(os.path.join(tmp_path, "rccl_rank0.txt")).read()


def test_bench_gpus_n_starts_its_own_ranks_and_prints_one_json_line_last(tmp_path):
    """`python bench.py --gpus N --full` with no launcher (the form the driver uses at N = 1): the sharded path is forced with a
    world of one, so the self-launch (torch.distributed.run on 127.0.0.1), the RCCL process group, the exchange inside the
    timed step and the --full legs all execute; the last stdout line is the JSON line."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TCGNN_BENCH_FORCE_SHARDED="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--scale", "0.05", "--steps", "5", "--warmup", "2", "--epochs", "4", "--full",
                        "--dump-outputs", str(tmp_path / "out")], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines[-1]) < 4096, len(lines[-1])          # (the driver parses this line; r03's 20 KB object came back unparsed)
    line = json.loads(lines[-1])
    assert line["n_gpus"] == 1 and line["steps"] == 5 and line["value"] > 0 and line["scaling"] == "weak"
    assert line["roofline"]["frac"] > 0 and line["roofline"]["kernel_ms_mean"] > 0
    s = line["summary"]
    assert s["exchange_in_timed_step"] is True and s["gcn_ms_per_epoch_sharded"] is not None
    with open(os.path.join(root, line["detail"])) as f:   # everything else: bench_detail.json
        ex = json.load(f)["extra"]
    assert ex["exchange_in_timed_step"] is True
    assert ex["ms_per_step_with_exchange"] > 0 and ex["ms_per_step_with_fp16_exchange"] is not None
    assert ex["gcn_ms_per_epoch_sharded"] is not None
    assert ex["ms_per_step_with_overlapped_exchange"] is not None and 0.0 <= ex["exchange_fraction_if_overlapped"] < 1.0
    y = np.load(tmp_path / "out" / "spmm_out_rank0.npy")      # --dump-outputs: the rank's rows of the last timed step
    assert y.dtype == np.float32 and y.shape == (int(232965 * 0.05), 64) and np.isfinite(y).all() and np.abs(y).max() > 0


@pytest.mark.gpu
def test_bench_single_gpu_line_is_bounded_and_carries_roofline_and_cpu_baseline():
    """The N = 1 form the driver runs with --full (scaled down): last stdout line < 4 KB, parses, holds `roofline` and `cpu_baseline`."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "TCGNN_BENCH_FORCE_SHARDED"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--scale", "0.05", "--steps", "5", "--warmup", "2", "--epochs", "3", "--full"],
                       env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines[-1]) < 4096, len(lines[-1])
    line = json.loads(lines[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data"):
        assert k in line, k
    assert line["roofline"]["bound"] == "hbm" and line["roofline"]["frac"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["cores"] >= 1 and line["cpu_baseline"]["kind"] == "port"
    assert line["summary"]["gcn_ms_per_epoch"] > 0 and line["summary"]["agnn_ms_per_epoch"] > 0


@pytest.mark.gpu
def test_plain_bench_run_times_k_steps_and_dumps_what_the_last_step_returned(tmp_path):
    """`python bench.py --steps K --warmup W --dump-outputs DIR` (scaled down), no --full: the line holds the headline keys and
    K timed steps and none of the --full legs; DIR/spmm_out.npy is Y = A X of the seeded inputs (graph and X from --seed), so
    it equals the same product computed here from the same seeds."""
    import json
    import subprocess
    import sys
    import TCGNN
    import tcgnn_graph as G
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "TCGNN_BENCH_FORCE_SHARDED"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--scale", "0.05", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(tmp_path / "out")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.strip()][-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "roofline"):
        assert k in line, k
    assert line["steps"] == 7 and line["warmup"] == 2 and line["value"] > 0 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
    assert "cpu_baseline" not in line and "sddmm_d64_ms" not in line["summary"] and "gcn_ms_per_epoch" not in line["summary"]
    with open(os.path.join(root, line["detail"])) as f:
        detail = json.load(f)
    assert detail["roofline"]["kernel_launches_timed"] == 7 and len(detail["datasets"]) == 1
    got = np.load(tmp_path / "out" / "spmm_out.npy")
    n, nnz, _, _ = G.SHAPES["reddit"]
    n, nnz = int(n * 0.05), int(nnz * 0.05 * 0.05)
    dev = torch.device("cuda:0")
    rp, col = G.GENERATORS["sbm_reddit"](n, nnz, seed=0, device=dev)
    E = col.numel()
    bp = torch.zeros((n + 15) // 16, dtype=torch.int32, device=dev)
    e2c = torch.zeros(E, dtype=torch.int32, device=dev); e2r = torch.zeros(E, dtype=torch.int32, device=dev)
    TCGNN.preprocess_gpu(col, rp, n, 16, 8, bp, e2c, e2r)
    X = torch.randn(n, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    want = TCGNN.forward(X, rp, col, bp, e2c, e2r)[0].cpu().numpy()
    TCGNN.clear_plan_cache()
    assert got.dtype == np.float32 and got.shape == want.shape == (n, 64)
    assert np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))) <= 1e-3
