"""Parity of the HIP path (TCGNN module -> C ABI -> gfx950 kernels) with the oracle.  Needs an
MI355X: run with `pytest -m gpu`.

Bar (BASELINE.json north_star): every output element within 1e-3 * max(1, |ref|) of the reference
kernels' semantics = the oracle in TF32 mode (operands rounded like wmma::__float_to_tf32, fp32
accumulate).  Because the staging pass rounds exactly like cvt.rna.tf32, the measured distance is
accumulation-order noise only, so a second, much tighter bound relative to sum|a||x| is asserted too.
"""
import os
import sys
import subprocess

import numpy as np
import pytest
import torch

import graphs
from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TOL = 1e-3          # the bar
TIGHT = 4e-6        # accumulation-order noise, relative to sum |a||x| (+1)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def T():
    import TCGNN
    return TCGNN


def to_dev(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def meta_for(dev, rp, col):
    bp, e2c, e2r, _ = graphs.host_sgt(rp, col)
    return (bp, e2c, e2r), to_dev(dev, rp, col, bp, e2c, e2r)


def assert_parity(got, ref_tf32, ref64, scale64, what, unit_scale=True):
    if unit_scale:
        # the north-star bar is stated for O(1) data; with inputs scaled by 300 a cancelling sum has
        # |ref| << sum|a||x| and fp32 accumulation order alone exceeds 1e-3 * max(1, |ref|) - the
        # reference's own tensor-core summation order would too.  Scaled inputs get the tight,
        # scale-relative bound below only.
        bar = np.abs(got - ref_tf32) / np.maximum(1.0, np.abs(ref_tf32))
        assert bar.size == 0 or bar.max() <= TOL, "%s: %.3e exceeds the 1e-3 bar" % (what, bar.max())
    tight = np.abs(got - ref_tf32) / (scale64 + 1.0)
    assert tight.size == 0 or tight.max() <= TIGHT, "%s: %.3e vs TF32-mode oracle (accumulation noise expected)" % (what, tight.max())
    # and it is as close to the exact fp64 contract as 10-bit operand rounding allows
    loose = np.abs(got - ref64) / (scale64 + 1.0)
    assert loose.size == 0 or loose.max() <= 2.0 ** -9


CASES = [(n, rp, c) for n, rp, c in graphs.edge_case_graphs()]
CASES.append(("citeseer_shape", *graphs.uniform_graph(3327, 2.8, seed=1)))
CASES.append(("dense_n3000_deg150", *graphs.uniform_graph(3000, 150, seed=2)))     # 4 wavefronts per window
CASES.append(("powerlaw_n12000_deg40", *graphs.powerlaw_graph(12000, 40, seed=3)))  # skewed window lengths
CASES.append(("hub_rows_n2500", *graphs.hub_rows_graph(2500, seed=77)))             # runs of more than four edges inside eight columns


def test_hardware_contracts_probe():
    """MFMA fragment layout, ds_read_b64_tr_b16 semantics, LDS-DMA destination order."""
    exe = os.path.join(ROOT, "tools", "bin", "probe_gfx950")
    if not os.path.exists(exe):
        pytest.skip("probe binary not built")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("D", [16, 64, 128, 1, 7, 41, 48, 200, 256])
def test_three_kernels_match_oracle(dev, T, case, D):
    name, rp, col = case
    n, nnz = len(rp) - 1, len(col)
    if n > 5000 and D in (1, 7, 48, 200, 256):
        pytest.skip("large graphs: headline widths only")
    (bp, e2c, e2r), (trp, tcol, tbp, te2c, te2r) = meta_for(dev, rp, col)
    rng = np.random.default_rng(1000 * D + n)
    mag = float(rng.choice([0.01, 1.0, 1.0, 300.0]))                                       # exercises the power-of-two scaling
    unit = mag <= 1.0
    X = (rng.standard_normal((n, D)) * mag).astype(np.float32)
    att = rng.standard_normal(nnz).astype(np.float32)
    tX, tatt = to_dev(dev, X, att)

    Y = T.forward(tX, trp, tcol, tbp, te2c, te2r)
    assert isinstance(Y, list) and len(Y) == 1 and Y[0].shape == (n, D) and Y[0].dtype == torch.float32
    Y64, absY = O.spmm_f64(X, rp, col)
    Yref = O.spmm(X, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32)
    assert_parity(Y[0].cpu().numpy(), Yref, Y64, absY, "spmm", unit)
    # small graphs take the single-launch fp32-MFMA kernel automatically: both it and the fp16 per-window kernel are
    # checked on every case (mode 4 / mode 1), whatever the automatic choice was
    import tcgnn_capi as c
    try:
        for mode in (1, 4):
            c.check(c.lib.tcgnn_set_spmm_mode(mode), "tcgnn_set_spmm_mode")
            assert_parity(T.forward(tX, trp, tcol, tbp, te2c, te2r)[0].cpu().numpy(), Yref, Y64, absY, "spmm mode %d" % mode, unit)
    finally:
        c.lib.tcgnn_set_spmm_mode(0)

    Yv = T.forward_AGNN(tX, trp, tcol, tatt.view(1, -1), tbp, te2c, te2r)[0]
    Yv64, absYv = O.spmm_f64(X, rp, col, att)
    assert_parity(Yv.cpu().numpy(), O.spmm_val(X, rp, col, att, bp, e2c, e2r, round_mode=O.ROUND_TF32), Yv64, absYv, "spmm_val", unit)

    ef = T.forward_ef(tX, trp, tcol, tbp, te2c, te2r)
    assert len(ef) == 1 and ef[0].shape == (nnz,) and ef[0].dtype == torch.float32
    ef64, absef = O.sddmm_f64(X, rp, col)
    assert_parity(ef[0].cpu().numpy(), O.sddmm(X, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32), ef64, absef, "sddmm", unit)


def test_edge_valued_spmm_on_hub_rows_with_runs_longer_than_four(dev, T):
    """Rows that are edges to (nearly) every column: a lane's run of values inside its eight tile columns is up to eight long
    and takes the second value fetch of TileWalker::dma_vals (TCGNN_kernel.cu:459-578 gathers value by value); every gather walk."""
    rp, col = graphs.hub_rows_graph(2500, seed=77)
    n, nnz = len(rp) - 1, len(col)
    (bp, e2c, e2r), (trp, tcol, tbp, te2c, te2r) = meta_for(dev, rp, col)
    rng = np.random.default_rng(78)
    import tcgnn_capi as c
    for D in (64, 41):
        X = rng.standard_normal((n, D)).astype(np.float32)
        att = rng.standard_normal(nnz).astype(np.float32)
        tX, tatt = to_dev(dev, X, att)
        Yv64, absYv = O.spmm_f64(X, rp, col, att)
        Yref = O.spmm_val(X, rp, col, att, bp, e2c, e2r, round_mode=O.ROUND_TF32)
        try:
            for mode in (0, 1, 2):
                c.check(c.lib.tcgnn_set_spmm_mode(mode), "tcgnn_set_spmm_mode")
                Yv = T.forward_AGNN(tX, trp, tcol, tatt.view(1, -1), tbp, te2c, te2r)[0]
                assert_parity(Yv.cpu().numpy(), Yref, Yv64, absYv, "spmm_val hub rows, mode %d" % mode, True)
        finally:
            c.lib.tcgnn_set_spmm_mode(0)


@pytest.mark.parametrize("D", [16, 64, 41, 128, 160])
def test_range_blocked_walk_matches_oracle_and_plain_walk(dev, T, D):
    """The persistent, column-range-blocked SpMM (chosen automatically for big feature matrices) is
    forced here on a graph small enough for the oracle; it must agree with the oracle and with the
    per-window kernel."""
    import tcgnn_capi as c
    rp, col = graphs.uniform_graph(16448, 180, seed=12)
    n, nnz = len(rp) - 1, len(col)
    (bp, e2c, e2r), (trp, tcol, tbp, te2c, te2r) = meta_for(dev, rp, col)
    rng = np.random.default_rng(D)
    X = rng.standard_normal((n, D)).astype(np.float32)
    att = rng.standard_normal(nnz).astype(np.float32)
    tX, tatt = to_dev(dev, X, att)
    out = {}
    try:
        for mode in (1, 2):
            c.check(c.lib.tcgnn_set_spmm_mode(mode), "tcgnn_set_spmm_mode")
            out[mode] = (T.forward(tX, trp, tcol, tbp, te2c, te2r)[0].cpu().numpy(),
                         T.forward_AGNN(tX, trp, tcol, tatt.view(1, -1), tbp, te2c, te2r)[0].cpu().numpy())
    finally:
        c.lib.tcgnn_set_spmm_mode(0)
    Y64, absY = O.spmm_f64(X, rp, col)
    Yv64, absYv = O.spmm_f64(X, rp, col, att)
    ref = O.spmm(X, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32)
    refv = O.spmm_val(X, rp, col, att, bp, e2c, e2r, round_mode=O.ROUND_TF32)
    for mode in (1, 2):
        assert_parity(out[mode][0], ref, Y64, absY, "spmm mode %d" % mode)
        assert_parity(out[mode][1], refv, Yv64, absYv, "spmm_val mode %d" % mode)


@pytest.mark.parametrize("range_kb", ["256", "1024", None])
@pytest.mark.parametrize("D", [16, 64, 41, 128, 96, 112])   # (96 / 112: the single-buffer run-list kernels at 6 and 7 tiles of width)
def test_slice_synchronised_walk_matches_oracle_and_plain_walk(dev, T, D, range_kb, monkeypatch, capfd):
    """r06: the slice-synchronised range walk (tcgnn_sync_walk.inc) - per slice of an XCD's share of the windows a
    list of hot column buckets, phases of a few buckets, one launch per slice round - forced (mode 5) on a community graph small enough
    for the oracle: 16 communities of 2 500 rows, 90 % of the edges inside, N % 16 = 3, with one, two or every hot bucket per phase.
    Binary and edge-valued SpMM against the oracle, fp64 and the per-window walk; SDDMM bit for bit equal to the per-window walk."""
    import re
    import tcgnn_capi as c
    rp, col = graphs.community_graph(40003, 16, 60, 0.9, seed=31)
    n, nnz = len(rp) - 1, len(col)
    (bp, e2c, e2r), meta = meta_for(dev, rp, col)
    rng = np.random.default_rng(D + 5)
    X = rng.standard_normal((n, D)).astype(np.float32)
    att = rng.standard_normal(nnz).astype(np.float32)
    tX, tatt = to_dev(dev, X, att)
    Xs = (X / np.sqrt(D)).astype(np.float32)
    tXs = to_dev(dev, Xs)[0]
    tdY = to_dev(dev, (rng.standard_normal((n, D)) / np.sqrt(D)).astype(np.float32))[0]
    tw = torch.tensor([0.7], device=dev)
    monkeypatch.setenv("TCGNN_VERBOSE", "1")
    if range_kb:
        monkeypatch.setenv("TCGNN_RANGE_KB", range_kb)
    out = {}
    try:
        T.clear_plan_cache()
        for mode in (1, 5):
            c.check(c.lib.tcgnn_set_spmm_mode(mode), "tcgnn_set_spmm_mode")
            Y = T.forward(tX, *meta)[0]
            k1 = T.last_kernel(*meta)
            Yv = T.forward_AGNN(tX, meta[0], meta[1], tatt.view(1, -1), *meta[2:])[0]
            k2 = T.last_kernel(*meta)
            ef = T.forward_ef(tXs, *meta)[0]
            k3 = T.last_kernel(*meta)
            Yf, eff, efm = T.agnn_fused_forward(tXs, meta[0], meta[1], tw, *meta[2:])
            k4 = T.last_kernel(*meta)
            Gb, dw = T.agnn_fused_backward(tdY, meta[0], meta[1], tw, eff, efm, *meta[2:])
            out[mode] = (Y.cpu().numpy(), Yv.cpu().numpy(), ef, (k1, k2, k3), T.forward(tX, *meta)[0], (Yf, eff, Gb, float(dw), k4))
    finally:
        c.lib.tcgnn_set_spmm_mode(0)
        T.clear_plan_cache()
    err = capfd.readouterr().err
    stats = re.findall(r"sync walk: (\d+) slices of (\d+) windows, buckets of (\d+) rows, ([0-9.]+) hot buckets per slice \(max (\d+)\), (\d+) % of the tiles", err)
    assert stats, err[-1500:]
    assert float(stats[0][3]) >= 2 and int(stats[0][5]) >= 60, stats
    assert out[5][3] == ("spmm_sync_kernel", "spmm_sync_kernel", "sddmm_kernel (slice-synchronised)"), out[5][3]
    assert out[1][3][0] == "spmm_kernel", out[1][3]
    Y64, absY = O.spmm_f64(X, rp, col)
    Yv64, absYv = O.spmm_f64(X, rp, col, att)
    ref = O.spmm(X, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32)
    refv = O.spmm_val(X, rp, col, att, bp, e2c, e2r, round_mode=O.ROUND_TF32)
    refe = O.sddmm(Xs, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32)
    ef64, efabs = O.sddmm_f64(Xs, rp, col)
    for mode in (1, 5):
        assert_parity(out[mode][0], ref, Y64, absY, "spmm mode %d" % mode)
        assert_parity(out[mode][1], refv, Yv64, absYv, "spmm_val mode %d" % mode)
    assert_parity(out[5][2].cpu().numpy(), refe, ef64, efabs, "sddmm slice-synchronised")
    assert torch.equal(out[5][2], out[1][2])
    assert torch.equal(out[5][4].cpu(), torch.from_numpy(out[5][0]))   # deterministic
    # the fused AGNN pair on the same schedule: scores bit for bit those of the per-window walk, sums in another order
    (Yf1, ef1, G1, dw1, _), (Yf5, ef5, G5, dw5, k5) = out[1][5], out[5][5]
    assert k5 == "agnn_kernel (slice-synchronised)", k5
    assert torch.equal(ef5, ef1) and torch.equal(ef5, out[1][2])
    sy = float(Yf1.abs().max()) + 1.0
    assert float((Yf5 - Yf1).abs().max()) <= 1e-5 * sy and float((G5 - G1).abs().max()) <= 1e-5 * (float(G1.abs().max()) + 1.0)
    assert abs(dw5 - dw1) <= 1e-5 * (abs(dw1) + 1.0), (dw1, dw5)


def test_metadata_from_reference_fixture_feeds_the_kernels(dev, T):
    """The five legacy arrays exactly as the reference's preprocess wrote them (golden fixture)."""
    f = np.load(os.path.join(GOLD, "sgt_powerlaw_n1000.npz"))
    rp, col = f["rowptr"], f["col"]
    nw = (len(rp) - 1 + 15) // 16
    bp, e2c, e2r = f["bp_with_guard"][:nw], f["e2c"], f["e2r"]
    X = np.random.default_rng(0).standard_normal((1000, 64)).astype(np.float32)
    trp, tcol, tbp, te2c, te2r, tX = to_dev(dev, rp, col, bp, e2c, e2r, X)
    Y = T.forward(tX, trp, tcol, tbp, te2c, te2r)[0].cpu().numpy()
    assert np.abs(Y - O.spmm(X, rp, col, bp, e2c, e2r)).max() <= 1e-4
    # over-allocated edge arrays (main_tcgnn.py:45-46 sizes them by the raw edge count) are accepted
    pad = torch.zeros(50, dtype=torch.int32, device=dev)
    Y2 = T.forward(tX, trp, tcol, tbp, torch.cat([te2c, pad]), torch.cat([te2r, pad]))[0].cpu().numpy()
    assert np.array_equal(Y, Y2)


def test_device_sgt_is_bit_identical_to_host_sgt(dev, T, capfd):
    for name, rp, col in CASES:
        n = len(rp) - 1
        bp, e2c, e2r, tc = graphs.host_sgt(rp, col)
        trp, tcol = to_dev(dev, rp, col)
        gbp = torch.full((len(bp) + 2,), -7, dtype=torch.int32, device=dev)
        ge2c = torch.zeros(len(col), dtype=torch.int32, device=dev)
        ge2r = torch.zeros(len(col), dtype=torch.int32, device=dev)
        assert T.preprocess_gpu(tcol, trp, n, 16, 8, gbp, ge2c, ge2r) is None
        assert capfd.readouterr().out == "TC_Blocks:\t%d\nExp_Edges:\t%d\n" % (tc, tc * 128), name
        assert np.array_equal(gbp[: len(bp)].cpu().numpy(), bp), name
        assert np.array_equal(ge2c.cpu().numpy(), e2c) and np.array_equal(ge2r.cpu().numpy(), e2r), name
        if n % 16 == 0:   # the reference's phantom window lands in the guard slot when one exists
            assert gbp[len(bp)].item() == 1 and gbp[len(bp) + 1].item() == -7
        else:
            assert gbp[len(bp)].item() == -7


def test_device_sgt_equals_the_reference_written_fixtures(dev, T, capfd):
    """The chain device SGT -> reference closes ON the GPU box: tests/golden/sgt_*.npz were written by the reference's own compiled
    `preprocess` (TCGNN.cpp:172-226 through oracle/_ref, tests/golden/make_golden.py); the device translation must reproduce them
    bit for bit, the count it prints included (the test above only compares with the product's host SGT)."""
    import glob
    paths = sorted(glob.glob(os.path.join(GOLD, "sgt_*.npz")))
    assert len(paths) >= 10
    for path in paths:
        f = np.load(path)
        rp, col = f["rowptr"], f["col"]
        n = len(rp) - 1
        nw = (n + 15) // 16
        trp, tcol = to_dev(dev, rp, col)
        gbp = torch.full((nw + 2,), -7, dtype=torch.int32, device=dev)
        ge2c = torch.zeros(max(len(col), 1), dtype=torch.int32, device=dev)
        ge2r = torch.zeros(max(len(col), 1), dtype=torch.int32, device=dev)
        assert T.preprocess_gpu(tcol, trp, n, 16, 8, gbp, ge2c, ge2r) is None
        tc = int(f["tc_blocks"])
        assert capfd.readouterr().out == "TC_Blocks:\t%d\nExp_Edges:\t%d\n" % (tc, tc * 128), path
        assert np.array_equal(gbp[:nw].cpu().numpy(), f["bp_with_guard"][:nw]), path
        assert np.array_equal(ge2c[: len(col)].cpu().numpy(), f["e2c"]) and np.array_equal(ge2r[: len(col)].cpu().numpy(), f["e2r"]), path


def test_rows_wider_than_the_descriptor_stride_go_as_column_blocks(dev, T):
    """D > 8128: one fp16 row no longer fits the 14-bit stride field of the gather walks' buffer descriptor (r1 ADVICE: it
    wrapped silently and every gather read the wrong row).  Such calls are cut into 4096-column blocks that share the whole
    matrix's scale; D = 4100 .. 8128 fits one descriptor now that long rows are padded to whole lines, not powers of two."""
    rp, col = graphs.uniform_graph(4000, 100, seed=5)        # > kSmallMaxTiles wide blocks: the fp16 gather walk, not the fp32 kernel
    (bp, e2c, e2r), meta = meta_for(dev, rp, col)
    assert T.plan_info(*meta)["wide_blocks"] > 8192
    n = len(rp) - 1
    rng = np.random.default_rng(3)
    att = rng.standard_normal(len(col)).astype(np.float32)
    tatt = torch.from_numpy(att).to(dev).view(1, -1)
    for D in (8200, 4100):
        X = rng.standard_normal((n, D)).astype(np.float32)
        tX = torch.from_numpy(X).to(dev)
        Y = T.forward(tX, *meta)[0].cpu().numpy()
        Yv = T.forward_AGNN(tX, meta[0], meta[1], tatt, *meta[2:])[0].cpu().numpy()
        for c0 in sorted({0, 4090, D - 16}):                  # first block, across the 4096-column seam, the ragged tail
            sl = slice(c0, min(c0 + 16, D))
            Xs = np.ascontiguousarray(X[:, sl])
            ref = O.spmm(Xs, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32)
            r64, a64 = O.spmm_f64(Xs, rp, col)
            assert_parity(Y[:, sl], ref, r64, a64, "spmm D=%d cols %d.." % (D, c0))
            refv = O.spmm_val(Xs, rp, col, att, bp, e2c, e2r, round_mode=O.ROUND_TF32)
            v64, av64 = O.spmm_f64(Xs, rp, col, att)
            assert_parity(Yv[:, sl], refv, v64, av64, "spmm_val D=%d cols %d.." % (D, c0))
        # SDDMM beyond 128 columns (sddmm_wide_kernel) forms 64-bit addresses from plain pointers - no descriptor, so no stride
        # field to overflow: any width (r2 ADVICE asked for D > 8192 on a graph above kSmallMaxTiles: this one)
        ef = T.forward_ef(tX, *meta)[0].cpu().numpy()
        assert T.last_kernel(*meta) == "sddmm_wide_kernel"
        e64, ae64 = O.sddmm_f64(X, rp, col)
        assert (np.abs(ef - e64) / (ae64 + 1.0)).max() <= 2.0 ** -9


def test_device_sgt_with_edge_arrays_longer_than_the_csr(dev, T, capfd):
    """main_tcgnn.py:45-46 sizes edgeToColumn / edgeToRow by the RAW edge count, which exceeds nnz once duplicates are merged
    (dataset.py:79): preprocess_gpu must translate nodePointer[num_nodes] edges, not edgeList.numel() (r1 ADVICE: the tail
    of the sort buffers was read uninitialised).  Ids >= num_nodes sort correctly; inconsistent row pointers are refused."""
    rp, col = graphs.uniform_graph(1000, 10, seed=9)
    n, nnz = len(rp) - 1, len(col)
    bp_h, e2c_h, e2r_h, total = graphs.host_sgt(rp, col)
    pad = 777
    tcol = torch.cat([torch.from_numpy(col), torch.full((pad,), 123456789, dtype=torch.int32)]).to(dev)
    trp = torch.from_numpy(rp).to(dev)
    bp = torch.zeros((n + 15) // 16, dtype=torch.int32, device=dev)
    e2c = torch.full((nnz + pad,), -7, dtype=torch.int32, device=dev); e2r = torch.full((nnz + pad,), -7, dtype=torch.int32, device=dev)
    T.preprocess_gpu(tcol, trp, n, 16, 8, bp, e2c, e2r)
    assert "TC_Blocks:\t%d" % total in capfd.readouterr().out
    assert np.array_equal(bp.cpu().numpy(), bp_h) and np.array_equal(e2c[:nnz].cpu().numpy(), e2c_h) and np.array_equal(e2r[:nnz].cpu().numpy(), e2r_h)
    assert bool((e2c[nnz:] == -7).all()) and bool((e2r[nnz:] == -7).all())          # the padding is never touched
    # column ids beyond num_nodes (a row shard's global ids): same ranks as the host path
    col2 = col.copy(); col2[col2 > 500] += 10 ** 6
    bp2, e2c2, e2r2, _ = graphs.host_sgt(rp, col2)
    e2c.fill_(-7)
    T.preprocess_gpu(torch.from_numpy(col2).to(dev), trp, n, 16, 8, bp, e2c[:nnz], e2r[:nnz])
    assert np.array_equal(bp.cpu().numpy(), bp2) and np.array_equal(e2c[:nnz].cpu().numpy(), e2c2)
    # row pointers that promise more edges than the array holds
    with pytest.raises(RuntimeError, match="nodePointer"):
        T.preprocess_gpu(tcol[: nnz - 5].contiguous(), trp, n, 16, 8, bp, e2c, e2r)


def test_device_sgt_on_caller_scratch_allocates_nothing(dev, T):
    """r06: tcgnn_preprocess_gpu_ws runs on caller scratch - no hipMalloc / hipFree inside the call (r05's
    translation made ~10 of them, 1.8 GB at Reddit size, and read 95 ms instead of 5 whenever the driver had to map fresh memory).
    Shown two ways: the device's free memory is the same before and after three calls, and the call succeeds with less free memory
    left on the device than its scratch needs (an internal allocation of that size would fail).  Same outputs as the host path and as
    the reference-shaped entry point, which allocates the scratch itself."""
    import ctypes
    import tcgnn_capi as c
    rp, col = graphs.uniform_graph(200_003, 60, seed=41)
    n, nnz = len(rp) - 1, len(col)
    bp_h, e2c_h, e2r_h, total = graphs.host_sgt(rp, col)
    trp, tcol = to_dev(dev, rp, col)
    nw = (n + 15) // 16
    bp = torch.zeros(nw, dtype=torch.int32, device=dev); e2c = torch.zeros(nnz, dtype=torch.int32, device=dev); e2r = torch.zeros(nnz, dtype=torch.int32, device=dev)
    need = ctypes.c_size_t(0)
    c.check(c.lib.tcgnn_preprocess_gpu_workspace_bytes(n, nnz, 16, ctypes.byref(need)), "workspace_bytes")
    assert need.value >= 4 * 4 * nnz
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    got = ctypes.c_int64(0)
    call = lambda: c.lib.tcgnn_preprocess_gpu_ws(tcol.data_ptr(), trp.data_ptr(), n, nnz, 16, 8, bp.data_ptr(), nw, e2c.data_ptr(), e2r.data_ptr(), ws.data_ptr(), need.value, ctypes.byref(got), st)
    c.check(call(), "first call")
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(dev)[0]
    for _ in range(3):
        c.check(call(), "call")
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(dev)[0] == free0
    assert got.value == total
    assert np.array_equal(bp.cpu().numpy(), bp_h) and np.array_equal(e2c.cpu().numpy(), e2c_h) and np.array_equal(e2r.cpu().numpy(), e2r_h)
    # too small a workspace is refused, not overrun
    assert c.lib.tcgnn_preprocess_gpu_ws(tcol.data_ptr(), trp.data_ptr(), n, nnz, 16, 8, bp.data_ptr(), nw, e2c.data_ptr(), e2r.data_ptr(), ws.data_ptr(), need.value - 256, ctypes.byref(got), st) == 5   # TCGNN_ERR_WORKSPACE
    # under memory pressure: all but ~half the scratch size of the device's free memory taken
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info(dev)[0]
    hog = torch.empty(free - need.value // 2, dtype=torch.uint8, device=dev)
    try:
        e2c.zero_()
        c.check(call(), "call under memory pressure")
        torch.cuda.synchronize()
        assert np.array_equal(e2c.cpu().numpy(), e2c_h)
        # (the reference-shaped entry point allocates its scratch: with this little memory left it reports the failure instead of crashing)
        assert c.lib.tcgnn_preprocess_gpu(tcol.data_ptr(), trp.data_ptr(), n, nnz, 16, 8, bp.data_ptr(), nw, e2c.data_ptr(), e2r.data_ptr(), ctypes.byref(got), st) == 3   # TCGNN_ERR_OOM
    finally:
        del hog
        torch.cuda.empty_cache()
    e2c.zero_()
    c.check(c.lib.tcgnn_preprocess_gpu(tcol.data_ptr(), trp.data_ptr(), n, nnz, 16, 8, bp.data_ptr(), nw, e2c.data_ptr(), e2r.data_ptr(), ctypes.byref(got), st), "reference-shaped entry point")
    assert got.value == total and np.array_equal(e2c.cpu().numpy(), e2c_h)


def test_non_canonical_rows_take_the_fallback_kernels(dev, T):
    rp, col = graphs.uniform_graph(500, 12, seed=4)
    rng = np.random.default_rng(4)
    col = col.copy()
    for r in range(500):
        col[rp[r]: rp[r + 1]] = rng.permutation(col[rp[r]: rp[r + 1]])     # unsorted but unique
    (bp, e2c, e2r), (trp, tcol, tbp, te2c, te2r) = meta_for(dev, rp, col)
    assert T.plan_info(trp, tcol, tbp, te2c, te2r)["canonical"] == 0
    X = rng.standard_normal((500, 48)).astype(np.float32); att = rng.standard_normal(len(col)).astype(np.float32)
    tX, tatt = to_dev(dev, X, att)
    assert np.abs(T.forward(tX, trp, tcol, tbp, te2c, te2r)[0].cpu().numpy() - O.spmm(X, rp, col, bp, e2c, e2r)).max() < 1e-3
    # the fallback kernels round operands like the reference too (TF32), so compare in that mode
    Yv = T.forward_AGNN(tX, trp, tcol, tatt.view(1, -1), tbp, te2c, te2r)[0].cpu().numpy()
    assert np.abs(Yv - O.spmm_val(X, rp, col, att, bp, e2c, e2r, round_mode=O.ROUND_TF32)).max() < 1e-4
    ef = T.forward_ef(tX, trp, tcol, tbp, te2c, te2r)[0].cpu().numpy()
    assert np.abs(ef - O.sddmm(X, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32)).max() < 1e-4


def test_layers_with_hip_kernels_reproduce_reference_fixture(dev, T):
    import tcgnn_layers as L
    L.set_backend(T)
    f = np.load(os.path.join(GOLD, "layers_n200.npz"))
    t = lambda k: torch.from_numpy(f[k]).to(dev)
    meta = (t("rowptr"), t("col"), t("bp"), t("e2c"), t("e2r"))
    dY = t("dY")

    def close(a, key, tol=TOL):
        b = f[key]
        return np.all(np.abs(a.detach().cpu().numpy() - b) <= tol * np.maximum(1.0, np.abs(b)))

    x = t("Xs").clone().requires_grad_(True)
    y = L.TCGNNFunction_SAG.apply(x, *meta); y.backward(dY)
    assert close(y, "sag_Y") and close(x.grad, "sag_dX")
    x, w = t("X").clone().requires_grad_(True), t("W").clone().requires_grad_(True)
    y = L.TCGNNFunction.apply(x, w, *meta); y.backward(dY)
    assert close(y, "gcn_Y") and close(x.grad, "gcn_dX") and close(w.grad, "gcn_dW")
    x, w = t("X").clone().requires_grad_(True), t("W").clone().requires_grad_(True)
    y = L.TCGNNFunction_GIN.apply(x, w, *meta); y.backward(dY)
    assert close(y, "gin_Y") and close(x.grad, "gin_dX") and close(w.grad, "gin_dW")
    x, w, a = t("X").clone().requires_grad_(True), t("W").clone().requires_grad_(True), t("attention_w").clone().requires_grad_(True)
    y = L.TCGNNFunction_AGNN.apply(x, w, a, *meta); y.backward(dY)
    # AGNN chains two rounded operators (att = a * sddmm(H) is itself re-rounded to 10 bits as the A
    # operand): an ulp-sized difference in ef can flip that rounding, so outputs are compared on the
    # scale of the tensor instead of element by element
    def close_max(t_, key, tol=TOL):
        b = f[key]
        return np.abs(t_.detach().cpu().numpy() - b).max() <= tol * max(1.0, np.abs(b).max())
    assert close_max(y, "agnn_Y") and close_max(x.grad, "agnn_dX") and close_max(w.grad, "agnn_dW")
    # ... and ELEMENT BY ELEMENT against the oracle fed the kernel's own scores (r06, VERDICT r05 item 7: the fixture bound above is on the
    # tensor's scale only).  With ef taken from the HIP path the rounding of att = a * ef cannot flip between the two sides, so every
    # element of Y, of the aggregated gradient, of dX and of dW answers to the 1e-3 bar.
    rp_h, col_h, bp_h, e2c_h, e2r_h = (f[k] for k in ("rowptr", "col", "bp", "e2c", "e2r"))
    Ht = torch.mm(t("X"), t("W"))
    ef_k = T.forward_ef(Ht, *meta)[0]
    att_k = (t("attention_w").reshape(-1, 1) * ef_k.unsqueeze(0)).contiguous()
    H_h, att_h = Ht.cpu().numpy(), att_k.reshape(-1).cpu().numpy()
    ref_y = O.spmm_val(H_h, rp_h, col_h, att_h, bp_h, e2c_h, e2r_h, round_mode=O.ROUND_TF32)
    ref_g = O.spmm_val(f["dY"], rp_h, col_h, att_h, bp_h, e2c_h, e2r_h, round_mode=O.ROUND_TF32)
    elementwise = lambda got, ref: np.all(np.abs(got.detach().cpu().numpy() - ref) <= TOL * np.maximum(1.0, np.abs(ref)))
    assert elementwise(y, ref_y)
    assert elementwise(x.grad, (ref_g.astype(np.float64) @ f["W"].astype(np.float64).T))
    assert elementwise(w.grad, (f["X"].astype(np.float64).T @ ref_g.astype(np.float64)))
    # d_attention_w = sum_e d_att[e] * col[e]: a signed 1180-term sum of O(100) terms; compare on the
    # scale of the terms, not of the (cancelling) result
    d_att = T.forward_ef(dY, *meta)[0]
    term_scale = float((d_att.abs() * meta[1].float()).sum())
    assert abs(a.grad.item() - np.asarray(f["agnn_dattention_w"]).reshape(-1)[0].item()) <= 1e-5 * term_scale


FUSED_CASES = [c for c in CASES if c[0] in ("uniform_n17", "uniform_n40", "empty_middle_window_n48", "powerlaw_n1000", "citeseer_shape",
                                            "dense_n3000_deg150", "powerlaw_n12000_deg40", "hub_rows_n2500")]


@pytest.mark.parametrize("case", FUSED_CASES, ids=[c[0] for c in FUSED_CASES])
@pytest.mark.parametrize("D", [16, 64, 128, 7, 41, 96])
def test_fused_agnn_products_equal_the_separate_calls_and_the_oracle(dev, T, case, D):
    """tcgnn_agnn_pair_forward / tcgnn_agnn_pair_backward (one gather for SDDMM + edge-weighted SpMM) against
    (a) the oracle composed the way gnn_conv.py:125-153 composes the operators and (b) the separate HIP calls."""
    name, rp, col = case
    n, nnz = len(rp) - 1, len(col)
    if n > 5000 and D in (7, 96):
        pytest.skip("large graphs: headline widths only")
    (bp, e2c, e2r), (trp, tcol, tbp, te2c, te2r) = meta_for(dev, rp, col)
    meta = (trp, tcol, tbp, te2c, te2r)
    rng = np.random.default_rng(77 * D + n)
    mag = float(rng.choice([0.05, 1.0, 1.0, 40.0]))
    H = (rng.standard_normal((n, D)) * mag / np.sqrt(D)).astype(np.float32)
    dY = rng.standard_normal((n, D)).astype(np.float32)
    wv = np.float32(rng.choice([0.7, -1.3, 2.5]))
    tH, tdY = to_dev(dev, H, dY)
    tw = torch.tensor([wv], device=dev)
    assert T.agnn_fused_supported(tH, *meta)

    Y, ef, efmax = T.agnn_fused_forward(tH, trp, tcol, tw, tbp, te2c, te2r)
    ef_sep = T.forward_ef(tH, *meta)[0]
    assert torch.equal(ef, ef_sep), "fused scores differ from tcgnn_sddmm"
    assert efmax[:1].view(torch.float32).item() == ef_sep.abs().max().item()
    att = (tw.view(1, 1) * ef_sep.unsqueeze(0)).contiguous()
    Y_sep = T.forward_AGNN(tH, trp, tcol, att, tbp, te2c, te2r)[0]
    # same operand rounding, same accumulation order inside a wavefront's run of tiles; the two kernels cut a window's
    # tiles into runs differently, so sums may differ by accumulation order only
    att_np = att.cpu().numpy()[0]
    Y64, absY = O.spmm_f64(H, rp, col, att_np)
    ref = O.spmm_val(H, rp, col, att_np, bp, e2c, e2r, round_mode=O.ROUND_TF32)
    assert_parity(Y.cpu().numpy(), ref, Y64, absY, "fused forward Y", mag <= 1.0)
    assert np.abs(Y.cpu().numpy() - Y_sep.cpu().numpy()).max() <= TIGHT * (absY.max() + 1.0)

    G, dw = T.agnn_fused_backward(tdY, trp, tcol, tw, ef, efmax, tbp, te2c, te2r)
    G_sep = T.forward_AGNN(tdY, trp, tcol, att, tbp, te2c, te2r)[0]
    G64, absG = O.spmm_f64(dY, rp, col, att_np)
    refG = O.spmm_val(dY, rp, col, att_np, bp, e2c, e2r, round_mode=O.ROUND_TF32)
    assert_parity(G.cpu().numpy(), refG, G64, absG, "fused backward G", mag <= 1.0)
    assert np.abs(G.cpu().numpy() - G_sep.cpu().numpy()).max() <= TIGHT * (absG.max() + 1.0)
    d_att = O.sddmm(dY, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32).astype(np.float64)
    want = float((d_att * col.astype(np.float64)).sum())
    term_scale = float((np.abs(d_att) * col).sum()) + 1.0
    assert dw.shape == (1,) and abs(float(dw) - want) <= 1e-6 * term_scale, (float(dw), want, term_scale)
    # deterministic: a second call returns the same bits
    G2, dw2 = T.agnn_fused_backward(tdY, trp, tcol, tw, ef, efmax, tbp, te2c, te2r)
    assert torch.equal(G, G2) and torch.equal(dw, dw2)



@pytest.mark.parametrize("D", [16, 32, 41, 64, 100, 128, 160])
@pytest.mark.parametrize("shape", ["dense", "ragged"])
def test_lds_resident_range_kernel_matches_oracle_and_plain_walk(dev, T, D, shape):
    """The LDS-resident column-range SpMM (every workgroup streams each 504-row range of the fp16 image into LDS and
    reads the MFMA B operand out of it; chosen automatically for dense graphs like Reddit) is forced here on
    graphs small enough for the oracle: several ranges, windows with no edge in some ranges, a ragged last
    window, a last range shorter than 504 rows, and more than one 64-column pass."""
    import tcgnn_capi as c
    if shape == "dense":
        rp, col = graphs.uniform_graph(4100, 150, seed=21)       # 9 ranges, ~18 distinct columns per cell
    else:
        rp, col = graphs.powerlaw_graph(2061, 9.0, seed=22)     # N % 16 = 13, N % 504 = 45, hubs with > 6 tiles per range
    n, nnz = len(rp) - 1, len(col)
    (bp, e2c, e2r), (trp, tcol, tbp, te2c, te2r) = meta_for(dev, rp, col)
    rng = np.random.default_rng(D + 3)
    X = rng.standard_normal((n, D)).astype(np.float32)
    (tX,) = to_dev(dev, X)
    out = {}
    try:
        for mode in (1, 3):
            c.check(c.lib.tcgnn_set_spmm_mode(mode), "tcgnn_set_spmm_mode")
            out[mode] = T.forward(tX, trp, tcol, tbp, te2c, te2r)[0].cpu().numpy()
        assert T.last_kernel(trp, tcol, tbp, te2c, te2r).startswith("spmm_lds_"), T.last_kernel(trp, tcol, tbp, te2c, te2r)   # (mode 3 did not take another walk)
    finally:
        c.lib.tcgnn_set_spmm_mode(0)
    assert T.plan_info(trp, tcol, tbp, te2c, te2r)["lds_ranges"] in ((n + 503) // 504, (n + 631) // 632, (n + 759) // 760, (n + 1527) // 1528)   # finest cell stream built so far
    Y64, absY = O.spmm_f64(X, rp, col)
    ref = O.spmm(X, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32)
    for mode in (1, 3):
        assert_parity(out[mode], ref, Y64, absY, "spmm mode %d" % mode)

def test_reordered_graph_gives_the_same_results_under_the_new_names(dev, T):
    """tcgnn_graph.community_order + permute_csr rename the nodes; the operators on the renamed graph are the operators on the
    original one under the renaming: Y'[k] = Y[order[k]], and every edge keeps its score."""
    import tcgnn_graph as G
    n, nnz = 30000, 2400000
    rp, col = G.sbm_csr(n, nnz, seed=9, device=dev, blocks=30, shuffle=True)
    order = G.community_order(rp, col, seed=9)
    rp2, col2 = G.permute_csr(rp, col, order)
    def meta_of(rp_, col_):
        E_ = col_.numel()
        bp = torch.zeros((n + 15) // 16, dtype=torch.int32, device=dev); e2c = torch.zeros(E_, dtype=torch.int32, device=dev); e2r = torch.zeros(E_, dtype=torch.int32, device=dev)
        T.preprocess_gpu(col_, rp_, n, 16, 8, bp, e2c, e2r)
        return (rp_, col_, bp, e2c, e2r)
    m1, m2 = meta_of(rp, col), meta_of(rp2, col2)
    assert int(m2[2].sum()) < 0.8 * int(m1[2].sum())                           # the renamed graph condenses into fewer TC blocks
    X = torch.randn(n, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    Y1, Y2 = T.forward(X, *m1)[0], T.forward(X[order], *m2)[0]
    scale = float(Y1.abs().max()) + 1.0
    assert float((Y2 - Y1[order]).abs().max()) <= 1e-4 * scale                  # (summation order differs: other tiles)
    ef1, ef2 = T.forward_ef(X, *m1)[0], T.forward_ef(X[order], *m2)[0]
    assert abs(float(ef1.double().sum()) - float(ef2.double().sum())) <= 1e-6 * float(ef1.double().abs().sum())
    k = 4321                                                                     # one row's scores, edge by edge
    old = int(order[k])
    newid = torch.empty(n, dtype=torch.long, device=dev); newid[order] = torch.arange(n, device=dev)
    a = dict(zip(newid[col[rp[old]:rp[old + 1]].long()].tolist(), ef1[rp[old]:rp[old + 1]].tolist()))
    b = dict(zip(col2[rp2[k]:rp2[k + 1]].long().tolist(), ef2[rp2[k]:rp2[k + 1]].tolist()))
    assert a.keys() == b.keys() and all(abs(a[c] - b[c]) <= 1e-5 * (1.0 + abs(a[c])) for c in a)


def test_locality_statistic_of_the_numbering(dev, T, capfd, monkeypatch):
    """The plan-time statistic behind the choice between the per-window walk in contiguous order and the range-blocked walk
    (DESIGN.md 4.6): share of the condensed columns within num_cols / 16 rows of their window - 2/16 for a uniform graph, nearly
    all for consecutively numbered communities; the results of the walks agree either way."""
    import re
    import tcgnn_graph as G
    import tcgnn_capi as c
    monkeypatch.setenv("TCGNN_VERBOSE", "1")
    seen = {}
    for name, (rp, col) in (("uniform", G.synthetic_csr(40000, 2400000, seed=2, device=dev)), ("sbm", G.sbm_csr(40000, 2400000, seed=2, device=dev, blocks=40))):
        n, E = rp.numel() - 1, col.numel()
        bp = torch.zeros((n + 15) // 16, dtype=torch.int32, device=dev); e2c = torch.zeros(E, dtype=torch.int32, device=dev); e2r = torch.zeros(E, dtype=torch.int32, device=dev)
        T.preprocess_gpu(col, rp, n, 16, 8, bp, e2c, e2r)
        meta = (rp, col, bp, e2c, e2r)
        T.clear_plan_cache()
        capfd.readouterr()
        X = torch.randn(n, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        att = torch.randn(1, E, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
        out = {}
        try:
            for mode in (0, 1, 2):
                c.check(c.lib.tcgnn_set_spmm_mode(mode), "tcgnn_set_spmm_mode")
                out[mode] = (T.forward_AGNN(X, rp, col, att, bp, e2c, e2r)[0], T.forward_ef(X, *meta)[0])
        finally:
            c.lib.tcgnn_set_spmm_mode(0)
        m = re.search(r"plan: (\d+) % of the condensed columns", capfd.readouterr().err)
        assert m, "no locality line"
        seen[name] = int(m.group(1))
        scale = float(out[1][0].abs().max()) + 1.0
        for mode in (0, 2):
            assert float((out[mode][0] - out[1][0]).abs().max()) <= 1e-4 * scale
            assert torch.equal(out[mode][1], out[1][1])          # SDDMM: the same products whatever the walk
    assert 8 <= seen["uniform"] <= 20 and seen["sbm"] >= 75, seen


@pytest.mark.parametrize("graph", ["uniform", "communities"])   # (r06: a graph with communities - where the walk's window order decides whether it stays in step)
@pytest.mark.parametrize("D", [16, 64, 128])
def test_sddmm_range_major_walk_with_xcd_affinity_gives_the_same_scores(dev, T, D, graph, monkeypatch):
    """r03: the range-major SDDMM with XCD affinity (workgroup b takes the column ranges b % 8, b % 8 + 8, ... only, so an XCD's
    L2 is asked for an eighth of the image).  Every edge lies in exactly one range: the scores are bit for bit those of the
    per-window walk and of the range-major walk without affinity.  Forced here with small ranges (TCGNN_RANGE_KB) on a graph the
    oracle can handle, N % 16 != 0, so that there are 8, 16 and more ranges."""
    import tcgnn_capi as c
    rp, col = graphs.uniform_graph(70003, 80, seed=23) if graph == "uniform" else graphs.community_graph(70003, 50, 80, 0.3, seed=23)
    n = len(rp) - 1
    (bp, e2c, e2r), (trp, tcol, tbp, te2c, te2r) = meta_for(dev, rp, col)
    meta = (trp, tcol, tbp, te2c, te2r)
    assert T.plan_info(*meta)["column_buckets"] % 16 == 0
    X = (np.random.default_rng(D).standard_normal((n, D)) / np.sqrt(D)).astype(np.float32)
    tX = to_dev(dev, X)[0]
    ref = O.sddmm(X, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32)
    ef64, efabs = O.sddmm_f64(X, rp, col)
    out = {}
    try:
        c.check(c.lib.tcgnn_set_spmm_mode(1), "tcgnn_set_spmm_mode")
        out["per-window"] = T.forward_ef(tX, *meta)[0]
        c.check(c.lib.tcgnn_set_spmm_mode(2), "tcgnn_set_spmm_mode")
        image_kb = (n + 1) * max(32, 1 << int(np.ceil(np.log2(2 * ((D + 15) // 16 * 16))))) // 1024
        for xcd in ("0", "1"):
            for parts in (8, 16, 64):
                for ident in ("1", "0"):   # (r06: items in the graph's own order - the default - and through the plan's XCD-contiguous order)
                    monkeypatch.setenv("TCGNN_SDDMM_XCD", "2" if xcd == "1" else "0")
                    monkeypatch.setenv("TCGNN_RM_IDENT", ident)
                    monkeypatch.setenv("TCGNN_RANGE_KB", str(max(1, image_kb // parts)))
                    out[(xcd, parts, ident)] = T.forward_ef(tX, *meta)[0]
    finally:
        c.lib.tcgnn_set_spmm_mode(0)
    base = out["per-window"]
    assert_parity(base.cpu().numpy(), ref, ef64, efabs, "sddmm per-window")
    for k, v in out.items():
        assert torch.equal(v, base), k


@pytest.mark.parametrize("hot", [None, 1800])
@pytest.mark.parametrize("D", [16, 48, 64, 128])
def test_lds_resident_walk_splits_hub_windows_over_wavefronts(dev, T, D, hot, capfd, monkeypatch):
    """Hub rows: a window far heavier than a wavefront's share of its workgroup is split over several wavefronts, each taking
    runs of its tiles in every column range; the partial sums meet in LDS in a fixed order.  Forced LDS-resident walk (mode 3)
    on a graph with a few near-complete rows; against the oracle, the per-window gather walk and itself (deterministic);
    with the fused ReLU and the dense update behind it."""
    import tcgnn_capi as c
    rp, col = graphs.hub_rows_graph(9000, seed=5, full_rows=20, half_rows=4, background=250000, bg_cols=None if hot is None else 4500)
    n = len(rp) - 1
    (bp, e2c, e2r), meta = meta_for(dev, rp, col)
    rng = np.random.default_rng(D)
    X = rng.standard_normal((n, D)).astype(np.float32)
    (tX,) = to_dev(dev, X)
    monkeypatch.setenv("TCGNN_VERBOSE", "1")
    if hot is not None:   # with a cold remainder as well: part 0 of a split window emits the whole window's cold columns
        monkeypatch.setenv("TCGNN_LDS_HOT_COLS", str(hot))
    T.clear_plan_cache()
    try:
        c.check(c.lib.tcgnn_set_spmm_mode(3), "tcgnn_set_spmm_mode")
        Y = T.forward(tX, *meta)[0]
        assert T.last_kernel(*meta).startswith("spmm_lds_")
        with_cold = "cold remainder" in T.last_kernel(*meta)
        assert not (hot is None and with_cold)
        again = T.forward(tX, *meta)[0]
        Yr = T.forward_fused(tX, *meta, relu=True)[0]
        W = torch.randn(D, 24, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) if D <= 128 else None
        Yw = T.forward_gemm(tX, W, *meta)[0] if W is not None else None
        c.check(c.lib.tcgnn_set_spmm_mode(1), "tcgnn_set_spmm_mode")
        Y1 = T.forward(tX, *meta)[0]
    finally:
        c.lib.tcgnn_set_spmm_mode(0)
        T.clear_plan_cache()
    err = capfd.readouterr().err
    assert "windows split over several wavefronts" in err, err[-600:]
    if hot is not None and D in (16, 64):
        assert with_cold, err[-600:]   # (the threshold leaves both parts non-empty at these widths' layouts)
    assert torch.equal(Y, again)
    Y64, absY = O.spmm_f64(X, rp, col)
    ref = O.spmm(X, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32)
    assert_parity(Y.cpu().numpy(), ref, Y64, absY, "split hub windows", True)
    assert np.abs(Y.cpu().numpy() - Y1.cpu().numpy()).max() <= TIGHT * (absY.max() + 1.0)
    assert torch.equal(Yr, torch.relu(Y))
    if Yw is not None:
        ref_w = Y64 @ W.double().cpu().numpy()
        bound = (absY @ np.abs(W.double().cpu().numpy())) * 2.0 ** -9 + 1e-6
        assert (np.abs(Yw.cpu().numpy() - ref_w) <= bound).all()


@pytest.mark.parametrize("graph", ["powerlaw_n2061", "hub_rows_n9000"])
def test_refused_edge_valued_stream_leaves_the_plan_as_it_found_it(dev, T, graph, monkeypatch):
    """A failed cell-stream build leaves its slot of the plan exactly as it found it (cells_publish is the only writer and cannot
    fail).  The one failure that needs no provoked error: the edge-valued stream of a graph with split hub windows, which keep the
    ordinary stream, is refused (TCGNN_ERR_UNSUPPORTED inside the library, its text left in tcgnn_last_error; build_val_stream
    answers such a refusal by settling the plan on the gather walks, so tcgnn_plan_prepare_val itself returns TCGNN_OK, forced mode
    or not).  plan_bytes is then back at what it was before the attempt (the single-edge source released, nothing of a cell
    stream left behind), a second prepare finds the question settled, forward_AGNN takes the gather walk, and the plan is
    destroyed cleanly.  hub_rows_n9000 must take that path.  powerlaw_n2061 splits its hub windows only where the chip has few
    enough CUs for a window to exceed a wavefront's share (on the 256 CUs of the MI355X it does not: measured, the stream is
    built): there the stream must be in the plan's bytes and forward_AGNN must run on it."""
    import tcgnn_capi as c
    if graph == "powerlaw_n2061":
        rp, col = graphs.powerlaw_graph(2061, 9.0, seed=22)
    else:
        rp, col = graphs.hub_rows_graph(9000, seed=5, full_rows=20, half_rows=4, background=250000)
    n, nnz = len(rp) - 1, len(col)
    (bp, e2c, e2r), meta = meta_for(dev, rp, col)
    rng = np.random.default_rng(64)
    X = rng.standard_normal((n, 64)).astype(np.float32)
    att = rng.standard_normal(nnz).astype(np.float32)
    tX, tatt = to_dev(dev, X, att)
    monkeypatch.setenv("TCGNN_LDS_FLAT", "1")
    T.clear_plan_cache()
    try:
        c.check(c.lib.tcgnn_set_spmm_mode(3), "tcgnn_set_spmm_mode")
        T.prepare([64], *meta)                                # (the binary walk's streams of this width: theirs to keep)
        before = T.plan_info(*meta)["plan_bytes"]
        T.prepare([64], *meta, edge_valued=True)
        refusal = c.lib.tcgnn_last_error().decode("utf-8", "replace")
        after = T.plan_info(*meta)["plan_bytes"]
        T.prepare([64], *meta, edge_valued=True)              # settled either way: nothing is built, nothing released
        again = T.plan_info(*meta)["plan_bytes"]
        Y = T.forward_AGNN(tX, meta[0], meta[1], tatt.view(1, -1), *meta[2:])[0].cpu().numpy()
        kernel = T.last_kernel(*meta)
        at_end = T.plan_info(*meta)["plan_bytes"]
    finally:
        c.lib.tcgnn_set_spmm_mode(0)
        T.clear_plan_cache()
    print("%s: plan_bytes %d before, %d after prepare(edge_valued=True), kernel %s" % (graph, before, after, kernel))
    refused = kernel == "spmm_kernel"
    assert refused or graph == "powerlaw_n2061", kernel
    if refused:
        assert "edge-valued LDS-resident SpMM: the single-edge cells of this graph are not uniform enough for a flat stream" in refusal, refusal
        assert after == before, (before, after)
    else:
        assert "spmm_lds_val_kernel" in kernel and after > before, (kernel, before, after)
    assert again == after and at_end == after, (after, again, at_end)
    ref = O.spmm_val(X, rp, col, att, bp, e2c, e2r, round_mode=O.ROUND_TF32)
    Y64, absY = O.spmm_f64(X, rp, col, att)
    assert_parity(Y, ref, Y64, absY, "forward_AGNN behind a refused / built edge-valued stream")


@pytest.mark.parametrize("D", [16, 32, 41, 64, 100, 128, 160])
@pytest.mark.parametrize("flat", ["1", "2"])
@pytest.mark.parametrize("shape", ["dense", "denser", "ragged"])
def test_flat_cell_stream_matches_oracle_and_the_ordinary_stream(dev, T, D, flat, shape, monkeypatch, capfd):
    """r03: the LDS-resident walk over a FLAT cell stream (tcgnn_lds_flat.inc): every cell of a (workgroup, range) pair has exactly
    1 or 2 tiles at a computed position, the range body is straight-line code, and the columns a cell holds beyond its tiles go
    to the cold remainder, which spmm_cold_planar_kernel adds from the planar image.  Forced here (mode 3 + TCGNN_LDS_FLAT) on
    graphs whose cells overflow often (`denser`: ~50 columns per 760-row cell against a cap of 32) and hardly ever, every layout
    (1-4 planes x 4 windows, 2 planes x 8 windows), against the oracle, the per-window gather walk and the ordinary stream; the
    fused ReLU / gate and determinism ride along."""
    import tcgnn_capi as c
    if shape == "dense":
        rp, col = graphs.uniform_graph(4100, 150, seed=21)
    elif shape == "denser":
        rp, col = graphs.uniform_graph(3000, 400, seed=23)
    else:
        rp, col = graphs.powerlaw_graph(2061, 9.0, seed=22)      # N % 16 = 13; hub windows (split parts keep the ordinary stream)
    n = len(rp) - 1
    (bp, e2c, e2r), meta = meta_for(dev, rp, col)
    rng = np.random.default_rng(D + 5)
    X = rng.standard_normal((n, D)).astype(np.float32)
    W = (rng.standard_normal((D, 24)) / D ** 0.5).astype(np.float32)
    tX, tW = to_dev(dev, X, W)
    monkeypatch.setenv("TCGNN_VERBOSE", "1")
    monkeypatch.setenv("TCGNN_LDS_DENSE_COLS", "1000000000")   # (r05: no dense entries here - this test holds the COLD remainder of a flat stream; test_flat_stream_with_dense_entries has the other way)
    out, gemm = {}, {}
    try:
        for f in (flat, "0"):
            monkeypatch.setenv("TCGNN_LDS_FLAT", f)
            T.clear_plan_cache()
            c.check(c.lib.tcgnn_set_spmm_mode(3), "tcgnn_set_spmm_mode")
            Y = T.forward(tX, *meta)[0]
            out[f] = (Y, T.last_kernel(*meta), T.forward_fused(tX, *meta, relu=True)[0], T.forward_fused(tX, *meta, gate=Y)[0], T.forward(tX, *meta)[0])
            if D <= 64:    # the dense update in the epilogue (f3): the flat kernel multiplies its cold remainder itself, so it keeps the update
                gemm[f] = (T.forward_gemm(tX, tW, *meta)[0], T.last_kernel(*meta), T.forward_gemm(tX, tW, *meta, relu=True)[0])
        c.check(c.lib.tcgnn_set_spmm_mode(1), "tcgnn_set_spmm_mode")
        Y1 = T.forward(tX, *meta)[0]
        Yg1 = T.forward_fused(tX, *meta, gate=out[flat][0])[0]
    finally:
        c.lib.tcgnn_set_spmm_mode(0)
        T.clear_plan_cache()
    err = capfd.readouterr().err
    Y, kernel, Yr, Yg, again = out[flat]
    if "windows split over several wavefronts" in err:
        assert kernel.startswith("spmm_lds_kernel"), kernel          # split hub windows keep the ordinary stream
    else:
        assert kernel.startswith("spmm_lds_flat_kernel"), (kernel, err[-800:])
        assert ("flat, %s tile" % flat) in err or ("flat: %s tile" % flat) in err, err[-800:]
        if shape == "denser" and flat == "1":
            assert "columns beyond the cells' tiles moved to the cold remainder" in err and " 0 columns beyond" not in err
            # layouts with LDS to spare multiply the remainder inside the kernel, the others leave it to spmm_cold_planar_kernel
            inside = True                      # (every layout these widths use has the room: a 3-plane remainder goes as 8-window chunks)
            assert kernel == ("spmm_lds_flat_kernel" if inside else "spmm_lds_flat_kernel + spmm_cold_planar_kernel (cold remainder)"), kernel
    assert out["0"][1].startswith("spmm_lds_kernel")
    assert torch.equal(Y, again)
    Y64, absY = O.spmm_f64(X, rp, col)
    ref = O.spmm(X, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32)
    assert_parity(Y.cpu().numpy(), ref, Y64, absY, "flat stream")
    assert_parity(out["0"][0].cpu().numpy(), ref, Y64, absY, "ordinary stream")
    assert np.abs(Y.cpu().numpy() - Y1.cpu().numpy()).max() <= TIGHT * (absY.max() + 1.0)
    assert torch.equal(Yr, torch.relu(Y))
    assert np.abs(Yg.cpu().numpy() - Yg1.cpu().numpy()).max() <= TIGHT * (absY.max() + 1.0)
    if gemm:
        Z, zkernel, Zr = gemm[flat]
        # (a remainder the flat kernel multiplies itself keeps the update in its epilogue; one added by spmm_cold_planar_kernel - two
        #  tiles per cell in the 8-window layout leave no LDS for it - hands the call to the gather walk, whose epilogue has the update too)
        assert zkernel == ("spmm_lds_flat_kernel" if kernel == "spmm_lds_flat_kernel" else "spmm_kernel"), (kernel, zkernel)
        want = Y.double().cpu().numpy() @ W.astype(np.float64)          # the update of the kernel's own aggregate, fp32 MFMA
        scale = np.abs(absY).max() * np.abs(W).sum(0).max() + 1.0
        assert np.abs(Z.cpu().numpy() - want).max() <= 1e-5 * scale, np.abs(Z.cpu().numpy() - want).max()
        assert torch.equal(Zr, torch.relu(Z))
        if gemm["0"][1].startswith("spmm_lds_kernel"):
            assert np.abs(gemm["0"][0].cpu().numpy() - Z.cpu().numpy()).max() <= TIGHT * scale


@pytest.mark.parametrize("D", [16, 32, 41, 48, 64, 128])
@pytest.mark.parametrize("case", ["communities", "communities_some_cold", "denser_all_dense", "communities_default_threshold"])
def test_flat_stream_with_dense_entries(dev, T, D, case, monkeypatch, capfd):
    """r05: DENSE ENTRIES of the flat cell stream (tcgnn_lds_flat.inc).  A hot (workgroup, range) pair whose cells
    overflow their one tile by much keeps all its columns in the LDS-resident walk: the tiles beyond each cell's first sit in dense
    entries behind the workgroup's normal ones - ordinary-format tiles, a per-slot count word, a run-time loop per window slot.  On
    community graphs (a window's own community = two dense column ranges of ~19 tiles per cell, N % 16 != 0), with every overflowing
    pair dense, with only the community pairs dense and the rest of the overflow in the cold remainder, and with the default
    threshold; every layout the automatic passes use (1 - 2 planes x 4 / 8 windows; a 3-plane remainder goes as 8-window chunks).  Against the oracle, fp64, the ordinary stream and the per-window gather walk; ReLU epilogue, the fused dense update
    and determinism ride along."""
    import tcgnn_capi as c
    if case == "denser_all_dense":
        rp, col = graphs.uniform_graph(3000, 400, seed=23)
    else:
        rp, col = graphs.community_graph(6061, 4, 300, 0.5, seed=5)      # N % 16 = 13
    n = len(rp) - 1
    (bp, e2c, e2r), meta = meta_for(dev, rp, col)
    rng = np.random.default_rng(D + 17)
    X = rng.standard_normal((n, D)).astype(np.float32)
    W = (rng.standard_normal((D, 24)) / D ** 0.5).astype(np.float32)
    tX, tW = to_dev(dev, X, W)
    monkeypatch.setenv("TCGNN_VERBOSE", "1")
    if case != "communities_default_threshold":
        monkeypatch.setenv("TCGNN_LDS_DENSE_COLS", "5000" if case == "communities_some_cold" else "1")
    out = {}
    try:
        for f in ("1", "0"):
            monkeypatch.setenv("TCGNN_LDS_FLAT", f)
            T.clear_plan_cache()
            c.check(c.lib.tcgnn_set_spmm_mode(3), "tcgnn_set_spmm_mode")
            Y = T.forward(tX, *meta)[0]
            out[f] = [Y, T.last_kernel(*meta), T.forward_fused(tX, *meta, relu=True)[0], T.forward(tX, *meta)[0]]
            if D <= 64:
                out[f] += [T.forward_gemm(tX, tW, *meta)[0], T.last_kernel(*meta)]
        c.check(c.lib.tcgnn_set_spmm_mode(1), "tcgnn_set_spmm_mode")
        Y1 = T.forward(tX, *meta)[0]
    finally:
        c.lib.tcgnn_set_spmm_mode(0)
        T.clear_plan_cache()
    err = capfd.readouterr().err
    Y, kernel, Yr, again = out["1"][:4]
    assert kernel.startswith("spmm_lds_flat_kernel"), (kernel, err[-800:])
    import re
    dense = [int(x) for x in re.findall(r"entries \((\d+) dense\)", err)]
    assert dense, err[-1500:]
    assert max(dense) > 0, err[-1500:]               # (48 columns = 3 planes go as 8-window chunks of two planes: a dense walk too)
    Y64, absY = O.spmm_f64(X, rp, col)
    ref = O.spmm(X, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32)
    assert_parity(Y.cpu().numpy(), ref, Y64, absY, "flat stream with dense entries")
    assert_parity(out["0"][0].cpu().numpy(), ref, Y64, absY, "ordinary stream")
    assert torch.equal(Y, again)
    assert torch.equal(Yr, torch.relu(Y))
    assert np.abs(Y.cpu().numpy() - Y1.cpu().numpy()).max() <= TIGHT * (absY.max() + 1.0)
    if D <= 64:
        Z, zkernel = out["1"][4:6]
        want = (Y if zkernel.startswith("spmm_lds_flat_kernel") else Y1).double().cpu().numpy() @ W.astype(np.float64)
        scale = np.abs(absY).max() * np.abs(W).sum(0).max() + 1.0
        assert np.abs(Z.cpu().numpy() - want).max() <= 1e-5 * scale, (zkernel, np.abs(Z.cpu().numpy() - want).max())


@pytest.mark.parametrize("shape", ["dense", "denser", "multi_edge_columns", "ragged"])
@pytest.mark.parametrize("D", [64, 128])
def test_edge_valued_spmm_on_the_lds_resident_walk(dev, T, D, shape, monkeypatch, capfd):
    """r04: forward_AGNN on the LDS-resident flat walk (tcgnn_lds_val.inc) - the cell stream is cut from a
    SINGLE-EDGE tile stream, so a K slot carries one edge and the caller's values, brought into stream order per call by
    val_permute_kernel, sit beside the slots.  Forced (mode 3) on graphs whose cells overflow often (`denser`: the remainder goes
    through spmm_cold_val_kernel), hardly ever, whose columns hold MANY edges of a window (`multi_edge_columns`: half of all pairs are
    edges, so a condensed column carries ~8 of a window's rows and is repeated once per edge when the stream is cut) and with N % 16 != 0; against the oracle, the fp64 definition and the per-window gather walk.  The
    first call builds the stream and still takes a gather walk (its workspace was sized before the stream existed)."""
    import tcgnn_capi as c
    if shape == "dense":
        rp, col = graphs.uniform_graph(4100, 150, seed=21)
    elif shape == "denser":
        rp, col = graphs.uniform_graph(3000, 400, seed=23)
    elif shape == "multi_edge_columns":
        rp, col = graphs.uniform_graph(1000, 500, seed=25)
    else:
        rp, col = graphs.uniform_graph(2061, 120, seed=24)      # N % 16 = 13
    n, nnz = len(rp) - 1, len(col)
    (bp, e2c, e2r), meta = meta_for(dev, rp, col)
    rng = np.random.default_rng(D + 9)
    X = rng.standard_normal((n, D)).astype(np.float32)
    att = (rng.standard_normal(nnz) * rng.choice([0.01, 1.0, 30.0])).astype(np.float32)
    tX, tatt = to_dev(dev, X, att)
    args = (tX, meta[0], meta[1], tatt.view(1, -1), *meta[2:])
    monkeypatch.setenv("TCGNN_VERBOSE", "1")
    monkeypatch.setenv("TCGNN_LDS_DENSE_COLS", "1000000000")   # (r05: no dense entries - this test holds the cold remainder; test_edge_valued_lds_walk_with_dense_entries the other way)
    monkeypatch.setenv("TCGNN_LDS_FLAT", "1")    # (graphs the oracle can handle have few, long cells: one tile per cell is forced, the rest is the cold remainder)
    T.clear_plan_cache()
    try:
        c.check(c.lib.tcgnn_set_spmm_mode(3), "tcgnn_set_spmm_mode")
        first = T.forward_AGNN(*args)[0]
        k_first = T.last_kernel(*meta)
        Y = T.forward_AGNN(*args)[0]
        kernel = T.last_kernel(*meta)
        again = T.forward_AGNN(*args)[0]
        c.check(c.lib.tcgnn_set_spmm_mode(1), "tcgnn_set_spmm_mode")
        Y1 = T.forward_AGNN(*args)[0]
        assert T.last_kernel(*meta) == "spmm_kernel"
    finally:
        c.lib.tcgnn_set_spmm_mode(0)
        T.clear_plan_cache()
    err = capfd.readouterr().err
    ref = O.spmm_val(X, rp, col, att, bp, e2c, e2r, round_mode=O.ROUND_TF32)
    Y64, absY = O.spmm_f64(X, rp, col, att)
    unit = float(np.abs(att).max()) <= 8.0
    assert_parity(first.cpu().numpy(), ref, Y64, absY, "first call (%s)" % k_first, unit)
    assert_parity(Y1.cpu().numpy(), ref, Y64, absY, "per-window gather walk", unit)
    # (the first call takes the new walk too when the process already holds a workspace large enough for the slot values)
    assert "spmm_lds_val_kernel" in kernel, (k_first, kernel, err[-1500:])
    assert "cold remainder" in kernel, kernel        # (cells of 100+ edges against a cap of 32: most of these graphs is remainder)
    assert torch.equal(Y, again)                                                     # deterministic
    assert_parity(Y.cpu().numpy(), ref, Y64, absY, "LDS-resident edge-valued walk", unit)
    assert np.abs(Y.cpu().numpy() - Y1.cpu().numpy()).max() <= TIGHT * (absY.max() + 1.0)


def _lds_val_case(dev, T, monkeypatch, att_fn, x_scale=1.0, prepare=True, seed=31, graph=None, D=64):
    """forward_AGNN forced onto the LDS-resident edge-valued walk (mode 3 of ONE plan, stream built by prepare) -> (Y, kernel, refs)."""
    rp, col = graph if graph is not None else graphs.uniform_graph(3000, 200, seed=seed)
    n, nnz = len(rp) - 1, len(col)
    (bp, e2c, e2r), meta = meta_for(dev, rp, col)
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n, D)) * x_scale).astype(np.float32)
    att = att_fn(rng, nnz).astype(np.float32)
    tX, tatt = to_dev(dev, X, att)
    monkeypatch.setenv("TCGNN_LDS_FLAT", "1")
    T.clear_plan_cache()
    try:
        T.set_plan_modes(*meta, spmm_mode=3)
        if prepare:
            T.prepare([D], *meta, edge_valued=True)
        Y = T.forward_AGNN(tX, meta[0], meta[1], tatt.view(1, -1), *meta[2:])[0].cpu().numpy()
        kernel = T.last_kernel(*meta)
    finally:
        T.clear_plan_cache()
    ref = O.spmm_val(X, rp, col, att, bp, e2c, e2r, round_mode=O.ROUND_TF32)
    Y64, absY = O.spmm_f64(X, rp, col, att)
    return Y, kernel, ref, Y64, absY


@pytest.mark.parametrize("D", [64, 128, 41, 112])   # (41 / 112: a three-plane remainder - one more pair of 32-column chunks, the fourth plane zeros)
@pytest.mark.parametrize("dense_cols", ["1", "5000", None])
def test_edge_valued_lds_walk_with_dense_entries(dev, T, D, dense_cols, monkeypatch, capfd):
    """r05: forward_AGNN on the flat single-edge stream WITH dense entries (a community's own column ranges hold ~20 tiles of edges
    per cell): the values of a dense entry's tiles are brought into stream order by the window slot its descriptor names
    (val_permute_kernel), the walk multiplies them from ordinary-format tiles.  Every overflowing pair dense / only the community
    pairs (the rest in spmm_cold_val_kernel's remainder) / the default rule; N % 16 != 0."""
    monkeypatch.setenv("TCGNN_VERBOSE", "1")
    if dense_cols:
        monkeypatch.setenv("TCGNN_LDS_DENSE_COLS", dense_cols)
    g = graphs.community_graph(6061, 4, 300, 0.5, seed=5)
    Y, kernel, ref, Y64, absY = _lds_val_case(dev, T, monkeypatch, lambda rng, nnz: rng.standard_normal(nnz), graph=g, D=D, seed=33)
    err = capfd.readouterr().err
    assert "spmm_lds_val_kernel" in kernel, (kernel, err[-1500:])
    import re
    dense = [int(x) for x in re.findall(r"entries \((\d+) dense\)", err)]
    assert dense and max(dense) > 0, err[-1500:]
    assert_parity(Y, ref, Y64, absY, "edge-valued walk with dense entries")


def test_lds_val_walk_with_a_maximum_that_rounds_up_to_a_power_of_two(dev, T, monkeypatch):
    """the A fragment used to be 2.0 x value in fp16; a maximum edge value whose mantissa is all ones rounds up to
    2^15 in the scaled image and 2.0 x 32768 is inf - NaN wherever the feature is 0.  Top mantissa all ones, several binades; the
    value is now SELECTED by a mask.  Also the first call after tcgnn_plan_prepare_val takes the LDS-resident walk (VERDICT r04 6 ii)."""
    for k in (-3, 0, 7):
        def att_fn(rng, nnz, k=k):
            a = rng.standard_normal(nnz) * 0.1 * 2.0 ** k
            a[rng.integers(0, nnz, 50)] = np.float32(1.99999) * 2.0 ** k      # rounds (10-bit, ties away) to 2^(k+1)
            a[0] = -np.float32(1.99999) * 2.0 ** k
            return a
        Y, kernel, ref, Y64, absY = _lds_val_case(dev, T, monkeypatch, att_fn)
        assert "spmm_lds_val_kernel" in kernel, kernel
        assert np.isfinite(Y).all(), "inf / NaN at k = %d" % k
        assert_parity(Y, ref, Y64, absY, "max |value| = 1.99999 * 2^%d" % k, False)


def test_lds_val_walk_scales_whose_exponents_add_up_beyond_fp32(dev, T, monkeypatch):
    """kx + ka may reach +-253 - the output scale is two factors, as in the gather walks (both operands tiny /
    both huge; the products themselves stay representable)."""
    for xs, vs in ((2.0 ** -60, 2.0 ** -40), (2.0 ** 40, 2.0 ** 50), (2.0 ** -70, 2.0 ** 70)):
        Y, kernel, ref, Y64, absY = _lds_val_case(dev, T, monkeypatch, lambda rng, nnz, vs=vs: rng.standard_normal(nnz) * vs, x_scale=xs)
        assert "spmm_lds_val_kernel" in kernel, kernel
        scale = float(absY.max())
        assert np.isfinite(Y).all() and scale > 0
        assert np.abs(Y - Y64).max() <= 2.0 ** -9 * scale, (xs, vs)
        assert np.abs(Y - ref).max() <= 1e-4 * scale, (xs, vs)


def test_two_plans_of_one_process_walk_differently(dev, T):
    """VERDICT r04 6 iv: spmm_mode and range_guard per plan (tcgnn_plan_set_spmm_mode / _range_guard); the process-wide setters stay
    the defaults.  Same graph twice (two sets of tensors = two plans): one forced to the per-window gather walk, one to the
    LDS-resident kernel; and one plan with the guard off while the other keeps the default."""
    rp, col = graphs.uniform_graph(4000, 100, seed=41)
    n = len(rp) - 1
    (bp, e2c, e2r), m1 = meta_for(dev, rp, col)
    _, m2 = meta_for(dev, rp, col)
    X = np.random.default_rng(1).standard_normal((n, 64)).astype(np.float32)
    tX = torch.from_numpy(X).to(dev)
    T.clear_plan_cache()
    try:
        T.set_plan_modes(*m1, spmm_mode=1)
        T.set_plan_modes(*m2, spmm_mode=3)
        Y1 = T.forward(tX, *m1)[0]; k1 = T.last_kernel(*m1)
        Y2 = T.forward(tX, *m2)[0]; k2 = T.last_kernel(*m2)
        assert k1 == "spmm_kernel" and k2.startswith("spmm_lds"), (k1, k2)
        ref = O.spmm(X, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32)
        Y64, absY = O.spmm_f64(X, rp, col)
        assert_parity(Y1.cpu().numpy(), ref, Y64, absY, "plan 1")
        assert_parity(Y2.cpu().numpy(), ref, Y64, absY, "plan 2")
        # the guard: a wide matrix (one 3e7 row over 1e-3 data) - plan 1 with the guard off stays on MFMA, plan 2 (default) falls back
        Xw = (np.random.default_rng(2).standard_normal((n, 64)) * 1e-3).astype(np.float32); Xw[5] = 3e7
        tXw = torch.from_numpy(Xw).to(dev)
        T.set_plan_modes(*m1, spmm_mode=-1, range_guard=0)
        T.set_plan_modes(*m2, spmm_mode=-1)
        T.forward(tXw, *m1); w1 = T.range_mode()[0]
        Yw2 = T.forward(tXw, *m2)[0].cpu().numpy(); w2 = T.range_mode()[0]
        assert w1 == 0 and w2 == 1, (w1, w2)
        Yw64, absw = O.spmm_f64(Xw, rp, col)
        has5 = np.zeros(n, bool)
        has5[np.repeat(np.arange(n), np.diff(rp))[col == 5]] = True
        small = np.where(~has5)[0]                                       # rows that do not touch the huge row keep their own accuracy
        assert len(small) > n // 2
        assert (np.abs(Yw2[small] - Yw64[small]) <= 2.0 ** -9 * (absw[small] + 1e-30)).all()
    finally:
        T.clear_plan_cache()


@pytest.mark.parametrize("rot", ["0", "1"])   # (r06: windows in the plan's order / in their own order, rotated per XCD - AgnnArgs::rot, the default on graphs with locality)
@pytest.mark.parametrize("D", [16, 41, 64, 96, 128])   # (128: what the backward pass takes on the Reddit shape since r03; 96: the old row layout)
def test_fused_agnn_xcd_sliced_walk_equals_per_window_walk(dev, T, D, rot, monkeypatch):
    """r03: the XCD-sliced walk of the fused kernel (workgroup b gathers only rows of column slice b % 8, so an XCD's L2 holds the
    slice it is asked for; a wavefront = one window's tiles inside the slice; the slices' addends of Y summed in slice order by
    agnn_slice_sum_kernel).  Automatic for images of 6 - 16 MB, forced here (TCGNN_AGNN_SLICED = 2: eight slices, 16: two rounds
    of eight) on a graph the oracle can handle, N % 16 != 0: same scores bit for bit, same aggregation up to accumulation order,
    same d_w, deterministic."""
    rp, col = graphs.uniform_graph(70003, 80, seed=14)
    n, nnz = len(rp) - 1, len(col)
    (bp, e2c, e2r), (trp, tcol, tbp, te2c, te2r) = meta_for(dev, rp, col)
    meta = (trp, tcol, tbp, te2c, te2r)
    assert T.plan_info(*meta)["column_buckets"] % 16 == 0
    monkeypatch.setenv("TCGNN_AGNN_ROT", rot)
    rng = np.random.default_rng(D + 9)
    H = (rng.standard_normal((n, D)) / np.sqrt(D)).astype(np.float32)
    dY = rng.standard_normal((n, D)).astype(np.float32)
    tH, tdY = to_dev(dev, H, dY)
    tw = torch.tensor([-1.3], device=dev)
    out = {}
    val = rng.standard_normal(nnz).astype(np.float32)
    tval = to_dev(dev, val)[0].view(1, -1).contiguous()
    yv = {}
    for sl in ("0", "2", "16"):
        monkeypatch.setenv("TCGNN_AGNN_SLICED", sl)
        # the edge-valued SpMM takes the sliced walk too where the fused backward pass does (wider than 32 columns): the fused
        # kernel with its score half switched off
        yv[sl] = T.forward_AGNN(tH, trp, tcol, tval, tbp, te2c, te2r)[0].cpu().numpy()
        assert ("values only" in T.last_kernel(*meta)) == (sl != "0" and D > 32), (sl, D, T.last_kernel(*meta))
        Y, ef, efmax = T.agnn_fused_forward(tH, trp, tcol, tw, tbp, te2c, te2r)
        kf = T.last_kernel(*meta)
        G, dw = T.agnn_fused_backward(tdY, trp, tcol, tw, ef, efmax, tbp, te2c, te2r)
        G2, dw2 = T.agnn_fused_backward(tdY, trp, tcol, tw, ef, efmax, tbp, te2c, te2r)
        assert torch.equal(G, G2) and torch.equal(dw, dw2)
        assert ("XCD-sliced" in kf) == (sl != "0") and ("XCD-sliced" in T.last_kernel(*meta)) == (sl != "0"), (sl, kf)
        out[sl] = (Y.cpu().numpy(), ef.cpu().numpy(), efmax[0].item(), G.cpu().numpy(), float(dw))
    att = (np.float32(-1.3) * out["0"][1]).astype(np.float32)
    Y64, absY = O.spmm_f64(H, rp, col, att)
    G64, absG = O.spmm_f64(dY, rp, col, att)
    refY = O.spmm_val(H, rp, col, att, bp, e2c, e2r, round_mode=O.ROUND_TF32)
    refG = O.spmm_val(dY, rp, col, att, bp, e2c, e2r, round_mode=O.ROUND_TF32)
    d_att = O.sddmm(dY, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32).astype(np.float64)
    want = float((d_att * col).sum()); term_scale = float((np.abs(d_att) * col).sum()) + 1.0
    V64, absV = O.spmm_f64(H, rp, col, val)
    refV = O.spmm_val(H, rp, col, val, bp, e2c, e2r, round_mode=O.ROUND_TF32)
    for sl in ("0", "2", "16"):
        assert_parity(yv[sl], refV, V64, absV, "forward_AGNN sliced %s" % sl)
        assert np.abs(yv[sl] - yv["0"]).max() <= TIGHT * (absV.max() + 1.0)
    for sl in ("2", "16"):
        Y, ef, efm, G, dw = out[sl]
        assert np.array_equal(ef, out["0"][1]) and efm == out["0"][2]
        assert_parity(Y, refY, Y64, absY, "Y sliced %s" % sl)
        assert_parity(G, refG, G64, absG, "G sliced %s" % sl)
        assert np.abs(Y - out["0"][0]).max() <= TIGHT * (absY.max() + 1.0) and np.abs(G - out["0"][3]).max() <= TIGHT * (absG.max() + 1.0)
        assert abs(dw - want) <= 1e-6 * term_scale, (dw, want, term_scale)


@pytest.mark.parametrize("D", [16, 48, 64, 96, 128])
def test_lds_resident_walk_with_a_cold_remainder(dev, T, D, monkeypatch):
    """A graph with communities: the (workgroup, column range) pairs that hold few of a workgroup's columns are left out of the
    LDS-resident cell stream and go, re-condensed, to the gather walk, which ADDS its part to what the LDS-resident kernel
    stored.  Forced here (mode 3 + a threshold that splits this small graph): hot and cold parts both non-empty, several
    workgroups with different range lists, ReLU applied once on the sum, the gated staging on both images; against the
    oracle and the per-window gather walk."""
    import tcgnn_capi as c
    rng = np.random.default_rng(77)
    n, blocks = 6144, 6
    size = n // blocks
    src_in = rng.integers(0, n, size=380000); dst_in = (src_in // size) * size + rng.integers(0, size, size=380000)
    src_out = rng.integers(0, n, size=30000); dst_out = rng.integers(0, n, size=30000)
    src = np.concatenate([src_in, src_out]); dst = np.concatenate([dst_in, dst_out])
    rp, col = graphs.csr_from_edges(np.concatenate([src, dst]), np.concatenate([dst, src]), n)
    (bp, e2c, e2r), meta = meta_for(dev, rp, col)
    X = rng.standard_normal((n, D)).astype(np.float32)
    (tX,) = to_dev(dev, X)
    monkeypatch.setenv("TCGNN_LDS_HOT_COLS", "600")
    T.clear_plan_cache()
    try:
        c.check(c.lib.tcgnn_set_spmm_mode(3), "tcgnn_set_spmm_mode")
        Y = T.forward(tX, *meta)[0]
        kernel = T.last_kernel(*meta)
        Yr = T.forward_fused(tX, *meta, relu=True)[0]
        Yg = T.forward_fused(tX, *meta, gate=Y)[0]
        again = T.forward(tX, *meta)[0]
        c.check(c.lib.tcgnn_set_spmm_mode(1), "tcgnn_set_spmm_mode")
        Y1 = T.forward(tX, *meta)[0]
        Yg1 = T.forward_fused(tX, *meta, gate=Y)[0]
    finally:
        c.lib.tcgnn_set_spmm_mode(0)
        monkeypatch.delenv("TCGNN_LDS_HOT_COLS")
        T.clear_plan_cache()
    if D in (16, 48, 64, 128):                      # one cell stream serves every pass: the split path
        assert kernel == "spmm_lds_kernel + spmm_kernel (cold remainder)", kernel
    else:                                           # 64 + 32 columns use two streams: the call takes the gather walk
        assert kernel in ("spmm_kernel", "spmm_blocked_kernel"), kernel
    assert torch.equal(Y, again)
    Y64, absY = O.spmm_f64(X, rp, col)
    ref = O.spmm(X, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32)
    assert_parity(Y.cpu().numpy(), ref, Y64, absY, "spmm hot + cold")
    assert_parity(Y1.cpu().numpy(), ref, Y64, absY, "spmm gather")
    assert torch.equal(Yr, torch.relu(Y))
    assert ((Yg - Yg1).abs() / (torch.from_numpy(absY).to(dev) + 1.0)).max().item() <= TIGHT


@pytest.mark.parametrize("maxw", ["4", "8"])
def test_lds_resident_range_kernel_with_one_layout_forced(maxw):
    """By default whole 64-column chunks run in the 8-windows-per-wavefront layout and the 1-3 planes left over in the
    4-window one.  TCGNN_LDS_MAXW forces one layout for every pass (4: 64 columns per pass incl. the 4-plane kernel;
    8: 32 columns per pass incl. the 1-plane kernel); it is read when the library loads, so the parity test above is
    re-run in a child process with the variable set."""
    env = dict(os.environ, TCGNN_LDS_MAXW=maxw)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "test_lds_resident_range_kernel_matches_oracle_and_plain_walk and (64 or 41 or 160)"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout


@pytest.mark.parametrize("D", [16, 64, 41, 128])
def test_fused_agnn_range_major_walk_equals_per_window_walk(dev, T, D):
    """The persistent range-major variant of the fused kernel (picked automatically for big feature matrices) forced on
    a graph the oracle can handle: same scores bit for bit, same aggregation up to accumulation order, same d_w."""
    import tcgnn_capi as c
    rp, col = graphs.uniform_graph(16448, 180, seed=12)
    n, nnz = len(rp) - 1, len(col)
    (bp, e2c, e2r), (trp, tcol, tbp, te2c, te2r) = meta_for(dev, rp, col)
    meta = (trp, tcol, tbp, te2c, te2r)
    assert T.plan_info(*meta)["column_buckets"] > 0
    rng = np.random.default_rng(D + 5)
    H = (rng.standard_normal((n, D)) / np.sqrt(D)).astype(np.float32)
    dY = rng.standard_normal((n, D)).astype(np.float32)
    tH, tdY = to_dev(dev, H, dY)
    tw = torch.tensor([1.7], device=dev)
    out = {}
    try:
        for mode in (1, 2):
            c.check(c.lib.tcgnn_set_spmm_mode(mode), "tcgnn_set_spmm_mode")
            Y, ef, efmax = T.agnn_fused_forward(tH, trp, tcol, tw, tbp, te2c, te2r)
            G, dw = T.agnn_fused_backward(tdY, trp, tcol, tw, ef, efmax, tbp, te2c, te2r)
            out[mode] = (Y.cpu().numpy(), ef.cpu().numpy(), efmax[0].item(), G.cpu().numpy(), float(dw))
    finally:
        c.lib.tcgnn_set_spmm_mode(0)
    ef_ref = O.sddmm(H, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32)
    att = (np.float32(1.7) * out[1][1]).astype(np.float32)
    Y64, absY = O.spmm_f64(H, rp, col, att)
    G64, absG = O.spmm_f64(dY, rp, col, att)
    refY = O.spmm_val(H, rp, col, att, bp, e2c, e2r, round_mode=O.ROUND_TF32)
    refG = O.spmm_val(dY, rp, col, att, bp, e2c, e2r, round_mode=O.ROUND_TF32)
    d_att = O.sddmm(dY, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32).astype(np.float64)
    want = float((d_att * col).sum()); term_scale = float((np.abs(d_att) * col).sum()) + 1.0
    assert np.array_equal(out[1][1], out[2][1]) and out[1][2] == out[2][2]
    for mode in (1, 2):
        Y, ef, _, G, dw = out[mode]
        ef64, absef = O.sddmm_f64(H, rp, col)
        assert_parity(ef, ef_ref, ef64, absef, "scores mode %d" % mode)
        assert_parity(Y, refY, Y64, absY, "Y mode %d" % mode)
        assert_parity(G, refG, G64, absG, "G mode %d" % mode)
        assert abs(dw - want) <= 1e-6 * term_scale


def test_fused_agnn_refuses_what_it_does_not_cover(dev, T):
    import tcgnn_capi as c
    rp, col = graphs.uniform_graph(300, 6, seed=3)
    _, meta = meta_for(dev, rp, col)
    x = torch.randn(300, 160, device=dev)
    assert not T.agnn_fused_supported(x, *meta)
    with pytest.raises(RuntimeError, match="not supported"):
        T.agnn_fused_forward(x, meta[0], meta[1], torch.ones(1, device=dev), *meta[2:])
    assert c.lib.tcgnn_status_string(6) == b"not supported by the fused entry point"
    with pytest.raises(RuntimeError, match="one value"):
        T.agnn_fused_forward(x[:, :16].contiguous(), meta[0], meta[1], torch.ones(2, device=dev), *meta[2:])


def test_agnn_layer_gives_the_same_gradients_fused_and_separate(dev, T):
    import tcgnn_layers as L
    L.set_backend(T)
    rp, col = graphs.powerlaw_graph(2000, 30, seed=21)
    _, meta = meta_for(dev, rp, col)
    torch.manual_seed(4)
    X = torch.randn(2000, 50, device=dev)
    W0 = torch.randn(50, 32, device=dev) / 7.0
    a0 = torch.tensor([[0.8]], device=dev)
    dY = torch.randn(2000, 32, device=dev)
    res = {}
    for fused in (True, False):
        L.USE_FUSED_AGNN = fused
        try:
            x, w, a = X.clone().requires_grad_(True), W0.clone().requires_grad_(True), a0.clone().requires_grad_(True)
            y = L.TCGNNFunction_AGNN.apply(x, w, a, *meta)
            y.backward(dY)
            res[fused] = (y.detach(), x.grad, w.grad, a.grad)
        finally:
            L.USE_FUSED_AGNN = True
    for got, want, what in zip(res[True], res[False], ("Y", "dX", "dW", "d_attention_w")):
        scale = float(want.abs().max()) + 1.0
        tol = 2e-5 if what != "d_attention_w" else 2e-4
        assert got.shape == want.shape and float((got - want).abs().max()) <= tol * scale, what


@pytest.mark.parametrize("D", [16, 41, 64, 100])
def test_fused_relu_epilogue_and_gated_staging_are_bit_identical_to_the_unfused_steps(dev, T, D):
    """forward_fused(relu=True) == relu(forward(X)) and forward_fused(gate=G) == forward(X * (G > 0)),
    exactly, on every SpMM walk (per-window fp16, range-blocked, LDS-resident ranges, single-launch fp32)."""
    import tcgnn_capi as c
    rp, col = graphs.uniform_graph(16448, 40, seed=31)
    _, (trp, tcol, tbp, te2c, te2r) = meta_for(dev, rp, col)
    meta = (trp, tcol, tbp, te2c, te2r)
    n = len(rp) - 1
    g = torch.Generator(device=dev).manual_seed(D)
    X = torch.randn(n, D, device=dev, generator=g)
    G = torch.randn(n, D, device=dev, generator=g)
    try:
        for mode in (1, 2, 3, 4):
            c.check(c.lib.tcgnn_set_spmm_mode(mode), "tcgnn_set_spmm_mode")
            assert torch.equal(T.forward_fused(X, *meta, relu=True)[0], torch.relu(T.forward(X, *meta)[0])), mode
            assert torch.equal(T.forward_fused(X, *meta, gate=G)[0], T.forward(X * (G > 0), *meta)[0]), mode
    finally:
        c.lib.tcgnn_set_spmm_mode(0)


def test_gcn_layer_with_fused_relu_gives_the_same_values_and_gradients(dev, T):
    import tcgnn_layers as L
    rp, col = graphs.uniform_graph(3000, 30, seed=32)
    _, (trp, tcol, tbp, te2c, te2r) = meta_for(dev, rp, col)
    meta = (trp, tcol, tbp, te2c, te2r)
    torch.manual_seed(5)
    conv = L.GCNConv(24, 16).to(dev)
    x0 = torch.randn(3000, 24, device=dev)
    dy = torch.randn(3000, 16, device=dev)
    outs = []
    for fused in (False, True):
        x = x0.clone().requires_grad_(True)
        conv.weights.grad = None
        y = conv(x, *meta, fuse_relu=True) if fused else torch.relu(conv(x, *meta))
        y.backward(dy)
        outs.append((y.detach(), x.grad.clone(), conv.weights.grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("D", [64, 41])
def test_sharded_spmm_with_fp16_on_the_wire_equals_the_fp32_gather(dev, T, D):
    """tcgnn_stage_absmax / tcgnn_stage_rows / tcgnn_spmm_staged (the pre-staged image a rank would all-gather instead of
    fp32 X) against the ordinary path on one rank's shard: same kernel, same operands, identical results."""
    import tcgnn_capi as c
    import tcgnn_shard as S
    rp, col = graphs.uniform_graph(5000, 60, seed=41)
    n = len(rp) - 1
    shard = S.RowShard(rp, col, rank=0, world_size=1, device=dev)
    rng = np.random.default_rng(D)
    X = rng.standard_normal((n, D)).astype(np.float32) * 37.0
    (tX,) = to_dev(dev, X)
    try:
        for mode in (1, 2):
            c.check(c.lib.tcgnn_set_spmm_mode(mode), "tcgnn_set_spmm_mode")
            a = shard.spmm(tX)
            b = shard.spmm(tX, wire="fp16")
            assert torch.equal(a, b), mode
    finally:
        c.lib.tcgnn_set_spmm_mode(0)
    bp, e2c, e2r = (t.cpu().numpy() for t in shard.ops.meta[2:])
    Y64, absY = O.spmm_f64(X, rp, col)
    assert_parity(b.cpu().numpy(), O.spmm(X, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32), Y64, absY, "staged spmm", False)
    shard.ops.close()


def test_epoch_captured_in_a_hip_graph_trains_like_the_eager_loop(dev, T):
    """tcgnn_harness.time_training(hip_graph=True) captures forward + loss + backward + Adam step once and replays it: every
    kernel of the path must be capturable (no allocation outside torch's pool, no synchronisation, current-stream launches)
    and the replayed epochs must keep training (labels are all ones: the loss falls as in the eager loop)."""
    import tcgnn_harness as H
    rp, col = graphs.uniform_graph(3327, 2.8, seed=1)
    _, (trp, tcol, tbp, te2c, te2r) = meta_for(dev, rp, col)
    meta = (trp, tcol, tbp, te2c, te2r)
    n = len(rp) - 1
    x = torch.randn(n, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    y = torch.ones(n, dtype=torch.long, device=dev)
    for model in ("gcn", "agnn"):
        short = H.time_training(model, meta, x, y, 32, 16, 6, 2, epochs=1, seed=0, warmup=2, hip_graph=True)
        long_g = H.time_training(model, meta, x, y, 32, 16, 6, 2, epochs=40, seed=0, warmup=2, hip_graph=True)
        long_e = H.time_training(model, meta, x, y, 32, 16, 6, 2, epochs=44, seed=0, warmup=2, hip_graph=False)
        assert long_g.get("hip_graph") and np.isfinite(long_g["final_loss"]) and np.isfinite(long_e["final_loss"])
        assert long_g["final_loss"] < short["final_loss"], (model, short, long_g)
        # same number of optimiser steps; dropout draws differ between the two loops, so the bar is loose
        assert abs(long_g["final_loss"] - long_e["final_loss"]) <= 0.5 * max(long_e["final_loss"], short["final_loss"]), (model, long_g, long_e)


@pytest.mark.parametrize("hip_graph", [False, True])
def test_training_on_the_slice_synchronised_walk_follows_the_per_window_walk(dev, T, hip_graph):
    """r06: whole GCN and AGNN epochs (hidden 128: forward, forward_AGNN / the fused pair and their backward passes, autograd, Adam) with
    every aggregation on the slice-synchronised walk (mode 5: one launch per slice round, several launches per operator call) against
    the same epochs on the per-window walk - eager, and captured once in a HIP graph and replayed (every launch of a call must be
    capturable).  Both runs seed torch alike, so they draw the same dropout masks; the bar is loose all the same: summation orders
    differ between the walks."""
    import tcgnn_capi as c
    import tcgnn_harness as H
    rp, col = graphs.community_graph(40003, 16, 60, 0.9, seed=31)
    _, (trp, tcol, tbp, te2c, te2r) = meta_for(dev, rp, col)
    meta = (trp, tcol, tbp, te2c, te2r)
    n = len(rp) - 1
    x = torch.randn(n, 48, device=dev, generator=torch.Generator(device=dev).manual_seed(0)) * 0.1
    y = torch.ones(n, dtype=torch.long, device=dev)
    out = {}
    try:
        for mode in (1, 5):
            c.check(c.lib.tcgnn_set_spmm_mode(mode), "tcgnn_set_spmm_mode")
            T.clear_plan_cache()
            for model in ("gcn", "agnn"):
                torch.manual_seed(7)
                out[(mode, model)] = H.time_training(model, meta, x, y, 48, 128, 7, 2, epochs=6, seed=0, warmup=2, hip_graph=hip_graph)
            T.forward(torch.randn(n, 128, device=dev), *meta)
            assert (T.last_kernel(*meta) == "spmm_sync_kernel") == (mode == 5)
    finally:
        c.lib.tcgnn_set_spmm_mode(0)
        T.clear_plan_cache()
    for model in ("gcn", "agnn"):
        a, b = out[(1, model)]["final_loss"], out[(5, model)]["final_loss"]
        assert np.isfinite(a) and np.isfinite(b), (model, a, b)
        assert abs(a - b) <= 0.05 * max(abs(a), 1e-3) + 1e-4, (model, a, b)


@pytest.mark.parametrize("shape", [(40000, 64, 41), (70001, 96, 16), (33000, 602, 64), (40000, 16, 64)])
def test_tall_dense_updates_match_a_float64_product(dev, shape):
    """The layers' tall products (tcgnn_layers.tall_mm / tall_nt_mm / tall_tn_mm) against float64: fp32 GEMM accuracy, 1e-5 of
    the row-times-column norm bound - with the default candidates (no tune() call: nothing is measured inside a product, the
    table stays empty) and with whatever an explicit tune() picks for the shape; the library preference a candidate may switch
    for its call is restored afterwards, and a second call returns the same bits."""
    import tcgnn_layers as L
    n, k, m = shape
    g = torch.Generator(device=dev).manual_seed(n + k)
    A = torch.randn(n, k, device=dev, generator=g); W = torch.randn(k, m, device=dev, generator=g); G = torch.randn(n, m, device=dev, generator=g)
    before = torch.backends.cuda.preferred_blas_library()
    saved = dict(L._tuned); L._tuned.clear()
    got0 = {"A W": L.tall_mm(A, W), "G W^T": L.tall_nt_mm(G, W), "A^T G": L.tall_tn_mm(A, G)}
    assert not L._tuned                                                      # a product call decides nothing
    rep = L.tune([("mm", n, k, m), ("nt", n, m, k), ("tn", n, k, m)], device=dev)
    assert len(rep) == 3 and all(0 <= w < len(L._CANDIDATES[key[0]]) and len(t) == len(L._CANDIDATES[key[0]]) for key, (w, t) in rep.items())
    got = {"A W": L.tall_mm(A, W), "G W^T": L.tall_nt_mm(G, W), "A^T G": L.tall_tn_mm(A, G)}
    assert torch.backends.cuda.preferred_blas_library() == before
    assert torch.equal(got["A W"], L.tall_mm(A, W)) and torch.equal(got["A^T G"], L.tall_tn_mm(A, G))   # the choice is kept
    L._tuned.clear(); L._tuned.update(saved)
    want = {"A W": A.double() @ W.double(), "G W^T": G.double() @ W.double().t(), "A^T G": A.double().t() @ G.double()}
    bound = {"A W": A.double().norm(dim=1)[:, None] * W.double().norm(dim=0)[None, :],
             "G W^T": G.double().norm(dim=1)[:, None] * W.double().norm(dim=1)[None, :],
             "A^T G": A.double().norm(dim=0)[:, None] * G.double().norm(dim=0)[None, :]}
    for name in got:
        for res in (got, got0):
            err = ((res[name].double() - want[name]).abs() / bound[name]).max().item()
            assert err < 1e-5, (name, shape, err)


def test_first_call_of_a_width_inside_a_graph_capture_takes_a_gather_walk(dev, T):
    """A width whose cell stream does not exist yet cannot have it built while the stream is being captured (the build
    allocates and synchronises): the captured call runs a gather walk and leaves the plan as it was, the next eager call
    builds the stream, and both give the sums of the per-window walk.  (N = 60 k / 20 M edges: the LDS-resident kernel is
    the automatic choice at 16 columns, and plan creation only builds what a 64-column matrix needs.)"""
    import tcgnn_capi as c
    import tcgnn_graph as G
    if os.environ.get("TCGNN_SPMM_MODE", "0") == "3":
        pytest.skip("with the LDS-resident walk forced, capturing an unbuilt width is an error by design")
    n = 60000
    rp, col = G.synthetic_csr(n, 20_000_000, seed=5, device=dev)
    E = col.numel(); nw = (n + 15) // 16
    bp = torch.zeros(nw, dtype=torch.int32, device=dev); e2c = torch.zeros(E, dtype=torch.int32, device=dev); e2r = torch.zeros(E, dtype=torch.int32, device=dev)
    T.preprocess_gpu(col, rp, n, 16, 8, bp, e2c, e2r)
    meta = (rp, col, bp, e2c, e2r)
    X = torch.randn(n, 16, device=dev)
    bytes_created = T.plan_info(*meta)["plan_bytes"]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        Yw = T.forward(torch.randn(n, 64, device=dev), *meta)[0]   # warms torch's allocator on the capture stream (another width)
        bytes_before = T.plan_info(*meta)["plan_bytes"]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            Yg = T.forward(X, *meta)[0]
    torch.cuda.current_stream().wait_stream(side)
    g.replay(); torch.cuda.synchronize()
    assert T.plan_info(*meta)["plan_bytes"] == bytes_before >= bytes_created      # nothing was built under capture
    Ye = T.forward(X, *meta)[0]
    if os.environ.get("TCGNN_LDS_AUTO", "1") != "0" and os.environ.get("TCGNN_SPMM_MODE", "0") == "0" and not os.environ.get("TCGNN_LDS_MAXW"):
        assert T.plan_info(*meta)["plan_bytes"] > bytes_before                    # the eager call built the 16-column stream
    c.check(c.lib.tcgnn_set_spmm_mode(1), "mode")
    try:
        Y1 = T.forward(X, *meta)[0]
    finally:
        c.lib.tcgnn_set_spmm_mode(0)
    scale = float(X.abs().max()) * float((rp[1:] - rp[:-1]).max()) ** 0.5
    assert float((Yg - Y1).abs().max()) < 1e-4 * scale and float((Ye - Y1).abs().max()) < 1e-4 * scale
    del Yw


def test_automatic_walk_follows_the_time_models(dev, T):
    """The automatic mode picks the LDS-resident kernel per plan and width from its time models (DESIGN.md "Which walk
    runs"): a 60 k-node graph with 20 M edges takes it at 64 columns (cell stream built at plan creation); the Reddit node
    count at 15 M edges does not, at either width (its cells run empty: the range walk costs more than gathering 15 M rows)."""
    import tcgnn_graph as G
    if os.environ.get("TCGNN_LDS_AUTO", "1") == "0" or os.environ.get("TCGNN_SPMM_MODE", "0") != "0" or os.environ.get("TCGNN_LDS_MAXW"):
        pytest.skip("the automatic choice is overridden by the environment")
    for n, nnz, expect_lds in ((60000, 20_000_000, True), (232965, 15_000_000, False)):
        rp, col = G.synthetic_csr(n, nnz, seed=9, device=dev)
        E = col.numel(); nw = (n + 15) // 16
        bp = torch.zeros(nw, dtype=torch.int32, device=dev); e2c = torch.zeros(E, dtype=torch.int32, device=dev); e2r = torch.zeros(E, dtype=torch.int32, device=dev)
        T.preprocess_gpu(col, rp, n, 16, 8, bp, e2c, e2r)
        meta = (rp, col, bp, e2c, e2r)
        deg = (rp[1:] - rp[:-1]).float()
        for D in (64, 16):
            Y = T.forward(torch.ones(n, D, device=dev), *meta)[0]
            assert torch.equal(Y, deg[:, None].expand(-1, D))
        assert (T.plan_info(*meta)["lds_ranges"] > 0) == expect_lds, (n, nnz, T.plan_info(*meta))
        del rp, col, bp, e2c, e2r, meta, Y
        torch.cuda.empty_cache()


def test_range_robustness_beyond_fp16(dev, T):
    """Values far outside fp16's range (the reference's TF32 has fp32's exponent) survive the
    per-call power-of-two scaling."""
    rp, col = graphs.uniform_graph(400, 8, seed=6)
    (bp, e2c, e2r), (trp, tcol, tbp, te2c, te2r) = meta_for(dev, rp, col)
    rng = np.random.default_rng(6)
    for mag in (1e-20, 1e-6, 1e6, 1e18):
        X = (rng.standard_normal((400, 32)) * mag).astype(np.float32)
        att = (rng.standard_normal(len(col)) * mag).astype(np.float32)
        tX, tatt = to_dev(dev, X, att)
        Y = T.forward(tX, trp, tcol, tbp, te2c, te2r)[0].cpu().numpy()
        R = O.spmm(X, rp, col, bp, e2c, e2r)
        assert np.isfinite(Y).all() and np.abs(Y - R).max() <= 1e-5 * np.abs(R).max()
        ef = T.forward_ef(tX, trp, tcol, tbp, te2c, te2r)[0].cpu().numpy()
        Re = O.sddmm(X, rp, col, bp, e2c, e2r)
        assert np.isfinite(ef).all() and np.abs(ef - Re).max() <= 1e-5 * np.abs(Re).max()
        if mag < 1e10:
            Yv = T.forward_AGNN(tX, trp, tcol, tatt.view(1, -1), tbp, te2c, te2r)[0].cpu().numpy()
            Rv = O.spmm_val(X, rp, col, att, bp, e2c, e2r)
            assert np.isfinite(Yv).all() and np.abs(Yv - Rv).max() <= 1e-5 * np.abs(Rv).max()
    Z = T.forward(torch.zeros(400, 32, device=dev), trp, tcol, tbp, te2c, te2r)[0]
    assert not Z.any()


@pytest.mark.parametrize("flat", [0, 1])
def test_lds_resident_kernels_are_their_own_range_guard_fallback(dev, T, flat, monkeypatch):
    """r04: behind the LDS-resident binary SpMM the guard's fp32 fallback used to be a launch of its own - a gate that returns at once
    and costs 4.5 us of every aggregation.  spmm_lds_kernel / spmm_lds_flat_kernel now run that walk themselves when the staged
    matrix is wide (lds_own_fallback): forced here (mode 3; the flat stream on a small graph by TCGNN_LDS_FLAT), a 3e7 row over
    1e-3 data, N % 16 != 0, D = 64 (one launch) and 80 (two passes: the fallback stays a launch of its own), with a ReLU; against
    the oracle.  The same call on ordinary data stays on the MFMA kernel."""
    import tcgnn_capi as c
    rp, col = graphs.uniform_graph(4109, 100, seed=31)
    (bp, e2c, e2r), meta = meta_for(dev, rp, col)
    n = len(rp) - 1
    rng = np.random.default_rng(3 + flat)
    monkeypatch.setenv("TCGNN_LDS_FLAT", str(flat))
    T.clear_plan_cache()
    try:
        c.check(c.lib.tcgnn_set_spmm_mode(3), "tcgnn_set_spmm_mode")
        for D in (64, 80):
            for wide in (True, False):
                X = (rng.standard_normal((n, D)) * (1e-3 if wide else 1.0)).astype(np.float32)
                if wide:
                    X[777] = 3e7 * (1.0 + rng.random(D).astype(np.float32))
                Y = T.forward(torch.from_numpy(X).to(dev), *meta)[0].cpu().numpy()
                kernel = T.last_kernel(*meta)
                assert kernel.startswith("spmm_lds_flat_kernel" if flat else "spmm_lds_kernel"), kernel
                assert T.range_mode()[0] == (1 if wide else 0)
                ref = O.spmm(X, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32)
                r64, a64 = O.spmm_f64(X, rp, col)
                assert_parity(Y, ref, r64, a64, "D=%d wide=%s flat=%d" % (D, wide, flat), unit_scale=not wide)
                if wide:   # rows that never touch the outlier are what the fp16 image loses: they must be there, to accumulation accuracy
                    small = a64.max(axis=1) < 1.0
                    assert small.sum() > n // 2 and np.abs(Y[small] - r64[small]).max() <= 2.0 ** -9 * a64[small].max() and np.abs(Y[small]).max() > 0
    finally:
        c.lib.tcgnn_set_spmm_mode(0)
        T.clear_plan_cache()


def test_wide_range_inside_one_matrix_takes_the_fp32_fallback(dev, T):
    try:
        _wide_range_body(dev, T)
    finally:
        T.set_range_guard(2)      # the default level (r04), whatever happened
        T.clear_plan_cache()


@pytest.mark.parametrize("specks", [1, 5, 12, 300, -40, 1007, 1200])   # (300: far beyond r04's list of 48 rows; -40: 40 rows on a graph with hub rows, the hubs among them; 1007: 7 rows on a DIRECTED graph; 1200: 200 rows, symmetric)
def test_a_few_lost_elements_are_patched_behind_the_mfma_kernels(dev, T, specks):
    """r04: the default guard level covers SDDMM and the fused AGNN pair.  What training produces is a matrix
    of 1e4-sized activations with ONE element 2^28 below the maximum (tools/probe_training_ranges.py): the quadratic bound makes it
    "wide", and until r04 such a call either kept the documented bound (default) or spent ~25 ms in the CSR fallbacks (level 2).
    Now the MFMA kernels run and wide_patch_kernel recomputes the edges that touch the few dirty rows in fp32: range_mode says 2,
    the scores of exactly those edges come out to accumulation accuracy of their own terms (the fp16 image alone misses by orders
    of magnitude there), everything else is untouched, aggregate and d_w follow."""
    # r05: ANY number of dirty rows - the conversion pass marks them in a bitmap, the patch scans the edges and
    # recomputes every edge that touches one, a wavefront per edge; hub rows (thousands of edges each) are no special case.
    assert T.range_mode is not None
    T.set_range_guard(2)
    # r05, late: up to 256 dirty rows of a structurally SYMMETRIC square graph are patched row-driven (a dirty row's own edges + their mirrors by
    # binary search) instead of by the scan over every column id: 1 / 5 / 12 / 200 rows take that way, 300 rows and the directed graph the scan
    hubs = specks < 0
    directed = specks == 1007
    specks = abs(specks) % 1000
    rp, col = graphs.hub_rows_graph(2500, seed=77) if hubs else graphs.uniform_graph(4000, 100, seed=5, symmetric=not directed)
    if directed:
        import scipy.sparse as sp
        a_ = sp.csr_matrix((np.ones(len(col), np.int8), col, rp), shape=(len(rp) - 1, len(rp) - 1))
        assert (a_ != a_.T).nnz > 0
    (bp, e2c, e2r), meta = meta_for(dev, rp, col)
    n, D = len(rp) - 1, 64
    rng = np.random.default_rng(100 + specks)
    X = (rng.standard_normal((n, D)) * 1e4).astype(np.float32)
    X[np.abs(X) < 1.0] = 1.0
    rows = rng.choice(n, size=specks, replace=False)
    if hubs:
        rows[:8] = np.arange(8)                       # eight of the rows that are edges to every column
    for r in rows:
        X[r, rng.integers(0, D, size=3)] = 3e-5 * (1.0 + rng.random(3))       # ~2^30 below the maximum: fp16 subnormals lose most of their bits
    tX = torch.from_numpy(X).to(dev)
    ef = T.forward_ef(tX, *meta)[0].cpu().numpy()
    assert T.range_mode()[0] == 2
    refe = O.sddmm(X, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32); _, ae64 = O.sddmm_f64(X, rp, col)
    assert (np.abs(ef - refe) / (ae64 + 1e-30)).max() <= 4 * TIGHT
    # sensitivity: the lost elements' own products are visible at this accuracy (each is ~3e-5 x 1e4 = 0.3 against sums of ~1e9 x 4e-6)
    erow = np.repeat(np.arange(n), np.diff(rp))
    touched = np.isin(erow, rows) | np.isin(col, rows)
    assert touched.sum() >= specks * (20 if hubs else 100)
    w = np.float32(0.75)
    tw = torch.tensor([w], device=dev)
    Yf, ef_f, efm = T.agnn_fused_forward(tX, meta[0], meta[1], tw, *meta[2:])
    assert T.range_mode()[0] == 2
    ef_fh = ef_f.cpu().numpy()
    assert (np.abs(ef_fh - refe) / (ae64 + 1e-30)).max() <= 4 * TIGHT
    assert int(efm[0].item()) == int(np.abs(ef_fh).max().view(np.int32))
    att_ref = (w * ef_fh).astype(np.float32)
    refY = O.spmm_val(X, rp, col, att_ref, bp, e2c, e2r, round_mode=O.ROUND_TF32); _, aY = O.spmm_f64(X, rp, col, att_ref)
    assert (np.abs(Yf.cpu().numpy() - refY) / (aY + 1e-30)).max() <= 256 * TIGHT
    dY = (rng.standard_normal((n, D)) * 1e4).astype(np.float32)
    dY[np.abs(dY) < 1.0] = 1.0
    for r in rows:
        dY[r, rng.integers(0, D, size=2)] = 3e-5
    tdY = torch.from_numpy(dY).to(dev)
    G, dw = T.agnn_fused_backward(tdY, meta[0], meta[1], tw, ef_f, efm, *meta[2:])
    assert T.range_mode()[0] == 2
    refG = O.spmm_val(dY, rp, col, att_ref, bp, e2c, e2r, round_mode=O.ROUND_TF32); _, aG = O.spmm_f64(dY, rp, col, att_ref)
    assert (np.abs(G.cpu().numpy() - refG) / (aG + 1e-30)).max() <= 256 * TIGHT
    d_att = O.sddmm(dY, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32); _, ad = O.sddmm_f64(dY, rp, col)
    want_dw = float((d_att.astype(np.float64) * col.astype(np.float64)).sum())
    assert abs(float(dw) - want_dw) <= 1e-5 * (float((ad * col).sum()) + 1.0), (float(dw), want_dw)
    # with the guard at level 1 the same call stays on the MFMA path alone and misses the touched edges by far more than that
    T.set_range_guard(1)
    try:
        ef1 = T.forward_ef(tX, *meta)[0].cpu().numpy()
        assert T.range_mode()[0] == 0
        # (the lost elements' own products - 3e-5 x 1e4 against sums of |terms| ~ 6e9 - are far below accumulation noise here: what
        #  makes the matrix "wide" is the worst case over all cancellations, which the patch removes by construction)
        assert not np.array_equal(ef1[touched], ef[touched])                # the patch recomputed the touched edges (another summation order) ...
        assert np.array_equal(ef1[~touched], ef[~touched])                  # ... and nothing else
    finally:
        T.set_range_guard(2)
        T.clear_plan_cache()


@pytest.mark.parametrize("graph", ["uniform", "powerlaw", "hub_rows", "rmat"])
def test_agnn_training_with_the_reference_recipe_stays_inside_the_bar(dev, T, graph):
    """20 AGNN epochs with the reference's UNSCALED randn feature weights (gnn_conv.py:195 style activations of 1e4 and more) on a
    graph the oracle can follow: at the default guard level every fused forward call's scores and aggregate stay within
    1e-3 max(1, |ref|) of an fp64 evaluation of the definition on the TF32-rounded operands, whichever way the guard sent the call.
    r05: also on a power-law graph, on one with rows that are edges to every column, and on the R-MAT generator at
    scale 0.05 - hub rows under unscaled weights are what r04's 48-row patch left to the documented bound."""
    import tcgnn_harness as H
    import tcgnn_layers as L
    if graph == "uniform":
        rp, col = graphs.uniform_graph(3000, 30, seed=8)
    elif graph == "powerlaw":
        rp, col = graphs.powerlaw_graph(3000, 30, seed=8)
    elif graph == "hub_rows":
        rp, col = graphs.hub_rows_graph(2500, seed=77)
    else:
        import tcgnn_graph as G
        trp, tcol_ = G.rmat_csr(int(232965 * 0.05), int(114615892 * 0.05 * 0.05), seed=3)
        rp, col = trp.numpy().astype(np.int32), tcol_.numpy().astype(np.int32)
    (bp, e2c, e2r), meta = meta_for(dev, rp, col)
    n = len(rp) - 1
    erow = torch.from_numpy(np.repeat(np.arange(n), np.diff(rp))).to(dev)
    tcol = meta[1].long()
    seen = {"calls": 0, "wide": 0, "worst_ef": 0.0, "worst_Y": 0.0}
    real = T.agnn_fused_forward

    def rna10(t):
        u = t.contiguous().view(torch.int32)
        return ((u + 0x1000) & ~0x1fff).view(torch.float32)

    def checked(X, rowptr, cols, w, *rest):
        Y, ef, efm = real(X, rowptr, cols, w, *rest)
        seen["calls"] += 1
        seen["wide"] += int(T.range_mode()[0] != 0)
        xr = rna10(X).double()
        # the bar, plus what fp32 accumulation in ANY order (the reference's tensor-core order included) leaves on a cancelling sum:
        # noise relative to the sum of |terms| (assert_parity's two bounds in one)
        prod = xr[erow] * xr[tcol]
        ref_ef, abs_ef = prod.sum(1), prod.abs().sum(1)
        err = ((ef.double() - ref_ef).abs() / (TOL * ref_ef.abs().clamp(min=1.0) + 16 * TIGHT * abs_ef)).max().item()
        seen["worst_ef"] = max(seen["worst_ef"], err)
        att = rna10((w.reshape(-1)[0] * ef)).double()
        terms = att[:, None] * xr[tcol]
        ref_Y = torch.zeros(n, X.shape[1], dtype=torch.float64, device=dev).index_add_(0, erow, terms)
        abs_Y = torch.zeros(n, X.shape[1], dtype=torch.float64, device=dev).index_add_(0, erow, terms.abs())
        errY = ((Y.double() - ref_Y).abs() / (TOL * ref_Y.abs().clamp(min=1.0) + 16 * TIGHT * abs_Y)).max().item()
        seen["worst_Y"] = max(seen["worst_Y"], errY)
        return Y, ef, efm

    T.agnn_fused_forward = checked
    try:
        torch.manual_seed(0)
        g = torch.Generator(device=dev).manual_seed(0)
        feats = torch.randn(n, 96, device=dev, generator=g)
        labels = torch.ones(n, dtype=torch.long, device=dev)
        model = H.Net(L.AGNNConv, 96, 64, 8, 2).to(dev)
        for conv in (model.conv1, model.conv2):
            conv.weights.data.normal_()                  # the reference's GCN / GIN recipe, unscaled (AGNNConv's own reset scales by 1 / sqrt(out))
        opt = H.make_adam(model.parameters())
        for _ in range(20):
            model.train(); opt.zero_grad()
            loss = H.node_nll_loss(model(feats, meta), labels)
            loss.backward(); opt.step()
    finally:
        T.agnn_fused_forward = real
        T.clear_plan_cache()
    assert seen["calls"] >= 40
    assert seen["worst_ef"] <= 1.0 and seen["worst_Y"] <= 1.0, seen       # (errors in units of the combined bound)


def _wide_range_body(dev, T):
    """VERDICT r02 item 6 / SURVEY.md 7.3: ONE power-of-two scale per matrix loses the elements more than 2^28 below the largest
    (fp16 subnormals, then zero) where the reference's TF32 keeps fp32's exponent (TCGNN_kernel.cu:438-444).  O(1e-3) data with one
    3e7 row (a 1e6 row stays inside the contract on this graph - 130 edges per row x 2e6 x 2^-39 = 5e-4 - and on the MFMA path): rows that never touch the outlier must still come out to accumulation-order accuracy, which the fp16 image cannot
    deliver (its quantum there is 2e-6 per element) - the range guard routes the call, on the device, to the fp32 fallback kernels.
    A matrix whose maximum is small (< 2^8) keeps the fp16 path whatever its small elements are: what they lose is below 1e-9."""
    rp, col = graphs.uniform_graph(4000, 100, seed=5)        # > kSmallMaxTiles wide blocks: the fp16 walks, not the small fp32 kernel
    (bp, e2c, e2r), meta = meta_for(dev, rp, col)
    assert T.plan_info(*meta)["wide_blocks"] > 8192
    n, D = len(rp) - 1, 64
    rng = np.random.default_rng(11)
    T.set_range_guard(3)                                      # strict: every operator, whatever the number of lost elements
    att = rng.standard_normal(len(col)).astype(np.float32)
    # (third case, ADVICE r03: an outlier 2^40 above the rest converts everything else to EXACTLY zero - nothing subnormal is left in
    #  the image to count, so the count must come from the source values; before that fix n_tiny was 0 and the call stayed on MFMA)
    for name, outlier, wide in (("outlier 3e7 over 1e-3 data", 3e7, True), ("1e-14 specks in O(1) data", None, False),
                                ("outlier 1e12 over O(1) data: the rest flushes to zero", 1e12, True)):
        X = (rng.standard_normal((n, D)) * (1e-3 if outlier is None or outlier < 1e10 else 1.0)).astype(np.float32)
        if outlier is not None:
            X[1234] = outlier * (1.0 + rng.random(D).astype(np.float32))
        else:
            X *= 1e3                                             # unit scale, max ~ 4.5 < 2^8: never "wide"
            X[::7] *= 1e-14
        tX = torch.from_numpy(X).to(dev)
        tatt = torch.from_numpy(att).to(dev).view(1, -1)
        Y = T.forward(tX, *meta)[0].cpu().numpy()
        assert T.range_mode()[0] == (1 if wide else 0)       # which way the guard sent it (tcgnn_range_mode)
        Yr = T.forward_fused(tX, *meta, relu=True)[0].cpu().numpy()
        Yv = T.forward_AGNN(tX, meta[0], meta[1], tatt, *meta[2:])[0].cpu().numpy()
        assert T.range_mode()[1] == (1 if wide else 0)
        ef = T.forward_ef(tX, *meta)[0].cpu().numpy()
        assert T.range_mode()[0] == (1 if wide else 0)
        ref = O.spmm(X, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32); r64, a64 = O.spmm_f64(X, rp, col)
        refv = O.spmm_val(X, rp, col, att, bp, e2c, e2r, round_mode=O.ROUND_TF32); _, av64 = O.spmm_f64(X, rp, col, att)
        refe = O.sddmm(X, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32); _, ae64 = O.sddmm_f64(X, rp, col)
        # rows that never touch the outlier: the tight bound is relative to THEIR sum of |terms| (~0.1), not to the matrix maximum
        err = {"spmm": np.abs(Y - ref) / (a64 + 1e-30), "spmm+relu": np.abs(Yr - np.maximum(ref, 0)) / (a64 + 1e-30),
               "spmm_val": np.abs(Yv - refv) / (av64 + 1e-30), "sddmm": np.abs(ef - refe) / (ae64 + 1e-30)}
        for k, v in err.items():
            if wide:
                assert v.max() <= 4 * TIGHT, "%s, %s: %.3e relative to the row's own terms" % (name, k, v.max())
        # the north star's bar holds either way
        for got, want in ((Y, ref), (Yv, refv), (ef, refe)):
            assert (np.abs(got - want) / np.maximum(1.0, np.abs(want))).max() <= TOL
        if wide:   # the fp16 image alone would miss by orders of magnitude: the test is sensitive to the fallback
            small_rows = np.abs(ref).max(axis=1) < (1.0 if outlier < 1e10 else 1e4)   # rows without an edge to the outlier row
            assert small_rows.sum() > n // 2 and err["spmm"][small_rows].max() <= 4 * TIGHT
        # the fused AGNN pair, forward and backward, against the separate operators' definitions
        w = np.float32(0.75)
        tw = torch.tensor([w], device=dev)
        Yf, ef_f, efm = T.agnn_fused_forward(tX, meta[0], meta[1], tw, *meta[2:])
        if wide:
            assert (np.abs(ef_f.cpu().numpy() - refe) / (ae64 + 1e-30)).max() <= 4 * TIGHT
        assert (np.abs(ef_f.cpu().numpy() - refe) / np.maximum(1.0, np.abs(refe))).max() <= TOL
        # (the aggregation is checked on the scores the kernel itself produced: a score that differs from the oracle's by
        #  accumulation noise can round to the neighbouring 10-bit edge weight, a 2^-11 step that no summation order explains)
        att_ref = (w * ef_f.cpu().numpy()).astype(np.float32)
        refYf = O.spmm_val(X, rp, col, att_ref, bp, e2c, e2r, round_mode=O.ROUND_TF32); _, aYf = O.spmm_f64(X, rp, col, att_ref)
        def close(got):   # wide: to accumulation accuracy of every row's OWN terms (ef carries its noise into att: x 64); else the bar
            if wide:
                assert (np.abs(got - refYf) / (aYf + 1e-30)).max() <= 256 * TIGHT
            assert (np.abs(got - refYf) / np.maximum(1.0, np.abs(refYf))).max() <= TOL
        close(Yf.cpu().numpy())
        G, dw = T.agnn_fused_backward(tX, meta[0], meta[1], tw, ef_f, efm, *meta[2:])
        want_dw = float((refe.astype(np.float64) * col.astype(np.float64)).sum())
        scale_dw = float((ae64 * col).sum()) + 1.0
        assert abs(float(dw) - want_dw) <= 1e-5 * scale_dw, (float(dw), want_dw)
        close(G.cpu().numpy())
    # large but HARMLESS: what a training epoch's operands look like (tools/probe_training_ranges.py: max 2e4, ONE element 2^28.7
    # below it) - one lost element is one error of max 2^-39, whatever the graph: the MFMA path stays, for every operator
    X = (rng.standard_normal((n, D)) * 5e3).astype(np.float32)
    X[np.abs(X) < 1.0] = 1.0                     # nothing small ...
    X[77, 5] = 2e-5                              # ... but one speck
    tX = torch.from_numpy(X).to(dev)
    Y = T.forward(tX, *meta)[0].cpu().numpy()
    assert T.range_mode()[0] == 0 and T.last_kernel(*meta).startswith("spmm_")
    ref = O.spmm(X, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32)
    assert (np.abs(Y - ref) / np.maximum(1.0, np.abs(ref))).max() <= TOL
    T.forward_ef(tX, *meta)
    assert T.range_mode()[0] == 0
    # ... thousands of specks still are for the aggregation on this graph (130 edges x 2.5e4 x 2^-39 = 6e-6), but not for the scores,
    # whose bound is quadratic (128 terms x 6e8 x 2^-39 = 0.14): at level 2 SDDMM takes the fallback
    X[::3] = 2e-5
    tX = torch.from_numpy(X).to(dev)
    T.forward(tX, *meta)
    assert T.range_mode()[0] == 0
    ef = T.forward_ef(tX, *meta)[0].cpu().numpy()
    assert T.range_mode()[0] == 1
    refe = O.sddmm(X, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32); _, ae64 = O.sddmm_f64(X, rp, col)
    assert (np.abs(ef - refe) / (ae64 + 1e-30)).max() <= 4 * TIGHT
    # the switch: with the guard off the wide matrix of the first case stays on the MFMA path
    X = (rng.standard_normal((n, D)) * 1e-3).astype(np.float32); X[1234] = 3e7
    T.set_range_guard(0)
    try:
        T.forward(torch.from_numpy(X).to(dev), *meta)
        assert T.range_mode()[0] == 0
    finally:
        T.set_range_guard(1)
    T.forward(torch.from_numpy(X).to(dev), *meta)
    assert T.range_mode()[0] == 1
    T.forward_ef(torch.from_numpy(X).to(dev), *meta)          # level 1: SDDMM answers to its documented bound
    assert T.range_mode()[0] == 0
    T.set_range_guard(2)                                      # the default: dirty rows are patched - since r05 ANY number of them: a matrix that
    ef = T.forward_ef(torch.from_numpy(X).to(dev), *meta)[0].cpu().numpy()   # is wide all over (3 999 dirty rows here) no longer answers to the documented bound
    assert T.range_mode()[0] == 2
    e64, ae64 = O.sddmm_f64(X, rp, col)
    assert (np.abs(ef - e64) <= 2.0 ** -9 * (ae64 + 1e-30)).all()             # every score to the accuracy of its OWN terms (1e-6-sized products beside 3e4-sized ones)
    T.clear_plan_cache()


def test_plan_cache_follows_in_place_mutation_and_streams(dev, T):
    rp, col = graphs.uniform_graph(300, 6, seed=8)
    (bp, e2c, e2r), (trp, tcol, tbp, te2c, te2r) = meta_for(dev, rp, col)
    X = torch.randn(300, 16, device=dev)
    Y1 = T.forward(X, trp, tcol, tbp, te2c, te2r)[0]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                       # launches on torch's current stream
        Y2 = T.forward(X, trp, tcol, tbp, te2c, te2r)[0]
    s.synchronize()
    assert torch.equal(Y1, Y2)
    # replace the graph IN PLACE by one with the same sizes: cached plan must not be reused
    rp2, col2 = rp.copy(), col.copy()
    col2[rp2[0]: rp2[1]] = np.sort(np.random.default_rng(1).choice(300, rp2[1] - rp2[0], replace=False)).astype(np.int32)
    bp2, e2c2, e2r2, _ = graphs.host_sgt(rp2, col2)
    if len(bp2) == len(bp):
        tcol.copy_(torch.from_numpy(col2)); tbp.copy_(torch.from_numpy(bp2)); te2c.copy_(torch.from_numpy(e2c2))
        Y3 = T.forward(X, trp, tcol, tbp, te2c, te2r)[0].cpu().numpy()
        assert np.abs(Y3 - O.spmm(X.cpu().numpy(), rp2, col2, bp2, e2c2, e2r2)).max() < 1e-4


def test_plan_cache_retires_plans_in_stream_order_without_synchronising(dev, T, monkeypatch):
    """A loop over more graphs than the cache holds (a mini-batch of sub-graphs): eviction must not synchronise the device
    (r1 VERDICT: every 9th graph did), the evicted plan must stay alive until the kernels queued on it have run, results stay
    right, and the size is configurable."""
    T.clear_plan_cache()
    T.set_plan_cache_size(3)
    calls = {"n": 0}
    real_sync = torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (calls.__setitem__("n", calls["n"] + 1), real_sync(*a, **k))[1])
    try:
        gs = []
        for k in range(7):
            rp, col = graphs.uniform_graph(2000 + 16 * k, 30, seed=50 + k)
            (bp, e2c, e2r), meta = meta_for(dev, rp, col)
            gs.append((rp, col, bp, e2c, e2r, meta, torch.randn(len(rp) - 1, 32, device=dev)))
        outs = []
        for rnd in range(3):                                   # 21 calls over 7 graphs through 3 slots: every call past the third evicts
            for g in gs:
                outs.append((g, T.forward(g[6], *g[5])[0]))
        assert calls["n"] == 0, "eviction synchronised the device"
        assert T.cache_stats()["plans"] == 3 and T.cache_stats()["retired"] <= 21
    finally:
        monkeypatch.undo()
    torch.cuda.synchronize()
    for (rp, col, bp, e2c, e2r, meta, X), Y in outs[-7:]:
        ref = O.spmm(X.cpu().numpy(), rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32)
        assert np.abs(Y.cpu().numpy() - ref).max() <= 1e-3 * max(1.0, np.abs(ref).max())
    T.forward(gs[0][6], *gs[0][5])                             # a later call reaps what has finished (and retires one more itself)
    assert T.cache_stats()["retired"] <= 1
    T.set_plan_cache_size(8)
    T.clear_plan_cache()


def test_errors_raise_instead_of_exiting(dev, T):
    rp, col = graphs.uniform_graph(100, 5, seed=9)
    (bp, e2c, e2r), (trp, tcol, tbp, te2c, te2r) = meta_for(dev, rp, col)
    X = torch.randn(100, 16, device=dev)
    with pytest.raises(RuntimeError, match="must be contiguous"):
        T.forward(torch.randn(16, 100, device=dev).t(), trp, tcol, tbp, te2c, te2r)
    with pytest.raises(RuntimeError, match="edgeToColumn must be a CUDA tensor"):
        T.forward(X, trp, tcol, tbp, te2c.cpu(), te2r)
    bad = te2c.clone(); bad[0] = 10 ** 6
    with pytest.raises(RuntimeError, match="inconsistent"):
        T.forward(X, trp, tcol, tbp, bad, te2r)
    with pytest.raises(RuntimeError, match="Float"):
        T.forward(X.double(), trp, tcol, tbp, te2c, te2r)


def test_full_size_reddit_shape_properties(dev, T):
    """BASELINE size (N = 232 965, nnz = 114.6 M): size-independent properties instead of the oracle.
      * A @ 1 = degree, exactly (integers below 2^24)
      * linearity: A(X1 + 2 X2) = A X1 + 2 A X2 up to rounding
      * SDDMM on a symmetric graph: ef[(r,c)] = ef[(c,r)]; and sum_e ef[e] = sum_r <x_r, (A x)_r>
      * SpMM-AGNN with all-ones edge values = SpMM
    """
    import tcgnn_graph as G
    n, nnz, _, _ = G.SHAPES["reddit"]
    rp, col = G.synthetic_csr(n, nnz, seed=0, device=dev)
    E = col.numel()
    assert abs(E - nnz) / nnz < 2e-3
    nw = (n + 15) // 16
    bp = torch.zeros(nw, dtype=torch.int32, device=dev); e2c = torch.zeros(E, dtype=torch.int32, device=dev); e2r = torch.zeros(E, dtype=torch.int32, device=dev)
    T.preprocess_gpu(col, rp, n, 16, 8, bp, e2c, e2r)
    meta = (rp, col, bp, e2c, e2r)
    deg = (rp[1:] - rp[:-1]).float()
    ones = torch.ones(n, 16, device=dev)
    Yd = T.forward(ones, *meta)[0]
    assert torch.equal(Yd, deg[:, None].expand(-1, 16))
    g = torch.Generator(device=dev).manual_seed(0)
    X1 = torch.randn(n, 64, device=dev, generator=g); X2 = torch.randn(n, 64, device=dev, generator=g)
    Y1 = T.forward(X1, *meta)[0]; Y2 = T.forward(X2, *meta)[0]; Y12 = T.forward(X1 + 2 * X2, *meta)[0]
    # this graph is dense enough for the LDS-resident column-range kernel (the automatic choice above): the range-blocked
    # gather walk and the per-window walk must give the same sums (fp32 accumulation order differs: ~1e-5 of the scale)
    import tcgnn_capi as c
    if os.environ.get("TCGNN_LDS_AUTO", "1") != "0":   # (the variable switches the automatic choice off)
        assert T.plan_info(*meta)["lds_ranges"] in ((n + 503) // 504, (n + 759) // 760)   # 4- or 8-window layout (TCGNN_LDS_MAXW)
    try:
        for mode in (1, 2):
            c.check(c.lib.tcgnn_set_spmm_mode(mode), "tcgnn_set_spmm_mode")
            Ym = T.forward(X1, *meta)[0]
            assert ((Ym - Y1).abs() / (deg.sqrt()[:, None] + 1)).max().item() < 1e-4, mode
            assert torch.equal(T.forward(ones, *meta)[0], Yd)
    finally:
        c.lib.tcgnn_set_spmm_mode(0)
    scale = deg.sqrt()[:, None] * 3 + 1
    assert ((Y12 - (Y1 + 2 * Y2)).abs() / scale).max().item() < 3e-2      # three independently rounded operands
    Yv = T.forward_AGNN(X1, rp, col, torch.ones(1, E, device=dev), bp, e2c, e2r)[0]
    assert (Yv - Y1).abs().max().item() <= 1e-3
    ef = T.forward_ef(X1, *meta)[0]
    rows = e2r.long()
    key_fwd = rows * n + col.long(); key_bwd = col.long() * n + rows
    order_f = torch.argsort(key_fwd); order_b = torch.argsort(key_bwd)
    assert torch.equal(key_fwd[order_f], key_bwd[order_b])                   # the graph is symmetric
    assert (ef[order_f] - ef[order_b]).abs().max().item() <= 1e-3
    lhs = ef.double().sum().item()
    rhs = (X1.double() * Y1.double()).sum().item()
    assert abs(lhs - rhs) <= 1e-5 * ef.double().abs().sum().item()
    del X1, X2, Y1, Y2, Y12, Yv, ef, order_f, order_b, key_fwd, key_bwd
    # ... and the oracle itself on a sample of row windows, every walk (the headline kernel among them)
    kernels = _sampled_oracle_checks(dev, T, n, E, meta, 64, lds_ordinary=True)
    if os.environ.get("TCGNN_LDS_AUTO", "1") != "0":
        assert kernels["automatic spmm"].startswith("spmm_lds_flat_kernel"), kernels
    T.clear_plan_cache()


def test_full_size_sbm_reddit_headline_graph_against_the_oracle(dev, T, capfd, monkeypatch):
    """r05: the HEADLINE graph - Reddit shape from the SBM calibrated to real Reddit's TC-block count - at full
    size: A @ 1 = degree exactly, and the oracle's own window bodies on 256 sampled windows for forward, forward_AGNN, forward_ef
    and the fused pair, for the automatic kernels (the flat stream WITH dense entries: spmm_lds_flat_kernel; the edge-valued walk
    with dense entries: spmm_lds_val_kernel), both forced gather walks and the ordinary LDS stream."""
    import tcgnn_graph as G
    monkeypatch.setenv("TCGNN_VERBOSE", "1")
    n, nnz, _, _ = G.SHAPES["reddit"]
    rp, col = G.GENERATORS["sbm_reddit"](n, nnz, seed=0, device=dev)
    E = col.numel()
    nw = (n + 15) // 16
    bp = torch.zeros(nw, dtype=torch.int32, device=dev); e2c = torch.zeros(E, dtype=torch.int32, device=dev); e2r = torch.zeros(E, dtype=torch.int32, device=dev)
    T.preprocess_gpu(col, rp, n, 16, 8, bp, e2c, e2r)
    meta = (rp, col, bp, e2c, e2r)
    assert abs(T.plan_info(*meta)["tc_blocks"] - 13566510) / 13566510 < 0.01          # /root/reference/logs/reduce_blocks.csv:18 (real Reddit)
    deg = (rp[1:] - rp[:-1]).float()
    assert torch.equal(T.forward(torch.ones(n, 64, device=dev), *meta)[0], deg[:, None].expand(-1, 64))
    kernels = _sampled_oracle_checks(dev, T, n, E, meta, 64, lds_ordinary=True)
    err = capfd.readouterr().err
    if os.environ.get("TCGNN_LDS_AUTO", "1") != "0":
        assert kernels["automatic spmm"].startswith("spmm_lds_flat_kernel"), kernels
        assert "spmm_lds_val_kernel" in kernels["automatic spmm_val"], kernels
        import re
        dense = [int(x) for x in re.findall(r"entries \((\d+) dense\)", err)]
        assert len(dense) >= 2 and min(dense[:2]) > 1000, err[-2000:]                 # both streams carry dense entries
    T.clear_plan_cache()


def _sampled_oracle_checks(dev, T, n, E, meta, D, nwin=256, seed=0, lds_ordinary=False, extra_modes=(), must_include=None):
    """VERDICT r03 "oracle evidence at BASELINE size": the full-size tests above assert size-independent properties; here the SAME
    launches are compared with the ORACLE itself on a sample - `nwin` random row windows (16 rows each: 4 096 rows, ~1-2 M edges
    on the Reddit shape) evaluated by the oracle's own thread-block / warp bodies (oracle_spmm_windows / oracle_sddmm_windows =
    TCGNN_kernel.cu:336-454, :459-578, :584-727 restated) on the full-size inputs, next to fp64 gathers of the definition on the
    device - with the bounds of assert_parity (1e-3 max(1, |ref|); accumulation noise against the TF32-mode oracle; 2^-9 of the
    sum of |terms| against fp64), for the automatic kernel AND every forced walk, for forward, forward_AGNN, forward_ef and the
    fused AGNN pair."""
    import tcgnn_capi as c
    rp, col, bp, e2c, e2r = meta
    host = tuple(t.cpu().numpy() for t in meta)
    rng = np.random.default_rng(seed + D)
    nw = (n + 15) // 16
    windows = rng.choice(nw, size=min(nwin, nw), replace=False)
    if must_include is not None:   # (e.g. the hub windows of a skewed graph: a random sample of 256 in 14 561 would miss them)
        windows = np.union1d(windows, np.asarray(must_include))
    windows = np.sort(windows).astype(np.int32)
    g = torch.Generator(device=dev).manual_seed(1000 + D + seed)
    X = torch.randn(n, D, device=dev, generator=g)
    att = torch.randn(E, device=dev, generator=g)
    Xh, atth = X.cpu().numpy(), att.cpu().numpy()
    rows, Yref = O.spmm_windows(Xh, *host, windows)
    _, Yvref = O.spmm_windows(Xh, *host, windows, att=atth)
    edges, efref = O.sddmm_windows(Xh, *host, windows)
    # fp64 evaluation of the definitions for the sampled rows / edges, on the device
    trows = torch.from_numpy(rows).to(dev)
    lens = (rp[trows + 1] - rp[trows]).long()
    seg = torch.repeat_interleave(torch.arange(len(rows), device=dev), lens)
    first = torch.cumsum(lens, 0) - lens
    eidx = rp[trows].long()[seg] + (torch.arange(int(lens.sum()), device=dev) - first[seg])
    assert torch.equal(eidx, torch.from_numpy(edges).to(dev))           # (the oracle's edge list of the windows = the CSR's)
    xc = X[col[eidx].long()].double()
    Y64 = torch.zeros(len(rows), D, dtype=torch.float64, device=dev).index_add_(0, seg, xc)
    A64 = torch.zeros_like(Y64).index_add_(0, seg, xc.abs())
    av = att[eidx].double()[:, None]
    Yv64 = torch.zeros_like(Y64).index_add_(0, seg, xc * av)
    Av64 = torch.zeros_like(Y64).index_add_(0, seg, xc.abs() * av.abs())
    xr = X[trows[seg]].double()
    ef64 = (xr * xc).sum(1); aef64 = (xr * xc).abs().sum(1)
    del xr, av
    Y64, A64, Yv64, Av64, ef64, aef64 = (t.cpu().numpy() for t in (Y64, A64, Yv64, Av64, ef64, aef64))
    tedges = eidx
    w = torch.tensor([0.37], device=dev)
    dY = torch.randn(n, D, device=dev, generator=g)
    dYh = dY.cpu().numpy()
    kernels = {}

    def one_walk(tag, spmm_only=False):
        got = T.forward(X, *meta)[0][trows].cpu().numpy()
        kernels["%s spmm" % tag] = T.last_kernel(*meta)
        assert_parity(got, Yref, Y64, A64, "full-size spmm D=%d, %s (%s)" % (D, tag, T.last_kernel(*meta)))
        if spmm_only:
            return
        T.forward_AGNN(X, rp, col, att.view(1, -1), bp, e2c, e2r)     # (the first edge-valued call of a plan builds the LDS-resident walk's stream)
        got = T.forward_AGNN(X, rp, col, att.view(1, -1), bp, e2c, e2r)[0][trows].cpu().numpy()
        kernels["%s spmm_val" % tag] = T.last_kernel(*meta)
        assert_parity(got, Yvref, Yv64, Av64, "full-size forward_AGNN D=%d, %s (%s)" % (D, tag, T.last_kernel(*meta)))
        got = T.forward_ef(X, *meta)[0][tedges].cpu().numpy()
        kernels["%s sddmm" % tag] = T.last_kernel(*meta)
        assert_parity(got, efref, ef64, aef64, "full-size forward_ef D=%d, %s (%s)" % (D, tag, T.last_kernel(*meta)))
        # the fused pair: scores against the oracle's SDDMM; the aggregation against the oracle's edge-valued SpMM fed with the edge
        # weights the kernel itself produced (a score one accumulation-noise step away can round to the neighbouring 10-bit weight)
        Yf, ef_f, efm = T.agnn_fused_forward(X, rp, col, w, bp, e2c, e2r)
        kernels["%s fused fwd" % tag] = T.last_kernel(*meta)
        assert_parity(ef_f[tedges].cpu().numpy(), efref, ef64, aef64, "full-size fused ef D=%d, %s" % (D, tag))
        att_k = (w * ef_f)
        att_kh = att_k.cpu().numpy()
        _, Yfref = O.spmm_windows(Xh, *host, windows, att=att_kh)
        akk = att_k[eidx].double()[:, None]
        xcc = X[col[eidx].long()].double()
        Yf64 = torch.zeros(len(rows), D, dtype=torch.float64, device=dev).index_add_(0, seg, xcc * akk).cpu().numpy()
        Af64 = torch.zeros(len(rows), D, dtype=torch.float64, device=dev).index_add_(0, seg, xcc.abs() * akk.abs()).cpu().numpy()
        # (|att| ~ 0.37 sqrt(D) |x|^2: the 1e-3 bar is stated for O(1) operands - here the tight, scale-relative bounds decide)
        assert_parity(Yf[trows].cpu().numpy(), Yfref, Yf64, Af64, "full-size fused Y D=%d, %s" % (D, tag), unit_scale=False)
        G, _ = T.agnn_fused_backward(dY, rp, col, w, ef_f, efm, bp, e2c, e2r)
        kernels["%s fused bwd" % tag] = T.last_kernel(*meta)
        _, Gref = O.spmm_windows(dYh, *host, windows, att=att_kh)
        dc = dY[col[eidx].long()].double()
        G64 = torch.zeros(len(rows), D, dtype=torch.float64, device=dev).index_add_(0, seg, dc * akk).cpu().numpy()
        Ag64 = torch.zeros(len(rows), D, dtype=torch.float64, device=dev).index_add_(0, seg, dc.abs() * akk.abs()).cpu().numpy()
        assert_parity(G[trows].cpu().numpy(), Gref, G64, Ag64, "full-size fused G D=%d, %s" % (D, tag), unit_scale=False)

    try:
        for mode, tag in ((0, "automatic"), (1, "per-window walk"), (2, "range-blocked / range-major walk")) + tuple(extra_modes):
            c.check(c.lib.tcgnn_set_spmm_mode(mode), "tcgnn_set_spmm_mode")
            one_walk(tag)
        if lds_ordinary:   # the ordinary cell stream of the LDS-resident kernel (what graphs with communities or hubs take)
            os.environ["TCGNN_LDS_FLAT"] = "0"
            T.clear_plan_cache()
            try:
                c.check(c.lib.tcgnn_set_spmm_mode(3), "tcgnn_set_spmm_mode")
                one_walk("LDS-resident, ordinary stream", spmm_only=True)
                assert kernels["LDS-resident, ordinary stream spmm"].startswith("spmm_lds_kernel")
            finally:
                os.environ.pop("TCGNN_LDS_FLAT", None)
                T.clear_plan_cache()
    finally:
        c.lib.tcgnn_set_spmm_mode(0)
    return kernels


def test_full_size_reddit_shape_with_hub_rows_against_the_oracle(dev, T):
    """r06: the degree-skewed Reddit-sized graph bench.py times (`skewed_spmm_ms`: a ~24 k-degree hub at a mean of
    492 - real Reddit: 21 657) had never been CHECKED at that size.  A @ 1 = degree exactly, and the oracle's window bodies on 128
    random windows plus the eight heaviest (the hub rows' own), for the automatic kernels and both forced gather walks."""
    import tcgnn_graph as G
    n, nnz, _, _ = G.SHAPES["reddit"]
    rp, col = G.synthetic_csr(n, nnz, seed=1, device=dev, skew=0.6)
    E = col.numel()
    nw = (n + 15) // 16
    bp = torch.zeros(nw, dtype=torch.int32, device=dev); e2c = torch.zeros(E, dtype=torch.int32, device=dev); e2r = torch.zeros(E, dtype=torch.int32, device=dev)
    T.preprocess_gpu(col, rp, n, 16, 8, bp, e2c, e2r)
    meta = (rp, col, bp, e2c, e2r)
    deg = (rp[1:] - rp[:-1])
    assert int(deg.max()) >= 20000
    assert torch.equal(T.forward(torch.ones(n, 64, device=dev), *meta)[0], deg.float()[:, None].expand(-1, 64))
    heavy = torch.topk(bp.float(), 8).indices.cpu().numpy()
    _sampled_oracle_checks(dev, T, n, E, meta, 64, nwin=128, must_include=heavy)
    T.clear_plan_cache()


def test_full_size_ogbn_products_sbm_graph_on_the_slice_synchronised_walk(dev, T):
    """r06: BASELINE.json configs[3]'s shape from the community generator (50 communities of 49 k rows, 90 % of the
    edges inside: a community's image is 12.5 MB at D = 128, three times an XCD's L2) - the graph the slice-synchronised range walk was
    built for.  The automatic mode takes it for SpMM, forward_AGNN, SDDMM and the fused forward pass; A @ 1 = degree exactly; and the
    oracle's window bodies on 512 sampled windows for that walk, the per-window and range-blocked walks and the walk forced in both
    directions of the fused pair (mode 5)."""
    import tcgnn_graph as G
    n, nnz, _, _ = G.SHAPES["ogbn-products"]
    rp, col = G.GENERATORS["sbm"](n, nnz, seed=0, device=dev)
    E = col.numel()
    nw = (n + 15) // 16
    bp = torch.zeros(nw, dtype=torch.int32, device=dev); e2c = torch.zeros(E, dtype=torch.int32, device=dev); e2r = torch.zeros(E, dtype=torch.int32, device=dev)
    T.preprocess_gpu(col, rp, n, 16, 8, bp, e2c, e2r)
    meta = (rp, col, bp, e2c, e2r)
    deg = (rp[1:] - rp[:-1]).float()
    assert torch.equal(T.forward(torch.ones(n, 128, device=dev), *meta)[0], deg[:, None].expand(-1, 128))
    assert T.last_kernel(*meta) == "spmm_sync_kernel"
    kernels = _sampled_oracle_checks(dev, T, n, E, meta, 128, nwin=512, extra_modes=((5, "slice-synchronised walk, forced"),))
    assert kernels["automatic spmm"] == "spmm_sync_kernel" and kernels["automatic spmm_val"] == "spmm_sync_kernel", kernels
    assert kernels["automatic sddmm"] == "sddmm_kernel (slice-synchronised)" and kernels["automatic fused fwd"] == "agnn_kernel (slice-synchronised)", kernels
    assert kernels["slice-synchronised walk, forced fused bwd"] == "agnn_kernel (slice-synchronised)", kernels
    T.clear_plan_cache()


GEMM_CASES = [c for c in CASES if c[0] in ("uniform_n17", "uniform_n1000", "empty_middle_window_n48", "powerlaw_n1000", "citeseer_shape", "dense_n3000_deg150", "no_edges_n20")]


@pytest.mark.parametrize("case", GEMM_CASES, ids=[c[0] for c in GEMM_CASES])
@pytest.mark.parametrize("dims", [(64, 41), (16, 16), (41, 7), (128, 128), (96, 33), (32, 64)])
def test_dense_update_fused_behind_the_aggregation(dev, T, case, dims):
    """f3: forward_gemm(X, W) = (A X) W in one launch (gnn_conv.py:92-97 as one kernel) against the two steps it replaces -
    forward() then an fp64 product of the fp32 aggregate - at accumulation-noise distance, with and without the fused ReLU."""
    _, rp, col = case
    din, dout = dims
    n = len(rp) - 1
    (bp, e2c, e2r), meta = meta_for(dev, rp, col)
    rng = np.random.default_rng(din * 131 + dout + n)
    X = rng.standard_normal((n, din)).astype(np.float32); W = (rng.standard_normal((din, dout)) / np.sqrt(din)).astype(np.float32)
    tX, tW = to_dev(dev, X, W)
    # expected value: the ORACLE's aggregate (TF32-mode operands, as forward() rounds them) times W in fp64 - not the HIP path's own
    # forward() (HIP against HIP).  The oracle accumulates in fp32 in its own order: its distance to the kernel's
    # aggregate is accumulation noise relative to sum |a||x| (TIGHT), carried through |W|.
    agg_o = O.spmm(X, rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32).astype(np.float64)
    _, abs_o = O.spmm_f64(X, rp, col)
    want = torch.from_numpy(agg_o @ W.astype(np.float64)).to(dev)
    bound = torch.from_numpy((abs_o + 1.0) @ np.abs(W.astype(np.float64)) + 1.0).to(dev)
    got = T.forward_gemm(tX, tW, *meta)[0]
    assert got.shape == (n, dout) and got.dtype == torch.float32
    assert n == 0 or ((got.double() - want).abs() / bound).max().item() <= 2 * TIGHT
    got_r = T.forward_gemm(tX, tW, *meta, relu=True)[0]
    assert n == 0 or ((got_r.double() - want.clamp(min=0)).abs() / bound).max().item() <= 2 * TIGHT
    # ... and the two-step form it replaces stays within the same distance
    agg = T.forward(tX, *meta)[0]
    assert n == 0 or ((agg.double() @ tW.double() - want).abs() / bound).max().item() <= 2 * TIGHT
    assert torch.equal(got, T.forward_gemm(tX, tW, *meta)[0])                      # deterministic
    with pytest.raises(RuntimeError, match="D_in, D_out <= 128"):
        T.forward_gemm(torch.zeros(n, 129, device=dev), torch.zeros(129, 4, device=dev), *meta)


@pytest.mark.parametrize("dims", [(64, 41), (32, 48), (41, 64), (48, 16)])
def test_dense_update_on_the_lds_resident_kernel(dev, T, dims, monkeypatch):
    """The same on a graph dense enough for the LDS-resident kernel (forced: mode 3): a 64-column input runs as two 32-column
    passes that ADD their products into a zeroed Y (two addends - bit-reproducible), narrower inputs as one pass that stores."""
    import tcgnn_capi as c
    import tcgnn_graph as G
    din, dout = dims
    rp, col = G.synthetic_csr(30000, 6_000_000, seed=3, device=dev)
    n, E = rp.numel() - 1, col.numel()
    bp = torch.zeros((n + 15) // 16, dtype=torch.int32, device=dev); e2c = torch.zeros(E, dtype=torch.int32, device=dev); e2r = torch.zeros(E, dtype=torch.int32, device=dev)
    T.preprocess_gpu(col, rp, n, 16, 8, bp, e2c, e2r)
    meta = (rp, col, bp, e2c, e2r)
    g = torch.Generator(device=dev).manual_seed(din + dout)
    X = torch.randn(n, din, device=dev, generator=g); W = torch.randn(din, dout, device=dev, generator=g) / din ** 0.5
    monkeypatch.setenv("TCGNN_LDS_FLAT", "0")   # (the ordinary cell stream: a flat one with a cold remainder leaves the fused update to the gather walk)
    T.clear_plan_cache()
    try:
        c.check(c.lib.tcgnn_set_spmm_mode(3), "tcgnn_set_spmm_mode")
        agg = T.forward(X, *meta)[0]
        assert T.last_kernel(*meta) == "spmm_lds_kernel"
        got = T.forward_gemm(X, W, *meta)[0]
        assert T.last_kernel(*meta) == "spmm_lds_kernel"
        got_r = T.forward_gemm(X, W, *meta, relu=True)[0]
        again = T.forward_gemm(X, W, *meta)[0]
    finally:
        c.lib.tcgnn_set_spmm_mode(0)
    # expected value from the oracle's aggregate (see test_dense_update_fused_behind_the_aggregation), on 512 sampled row windows
    host = tuple(t.cpu().numpy() for t in meta)
    wins = np.sort(np.random.default_rng(din).choice((n + 15) // 16, size=512, replace=False)).astype(np.int32)
    rows, agg_o = O.spmm_windows(X.cpu().numpy(), *host, wins)
    trows = torch.from_numpy(rows).to(dev)
    assert ((agg[trows].double().cpu().numpy() - agg_o) ** 2).sum() <= 1e-8 * (agg_o.astype(np.float64) ** 2).sum()
    want_o = torch.from_numpy(agg_o.astype(np.float64)).to(dev) @ W.double()
    bound_o = torch.from_numpy(np.abs(agg_o).astype(np.float64)).to(dev) @ W.double().abs() + 200.0    # (+ the aggregate's own accumulation noise: ~200 terms per row)
    assert ((got[trows].double() - want_o).abs() / bound_o).max().item() <= 2 * TIGHT
    want = agg.double() @ W.double()
    bound = agg.double().abs() @ W.double().abs() + 1.0
    assert ((got.double() - want).abs() / bound).max().item() <= 4e-6
    assert ((got_r.double() - want.clamp(min=0)).abs() / bound).max().item() <= 4e-6
    assert torch.equal(got, again)
    # the per-window gather walk gives the same product
    c.check(c.lib.tcgnn_set_spmm_mode(1), "tcgnn_set_spmm_mode")
    try:
        ref = T.forward_gemm(X, W, *meta)[0]
        assert T.last_kernel(*meta) == "spmm_kernel"
    finally:
        c.lib.tcgnn_set_spmm_mode(0)
    assert ((got - ref).abs().double() / bound).max().item() <= 4e-6


def test_gcn_layer_that_aggregates_first_trains_like_the_reference_order(dev, T):
    """GCNConv(aggregate_first=True): (A X) W in one launch instead of A (X W).  Same matrix, rounded at a different point:
    forward within the 1e-3 bar of the reference order, gradients from the unchanged backward pass identical in form
    (G = A dY; dX = G W^T; dW = X^T G), and GIN takes the fused launch only when no gradient is asked for."""
    import tcgnn_layers as L
    rp, col = graphs.uniform_graph(3000, 150, seed=2)
    _, meta = meta_for(dev, rp, col)
    torch.manual_seed(0)
    conv = L.GCNConv(64, 41).to(dev)
    conv.weights.data.mul_(0.125)
    x = torch.randn(3000, 64, device=dev)
    xa = x.clone().requires_grad_(True); xb = x.clone().requires_grad_(True)
    ya = conv(xa, *meta)
    yb = conv(xb, *meta, aggregate_first=True)
    A = torch.zeros(3000, 3000, dtype=torch.float64, device=dev)
    A[torch.from_numpy(np.repeat(np.arange(3000), np.diff(rp))).to(dev), meta[1].long()] = 1.0
    exact = A @ (x.double() @ conv.weights.detach().double())
    scale = A @ (x.double().abs() @ conv.weights.detach().double().abs()) + 1.0       # sum of |terms|: what 10-bit operand rounding is relative to
    for y in (ya, yb):                                                          # either order is within operand rounding of the exact matrix
        assert ((y.detach().double() - exact).abs() / scale).max().item() <= 2.0 ** -9
    dY = torch.randn_like(ya)
    ya.backward(dY); ga, gwa = xa.grad.clone(), conv.weights.grad.clone(); conv.weights.grad = None
    yb.backward(dY)
    assert torch.equal(ga, xb.grad) and torch.equal(gwa, conv.weights.grad)
    gin = L.GINConv(64, 41).to(dev)
    calls = []
    real_gemm = T.forward_gemm
    T.forward_gemm = lambda *a, **k: (calls.append(1), real_gemm(*a, **k))[1]
    try:
        with torch.no_grad():                         # ordinary Parameters (requires_grad = True): the grad MODE decides (r2 ADVICE)
            y_fused = gin(x, *meta)
        assert len(calls) == 1 and gin.weights.requires_grad and y_fused.grad_fn is None
        gin(x.clone().requires_grad_(True), *meta)     # training: the two-step form, A X is needed for dW
        assert len(calls) == 1
    finally:
        T.forward_gemm = real_gemm
    assert T.last_kernel(*meta).split(" ")[0] in ("spmm_kernel", "spmm_lds_kernel", "spmm_lds_flat_kernel")
    y_two = gin(x.clone().requires_grad_(True), *meta)
    assert ((y_fused - y_two).abs() / (y_two.abs() + 10.0)).max().item() <= 1e-5



def test_gin_layer_eval_and_train_forward_agree(dev, T):
    """GINConv under no_grad takes the one-launch (A X) W of tcgnn_spmm_gemm, in training forward() + torch.mm - another
    summation order.  The two agree within the bar at layer level, against the oracle's aggregate too, and the switch
    (tcgnn_layers.GIN_FUSED_INFERENCE / TCGNN_GIN_FUSED_INFERENCE=0) puts eval on the training path's arithmetic bit for bit."""
    import tcgnn_layers as L
    for name, (rp, col), din, dout in (("sparse", graphs.uniform_graph(3000, 150, seed=2), 64, 41), ("citeseer shape", graphs.uniform_graph(3327, 2.8, seed=1), 16, 16),
                                       ("dense enough for the LDS-resident kernel", graphs.uniform_graph(20000, 300, seed=9), 64, 64)):
        (bp, e2c, e2r), meta = meta_for(dev, rp, col)
        n = len(rp) - 1
        torch.manual_seed(3)
        gin = L.GINConv(din, dout).to(dev)
        gin.weights.data.mul_(din ** -0.5)
        x = torch.randn(n, din, device=dev)
        y_train = gin(x.clone().requires_grad_(True), *meta).detach()
        with torch.no_grad():
            y_eval = gin(x, *meta)
        agg_o = O.spmm(x.cpu().numpy(), rp, col, bp, e2c, e2r, round_mode=O.ROUND_TF32).astype(np.float64)
        want = agg_o @ gin.weights.detach().double().cpu().numpy()
        for y in (y_train, y_eval):
            err = np.abs(y.double().cpu().numpy() - want) / np.maximum(1.0, np.abs(want))
            assert err.max() <= TOL, (name, err.max())
        assert ((y_eval - y_train).abs() / (y_train.abs() + 10.0)).max().item() <= 1e-5, name
        old = L.GIN_FUSED_INFERENCE
        L.GIN_FUSED_INFERENCE = False
        try:
            with torch.no_grad():
                assert torch.equal(gin(x, *meta), y_train), name
        finally:
            L.GIN_FUSED_INFERENCE = old
        T.clear_plan_cache()


def _device_meta(dev, T, shape, seed=0):
    import tcgnn_graph as G
    n, nnz, _, _ = G.SHAPES[shape]
    rp, col = G.synthetic_csr(n, nnz, seed=seed, device=dev)
    E = col.numel()
    assert abs(E - nnz) / nnz < 2e-3
    nw = (n + 15) // 16
    bp = torch.zeros(nw, dtype=torch.int32, device=dev); e2c = torch.zeros(E, dtype=torch.int32, device=dev); e2r = torch.zeros(E, dtype=torch.int32, device=dev)
    T.preprocess_gpu(col, rp, n, 16, 8, bp, e2c, e2r)
    return n, E, (rp, col, bp, e2c, e2r)


def _wide_agnn_properties(dev, T, n, E, meta, D):
    """Size-independent properties of the AGNN operators at full size and width D (BASELINE.json configs[3] is D = 128):
    SDDMM symmetry and the trace identity sum_e ef[e] = sum_r <x_r, (A x)_r>; forward_AGNN(ones) = forward; the fused pair
    (one gather for SDDMM + edge-weighted SpMM, forward and backward) = the separate calls."""
    rp, col, bp, e2c, e2r = meta
    g = torch.Generator(device=dev).manual_seed(D)
    X = torch.randn(n, D, device=dev, generator=g)
    deg = (rp[1:] - rp[:-1]).float()
    Y = T.forward(X, *meta)[0]
    Yv = T.forward_AGNN(X, rp, col, torch.ones(1, E, device=dev), bp, e2c, e2r)[0]
    assert ((Yv - Y).abs() / (deg.sqrt()[:, None] + 1)).max().item() <= 1e-4
    ef = T.forward_ef(X, *meta)[0]
    rows = e2r.long()
    key_fwd = rows * n + col.long()
    order_f = torch.argsort(key_fwd)
    key_bwd = col.long() * n + rows
    order_b = torch.argsort(key_bwd)
    assert torch.equal(key_fwd[order_f], key_bwd[order_b])                   # the graph is symmetric
    del key_fwd, key_bwd
    assert (ef[order_f] - ef[order_b]).abs().max().item() <= 1e-3 * (D / 64.0) ** 0.5
    del order_f, order_b
    lhs = ef.double().sum().item()
    rhs = (X.double() * Y.double()).sum().item()
    assert abs(lhs - rhs) <= 1e-5 * ef.double().abs().sum().item()
    # fused pair against the separate calls
    w = torch.tensor([0.37], device=dev)
    assert T.agnn_fused_supported(X, *meta)
    Yf, ef_f, efm = T.agnn_fused_forward(X, rp, col, w, bp, e2c, e2r)
    assert (ef_f - ef).abs().max().item() <= 1e-5 * (1.0 + ef.abs().max().item())
    assert int(efm[0].item()) == int(ef_f.abs().max().reshape(1).view(torch.int32).item())
    att = (w * ef).view(1, -1).contiguous()
    Ys = T.forward_AGNN(X, rp, col, att, bp, e2c, e2r)[0]
    bound = (deg.sqrt()[:, None] * float(D) + 1.0)                           # |att| ~ 0.37 sqrt(D), |x| ~ 1: row sums ~ sqrt(deg D)
    assert ((Yf - Ys).abs() / bound).max().item() <= 1e-4
    dY = torch.randn(n, D, device=dev, generator=g)
    Gf, dwf = T.agnn_fused_backward(dY, rp, col, w, ef_f, efm, bp, e2c, e2r)
    Gs = T.forward_AGNN(dY, rp, col, att, bp, e2c, e2r)[0]
    assert ((Gf - Gs).abs() / bound).max().item() <= 1e-4
    del Gs, Ys, att
    d_att = T.forward_ef(dY, *meta)[0]
    dws = (d_att.double() * col.double()).sum().item()
    scale = (d_att.double().abs() * col.double()).sum().item()
    assert abs(float(dwf.item()) - dws) <= 1e-6 * scale + 1e-3 * abs(dws)    # d_w is returned as float32


def test_full_size_reddit_shape_wide_and_fused_properties(dev, T):
    """The Reddit-sized graph again at D = 128 and through the fused AGNN pair (r1 VERDICT: not covered at full size)."""
    n, E, meta = _device_meta(dev, T, "reddit")
    _wide_agnn_properties(dev, T, n, E, meta, 128)
    _sampled_oracle_checks(dev, T, n, E, meta, 128)
    T.clear_plan_cache()


def test_full_size_ogbn_products_shape_properties(dev, T):
    """BASELINE.json configs[3] at its own size: ogbn-products shape, N = 2 449 029, nnz = 123.7 M, AGNN hidden = 128.
      * A @ 1 = degree, exactly
      * SDDMM symmetry + trace identity, forward_AGNN(ones) = forward, fused AGNN pair = separate calls (D = 128)
      * every SpMM walk that applies gives the same sums
    """
    n, E, meta = _device_meta(dev, T, "ogbn-products")
    rp = meta[0]
    deg = (rp[1:] - rp[:-1]).float()
    ones = torch.ones(n, 16, device=dev)
    Yd = T.forward(ones, *meta)[0]
    assert torch.equal(Yd, deg[:, None].expand(-1, 16))
    import tcgnn_capi as c
    g = torch.Generator(device=dev).manual_seed(1)
    X1 = torch.randn(n, 128, device=dev, generator=g)
    Y1 = T.forward(X1, *meta)[0]
    try:
        for mode in (1, 2):
            c.check(c.lib.tcgnn_set_spmm_mode(mode), "tcgnn_set_spmm_mode")
            Ym = T.forward(X1, *meta)[0]
            assert ((Ym - Y1).abs() / (deg.sqrt()[:, None] + 1)).max().item() < 1e-4, mode
            assert torch.equal(T.forward(ones, *meta)[0], Yd)
    finally:
        c.lib.tcgnn_set_spmm_mode(0)
    del X1, Y1, Ym, ones, Yd
    _wide_agnn_properties(dev, T, n, E, meta, 128)
    _sampled_oracle_checks(dev, T, n, E, meta, 128, nwin=512)   # (50 edges per row: 512 windows = 8 192 rows, ~0.4 M edges)
    T.clear_plan_cache()
