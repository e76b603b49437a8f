"""Every layer, and the operators the layers do not isolate, on the graphs mini-batch training builds (tests/minibatch_ref.py's catalogue:
ragged last windows, fewer than 16 rows, windows without edges between populated ones, fewer than 4 edges, no edges at all), and the
harness on mini-batches for the models no other test runs there.

(a) layers: the batch is built on the device and read back against the numpy restatement; the layer runs on batch.metas[i] and its
    output, input gradient and every parameter gradient are judged against the dense fp64 model with the bound of the layer's own GPU
    test (minibatch_ref.LAYERS names each); rows without edges hold the empty-sum value exactly.
(b) operators: transposed, scaled, edge-valued and SDDMM calls against the fp64 products with the project's three bounds
    (test_gpu_parity.assert_parity through walks.judge), routing automatic, and the staged fp16 walk forced on the ragged block.
(c) harness: --sampler dense against rows bit for bit, saint and cluster reproducible, the plan / CSR cache within its size."""
import numpy as np
import pytest
import torch

import edge_ops_ref as EO
import graphs
import minibatch_ref as MB
import walks as W
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ENTRY_IDS = [e.name for e in MB.CATALOGUE]
LAYER_IDS = [c.name for c in MB.LAYERS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def T():
    import TCGNN
    return TCGNN


def _dev(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


_CSR = []


def _csr(dev):
    if not _CSR:
        rp, col = MB.full_graph()
        _CSR.append((_dev(dev, rp.astype(np.int32)), _dev(dev, col.astype(np.int32))))
    return _CSR[0]


def _same(got, want, what, dtype=torch.int32):
    assert got.dtype == dtype, "%s is %s" % (what, got.dtype)
    assert torch.equal(got.cpu(), torch.from_numpy(np.ascontiguousarray(want)).to(dtype)), "%s differs from the restatement" % what


def _batch(dev, entry):
    """the entry's batch built on the device, every field read back against the numpy restatement and the host translation"""
    import tcgnn_layers as L
    batch = entry.device(L, _csr(dev))
    nodes, new_id, seed_pos, blocks, eids = entry.host()
    _same(batch.nodes, nodes, entry.name + ": nodes")
    _same(batch.new_id, new_id, entry.name + ": new_id")
    _same(batch.seed_pos, seed_pos, entry.name + ": seed_pos", torch.int64)
    assert len(batch.metas) == len(batch.eids) == len(blocks)
    for i, (meta, eid, (rp_b, col_b), weid) in enumerate(zip(batch.metas, batch.eids, blocks, eids)):
        what = "%s layer graph %d: " % (entry.name, i)
        _same(meta[0], rp_b, what + "nodePointer_b"); _same(meta[1], col_b, what + "edgeList_b"); _same(eid, weid, what + "eid")
        for t, w, k in zip(meta[2:], graphs.host_sgt(rp_b, col_b)[:3], ("blockPartition", "edgeToColumn", "edgeToRow")):
            _same(t, w, what + k)
    return batch


# ---- (a) layers on blocks against dense fp64 ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layer", MB.LAYERS, ids=LAYER_IDS)
@pytest.mark.parametrize("entry", MB.CATALOGUE, ids=ENTRY_IDS)
def test_layer_on_a_block_against_the_dense_fp64_model(dev, T, entry, layer):
    """Bounds: minibatch_ref.LAYERS (each the one the layer's own GPU test applies); tests/test_minibatch_cpu.py shows that operand
    rounding alone stays within half of them on these inputs and that a backward pass through A would not pass.  On `isolated_seed`
    (E = 0, null edge tensors) the call must return, Y is the empty-sum value and every gradient the dense model's."""
    import tcgnn_edge_ops as E
    import tcgnn_layers as L
    batch = _batch(dev, entry)
    nodes, _, _, blocks, eids = entry.host()
    M = len(nodes)
    names = ["Y"] + layer.leaf_names()
    failures = []
    for i, ((rp_b, col_b), eid) in enumerate(zip(blocks, eids)):
        meta = batch.metas[i]
        what = "%s %s layer graph %d" % (entry.name, layer.name, i)
        ctx = MB.block_context(rp_b, col_b)
        leaves, dY = layer.leaves(entry.name, M, eid)
        lv = [t.clone().requires_grad_(True) for t in leaves]
        Yd = layer.dense(ctx, lv)
        want = dict(zip(names, [Yd.detach()] + MB.gradients(Yd, dY, lv)))
        module = layer.make(L)
        layer.assign(module, leaves)
        module = module.to(dev)
        params = [getattr(module, a) for a, _, _ in layer.attrs]
        inputs = [t.float().to(dev).requires_grad_(True) for t in leaves[:len(leaves) - len(params)]]
        Y = module(inputs[0], *meta, **({"edge_attr": inputs[1]} if layer.name == "gine" else {}))
        got = dict(zip(names, [Y.detach()] + MB.gradients(Y, dY.float().to(dev), inputs + params)))
        got = {k: v.reshape(want[k].shape) for k, v in got.items()}
        judged = list(names)
        extra = ""
        if layer.name == "agnn":   # the reference's d attention_w is not the model's gradient (minibatch_ref.agnn_reference_dw)
            judged.remove("attention_w")
            d_w, scale = MB.agnn_reference_dw(rp_b, col_b, dY)
            err = abs(float(got["attention_w"]) - d_w)
            extra = " d_attention_w %.3f" % (err / (MB.AGNN_DW_TOL * scale) if scale else float(err != 0))
            if err > MB.AGNN_DW_TOL * scale:
                failures.append("%s: d attention_w %.6g, the reference's formula gives %.6g (scale %.3g)" % (what, float(got["attention_w"]), d_w, scale))
        sh = MB.shares(layer, judged, got, want)
        lonely = torch.from_numpy(np.diff(rp_b) == 0).to(dev)
        if bool(lonely.any()) and not torch.equal(Y.detach()[lonely], layer.empty(module, inputs[0])[lonely]):
            failures.append("%s: a row without edges does not hold the empty sum's value" % what)
        if layer.name in ("sage_max", "pna"):   # the extrema stay exact
            X32 = inputs[0].detach()
            A, Xd = ctx.A, X32.double().cpu()
            has = A.sum(1, keepdim=True) > 0
            hi = torch.where(has, Xd.unsqueeze(0).expand(M, -1, -1).masked_fill((A == 0).unsqueeze(2), float("-inf")).max(1).values, torch.zeros((), dtype=torch.float64))
            lo = torch.where(has, Xd.unsqueeze(0).expand(M, -1, -1).masked_fill((A == 0).unsqueeze(2), float("inf")).min(1).values, torch.zeros((), dtype=torch.float64))
            if layer.name == "sage_max":
                exact = torch.equal(E.aggregate_max(X32, meta[0], meta[1]).double().cpu(), hi)
            else:
                st = E.aggregate_stats(X32, meta[0], meta[1], ("max", "min"))
                exact = torch.equal(st[0].double().cpu(), hi) and torch.equal(st[1].double().cpu(), lo)
            if not exact:
                failures.append("%s: an extremum is not exact" % what)
        kernels = (T.last_kernel(*meta), T.last_kernel(*meta, transpose=True)) if layer.plan_based else ("planless", "planless")
        print("FIG %-46s E %4d worst %.3f of its bound (%s)%s | forward %s | transposed %s"
              % (what, len(col_b), max(sh.values()), " ".join("%s %.3f" % (k, v) for k, v in sh.items()), extra, kernels[0] or "-", kernels[1] or "-"))
        failures += ["%s: %s uses %.3f of its bound" % (what, k, v) for k, v in sh.items() if not v <= 1.0]
    T.clear_plan_cache()
    assert not failures, "\n".join(failures)


# ---- (b) the operators the layers do not isolate ------------------------------------------------------------------------------------------

OP_BLOCKS = [("fanout_4_3", 0), ("fanout_4_3", 1), ("one_1_1", 0), ("one_1_1", 1), ("cluster_310", 0)]


def _scaled_refs(X, rp, col, meta, r, c):
    """(ref, r64, scale) of r * (A (c * X)): the TF32-mode oracle and the fp64 product on the scaled operand, as tests/test_gpu_structures.py forms them"""
    Xc = (c[:, None] * X).astype(np.float32)
    a = O.spmm(Xc, rp, col, *meta, round_mode=O.ROUND_TF32)
    a64, as64 = O.spmm_f64(Xc, rp, col)
    r64 = r[:, None].astype(np.float64)
    return (a * r[:, None]).astype(np.float32), a64 * r64, as64 * r64


@pytest.mark.parametrize("D", [16, 41, 64])
@pytest.mark.parametrize("block", OP_BLOCKS, ids=["%s-%d" % b for b in OP_BLOCKS])
def test_operators_on_a_block_against_the_fp64_products(dev, T, monkeypatch, block, D):
    import tcgnn_layers as L
    name, i = block
    entry = MB.ENTRIES[name]
    batch = _batch(dev, entry)
    meta = batch.metas[i]
    rp, col = entry.host()[3][i]
    M, nnz = len(rp) - 1, len(col)
    tag = "%s-%d D=%d" % (name, i, D)
    X, att = W.case_data(M, nnz, D)
    Z = np.random.default_rng(7 * D + M).standard_normal((M, D)).astype(np.float32)
    host = W.host_meta(rp, col)
    rp_t, col_t, perm = W.transposed_csr(rp, col)
    host_t = W.host_meta(rp_t, col_t)
    zero, zero_t = W.zero_rows(name, rp), W.zero_rows(name, rp_t)
    tX, tZ, tatt = _dev(dev, X), _dev(dev, Z), _dev(dev, att).view(1, -1)
    failures = []

    def judge(got, ref, r64, s64, what, z=None):
        failures.extend(W.judge(name, got.cpu().numpy(), ref, r64, s64, "%s %s" % (tag, what), z))

    # A^T X
    got = T.forward(tX, *meta, transpose=True)[0]
    judge(got, O.spmm(X, rp_t, col_t, *host_t, round_mode=O.ROUND_TF32), *O.spmm_f64(X, rp_t, col_t), "transposed (%s)" % T.last_kernel(*meta, transpose=True), zero_t)
    # the normalised aggregation with the block's own degree scales, forward and backward orientation
    tr, tc = L.degree_scales(meta[0], meta[1], "both")
    r, c = tr.cpu().numpy(), tc.cpu().numpy()
    assert np.allclose(r, np.maximum(np.diff(rp), 1) ** -0.5, rtol=1e-6, atol=0) and np.allclose(c, np.maximum(np.bincount(col, minlength=M), 1) ** -0.5, rtol=1e-6, atol=0)
    got = T.forward_scaled(tX, *meta, row_scale=tr, col_scale=tc)[0]
    judge(got, *_scaled_refs(X, rp, col, host, r, c), "scaled (%s)" % T.last_kernel(*meta), zero)
    got = T.forward_scaled(tX, *meta, row_scale=tc, col_scale=tr, transpose=True)[0]
    judge(got, *_scaled_refs(X, rp_t, col_t, host_t, c, r), "scaled transposed (%s)" % T.last_kernel(*meta, transpose=True), zero_t)
    # the edge-valued aggregation and its transpose
    got = T.forward_AGNN(tX, meta[0], meta[1], tatt, *meta[2:])[0]
    judge(got, O.spmm_val(X, rp, col, att, *host, round_mode=O.ROUND_TF32), *O.spmm_f64(X, rp, col, att), "edge-valued (%s)" % T.last_kernel(*meta), zero)
    got = T.forward_AGNN(tX, meta[0], meta[1], tatt, *meta[2:], transpose=True)[0]
    att_t = np.ascontiguousarray(att[perm])
    judge(got, O.spmm_val(X, rp_t, col_t, att_t, *host_t, round_mode=O.ROUND_TF32), *O.spmm_f64(X, rp_t, col_t, att_t),
          "edge-valued transposed (%s)" % T.last_kernel(*meta, transpose=True), zero_t)
    # the two SDDMMs
    got = T.forward_ef(tX, *meta)[0]
    judge(got, O.sddmm(X, rp, col, *host, round_mode=O.ROUND_TF32), *O.sddmm_f64(X, rp, col), "sddmm (%s)" % T.last_kernel(*meta))
    got = T.forward_ef2(tX, tZ, *meta)[0]
    judge(got, EO.sddmm2_tf32(X, Z, rp, col)[0], *EO.sddmm2_f64(X, Z, rp, col), "sddmm2 (%s)" % T.last_kernel(*meta))
    if name == "fanout_4_3":   # the staged fp16 walk, forced: automatic routing never takes it on a block this small
        def body():
            Y = T.forward(tX, *meta)[0]
            k = T.last_kernel(*meta)
            return Y, k, T.forward_AGNN(tX, meta[0], meta[1], tatt, *meta[2:])[0], T.last_kernel(*meta)
        Y, k, Yv, kv = W.forced(T, monkeypatch, W.FORWARD_WALKS["per_window"][0], {}, body, {"n": M, "D": D, "capfd": None})
        if not (W.FORWARD_WALKS["per_window"][2](k) and W.AGNN_WALKS["per_window"][2](kv)):
            failures.append("%s: mode 1 ran %r / %r" % (tag, k, kv))
        judge(Y, O.spmm(X, rp, col, *host, round_mode=O.ROUND_TF32), *O.spmm_f64(X, rp, col), "forward per_window (%s)" % k, zero)
        judge(Yv, O.spmm_val(X, rp, col, att, *host, round_mode=O.ROUND_TF32), *O.spmm_f64(X, rp, col, att), "edge-valued per_window (%s)" % kv, zero)
    T.clear_plan_cache()
    assert not failures, "\n".join(failures)


# ---- (c) the harness ----------------------------------------------------------------------------------------------------------------------

MODELS = ("gin", "agnn", "gat", "gatv2", "transformer", "pna", "gine")
CHECKS = ("dense-vs-rows", "saint-twice", "cluster-twice")


def _harness_args(model, seen, within, T, *flags):
    import tcgnn_harness as H
    heads = ["--heads", "2"] if model in ("gat", "gatv2", "transformer") else []
    args = H.build_parser().parse_args(["--synthetic", "citeseer", "--dim", "16", "--hidden", "16", "--classes", "4", "--epochs", "1", "--gpu_preprocess",
                                        "--model", model] + heads + list(flags))

    def hook(epoch, index, seeds):
        seen.append((epoch, index, seeds.cpu()))
        s = T.cache_stats()
        within.append(s["plans"] <= 4 and s["csrs"] <= 8)
    args.batch_hook = hook
    return args


@pytest.mark.parametrize("check", CHECKS)
@pytest.mark.parametrize("model", MODELS)
def test_harness_trains_every_other_model_on_mini_batches(dev, T, model, check):
    import tcgnn_harness as H
    flags = {"dense-vs-rows": (("--fanout", "5,3", "--batch-size", "512", "--sampler", "dense"), ("--fanout", "5,3", "--batch-size", "512", "--sampler", "rows")),
             "saint-twice": (("--sampler", "saint", "--batch-size", "512", "--walk-length", "2"),) * 2,
             "cluster-twice": (("--sampler", "cluster", "--batch-size", "512"),) * 2}[check]
    T.clear_plan_cache()
    T.set_plan_cache_size(4)
    try:
        runs, seen, within = [], ([], []), []
        for f, s in zip(flags, seen):
            runs.append(H.run(_harness_args(model, s, within, T, *f), quiet=True))
        stats = T.cache_stats()
    finally:
        T.set_plan_cache_size(8)
        T.clear_plan_cache()
    a, b = runs
    print("FIG harness %-11s %-13s final_loss %.6f sampled_loss %.6f batches %d mean block nodes %.0f" %
          (model, check, a["final_loss"], a["sampled_loss"], a["batches"], a["mean_block_nodes"]))
    assert a["batches"] == (3327 + 511) // 512 and len(seen[0]) == len(seen[1]) == a["batches"]
    assert np.isfinite(a["final_loss"]) and np.isfinite(a["sampled_loss"])
    assert b["final_loss"] == a["final_loss"] and b["sampled_loss"] == a["sampled_loss"], (a["final_loss"], b["final_loss"], a["sampled_loss"], b["sampled_loss"])
    assert all(torch.equal(x[2], y[2]) for x, y in zip(*seen)), "the two runs drew other batches"
    assert all(within) and stats["plans"] <= 4 and stats["csrs"] <= 8, stats
