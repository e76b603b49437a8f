"""The mini-batch catalogue and the layer table of tests/minibatch_ref.py without a GPU: what every catalogue entry is there for, pinned;
the conditions the dense fp64 references must meet before tests/test_gpu_minibatch.py may judge a kernel with them - operand rounding
alone within half of every bound, a backward pass through the wrong matrix far outside it, not every row empty; and the layers that
have a pure-torch backend run through it on every entry, against the dense models."""
import numpy as np
import pytest
import torch

import edge_message_ref as EM
import gatv2_ref as V
import minibatch_ref as MB

ENTRY_IDS = [e.name for e in MB.CATALOGUE]
LAYER_IDS = [c.name for c in MB.LAYERS]


def test_every_entry_is_what_it_is_in_the_catalogue_for():
    rp, col = MB.full_graph()
    assert len(rp) - 1 == 1500 and not np.diff(rp)[96:112].any() and (col == 100).any()      # (node 100: no in-edges, still a source)
    for e in MB.CATALOGUE:
        nodes, new_id, seed_pos, blocks, eids = e.host()
        facts = MB.block_facts(nodes, blocks)
        print("FACTS %-14s M %4d (M %% 16 = %2d)  E %s  rows with edges %s  empty windows %s of %d  symmetric %s"
              % (e.name, facts["M"], facts["M"] % 16, facts["E"], facts["rows"], facts["empty_windows"], (facts["M"] + 15) // 16, facts["symmetric"]))
        assert facts == MB.FACTS[e.name], (e.name, facts)
        assert all(len(eid) == len(b[1]) and len(b[0]) == len(nodes) + 1 for b, eid in zip(blocks, eids))
        assert np.array_equal(nodes[seed_pos], np.asarray(e.ids).reshape(-1)[:len(seed_pos)]) or e.kind == "saint"
    F = MB.FACTS
    assert F["fanout_4_3"]["M"] % 16 and F["fanout_4_3"]["empty_windows"][1] >= 10                       # ragged last window, empty windows between
    assert F["fanout_5_3_2"]["empty_windows"][2] * 2 >= (F["fanout_5_3_2"]["M"] + 15) // 16               # half of the last layer's windows
    assert F["one_1_1"]["M"] < 16 and all(0 < n < 4 for n in F["one_1_1"]["E"])                           # below the tile paths' 4-edge limit
    assert F["isolated_seed"]["M"] == 1 and F["isolated_seed"]["E"] == [0, 0]
    assert F["few_2_2"]["M"] > 16 and F["saint_40x2"]["M"] % 16
    # every block with edges is directed, but the one a symmetric graph induces on a range of ids
    assert [k for k, f in F.items() if any(s and n for s, n in zip(f["symmetric"], f["E"]))] == ["cluster_310"]
    assert set(MB.INSENSITIVE) == {"isolated_seed", "cluster_310"}


def _evaluate(layer, ctx, leaves, dY, **kw):
    lv = [t.clone().requires_grad_(True) for t in leaves]
    Y = layer.dense(ctx, lv, **kw)
    return dict(zip(["Y"] + layer.leaf_names(), [Y.detach()] + MB.gradients(Y, dY, lv)))


@pytest.mark.parametrize("layer", MB.LAYERS, ids=LAYER_IDS)
@pytest.mark.parametrize("entry", MB.CATALOGUE, ids=ENTRY_IDS)
def test_the_reference_alone_meets_the_conditions_of_the_gpu_test(entry, layer):
    """On every layer graph with edges: (rounding) the dense model with its aggregation operands rounded as the kernels round them is
    within HALF of every bound of the unrounded one, where the model has that switch; (sensitivity) the input gradient through the wrong
    matrix - minibatch_ref.wrong_matrix_mode, or the reversed block for the gather-based layers - is beyond TEN times the input
    gradient's bound, except on the entries minibatch_ref.INSENSITIVE names; (empty rows) not every output row is without edges."""
    nodes, _, _, blocks, eids = entry.host()
    names = ["Y"] + layer.leaf_names()
    for i, ((rp_b, col_b), eid) in enumerate(zip(blocks, eids)):
        empty_share = float((np.diff(rp_b) == 0).mean())
        what = "%s %s layer graph %d" % (entry.name, layer.name, i)
        if len(col_b) == 0:
            assert entry.name == "isolated_seed" and empty_share == 1.0
            leaves, dY = layer.leaves(entry.name, len(nodes), eid)
            want = _evaluate(layer, MB.block_context(rp_b, col_b), leaves, dY)      # (the dense model itself takes a block without edges)
            assert all(bool(torch.isfinite(v).all()) for v in want.values())
            print("COND %-44s no edges" % what)
            continue
        assert empty_share < 1.0
        ctx = MB.block_context(rp_b, col_b)
        leaves, dY = layer.leaves(entry.name, len(nodes), eid)
        want = _evaluate(layer, ctx, leaves, dY)
        rounding = None
        if layer.rounds:
            rounded = _evaluate(layer, ctx, leaves, dY, round_operands=True)
            rounding = max(MB.shares(layer, names, rounded, want).values())
        if layer.wrong == "mode":
            with MB.wrong_matrix_mode(ctx.A):
                wrong = _evaluate(layer, ctx, leaves, dY)
            assert MB.share("largest", 1e-12, wrong["Y"], want["Y"]) <= 1.0, "the wrong-matrix mode changed the forward pass"
        else:
            back, perm = MB.reversed_context(ctx)
            lv = list(leaves)
            if layer.name == "gine":
                lv[1] = leaves[1][torch.from_numpy(perm)]
            wrong = _evaluate(layer, back, lv, dY)
        metric, bound = layer.check("X")
        sensitivity = MB.share(metric, bound, wrong["X"], want["X"])
        print("COND %-44s rounding %s of the bound, wrong matrix %.3g x the bound, rows without edges %.2f"
              % (what, "n/a" if rounding is None else "%.3f" % rounding, sensitivity, empty_share))
        assert rounding is None or rounding <= 0.5, "%s: operand rounding alone uses %.3f of a bound" % (what, rounding)
        assert sensitivity > 10.0 or entry.name in MB.INSENSITIVE, "%s: a backward pass through A would pass (%.3g x the bound)" % (what, sensitivity)


class _GatBackend(V.TorchBackend):
    """gatv2_ref's pure-torch backend (gat_ref's plus the GATv2 calls), its edge_softmax taking out= as the product's does"""

    def edge_softmax(self, s, rp, beta=None, out=None):
        return super().edge_softmax(s, rp, beta)


@pytest.fixture()
def backend():
    import tcgnn_layers as L
    old = L._backend

    def install(b):
        L.set_backend(b)
        return b
    yield install
    L.set_backend(old)


@pytest.mark.parametrize("name", ["gat", "gatv2", "gine"])
@pytest.mark.parametrize("entry", MB.CATALOGUE, ids=ENTRY_IDS)
def test_layers_with_a_torch_backend_equal_the_dense_models_on_every_entry(backend, entry, name):
    """the layer itself, in fp64 on the pure-torch backend of its family, against the dense model: the catalogue, the leaves and the
    dense models agree before a kernel is involved (E = 0 included: the call returns, the output is the bias row)"""
    import tcgnn_layers as L
    backend(EM.TorchBackend() if name == "gine" else _GatBackend())
    layer = MB.LAYER[name]
    nodes, _, _, blocks, eids = entry.host()
    names = ["Y"] + layer.leaf_names()
    for (rp_b, col_b), eid in zip(blocks, eids):
        ctx = MB.block_context(rp_b, col_b)
        leaves, dY = layer.leaves(entry.name, len(nodes), eid)
        want = _evaluate(layer, ctx, leaves, dY)
        module = layer.make(L).double()
        params = layer.assign(module, leaves)
        for p, leaf in zip(params, leaves[len(leaves) - len(params):]):
            p.data.copy_(leaf.reshape(p.shape))            # (fp64 leaves, not their fp32 roundings)
        inputs = [t.clone().requires_grad_(True) for t in leaves[:len(leaves) - len(params)]]
        meta = (torch.from_numpy(rp_b), torch.from_numpy(col_b), None, None, None)
        Y = module(inputs[0], *meta, **({"edge_attr": inputs[1]} if name == "gine" else {}))
        got = dict(zip(names, [Y.detach()] + MB.gradients(Y, dY, inputs + params)))
        for k in names:
            g, w = got[k].reshape(want[k].shape), want[k]
            assert MB.share("unit", 1e-9, g, w) <= 1.0, (entry.name, name, k)
        lonely = torch.from_numpy(np.diff(rp_b) == 0)
        if bool(lonely.any()):
            assert torch.allclose(Y.detach()[lonely], layer.empty(module, inputs[0])[lonely], rtol=0, atol=1e-12)
