"""Fused attention with edge features without a GPU: the three symbols are declared, exported and bound, the layer refuses what it cannot
serve, and the restated contract with ee = 0 is the one without edges."""
import inspect
import os
import re

import numpy as np
import pytest

import attn_edge_ref as R
import attn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("symbol,arity,python,params", [("tcgnn_attn_edge_forward", 14, "forward_attn_edge", 7), ("tcgnn_attn_edge_backward", 19, "backward_attn_edge", 10),
                                                        ("tcgnn_attn_edge_source_grad", 14, "source_grad_attn_edge", 6)])
def test_the_symbols_are_declared_exported_and_bound_with_the_right_arity(symbol, arity, python, params):
    import TCGNN
    import tcgnn_capi as C
    header = open(os.path.join(ROOT, "include", "tcgnn.h")).read()
    declared = re.search(r"\bint %s\(([^;]*)\);" % symbol, header)
    assert declared and len(declared.group(1).split(",")) == arity == len(C.SIGNATURES[symbol][1]) and hasattr(C.lib, symbol)
    required = [p for p in inspect.signature(getattr(TCGNN, python)).parameters.values() if p.default is p.empty]
    assert python in TCGNN.__all__ and len(required) == params
    assert 'm.def("%s"' % python in open(os.path.join(ROOT, "integration", "TCGNN_binding.cpp")).read()


def test_the_layer_refuses_edges_without_the_fused_walk_and_a_gate_without_a_root_term():
    import tcgnn_layers as L
    with pytest.raises(ValueError):
        L.TransformerConv(8, 4, edge_dim=4)
    with pytest.raises(ValueError):
        L.TransformerConv(8, 4, beta=True, root_weight=False)
    conv = L.TransformerConv(8, 4, heads=2, fused=True, edge_dim=4, beta=True)
    assert tuple(conv.weights_edge.shape) == (4, 8) and tuple(conv.weights_beta.shape) == (24, 1)


def test_the_reference_with_a_zero_edge_vector_is_the_reference_without_edges():
    rp, col = R.row_class_graphs()["A"]
    q, k, v, dY, ee = R.inputs("normal_x1", rp, col, 3, 5)
    with_edges, without = R.attn_edge_f64(rp, col, q, k, v, dY, np.zeros_like(ee), 3, 0.5), attn_ref.attn_f64(rp, col, q, k, v, dY, 3, 0.5)
    # (dk is left out: attn_ref's source call is handed fl32(delta) and forms g from it, this one is handed g itself)
    assert all(np.array_equal(with_edges[name][0], without[name][0]) for name in ("Y", "L", "delta", "dq", "dv"))
