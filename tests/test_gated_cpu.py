"""Without a GPU: gated_ref's restatement against autograd of the fp64 composition, and aggregate_gated's identity dk = dY * S."""
import types

import numpy as np
import torch

import gated_ref as R
import graphs


def _case():
    rp, col = graphs.uniform_graph(300, 5, seed=7, symmetric=False)
    rng = np.random.default_rng(3)
    k, q, v, dY = ((s * rng.standard_normal((len(rp) - 1, 7))).astype(np.float32) for s in (4.0, 4.0, 1.0, 1.0))
    hi = [torch.from_numpy(t.astype(np.float64)).requires_grad_(True) for t in (k, q, v)]
    want = R.dense_f64(rp, col, *hi)
    grads = torch.autograd.grad((want * torch.from_numpy(dY.astype(np.float64))).sum(), hi)
    return rp, col, (k, q, v, dY), want.detach().numpy(), [g.numpy() for g in grads]


def test_the_restatement_is_the_fp64_composition_and_its_autograd_gradients():   # (z rounded to fp32 first: within EPS_GATE)
    rp, col, (k, q, v, dY), want, (dk, dq, dv) = _case()
    r = R.gated_f64(rp, col, k, q, v, dY)
    r["dk"] = (dY.astype(np.float64) * r["S"][0], np.abs(dY) * r["S"][1])
    for name, ref in (("Y", want), ("dk", dk), ("dq", dq), ("dv", dv)):
        assert np.abs(ref).max() > 0.1 and R.worst_share(ref, *r[name]) <= 1.0, name


def test_aggregate_gated_forms_dk_as_dy_times_s():
    import tcgnn_edge_ops as E
    import tcgnn_layers as L
    rp, col, (k, q, v, dY), _, _ = _case()
    r = R.gated_f64(rp, col, k, q, v, dY)
    t64 = lambda name: torch.from_numpy(r[name][0])   # noqa: E731
    old = L._backend
    L.set_backend(types.SimpleNamespace(forward_gated=lambda *a: (t64("Y"), t64("S")), source_grad_gated=lambda *a: (t64("dq"), t64("dv"))))
    try:
        leaves = [torch.from_numpy(t.astype(np.float64)).requires_grad_(True) for t in (k, q, v)]
        Y = E.aggregate_gated(*leaves, torch.from_numpy(rp), torch.from_numpy(col))
        got = torch.autograd.grad((Y * torch.from_numpy(dY.astype(np.float64))).sum(), leaves)
    finally:
        L.set_backend(old)
    assert np.array_equal(got[0].numpy(), dY.astype(np.float64) * r["S"][0])
    assert all(np.array_equal(g.numpy(), r[name][0]) for g, name in zip(got[1:], ("dq", "dv")))
