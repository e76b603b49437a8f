"""Plain fp64 restatement of GatedGCN's aggregation with edge features (tcgnn_gatedgcn_forward / _backward / _source_grad), in numpy for the
kernels and in torch - differentiable - for the operator and the layer.  Used by tests/test_gpu_gatedgcn.py; no GPU needed to import.

Z is formed in fp32 exactly as the contract says, ((k[row] + q[col]) + c), and compared bit for bit; everything behind it is fp64 and starts
from that fp32 Z.  The bounds are the project's: 1e-5 of the reference's largest entry for Y and Den, 1e-4 for gradients."""
import numpy as np

import gated_ref as R

VALUE_BOUND, GRAD_BOUND = 1e-5, 1e-4
BOUNDS = {"Y": VALUE_BOUND, "Den": VALUE_BOUND, "G": GRAD_BOUND, "dk": GRAD_BOUND, "dq": GRAD_BOUND, "dv": GRAD_BOUND}


def inputs(n, E, D, scale, seed=31):
    """{k, q, v, dY: fp32 [n, D]; c, dZ: fp32 [E, D]}, standard normal; k, q, v and c times `scale`"""
    rng = np.random.default_rng([seed, D])
    t = {name: rng.standard_normal((E if name in ("c", "dZ") else n, D)).astype(np.float32) for name in ("k", "q", "v", "c", "dY", "dZ")}
    for name in ("k", "q", "v", "c"):
        t[name] *= np.float32(scale)
    return t


def gatedgcn_f64(rp, col, t, eps):
    """{Z: fp32 [E, D]; Y, Den, dk, dq, dv: fp64 [n, D]; G: fp64 [E, D]} for the inputs of inputs(); eps as the C call widens it"""
    n, rows, cols, eps = len(rp) - 1, R.edge_rows(rp), np.asarray(col[:int(rp[-1])], np.int64), float(np.float32(eps))
    Z = ((t["k"][rows] + t["q"][cols]).astype(np.float32) + t["c"]).astype(np.float32)
    z, v, dY = Z.astype(np.float64), t["v"].astype(np.float64), t["dY"].astype(np.float64)
    e = np.exp(-np.abs(z))
    eta, cc = np.where(z >= 0, 1.0, e) / (1.0 + e), np.where(z >= 0, e, 1.0) / (1.0 + e)
    den = R._sum_by(rows, eta, n)
    s = den + eps
    live = s > 0
    Y = np.where(live, R._sum_by(rows, eta * v[cols], n) / np.where(live, s, 1.0), 0.0)
    u = np.where(live, dY / np.where(live, s, 1.0), 0.0)
    G = t["dZ"].astype(np.float64) + eta * cc * u[rows] * (v[cols] - Y[rows])
    return {"Z": Z, "Y": Y, "Den": den, "G": G, "dk": R._sum_by(rows, G, n), "dq": R._sum_by(cols, G, n), "dv": R._sum_by(cols, eta * u[rows], n)}


def share(got, ref, bound):   # max |got - ref| over bound * max |ref|; anything not finite counts as infinite
    got = np.asarray(got, np.float64)
    return float(np.abs(got - ref).max() / (bound * np.abs(ref).max())) if np.isfinite(got).all() else np.inf


def dense_f64(rp, col, k, q, v, c, eps):   # torch's plain composition -> (Y, Z)
    import torch
    rows, cols = torch.from_numpy(R.edge_rows(rp)), torch.from_numpy(np.asarray(col[:int(rp[-1])], np.int64))
    Z = k[rows] + q[cols] + c
    eta = torch.sigmoid(Z)
    return torch.zeros_like(k).index_add_(0, rows, eta * v[cols]) / (torch.zeros_like(k).index_add_(0, rows, eta) + eps), Z
