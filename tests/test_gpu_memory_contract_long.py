"""The C ABI's memory contract (tests/test_gpu_memory_contract.py has the rules) for the long flat walk - 952-row ranges, forced with
TCGNN_LDS_LONG=1 as tests/test_gpu_long_ranges.py forces it: tcgnn_spmm and tcgnn_spmm_scaled through ctypes with a workspace of exactly
tcgnn_workspace_bytes between moats, outputs between moats pre-filled with NaN, guarded inputs; one byte less is refused with
everything untouched.  The ctypes path only: the module's path is judged in tests/test_gpu_long_ranges.py.  Needs an MI355X."""
import re

import numpy as np
import pytest
import torch

import long_range_graphs as LG
import test_gpu_memory_contract as M
import walks as W

pytestmark = pytest.mark.gpu

NAMES = ("pool_every_cell_overflows_n4760", "range_arithmetic_n1905")
GRAPHS = {name: (rp, col) for name, rp, col in LG.catalogue() if name in NAMES}
LONG = {"TCGNN_LDS_FLAT": "1", "TCGNN_LDS_LONG": "1"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def T():
    import TCGNN
    return TCGNN


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_on_the_device(T):
    """the graphs of this file leave the shared module's caches, and the device, when its tests are over"""
    yield
    M._META.clear()
    M._CACHE.clear(); M._CACHE["key"] = None
    W._REFS.clear()
    T.clear_plan_cache()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name,D", [(NAMES[0], 64), (NAMES[0], 96), (NAMES[1], 64), (NAMES[1], 41)])
def test_long_walk_keeps_the_memory_contract(dev, T, monkeypatch, capfd, name, D):
    monkeypatch.setitem(M.GRAPHS, name, GRAPHS[name])      # (Case looks its graph up there; undone when the test ends)
    cs = M.Case(dev, T, monkeypatch, name, D)
    lib = cs.lib
    ref, (X, _), (bp, e2c, e2r) = W.references(name, cs.rp, cs.col, D, ops=("spmm",))
    rng = np.random.default_rng(5)
    r = rng.uniform(0.1, 1.0, cs.n).astype(np.float32); b = rng.standard_normal(D).astype(np.float32)
    monkeypatch.setenv("TCGNN_VERBOSE", "1")
    capfd.readouterr()

    def body():
        plan = cs.plan()
        try:
            build = lambda p, ws, nb: (plan, p["X"], p["Y"], D, ws, nb, cs.stream)   # noqa: E731
            out = cs.call("tcgnn_spmm (long ranges)", lib.tcgnn_spmm, build, {"Y": ((cs.n, D), M.F32)}, {"X": X}, cs.ws_bytes(plan))
            kernel = cs.kernel(plan)
            if out is not None and cs.written("tcgnn_spmm (long ranges)", "Y", out["Y"]):
                cs.judge("forward long ranges D=%d (%s)" % (D, kernel), out["Y"], ref["spmm"], cs.zero)
            # the _epi_ twin: row scale and bias in the kernel's own store
            sbuild = lambda p, ws, nb: (plan, p["X"], None, None, p["rs"], p["bias"], p["Y"], D, 0, ws, nb, cs.stream)   # noqa: E731
            sout = cs.call("tcgnn_spmm_scaled (long ranges)", lib.tcgnn_spmm_scaled, sbuild, {"Y": ((cs.n, D), M.F32)}, {"X": X, "rs": r, "bias": b}, cs.ws_bytes(plan))
            if sout is not None and cs.written("tcgnn_spmm_scaled (long ranges)", "Y", sout["Y"]) and out is not None:
                want = (out["Y"] * torch.from_numpy(r).to(dev)[:, None]) + torch.from_numpy(b).to(dev)
                cs.same("tcgnn_spmm_scaled (long ranges)", sout["Y"], want, "row scale and bias applied to tcgnn_spmm's result")
            return kernel
        finally:
            cs.destroy(plan)
            cs.end_of_walk("long ranges")
    try:
        kernel = W.forced(T, monkeypatch, 3, LONG, body, cs.ctx)
    finally:
        monkeypatch.delenv("TCGNN_VERBOSE", raising=False)
    cs.end_of_case()
    err = capfd.readouterr().err
    W._REFS.clear()
    assert kernel == "spmm_lds_flat_kernel", kernel
    assert re.search(r"cell stream 7 \(8 windows per wavefront, 952-row ranges\)", err) and "cell stream 4 (" not in err, err[-800:]
    assert not cs.fail, "\n".join(cs.fail)
