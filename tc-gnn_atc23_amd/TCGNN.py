"""`TCGNN` - drop-in replacement of the reference's PyTorch extension module of the same name.

Same seven names, same positional signatures, same return shapes as the pybind11 module built from
TCGNN_conv/TCGNN.cpp:260-272, so the reference's gnn_conv.py / main_tcgnn.py import and call it
unchanged (`import TCGNN`):

    preprocess(edgeList, nodePointer, num_nodes, blockSize_h, blockSize_w,
               blockPartition, edgeToColumn, edgeToRow) -> None        TCGNN.cpp:172
    preprocess_gpu(... same, CUDA tensors ...)              -> None        TCGNN.cpp:229
    forward(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow) -> [Y]    :63
    forward_ef(...same six...)                                                    -> [ef]   :126
    forward_AGNN(input, nodePointer, edgeList, edgeAttention, blockPartition,
                 edgeToColumn, edgeToRow)                                         -> [Y]    :93
    backward = forward, backward_ef = forward_ef                                            :270-271

Behind it sits the C ABI of include/tcgnn.h (libtcgnn_hip.so, hand-written gfx950 kernels).  Torch
is only plumbing here: device memory, the current HIP stream, tensor lifetime.  There is no CPU or
eager fallback; a missing library fails at import.

Differences from the reference that a caller can observe (all supersets):
  * any embedding_dim is computed in full (the reference leaves columns >= 16*min(D//16, 8) zero),
  * launch errors raise RuntimeError instead of printf + exit(-1) (TCGNN_kernel.cu:211-217),
  * kernels run on torch's current stream (the reference uses the legacy default stream and, for
    forward_AGNN, a leaked stream per call, TCGNN_kernel.cu:245-255),
  * preprocess never writes past the end of blockPartition when num_nodes % blockSize_h == 0.
"""
import collections
import os
import sys

import torch

import tcgnn_capi as _c

__all__ = ["preprocess", "preprocess_gpu", "forward", "forward_ef", "forward_AGNN", "backward", "backward_ef",
           "plan_info", "kernel_timing", "last_kernel", "clear_plan_cache", "set_plan_cache_size", "agnn_fused_supported", "agnn_fused_forward", "agnn_fused_backward",
           "forward_fused", "forward_gemm", "forward_scaled", "degree_scales", "transpose_graph",
           "forward_ef2", "edge_softmax", "edge_softmax_backward", "gat_softmax", "gat_softmax_backward", "edge_colsum"]

_plan_cache_size = max(1, int(os.environ.get("TCGNN_PLAN_CACHE_SIZE", "8")))
_plans = collections.OrderedDict()  # key -> (handle, tensors kept alive, device index)
_retired = []                       # evicted plans waiting for the kernels that may still read them: (events, handle, tensors)
_workspaces = {}                    # (device index, stream id) -> uint8 tensor
_scales = {}                        # (nodePointer, edgeList) key -> (tensors kept alive, {norm: (row_scale, col_scale)}): degree_scales
_transposed_csr = {}                # (nodePointer, edgeList) key -> (nodePointer, edgeList, nodePointer_t, edgeList_t, perm, symmetric): transpose_graph
_transposed = {}                    # A's plan key -> dict(plan=, own=, meta=, perm=, symmetric=): what transpose=True calls run on, evicted with A's plan
_values_t = {}                      # (device index, stream id) -> fp32 buffer: edge values in A^T's order (forward_AGNN(transpose=True))
_softmax_scratch = {}               # (device index, stream id) -> uint8 buffer: the fp64 partials of edge_softmax_backward's d_beta


def set_plan_cache_size(n):
    """Plans (packed tile streams, ~3x the CSR's bytes each) kept per process; the least recently used one beyond this is
    retired.  A mini-batch loop over k graphs wants n >= k.  Also the environment variable TCGNN_PLAN_CACHE_SIZE."""
    global _plan_cache_size
    _plan_cache_size = max(1, int(n))
    _evict()


def _reap(block=False):
    """Destroy retired plans whose last possible reader has finished (stream-ordered: an event per stream this module has
    launched on for that device, recorded at eviction time; nothing is synchronised unless block=True)."""
    keep = []
    for events, handle, tensors in _retired:
        if block:
            for e in events:
                e.synchronize()
        if all(e.query() for e in events):
            _c.lib.tcgnn_plan_destroy(handle)
        else:
            keep.append((events, handle, tensors))
    _retired[:] = keep


def _evict():
    while len(_plans) > _plan_cache_size:
        key, (old, keep, dev_index) = _plans.popitem(last=False)
        _drop_scales()
        tr = _transposed.pop(key, None)
        _drop_transposed_csr()
        events = []
        for (d, stream_id) in list(_workspaces):
            if d == dev_index:   # the streams this module has launched kernels on, on the EVICTED plan's device
                with torch.cuda.device(d):
                    e = torch.cuda.Event()
                    e.record(torch.cuda.ExternalStream(stream_id, device=d) if stream_id else torch.cuda.default_stream(d))
                    events.append(e)
        _retired.append((events, old, keep))
        if tr is not None and tr["own"] is not None:   # A^T's own plan (a graph that is not symmetric) leaves with A's
            _retired.append((events, tr["own"], tr["meta"]))
    if _retired:
        _reap()


# ---------------------------------------------------------------- argument checks (TCGNN.cpp:54-56)

def _check_input(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor" % name)
    if not t.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)


def _check_int(t, name):
    if t.dtype != torch.int32:  # libtorch's data<int>() raises the same way in the reference
        raise RuntimeError("expected scalar type Int but found %s (%s)" % (str(t.dtype).replace("torch.", "").capitalize(), name))


def _check_float(t, name):
    if t.dtype != torch.float32:
        raise RuntimeError("expected scalar type Float but found %s (%s)" % (str(t.dtype).replace("torch.", "").capitalize(), name))


def _stream_handle(device):
    return torch.cuda.current_stream(device).cuda_stream


# ---------------------------------------------------------------- plan cache

def _plan_key(tensors):
    return tuple((t.data_ptr(), t.numel(), t._version) for t in tensors) + (tensors[0].device.index,)


def _plan_for(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow):
    """The packed tile stream is a pure function of the five metadata tensors; it is built on the
    device the first time they are seen and reused while they are unchanged (storage address,
    length and in-place version counter).  The cache keeps the tensors alive, so an address can not
    be recycled under a live entry."""
    tensors = (nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    key = _plan_key(tensors)
    hit = _plans.get(key)
    if hit is not None:
        _plans.move_to_end(key)
        return hit[0]
    dev = nodePointer.device
    for t, n in zip(tensors, ("nodePointer", "edgeList", "blockPartition", "edgeToColumn", "edgeToRow")):
        _check_int(t, n)
        if t.device != dev:
            raise RuntimeError("%s is on %s but nodePointer is on %s" % (n, t.device, dev))
    N = nodePointer.numel() - 1
    E = edgeList.numel()
    if N < 0:
        raise RuntimeError("nodePointer must hold num_nodes + 1 entries")
    if edgeToColumn.numel() < E or edgeToRow.numel() < E:
        raise RuntimeError("edgeToColumn / edgeToRow are shorter than edgeList")
    handle = _c._vp()
    with torch.cuda.device(dev):
        st = _c.lib.tcgnn_plan_create(nodePointer.data_ptr(), edgeList.data_ptr(), blockPartition.data_ptr(),
                                      edgeToColumn.data_ptr(), edgeToRow.data_ptr(), N, E, blockPartition.numel(),
                                      _stream_handle(dev), _c.ctypes.byref(handle))
    _c.check(st, "tcgnn_plan_create")
    _plans[key] = (handle, tensors, dev.index)
    _evict()
    return handle


def clear_plan_cache():
    if torch.cuda.is_available():
        for d in {v[2] for v in _plans.values()}:
            torch.cuda.synchronize(d)
    while _plans:
        _, (old, _keep, _d) = _plans.popitem()
        _c.lib.tcgnn_plan_destroy(old)
    for tr in _transposed.values():
        if tr["own"] is not None:
            _c.lib.tcgnn_plan_destroy(tr["own"])
    _transposed.clear()
    _transposed_csr.clear()
    _values_t.clear()
    _softmax_scratch.clear()
    _reap(block=True)
    _workspaces.clear()
    _scales.clear()


# ---------------------------------------------------------------- the transposed graph (A^T)

def _drop_transposed_csr():
    """Transposed CSRs of graphs no cached plan uses any more leave with their plans (as the scales do)."""
    live = {k[:2] + (k[-1],) for k in _plans}
    for k in [k for k in _transposed_csr if k not in live]:
        del _transposed_csr[k]


def _scratch(nbytes, dev):
    """(tensor kept alive, 256-byte aligned address, usable bytes) of torch-allocator scratch for one library call"""
    ws = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=dev)
    return ws, ws.data_ptr() + (-ws.data_ptr()) % 256, int(nbytes)


def _transpose_csr(nodePointer, edgeList):
    """(nodePointer, edgeList, nodePointer_t, edgeList_t, perm, symmetric) - tcgnn_transpose_ws on torch-allocator scratch (one
    synchronisation), cached per graph like degree_scales."""
    for t, n in ((nodePointer, "nodePointer"), (edgeList, "edgeList")):
        _check_input(t, n)
        _check_int(t, n)
    if edgeList.device != nodePointer.device:
        raise RuntimeError("edgeList is on %s but nodePointer is on %s" % (edgeList.device, nodePointer.device))
    key = tuple((t.data_ptr(), t.numel(), t._version) for t in (nodePointer, edgeList)) + (nodePointer.device.index,)
    hit = _transposed_csr.get(key)
    if hit is not None:
        return hit
    N, E = nodePointer.numel() - 1, edgeList.numel()
    if N < 0:
        raise RuntimeError("nodePointer must hold num_nodes + 1 entries")
    dev = nodePointer.device
    with torch.cuda.device(dev):
        rp_t = torch.empty(N + 1, dtype=torch.int32, device=dev)
        col_t = torch.empty(E, dtype=torch.int32, device=dev)
        perm = torch.empty(E, dtype=torch.int32, device=dev)
        need = _c._sz(0)
        _c.check(_c.lib.tcgnn_transpose_workspace_bytes(N, E, _c.ctypes.byref(need)), "tcgnn_transpose_workspace_bytes")
        ws, ptr, nbytes = _scratch(need.value, dev)
        sym = _c._i32(0)
        st = _c.lib.tcgnn_transpose_ws(nodePointer.data_ptr(), edgeList.data_ptr(), N, E, rp_t.data_ptr(), col_t.data_ptr(), perm.data_ptr(),
                                       ptr, nbytes, _c.ctypes.byref(sym), _stream_handle(dev))
        del ws   # (the call synchronised the stream: nothing still reads it)
    _c.check(st, "tcgnn_transpose_ws")
    symmetric = bool(sym.value)
    if symmetric:   # A^T = A: its arrays are A's own
        rp_t, col_t = nodePointer, edgeList
    entry = (nodePointer, edgeList, rp_t, col_t, perm, symmetric)
    _transposed_csr[key] = entry
    while len(_transposed_csr) > _plan_cache_size:   # (a graph never handed to the kernels has no plan to leave with)
        _transposed_csr.pop(next(iter(_transposed_csr)))
    return entry


def transpose_graph(nodePointer, edgeList):
    """Not in the reference module: the CSR of A^T on the device, (nodePointer_t, edgeList_t, perm, symmetric).  Row c of A^T lists
    the rows r of every entry (r, c) of A in increasing CSR position (sorted; A's duplicates kept); perm[eT] = the CSR position in A
    of A^T's entry eT; symmetric = A^T has exactly A's arrays (then nodePointer_t / edgeList_t ARE nodePointer / edgeList).  Column
    ids must lie in [0, num_nodes).  Built on the GPU (tcgnn_transpose_ws) and cached beside the graph's plan: the transpose=True
    calls use the same entry."""
    return _transpose_csr(nodePointer, edgeList)[2:]


def _transposed_for(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow):
    """What transpose=True calls run on, built at first use and kept beside A's plan (and evicted with it): dict(plan = the plan of
    A^T - A's own when the graph is symmetric -, own = that plan when it is A^T's own else None, meta = A^T's five metadata tensors,
    perm, symmetric).  A^T's metadata: the transpose, the device SGT on torch-allocator scratch, tcgnn_plan_create."""
    tensors = (nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    plan = _plan_for(*tensors)
    key = _plan_key(tensors)
    hit = _transposed.get(key)
    if hit is not None:
        return hit
    _, _, rp_t, col_t, perm, symmetric = _transpose_csr(nodePointer, edgeList)
    if symmetric:
        entry = dict(plan=plan, own=None, meta=tensors, perm=perm, symmetric=True)
    else:
        dev = nodePointer.device
        N, E, bp_len = nodePointer.numel() - 1, edgeList.numel(), blockPartition.numel()
        with torch.cuda.device(dev):
            bp_t = torch.zeros(bp_len, dtype=torch.int32, device=dev)
            e2c_t = torch.empty(E, dtype=torch.int32, device=dev)
            e2r_t = torch.empty(E, dtype=torch.int32, device=dev)
            need = _c._sz(0)
            _c.check(_c.lib.tcgnn_preprocess_gpu_workspace_bytes(N, E, 16, _c.ctypes.byref(need)), "tcgnn_preprocess_gpu_workspace_bytes")
            ws, ptr, nbytes = _scratch(need.value, dev)
            tc = _c._i64(0)
            st = _c.lib.tcgnn_preprocess_gpu_ws(col_t.data_ptr(), rp_t.data_ptr(), N, E, 16, 8, bp_t.data_ptr(), bp_len, e2c_t.data_ptr(),
                                                e2r_t.data_ptr(), ptr, nbytes, _c.ctypes.byref(tc), _stream_handle(dev))
            del ws
            _c.check(st, "tcgnn_preprocess_gpu_ws")
            handle = _c._vp()
            _c.check(_c.lib.tcgnn_plan_create(rp_t.data_ptr(), col_t.data_ptr(), bp_t.data_ptr(), e2c_t.data_ptr(), e2r_t.data_ptr(), N, E, bp_len,
                                              _stream_handle(dev), _c.ctypes.byref(handle)), "tcgnn_plan_create")
        entry = dict(plan=handle, own=handle, meta=(rp_t, col_t, bp_t, e2c_t, e2r_t), perm=perm, symmetric=False)
    _transposed[key] = entry
    return entry


def _plan_of(meta, transpose):
    return _transposed_for(*meta)["plan"] if transpose else _plan_for(*meta)


def _values_buffer(E, device):
    """fp32 [max(E, 1)] per (device, stream), like the workspace: A's edge values in A^T's order for forward_AGNN(transpose=True)"""
    key = (device.index, _stream_handle(device))
    buf = _values_t.get(key)
    if buf is None or buf.numel() < max(E, 1):
        buf = torch.empty(max(E, 1), dtype=torch.float32, device=device)
        _values_t[key] = buf
    return buf


def plan_info(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow, transpose=False):
    """Not part of the reference API: statistics of the packed tile stream (dict).  transpose=True: of the plan transpose=True calls
    run on (A's own on a symmetric graph), plus symmetric, shares_plan (no plan of A^T's own) and transpose_bytes (the arrays the
    transposed entry owns: perm, and A^T's five metadata tensors unless the graph is symmetric)."""
    meta = (nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    info = _c.PlanInfo()
    _c.check(_c.lib.tcgnn_plan_get_info(_plan_of(meta, transpose), _c.ctypes.byref(info)), "tcgnn_plan_get_info")
    out = {f: getattr(info, f) for f, _ in info._fields_}
    if transpose:
        tr = _transposed_for(*meta)
        owned = [tr["perm"]] + ([] if tr["symmetric"] else list(tr["meta"]))
        out.update(symmetric=tr["symmetric"], shares_plan=tr["own"] is None, transpose_bytes=sum(t.numel() * t.element_size() for t in owned))
    return out


def prepare(widths, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow, edge_valued=False, transpose=False, attention=False):
    """Not part of the reference API: build, now, what the hot path would otherwise build at its first call of each feature width
    in `widths` (tcgnn_plan_prepare: the cell streams of the LDS-resident kernel where the plan's time model picks it; with
    edge_valued=True also tcgnn_plan_prepare_val: the single-edge stream forward_AGNN's LDS-resident walk reads).  After it no
    forward / backward (/ forward_AGNN) call of those widths synchronises or allocates inside the library, and a call captured into
    a HIP graph takes the walk it would take outside one.  The harness calls it with the model's widths before the dry epochs.
    transpose=True (a model with directed=True layers runs both): also A^T's plan - built now if it is not cached - the same way,
    and with edge_valued=True the buffer forward_AGNN(transpose=True) permutes the edge values into, on the current stream.
    attention=True (a model with softmax-attention layers: forward_ef2, edge_softmax, edge_softmax_backward): the workspace grown to
    forward_ef2's two images at every width and the scratch of edge_softmax_backward's d_beta, on the current stream - a step that
    uses them then allocates nothing outside torch's pool and never synchronises.
    A GAT model (gat_softmax, gat_softmax_backward, edge_colsum and the per-head forward_AGNN / forward_ef2 calls of
    tcgnn_edge_ops.aggregate_heads) passes the PER-HEAD widths with edge_valued=True, transpose=True and attention=True: the
    edge-valued streams of A and A^T at that width, the two-image SDDMM workspace, and - with A^T's plan - the transposed CSR
    edge_colsum sums over."""
    plan = _plan_for(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    plans = [plan]
    dev = nodePointer.device
    if attention:
        with torch.cuda.device(dev):
            for d in sorted({int(w) for w in widths if int(w) >= 1}):
                _workspace(plan, d, dev, need=_c.lib.tcgnn_sddmm2_workspace_bytes(plan, d))
            _softmax_scratch_for(nodePointer.numel() - 1, edgeList.numel(), dev)
    if transpose:
        tr = _transposed_for(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
        if tr["own"] is not None:
            plans.append(tr["own"])
        if edge_valued:
            with torch.cuda.device(dev):
                _values_buffer(edgeList.numel(), dev)
    with torch.cuda.device(dev):
        for d in sorted({int(w) for w in widths if int(w) >= 1}):
            for p in plans:
                _c.check(_c.lib.tcgnn_plan_prepare(p, d, _stream_handle(dev)), "tcgnn_plan_prepare")
                if edge_valued:
                    _c.check(_c.lib.tcgnn_plan_prepare_val(p, d, _stream_handle(dev)), "tcgnn_plan_prepare_val")


def set_plan_modes(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow, spmm_mode=None, range_guard=None):
    """Not part of the reference API: the walk (tcgnn_plan_set_spmm_mode) and the range-guard level (tcgnn_plan_set_range_guard) of
    THIS graph's plan only; -1 hands a setting back to the process-wide value.  Two graphs of one process may differ."""
    plan = _plan_for(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    if spmm_mode is not None:
        _c.check(_c.lib.tcgnn_plan_set_spmm_mode(plan, int(spmm_mode)), "tcgnn_plan_set_spmm_mode")
    if range_guard is not None:
        _c.check(_c.lib.tcgnn_plan_set_range_guard(plan, int(range_guard)), "tcgnn_plan_set_range_guard")


def range_mode(device=None):
    """Not part of the reference API: which way the range guard sent the LAST call staged on this device's current stream -
    (wide_x, wide_val): 1 = the fp32 fallback ran (a matrix with a wide dynamic range, include/tcgnn.h "Operand range"), 0 = the
    MFMA path.  Reads the workspace header back (synchronises the stream): a test / diagnosis aid."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    ws = _workspaces.get((dev.index, _stream_handle(dev)))
    if ws is None:
        return (0, 0)
    off = (-ws.data_ptr()) % 256
    a, b = _c._i32(0), _c._i32(0)
    _c.check(_c.lib.tcgnn_range_mode(ws.data_ptr() + off, _stream_handle(dev), _c.ctypes.byref(a), _c.ctypes.byref(b)), "tcgnn_range_mode")
    return (a.value, b.value)


def set_range_guard(level):
    """Not part of the reference API: the range guard's level - 0 off, 1 the SpMM operators only, 2 (default since r04) also SDDMM and
    the fused AGNN pair when a matrix has a few lost elements (patched behind the MFMA kernels), 3 strict: any wide matrix in fp32
    (include/tcgnn.h: tcgnn_set_range_guard)."""
    _c.check(_c.lib.tcgnn_set_range_guard(int(level)), "tcgnn_set_range_guard")


def kernel_timing(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow, max_calls=None):
    """Not part of the reference API.  kernel_timing(meta..., max_calls=K) arms HIP-event timing of
    the main kernel for the next K calls on this graph; kernel_timing(meta...) (no max_calls) waits
    for them and returns their durations in ms."""
    plan = _plan_for(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    if max_calls is not None:
        _c.check(_c.lib.tcgnn_plan_set_timing(plan, int(max_calls)), "tcgnn_plan_set_timing")
        return None
    buf = (_c.ctypes.c_float * 4096)()
    n = _c._i32(0)
    _c.check(_c.lib.tcgnn_plan_read_timing(plan, buf, 4096, _c.ctypes.byref(n)), "tcgnn_plan_read_timing")
    return [buf[i] for i in range(n.value)]


def last_kernel(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow, transpose=False):
    """Not part of the reference API: name of the main kernel the most recent call on this graph launched (transpose=True: on the
    plan the transposed calls run on)."""
    return _c.lib.tcgnn_plan_last_kernel(_plan_of((nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow), transpose)).decode()


def _workspace(plan, D, device, need=None):
    if need is None:
        need = _c.lib.tcgnn_workspace_bytes(plan, D)
    key = (device.index, _stream_handle(device))
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < need + 256:
        ws = torch.empty(int(need * 1.25) + 256, dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    off = (-ws.data_ptr()) % 256
    return ws.data_ptr() + off, ws.numel() - off


# ---------------------------------------------------------------- sparse-graph translation

def _report(tc_blocks):
    # the reference prints exactly this from C (TCGNN.cpp:225); 1_log2csv.py-style scrapers and the
    # committed logs (logs/RTX3090_GCN.log:1-2) rely on the two lines
    sys.stdout.write("TC_Blocks:\t%d\nExp_Edges:\t%d\n" % (tc_blocks, tc_blocks * 8 * 16))
    sys.stdout.flush()


def preprocess(edgeList, nodePointer, num_nodes, blockSize_h, blockSize_w, blockPartition, edgeToColumn, edgeToRow):
    """Host SGT: fills blockPartition / edgeToColumn / edgeToRow in place (CPU int32 tensors)."""
    names = ("edgeList", "nodePointer", "blockPartition", "edgeToColumn", "edgeToRow")
    for t, n in zip((edgeList, nodePointer, blockPartition, edgeToColumn, edgeToRow), names):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % n)
        if t.is_cuda:
            raise RuntimeError("%s must be a CPU tensor (use preprocess_gpu for device tensors)" % n)
        _check_int(t, n)
        if not t.is_contiguous():
            raise RuntimeError("%s must be contiguous" % n)
    num_nodes = int(num_nodes)
    if nodePointer.numel() < num_nodes + 1:
        raise RuntimeError("nodePointer holds %d entries, need num_nodes + 1 = %d" % (nodePointer.numel(), num_nodes + 1))
    E = int(nodePointer[num_nodes])
    if edgeList.numel() < E or edgeToColumn.numel() < E or edgeToRow.numel() < E:
        raise RuntimeError("edgeList / edgeToColumn / edgeToRow hold fewer than nodePointer[num_nodes] = %d entries" % E)
    n = _c._i64(0)
    st = _c.lib.tcgnn_preprocess(edgeList.data_ptr(), nodePointer.data_ptr(), num_nodes, int(blockSize_h), int(blockSize_w),
                                 blockPartition.data_ptr(), blockPartition.numel(), edgeToColumn.data_ptr(),
                                 edgeToRow.data_ptr(), _c.ctypes.byref(n), 0)
    _c.check(st, "tcgnn_preprocess")
    _report(n.value)


def preprocess_gpu(edgeList, nodePointer, num_nodes, blockSize_h, blockSize_w, blockPartition, edgeToColumn, edgeToRow):
    """Device SGT: same outputs as preprocess, all tensors on the GPU."""
    names = ("edgeList", "nodePointer", "blockPartition", "edgeToColumn", "edgeToRow")
    for t, n in zip((edgeList, nodePointer, blockPartition, edgeToColumn, edgeToRow), names):
        _check_input(t, n)
        _check_int(t, n)
    num_nodes = int(num_nodes)
    if nodePointer.numel() < num_nodes + 1:
        raise RuntimeError("nodePointer holds %d entries, need num_nodes + 1 = %d" % (nodePointer.numel(), num_nodes + 1))
    E = edgeList.numel()
    if edgeToColumn.numel() < E or edgeToRow.numel() < E:
        raise RuntimeError("edgeToColumn / edgeToRow are shorter than edgeList")
    n = _c._i64(0)
    dev = edgeList.device
    with torch.cuda.device(dev):
        # the translation's scratch (sort keys, positions, flags, ranks, rocPRIM's own) comes from torch's caching allocator: the library call
        # allocates nothing and synchronises once (include/tcgnn.h, tcgnn_preprocess_gpu_ws); a second translation of a graph this size
        # finds the block in the cache
        need = _c._sz(0)
        _c.check(_c.lib.tcgnn_preprocess_gpu_workspace_bytes(num_nodes, E, int(blockSize_h), _c.ctypes.byref(need)), "tcgnn_preprocess_gpu_workspace_bytes")
        ws = torch.empty(max(int(need.value), 256), dtype=torch.uint8, device=dev)
        st = _c.lib.tcgnn_preprocess_gpu_ws(edgeList.data_ptr(), nodePointer.data_ptr(), num_nodes, E, int(blockSize_h),
                                            int(blockSize_w), blockPartition.data_ptr(), blockPartition.numel(),
                                            edgeToColumn.data_ptr(), edgeToRow.data_ptr(), ws.data_ptr(), ws.numel(), _c.ctypes.byref(n), _stream_handle(dev))
        del ws   # (the call synchronised the stream: nothing still reads it)
    _c.check(st, "tcgnn_preprocess_gpu_ws")
    _report(n.value)


# ---------------------------------------------------------------- the hot path

def _six(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow):
    _check_input(input, "input")
    _check_input(nodePointer, "nodePointer")
    _check_input(edgeList, "edgeList")
    _check_input(blockPartition, "blockPartition")
    _check_input(edgeToColumn, "edgeToColumn")
    _check_input(edgeToRow, "edgeToRow")
    _check_float(input, "input")
    if input.dim() != 2:
        raise RuntimeError("input must be [num_nodes, embedding_dim]")
    N = nodePointer.numel() - 1
    if input.size(0) != N:
        raise RuntimeError("input has %d rows but nodePointer describes %d nodes" % (input.size(0), N))
    if input.device != nodePointer.device:
        raise RuntimeError("input and nodePointer are on different devices")


def forward(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow, transpose=False):
    """SpMM  Y = A_bin @ input  (GCN / GIN / SAG aggregation, forward and backward).
    transpose=True (not in the reference module): Y = A_bin^T @ input - the metadata still describe A; A^T's plan is built at
    first use and cached beside A's (A's own plan when the graph is symmetric)."""
    _six(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    dev = input.device
    N, D = input.shape
    out = torch.empty_like(input)
    if N == 0 or D == 0:
        return [out]
    with torch.cuda.device(dev):
        plan = _plan_of((nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow), transpose)
        ws, ws_bytes = _workspace(plan, D, dev)
        st = _c.lib.tcgnn_spmm(plan, input.data_ptr(), out.data_ptr(), D, ws, ws_bytes, _stream_handle(dev))
    _c.check(st, "tcgnn_spmm")
    return [out]


def forward_fused(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow, relu=False, gate=None, transpose=False):
    """Not in the reference module: `forward` with the layer's element-wise steps fused in.
    relu=True: max(A @ input, 0) - the ReLU the reference applies after the layer (main_tcgnn.py:100-139) runs in the
    kernel's stores.  gate (same shape as input): A @ (input * (gate > 0)) - with gate = the forward output, the ReLU
    backward mask is applied to dY while it is staged.  Bit-identical to the unfused compositions.  transpose=True: with A^T."""
    _six(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    if gate is not None:
        _check_input(gate, "gate")
        _check_float(gate, "gate")
        if gate.shape != input.shape or gate.device != input.device:
            raise RuntimeError("gate must have the shape and device of input")
    dev = input.device
    N, D = input.shape
    out = torch.empty_like(input)
    if N == 0 or D == 0:
        return [out]
    with torch.cuda.device(dev):
        plan = _plan_of((nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow), transpose)
        ws, ws_bytes = _workspace(plan, D, dev)
        st = _c.lib.tcgnn_spmm_fused(plan, input.data_ptr(), gate.data_ptr() if gate is not None else None, out.data_ptr(), D,
                                     1 if relu else 0, ws, ws_bytes, _stream_handle(dev))
    _c.check(st, "tcgnn_spmm_fused")
    return [out]


def _check_vector(t, name, n, dev):
    _check_input(t, name)
    _check_float(t, name)
    if t.dim() != 1 or t.numel() != n:
        raise RuntimeError("%s must be a 1-D tensor of %d elements, got shape %s" % (name, n, tuple(t.shape)))
    if t.device != dev:
        raise RuntimeError("%s is on %s but input is on %s" % (name, t.device, dev))


def forward_scaled(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow, row_scale=None, col_scale=None,
                   bias=None, relu=False, gate=None, transpose=False):
    """Not in the reference module: the normalised GCN aggregation with its element-wise steps fused in (tcgnn_spmm_scaled),
        Y = act(row_scale[:, None] * (A @ (col_scale[:, None] * X')) + bias),  X' = input * (gate > 0) when gate is given,
    act = ReLU when relu=True.  row_scale / col_scale: fp32 [N], bias: fp32 [D], gate: like input; each may be None.  The
    column scale is applied while the input is staged, the rest where the kernel stores Y: bit-identical to the unfused
    composition forward(col_scale * X') * row_scale + bias, then ReLU, on every walk.  degree_scales gives DGL's scales.
    transpose=True: A^T in place of A, act(row_scale * (A^T @ (col_scale * X')) + bias) - the backward aggregation of the normalised
    layer on a directed graph."""
    # shapes and dtypes of the optional operands first (they do not depend on the device), then the six of forward
    if isinstance(input, torch.Tensor) and input.dim() == 2:
        for t, name, n in ((row_scale, "row_scale", input.size(0)), (col_scale, "col_scale", input.size(0)), (bias, "bias", input.size(1))):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor):
                raise TypeError("%s must be a torch.Tensor" % name)
            _check_float(t, name)
            if t.dim() != 1 or t.numel() != n:
                raise RuntimeError("%s must be a 1-D tensor of %d elements, got shape %s" % (name, n, tuple(t.shape)))
    _six(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    dev = input.device
    N, D = input.shape
    if gate is not None:
        _check_input(gate, "gate")
        _check_float(gate, "gate")
        if gate.shape != input.shape or gate.device != dev:
            raise RuntimeError("gate must have the shape and device of input")
    if row_scale is not None:
        _check_vector(row_scale, "row_scale", N, dev)
    if col_scale is not None:
        _check_vector(col_scale, "col_scale", N, dev)
    if bias is not None:
        _check_vector(bias, "bias", D, dev)
    out = torch.empty_like(input)
    if N == 0 or D == 0:
        return [out]
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    with torch.cuda.device(dev):
        plan = _plan_of((nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow), transpose)
        ws, ws_bytes = _workspace(plan, D, dev)
        st = _c.lib.tcgnn_spmm_scaled(plan, input.data_ptr(), ptr(col_scale), ptr(gate), ptr(row_scale), ptr(bias), out.data_ptr(), D,
                                      1 if relu else 0, ws, ws_bytes, _stream_handle(dev))
    _c.check(st, "tcgnn_spmm_scaled")
    return [out]


NORMS = ("none", "both", "right", "left")


def _drop_scales():
    """Scales of graphs no cached plan uses any more leave with their plans."""
    live = {k[:2] + (k[-1],) for k in _plans}
    for k in [k for k in _scales if k not in live]:
        del _scales[k]


def degree_scales(nodePointer, edgeList, norm):
    """Not in the reference module: the degree normalisation of DGL's GraphConv as (row_scale, col_scale) for forward_scaled.
    in_deg = row length, out_deg = column count, both clamped to >= 1:
        'both'  -> (in_deg^-1/2, out_deg^-1/2)    'right' -> (1 / in_deg, None)
        'left'  -> (None, 1 / out_deg)             'none'  -> (None, None)
    fp32 [N] tensors on the graph's device (CPU tensors work too).  For a graph on the GPU the result is cached beside its plan
    and leaves with it: repeated layer calls neither recompute nor allocate (which a call captured into a HIP graph needs)."""
    if norm not in NORMS:
        raise ValueError("norm must be one of %s, got %r" % (", ".join(NORMS), norm))
    if norm == "none":
        return (None, None)
    for t, n in ((nodePointer, "nodePointer"), (edgeList, "edgeList")):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % n)
        _check_int(t, n)
    if edgeList.device != nodePointer.device:
        raise RuntimeError("edgeList is on %s but nodePointer is on %s" % (edgeList.device, nodePointer.device))
    key = None
    if nodePointer.is_cuda:
        key = tuple((t.data_ptr(), t.numel(), t._version) for t in (nodePointer, edgeList)) + (nodePointer.device.index,)
        hit = _scales.get(key)
        if hit is not None and norm in hit[1]:
            return hit[1][norm]
    N = nodePointer.numel() - 1
    rp = nodePointer.to(torch.int64)
    in_deg = (rp[1:] - rp[:-1]).clamp(min=1).to(torch.float32)
    # (index_add_, not bincount: bincount sizes its output from max(edgeList), a read-back that would synchronise the stream - and
    #  break a HIP-graph capture - whenever the cache misses; ids beyond the node count land in a slot that is cut off)
    n = max(N, 0)
    out_deg = torch.zeros(n + 1, dtype=torch.float32, device=edgeList.device)
    out_deg.index_add_(0, edgeList.to(torch.int64).clamp(max=n), torch.ones(edgeList.numel(), dtype=torch.float32, device=edgeList.device))
    out_deg = out_deg[:n].clamp(min=1)
    if norm == "both":
        res = (in_deg.pow(-0.5), out_deg.pow(-0.5))
    elif norm == "right":
        res = (in_deg.reciprocal(), None)
    else:
        res = (None, out_deg.reciprocal())
    res = tuple(t.contiguous() if t is not None else None for t in res)
    if key is not None:
        if key not in _scales:
            _scales[key] = ((nodePointer, edgeList), {})
        _scales[key][1][norm] = res
        while len(_scales) > _plan_cache_size:   # (a graph never handed to the kernels has no plan to leave with)
            _scales.pop(next(iter(_scales)))
    return res


GEMM_FUSED_MAX_DIM = 128


def forward_gemm(input, weights, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow, relu=False):
    """Not in the reference module: [(A @ input) @ weights] in ONE launch - the GIN order of
    gnn_conv.py:92-97 (`X' = TCGNN.forward(X, ...)[0]; X' = torch.mm(X', weights)`) without the N x D_in round trip: the
    aggregated rows go from the accumulators through LDS into the fp32 matrix pipe against W.  input [N, D_in], weights
    [D_in, D_out], both <= 128 wide.  relu=True fuses max(., 0) where the kernel writes the product in one pass; where it
    accumulates over column passes (the LDS-resident kernel on a 64-column input) the ReLU runs as a separate step here."""
    _six(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    _check_input(weights, "weights")
    _check_float(weights, "weights")
    N, D = input.shape
    if weights.dim() != 2 or weights.shape[0] != D or weights.device != input.device:
        raise RuntimeError("weights must be [input.size(1), D_out] on the input's device")
    Dout = weights.shape[1]
    if D > GEMM_FUSED_MAX_DIM or Dout > GEMM_FUSED_MAX_DIM or D == 0 or Dout == 0:
        raise RuntimeError("forward_gemm covers 1 <= D_in, D_out <= %d (got %d -> %d): compose forward() with torch.mm" % (GEMM_FUSED_MAX_DIM, D, Dout))
    dev = input.device
    out = torch.empty(N, Dout, dtype=torch.float32, device=dev)
    if N == 0:
        return [out]
    with torch.cuda.device(dev):
        plan = _plan_for(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
        ws, ws_bytes = _workspace(plan, D, dev)
        st = _c.lib.tcgnn_spmm_gemm(plan, input.data_ptr(), weights.data_ptr(), out.data_ptr(), D, Dout, 1 if relu else 0, ws, ws_bytes,
                                    _stream_handle(dev))
        if st == 6 and relu:   # TCGNN_ERR_UNSUPPORTED: the product is accumulated over column passes - ReLU as its own step
            st = _c.lib.tcgnn_spmm_gemm(plan, input.data_ptr(), weights.data_ptr(), out.data_ptr(), D, Dout, 0, ws, ws_bytes, _stream_handle(dev))
            _c.check(st, "tcgnn_spmm_gemm")
            return [torch.relu_(out)]
    _c.check(st, "tcgnn_spmm_gemm")
    return [out]


def forward_AGNN(input, nodePointer, edgeList, edgeAttention, blockPartition, edgeToColumn, edgeToRow, transpose=False):
    """SpMM with edge values  Y = A_val @ input,  A_val[row(e), col(e)] = edgeAttention[0, e].
    transpose=True (not in the reference module): Y = A_val^T @ input, edgeAttention still in A's CSR order (row 0): the values are
    permuted into A^T's order (tcgnn_permute_edge_values, into a buffer held per stream) and A^T's plan aggregates them."""
    _six(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    _check_input(edgeAttention, "edgeAttention")
    _check_float(edgeAttention, "edgeAttention")
    dev = input.device
    N, D = input.shape
    E = edgeList.numel()
    # [n_heads, E]; every head's launch in the reference reads row 0 and overwrites the same output
    # (TCGNN_kernel.cu:253-268, :529), so only row 0 is meaningful
    if edgeAttention.numel() < E:
        raise RuntimeError("edgeAttention holds %d values for %d edges" % (edgeAttention.numel(), E))
    out = torch.empty_like(input)
    if N == 0 or D == 0:
        return [out]
    with torch.cuda.device(dev):
        val = edgeAttention.data_ptr()
        if transpose:
            tr = _transposed_for(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
            plan, buf = tr["plan"], _values_buffer(E, dev)
            _c.check(_c.lib.tcgnn_permute_edge_values(val, tr["perm"].data_ptr(), E, buf.data_ptr(), _stream_handle(dev)), "tcgnn_permute_edge_values")
            val = buf.data_ptr()
        else:
            plan = _plan_for(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
        ws, ws_bytes = _workspace(plan, D, dev)
        st = _c.lib.tcgnn_spmm_val(plan, input.data_ptr(), val, out.data_ptr(), D, ws, ws_bytes,
                                   _stream_handle(dev))
    _c.check(st, "tcgnn_spmm_val")
    return [out]


def forward_ef(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow):
    """SDDMM  ef[e] = <input[row(e)], input[col(e)]>  for every CSR edge, fp32 [E]."""
    _six(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    dev = input.device
    N, D = input.shape
    E = edgeList.numel()
    out = torch.empty(E, dtype=torch.float32, device=dev)
    if E == 0:
        return [out]
    if D == 0:
        return [out.zero_()]
    with torch.cuda.device(dev):
        plan = _plan_for(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
        ws, ws_bytes = _workspace(plan, D, dev)
        st = _c.lib.tcgnn_sddmm(plan, input.data_ptr(), out.data_ptr(), D, ws, ws_bytes, _stream_handle(dev))
    _c.check(st, "tcgnn_sddmm")
    return [out]


# ---- additions (not in the reference module): what a softmax-attention layer needs -----------------------

def forward_ef2(X, Z, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow):
    """Not in the reference module: the SDDMM with two operands, ef[e] = <X[row(e)], Z[col(e)]>, fp32 [E] (tcgnn_sddmm2) - the
    gradient of forward_AGNN with respect to its edge values is forward_ef2(dY, input).  Same walks as forward_ef; each operand is
    rounded with its own scale; forward_ef2(X, X) equals forward_ef(X) bit for bit (unless the range guard takes X for wide: the
    single-operand call then patches the dirty rows' edges, this one recomputes the whole call in fp32 - include/tcgnn.h)."""
    _six(X, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    _check_input(Z, "Z")
    _check_float(Z, "Z")
    if Z.shape != X.shape or Z.device != X.device:
        raise RuntimeError("Z must have the shape and device of X")
    dev = X.device
    N, D = X.shape
    E = edgeList.numel()
    out = torch.empty(E, dtype=torch.float32, device=dev)
    if E == 0:
        return [out]
    if D == 0:
        return [out.zero_()]
    with torch.cuda.device(dev):
        plan = _plan_for(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
        ws, ws_bytes = _workspace(plan, D, dev, need=_c.lib.tcgnn_sddmm2_workspace_bytes(plan, D))
        st = _c.lib.tcgnn_sddmm2(plan, X.data_ptr(), Z.data_ptr(), out.data_ptr(), D, ws, ws_bytes, _stream_handle(dev))
    _c.check(st, "tcgnn_sddmm2")
    return [out]


def _softmax_args(score, nodePointer, beta):
    _check_input(score, "score")
    _check_float(score, "score")
    _check_input(nodePointer, "nodePointer")
    _check_int(nodePointer, "nodePointer")
    if score.dim() != 1:
        raise RuntimeError("score must be a 1-D tensor of one value per edge")
    if nodePointer.numel() < 1 or nodePointer.device != score.device:
        raise RuntimeError("nodePointer must hold num_nodes + 1 entries on score's device")
    if beta is not None:
        _check_input(beta, "beta")
        _check_float(beta, "beta")
        if beta.numel() != 1 or beta.device != score.device:
            raise RuntimeError("beta must hold one value on score's device")


def _softmax_scratch_for(N, E, device):
    need = int(_c.lib.tcgnn_edge_softmax_workspace_bytes(max(N, 0), E))
    key = (device.index, _stream_handle(device))
    buf = _softmax_scratch.get(key)
    if buf is None or buf.numel() < need + 256:
        buf = torch.empty(need + 256, dtype=torch.uint8, device=device)
        _softmax_scratch[key] = buf
    off = (-buf.data_ptr()) % 256
    return buf.data_ptr() + off, buf.numel() - off


def edge_softmax(score, nodePointer, beta=None, out=None):
    """Not in the reference module: softmax over every node's incoming edges (DGL's edge_softmax; tcgnn_edge_softmax),
        p[e] = exp(beta s[e] - m_r) / sum_{e' in row r} exp(beta s[e'] - m_r),   row r = nodePointer[r] .. nodePointer[r + 1].
    score: fp32 [E]; beta: a one-element fp32 tensor on the device (None: 1).  out may be score itself (in place).  Entries of
    positions no row covers are left as allocated.  Deterministic: a second call returns the same bits."""
    _softmax_args(score, nodePointer, beta)
    if out is None:
        out = torch.empty_like(score)
    elif out.shape != score.shape or out.dtype != torch.float32 or out.device != score.device or not out.is_contiguous():
        raise RuntimeError("out must be a contiguous fp32 tensor of score's shape on its device")
    dev = score.device
    with torch.cuda.device(dev):
        st = _c.lib.tcgnn_edge_softmax(nodePointer.data_ptr(), nodePointer.numel() - 1, score.numel(), score.data_ptr(),
                                       beta.data_ptr() if beta is not None else None, out.data_ptr(), _stream_handle(dev))
    _c.check(st, "tcgnn_edge_softmax")
    return out


def edge_softmax_backward(p, dp, nodePointer, beta=None, score=None, need_dbeta=False, out=None):
    """Not in the reference module: the backward of edge_softmax (tcgnn_edge_softmax_backward) - (ds, dbeta) with
        g[e] = p[e] (dp[e] - sum_{row} p dp),  ds[e] = beta g[e],  dbeta = sum_e score[e] g[e]   (a one-element tensor, or None
    unless need_dbeta; it needs score).  out may be dp itself.  The partial sums of dbeta live in a buffer held per stream."""
    _softmax_args(p, nodePointer, beta)
    _check_input(dp, "dp")
    _check_float(dp, "dp")
    if dp.shape != p.shape or dp.device != p.device:
        raise RuntimeError("dp must have the shape and device of p")
    if need_dbeta:
        if score is None:
            raise RuntimeError("dbeta needs the scores the softmax was taken of")
        _check_input(score, "score")
        _check_float(score, "score")
        if score.shape != p.shape or score.device != p.device:
            raise RuntimeError("score must have the shape and device of p")
    if out is None:
        out = torch.empty_like(dp)
    elif out.shape != dp.shape or out.dtype != torch.float32 or out.device != dp.device or not out.is_contiguous():
        raise RuntimeError("out must be a contiguous fp32 tensor of dp's shape on its device")
    dev = p.device
    N, E = nodePointer.numel() - 1, p.numel()
    dbeta = torch.empty(1, dtype=torch.float32, device=dev) if need_dbeta else None
    with torch.cuda.device(dev):
        scratch, scratch_bytes = _softmax_scratch_for(N, E, dev) if need_dbeta else (None, 0)
        st = _c.lib.tcgnn_edge_softmax_backward(nodePointer.data_ptr(), N, E, p.data_ptr(), dp.data_ptr(),
                                                score.data_ptr() if need_dbeta else None, beta.data_ptr() if beta is not None else None,
                                                out.data_ptr(), dbeta.data_ptr() if need_dbeta else None, scratch, scratch_bytes,
                                                _stream_handle(dev))
    _c.check(st, "tcgnn_edge_softmax_backward")
    return out, dbeta


# ---- additions (not in the reference module): multi-head GAT attention ----------------------------------

def _gat_args(el, er, nodePointer, edgeList):
    for t, n in ((el, "el"), (er, "er")):
        _check_input(t, n)
        _check_float(t, n)
    for t, n in ((nodePointer, "nodePointer"), (edgeList, "edgeList")):
        _check_input(t, n)
        _check_int(t, n)
    N = nodePointer.numel() - 1
    if N < 0:
        raise RuntimeError("nodePointer must hold num_nodes + 1 entries")
    if el.dim() != 2 or el.size(0) != N or el.size(1) < 1 or er.shape != el.shape:
        raise RuntimeError("el and er must be [num_nodes, heads] (heads >= 1) with num_nodes = %d, got %s and %s" % (N, tuple(el.shape), tuple(er.shape)))
    if any(t.device != el.device for t in (er, nodePointer, edgeList)):
        raise RuntimeError("el, er, nodePointer and edgeList must be on one device")
    return N, edgeList.numel(), el.size(1)


def _head_major(t, name, H, E, like):
    _check_input(t, name)
    _check_float(t, name)
    if tuple(t.shape) != (H, E) or t.device != like.device:
        raise RuntimeError("%s must be a contiguous fp32 [heads, num_edges] = [%d, %d] tensor on the device of el, got %s" % (name, H, E, tuple(t.shape)))


def gat_softmax(el, er, nodePointer, edgeList, negative_slope=0.2, out=None):
    """Not in the reference module: GAT's attention in one kernel (tcgnn_gat_softmax), p fp32 [heads, E] (the reference's edgeAttention
    layout: p[h] is what forward_AGNN takes),
        s[h, e] = leaky_relu(el[col(e), h] + er[row(e), h]),   p[h, .] = softmax of s[h, .] over every node's incoming edges.
    el / er: fp32 [N, heads], the source- and the destination-side term of every node.  The scores never reach memory.  Entries of
    positions no row covers are left as allocated.  Deterministic: a second call returns the same bits."""
    N, E, H = _gat_args(el, er, nodePointer, edgeList)
    if out is None:
        out = torch.empty(H, E, dtype=torch.float32, device=el.device)
    else:
        _head_major(out, "out", H, E, el)
    dev = el.device
    with torch.cuda.device(dev):
        st = _c.lib.tcgnn_gat_softmax(nodePointer.data_ptr(), edgeList.data_ptr(), N, E, H, el.data_ptr(), er.data_ptr(), float(negative_slope),
                                      out.data_ptr(), _stream_handle(dev))
    _c.check(st, "tcgnn_gat_softmax")
    return out


def gat_softmax_backward(p, dp, el, er, nodePointer, edgeList, negative_slope=0.2, out=None):
    """Not in the reference module: the backward of gat_softmax (tcgnn_gat_softmax_backward) - (ds [heads, E], d_er [N, heads]) with
        g = p (dp - sum_row p dp),   ds[h, e] = g (el[col e, h] + er[row e, h] > 0 ? 1 : negative_slope),   d_er[r, h] = sum_{row r} ds[h, .]
    out may be dp itself.  d_el is edge_colsum(ds, nodePointer, edgeList)."""
    N, E, H = _gat_args(el, er, nodePointer, edgeList)
    _head_major(p, "p", H, E, el)
    _head_major(dp, "dp", H, E, el)
    if out is None:
        out = torch.empty_like(dp)
    else:
        _head_major(out, "out", H, E, el)
    dev = el.device
    d_er = torch.empty(N, H, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        st = _c.lib.tcgnn_gat_softmax_backward(nodePointer.data_ptr(), edgeList.data_ptr(), N, E, H, el.data_ptr(), er.data_ptr(), float(negative_slope),
                                               p.data_ptr(), dp.data_ptr(), out.data_ptr(), d_er.data_ptr(), _stream_handle(dev))
    _c.check(st, "tcgnn_gat_softmax_backward")
    return out, d_er


def edge_colsum(val, nodePointer, edgeList):
    """Not in the reference module: out[c, h] = the sum of val[h, e] over the edges e with col(e) = c, fp32 [N, heads] (tcgnn_edge_colsum) -
    a segmented sum over the rows of A^T in a fixed order, no atomics.  val: fp32 [heads, E] in A's CSR order.  The transposed CSR
    is the module's cached one (transpose_graph): built at the first call for a graph, or by prepare(..., transpose=True)."""
    _check_input(val, "val")
    _check_float(val, "val")
    E = edgeList.numel()
    if val.dim() != 2 or val.size(0) < 1 or val.size(1) != E:
        raise RuntimeError("val must be [heads, num_edges] (heads >= 1) with num_edges = %d, got %s" % (E, tuple(val.shape)))
    _, _, rp_t, _, perm, _ = _transpose_csr(nodePointer, edgeList)
    if val.device != nodePointer.device:
        raise RuntimeError("val is on %s but nodePointer is on %s" % (val.device, nodePointer.device))
    dev = val.device
    N, H = nodePointer.numel() - 1, val.size(0)
    out = torch.empty(N, H, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        st = _c.lib.tcgnn_edge_colsum(rp_t.data_ptr(), perm.data_ptr(), N, E, H, val.data_ptr(), out.data_ptr(), _stream_handle(dev))
    _c.check(st, "tcgnn_edge_colsum")
    return out


# ---- additions (not in the reference module): the two products of an AGNN layer in one pass ------------

def agnn_fused_supported(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow):
    """True if agnn_fused_forward / agnn_fused_backward cover this graph and width (canonical CSR, D <= 128, E >= 8)."""
    if not (input.is_cuda and input.dim() == 2 and input.dtype == torch.float32) or input.shape[0] == 0 or input.shape[1] == 0:
        return False
    with torch.cuda.device(input.device):
        plan = _plan_for(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    return bool(_c.lib.tcgnn_agnn_supported(plan, input.shape[1]))


def _weight_scalar(attention_w, dev):
    _check_input(attention_w, "attention_w")
    _check_float(attention_w, "attention_w")
    if attention_w.numel() != 1 or attention_w.device != dev:
        raise RuntimeError("attention_w must hold one value (n_heads = 1) on the input's device")


def agnn_fused_forward(input, nodePointer, edgeList, attention_w, blockPartition, edgeToColumn, edgeToRow):
    """[Y, ef, ef_absmax] with ef = forward_ef(input), Y = forward_AGNN(input, attention_w * ef): what
    gnn_conv.py:125-132 computes with two calls (two gathers of the neighbour rows), here in one pass.
    ef_absmax (1 + N int32 words on the device: max |ef| and the per-row scale exponents) must be handed to agnn_fused_backward."""
    _six(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    dev = input.device
    _weight_scalar(attention_w, dev)
    N, D = input.shape
    out = torch.empty_like(input)
    ef = torch.empty(edgeList.numel(), dtype=torch.float32, device=dev)
    absmax = torch.zeros(1 + input.shape[0], dtype=torch.int32, device=dev)   # word 0: max |ef|; words 1 .. N: per-row exponents of the edge weights (include/tcgnn.h)
    with torch.cuda.device(dev):
        plan = _plan_for(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
        ws, ws_bytes = _workspace(plan, D, dev)
        st = _c.lib.tcgnn_agnn_pair_forward(plan, input.data_ptr(), attention_w.data_ptr(), ef.data_ptr(), absmax.data_ptr(), absmax.numel(),
                                            out.data_ptr(), D, ws, ws_bytes, _stream_handle(dev))
    _c.check(st, "tcgnn_agnn_pair_forward")
    return [out, ef, absmax]


def agnn_fused_backward(d_output, nodePointer, edgeList, attention_w, ef, ef_absmax, blockPartition, edgeToColumn, edgeToRow):
    """[G, d_w] with G = forward_AGNN(d_output, attention_w * ef) and d_w = <forward_ef(d_output), edgeList.float()>
    (gnn_conv.py:143 and :150-153), one pass."""
    _six(d_output, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    dev = d_output.device
    _weight_scalar(attention_w, dev)
    _check_input(ef, "ef")
    _check_float(ef, "ef")
    if ef.numel() != edgeList.numel() or ef_absmax.numel() != 1 + d_output.shape[0] or ef_absmax.dtype != torch.int32 or not ef_absmax.is_cuda:
        raise RuntimeError("ef / ef_absmax are not what agnn_fused_forward returned for this graph")
    N, D = d_output.shape
    out = torch.empty_like(d_output)
    d_w = torch.empty(1, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        plan = _plan_for(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
        ws, ws_bytes = _workspace(plan, D, dev)
        st = _c.lib.tcgnn_agnn_pair_backward(plan, d_output.data_ptr(), attention_w.data_ptr(), ef.data_ptr(), ef_absmax.data_ptr(), ef_absmax.numel(),
                                             out.data_ptr(), d_w.data_ptr(), D, ws, ws_bytes, _stream_handle(dev))
    _c.check(st, "tcgnn_agnn_pair_backward")
    return [out, d_w]


backward = forward        # TCGNN.cpp:270
backward_ef = forward_ef  # TCGNN.cpp:271
