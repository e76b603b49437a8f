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
import os
import sys

import torch

import tcgnn_capi as _c
from tcgnn_graph_cache import GraphCache, TransposedCsr, TransposedPlan, graph_key

__all__ = ["preprocess", "preprocess_gpu", "forward", "forward_ef", "forward_AGNN", "backward", "backward_ef",
           "plan_info", "kernel_timing", "last_kernel", "clear_plan_cache", "set_plan_cache_size", "agnn_fused_supported", "agnn_fused_forward", "agnn_fused_backward",
           "forward_fused", "forward_gemm", "forward_scaled", "degree_scales", "transpose_graph",
           "forward_ef2", "edge_softmax", "edge_softmax_backward", "gat_softmax", "gat_softmax_backward", "edge_colsum", "forward_heads", "forward_ef_heads",
           "forward_max", "backward_max", "forward_stats", "backward_stats", "cache_stats", "drop_scales", "gatv2_softmax", "gatv2_softmax_backward", "gatv2_source_grad",
           "forward_ue", "backward_ue", "edge_sum", "sample_neighbors", "compact_nodes", "compact_graph",
           "sample_rows", "extend_nodes", "compact_rows_graph", "random_walk", "induce_subgraph"]


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _record_event(device, stream):
    with torch.cuda.device(device):
        e = torch.cuda.Event()
        e.record(torch.cuda.ExternalStream(stream, device=device) if stream else torch.cuda.default_stream(device))
    return e


# Everything kept per graph (tcgnn_graph_cache.py): plans, their transposed parts, degree scales, transposed CSRs, retired plans and
# the streams plan-using calls ran on.  Size: plans (packed tile streams, ~3x the CSR's bytes each) kept per process.
_cache = GraphCache(os.environ.get("TCGNN_PLAN_CACHE_SIZE", "8"), _c.lib.tcgnn_plan_destroy, _record_event,
                    lambda e: e.query(), lambda e: e.synchronize())

# Buffers held per stream: (device index, stream id, kind) -> uint8 tensor.  kind -> (growth when it has to be replaced, alignment,
# for which the allocation carries as many spare bytes; 0: the buffer is used from its first byte)
_buffers = {}
_KINDS = {"workspace": (1.25, 256),   # what the plan-based calls stage into (and leave the range guard's header in)
          "values": (1, 0),           # fp32 [max(H E, 1)]: A's edge values in A^T's order, forward_AGNN / forward_heads(transpose=True)
          "softmax": (1, 256),        # the fp64 partials of edge_softmax_backward's d_beta and of gatv2_softmax_backward's d_attn
          "sample": (1, 256),         # sample_neighbors' / sample_rows' / induce_subgraph's row counts and scan scratch (the count call synchronises: nothing reads it afterwards)
          "compact": (1, 256)}        # compact_nodes' / extend_nodes' validation words and scan scratch (likewise: the count call synchronises)


def _buffer(kind, need, device, stream=None):
    """(aligned address, usable bytes) of the buffer of `kind` of the device's current stream, replaced by a larger one when it
    holds fewer than `need` bytes.  need=None: only look - None when the stream has none yet."""
    growth, align = _KINDS[kind]
    key = (device.index, _stream(device) if stream is None else stream, kind)
    buf = _buffers.get(key)
    if need is not None and (buf is None or buf.numel() < need + align):
        buf = _buffers[key] = torch.empty(int(need * growth) + align, dtype=torch.uint8, device=device)
    if buf is None:
        return None
    off = (-buf.data_ptr()) % align if align else 0
    return buf.data_ptr() + off, buf.numel() - off


def set_plan_cache_size(n):
    """Plans kept per process; the least recently used one beyond this is retired.  A mini-batch loop over k graphs wants n >= k.
    Also the environment variable TCGNN_PLAN_CACHE_SIZE."""
    _cache.size = max(1, int(n))
    _cache.trim()


def clear_plan_cache():
    if torch.cuda.is_available():
        for d in _cache.devices():
            torch.cuda.synchronize(d)
    _cache.clear()
    _buffers.clear()


def cache_stats():
    """Not part of the reference API: counts of what the module holds - plans (plan entries), csrs (per-(nodePointer, edgeList)
    entries: scales, transposed CSR), transposed (plan entries whose transpose=True part is built), retired (evicted plan handles
    waiting for their events), buffers / buffer_bytes (the per-stream workspaces, value and softmax buffers)."""
    return dict(_cache.stats(), buffers=len(_buffers), buffer_bytes=sum(b.numel() for b in _buffers.values()))


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


# ---------------------------------------------------------------- plans

def _create_plan(meta, dev, stream):
    for t, n in zip(meta, ("nodePointer", "edgeList", "blockPartition", "edgeToColumn", "edgeToRow")):
        _check_int(t, n)
        if t.device != dev:
            raise RuntimeError("%s is on %s but nodePointer is on %s" % (n, t.device, dev))
    nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow = meta
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
                                      stream, _c.ctypes.byref(handle))
    _c.check(st, "tcgnn_plan_create")
    return handle


def _plan_entry(meta, stream=None):
    """The packed tile stream is a pure function of the five metadata tensors; it is built on the
    device the first time they are seen and reused while they are unchanged (tcgnn_graph_cache.graph_key).
    Every plan-using entry point comes through here, so this is where the stream it runs on is registered:
    an evicted plan waits for an event on each of them."""
    dev = meta[0].device
    if stream is None:
        stream = _stream(dev)
    _cache.register_stream(dev.index, stream)
    key = graph_key(meta)
    e = _cache.plan(key)
    if e is None:
        e = _cache.add_plan(key, _create_plan(meta, dev, stream), meta, dev.index)
    return e


def _plan_of(meta, transpose=False, stream=None):
    e = _plan_entry(meta, stream)
    return _transposed_plan(e).plan if transpose else e.handle


# ---------------------------------------------------------------- the transposed graph (A^T)

def _scratch(nbytes, dev):
    """(tensor kept alive, 256-byte aligned address, usable bytes) of torch-allocator scratch for one library call"""
    ws = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=dev)
    return ws, ws.data_ptr() + (-ws.data_ptr()) % 256, int(nbytes)


def _transpose(nodePointer, edgeList):
    """TransposedCsr of a graph: tcgnn_transpose_ws on torch-allocator scratch (one synchronisation)"""
    N, E = nodePointer.numel() - 1, edgeList.numel()
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
                                       ptr, nbytes, _c.ctypes.byref(sym), _stream(dev))
        del ws   # (the call synchronised the stream: nothing still reads it)
    _c.check(st, "tcgnn_transpose_ws")
    if sym.value:   # A^T = A: its arrays are A's own
        return TransposedCsr(nodePointer, edgeList, perm, True)
    return TransposedCsr(rp_t, col_t, perm, False)


def transpose_graph(nodePointer, edgeList):
    """Not in the reference module: the CSR of A^T on the device, (nodePointer_t, edgeList_t, perm, symmetric).  Row c of A^T lists
    the rows r of every entry (r, c) of A in increasing CSR position (sorted; A's duplicates kept); perm[eT] = the CSR position in A
    of A^T's entry eT; symmetric = A^T has exactly A's arrays (then nodePointer_t / edgeList_t ARE nodePointer / edgeList).  Column
    ids must lie in [0, num_nodes).  Built on the GPU (tcgnn_transpose_ws) and cached in the graph's CSR entry: the transpose=True
    calls and edge_colsum use the same one."""
    for t, n in ((nodePointer, "nodePointer"), (edgeList, "edgeList")):
        _check_input(t, n)
        _check_int(t, n)
    if edgeList.device != nodePointer.device:
        raise RuntimeError("edgeList is on %s but nodePointer is on %s" % (edgeList.device, nodePointer.device))
    if nodePointer.numel() < 1:
        raise RuntimeError("nodePointer must hold num_nodes + 1 entries")
    c = _cache.csr((nodePointer, edgeList))
    if c.transposed is None:
        c.transposed = _transpose(nodePointer, edgeList)
    return c.transposed


# ---------------------------------------------------------------- neighbour sampling

def sample_neighbors(nodePointer, edgeList, fanout, seed, row_mask=None):
    """Not in the reference module: seeded fan-out sampling, (nodePointer_s, edgeList_s, eid).  The sampled graph keeps the node set
    (DGL's sample_neighbors): a square CSR over the same nodes in which a row of degree d keeps all its in-edges when d <= fanout and
    else the fanout positions with the smallest words (h32(seed, e) << 32) | e (include/tcgnn.h states h32), in CSR order; a row whose
    row_mask entry (uint8 or bool [num_nodes]) is 0 keeps none.  eid (int32 [E']) = the CSR position in edgeList of every kept edge:
    edge values or features of the sampled graph are val[eid].  A pure function of its arguments.  fanout=None keeps every edge of the
    unmasked rows; seed is any int, taken modulo 2**64.  One stream synchronisation (to size the outputs)."""
    for t, n in ((nodePointer, "nodePointer"), (edgeList, "edgeList")):
        _check_input(t, n)
        _check_int(t, n)
    dev = nodePointer.device
    if edgeList.device != dev:
        raise RuntimeError("edgeList is on %s but nodePointer is on %s" % (edgeList.device, dev))
    if nodePointer.numel() < 1:
        raise RuntimeError("nodePointer must hold num_nodes + 1 entries")
    N, E = nodePointer.numel() - 1, edgeList.numel()
    if row_mask is not None:
        _check_input(row_mask, "row_mask")
        if row_mask.dtype not in (torch.uint8, torch.bool):
            raise RuntimeError("row_mask must be uint8 or bool, not %s" % row_mask.dtype)
        if row_mask.numel() != N or row_mask.device != dev:
            raise RuntimeError("row_mask must hold one entry per node (%d) on %s" % (N, dev))
    if fanout is not None and int(fanout) < 0:
        raise ValueError("fanout must be None or >= 0, not %r" % (fanout,))
    k = 0x7fffffff if fanout is None else min(int(fanout), 0x7fffffff)
    with torch.cuda.device(dev):
        stream = _stream(dev)
        need = _c._sz(0)
        _c.check(_c.lib.tcgnn_sample_workspace_bytes(N, _c.ctypes.byref(need)), "tcgnn_sample_workspace_bytes")
        ws, ws_bytes = _buffer("sample", need.value, dev, stream)
        rp_s = torch.empty(N + 1, dtype=torch.int32, device=dev)
        kept = _c._i64(0)
        _c.check(_c.lib.tcgnn_sample_neighbors_count(nodePointer.data_ptr(), _ptr(row_mask), N, E, k, rp_s.data_ptr(), ws, ws_bytes,
                                                     _c.ctypes.byref(kept), stream), "tcgnn_sample_neighbors_count")
        col_s = torch.empty(kept.value, dtype=torch.int32, device=dev)
        eid = torch.empty(kept.value, dtype=torch.int32, device=dev)
        if kept.value:
            _c.check(_c.lib.tcgnn_sample_neighbors(nodePointer.data_ptr(), edgeList.data_ptr(), _ptr(row_mask), rp_s.data_ptr(), N, E, k,
                                                   int(seed) & 0xFFFFFFFFFFFFFFFF, col_s.data_ptr(), eid.data_ptr(), stream), "tcgnn_sample_neighbors")
    return rp_s, col_s, eid


# ---------------------------------------------------------------- relabelled mini-batch blocks

def _check_csr_pair(nodePointer, edgeList, dev=None):
    for t, n in ((nodePointer, "nodePointer"), (edgeList, "edgeList")):
        _check_input(t, n)
        _check_int(t, n)
    if edgeList.device != (dev or nodePointer.device):
        raise RuntimeError("edgeList is on %s but nodePointer is on %s" % (edgeList.device, dev or nodePointer.device))
    if dev is not None and nodePointer.device != dev:
        raise RuntimeError("nodePointer is on %s but the first graph's is on %s" % (nodePointer.device, dev))
    if nodePointer.numel() < 1:
        raise RuntimeError("nodePointer must hold num_nodes + 1 entries")


def compact_nodes(graphs, keep=None):
    """Not in the reference module: the node set of one mini-batch, (nodes, new_id).  graphs: a sequence of (nodePointer, edgeList)
    pairs over the same N nodes (the layer graphs of sample_layers); keep: uint8 or bool [N], e.g. the seeds (None: nothing beyond the
    graphs; it is not written).  A node is kept when keep says so, when it has an edge or when it is a column id in any of the graphs.
    nodes (int32 [M]) = the kept ids in increasing order, new_id (int32 [N]) = the rank of a node in nodes, or -1.  A pure function of
    its arguments; column ids must lie in [0, N) and the row pointers be well-formed.  One stream synchronisation (to size nodes),
    however many graphs."""
    graphs = [tuple(g[:2]) for g in graphs]
    if not graphs:
        raise ValueError("compact_nodes needs at least one (nodePointer, edgeList) pair")
    dev = graphs[0][0].device if isinstance(graphs[0][0], torch.Tensor) else None
    for rp, col in graphs:
        _check_csr_pair(rp, col, dev)
    N = graphs[0][0].numel() - 1
    if any(rp.numel() - 1 != N for rp, _ in graphs):
        raise RuntimeError("every graph must have the same number of nodes (%d)" % N)
    if keep is not None:
        _check_input(keep, "keep")
        if keep.dtype not in (torch.uint8, torch.bool):
            raise RuntimeError("keep must be uint8 or bool, not %s" % keep.dtype)
        if keep.numel() != N or keep.device != dev:
            raise RuntimeError("keep must hold one entry per node (%d) on %s" % (N, dev))
    with torch.cuda.device(dev):
        stream = _stream(dev)
        mask = torch.zeros(N, dtype=torch.uint8, device=dev) if keep is None else keep.view(-1).to(torch.uint8, copy=True)
        need = _c._sz(0)
        _c.check(_c.lib.tcgnn_compact_workspace_bytes(N, _c.ctypes.byref(need)), "tcgnn_compact_workspace_bytes")
        ws, ws_bytes = _buffer("compact", need.value, dev, stream)
        _c.check(_c.lib.tcgnn_compact_begin(N, ws, ws_bytes, stream), "tcgnn_compact_begin")
        for rp, col in graphs:
            _c.check(_c.lib.tcgnn_compact_mark(rp.data_ptr(), col.data_ptr(), N, col.numel(), mask.data_ptr(), ws, ws_bytes, stream), "tcgnn_compact_mark")
        new_id = torch.empty(N, dtype=torch.int32, device=dev)
        kept = _c._i32(0)
        _c.check(_c.lib.tcgnn_compact_count(mask.data_ptr(), N, new_id.data_ptr(), ws, ws_bytes, _c.ctypes.byref(kept), stream), "tcgnn_compact_count")
        nodes = torch.empty(kept.value, dtype=torch.int32, device=dev)
        _c.check(_c.lib.tcgnn_compact_nodes(new_id.data_ptr(), N, kept.value, nodes.data_ptr(), stream), "tcgnn_compact_nodes")
    return nodes, new_id


def compact_graph(nodePointer, edgeList, nodes, new_id):
    """Not in the reference module: (nodePointer_b [M + 1], edgeList_b [E]) - the graph over the M nodes of compact_nodes, which must have
    been given this graph: nodePointer_b[i] = nodePointer[nodes[i]], edgeList_b[e] = new_id[edgeList[e]].  The relabelling is monotone: a
    square CSR whose rows keep their edges in their order, so every operator here takes it and per-edge data of the uncompacted graph
    (a sampled graph's eid) serves it unchanged.  No synchronisation.  With a (nodes, new_id) that did not see this graph the call is
    memory-safe and its result unspecified."""
    _check_csr_pair(nodePointer, edgeList)
    dev = nodePointer.device
    N, E = nodePointer.numel() - 1, edgeList.numel()
    for t, n in ((nodes, "nodes"), (new_id, "new_id")):
        _check_input(t, n)
        _check_int(t, n)
        if t.device != dev:
            raise RuntimeError("%s is on %s but nodePointer is on %s" % (n, t.device, dev))
    if new_id.numel() != N:
        raise RuntimeError("new_id must hold one entry per node (%d), not %d" % (N, new_id.numel()))
    M = nodes.numel()
    if M > N:
        raise RuntimeError("nodes holds %d entries, more than the graph's %d nodes" % (M, N))
    with torch.cuda.device(dev):
        rp_b = torch.empty(M + 1, dtype=torch.int32, device=dev)
        col_b = torch.empty(E, dtype=torch.int32, device=dev)
        _c.check(_c.lib.tcgnn_compact_graph(nodePointer.data_ptr(), edgeList.data_ptr(), new_id.data_ptr(), nodes.data_ptr(), N, M, E,
                                            rp_b.data_ptr(), col_b.data_ptr(), _stream(dev)), "tcgnn_compact_graph")
    return rp_b, col_b


# ---------------------------------------------------------------- seed-list sampling: a mini-batch costs its frontier

def _check_id_types(*named):
    """every (tensor, name) is an int32 tensor - the type before the place: a wrong dtype is named wherever the tensor lives"""
    for t, name in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
        _check_int(t, name)


def _check_ids(t, name, dev):
    _check_input(t, name)
    if t.device != dev:
        raise RuntimeError("%s is on %s, expected %s" % (name, t.device, dev))


def sample_rows(nodePointer, edgeList, rows, fanout, seed):
    """Not in the reference module: sample_neighbors from a LIST of row ids, (rowPointer_s, edgeList_s, eid).  rows: int32 [R], any
    order, ids may repeat (every occurrence gets its own slot).  The result has one row per list entry - rowPointer_s int32 [R + 1] -
    and slot i holds exactly what row rows[i] of sample_neighbors(nodePointer, edgeList, fanout, seed) holds: the same edges in CSR
    order and the same eid (positions in the FULL edgeList).  The work follows R, not the number of nodes; nodePointer is read, and
    validated, at the listed rows only.  fanout=None keeps every edge of the listed rows; seed is any int, taken modulo 2**64.  One
    stream synchronisation (to size the outputs)."""
    _check_id_types((nodePointer, "nodePointer"), (edgeList, "edgeList"), (rows, "rows"))
    if fanout is not None and int(fanout) < 0:
        raise ValueError("fanout must be None or >= 0, not %r" % (fanout,))
    _check_csr_pair(nodePointer, edgeList)
    dev = nodePointer.device
    _check_ids(rows, "rows", dev)
    N, E, R = nodePointer.numel() - 1, edgeList.numel(), rows.numel()
    k = 0x7fffffff if fanout is None else min(int(fanout), 0x7fffffff)
    with torch.cuda.device(dev):
        stream = _stream(dev)
        need = _c._sz(0)
        _c.check(_c.lib.tcgnn_sample_rows_workspace_bytes(R, _c.ctypes.byref(need)), "tcgnn_sample_rows_workspace_bytes")
        ws, ws_bytes = _buffer("sample", need.value, dev, stream)
        rp_s = torch.empty(R + 1, dtype=torch.int32, device=dev)
        kept = _c._i64(0)
        _c.check(_c.lib.tcgnn_sample_rows_count(nodePointer.data_ptr(), _ptr(rows), R, N, E, k, rp_s.data_ptr(), ws, ws_bytes, _c.ctypes.byref(kept),
                                                stream), "tcgnn_sample_rows_count")
        col_s = torch.empty(kept.value, dtype=torch.int32, device=dev)
        eid = torch.empty(kept.value, dtype=torch.int32, device=dev)
        if kept.value:
            _c.check(_c.lib.tcgnn_sample_rows(nodePointer.data_ptr(), edgeList.data_ptr(), rows.data_ptr(), rp_s.data_ptr(), R, N, E, k,
                                              int(seed) & 0xFFFFFFFFFFFFFFFF, col_s.data_ptr(), eid.data_ptr(), stream), "tcgnn_sample_rows")
    return rp_s, col_s, eid


def extend_nodes(keep, ids):
    """Not in the reference module: marks ids into the caller's mask IN PLACE and returns (nodes, new_id) of the mask afterwards.
    keep: uint8 [N], contiguous - the node set so far (zeros to start one); ids: an int32 tensor or a sequence of them (seeds, the
    edgeList_s of sample_rows), in any order, repeats allowed, every id in [0, N).  nodes (int32 [M]) = the kept ids in increasing order -
    the next hop's row list - and new_id (int32 [N]) = the rank of a node in nodes, or -1.  One stream synchronisation (to size nodes),
    however many tensors."""
    if not isinstance(keep, torch.Tensor):
        raise TypeError("keep must be a torch.Tensor")
    if keep.dtype != torch.uint8:
        raise RuntimeError("keep must be uint8 (it is written in place), not %s" % keep.dtype)
    ids = [ids] if isinstance(ids, torch.Tensor) else list(ids)
    _check_id_types(*((t, "ids") for t in ids))
    _check_input(keep, "keep")
    dev = keep.device
    for t in ids:
        _check_ids(t, "ids", dev)
    N = keep.numel()
    with torch.cuda.device(dev):
        stream = _stream(dev)
        need = _c._sz(0)
        _c.check(_c.lib.tcgnn_compact_workspace_bytes(N, _c.ctypes.byref(need)), "tcgnn_compact_workspace_bytes")
        ws, ws_bytes = _buffer("compact", need.value, dev, stream)
        _c.check(_c.lib.tcgnn_compact_begin(N, ws, ws_bytes, stream), "tcgnn_compact_begin")
        for t in ids:
            _c.check(_c.lib.tcgnn_compact_mark_ids(_ptr(t), t.numel(), N, _ptr(keep), ws, ws_bytes, stream), "tcgnn_compact_mark_ids")
        new_id = torch.empty(N, dtype=torch.int32, device=dev)
        kept = _c._i32(0)
        _c.check(_c.lib.tcgnn_compact_count(_ptr(keep), N, _ptr(new_id), ws, ws_bytes, _c.ctypes.byref(kept), stream), "tcgnn_compact_count")
        nodes = torch.empty(kept.value, dtype=torch.int32, device=dev)
        _c.check(_c.lib.tcgnn_compact_nodes(_ptr(new_id), N, kept.value, _ptr(nodes), stream), "tcgnn_compact_nodes")
    return nodes, new_id


def compact_rows_graph(rows, rowPointer_s, edgeList_s, nodes, new_id):
    """Not in the reference module: (nodePointer_b [M + 1], edgeList_b [E']) - the square block over the M nodes of extend_nodes of a
    sample_rows graph whose rows are STRICTLY INCREASING (a `nodes` of extend_nodes) and whose rows and columns the mask has seen.  A
    node of the batch that is not listed gets an empty row; edgeList_b[e] = new_id[edgeList_s[e]].  The result equals compact_graph of
    the same sampled graph written over all N rows: eid serves it unchanged.  No synchronisation.  With other rows or another new_id
    the call is memory-safe and its result unspecified."""
    named = ((rows, "rows"), (rowPointer_s, "rowPointer_s"), (edgeList_s, "edgeList_s"), (nodes, "nodes"), (new_id, "new_id"))
    _check_id_types(*named)
    dev = rows.device
    for t, n in named:
        _check_ids(t, n, dev)
    R, E, M, N = rows.numel(), edgeList_s.numel(), nodes.numel(), new_id.numel()
    if rowPointer_s.numel() != R + 1:
        raise RuntimeError("rowPointer_s must hold one entry per listed row and one more (%d), not %d" % (R + 1, rowPointer_s.numel()))
    if M > N:
        raise RuntimeError("nodes holds %d entries, more than new_id's %d nodes" % (M, N))
    with torch.cuda.device(dev):
        rp_b = torch.empty(M + 1, dtype=torch.int32, device=dev)
        col_b = torch.empty(E, dtype=torch.int32, device=dev)
        _c.check(_c.lib.tcgnn_compact_rows_graph(_ptr(rows), R, rowPointer_s.data_ptr(), _ptr(edgeList_s), E, _ptr(new_id), N, M, rp_b.data_ptr(),
                                                 _ptr(col_b), _stream(dev)), "tcgnn_compact_rows_graph")
    return rp_b, col_b


# ---------------------------------------------------------------- subgraph sampling: random walks and induced subgraphs

def random_walk(nodePointer, edgeList, starts, length, seed):
    """Not in the reference module: walks, int32 [W, length + 1] - one seeded random walk of `length` steps from every entry of starts
    (int32 [W], ids may repeat: every occurrence walks on its own).  walks[w][0] = starts[w]; step t of walk w moves from v to
    edgeList[nodePointer[v] + ((h32(seed, w * length + t) * degree(v)) >> 32)] - rows hold in-edges, so to one of v's SOURCES, the
    direction neighbour sampling expands in.  A node without edges keeps the walk where it is (torch_cluster's rule); an id outside
    [0, N) is carried through unfollowed.  A pure function of its arguments; seed is any int, taken modulo 2**64.  No synchronisation."""
    _check_id_types((nodePointer, "nodePointer"), (edgeList, "edgeList"), (starts, "starts"))
    if int(length) < 0:
        raise ValueError("length must be >= 0, not %r" % (length,))
    _check_csr_pair(nodePointer, edgeList)
    dev = nodePointer.device
    _check_ids(starts, "starts", dev)
    N, E, W, length = nodePointer.numel() - 1, edgeList.numel(), starts.numel(), int(length)
    with torch.cuda.device(dev):
        walks = torch.empty((W, length + 1), dtype=torch.int32, device=dev)
        _c.check(_c.lib.tcgnn_random_walk(nodePointer.data_ptr(), _ptr(edgeList), _ptr(starts), W, N, E, length, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                          _ptr(walks), _stream(dev)), "tcgnn_random_walk")
    return walks


def induce_subgraph(nodePointer, edgeList, nodes, new_id):
    """Not in the reference module: (nodePointer_b [M + 1], edgeList_b [E_b], eid [E_b]) - the subgraph the graph induces on the M nodes
    of extend_nodes / compact_nodes (nodes strictly increasing, new_id of the same mask).  Row i keeps, in CSR order, the edges of row
    nodes[i] whose column is in the set; edgeList_b = new_id[edgeList[e]], eid = e, the position in the FULL edgeList (edge values of
    the block are val[eid.long()]).  A square CSR over M nodes in which every row is used: one block serves every layer.  The work
    follows the edges of the listed rows; nodePointer is read, and validated, at the listed rows only.  One stream synchronisation (to
    size the outputs).  With other nodes or another new_id the call is memory-safe and its result unspecified."""
    named = ((nodePointer, "nodePointer"), (edgeList, "edgeList"), (nodes, "nodes"), (new_id, "new_id"))
    _check_id_types(*named)
    _check_csr_pair(nodePointer, edgeList)
    dev = nodePointer.device
    _check_ids(nodes, "nodes", dev)
    _check_ids(new_id, "new_id", dev)
    N, E, M = nodePointer.numel() - 1, edgeList.numel(), nodes.numel()
    if new_id.numel() != N:
        raise RuntimeError("new_id must hold one entry per node (%d), not %d" % (N, new_id.numel()))
    if M > N:
        raise RuntimeError("nodes holds %d entries, more than the graph's %d nodes" % (M, N))
    with torch.cuda.device(dev):
        stream = _stream(dev)
        need = _c._sz(0)
        _c.check(_c.lib.tcgnn_induce_workspace_bytes(M, _c.ctypes.byref(need)), "tcgnn_induce_workspace_bytes")
        ws, ws_bytes = _buffer("sample", need.value, dev, stream)
        rp_b = torch.empty(M + 1, dtype=torch.int32, device=dev)
        kept = _c._i64(0)
        _c.check(_c.lib.tcgnn_induce_count(nodePointer.data_ptr(), _ptr(edgeList), _ptr(nodes), _ptr(new_id), M, N, E, rp_b.data_ptr(), ws, ws_bytes,
                                           _c.ctypes.byref(kept), stream), "tcgnn_induce_count")
        col_b = torch.empty(kept.value, dtype=torch.int32, device=dev)
        eid = torch.empty(kept.value, dtype=torch.int32, device=dev)
        if kept.value:
            _c.check(_c.lib.tcgnn_induce(nodePointer.data_ptr(), _ptr(edgeList), _ptr(nodes), _ptr(new_id), rp_b.data_ptr(), M, N, E, kept.value,
                                         col_b.data_ptr(), eid.data_ptr(), stream), "tcgnn_induce")
    return rp_b, col_b, eid


def _transposed_plan(e):
    """What transpose=True calls run on, built at first use and owned by A's plan entry (it leaves with it): the plan of A^T - A's
    own when the graph is symmetric.  A^T's metadata: the transpose (the CSR entry's), the device SGT on torch-allocator scratch,
    tcgnn_plan_create."""
    if e.transposed is not None:
        return e.transposed
    c = e.csr
    if c.transposed is None:
        c.transposed = _transpose(*e.tensors[:2])
    rp_t, col_t, _, symmetric = c.transposed
    if symmetric:
        e.transposed = TransposedPlan(e.handle, None, e.tensors)
        return e.transposed
    dev = rp_t.device
    N, E, bp_len = rp_t.numel() - 1, col_t.numel(), e.tensors[2].numel()
    with torch.cuda.device(dev):
        bp_t = torch.zeros(bp_len, dtype=torch.int32, device=dev)
        e2c_t = torch.empty(E, dtype=torch.int32, device=dev)
        e2r_t = torch.empty(E, dtype=torch.int32, device=dev)
        need = _c._sz(0)
        _c.check(_c.lib.tcgnn_preprocess_gpu_workspace_bytes(N, E, 16, _c.ctypes.byref(need)), "tcgnn_preprocess_gpu_workspace_bytes")
        ws, ptr, nbytes = _scratch(need.value, dev)
        tc = _c._i64(0)
        st = _c.lib.tcgnn_preprocess_gpu_ws(col_t.data_ptr(), rp_t.data_ptr(), N, E, 16, 8, bp_t.data_ptr(), bp_len, e2c_t.data_ptr(),
                                            e2r_t.data_ptr(), ptr, nbytes, _c.ctypes.byref(tc), _stream(dev))
        del ws
    _c.check(st, "tcgnn_preprocess_gpu_ws")
    meta_t = (rp_t, col_t, bp_t, e2c_t, e2r_t)
    handle = _create_plan(meta_t, dev, _stream(dev))
    e.transposed = TransposedPlan(handle, handle, meta_t)
    return e.transposed


def plan_info(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow, transpose=False):
    """Not part of the reference API: statistics of the packed tile stream (dict).  transpose=True: of the plan transpose=True calls
    run on (A's own on a symmetric graph), plus symmetric, shares_plan (no plan of A^T's own) and transpose_bytes (the arrays the
    transposed entry owns: perm, and A^T's five metadata tensors unless the graph is symmetric)."""
    e = _plan_entry((nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow))
    info = _c.PlanInfo()
    _c.check(_c.lib.tcgnn_plan_get_info(_transposed_plan(e).plan if transpose else e.handle, _c.ctypes.byref(info)), "tcgnn_plan_get_info")
    out = {f: getattr(info, f) for f, _ in info._fields_}
    if transpose:
        csr_t = e.csr.transposed
        owned = [csr_t.perm] + ([] if csr_t.symmetric else list(e.transposed.meta))
        out.update(symmetric=csr_t.symmetric, shares_plan=e.transposed.own is None, transpose_bytes=sum(t.numel() * t.element_size() for t in owned))
    return out


def prepare(widths, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow, edge_valued=False, transpose=False, attention=False, heads=1,
            max_aggregation=False):
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
    A GAT or TransformerConv model (gat_softmax, gat_softmax_backward, edge_colsum, forward_heads and the forward_ef_heads calls of
    tcgnn_edge_ops.aggregate_heads / sddmm_heads) passes the PER-HEAD widths with edge_valued=True, transpose=True, attention=True and heads=H: the
    edge-valued streams of A and A^T at that width (what a layer of ONE head runs on), the two-image SDDMM workspace, with A^T's
    plan the transposed CSR edge_colsum sums over, and - heads > 1 - the workspaces of forward_ef_heads and of forward_heads at H heads of every width in
    `widths` (more than a width the model aggregates with one head needs) on both plans and the [H, E] buffer forward_heads(transpose=True) permutes the values into, on the current stream.
    max_aggregation=True (a model with forward_max / backward_max: SAGEConv's max and pool aggregators - or with forward_stats /
    backward_stats: PNAConv): the transposed CSR backward_max and backward_stats walk, built now (transpose_graph: the graph's one
    transpose) - the calls are planless and need nothing else."""
    if max_aggregation:
        transpose_graph(nodePointer, edgeList)
    e = _plan_entry((nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow))
    plans = [e.handle]
    dev = nodePointer.device
    widths = sorted({int(w) for w in widths if int(w) >= 1})
    with torch.cuda.device(dev):
        stream = _stream(dev)
        if attention:
            for d in widths:
                _buffer("workspace", _c.lib.tcgnn_sddmm2_workspace_bytes(e.handle, d), dev, stream)
                if int(heads) > 1:
                    _buffer("workspace", _c.lib.tcgnn_sddmm_heads_workspace_bytes(e.handle, int(heads), d), dev, stream)
            N, E = max(nodePointer.numel() - 1, 0), edgeList.numel()
            # (... and of gatv2_softmax_backward's d_attn at `heads` heads - and at the one head of an output layer - of every width)
            _buffer("softmax", max([_c.lib.tcgnn_edge_softmax_workspace_bytes(N, E)] +
                                   [_c.lib.tcgnn_gatv2_workspace_bytes(N, E, h, d) for d in widths for h in {1, max(int(heads), 1)}]), dev, stream)
        if transpose:
            own = _transposed_plan(e).own
            if own is not None:
                plans.append(own)
            if edge_valued:
                _buffer("values", 4 * max(int(heads) * edgeList.numel(), 1), dev, stream)
        for d in widths:
            for p in plans:
                if int(heads) > 1:
                    _buffer("workspace", _c.lib.tcgnn_spmm_heads_workspace_bytes(p, int(heads), d), dev, stream)
                _c.check(_c.lib.tcgnn_plan_prepare(p, d, stream), "tcgnn_plan_prepare")
                if edge_valued:
                    _c.check(_c.lib.tcgnn_plan_prepare_val(p, d, stream), "tcgnn_plan_prepare_val")


def set_plan_modes(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow, spmm_mode=None, range_guard=None):
    """Not part of the reference API: the walk (tcgnn_plan_set_spmm_mode) and the range-guard level (tcgnn_plan_set_range_guard) of
    THIS graph's plan only; -1 hands a setting back to the process-wide value.  Two graphs of one process may differ."""
    plan = _plan_of((nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow))
    if spmm_mode is not None:
        _c.check(_c.lib.tcgnn_plan_set_spmm_mode(plan, int(spmm_mode)), "tcgnn_plan_set_spmm_mode")
    if range_guard is not None:
        _c.check(_c.lib.tcgnn_plan_set_range_guard(plan, int(range_guard)), "tcgnn_plan_set_range_guard")


def range_mode(device=None):
    """Not part of the reference API: which way the range guard sent the LAST call staged on this device's current stream -
    (wide_x, wide_val): 1 = the fp32 fallback ran (a matrix with a wide dynamic range, include/tcgnn.h "Operand range"), 0 = the
    MFMA path.  Reads the workspace header back (synchronises the stream): a test / diagnosis aid."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    ws = _buffer("workspace", None, dev)
    if ws is None:
        return (0, 0)
    a, b = _c._i32(0), _c._i32(0)
    _c.check(_c.lib.tcgnn_range_mode(ws[0], _stream(dev), _c.ctypes.byref(a), _c.ctypes.byref(b)), "tcgnn_range_mode")
    return (a.value, b.value)


def set_range_guard(level):
    """Not part of the reference API: the range guard's level - 0 off, 1 the SpMM operators only, 2 (default since r04) also SDDMM and
    the fused AGNN pair when a matrix has a few lost elements (patched behind the MFMA kernels), 3 strict: any wide matrix in fp32
    (include/tcgnn.h: tcgnn_set_range_guard)."""
    _c.check(_c.lib.tcgnn_set_range_guard(int(level)), "tcgnn_set_range_guard")


def set_stage_onepass(on):
    """Not part of the reference API: 0 keeps every call on the two-pass staging (memset + abs-max + convert), 1 (default) stages the
    planar image in one pass over X where that applies (include/tcgnn.h: tcgnn_set_stage_onepass).  Results do not depend on it."""
    _c.check(_c.lib.tcgnn_set_stage_onepass(int(on)), "tcgnn_set_stage_onepass")


def stage_stats(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow):
    """Not part of the reference API: (hits, misses) of the one-pass staging over this graph's calls so far - calls whose remembered
    scale held, and calls that converted again.  Synchronises the current stream: a test / diagnosis aid."""
    plan = _plan_of((nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow))
    h, m = _c._i64(0), _c._i64(0)
    _c.check(_c.lib.tcgnn_plan_stage_stats(plan, _stream(nodePointer.device), _c.ctypes.byref(h), _c.ctypes.byref(m)), "tcgnn_plan_stage_stats")
    return (h.value, m.value)


def kernel_timing(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow, max_calls=None):
    """Not part of the reference API.  kernel_timing(meta..., max_calls=K) arms HIP-event timing of
    the main kernel for the next K calls on this graph; kernel_timing(meta...) (no max_calls) waits
    for them and returns their durations in ms."""
    plan = _plan_of((nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow))
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


def _run(fn, meta, dev, D, operands, transpose=False, need=_c.lib.tcgnn_workspace_bytes, allow=()):
    """The one path of a plan-based call, on dev and its current stream: fn(plan of the graph - with transpose, the one of A^T -,
    *operands, the stream's workspace and its bytes, stream).  need(plan, D): the library's size of that workspace.  A status in
    `allow` is returned, any other but 0 raises."""
    with torch.cuda.device(dev):
        stream = _stream(dev)
        plan = _plan_of(meta, transpose, stream)
        ws, ws_bytes = _buffer("workspace", need(plan, D), dev, stream)
        st = fn(plan, *operands, ws, ws_bytes, stream)
    if st not in allow:
        _c.check(st, fn.__name__)
    return st


def _call(fn, dev, *args):
    """A library call that takes no plan, on dev and its current stream (fn's last argument), status checked"""
    with torch.cuda.device(dev):
        st = fn(*args, _stream(dev))
    _c.check(st, fn.__name__)


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
                                            edgeToColumn.data_ptr(), edgeToRow.data_ptr(), ws.data_ptr(), ws.numel(), _c.ctypes.byref(n), _stream(dev))
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
    return (nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)


def _check_like(t, name, other, other_name):
    _check_input(t, name)
    _check_float(t, name)
    if t.shape != other.shape or t.device != other.device:
        raise RuntimeError("%s must have the shape and device of %s" % (name, other_name))


def _ptr(t):
    return t.data_ptr() if t is not None else None


def forward(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow, transpose=False):
    """SpMM  Y = A_bin @ input  (GCN / GIN / SAG aggregation, forward and backward).
    transpose=True (not in the reference module): Y = A_bin^T @ input - the metadata still describe A; A^T's plan is built at
    first use and cached beside A's (A's own plan when the graph is symmetric)."""
    meta = _six(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    N, D = input.shape
    out = torch.empty_like(input)
    if N and D:
        _run(_c.lib.tcgnn_spmm, meta, input.device, D, (input.data_ptr(), out.data_ptr(), D), transpose)
    return [out]


def forward_fused(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow, relu=False, gate=None, transpose=False):
    """Not in the reference module: `forward` with the layer's element-wise steps fused in.
    relu=True: max(A @ input, 0) - the ReLU the reference applies after the layer (main_tcgnn.py:100-139) runs in the
    kernel's stores.  gate (same shape as input): A @ (input * (gate > 0)) - with gate = the forward output, the ReLU
    backward mask is applied to dY while it is staged.  Bit-identical to the unfused compositions.  transpose=True: with A^T."""
    meta = _six(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    if gate is not None:
        _check_like(gate, "gate", input, "input")
    N, D = input.shape
    out = torch.empty_like(input)
    if N and D:
        _run(_c.lib.tcgnn_spmm_fused, meta, input.device, D, (input.data_ptr(), _ptr(gate), out.data_ptr(), D, 1 if relu else 0), transpose)
    return [out]


def forward_scaled(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow, row_scale=None, col_scale=None,
                   bias=None, relu=False, gate=None, transpose=False):
    """Not in the reference module: the normalised GCN aggregation with its element-wise steps fused in (tcgnn_spmm_scaled),
        Y = act(row_scale[:, None] * (A @ (col_scale[:, None] * X')) + bias),  X' = input * (gate > 0) when gate is given,
    act = ReLU when relu=True.  row_scale / col_scale: fp32 [N], bias: fp32 [D], gate: like input; each may be None.  The
    column scale is applied while the input is staged, the rest where the kernel stores Y: bit-identical to the unfused
    composition forward(col_scale * X') * row_scale + bias, then ReLU, on every walk.  degree_scales gives DGL's scales.
    transpose=True: A^T in place of A, act(row_scale * (A^T @ (col_scale * X')) + bias) - the backward aggregation of the normalised
    layer on a directed graph."""
    vectors = [v for v in ((row_scale, "row_scale", 0), (col_scale, "col_scale", 0), (bias, "bias", 1)) if v[0] is not None]
    # type, dtype and shape of the optional vectors first (they do not depend on the device), then the six of forward, then where
    # the vectors live (an input that is no 2-D tensor fails in the six)
    if isinstance(input, torch.Tensor) and input.dim() == 2:
        for t, name, axis in vectors:
            n = input.size(axis)
            if not isinstance(t, torch.Tensor):
                raise TypeError("%s must be a torch.Tensor" % name)
            _check_float(t, name)
            if t.dim() != 1 or t.numel() != n:
                raise RuntimeError("%s must be a 1-D tensor of %d elements, got shape %s" % (name, n, tuple(t.shape)))
    meta = _six(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    dev = input.device
    if gate is not None:
        _check_like(gate, "gate", input, "input")
    for t, name, _ in vectors:
        _check_input(t, name)
        if t.device != dev:
            raise RuntimeError("%s is on %s but input is on %s" % (name, t.device, dev))
    N, D = input.shape
    out = torch.empty_like(input)
    if N and D:
        _run(_c.lib.tcgnn_spmm_scaled, meta, dev, D, (input.data_ptr(), _ptr(col_scale), _ptr(gate), _ptr(row_scale), _ptr(bias), out.data_ptr(), D,
                                                      1 if relu else 0), transpose)
    return [out]


NORMS = ("none", "both", "right", "left")


def degree_scales(nodePointer, edgeList, norm):
    """Not in the reference module: the degree normalisation of DGL's GraphConv as (row_scale, col_scale) for forward_scaled.
    in_deg = row length, out_deg = column count, both clamped to >= 1:
        'both'  -> (in_deg^-1/2, out_deg^-1/2)    'right' -> (1 / in_deg, None)
        'left'  -> (None, 1 / out_deg)             'none'  -> (None, None)
    fp32 [N] tensors on the graph's device (CPU tensors work too).  For a graph on the GPU the result is cached in the graph's CSR
    entry and leaves with it: repeated layer calls neither recompute nor allocate (which a call captured into a HIP graph needs)."""
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
    scales = _cache.csr((nodePointer, edgeList)).scales if nodePointer.is_cuda else {}
    if norm in scales:
        return scales[norm]
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
    scales[norm] = res = tuple(t.contiguous() if t is not None else None for t in res)
    return res


def drop_scales(nodePointer, edgeList):
    """Not in the reference module: forget the cached degree scales of one graph (the next degree_scales call computes them again)."""
    _cache.csr((nodePointer, edgeList)).scales.clear()


GEMM_FUSED_MAX_DIM = 128


def forward_gemm(input, weights, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow, relu=False):
    """Not in the reference module: [(A @ input) @ weights] in ONE launch - the GIN order of
    gnn_conv.py:92-97 (`X' = TCGNN.forward(X, ...)[0]; X' = torch.mm(X', weights)`) without the N x D_in round trip: the
    aggregated rows go from the accumulators through LDS into the fp32 matrix pipe against W.  input [N, D_in], weights
    [D_in, D_out], both <= 128 wide.  relu=True fuses max(., 0) where the kernel writes the product in one pass; where it
    accumulates over column passes (the LDS-resident kernel on a 64-column input) the ReLU runs as a separate step here."""
    meta = _six(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
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
    if N:
        operands = (input.data_ptr(), weights.data_ptr(), out.data_ptr(), D, Dout)
        # TCGNN_ERR_UNSUPPORTED (6) with relu: the product is accumulated over column passes - ReLU as its own step
        if _run(_c.lib.tcgnn_spmm_gemm, meta, dev, D, operands + (1 if relu else 0,), allow=(6,) if relu else ()) == 6:
            _run(_c.lib.tcgnn_spmm_gemm, meta, dev, D, operands + (0,))
            torch.relu_(out)
    return [out]


def forward_AGNN(input, nodePointer, edgeList, edgeAttention, blockPartition, edgeToColumn, edgeToRow, transpose=False):
    """SpMM with edge values  Y = A_val @ input,  A_val[row(e), col(e)] = edgeAttention[0, e].
    transpose=True (not in the reference module): Y = A_val^T @ input, edgeAttention still in A's CSR order (row 0): the values are
    permuted into A^T's order (tcgnn_permute_edge_values, into a buffer held per stream) and A^T's plan aggregates them."""
    meta = _six(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
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
    if N and D:
        val = edgeAttention.data_ptr()
        if transpose:
            e = _plan_entry(meta)
            _transposed_plan(e)
            val = _buffer("values", 4 * max(E, 1), dev)[0]
            _call(_c.lib.tcgnn_permute_edge_values, dev, edgeAttention.data_ptr(), e.csr.transposed.perm.data_ptr(), E, val)
        _run(_c.lib.tcgnn_spmm_val, meta, dev, D, (input.data_ptr(), val, out.data_ptr(), D), transpose)
    return [out]


def forward_heads(input, nodePointer, edgeList, edgeAttention, blockPartition, edgeToColumn, edgeToRow, heads, transpose=False):
    """Not in the reference module (whose n_heads is the constant 1): the edge-valued SpMM for every head at once (tcgnn_spmm_heads),
        Y[:, hF:(h+1)F] = A_val(edgeAttention[h]) @ input[:, hF:(h+1)F],   F = input.size(1) / heads.
    edgeAttention: fp32 [heads, E], head-major (what gat_softmax returns).  One call whatever the shape: the library takes the fused
    walk - one gather of the neighbour rows feeds every head - where it covers (heads, F) and goes head by head itself elsewhere
    (include/tcgnn.h; last_kernel tells).  heads = 1 is forward_AGNN bit for bit.  transpose=True: with A_val^T - every head's row is
    permuted into A^T's order (tcgnn_permute_edge_values, into the [heads, E] buffer held per stream) and A^T's plan aggregates."""
    meta = _six(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    _check_input(edgeAttention, "edgeAttention")
    _check_float(edgeAttention, "edgeAttention")
    dev = input.device
    N, D = input.shape
    E = edgeList.numel()
    H = int(heads)
    if H < 1 or D % H:
        raise RuntimeError("input has %d columns, which %d heads do not divide" % (D, H))
    if tuple(edgeAttention.shape) != (H, E) or edgeAttention.device != dev:
        raise RuntimeError("edgeAttention must be [heads, num_edges] = [%d, %d] on the input's device, got %s" % (H, E, tuple(edgeAttention.shape)))
    out = torch.empty_like(input)
    if N and D:
        F = D // H
        val = edgeAttention.data_ptr()
        if transpose:
            e = _plan_entry(meta)
            _transposed_plan(e)
            val = _buffer("values", 4 * max(H * E, 1), dev)[0]
            perm = e.csr.transposed.perm.data_ptr()
            for h in range(H):
                _call(_c.lib.tcgnn_permute_edge_values, dev, edgeAttention.data_ptr() + 4 * h * E, perm, E, val + 4 * h * E)
        _run(_c.lib.tcgnn_spmm_heads, meta, dev, D, (input.data_ptr(), val, out.data_ptr(), H, F), transpose,
             need=lambda plan, _: _c.lib.tcgnn_spmm_heads_workspace_bytes(plan, H, F))
    return [out]


def forward_ef(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow):
    """SDDMM  ef[e] = <input[row(e)], input[col(e)]>  for every CSR edge, fp32 [E]."""
    meta = _six(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    D = input.size(1)
    out = torch.empty(edgeList.numel(), dtype=torch.float32, device=input.device)
    if out.numel() and D:
        _run(_c.lib.tcgnn_sddmm, meta, input.device, D, (input.data_ptr(), out.data_ptr(), D))
    elif out.numel():
        out.zero_()
    return [out]


# ---- additions (not in the reference module): what a softmax-attention layer needs -----------------------

def forward_ef2(X, Z, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow):
    """Not in the reference module: the SDDMM with two operands, ef[e] = <X[row(e)], Z[col(e)]>, fp32 [E] (tcgnn_sddmm2) - the
    gradient of forward_AGNN with respect to its edge values is forward_ef2(dY, input).  Same walks as forward_ef; each operand is
    rounded with its own scale; forward_ef2(X, X) equals forward_ef(X) bit for bit (unless the range guard takes X for wide: the
    single-operand call then patches the dirty rows' edges, this one recomputes the whole call in fp32 - include/tcgnn.h)."""
    meta = _six(X, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    _check_like(Z, "Z", X, "X")
    D = X.size(1)
    out = torch.empty(edgeList.numel(), dtype=torch.float32, device=X.device)
    if out.numel() and D:
        _run(_c.lib.tcgnn_sddmm2, meta, X.device, D, (X.data_ptr(), Z.data_ptr(), out.data_ptr(), D), need=_c.lib.tcgnn_sddmm2_workspace_bytes)
    elif out.numel():
        out.zero_()
    return [out]


def forward_ef_heads(X, Z, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow, heads):
    """Not in the reference module: forward_ef2 for every head at once (tcgnn_sddmm_heads),
        ef[h, e] = <X[row(e), hF:(h+1)F], Z[col(e), hF:(h+1)F]>,   F = X.size(1) / heads,
    fp32 [heads, E], head-major - the layout gat_softmax returns and forward_heads takes: the scores of multi-head dot-product
    attention, and forward_heads' gradient with respect to its edge values, forward_ef_heads(dY, input).  One call whatever the
    shape: the library takes the fused walk - one gather of the neighbour rows feeds every head's dot product - where it covers
    (heads, F) and goes head by head itself elsewhere (include/tcgnn.h; last_kernel tells).  Each operand is rounded with one scale
    over all its columns.  heads = 1 is forward_ef2 bit for bit."""
    meta = _six(X, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    _check_like(Z, "Z", X, "X")
    D = X.size(1)
    H = int(heads)
    if H < 1 or D % H:
        raise RuntimeError("X has %d columns, which %d heads do not divide" % (D, H))
    out = torch.empty((H, edgeList.numel()), dtype=torch.float32, device=X.device)
    if out.numel() and D:
        F = D // H
        _run(_c.lib.tcgnn_sddmm_heads, meta, X.device, D, (X.data_ptr(), Z.data_ptr(), out.data_ptr(), H, F),
             need=lambda plan, _: _c.lib.tcgnn_sddmm_heads_workspace_bytes(plan, H, F))
    elif out.numel():
        out.zero_()
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


def _out_like(out, t, name):
    if out is None:
        return torch.empty_like(t)
    if out.shape != t.shape or out.dtype != torch.float32 or out.device != t.device or not out.is_contiguous():
        raise RuntimeError("out must be a contiguous fp32 tensor of %s's shape on its device" % name)
    return out


def edge_softmax(score, nodePointer, beta=None, out=None):
    """Not in the reference module: softmax over every node's incoming edges (DGL's edge_softmax; tcgnn_edge_softmax),
        p[e] = exp(beta s[e] - m_r) / sum_{e' in row r} exp(beta s[e'] - m_r),   row r = nodePointer[r] .. nodePointer[r + 1].
    score: fp32 [E]; beta: a one-element fp32 tensor on the device (None: 1).  out may be score itself (in place).  Entries of
    positions no row covers are left as allocated.  Deterministic: a second call returns the same bits."""
    _softmax_args(score, nodePointer, beta)
    out = _out_like(out, score, "score")
    _call(_c.lib.tcgnn_edge_softmax, score.device, nodePointer.data_ptr(), nodePointer.numel() - 1, score.numel(), score.data_ptr(), _ptr(beta),
          out.data_ptr())
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
    out = _out_like(out, dp, "dp")
    dev = p.device
    N, E = nodePointer.numel() - 1, p.numel()
    dbeta = torch.empty(1, dtype=torch.float32, device=dev) if need_dbeta else None
    scratch = _buffer("softmax", _c.lib.tcgnn_edge_softmax_workspace_bytes(max(N, 0), E), dev) if need_dbeta else (None, 0)
    _call(_c.lib.tcgnn_edge_softmax_backward, dev, nodePointer.data_ptr(), N, E, p.data_ptr(), dp.data_ptr(), _ptr(score if need_dbeta else None),
          _ptr(beta), out.data_ptr(), _ptr(dbeta), *scratch)
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


def _head_major(t, name, H, E, like, of="el"):
    _check_input(t, name)
    _check_float(t, name)
    if tuple(t.shape) != (H, E) or t.device != like.device:
        raise RuntimeError("%s must be a contiguous fp32 [heads, num_edges] = [%d, %d] tensor on the device of %s, got %s" % (name, H, E, of, tuple(t.shape)))


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
    _call(_c.lib.tcgnn_gat_softmax, el.device, nodePointer.data_ptr(), edgeList.data_ptr(), N, E, H, el.data_ptr(), er.data_ptr(), float(negative_slope),
          out.data_ptr())
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
    d_er = torch.empty(N, H, dtype=torch.float32, device=el.device)
    _call(_c.lib.tcgnn_gat_softmax_backward, el.device, nodePointer.data_ptr(), edgeList.data_ptr(), N, E, H, el.data_ptr(), er.data_ptr(),
          float(negative_slope), p.data_ptr(), dp.data_ptr(), out.data_ptr(), d_er.data_ptr())
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
    rp_t, _, perm, _ = transpose_graph(nodePointer, edgeList)
    if val.device != nodePointer.device:
        raise RuntimeError("val is on %s but nodePointer is on %s" % (val.device, nodePointer.device))
    N, H = nodePointer.numel() - 1, val.size(0)
    out = torch.empty(N, H, dtype=torch.float32, device=val.device)
    _call(_c.lib.tcgnn_edge_colsum, val.device, rp_t.data_ptr(), perm.data_ptr(), N, E, H, val.data_ptr(), out.data_ptr())
    return out


# ---- additions (not in the reference module): GATv2 attention ------------------------------------------------

def _gatv2_args(xl, xr, attn, nodePointer, edgeList):
    for t, n in ((xl, "xl"), (xr, "xr"), (attn, "attn")):
        _check_input(t, n)
        _check_float(t, n)
    for t, n in ((nodePointer, "nodePointer"), (edgeList, "edgeList")):
        _check_input(t, n)
        _check_int(t, n)
    N = nodePointer.numel() - 1
    if N < 0:
        raise RuntimeError("nodePointer must hold num_nodes + 1 entries")
    if attn.dim() != 2 or attn.size(0) < 1 or attn.size(1) < 1:
        raise RuntimeError("attn must be [heads, features] (heads >= 1, features >= 1), got %s" % (tuple(attn.shape),))
    H, F = attn.size(0), attn.size(1)
    if xl.dim() != 2 or xl.size(0) != N or xl.size(1) != H * F or xr.shape != xl.shape:
        raise RuntimeError("xl and xr must be [num_nodes, heads * features] = [%d, %d], got %s and %s" % (N, H * F, tuple(xl.shape), tuple(xr.shape)))
    if any(t.device != xl.device for t in (xr, attn, nodePointer, edgeList)):
        raise RuntimeError("xl, xr, attn, nodePointer and edgeList must be on one device")
    return N, edgeList.numel(), H, F


def gatv2_softmax(xl, xr, attn, nodePointer, edgeList, negative_slope=0.2, out=None, score_out=None):
    """Not in the reference module: GATv2's attention in one kernel (tcgnn_gatv2_softmax), p fp32 [heads, E] (the reference's
    edgeAttention layout: p is what forward_heads takes),
        s[h, e] = sum_f attn[h, f] leaky_relu(xl[col(e), hF + f] + xr[row(e), hF + f]),   p[h, .] = softmax of s[h, .] over every node's incoming edges.
    xl / xr: fp32 [N, heads * F], the source- and the destination-side projection (they may be one tensor); attn: fp32 [heads, F].  No
    [E, heads * F] tensor is formed: every neighbour row is gathered once, the score's sum is fp64 and rounded once.  score_out
    (fp32 [heads, E]) receives the scores; p has the same bits with and without it.  Entries of positions no row covers are left as
    allocated.  Deterministic: a second call returns the same bits."""
    N, E, H, F = _gatv2_args(xl, xr, attn, nodePointer, edgeList)
    if out is None:
        out = torch.empty(H, E, dtype=torch.float32, device=xl.device)
    else:
        _head_major(out, "out", H, E, xl, "xl")
    if score_out is not None:
        _head_major(score_out, "score_out", H, E, xl, "xl")
    _call(_c.lib.tcgnn_gatv2_softmax, xl.device, nodePointer.data_ptr(), edgeList.data_ptr(), N, E, H, F, xl.data_ptr(), xr.data_ptr(), attn.data_ptr(),
          float(negative_slope), _ptr(score_out), out.data_ptr())
    return out


def gatv2_softmax_backward(p, dp, xl, xr, attn, nodePointer, edgeList, negative_slope=0.2, out=None):
    """Not in the reference module: the row side of gatv2_softmax's backward (tcgnn_gatv2_softmax_backward) - (g [heads, E], d_xr
    [N, heads * F], d_attn [heads, F]) with z = xl[col e] + xr[row e] and
        g = p (dp - sum_row p dp),   d_xr[i] = sum_{row i} g attn lrelu'(z),   d_attn[h, f] = sum_e g[h, e] leaky_relu(z)[hF + f]
    out (g) may be dp itself.  d_xl is gatv2_source_grad(g, ...).  The partial sums of d_attn live in a buffer held per stream."""
    N, E, H, F = _gatv2_args(xl, xr, attn, nodePointer, edgeList)
    _head_major(p, "p", H, E, xl, "xl")
    _head_major(dp, "dp", H, E, xl, "xl")
    if out is None:
        out = torch.empty_like(dp)
    else:
        _head_major(out, "out", H, E, xl, "xl")
    dev = xl.device
    d_xr = torch.empty(N, H * F, dtype=torch.float32, device=dev)
    d_attn = torch.empty(H, F, dtype=torch.float32, device=dev)
    scratch = _buffer("softmax", _c.lib.tcgnn_gatv2_workspace_bytes(N, E, H, F), dev)
    _call(_c.lib.tcgnn_gatv2_softmax_backward, dev, nodePointer.data_ptr(), edgeList.data_ptr(), N, E, H, F, xl.data_ptr(), xr.data_ptr(), attn.data_ptr(),
          float(negative_slope), p.data_ptr(), dp.data_ptr(), out.data_ptr(), d_xr.data_ptr(), d_attn.data_ptr(), *scratch)
    return out, d_xr, d_attn


def gatv2_source_grad(g, xl, xr, attn, nodePointer, edgeList, negative_slope=0.2):
    """Not in the reference module: the source side of gatv2_softmax's backward (tcgnn_gatv2_source_grad), fp32 [N, heads * F],
        d_xl[j] = sum over the edges e with col(e) = j of g[., e] attn lrelu'(xl[j] + xr[row e])
    - a walk over the rows of A^T in a fixed order (fp64 sums, no atomics); a node nobody reads gets 0.  g: what gatv2_softmax_backward
    returned, in A's CSR order.  The transposed CSR is the module's cached one (transpose_graph): built at the first call for a graph,
    or by prepare(..., transpose=True)."""
    N, E, H, F = _gatv2_args(xl, xr, attn, nodePointer, edgeList)
    _head_major(g, "g", H, E, xl, "xl")
    rp_t, col_t, perm, _ = transpose_graph(nodePointer, edgeList)
    out = torch.empty(N, H * F, dtype=torch.float32, device=xl.device)
    _call(_c.lib.tcgnn_gatv2_source_grad, xl.device, rp_t.data_ptr(), col_t.data_ptr(), perm.data_ptr(), N, E, H, F, xl.data_ptr(), xr.data_ptr(),
          attn.data_ptr(), float(negative_slope), g.data_ptr(), out.data_ptr())
    return out


# ---- additions (not in the reference module): element-wise maximum over a node's incoming edges (GraphSAGE max / pool) -----

def _max_args(t, name, nodePointer, edgeList):
    _check_input(t, name)
    _check_float(t, name)
    for g, n in ((nodePointer, "nodePointer"), (edgeList, "edgeList")):
        _check_input(g, n)
        _check_int(g, n)
    N = nodePointer.numel() - 1
    if N < 0:
        raise RuntimeError("nodePointer must hold num_nodes + 1 entries")
    if t.dim() != 2 or t.size(0) != N:
        raise RuntimeError("%s must be [num_nodes, embedding_dim] with num_nodes = %d, got %s" % (name, N, tuple(t.shape)))
    if any(g.device != t.device for g in (nodePointer, edgeList)):
        raise RuntimeError("%s, nodePointer and edgeList must be on one device" % name)
    return N, edgeList.numel(), t.size(1)


def forward_max(input, nodePointer, edgeList, return_arg=True, out=None):
    """Not in the reference module: (Y, arg) with Y[i, d] = the maximum of input[col(e), d] over the edges e of row i and arg[i, d]
    (int32) the CSR position that supplied it (tcgnn_segment_max).  Exact: input is read as fp32 and Y holds the winner's bits; among
    equal values the smallest position wins, a NaN beats every number (numpy.argmax over the row's slice).  A row without edges:
    Y = 0, arg = -1.  return_arg=False: arg is None (nothing is written for it).  Deterministic, no atomics."""
    N, E, D = _max_args(input, "input", nodePointer, edgeList)
    out = _out_like(out, input, "input")
    arg = torch.empty(N, D, dtype=torch.int32, device=input.device) if return_arg else None
    _call(_c.lib.tcgnn_segment_max, input.device, nodePointer.data_ptr(), edgeList.data_ptr(), N, E, input.data_ptr(), D, out.data_ptr(), _ptr(arg))
    return out, arg


def backward_max(dY, arg, nodePointer, edgeList, out=None):
    """Not in the reference module: the gradient of forward_max with respect to its input (tcgnn_segment_max_backward),
        dX[j, d] = the sum of dY[i, d] over the edges (i <- j) at CSR position e with arg[i, d] == e,
    a walk over the rows of A^T in a fixed order (fp64 sums, no atomics); a node nobody chose gets 0.  The transposed CSR is the
    module's cached one (transpose_graph): built at the first call for a graph, or by prepare(..., max_aggregation=True)."""
    N, E, D = _max_args(dY, "dY", nodePointer, edgeList)
    _check_input(arg, "arg")
    _check_int(arg, "arg")
    if arg.shape != dY.shape or arg.device != dY.device:
        raise RuntimeError("arg must have the shape and device of dY")
    out = _out_like(out, dY, "dY")
    rp_t, col_t, perm, _ = transpose_graph(nodePointer, edgeList)
    _call(_c.lib.tcgnn_segment_max_backward, dY.device, rp_t.data_ptr(), col_t.data_ptr(), perm.data_ptr(), N, E, arg.data_ptr(), dY.data_ptr(), D,
          out.data_ptr())
    return out


# ---- additions (not in the reference module): mean / std / max / min over a node's incoming edges in one walk (PNA) --------

STATS_AGGREGATORS = ("mean", "std", "max", "min")


def _stats_names(aggregators):
    names = (aggregators,) if isinstance(aggregators, str) else tuple(aggregators)
    for a in names:
        if a not in STATS_AGGREGATORS:
            raise ValueError("aggregators must be among %s, got %r" % (", ".join(STATS_AGGREGATORS), a))
    if not names:
        raise ValueError("aggregators must name at least one of %s" % ", ".join(STATS_AGGREGATORS))
    return names


def forward_stats(input, nodePointer, edgeList, aggregators=STATS_AGGREGATORS, eps=1e-5, return_arg=True):
    """Not in the reference module: the aggregators of PNA over every node's incoming edges from ONE gather of the neighbour rows
    (tcgnn_segment_stats) - a dict with the keys named in `aggregators` (among 'mean', 'std', 'max', 'min'; fp32 [N, D]) and, with
    return_arg, 'argmax' / 'argmin' (int32 [N, D]: the CSR position that supplied the value) for the extrema asked for.
        mean = sum x / k;   std = sqrt(max(var, 0) + eps), var the population variance;   max / argmax as forward_max;
        min / argmin its mirror image (numpy.argmin; a NaN beats every number).
    input is read as fp32; the moments are fp64 sums shifted by the row's first neighbour, rounded once.  A row without edges: 0 in
    every value (std too), -1 in the args.  Deterministic, no atomics.  An unknown aggregator name raises ValueError."""
    names = _stats_names(aggregators)
    N, E, D = _max_args(input, "input", nodePointer, edgeList)
    dev = input.device
    out = {a: torch.empty(N, D, dtype=torch.float32, device=dev) for a in STATS_AGGREGATORS if a in names}
    if return_arg:
        out.update({"arg" + a: torch.empty(N, D, dtype=torch.int32, device=dev) for a in ("max", "min") if a in names})
    if N and D:   # (a tensor without elements has no address to give)
        _call(_c.lib.tcgnn_segment_stats, dev, nodePointer.data_ptr(), edgeList.data_ptr(), N, E, input.data_ptr(), D, float(eps),
              *[_ptr(out.get(k)) for k in ("mean", "std", "max", "argmax", "min", "argmin")])
    return out


def backward_stats(grads, saved, nodePointer, edgeList, out=None):
    """Not in the reference module: the gradient of forward_stats with respect to its input (tcgnn_segment_stats_backward), one
    walk over the rows of A^T in a fixed order (fp64 terms and sums, no atomics).  grads: aggregator name -> dY fp32 [N, D] (entries
    may be missing or None); saved: 'Z' (the forward's input) and, as far as those aggregators have a gradient, 'mean', 'std',
    'argmax', 'argmin' as forward_stats returned them.  With k the row's edge count, on rows with k > 0
        b = d_std / (k std),   a = d_mean / k - b mean      (both 0 on a row without edges)
    are formed here with fp32 element-wise operations on [N, D] tensors, and
        dZ[j, d] = sum over the edges (i <- j) at CSR position e of  a[i, d] + b[i, d] Z[j, d] + [argmax[i, d] == e] d_max[i, d]
                                                                     + [argmin[i, d] == e] d_min[i, d].
    Conditioning: mean is stored in fp32, so the std gradient a + b Z = b (Z - mean) loses about |mean| / std * 2^-24 of relative
    accuracy - as in any fp32 implementation.  The transposed CSR is the module's cached one (transpose_graph): built at the first
    call for a graph, or by prepare(..., max_aggregation=True)."""
    for k in grads:
        if k not in STATS_AGGREGATORS:
            raise ValueError("grads must be keyed by %s, got %r" % (", ".join(STATS_AGGREGATORS), k))
    g = {k: v for k, v in grads.items() if v is not None}
    Z = saved["Z"]
    N, E, D = _max_args(Z, "Z", nodePointer, edgeList)
    for k, v in g.items():
        _check_input(v, "grads[%r]" % k)
        _check_float(v, "grads[%r]" % k)
        if v.shape != Z.shape or v.device != Z.device:
            raise RuntimeError("grads[%r] must have the shape and device of Z" % k)
    for k in ("max", "min"):
        if k in g:
            arg = saved["arg" + k]
            _check_input(arg, "arg" + k)
            _check_int(arg, "arg" + k)
            if arg.shape != Z.shape or arg.device != Z.device:
                raise RuntimeError("arg%s must have the shape and device of Z" % k)
    out = _out_like(out, Z, "Z")
    if not (N and D):
        return out
    a = b = None
    if "mean" in g or "std" in g:
        has = (nodePointer[1:] > nodePointer[:-1]).unsqueeze(1)
        inv_k = has.to(torch.float32) / (nodePointer[1:] - nodePointer[:-1]).clamp(min=1).to(torch.float32).unsqueeze(1)   # 1 / k, 0 on a row without edges
        if "std" in g:
            b = (g["std"] * inv_k) / torch.where(has, saved["std"], 1.0)   # (std is 0 on a row without edges: keep 0 / 0 out)
            a = (g["mean"] * inv_k - b * saved["mean"]) if "mean" in g else -(b * saved["mean"])
        else:
            a = g["mean"] * inv_k
    rp_t, col_t, perm, _ = transpose_graph(nodePointer, edgeList)
    _call(_c.lib.tcgnn_segment_stats_backward, Z.device, rp_t.data_ptr(), col_t.data_ptr(), perm.data_ptr(), N, E, Z.data_ptr() if b is not None else None,
          _ptr(a), _ptr(b), saved["argmax"].data_ptr() if "max" in g else None, _ptr(g.get("max")), saved["argmin"].data_ptr() if "min" in g else None,
          _ptr(g.get("min")), D, out.data_ptr())
    return out


# ---- additions (not in the reference module): a feature vector per edge (u_add_e / sum, copy_e / sum; GINEConv) -------------

UE_ACTS = {None: 0, "identity": 0, "relu": 1}   # (TCGNN_ACT_IDENTITY, TCGNN_ACT_RELU)


def _ue_act(act):
    if act not in UE_ACTS:
        raise ValueError("act must be 'relu', 'identity' or None, got %r" % (act,))
    return UE_ACTS[act]


def _edge_rows(t, name, E, D, like):
    _check_input(t, name)
    _check_float(t, name)
    if t.dim() != 2 or t.size(0) != E or (D is not None and t.size(1) != D) or t.device != like.device:
        raise RuntimeError("%s must be a contiguous fp32 [num_edges, embedding_dim] = [%d, %s] tensor on the device of nodePointer, got %s"
                           % (name, E, "D" if D is None else D, tuple(t.shape)))


def _out_apart(out, given, *inputs):
    """_out_like's result may not share memory with an operand the kernel still reads while it writes"""
    if given is None or not out.numel():
        return
    lo, hi = out.data_ptr(), out.data_ptr() + out.numel() * out.element_size()
    for t in inputs:
        if t is not None and t.numel() and t.data_ptr() < hi and lo < t.data_ptr() + t.numel() * t.element_size():
            raise RuntimeError("out must not share memory with an input")


def forward_ue(X, Ef, nodePointer, edgeList, act="relu", out=None):
    """Not in the reference module: message passing with a feature vector per edge (tcgnn_edge_message; DGL's u_add_e / sum),
        Y[i, d] = the sum over the edges e of row i of act(X[col(e), d] + Ef[e, d]),   act: 'relu', or 'identity' / None.
    X: fp32 [N, D]; Ef: fp32 [E, D] in CSR position order.  The message is formed in fp32 and summed in fp64 in a fixed order, rounded
    once; no [E, D] tensor is made.  A row without edges gives 0.  ReLU as torch.relu (a NaN stays NaN).  Deterministic, no atomics."""
    N, E, D = _max_args(X, "X", nodePointer, edgeList)
    code = _ue_act(act)
    _edge_rows(Ef, "Ef", E, D, nodePointer)
    res = _out_like(out, X, "X")
    _out_apart(res, out, X, Ef)
    _call(_c.lib.tcgnn_edge_message, X.device, nodePointer.data_ptr(), edgeList.data_ptr(), N, E, X.data_ptr(), Ef.data_ptr(), D, code, res.data_ptr())
    return res


def backward_ue(dY, X, Ef, nodePointer, edgeList, act="relu", out=None):
    """Not in the reference module: the per-edge gradient of forward_ue (tcgnn_edge_message_backward), fp32 [E, D],
        dM[e, d] = dY[row(e), d] where act is the identity or X[col(e), d] + Ef[e, d] is positive or a NaN (torch's ReLU backward), else 0
    - exact: the bits of dY or zero.  dM is the gradient with respect to Ef; the gradient with respect to X is
    edge_sum(dM, nodePointer_t, perm) over the transposed graph.  With act 'identity' / None X and Ef are not read and may be None."""
    N, E, D = _max_args(dY, "dY", nodePointer, edgeList)
    code = _ue_act(act)
    if code:
        _check_input(X, "X")
        _check_float(X, "X")
        if X.shape != dY.shape or X.device != dY.device:
            raise RuntimeError("X must have the shape and device of dY")
        _edge_rows(Ef, "Ef", E, D, nodePointer)
    if out is None:
        res = torch.empty(E, D, dtype=torch.float32, device=dY.device)
    else:
        _edge_rows(out, "out", E, D, nodePointer)
        res = out
    _out_apart(res, out, dY, X if code else None, Ef if code else None)
    _call(_c.lib.tcgnn_edge_message_backward, dY.device, nodePointer.data_ptr(), edgeList.data_ptr(), N, E, _ptr(X) if code else None,
          _ptr(Ef) if code else None, dY.data_ptr(), D, code, res.data_ptr())
    return res


def edge_sum(M, nodePointer, perm=None, out=None):
    """Not in the reference module: per-edge rows summed into nodes (tcgnn_edge_sum), fp32 [N, D],
        Y[r, d] = the sum over the positions t of row r of M[perm[t], d]   (perm=None: M[t, d] - DGL's copy_e / sum),
    fp64 sums in a fixed order, rounded once; a row without edges gives 0.  M: fp32 [E, D] in A's CSR position order.  With
    (nodePointer_t, _, perm, _) = transpose_graph(nodePointer, edgeList) it sums by SOURCE node: the gradient of forward_ue with respect
    to X from backward_ue's dM.  Deterministic, no atomics."""
    _check_input(nodePointer, "nodePointer")
    _check_int(nodePointer, "nodePointer")
    N = nodePointer.numel() - 1
    if N < 0:
        raise RuntimeError("nodePointer must hold num_nodes + 1 entries")
    _check_input(M, "M")
    _check_float(M, "M")
    if M.dim() != 2 or M.device != nodePointer.device:
        raise RuntimeError("M must be [num_edges, embedding_dim] on nodePointer's device, got %s" % (tuple(M.shape),))
    E, D = M.shape
    if perm is not None:
        _check_input(perm, "perm")
        _check_int(perm, "perm")
        if perm.dim() != 1 or perm.numel() != E or perm.device != M.device:
            raise RuntimeError("perm must hold num_edges = %d entries on M's device, got %s" % (E, tuple(perm.shape)))
    if out is None:
        res = torch.empty(N, D, dtype=torch.float32, device=M.device)
    else:
        if tuple(out.shape) != (N, D) or out.dtype != torch.float32 or out.device != M.device or not out.is_contiguous():
            raise RuntimeError("out must be a contiguous fp32 [num_nodes, embedding_dim] = [%d, %d] tensor on M's device" % (N, D))
        res = out
    _out_apart(res, out, M)
    _call(_c.lib.tcgnn_edge_sum, M.device, nodePointer.data_ptr(), _ptr(perm), N, E, M.data_ptr(), D, res.data_ptr())
    return res


# ---- additions (not in the reference module): the two products of an AGNN layer in one pass ------------

def agnn_fused_supported(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow):
    """True if agnn_fused_forward / agnn_fused_backward cover this graph and width (canonical CSR, D <= 128, E >= 8)."""
    if not (input.is_cuda and input.dim() == 2 and input.dtype == torch.float32) or input.shape[0] == 0 or input.shape[1] == 0:
        return False
    return bool(_c.lib.tcgnn_agnn_supported(_plan_of((nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)), input.shape[1]))


def _weight_scalar(attention_w, dev):
    _check_input(attention_w, "attention_w")
    _check_float(attention_w, "attention_w")
    if attention_w.numel() != 1 or attention_w.device != dev:
        raise RuntimeError("attention_w must hold one value (n_heads = 1) on the input's device")


def agnn_fused_forward(input, nodePointer, edgeList, attention_w, blockPartition, edgeToColumn, edgeToRow):
    """[Y, ef, ef_absmax] with ef = forward_ef(input), Y = forward_AGNN(input, attention_w * ef): what
    gnn_conv.py:125-132 computes with two calls (two gathers of the neighbour rows), here in one pass.
    ef_absmax (1 + N int32 words on the device: max |ef| and the per-row scale exponents) must be handed to agnn_fused_backward."""
    meta = _six(input, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    dev = input.device
    _weight_scalar(attention_w, dev)
    N, D = input.shape
    out = torch.empty_like(input)
    ef = torch.empty(edgeList.numel(), dtype=torch.float32, device=dev)
    absmax = torch.zeros(1 + N, dtype=torch.int32, device=dev)   # word 0: max |ef|; words 1 .. N: per-row exponents of the edge weights (include/tcgnn.h)
    _run(_c.lib.tcgnn_agnn_pair_forward, meta, dev, D, (input.data_ptr(), attention_w.data_ptr(), ef.data_ptr(), absmax.data_ptr(), absmax.numel(),
                                                        out.data_ptr(), D))
    return [out, ef, absmax]


def agnn_fused_backward(d_output, nodePointer, edgeList, attention_w, ef, ef_absmax, blockPartition, edgeToColumn, edgeToRow):
    """[G, d_w] with G = forward_AGNN(d_output, attention_w * ef) and d_w = <forward_ef(d_output), edgeList.float()>
    (gnn_conv.py:143 and :150-153), one pass."""
    meta = _six(d_output, nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow)
    dev = d_output.device
    _weight_scalar(attention_w, dev)
    _check_input(ef, "ef")
    _check_float(ef, "ef")
    N, D = d_output.shape
    if ef.numel() != edgeList.numel() or ef_absmax.numel() != 1 + N or ef_absmax.dtype != torch.int32 or not ef_absmax.is_cuda:
        raise RuntimeError("ef / ef_absmax are not what agnn_fused_forward returned for this graph")
    out = torch.empty_like(d_output)
    d_w = torch.empty(1, dtype=torch.float32, device=dev)
    _run(_c.lib.tcgnn_agnn_pair_backward, meta, dev, D, (d_output.data_ptr(), attention_w.data_ptr(), ef.data_ptr(), ef_absmax.data_ptr(), ef_absmax.numel(),
                                                         out.data_ptr(), d_w.data_ptr(), D))
    return [out, d_w]


backward = forward        # TCGNN.cpp:270
backward_ef = forward_ef  # TCGNN.cpp:271
