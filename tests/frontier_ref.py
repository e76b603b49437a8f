"""numpy restatement of seed-list sampling (include/tcgnn.h, "Seed-list sampling") on top of sample_ref.sample_neighbors and
compact_ref: sample_rows, extend_nodes and compact_rows_graph, the row-list pipeline built from them and the dense pipeline
(sample_layers + compact_layers) it must equal.  Nothing here shares code with the library."""
import numpy as np

import compact_ref as CR
import sample_ref as SR

SCAN_ROWS = 1024   # list slots one workgroup of the rows scan covers (slot R, the total, included)


def workspace_bytes(num_rows):
    """what tcgnn_sample_rows_workspace_bytes states: 32 bytes of result words and one 4-byte partial sum per SCAN_ROWS of the list's
    num_rows + 1 slots, each part rounded up to 256 bytes"""
    blocks = (num_rows + 1 + SCAN_ROWS - 1) // SCAN_ROWS
    return 256 + (blocks * 4 + 255) // 256 * 256


def sample_rows(rp, col, rows, k, seed, dense=None):
    """(rowPointer_s [R + 1], edgeList_s, eid) int32: slot i = row rows[i] of sample_neighbors(rp, col, k, seed).
    dense: that sample, when the caller already has it."""
    rp_d, col_d, eid_d = SR.sample_neighbors(rp, col, k, seed) if dense is None else dense
    rows = np.asarray(rows, dtype=np.int64)
    rp_d = np.asarray(rp_d, dtype=np.int64)
    counts = rp_d[rows + 1] - rp_d[rows]
    start = np.concatenate([[0], np.cumsum(counts)])
    # entry t of slot i is entry rp_d[rows[i]] + (t - start[i]) of the dense sample
    take = np.repeat(rp_d[rows] - start[:-1], counts) + np.arange(start[-1], dtype=np.int64)
    return start.astype(np.int32), col_d[take].astype(np.int32), eid_d[take].astype(np.int32)


def extend_nodes(keep, ids):
    """marks ids (an array or a list of arrays) into the uint8 mask IN PLACE -> (nodes, new_id)"""
    for a in (ids if isinstance(ids, (list, tuple)) else [ids]):
        keep[np.asarray(a, dtype=np.int64)] = 1
    nodes = np.nonzero(keep)[0].astype(np.int32)
    new_id = np.full(len(keep), -1, dtype=np.int32)
    new_id[nodes] = np.arange(len(nodes), dtype=np.int32)
    return nodes, new_id


def compact_rows_graph(rows, rp_s, col_s, nodes, new_id):
    """(nodePointer_b [M + 1], edgeList_b [E']): nodePointer_b[j] = rowPointer_s[#{i : new_id[rows[i]] < j}]; rows strictly increasing"""
    pos = new_id[np.asarray(rows, dtype=np.int64)].astype(np.int64)
    below = np.array([(pos < j).sum() for j in range(len(nodes) + 1)], dtype=np.int64)
    return np.asarray(rp_s)[below].astype(np.int32), new_id[np.asarray(col_s, dtype=np.int64)].astype(np.int32)


def expand_rows(rows, rp_s, n):
    """the row pointers over all n rows of a row-list graph whose rows are strictly increasing"""
    counts = np.zeros(n, dtype=np.int64)
    counts[np.asarray(rows, dtype=np.int64)] = np.diff(np.asarray(rp_s, dtype=np.int64))
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def batch_rows(rp, col, seeds, fanouts, seed):
    """the row-list pipeline -> (nodes, new_id, seed_pos, [(nodePointer_b, edgeList_b)] input layer first, [eid])"""
    n = len(rp) - 1
    keep = np.zeros(n, dtype=np.uint8)
    nodes, new_id = extend_nodes(keep, seeds)
    hops = []
    for hop, k in enumerate(reversed(list(fanouts))):
        rows = nodes
        rp_s, col_s, eid = sample_rows(rp, col, rows, k, seed + hop)
        nodes, new_id = extend_nodes(keep, col_s)
        hops.insert(0, (rows, rp_s, col_s, eid))
    blocks = [compact_rows_graph(rows, rp_s, col_s, nodes, new_id) for rows, rp_s, col_s, _ in hops]
    return nodes, new_id, new_id[np.asarray(seeds, dtype=np.int64)].astype(np.int64), blocks, [h[3] for h in hops]


def batch_dense(rp, col, seeds, fanouts, seed):
    """the dense pipeline (sample_layers + compact_layers restated) -> the same tuple"""
    n = len(rp) - 1
    frontier = np.zeros(n, dtype=np.uint8)
    frontier[np.asarray(seeds, dtype=np.int64)] = 1
    first = frontier.copy()
    graphs = []
    for hop, k in enumerate(reversed(list(fanouts))):
        g = SR.sample_neighbors(rp, col, k, seed + hop, frontier)
        graphs.insert(0, g)
        frontier = frontier.copy()
        frontier[g[1]] = 1
    nodes, new_id, blocks = CR.compact([(g[0], g[1]) for g in graphs], first)
    return nodes, new_id, new_id[np.asarray(seeds, dtype=np.int64)].astype(np.int64), blocks, [g[2] for g in graphs]
