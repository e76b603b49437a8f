"""numpy restatement of subgraph sampling (include/tcgnn.h, "Subgraph sampling"): random_walk, induce_subgraph, the batches built from
them (subgraph_batch, saint_batch) and the workspace formula, on top of sample_ref.h32 and frontier_ref.extend_nodes.  Nothing here
shares code with the library."""
import numpy as np

import frontier_ref as FR
import sample_ref as SR

SCAN_ROWS = 1024   # list slots one workgroup of the induce scan covers (slot M, the total, included)


def workspace_bytes(num_kept):
    """what tcgnn_induce_workspace_bytes states: 256 bytes for the result words and, rounded up to 256 bytes, one 4-byte partial sum per
    SCAN_ROWS of the list's num_kept + 1 slots"""
    blocks = (num_kept + 1 + SCAN_ROWS - 1) // SCAN_ROWS
    return 256 + (blocks * 4 + 255) // 256 * 256


def pick(seed, i, d):
    """(h32(seed, i) * d) >> 32 for arrays of counters i and degrees d > 0: uint64 arithmetic, the product below 2^63"""
    return (SR.h32(seed, i) * np.asarray(d, dtype=np.uint64)) >> np.uint64(32)


def random_walk(rp, col, starts, length, seed):
    """walks int32 [W, length + 1]; only col[:len(col)] is looked at, pointers are clamped to [0, len(col)]"""
    rp = np.asarray(rp, dtype=np.int64)
    col = np.asarray(col)
    n, E = len(rp) - 1, len(col)
    starts = np.asarray(starts, dtype=np.int32)
    W = len(starts)
    walks = np.zeros((W, length + 1), dtype=np.int32)
    walks[:, 0] = starts
    for t in range(length):
        v = walks[:, t].astype(np.int64)
        inside = (v >= 0) & (v < n)
        at = np.where(inside, v, 0)
        lo = np.clip(rp[at], 0, E) if n else np.zeros(W, np.int64)
        hi = np.clip(rp[at + 1], 0, E) if n else np.zeros(W, np.int64)
        d = hi - lo
        move = inside & (d > 0)
        nxt = v.copy()
        if move.any():
            i = np.arange(W, dtype=np.uint64) * np.uint64(length) + np.uint64(t)
            j = pick(seed, i[move], d[move]).astype(np.int64)
            nxt[move] = col[lo[move] + j]
        walks[:, t + 1] = nxt
    return walks


def induce_subgraph(rp, col, nodes, new_id):
    """(nodePointer_b [M + 1], edgeList_b, eid) int32 of the subgraph induced on nodes (strictly increasing; new_id of the same set)"""
    rp = np.asarray(rp, dtype=np.int64)
    col = np.asarray(col)
    nodes = np.asarray(nodes, dtype=np.int64)
    m = len(nodes)
    lo, d = rp[nodes], rp[nodes + 1] - rp[nodes]
    start = np.concatenate([[0], np.cumsum(d)])
    pos = np.repeat(lo - start[:-1], d) + np.arange(start[-1], dtype=np.int64)   # every position of every listed row, row by row
    row = np.repeat(np.arange(m, dtype=np.int64), d)
    ids = np.asarray(new_id)[col[pos]] if len(pos) else np.zeros(0, np.int32)
    kept = ids >= 0
    counts = np.bincount(row[kept], minlength=m) if m else np.zeros(0, np.int64)
    rp_b = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return rp_b, ids[kept].astype(np.int32), pos[kept].astype(np.int32)


def subgraph_batch(rp, col, ids):
    """-> (nodes, new_id, seed_pos int64, (nodePointer_b, edgeList_b), eid): ids in any order, repeats allowed"""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    keep = np.zeros(len(rp) - 1, dtype=np.uint8)
    nodes, new_id = FR.extend_nodes(keep, ids)
    rp_b, col_b, eid = induce_subgraph(rp, col, nodes, new_id)
    return nodes, new_id, new_id[ids].astype(np.int64), (rp_b, col_b), eid


def saint_batch(rp, col, roots, walk_length, seed):
    return subgraph_batch(rp, col, random_walk(rp, col, roots, walk_length, seed).reshape(-1))
