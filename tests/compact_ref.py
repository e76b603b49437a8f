"""numpy restatement of the relabelled mini-batch blocks (include/tcgnn.h, "Relabelled mini-batch blocks").

Inputs: one or more CSRs over the same N nodes and an optional byte mask `keep` of N entries.  A node v is kept when keep[v] != 0, when
v has at least one edge or when v is a column id, in any of the graphs.  nodes = the kept ids, increasing; new_id[v] = the rank of v in
nodes, or -1; per graph nodePointer_b[i] = nodePointer[nodes[i]], nodePointer_b[M] = E, edgeList_b[e] = new_id[edgeList[e]].
Nothing here shares code with the library: boolean masks, np.nonzero and fancy indexing."""
import numpy as np

# the library's launch geometry (csrc/tcgnn_compact.inc), for the size classes of the tests
SCAN_ROWS = 1024       # S: mask entries one workgroup of the scan covers
SUMS_PER_PASS = 256    # C: block sums one pass of the scan's second level covers


def kept_mask(graphs, n, keep=None):
    mask = np.zeros(n, dtype=bool) if keep is None else (np.asarray(keep).reshape(-1) != 0)
    assert mask.shape == (n,)
    mask = mask.copy()
    for rp, col in graphs:
        rp = np.asarray(rp, dtype=np.int64)
        assert len(rp) == n + 1
        mask |= np.diff(rp) > 0
        mask[np.asarray(col[:rp[-1]], dtype=np.int64)] = True
    return mask


def compact_nodes(graphs, keep=None):
    """(nodes int32 [M], new_id int32 [N])"""
    n = len(graphs[0][0]) - 1
    mask = kept_mask(graphs, n, keep)
    nodes = np.nonzero(mask)[0].astype(np.int32)
    new_id = np.full(n, -1, dtype=np.int32)
    new_id[nodes] = np.arange(len(nodes), dtype=np.int32)
    return nodes, new_id


def compact_graph(rp, col, nodes, new_id):
    """(nodePointer_b int32 [M + 1], edgeList_b int32 [E])"""
    rp = np.asarray(rp)
    e = int(rp[-1])
    rp_b = np.concatenate([rp[nodes], [e]]).astype(np.int32)
    return rp_b, new_id[np.asarray(col[:e], dtype=np.int64)].astype(np.int32)


def compact(graphs, keep=None):
    """-> (nodes, new_id, [(nodePointer_b, edgeList_b) per graph])"""
    nodes, new_id = compact_nodes(graphs, keep)
    return nodes, new_id, [compact_graph(rp, col, nodes, new_id) for rp, col in graphs]


def check_properties(graphs, keep, nodes, new_id, blocks):
    """the properties that need no second implementation; every argument a numpy array"""
    n = len(graphs[0][0]) - 1
    m = len(nodes)
    assert nodes.dtype == np.int32 and new_id.dtype == np.int32 and new_id.shape == (n,)
    assert np.all(np.diff(nodes.astype(np.int64)) > 0), "nodes is not strictly increasing"
    assert m == 0 or (nodes[0] >= 0 and nodes[-1] < n)
    assert np.array_equal(new_id[nodes], np.arange(m)), "new_id[nodes] is not 0 .. M - 1"
    outside = np.ones(n, dtype=bool)
    outside[nodes] = False
    assert np.all(new_id[outside] == -1), "a node outside nodes has a new id"
    if keep is not None:
        assert np.all(new_id[np.asarray(keep).reshape(-1) != 0] >= 0), "a node of keep was dropped"
    for (rp, col), (rp_b, col_b) in zip(graphs, blocks):
        rp = np.asarray(rp, dtype=np.int64)
        e = int(rp[-1])
        assert rp_b.dtype == np.int32 and col_b.dtype == np.int32 and rp_b.shape == (m + 1,) and col_b.shape == (e,)
        assert np.array_equal(nodes[col_b], np.asarray(col[:e])), "nodes[edgeList_b] is not edgeList"
        d = np.diff(rp)
        assert np.array_equal(np.diff(rp_b.astype(np.int64)), d[nodes]), "a kept row changed its length"
        assert d.sum() == d[nodes].sum(), "a row with edges was dropped"
        assert rp_b[m] == e and rp_b[0] == 0   # (with the lengths above: every pointer; rows in front of the first kept one are empty)
    # the same by numpy.unique over everything that names a node
    parts = [np.nonzero(np.asarray(keep).reshape(-1) != 0)[0]] if keep is not None else []
    for rp, col in graphs:
        rp = np.asarray(rp, dtype=np.int64)
        parts += [np.nonzero(np.diff(rp) > 0)[0], np.asarray(col[:rp[-1]], dtype=np.int64)]
    named = np.concatenate(parts).astype(np.int64)
    uniq, inverse = np.unique(named, return_inverse=True)
    assert np.array_equal(uniq, nodes), "nodes is not numpy.unique of the seeds, rows and columns"
    assert np.array_equal(new_id[named], inverse.reshape(-1)), "new_id is not numpy.unique's inverse"
