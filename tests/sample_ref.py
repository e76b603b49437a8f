"""numpy restatement of the seeded neighbour sampler (include/tcgnn.h, "Seeded neighbour sampling"), and the graphs its tests use.

Every CSR position e carries word(seed, e) = (h32(seed, e) << 32) | e; a row of degree d keeps all its edges when d <= k and else
the k positions with the smallest words, in CSR order; a row whose mask entry is 0 keeps none.  Nothing here shares code with the
library: uint64 arithmetic and np.argsort of the words per row."""
import numpy as np

G = np.uint64(0x9E3779B97F4A7C15)
C1 = np.uint64(0xBF58476D1CE4E5B9)
C2 = np.uint64(0x94D049BB133111EB)
WAVE_ROW = 1024   # the library's class boundary: rows up to here are selected by one wavefront, longer ones by a workgroup


def mix(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * C1
        z = (z ^ (z >> np.uint64(27))) * C2
    return z ^ (z >> np.uint64(31))


def h32(seed, e):
    """h32(seed, e) of every position in e (any integer array), as uint64 values below 2^32"""
    with np.errstate(over="ignore"):
        s = mix(np.uint64(int(seed) % (1 << 64)) + G)
        return mix(s + (np.asarray(e, dtype=np.uint64) + np.uint64(1)) * G) >> np.uint64(32)


def words(seed, e):
    e = np.asarray(e, dtype=np.uint64)
    return (h32(seed, e) << np.uint64(32)) | e


def sample_neighbors(rp, col, k, seed, mask=None):
    """(rp_s, col_s, eid) int32.  k=None keeps every edge of the unmasked rows.  Only col[:rp[-1]] is looked at."""
    rp = np.asarray(rp, dtype=np.int64)
    n = len(rp) - 1
    kept = []
    counts = np.zeros(n, dtype=np.int64)
    for r in range(n):
        lo, hi = int(rp[r]), int(rp[r + 1])
        d = hi - lo
        if d == 0 or (mask is not None and not mask[r]) or (k is not None and k == 0):
            continue
        pos = np.arange(lo, hi, dtype=np.int64)
        if k is not None and d > k:
            order = np.argsort(words(seed, pos), kind="stable")
            pos = np.sort(pos[order[:k]])
        kept.append(pos)
        counts[r] = len(pos)
    eid = np.concatenate(kept).astype(np.int32) if kept else np.zeros(0, np.int32)
    rp_s = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return rp_s, np.asarray(col)[eid].astype(np.int32), eid


def brute_force_row(seed, lo, d, k):
    """the kept positions of one unmasked row, from Python integers alone (no numpy arithmetic): the check of the restatement"""
    M = (1 << 64) - 1

    def mx(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    s = mx((int(seed) % (1 << 64) + 0x9E3779B97F4A7C15) & M)
    w = sorted(((mx((s + (e + 1) * 0x9E3779B97F4A7C15) & M) >> 32) << 32) | e for e in range(lo, lo + d))
    return sorted(x & 0xFFFFFFFF for x in (w if d <= k else w[:k]))


# ---------------------------------------------------------------- graphs

N_ROWS = 2048
NO_ROW = 24       # entries of edgeList behind nodePointer[N], holding ids no node has
ROW_LENGTHS = (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4099)   # (WAVE_ROW and WAVE_ROW +- 1 are among them)
LONG_ROW = 70000
_ROW_GRAPH = []


def row_length_graph():
    """N_ROWS nodes: two rows of each of ROW_LENGTHS and one of LONG_ROW edges, scattered among 600 short rows and empty ones;
    columns drawn with repetition; NO_ROW uncovered entries holding out-of-range ids behind the last row.  -> (rp, col, long_row)"""
    if not _ROW_GRAPH:
        lens = [ln for ln in ROW_LENGTHS for _ in range(2)] + [LONG_ROW]
        rng = np.random.default_rng(26)
        order = rng.permutation(N_ROWS)
        cols_all = [np.zeros(0, np.int32)] * N_ROWS
        for i, ln in enumerate(lens):
            cols_all[order[i]] = rng.integers(0, N_ROWS, ln).astype(np.int32)
        for r in order[len(lens):len(lens) + 600]:
            cols_all[r] = rng.integers(0, N_ROWS, int(rng.integers(1, 40))).astype(np.int32)
        rp = np.concatenate([[0], np.cumsum([len(c) for c in cols_all])]).astype(np.int32)
        col = np.concatenate(cols_all + [np.full(NO_ROW, 0x7FFFFFF0, np.int32)]).astype(np.int32)
        _ROW_GRAPH.append((rp, col, int(order[len(lens) - 1])))
    return _ROW_GRAPH[0]


def equal_hash_pair(rp, row, seeds=range(16)):
    """(seed, k) such that two positions of `row` have the same h32 under `seed` and exactly the earlier one is among the k smallest
    words - a select that looks at the hashed half alone can not tell them apart - or None"""
    lo, hi = int(rp[row]), int(rp[row + 1])
    pos = np.arange(lo, hi, dtype=np.int64)
    for seed in seeds:
        w = np.sort(words(seed, pos))
        same = np.nonzero((w[1:] >> np.uint64(32)) == (w[:-1] >> np.uint64(32)))[0]
        if len(same):
            return int(seed), int(same[0]) + 1   # ranks same[0] and same[0] + 1 (0-based): keep same[0] + 1 words
    return None
