// tcgnn_compact.inc - relabelled mini-batch blocks: the kernels behind tcgnn_compact_* (include/tcgnn.h states the semantics).  Included by
// tcgnn_compact.hip alone - a translation unit of its own, so that every other object of the library compiles as it did; `make audit`
// lists this unit next to tcgnn_device.hip.
//
// From a byte mask `keep` over N nodes: new_id[v] = the number of kept nodes below v, or -1; nodes = the kept ids in increasing order;
// per graph, the row pointers of the kept nodes and every column id sent through new_id.
//
// Launch geometry, stated once: kCompactThreads threads = four wavefronts per workgroup, and every thread owns FOUR consecutive items
// (mask bytes, ids, edges), so that where the arrays are aligned a thread moves one dword of mask bytes or one dword x 4 of ids:
//   compact_mark_kernel     thread t: rows 4 t .. 4 t + 3 (a row with edges is kept) and edges 4 t .. 4 t + 3 (a column in range is kept)
//   compact_count_kernel    workgroup b sums keep != 0 over nodes kCompactScanRows b ... into sums[b]
//   compact_scan_sums_kernel  ONE workgroup turns sums[] into its exclusive sums, kCompactSumsPerPass at a step with a carry; res[1] = M
//   compact_offsets_kernel  the mask again, scanned inside the workgroup on top of sums[b]: new_id[v], v = 0 .. N - 1
//   compact_nodes_kernel    thread t: nodes[new_id[v]] = v for v = 4 t .. 4 t + 3
//   compact_graph_kernel    thread t: nodePointer_b[4 t .. 4 t + 3] through nodes, edgeList_b[4 t .. 4 t + 3] through new_id
//   compact_mark_ids_kernel   thread t: ids 4 t .. 4 t + 3 of a list (an id in range is kept)
//   compact_rows_graph_kernel thread t: nodePointer_b[4 t .. 4 t + 3] by a search over the row list, edgeList_b[4 t .. 4 t + 3] through new_id
// No global atomics: every output slot has one writer; the mask and the validation word only ever receive the same value (1) from
// whoever stores to them.  The scan is this file's own (block sums, one workgroup over the sums, offsets), for the reason
// tcgnn_sample.hip gives; it shares no code with tcgnn_sample.inc, whose kernels stay as they are.
// Every index read from the caller's arrays is checked or clamped before it is used as one.

namespace {

constexpr int kCompactThreads = 256;
constexpr int kCompactWaves = kCompactThreads / 64;
constexpr int kCompactItems = 4;                                      // consecutive items per thread
constexpr int kCompactScanRows = kCompactItems * kCompactThreads;     // mask entries per workgroup of the scan
constexpr int kCompactSumsPerPass = kCompactThreads;                  // block sums one pass of the scan's second level covers

// validation words of the workspace: res[0] != 0 - a mark call saw a bad id or pointer; res[1] = M
constexpr int kCompactResBad = 0, kCompactResTotal = 1;

// exclusive sum of v over the workgroup's threads in thread order; *total = the sum over all of them.  part: kCompactWaves words of LDS
__device__ __forceinline__ uint32_t compact_group_scan(uint32_t v, uint32_t* part, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t up = __shfl_up(incl, s);
        if (lane >= s) incl += up;
    }
    __syncthreads();   // (part may still be read from the call before)
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kCompactWaves; ++w) {
        const uint32_t p = part[w];
        if (w < wave) before += p;
        all += p;
    }
    *total = all;
    return before + incl - v;
}

// VEC: edgeList is 16-byte aligned, so a thread's four edges are one dword x 4 load
template <bool VEC>
__global__ __launch_bounds__(kCompactThreads) void compact_mark_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int32_t N,
                                                                       int64_t E, uint8_t* keep, uint32_t* res) {
    const int64_t first = ((int64_t)blockIdx.x * kCompactThreads + threadIdx.x) * kCompactItems;
    bool bad = false;
    if (first == 0) bad = rowptr[0] != 0 || (int64_t)rowptr[N] != E;
#pragma unroll
    for (int j = 0; j < kCompactItems; ++j) {
        const int64_t v = first + j;
        if (v < N) {
            const int32_t lo = rowptr[v], hi = rowptr[v + 1];
            bad |= lo > hi || lo < 0 || hi > E;
            if (hi > lo) keep[v] = 1;
        }
    }
    int32_t c[kCompactItems];
    int n = 0;
    if (first + kCompactItems <= E) {
        n = kCompactItems;
        if (VEC) {
            const int4 q = *reinterpret_cast<const int4*>(col + first);
            c[0] = q.x; c[1] = q.y; c[2] = q.z; c[3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < kCompactItems; ++j) c[j] = col[first + j];
        }
    } else if (first < E) {
        n = (int)(E - first);
#pragma unroll
        for (int j = 0; j < kCompactItems; ++j) c[j] = j < n ? col[first + j] : 0;
    }
#pragma unroll
    for (int j = 0; j < kCompactItems; ++j) {
        if (j < n) {
            if ((uint32_t)c[j] < (uint32_t)N) keep[c[j]] = 1;   // (a negative id is a large unsigned one)
            else bad = true;
        }
    }
    if (bad) res[kCompactResBad] = 1u;   // never followed; every thread that finds one stores the same 1
}

// keep != 0 of the thread's four nodes, as bits 0 .. 3.  WORD: keep is 4-byte aligned, four whole bytes are one dword
__device__ __forceinline__ uint32_t compact_kept_bits(const uint8_t* __restrict__ keep, int64_t first, int32_t N, bool word) {
    uint32_t bits = 0;
    if (word && first + kCompactItems <= N) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(keep + first);
#pragma unroll
        for (int j = 0; j < kCompactItems; ++j) bits |= ((w >> (8 * j)) & 255u) ? 1u << j : 0u;
    } else {
#pragma unroll
        for (int j = 0; j < kCompactItems; ++j)
            if (first + j < N && keep[first + j]) bits |= 1u << j;
    }
    return bits;
}

__global__ __launch_bounds__(kCompactThreads) void compact_count_kernel(const uint8_t* __restrict__ keep, int32_t N, bool word,
                                                                        uint32_t* __restrict__ sums) {
    __shared__ uint32_t part[kCompactWaves];
    const int64_t first = (int64_t)blockIdx.x * kCompactScanRows + (int64_t)kCompactItems * threadIdx.x;
    uint32_t total;
    compact_group_scan((uint32_t)__popc(compact_kept_bits(keep, first, N, word)), part, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kCompactThreads) void compact_scan_sums_kernel(uint32_t* __restrict__ sums, int64_t blocks, uint32_t* res) {
    __shared__ uint32_t part[kCompactWaves];
    uint32_t carry = 0;
    for (int64_t b0 = 0; b0 < blocks; b0 += kCompactSumsPerPass) {
        const int64_t b = b0 + threadIdx.x;
        const uint32_t v = b < blocks ? sums[b] : 0u;
        uint32_t total;
        const uint32_t before = compact_group_scan(v, part, &total);
        if (b < blocks) sums[b] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) res[kCompactResTotal] = carry;
}

// VEC: new_id is 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(kCompactThreads) void compact_offsets_kernel(const uint8_t* __restrict__ keep, int32_t N, bool word,
                                                                          const uint32_t* __restrict__ sums, int32_t* __restrict__ new_id) {
    __shared__ uint32_t part[kCompactWaves];
    const int64_t first = (int64_t)blockIdx.x * kCompactScanRows + (int64_t)kCompactItems * threadIdx.x;
    const uint32_t bits = compact_kept_bits(keep, first, N, word);
    uint32_t total;
    uint32_t at = sums[blockIdx.x] + compact_group_scan((uint32_t)__popc(bits), part, &total);
    int32_t id[kCompactItems];
#pragma unroll
    for (int j = 0; j < kCompactItems; ++j) {
        const bool k = (bits >> j) & 1u;
        id[j] = k ? (int32_t)at : -1;
        at += k;
    }
    if (VEC && first + kCompactItems <= N) {
        *reinterpret_cast<int4*>(new_id + first) = make_int4(id[0], id[1], id[2], id[3]);
    } else {
#pragma unroll
        for (int j = 0; j < kCompactItems; ++j)
            if (first + j < N) new_id[first + j] = id[j];
    }
}

template <bool VEC>
__global__ __launch_bounds__(kCompactThreads) void compact_nodes_kernel(const int32_t* __restrict__ new_id, int32_t N, int32_t M,
                                                                        int32_t* __restrict__ nodes) {
    const int64_t first = ((int64_t)blockIdx.x * kCompactThreads + threadIdx.x) * kCompactItems;
    int32_t id[kCompactItems];
    if (VEC && first + kCompactItems <= N) {
        const int4 q = *reinterpret_cast<const int4*>(new_id + first);
        id[0] = q.x; id[1] = q.y; id[2] = q.z; id[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < kCompactItems; ++j) id[j] = first + j < N ? new_id[first + j] : -1;
    }
#pragma unroll
    for (int j = 0; j < kCompactItems; ++j)
        if ((uint32_t)id[j] < (uint32_t)M) nodes[id[j]] = (int32_t)(first + j);
}

// VEC: edgeList and edgeList_b are 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(kCompactThreads) void compact_graph_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                        const int32_t* __restrict__ new_id, const int32_t* __restrict__ nodes,
                                                                        int32_t N, int32_t M, int64_t E, int32_t* __restrict__ rowptr_b,
                                                                        int32_t* __restrict__ col_b) {
    const int64_t first = ((int64_t)blockIdx.x * kCompactThreads + threadIdx.x) * kCompactItems;
    // row pointers: slot i < M is the kept node's own, slot M the edge count
#pragma unroll
    for (int j = 0; j < kCompactItems; ++j) {
        const int64_t i = first + j;
        if (i < M) {
            const int32_t v = nodes[i];
            int64_t p = (uint32_t)v < (uint32_t)N ? (int64_t)rowptr[v] : 0;
            p = p < 0 ? 0 : (p > E ? E : p);
            rowptr_b[i] = (int32_t)p;
        } else if (i == M) {
            rowptr_b[i] = (int32_t)E;
        }
    }
    if (first >= E) return;
    const bool whole = first + kCompactItems <= E;
    const int n = whole ? kCompactItems : (int)(E - first);
    int32_t c[kCompactItems];
    if (VEC && whole) {
        const int4 q = *reinterpret_cast<const int4*>(col + first);
        c[0] = q.x; c[1] = q.y; c[2] = q.z; c[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < kCompactItems; ++j) c[j] = j < n ? col[first + j] : -1;
    }
#pragma unroll
    for (int j = 0; j < kCompactItems; ++j) {   // the gather through new_id: a column without a new id becomes 0
        const int32_t id = (uint32_t)c[j] < (uint32_t)N ? new_id[c[j]] : -1;
        c[j] = (uint32_t)id < (uint32_t)M ? id : 0;
    }
    if (VEC && whole) {
        *reinterpret_cast<int4*>(col_b + first) = make_int4(c[0], c[1], c[2], c[3]);
    } else {
#pragma unroll
        for (int j = 0; j < kCompactItems; ++j)
            if (j < n) col_b[first + j] = c[j];
    }
}

// ---- row-list graphs (tcgnn_sample_rows' results): the same node set and blocks without the N-row CSRs in between.

// keep[id] = 1 for a list of ids (seeds, the columns of a row-list graph); thread t: ids 4 t .. 4 t + 3.  VEC: ids is 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(kCompactThreads) void compact_mark_ids_kernel(const int32_t* __restrict__ ids, int64_t count, int32_t N, uint8_t* keep,
                                                                           uint32_t* res) {
    const int64_t first = ((int64_t)blockIdx.x * kCompactThreads + threadIdx.x) * kCompactItems;
    if (first >= count) return;
    const bool whole = first + kCompactItems <= count;
    const int n = whole ? kCompactItems : (int)(count - first);
    int32_t c[kCompactItems];
    if (VEC && whole) {
        const int4 q = *reinterpret_cast<const int4*>(ids + first);
        c[0] = q.x; c[1] = q.y; c[2] = q.z; c[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < kCompactItems; ++j) c[j] = j < n ? ids[first + j] : 0;
    }
    bool bad = false;
#pragma unroll
    for (int j = 0; j < kCompactItems; ++j) {
        if (j < n) {
            if ((uint32_t)c[j] < (uint32_t)N) keep[c[j]] = 1;   // (a negative id is a large unsigned one)
            else bad = true;
        }
    }
    if (bad) res[kCompactResBad] = 1u;   // never followed; every thread that finds one stores the same 1
}

// the block position of list slot i: new_id[rows[i]], or -1 where either index fails its check
__device__ __forceinline__ int32_t compact_list_pos(const int32_t* __restrict__ rows, const int32_t* __restrict__ new_id, int32_t i, int32_t N) {
    const int32_t v = rows[i];
    return (uint32_t)v < (uint32_t)N ? new_id[v] : -1;
}

// The square M-node block of a row-list graph whose R rows are strictly increasing.  Thread t owns row-pointer slots 4 t .. 4 t + 3 and
// edges 4 t .. 4 t + 3.  Slot j <= M: new_id is monotone over increasing rows, so #{i : new_id[rows[i]] < j} is the lower bound of j in
// the list's block positions - a binary search over [0, R], whose result indexes rowptr_s [R + 1] whatever the arrays hold.
// VEC: edgeList_s and edgeList_b are 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(kCompactThreads) void compact_rows_graph_kernel(const int32_t* __restrict__ rows, int32_t R,
                                                                             const int32_t* __restrict__ rowptr_s, const int32_t* __restrict__ col,
                                                                             int64_t E, const int32_t* __restrict__ new_id, int32_t N, int32_t M,
                                                                             int32_t* __restrict__ rowptr_b, int32_t* __restrict__ col_b) {
    const int64_t first = ((int64_t)blockIdx.x * kCompactThreads + threadIdx.x) * kCompactItems;
#pragma unroll
    for (int j = 0; j < kCompactItems; ++j) {
        const int64_t slot = first + j;
        if (slot < M) {
            int32_t lo = 0, hi = R;   // the first list slot whose block position is >= slot
            while (lo < hi) {
                const int32_t mid = lo + ((hi - lo) >> 1);
                if (compact_list_pos(rows, new_id, mid, N) < (int32_t)slot) lo = mid + 1;
                else hi = mid;
            }
            int64_t p = rowptr_s[lo];
            p = p < 0 ? 0 : (p > E ? E : p);
            rowptr_b[slot] = (int32_t)p;
        } else if (slot == M) {
            rowptr_b[slot] = (int32_t)E;
        }
    }
    if (first >= E) return;
    const bool whole = first + kCompactItems <= E;
    const int n = whole ? kCompactItems : (int)(E - first);
    int32_t c[kCompactItems];
    if (VEC && whole) {
        const int4 q = *reinterpret_cast<const int4*>(col + first);
        c[0] = q.x; c[1] = q.y; c[2] = q.z; c[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < kCompactItems; ++j) c[j] = j < n ? col[first + j] : -1;
    }
#pragma unroll
    for (int j = 0; j < kCompactItems; ++j) {   // the gather through new_id: a column without a new id becomes 0
        const int32_t id = (uint32_t)c[j] < (uint32_t)N ? new_id[c[j]] : -1;
        c[j] = (uint32_t)id < (uint32_t)M ? id : 0;
    }
    if (VEC && whole) {
        *reinterpret_cast<int4*>(col_b + first) = make_int4(c[0], c[1], c[2], c[3]);
    } else {
#pragma unroll
        for (int j = 0; j < kCompactItems; ++j)
            if (j < n) col_b[first + j] = c[j];
    }
}

inline bool compact_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// workgroups whose threads own `items` items, four a thread
inline unsigned compact_grid(int64_t items) {
    const int64_t per = (int64_t)kCompactThreads * kCompactItems;
    return (unsigned)((items + per - 1) / per);
}

int64_t compact_scan_blocks(int32_t N) { return ((int64_t)N + kCompactScanRows - 1) / kCompactScanRows; }

int compact_mark(const int32_t* rowptr, const int32_t* col, int32_t N, int64_t E, uint8_t* keep, uint32_t* res, hipStream_t stream) {
    const dim3 grid(compact_grid(N > E ? (int64_t)N : E)), block(kCompactThreads);
    if (grid.x == 0) return (int)hipSuccess;
    if (compact_aligned(col, 16)) hipLaunchKernelGGL(compact_mark_kernel<true>, grid, block, 0, stream, rowptr, col, N, E, keep, res);
    else hipLaunchKernelGGL(compact_mark_kernel<false>, grid, block, 0, stream, rowptr, col, N, E, keep, res);
    return (int)hipGetLastError();
}

// new_id and res[kCompactResTotal]; sums: compact_scan_blocks(N) words of scratch
int compact_count(const uint8_t* keep, int32_t N, uint32_t* sums, uint32_t* res, int32_t* new_id, hipStream_t stream) {
    const int64_t blocks = compact_scan_blocks(N);
    const bool word = compact_aligned(keep, 4);
    const dim3 grid((unsigned)blocks), block(kCompactThreads);
    if (blocks > 0) hipLaunchKernelGGL(compact_count_kernel, grid, block, 0, stream, keep, N, word, sums);
    hipLaunchKernelGGL(compact_scan_sums_kernel, dim3(1), block, 0, stream, sums, blocks, res);
    if (blocks > 0) {
        if (compact_aligned(new_id, 16)) hipLaunchKernelGGL(compact_offsets_kernel<true>, grid, block, 0, stream, keep, N, word, sums, new_id);
        else hipLaunchKernelGGL(compact_offsets_kernel<false>, grid, block, 0, stream, keep, N, word, sums, new_id);
    }
    return (int)hipGetLastError();
}

int compact_nodes(const int32_t* new_id, int32_t N, int32_t M, int32_t* nodes, hipStream_t stream) {
    const dim3 grid(compact_grid(N)), block(kCompactThreads);
    if (grid.x == 0 || M == 0) return (int)hipSuccess;
    if (compact_aligned(new_id, 16)) hipLaunchKernelGGL(compact_nodes_kernel<true>, grid, block, 0, stream, new_id, N, M, nodes);
    else hipLaunchKernelGGL(compact_nodes_kernel<false>, grid, block, 0, stream, new_id, N, M, nodes);
    return (int)hipGetLastError();
}

int compact_graph(const int32_t* rowptr, const int32_t* col, const int32_t* new_id, const int32_t* nodes, int32_t N, int32_t M, int64_t E,
                  int32_t* rowptr_b, int32_t* col_b, hipStream_t stream) {
    const int64_t slots = (int64_t)M + 1;
    const dim3 grid(compact_grid(slots > E ? slots : E)), block(kCompactThreads);
    if (compact_aligned(col, 16) && compact_aligned(col_b, 16))
        hipLaunchKernelGGL(compact_graph_kernel<true>, grid, block, 0, stream, rowptr, col, new_id, nodes, N, M, E, rowptr_b, col_b);
    else
        hipLaunchKernelGGL(compact_graph_kernel<false>, grid, block, 0, stream, rowptr, col, new_id, nodes, N, M, E, rowptr_b, col_b);
    return (int)hipGetLastError();
}

int compact_mark_ids(const int32_t* ids, int64_t count, int32_t N, uint8_t* keep, uint32_t* res, hipStream_t stream) {
    const dim3 grid(compact_grid(count)), block(kCompactThreads);
    if (grid.x == 0) return (int)hipSuccess;
    if (compact_aligned(ids, 16)) hipLaunchKernelGGL(compact_mark_ids_kernel<true>, grid, block, 0, stream, ids, count, N, keep, res);
    else hipLaunchKernelGGL(compact_mark_ids_kernel<false>, grid, block, 0, stream, ids, count, N, keep, res);
    return (int)hipGetLastError();
}

int compact_rows_graph(const int32_t* rows, int32_t R, const int32_t* rowptr_s, const int32_t* col, int64_t E, const int32_t* new_id, int32_t N,
                       int32_t M, int32_t* rowptr_b, int32_t* col_b, hipStream_t stream) {
    const int64_t slots = (int64_t)M + 1;
    const dim3 grid(compact_grid(slots > E ? slots : E)), block(kCompactThreads);
    if (compact_aligned(col, 16) && compact_aligned(col_b, 16))
        hipLaunchKernelGGL(compact_rows_graph_kernel<true>, grid, block, 0, stream, rows, R, rowptr_s, col, E, new_id, N, M, rowptr_b, col_b);
    else
        hipLaunchKernelGGL(compact_rows_graph_kernel<false>, grid, block, 0, stream, rows, R, rowptr_s, col, E, new_id, N, M, rowptr_b, col_b);
    return (int)hipGetLastError();
}

} // namespace
