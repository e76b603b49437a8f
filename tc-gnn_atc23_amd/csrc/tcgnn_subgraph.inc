// tcgnn_subgraph.inc - subgraph sampling: the kernels behind tcgnn_random_walk and tcgnn_induce* (include/tcgnn.h states the semantics).
// Included by tcgnn_subgraph.hip alone - a translation unit of its own, so that every other object of the library compiles as it did;
// `make audit` lists this unit next to tcgnn_device.hip and tcgnn_compact.hip.  It restates the few lines it shares with
// tcgnn_sample.inc (h32's mixer, the lane rank, the saturating workgroup scan): that file also defines the sampler's launchers, which
// must not be compiled twice.
//
// random_walk_kernel     one lane per walk: `length` dependent steps of three loads (two row pointers, one column id).
//
// The node-induced subgraph of a CSR over a strictly increasing node list nodes[0 .. M): row i of the result holds, in CSR order, the
// positions e of row nodes[i] whose column has a new id (new_id[col[e]] >= 0).  Launch geometry, stated once: kInduceThreads threads =
// four wavefronts per workgroup, workgroup b owns list slots 4 b .. 4 b + 3, as sample_rows_select_kernel owns them:
//   1. wavefront w takes slot 4 b + w when its row holds at most kInduceWaveRow edges, 256 positions at a step;
//   2. then the whole workgroup walks the (rare) longer rows among its four, one after the other, 1 024 positions at a step.
// Either way a thread owns FOUR consecutive positions of a step, cut so that they are one aligned dword x 4 load wherever the row starts
// (induce_quad); positions of the quad outside the row are masked, a quad that would leave edgeList is read entry by entry.  The
// compaction keeps the order: four ballots, one per position of the quad, and the number of set bits below the lane give the offset
// of a lane's first kept edge; across wavefronts the per-wavefront totals go through LDS.
//   induce_rows_kernel<false>   the count of every listed row into nodePointer_b[i], and the validation words
//   induce_sums_kernel          workgroup b sums the counts of slots kInduceScanRows b ... into sums[b]
//   induce_scan_sums_kernel     ONE workgroup turns sums[] into its exclusive sums, 256 at a step with a carry; res[kInduceResTotal] = E_b
//   induce_offsets_kernel       the counts again, scanned inside the workgroup on top of sums[b], IN PLACE: nodePointer_b[i], i = 0 .. M
//   induce_rows_kernel<true>    the same walk, the same predicate on the same data, writing edgeList_b and eid
// No global atomics: every output slot has one writer, fixed by the row pointers the count call wrote.  Every index read from the
// caller's arrays is checked or clamped before it is used as one, and every store of the write pass is bounded by the end of its row's
// slot and by E_b.  Every add of the scan saturates at kInduceSumCap (a list with repeats can pass 2^31 - 1), which as an int32 row
// pointer is negative: the write pass keeps nothing behind it.

namespace {

constexpr int kInduceThreads = 256;
constexpr int kInduceWaves = kInduceThreads / 64;
constexpr int kInduceQuad = 4;                                    // consecutive positions per thread and step
constexpr int kInduceWaveRow = 1024;                              // longest row one wavefront takes (kSampleWaveRow)
constexpr int kInduceScanRows = 4 * kInduceThreads;               // list slots per workgroup of the scan
constexpr uint64_t kInduceG = 0x9E3779B97F4A7C15ull;
constexpr uint32_t kInduceSumCap = 0x80000000u;

// validation words of the workspace
constexpr int kInduceResBadId = 0, kInduceResBadPtr = 1, kInduceResDescending = 2, kInduceResBadCol = 3, kInduceResTotal = 4;
constexpr uint32_t kInduceFaultId = 1u, kInduceFaultPtr = 2u, kInduceFaultDescending = 4u, kInduceFaultCol = 8u;

// h32 of the counter whose pre-mixed word is x = mix(seed + G) + (i + 1) G
__device__ __forceinline__ uint32_t induce_h32(uint64_t x) {
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((x ^ (x >> 31)) >> 32);
}

// set bits of `m` below this lane
__device__ __forceinline__ int induce_rank(uint64_t m) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ __forceinline__ int64_t induce_clamp(int64_t p, int64_t E) { return p < 0 ? 0 : (p > E ? E : p); }

// ---- the walk: thread w owns walk w.  Step t draws h32(seed, w length + t); x carries mix(seed + G) + (w length + t + 1) G
__global__ __launch_bounds__(kInduceThreads) void random_walk_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                     const int32_t* __restrict__ starts, int32_t W, int32_t N, int64_t E,
                                                                     int32_t length, uint64_t S, int32_t* __restrict__ walks) {
    const int64_t w = (int64_t)blockIdx.x * kInduceThreads + threadIdx.x;
    if (w >= W) return;
    int32_t v = starts[w];
    int32_t* const out = walks + w * ((int64_t)length + 1);
    out[0] = v;
    uint64_t x = S + ((uint64_t)w * (uint64_t)length + 1u) * kInduceG;
    for (int32_t t = 0; t < length; ++t, x += kInduceG) {
        if ((uint32_t)v < (uint32_t)N) {   // (a negative id is a large unsigned one: written, not followed)
            const int64_t lo = induce_clamp(rowptr[v], E), hi = induce_clamp(rowptr[v + 1], E);
            if (hi > lo) v = col[lo + (int64_t)(((uint64_t)induce_h32(x) * (uint64_t)(hi - lo)) >> 32)];
        }
        out[t + 1] = v;
    }
}

// ---- induce

// A listed row as both passes see it: first position, one past the last (lo <= hi, both in [0, E])
struct InduceRow { int64_t lo, hi; };

__device__ __forceinline__ InduceRow induce_row(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ nodes, int64_t slot, int32_t N,
                                                int64_t E, uint32_t& faults) {
    const int32_t v = nodes[slot];
    int64_t lo = 0, hi = 0;
    if ((uint32_t)v < (uint32_t)N) {
        lo = rowptr[v];
        hi = rowptr[v + 1];
        if (lo < 0 || lo > E || hi < 0 || hi > E) faults |= kInduceFaultPtr;
        if (lo > hi) faults |= kInduceFaultDescending;
    } else {
        faults |= kInduceFaultId;
    }
    InduceRow r;
    r.lo = induce_clamp(lo, E);
    r.hi = induce_clamp(hi, E);
    if (r.hi < r.lo) r.hi = r.lo;
    return r;
}

// Positions p .. p + 3 (col + p is 16-byte aligned): bit j of the result = position p + j lies in the row and its column has a new id,
// which is then id[j] (a new id outside [0, M) is written as 0).  THE predicate of both passes.
__device__ __forceinline__ uint32_t induce_quad(const int32_t* __restrict__ col, const int32_t* __restrict__ new_id, int64_t p, const InduceRow& r,
                                                int32_t N, int32_t M, int64_t E, int32_t (&id)[kInduceQuad], uint32_t& faults) {
    if (p >= r.hi || p + kInduceQuad <= r.lo) return 0u;
    int32_t c[kInduceQuad];
    if (p >= 0 && p + kInduceQuad <= E) {
        const int4 q = *reinterpret_cast<const int4*>(col + p);
        c[0] = q.x; c[1] = q.y; c[2] = q.z; c[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < kInduceQuad; ++j) c[j] = (p + j >= r.lo && p + j < r.hi) ? col[p + j] : 0;
    }
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < kInduceQuad; ++j) {
        id[j] = 0;
        if (p + j >= r.lo && p + j < r.hi) {
            if ((uint32_t)c[j] < (uint32_t)N) {   // (a negative id is a large unsigned one)
                const int32_t n = new_id[c[j]];
                if (n >= 0) {
                    bits |= 1u << j;
                    id[j] = (uint32_t)n < (uint32_t)M ? n : 0;
                }
            } else {
                faults |= kInduceFaultCol;   // dropped
            }
        }
    }
    return bits;
}

// One step of a wavefront: the kept edges of a lane's quad go to out + (the kept edges of the step's lower lanes) ..., bounded by
// `end`; `out` already counts what lower wavefronts of the step keep.  Returns the wavefront's kept edges of the step.
template <bool WRITE>
__device__ __forceinline__ uint32_t induce_wave_step(uint32_t bits, const int32_t (&id)[kInduceQuad], int64_t p, int64_t out, int64_t end,
                                                     int32_t* __restrict__ col_b, int32_t* __restrict__ eid, uint64_t (&m)[kInduceQuad]) {
    uint32_t total = 0;
#pragma unroll
    for (int j = 0; j < kInduceQuad; ++j) {
        m[j] = __ballot((bits >> j) & 1u);
        total += (uint32_t)__popcll(m[j]);
    }
    if (WRITE && bits) {
        int64_t at = out;
#pragma unroll
        for (int j = 0; j < kInduceQuad; ++j) at += induce_rank(m[j]);
#pragma unroll
        for (int j = 0; j < kInduceQuad; ++j) {
            if ((bits >> j) & 1u) {
                if (at < end) {
                    col_b[at] = id[j];
                    eid[at] = (int32_t)(p + j);
                }
                ++at;
            }
        }
    }
    return total;
}

// the first position of the walk: the last one at or below lo at which col is 16-byte aligned (it may be negative: induce_quad masks)
__device__ __forceinline__ int64_t induce_first(const int32_t* col, int64_t lo) {
    const int64_t shift = (int64_t)((reinterpret_cast<uintptr_t>(col) >> 2) & 3u);
    return lo - ((lo + shift) & 3);
}

// WRITE = false: nodePointer_b[i] = the count of list slot i, and the validation words.  WRITE = true: nodePointer_b holds the offsets.
template <bool WRITE>
__global__ __launch_bounds__(kInduceThreads) void induce_rows_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                     const int32_t* __restrict__ nodes, const int32_t* __restrict__ new_id,
                                                                     int32_t M, int32_t N, int64_t E, int64_t Eb, int32_t* rowptr_b,
                                                                     int32_t* __restrict__ col_b, int32_t* __restrict__ eid, uint32_t* res) {
    __shared__ uint32_t part[2][kInduceWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t first = (int64_t)blockIdx.x * kInduceWaves;
    uint32_t faults = 0;
    int32_t id[kInduceQuad];
    uint64_t m[kInduceQuad];
    const int64_t mine = first + wave;
    if (mine < M) {
        const InduceRow r = induce_row(rowptr, nodes, mine, N, E, faults);
        if (r.hi - r.lo <= kInduceWaveRow) {
            int64_t out = 0, end = 0;
            if (WRITE) {   // (an offset the count call did not write: nothing rather than beyond the slot)
                out = rowptr_b[mine];
                end = rowptr_b[mine + 1];
                if (end > Eb) end = Eb;
                if (out < 0) end = 0;
            }
            uint32_t count = 0;
            for (int64_t base = induce_first(col, r.lo); base < r.hi; base += 64 * kInduceQuad) {   // (wave-uniform)
                const int64_t p = base + kInduceQuad * lane;
                const uint32_t bits = induce_quad(col, new_id, p, r, N, M, E, id, faults);
                const uint32_t kept = induce_wave_step<WRITE>(bits, id, p, out, end, col_b, eid, m);
                out += kept;
                count += kept;
            }
            if (!WRITE && lane == 0) rowptr_b[mine] = (int32_t)count;   // (at most kInduceWaveRow)
        }
    }
    for (int q = 0; q < kInduceWaves; ++q) {   // the same slots for every thread: the barriers inside are uniform
        const int64_t slot = first + q;
        if (slot >= M) break;
        uint32_t ignored = 0;   // (the slot's own wavefront has reported its pointers)
        const InduceRow r = induce_row(rowptr, nodes, slot, N, E, ignored);
        if (r.hi - r.lo <= kInduceWaveRow) continue;
        int64_t out = 0, end = 0;
        if (WRITE) {
            out = rowptr_b[slot];
            end = rowptr_b[slot + 1];
            if (end > Eb) end = Eb;
            if (out < 0) end = 0;
        }
        uint32_t count = 0;
        int buf = 0;
        for (int64_t base = induce_first(col, r.lo); base < r.hi; base += kInduceThreads * kInduceQuad, buf ^= 1) {
            const int64_t p = base + kInduceQuad * (int64_t)threadIdx.x;
            const uint32_t bits = induce_quad(col, new_id, p, r, N, M, E, id, faults);
            uint32_t mine_kept = 0;
#pragma unroll
            for (int j = 0; j < kInduceQuad; ++j) mine_kept += (uint32_t)__popcll(__ballot((bits >> j) & 1u));
            // the two halves of part alternate: a wavefront writes part[buf] again only behind the barrier of the step in between
            if (lane == 0) part[buf][wave] = mine_kept;
            __syncthreads();
            uint32_t before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < kInduceWaves; ++w) {
                const uint32_t k = part[buf][w];
                if (w < wave) before += k;
                all += k;
            }
            if (WRITE) induce_wave_step<true>(bits, id, p, out + before, end, col_b, eid, m);
            out += all;
            count += all;   // (at most E <= 2^31 - 1)
        }
        if (!WRITE && threadIdx.x == 0) rowptr_b[slot] = (int32_t)count;
        __syncthreads();   // (the next long row of this workgroup starts on part[0] again)
    }
    if (!WRITE) {   // every thread that finds a fault stores the same 1
        if (faults & kInduceFaultId) res[kInduceResBadId] = 1u;
        if (faults & kInduceFaultPtr) res[kInduceResBadPtr] = 1u;
        if (faults & kInduceFaultDescending) res[kInduceResDescending] = 1u;
        if (faults & kInduceFaultCol) res[kInduceResBadCol] = 1u;
    }
}

// ---- the scan of the counts: sample_rows_count's three-launch pattern (block sums, one workgroup over the sums, offsets) over the
// M + 1 slots of nodePointer_b (slot M: the total), every add saturating

__device__ __forceinline__ uint32_t induce_sat_add(uint32_t a, uint32_t b) {   // a, b <= kInduceSumCap
    const uint64_t s = (uint64_t)a + b;
    return s > kInduceSumCap ? kInduceSumCap : (uint32_t)s;
}

// exclusive sum of v over the workgroup's threads in thread order, *total over all of them.  part: kInduceWaves words of LDS
__device__ __forceinline__ uint32_t induce_group_scan_sat(uint32_t v, uint32_t* part, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t up = __shfl_up(incl, s);
        if (lane >= s) incl = induce_sat_add(incl, up);
    }
    const uint32_t below = __shfl_up(incl, 1);
    const uint32_t excl = lane ? below : 0u;
    __syncthreads();   // (part may still be read from the call before)
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kInduceWaves; ++w) {
        const uint32_t p = part[w];
        if (w < wave) before = induce_sat_add(before, p);
        all = induce_sat_add(all, p);
    }
    *total = all;
    return induce_sat_add(before, excl);
}

// the count of slot i as the rows kernel left it (a count is at most E; anything else is not a count: 0)
__device__ __forceinline__ uint32_t induce_slot_count(const int32_t* counts, int64_t i, int32_t M) {
    if (i >= M) return 0u;   // (slot M: the total)
    const int32_t c = counts[i];
    return c > 0 ? (uint32_t)c : 0u;
}

__global__ __launch_bounds__(kInduceThreads) void induce_sums_kernel(const int32_t* counts, int32_t M, uint32_t* __restrict__ sums) {
    __shared__ uint32_t part[kInduceWaves];
    const int64_t first = (int64_t)blockIdx.x * kInduceScanRows + 4 * (int64_t)threadIdx.x;
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) c = induce_sat_add(c, induce_slot_count(counts, first + j, M));
    uint32_t total;
    induce_group_scan_sat(c, part, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kInduceThreads) void induce_scan_sums_kernel(uint32_t* __restrict__ sums, int64_t blocks, uint32_t* res) {
    __shared__ uint32_t part[kInduceWaves];
    uint32_t carry = 0;
    for (int64_t b0 = 0; b0 < blocks; b0 += kInduceThreads) {
        const int64_t b = b0 + threadIdx.x;
        const uint32_t v = b < blocks ? sums[b] : 0u;
        uint32_t total;
        const uint32_t before = induce_group_scan_sat(v, part, &total);
        if (b < blocks) sums[b] = induce_sat_add(carry, before);
        carry = induce_sat_add(carry, total);
    }
    if (threadIdx.x == 0) res[kInduceResTotal] = carry;
}

// in place: a thread reads its four slots, then writes the same four
__global__ __launch_bounds__(kInduceThreads) void induce_offsets_kernel(int32_t* rowptr_b, int32_t M, const uint32_t* __restrict__ sums) {
    __shared__ uint32_t part[kInduceWaves];
    const int64_t first = (int64_t)blockIdx.x * kInduceScanRows + 4 * (int64_t)threadIdx.x;
    uint32_t c[4], mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) mine = induce_sat_add(mine, c[j] = induce_slot_count(rowptr_b, first + j, M));
    uint32_t total;
    uint32_t at = induce_sat_add(sums[blockIdx.x], induce_group_scan_sat(mine, part, &total));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (first + j <= M) rowptr_b[first + j] = (int32_t)at;
        at = induce_sat_add(at, c[j]);
    }
}

uint64_t induce_seed_word(uint64_t seed) {   // mix(seed + G): the per-call half of h32, computed once on the host
    uint64_t z = seed + kInduceG;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int random_walk(const int32_t* rowptr, const int32_t* col, const int32_t* starts, int32_t W, int32_t N, int64_t E, int32_t length, uint64_t seed,
                int32_t* walks, hipStream_t stream) {
    if (W > 0)
        hipLaunchKernelGGL(random_walk_kernel, dim3((unsigned)(((int64_t)W + kInduceThreads - 1) / kInduceThreads)), dim3(kInduceThreads), 0, stream,
                           rowptr, col, starts, W, N, E, length, induce_seed_word(seed), walks);
    return (int)hipGetLastError();
}

int64_t induce_scan_blocks(int32_t M) { return ((int64_t)M + 1 + kInduceScanRows - 1) / kInduceScanRows; }

inline unsigned induce_grid(int32_t M) { return (unsigned)(((int64_t)M + kInduceWaves - 1) / kInduceWaves); }

// nodePointer_b [M + 1] and the result words; sums: induce_scan_blocks(M) words of scratch.  M > 0
int induce_count(const int32_t* rowptr, const int32_t* col, const int32_t* nodes, const int32_t* new_id, int32_t M, int32_t N, int64_t E,
                 uint32_t* sums, uint32_t* res, int32_t* rowptr_b, hipStream_t stream) {
    const int64_t blocks = induce_scan_blocks(M);
    const dim3 block(kInduceThreads);
    hipLaunchKernelGGL(induce_rows_kernel<false>, dim3(induce_grid(M)), block, 0, stream, rowptr, col, nodes, new_id, M, N, E, (int64_t)0, rowptr_b,
                       (int32_t*)nullptr, (int32_t*)nullptr, res);
    hipLaunchKernelGGL(induce_sums_kernel, dim3((unsigned)blocks), block, 0, stream, rowptr_b, M, sums);
    hipLaunchKernelGGL(induce_scan_sums_kernel, dim3(1), block, 0, stream, sums, blocks, res);
    hipLaunchKernelGGL(induce_offsets_kernel, dim3((unsigned)blocks), block, 0, stream, rowptr_b, M, sums);
    return (int)hipGetLastError();
}

// M > 0, Eb > 0
int induce_write(const int32_t* rowptr, const int32_t* col, const int32_t* nodes, const int32_t* new_id, int32_t M, int32_t N, int64_t E, int64_t Eb,
                 int32_t* rowptr_b, int32_t* col_b, int32_t* eid, hipStream_t stream) {
    hipLaunchKernelGGL(induce_rows_kernel<true>, dim3(induce_grid(M)), dim3(kInduceThreads), 0, stream, rowptr, col, nodes, new_id, M, N, E, Eb,
                       rowptr_b, col_b, eid, (uint32_t*)nullptr);
    return (int)hipGetLastError();
}

} // namespace
