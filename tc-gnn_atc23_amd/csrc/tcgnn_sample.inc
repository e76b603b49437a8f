// tcgnn_sample.inc - seeded neighbour sampling: from a CSR, the CSR over the same nodes that keeps at most `fanout` in-edges per row
// (tcgnn_sample.hip holds the entry points).  Included by tcgnn_device.hip so that `make audit` lists the
// kernels with every other kernel of the library.
//
// Every CSR position e carries the 64-bit word (h32(seed, e) << 32) | e (include/tcgnn.h states h32); a row longer than the fan-out
// keeps the positions with the `fanout` smallest words, in CSR order.  The low half of a word is its position, so "the k smallest
// words" is: with T the k-th smallest h32 of the row, every position whose h32 is below T, and of those whose h32 equals T the first
// ones in position order until k are kept.  Both selects below find T over the 32 hashed bits and break ties by position - the select
// over all 64 bits, without carrying the low half.
//
// Launch geometry, stated once: kSampleThreads threads = four wavefronts per workgroup, workgroup b owns rows 4 b .. 4 b + 3.
//   1. wavefront w takes row 4 b + w when it holds at most kSampleWaveRow edges: a copy when nothing is dropped, else the hashes of
//      the row in registers (16 per lane), T by a bitwise search (32 steps of ballot + popcount sums), an ordered compaction chunk by
//      chunk (ballot prefix over lanes);
//   2. then the whole workgroup walks the (rare) longer rows among its four, one after the other: T by a radix select over 8-bit
//      digits with a 256-bin LDS histogram (bin t belongs to thread t; four passes, hashes recomputed in each), then an ordered
//      compaction over chunks of 256 positions.
// No global atomics: every output slot has one writer, fixed by the row pointers the count call wrote.  The LDS histogram's integer
// adds commute, so the result is a pure function of the inputs.  A column id is read only for an edge that is kept.
// Every index derived from the caller's row pointers is clamped to [0, E]; a row writes no more than its slot of nodePointer_s holds.
// The second half of the file is the same selection from a LIST of row ids (sample_rows_select_kernel and its count): the grid follows the
// list, not N, and the device functions below are shared.

namespace {

constexpr int kSampleThreads = 256;
constexpr int kSampleRowsPerGroup = kSampleThreads / 64;
constexpr int kSampleWaveChunks = 16;                       // hashes per lane of the one-wavefront select
constexpr int kSampleWaveRow = 64 * kSampleWaveChunks;      // longest row of the one-wavefront select
constexpr uint64_t kSampleG = 0x9E3779B97F4A7C15ull;

// h32 of the position whose pre-mixed counter is x = mix(seed + G) + (e + 1) G
__device__ __forceinline__ uint32_t sample_h32(uint64_t x) {
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((x ^ (x >> 31)) >> 32);
}

// set bits of `m` below this lane
__device__ __forceinline__ int sample_rank(uint64_t m) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// A row as the selection sees it: first position, edges, edges to keep, first output slot
struct SampleRow { int64_t lo; int32_t d, keep; int64_t out; };

__device__ __forceinline__ SampleRow sample_row(const int32_t* __restrict__ rowptr, const uint8_t* __restrict__ mask,
                                                const int32_t* __restrict__ rowptr_s, int64_t row, int64_t E, int32_t fanout) {
    int64_t lo = rowptr[row], hi = rowptr[row + 1];
    lo = lo < 0 ? 0 : (lo > E ? E : lo);
    hi = hi < 0 ? 0 : (hi > E ? E : hi);
    SampleRow r;
    r.lo = lo;
    r.d = hi > lo ? (int32_t)(hi - lo) : 0;
    r.keep = r.d < fanout ? r.d : fanout;
    if (mask && !mask[row]) r.keep = 0;
    const int64_t o = rowptr_s[row], slot = (int64_t)rowptr_s[row + 1] - o;
    r.out = o;
    if (o < 0 || slot < r.keep) r.keep = 0;   // (not what the count call wrote: write nothing rather than beyond the slot)
    return r;
}

// nothing dropped: positions lo .. lo + d of `lanes` cooperating threads
__device__ __forceinline__ void sample_copy_row(const int32_t* __restrict__ col, const SampleRow& r, int lane, int lanes,
                                                int32_t* __restrict__ col_s, int32_t* __restrict__ eid) {
    for (int64_t i = lane; i < r.d; i += lanes) {
        col_s[r.out + i] = col[r.lo + i];
        eid[r.out + i] = (int32_t)(r.lo + i);
    }
}

// keep < d <= kSampleWaveRow: one wavefront, the row's hashes in registers (slot j of lane l: position lo + 64 j + l)
__device__ __forceinline__ void sample_wave_select(const int32_t* __restrict__ col, const SampleRow& r, uint64_t S, int lane,
                                                   int32_t* __restrict__ col_s, int32_t* __restrict__ eid) {
    const int nj = (r.d + 63) >> 6;
    const uint64_t x0 = S + (uint64_t)(r.lo + lane + 1) * kSampleG;
    uint32_t h[kSampleWaveChunks];
#pragma unroll
    for (int j = 0; j < kSampleWaveChunks; ++j)   // a slot beyond the row holds the largest hash: never below a candidate
        h[j] = (j * 64 + lane < r.d) ? sample_h32(x0 + (uint64_t)(j * 64) * kSampleG) : 0xFFFFFFFFu;
    // T = the keep-th smallest hash = the largest t with fewer than `keep` hashes below it
    uint32_t T = 0;
    int less = 0;
    for (int b = 31; b >= 0; --b) {
        const uint32_t cand = T | (1u << b);
        int c = 0;
#pragma unroll
        for (int j = 0; j < kSampleWaveChunks; ++j)
            if (j < nj) c += __popcll(__ballot(h[j] < cand));
        if (c < r.keep) { T = cand; less = c; }
    }
    const int ties = r.keep - less;   // of the positions whose hash is T, the first `ties` are kept
    int64_t o = r.out;
    int eq_seen = 0;
#pragma unroll
    for (int j = 0; j < kSampleWaveChunks; ++j) {
        if (j < nj) {   // (wave-uniform)
            const int pos = j * 64 + lane;
            const bool eq = pos < r.d && h[j] == T;
            const uint64_t meq = __ballot(eq);
            const bool kept = h[j] < T || (eq && eq_seen + sample_rank(meq) < ties);
            const uint64_t mk = __ballot(kept);
            if (kept) {
                const int64_t at = o + sample_rank(mk);
                col_s[at] = col[r.lo + pos];
                eid[at] = (int32_t)(r.lo + pos);
            }
            o += __popcll(mk);
            eq_seen += __popcll(meq);
        }
    }
}

// LDS of the workgroup select: the digit histogram, per-wavefront partial sums, the chosen (prefix, rank)
struct SampleShared {
    uint32_t hist[kSampleThreads];
    uint32_t part[2][kSampleRowsPerGroup];
    uint32_t chosen[2];
};

// d > kSampleWaveRow, keep < d: the whole workgroup.  Called by every thread of the workgroup with the same row.
__device__ __forceinline__ void sample_group_select(const int32_t* __restrict__ col, const SampleRow& r, uint64_t S, SampleShared& sh,
                                                    int32_t* __restrict__ col_s, int32_t* __restrict__ eid) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t x0 = S + (uint64_t)(r.lo + tid + 1) * kSampleG;
    const uint64_t step = (uint64_t)kSampleThreads * kSampleG;
    uint32_t prefix = 0, need = (uint32_t)r.keep;   // the need-th smallest among the hashes that share `prefix`'s decided digits
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const uint32_t decided = pass ? 0xFFFFFFFFu << (shift + 8) : 0u;
        sh.hist[tid] = 0;
        __syncthreads();
        uint64_t x = x0;
        for (int64_t i = tid; i < r.d; i += kSampleThreads, x += step) {
            const uint32_t h = sample_h32(x);
            if (((h ^ prefix) & decided) == 0) atomicAdd(&sh.hist[(h >> shift) & 255u], 1u);
        }
        __syncthreads();
        // inclusive sum of the bins up to this thread's
        const uint32_t cnt = sh.hist[tid];
        uint32_t incl = cnt;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const uint32_t up = __shfl_up(incl, s);
            if (lane >= s) incl += up;
        }
        if (lane == 63) sh.part[0][wave] = incl;
        __syncthreads();
        for (int w = 0; w < wave; ++w) incl += sh.part[0][w];
        if (incl - cnt < need && need <= incl) {   // exactly one bin: the need-th hash falls into it
            sh.chosen[0] = prefix | ((uint32_t)tid << shift);
            sh.chosen[1] = need - (incl - cnt);
        }
        __syncthreads();
        prefix = sh.chosen[0];
        need = sh.chosen[1];
    }
    // prefix = T, need = how many of the positions whose hash is T are kept (the first ones)
    const uint32_t T = prefix, ties = need;
    int64_t o = r.out;
    uint32_t eq_seen = 0;
    uint64_t x = x0;
    for (int64_t c0 = 0; c0 < r.d; c0 += kSampleThreads, x += step) {
        const int64_t pos = c0 + tid;
        const bool valid = pos < r.d;
        const uint32_t h = valid ? sample_h32(x) : 0xFFFFFFFFu;
        const bool eq = valid && h == T;
        const uint64_t meq = __ballot(eq);
        if (lane == 0) sh.part[0][wave] = (uint32_t)__popcll(meq);
        __syncthreads();
        uint32_t eq_before = eq_seen + (uint32_t)sample_rank(meq), eq_all = 0;
        for (int w = 0; w < kSampleRowsPerGroup; ++w) {
            const uint32_t p = sh.part[0][w];
            if (w < wave) eq_before += p;
            eq_all += p;
        }
        const bool kept = (valid && h < T) || (eq && eq_before < ties);
        const uint64_t mk = __ballot(kept);
        if (lane == 0) sh.part[1][wave] = (uint32_t)__popcll(mk);
        __syncthreads();
        uint32_t before = (uint32_t)sample_rank(mk), all = 0;
        for (int w = 0; w < kSampleRowsPerGroup; ++w) {
            const uint32_t p = sh.part[1][w];
            if (w < wave) before += p;
            all += p;
        }
        if (kept) {
            col_s[o + before] = col[r.lo + pos];
            eid[o + before] = (int32_t)(r.lo + pos);
        }
        o += all;
        eq_seen += eq_all;
    }
    __syncthreads();   // (the next long row of this workgroup starts by clearing the histogram)
}

__global__ __launch_bounds__(kSampleThreads) void sample_select_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                       const uint8_t* __restrict__ mask, const int32_t* __restrict__ rowptr_s,
                                                                       int32_t N, int64_t E, int32_t fanout, uint64_t S,
                                                                       int32_t* __restrict__ col_s, int32_t* __restrict__ eid) {
    __shared__ SampleShared sh;
    const int lane = threadIdx.x & 63;
    const int64_t first = (int64_t)blockIdx.x * kSampleRowsPerGroup;
    const int64_t mine = first + (threadIdx.x >> 6);
    if (mine < N) {
        const SampleRow r = sample_row(rowptr, mask, rowptr_s, mine, E, fanout);
        if (r.keep > 0 && r.d <= kSampleWaveRow) {
            if (r.keep == r.d) sample_copy_row(col, r, lane, 64, col_s, eid);
            else sample_wave_select(col, r, S, lane, col_s, eid);
        }
    }
    for (int q = 0; q < kSampleRowsPerGroup; ++q) {   // the same rows for every thread: the barriers inside are uniform
        if (first + q >= N) break;
        const SampleRow r = sample_row(rowptr, mask, rowptr_s, first + q, E, fanout);
        if (r.keep == 0 || r.d <= kSampleWaveRow) continue;
        if (r.keep == r.d) sample_copy_row(col, r, (int)threadIdx.x, kSampleThreads, col_s, eid);
        else sample_group_select(col, r, S, sh, col_s, eid);
    }
}

// ---- the count call: nodePointer_s = the exclusive sum of min(d_i, fanout) * mask_i, in three launches of fixed order (no atomics, no
// library scan: the scratch is kSampleScanRows-row block sums, a size that depends on N alone):
//   sample_count_kernel    workgroup b sums the counts of rows kSampleScanRows b ... (four consecutive rows a thread) into sums[b], and
//                          writes the validation words: res[0] = nodePointer[0], res[1] = nodePointer[N], res[2] = 1 if a row pointer
//                          exceeds its successor (every thread that finds one stores the same 1)
//   sample_scan_sums_kernel  ONE workgroup turns sums[] into its exclusive sums, 256 at a step with a carry; res[3] = E'
//   sample_offsets_kernel  the counts again, scanned inside the workgroup on top of sums[b]: nodePointer_s[i], i = 0 .. N
// Degrees are taken from pointers clamped to [0, E].
constexpr int kSampleScanRows = 4 * kSampleThreads;

__device__ __forceinline__ uint32_t sample_row_count(const int32_t* __restrict__ rowptr, const uint8_t* __restrict__ mask, int64_t i, int32_t N,
                                                     int64_t E, int32_t fanout, bool& descending) {
    if (i >= N) return 0;   // (slot N: the total)
    int64_t lo = rowptr[i], hi = rowptr[i + 1];
    descending |= lo > hi;
    lo = lo < 0 ? 0 : (lo > E ? E : lo);
    hi = hi < 0 ? 0 : (hi > E ? E : hi);
    int64_t c = hi > lo ? hi - lo : 0;
    if (c > fanout) c = fanout;
    if (mask && !mask[i]) c = 0;
    return (uint32_t)c;
}

// exclusive sum of v over the workgroup's threads in thread order; *total = the sum over all of them.  part: kSampleRowsPerGroup words of LDS
__device__ __forceinline__ uint32_t sample_group_scan(uint32_t v, uint32_t* part, uint32_t* total) {
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
    for (int w = 0; w < kSampleRowsPerGroup; ++w) {
        const uint32_t p = part[w];
        if (w < wave) before += p;
        all += p;
    }
    *total = all;
    return before + incl - v;
}

__global__ __launch_bounds__(kSampleThreads) void sample_count_kernel(const int32_t* __restrict__ rowptr, const uint8_t* __restrict__ mask, int32_t N,
                                                                      int64_t E, int32_t fanout, uint32_t* __restrict__ sums, uint32_t* res) {
    __shared__ uint32_t part[kSampleRowsPerGroup];
    const int64_t first = (int64_t)blockIdx.x * kSampleScanRows + 4 * (int64_t)threadIdx.x;
    bool descending = false;
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) c += sample_row_count(rowptr, mask, first + j, N, E, fanout, descending);
    if (descending) res[2] = 1u;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        res[0] = (uint32_t)rowptr[0];
        res[1] = (uint32_t)rowptr[N];
    }
    uint32_t total;
    sample_group_scan(c, part, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kSampleThreads) void sample_scan_sums_kernel(uint32_t* __restrict__ sums, int64_t blocks, uint32_t* res) {
    __shared__ uint32_t part[kSampleRowsPerGroup];
    uint32_t carry = 0;
    for (int64_t b0 = 0; b0 < blocks; b0 += kSampleThreads) {
        const int64_t b = b0 + threadIdx.x;
        const uint32_t v = b < blocks ? sums[b] : 0u;
        uint32_t total;
        const uint32_t before = sample_group_scan(v, part, &total);
        if (b < blocks) sums[b] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) res[3] = carry;
}

__global__ __launch_bounds__(kSampleThreads) void sample_offsets_kernel(const int32_t* __restrict__ rowptr, const uint8_t* __restrict__ mask, int32_t N,
                                                                        int64_t E, int32_t fanout, const uint32_t* __restrict__ sums,
                                                                        int32_t* __restrict__ rowptr_s) {
    __shared__ uint32_t part[kSampleRowsPerGroup];
    const int64_t first = (int64_t)blockIdx.x * kSampleScanRows + 4 * (int64_t)threadIdx.x;
    bool descending = false;
    uint32_t c[4], mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) mine += c[j] = sample_row_count(rowptr, mask, first + j, N, E, fanout, descending);
    uint32_t total;
    uint32_t at = sums[blockIdx.x] + sample_group_scan(mine, part, &total);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (first + j <= N) rowptr_s[first + j] = (int32_t)at;
        at += c[j];
    }
}

// ---- seed-list sampling (tcgnn_sample_rows*): the same selection over a LIST of row ids, so that the grid follows the list and not N.
// List slot i names row rows[i] (any order, repeats allowed: every occurrence has its own slot) and owns positions
// rowptr_s[i] .. rowptr_s[i + 1] of the outputs.  Workgroup b owns slots 4 b .. 4 b + 3 exactly as sample_select_kernel owns rows;
// the device functions above are shared, only the SampleRow comes through rows[].  nodePointer is read at listed rows alone.

// SampleRow of list slot `slot`; an id outside [0, N) is an empty row
__device__ __forceinline__ SampleRow sample_list_row(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ rows,
                                                     const int32_t* __restrict__ rowptr_s, int64_t slot, int32_t N, int64_t E, int32_t fanout) {
    const int32_t row = rows[slot];
    int64_t lo = 0, hi = 0;
    if ((uint32_t)row < (uint32_t)N) {   // (a negative id is a large unsigned one)
        lo = rowptr[row];
        hi = rowptr[row + 1];
    }
    lo = lo < 0 ? 0 : (lo > E ? E : lo);
    hi = hi < 0 ? 0 : (hi > E ? E : hi);
    SampleRow r;
    r.lo = lo;
    r.d = hi > lo ? (int32_t)(hi - lo) : 0;
    r.keep = r.d < fanout ? r.d : fanout;
    const int64_t o = rowptr_s[slot], size = (int64_t)rowptr_s[slot + 1] - o;
    r.out = o;
    if (o < 0 || size < r.keep) r.keep = 0;   // (not what the count call wrote: write nothing rather than beyond the slot)
    return r;
}

__global__ __launch_bounds__(kSampleThreads) void sample_rows_select_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                            const int32_t* __restrict__ rows, const int32_t* __restrict__ rowptr_s,
                                                                            int32_t R, int32_t N, int64_t E, int32_t fanout, uint64_t S,
                                                                            int32_t* __restrict__ col_s, int32_t* __restrict__ eid) {
    __shared__ SampleShared sh;
    const int lane = threadIdx.x & 63;
    const int64_t first = (int64_t)blockIdx.x * kSampleRowsPerGroup;
    const int64_t mine = first + (threadIdx.x >> 6);
    if (mine < R) {
        const SampleRow r = sample_list_row(rowptr, rows, rowptr_s, mine, N, E, fanout);
        if (r.keep > 0 && r.d <= kSampleWaveRow) {
            if (r.keep == r.d) sample_copy_row(col, r, lane, 64, col_s, eid);
            else sample_wave_select(col, r, S, lane, col_s, eid);
        }
    }
    for (int q = 0; q < kSampleRowsPerGroup; ++q) {   // the same slots for every thread: the barriers inside are uniform
        if (first + q >= R) break;
        const SampleRow r = sample_list_row(rowptr, rows, rowptr_s, first + q, N, E, fanout);
        if (r.keep == 0 || r.d <= kSampleWaveRow) continue;
        if (r.keep == r.d) sample_copy_row(col, r, (int)threadIdx.x, kSampleThreads, col_s, eid);
        else sample_group_select(col, r, S, sh, col_s, eid);
    }
}

// ---- the rows count call: rowPointer_s[i] = the exclusive sum of min(d(rows[j]), fanout) over j < i, i = 0 .. R, in the three launches
// of sample_count over R + 1 slots (slot R: the total), with the validation of the LISTED rows in the first:
//   res[kRowsResBadId] = 1 a listed id outside [0, N);  res[kRowsResBadPtr] = 1 a listed row's pointer outside [0, E];
//   res[kRowsResDescending] = 1 a listed row's pointers descend;  res[kRowsResTotal] = E'
// Every thread that finds a fault stores the same 1.  A list may repeat long rows, so unlike the sums above these can pass 2^31 - 1:
// every add saturates at kRowsSumCap, which as an int32 row pointer is negative - sample_list_row keeps nothing behind it - and the
// entry point reports a total that reached the cap.
constexpr int kRowsResBadId = 0, kRowsResBadPtr = 1, kRowsResDescending = 2, kRowsResTotal = 3;
constexpr uint32_t kRowsSumCap = 0x80000000u;

__device__ __forceinline__ uint32_t sample_sat_add(uint32_t a, uint32_t b) {   // a, b <= kRowsSumCap
    const uint64_t s = (uint64_t)a + b;
    return s > kRowsSumCap ? kRowsSumCap : (uint32_t)s;
}

// bit 0: id out of range, bit 1: pointer out of range, bit 2: descending pair
__device__ __forceinline__ uint32_t sample_list_count(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ rows, int64_t i, int32_t R,
                                                      int32_t N, int64_t E, int32_t fanout, uint32_t& faults) {
    if (i >= R) return 0;   // (slot R: the total)
    const int32_t row = rows[i];
    if ((uint32_t)row >= (uint32_t)N) {
        faults |= 1u;
        return 0;
    }
    int64_t lo = rowptr[row], hi = rowptr[row + 1];
    if (lo < 0 || lo > E || hi < 0 || hi > E) faults |= 2u;
    if (lo > hi) faults |= 4u;
    lo = lo < 0 ? 0 : (lo > E ? E : lo);
    hi = hi < 0 ? 0 : (hi > E ? E : hi);
    int64_t c = hi > lo ? hi - lo : 0;
    if (c > fanout) c = fanout;
    return (uint32_t)c;
}

// sample_group_scan with saturating adds: exclusive sum of v over the workgroup's threads in thread order, *total over all of them
__device__ __forceinline__ uint32_t sample_group_scan_sat(uint32_t v, uint32_t* part, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t up = __shfl_up(incl, s);
        if (lane >= s) incl = sample_sat_add(incl, up);
    }
    const uint32_t below = __shfl_up(incl, 1);
    const uint32_t excl = lane ? below : 0u;
    __syncthreads();   // (part may still be read from the call before)
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int w = 0; w < kSampleRowsPerGroup; ++w) {
        const uint32_t p = part[w];
        if (w < wave) before = sample_sat_add(before, p);
        all = sample_sat_add(all, p);
    }
    *total = all;
    return sample_sat_add(before, excl);
}

__global__ __launch_bounds__(kSampleThreads) void sample_rows_count_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ rows,
                                                                           int32_t R, int32_t N, int64_t E, int32_t fanout,
                                                                           uint32_t* __restrict__ sums, uint32_t* res) {
    __shared__ uint32_t part[kSampleRowsPerGroup];
    const int64_t first = (int64_t)blockIdx.x * kSampleScanRows + 4 * (int64_t)threadIdx.x;
    uint32_t faults = 0, c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) c = sample_sat_add(c, sample_list_count(rowptr, rows, first + j, R, N, E, fanout, faults));
    if (faults & 1u) res[kRowsResBadId] = 1u;
    if (faults & 2u) res[kRowsResBadPtr] = 1u;
    if (faults & 4u) res[kRowsResDescending] = 1u;
    uint32_t total;
    sample_group_scan_sat(c, part, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kSampleThreads) void sample_rows_scan_sums_kernel(uint32_t* __restrict__ sums, int64_t blocks, uint32_t* res) {
    __shared__ uint32_t part[kSampleRowsPerGroup];
    uint32_t carry = 0;
    for (int64_t b0 = 0; b0 < blocks; b0 += kSampleThreads) {
        const int64_t b = b0 + threadIdx.x;
        const uint32_t v = b < blocks ? sums[b] : 0u;
        uint32_t total;
        const uint32_t before = sample_group_scan_sat(v, part, &total);
        if (b < blocks) sums[b] = sample_sat_add(carry, before);
        carry = sample_sat_add(carry, total);
    }
    if (threadIdx.x == 0) res[kRowsResTotal] = carry;
}

__global__ __launch_bounds__(kSampleThreads) void sample_rows_offsets_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ rows,
                                                                             int32_t R, int32_t N, int64_t E, int32_t fanout,
                                                                             const uint32_t* __restrict__ sums, int32_t* __restrict__ rowptr_s) {
    __shared__ uint32_t part[kSampleRowsPerGroup];
    const int64_t first = (int64_t)blockIdx.x * kSampleScanRows + 4 * (int64_t)threadIdx.x;
    uint32_t faults = 0;
    uint32_t c[4], mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) mine = sample_sat_add(mine, c[j] = sample_list_count(rowptr, rows, first + j, R, N, E, fanout, faults));
    uint32_t total;
    uint32_t at = sample_sat_add(sums[blockIdx.x], sample_group_scan_sat(mine, part, &total));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (first + j <= R) rowptr_s[first + j] = (int32_t)at;
        at = sample_sat_add(at, c[j]);
    }
}

} // namespace

namespace tcgnn {

int64_t sample_scan_blocks(int32_t N) { return ((int64_t)N + 1 + kSampleScanRows - 1) / kSampleScanRows; }

// nodePointer_s and the four result words (see sample_count_kernel); sums: sample_scan_blocks(N) words of scratch
int sample_count(const int32_t* rowptr, const uint8_t* mask, int32_t N, int64_t E, int32_t fanout, uint32_t* sums, uint32_t* res, int32_t* rowptr_s,
                 void* stream_v) {
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const int64_t blocks = sample_scan_blocks(N);
    hipLaunchKernelGGL(sample_count_kernel, dim3((unsigned)blocks), dim3(kSampleThreads), 0, stream, rowptr, mask, N, E, fanout, sums, res);
    hipLaunchKernelGGL(sample_scan_sums_kernel, dim3(1), dim3(kSampleThreads), 0, stream, sums, blocks, res);
    hipLaunchKernelGGL(sample_offsets_kernel, dim3((unsigned)blocks), dim3(kSampleThreads), 0, stream, rowptr, mask, N, E, fanout, sums, rowptr_s);
    return (int)hipGetLastError();
}

uint64_t sample_seed_word(uint64_t seed) {   // mix(seed + G): the per-call half of h32, computed once on the host
    uint64_t z = seed + kSampleG;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int sample_select(const int32_t* rowptr, const int32_t* col, const uint8_t* mask, const int32_t* rowptr_s, int32_t N, int64_t E, int32_t fanout,
                  uint64_t seed, int32_t* col_s, int32_t* eid, void* stream) {
    if (N > 0 && E > 0 && fanout > 0)
        hipLaunchKernelGGL(sample_select_kernel, dim3((unsigned)(((int64_t)N + kSampleRowsPerGroup - 1) / kSampleRowsPerGroup)), dim3(kSampleThreads), 0,
                           static_cast<hipStream_t>(stream), rowptr, col, mask, rowptr_s, N, E, fanout, sample_seed_word(seed), col_s, eid);
    return (int)hipGetLastError();
}

int64_t sample_rows_scan_blocks(int32_t R) { return ((int64_t)R + 1 + kSampleScanRows - 1) / kSampleScanRows; }

// rowPointer_s [R + 1] and the four result words (see sample_rows_count_kernel); sums: sample_rows_scan_blocks(R) words of scratch
int sample_rows_count(const int32_t* rowptr, const int32_t* rows, int32_t R, int32_t N, int64_t E, int32_t fanout, uint32_t* sums, uint32_t* res,
                      int32_t* rowptr_s, void* stream_v) {
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const int64_t blocks = sample_rows_scan_blocks(R);
    hipLaunchKernelGGL(sample_rows_count_kernel, dim3((unsigned)blocks), dim3(kSampleThreads), 0, stream, rowptr, rows, R, N, E, fanout, sums, res);
    hipLaunchKernelGGL(sample_rows_scan_sums_kernel, dim3(1), dim3(kSampleThreads), 0, stream, sums, blocks, res);
    hipLaunchKernelGGL(sample_rows_offsets_kernel, dim3((unsigned)blocks), dim3(kSampleThreads), 0, stream, rowptr, rows, R, N, E, fanout, sums, rowptr_s);
    return (int)hipGetLastError();
}

int sample_rows_select(const int32_t* rowptr, const int32_t* col, const int32_t* rows, const int32_t* rowptr_s, int32_t R, int32_t N, int64_t E,
                       int32_t fanout, uint64_t seed, int32_t* col_s, int32_t* eid, void* stream) {
    if (R > 0 && E > 0 && fanout > 0)
        hipLaunchKernelGGL(sample_rows_select_kernel, dim3((unsigned)(((int64_t)R + kSampleRowsPerGroup - 1) / kSampleRowsPerGroup)), dim3(kSampleThreads),
                           0, static_cast<hipStream_t>(stream), rowptr, col, rows, rowptr_s, R, N, E, fanout, sample_seed_word(seed), col_s, eid);
    return (int)hipGetLastError();
}

} // namespace tcgnn
