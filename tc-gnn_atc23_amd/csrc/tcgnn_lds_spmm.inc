// tcgnn_lds_spmm.inc - LDS-resident column-range SpMM (binary A).  Included by tcgnn_device.hip.
//
// Why: the gather-based walks (spmm_kernel, spmm_blocked_kernel) fetch one fp16 feature row per EDGE - Reddit has 1.05
// edges per condensed column (logs/reduce_blocks.csv:18: 13.57 M 16x8 blocks for 114.6 M edges) - i.e. 57 MB of
// scattered lines per CU at D = 64, and the L2 -> CU path delivers those at ~55 GB/s per CU: 1.04 ms however the
// requests are issued.  tools/lds_range_bench.hip measured the alternative on MI355X: every CU STREAMS each column range
// of the fp16 image into its LDS once (coalesced LDS-DMA, 19 TB/s aggregate when all CUs read the same range: 29.8 MB per
// CU) and the MFMA B operand is read straight out of the resident range with ds_read_b64_tr_b16 at per-lane row addresses.
//
// Shape: one workgroup per CU, 16 wavefronts, each owning up to 4 row windows for the whole launch (accumulators stay in
// registers; no partial sums, no atomics, deterministic).  Columns are cut into ranges of 504 / 632 / 760 / 1528 rows
// (4 / 3 / 2 / 1 planes of 16 feature columns); per range r every workgroup
//   (1) issues the LDS-DMA of range r+1 into the other buffer,
//   (2) multiplies the cells (window, r) of its windows out of the resident buffer,
//   (3) s_waitcnt vmcnt(0),
//   (4) requests its tile metadata of range r+2 (LDS-DMA into the pad range r has finished with) and the cell offsets of
//       r+3: they cross the barrier in flight and have all of range r+1 to arrive from HBM,
//   (5) s_barrier.
// A cell's tiles are re-condensed per range (plan->lds[slot].d_cell_tiles): 32 K slots = 32 distinct columns of the window
// inside the range, as 16-bit row numbers local to the range, each placed in a slot whose bank group matches its row number
// (conflict-free transposed reads); unused slots point at one of the eight all-zero rows kept behind every buffer.
// Worth it when a loaded row is used more than once per workgroup: 64 windows x 16 rows x density >= 1.5 (Reddit: 2.2;
// ogbn-products: 0.02 -> gather walks).  DESIGN.md 4.2c has the measurements and what was tried and dropped.

static constexpr int kLdsWaves = 16;      // wavefronts per workgroup (one workgroup per CU)
static constexpr int kLdsMaxW = 4;        // windows owned by a wavefront, 64 feature columns per pass (accumulators: 64 VGPRs) ...
static constexpr int kLdsMaxW2 = 8;       // ... or twice the windows at 32 columns per pass: half as many workgroups stream each plane
// Rows of one LDS range buffer (the range + eight all-zero rows, one per bank group).  Every range costs a fixed ~1500 cycles
// (metadata latency, barrier) on top of its bytes, so narrow passes get longer ranges: 1 / 2 planes of 16 columns stream
// 1528 / 760-row ranges (48 KB buffers), 3 planes 632-row ranges (60 KB), 4 planes 504-row ranges (64 KB); the long flat walk streams
// two planes of 952 rows (60 KB buffers, slot 7).  The cell stream depends on the range length:
// a plan carries one stream per length in use (kLdsStreams slots).
// Two layouts: 4 windows per wavefront with up to 4 planes per pass, or 8 windows with 2 planes per pass (half as many
// workgroups stream each plane, 760-row ranges; measured better whenever the width is a multiple of 32 columns >= 64:
// Reddit D = 64 0.69 vs 0.77 ms, D = 128 1.36 vs 1.50 ms).  Stream slots: 0-3 = 4 windows x {4, 2, 1, 3} planes,
// 4-5 = 8 windows x {2, 1} planes, 7 = slot 4's layout with 952-row ranges (960-row buffers: the LONG flat walk, spmm_lds_flat_long_kernel,
// which pays for them with a shared pool of four cold tiles instead of one per wavefront).  A plan builds slot 4 OR slot 7, whichever
// build_lds_cells prices lower: graphs whose 760-row cells are under-filled (communities) take the long ranges - a fifth fewer entries.
static constexpr int kLdsStreams = 8;
static constexpr int kLdsValSlot = 6;     // 8 windows x 2 planes like slot 4, cut from the SINGLE-EDGE tile stream (tcgnn_lds_val.inc)
static constexpr int kLdsLongSlot = 7;    // 8 windows x 2 planes, 960-row buffers
__host__ __device__ constexpr int lds_stream_of(int nt, int maxw, bool long_ranges = false) { return maxw == 8 ? (nt == 2 ? (long_ranges ? 7 : 4) : 5) : (nt >= 4 ? 0 : (nt == 2 ? 1 : (nt == 1 ? 2 : 3))); }
__host__ __device__ constexpr int lds_stream_buf_rows(int slot) { return slot == 7 ? 960 : (slot == 0 ? 512 : (slot == 1 ? 768 : (slot == 2 ? 1536 : (slot == 3 ? 640 : (slot == 4 || slot == 6 ? 768 : 512))))); }
__host__ __device__ constexpr int lds_stream_maxw(int slot) { return slot >= 4 ? 8 : 4; }
__host__ __device__ constexpr int lds_stream_nt(int slot) { return slot == 0 ? 4 : (slot == 1 ? 2 : (slot == 2 ? 1 : (slot == 3 ? 3 : (slot == 4 || slot == 6 || slot == 7 ? 2 : 1)))); }
__host__ __device__ constexpr int lds_buf_rows(int nt, int maxw, bool long_ranges = false) { return lds_stream_buf_rows(lds_stream_of(nt, maxw, long_ranges)); }
static constexpr int lds_pad_tiles(int maxw, int buf_rows) { return maxw != 4 ? (buf_rows == 768 ? 12 : 16) : (buf_rows == 512 ? 6 : (buf_rows == 1536 ? 12 : 8)); }   // tiles of metadata prefetched per wavefront and range (8 per DMA instruction)
static constexpr int kCellWords = 32;     // one tile: 16 words holding 32 u16 row ids, then 16 mask words
static constexpr int lds_chunk_dims(int maxw) { return 256 / maxw; }     // feature columns per pass

// The range guard's fallback of the binary SpMM inside the LDS-resident kernels' own launch: a separate launch is a gate that almost
// always returns at once and still costs 4.5 us of every aggregation.  Every wavefront of the grid takes windows (fb.guard == nullptr:
// the host launches the fallback behind this kernel - fused dense update, several passes, an external cold remainder).
__device__ __forceinline__ void lds_own_fallback(const SpmmSmallArgs& fb) {
    if (!fb.guard) return;
    const int wave = (int)(threadIdx.x >> 6), wpb = (int)(blockDim.x >> 6);
    const int lin = (int)blockIdx.x + (int)gridDim.x * (int)blockIdx.y;
    const int total = (int)(gridDim.x * gridDim.y) * wpb;
    for (int coloff = 0; coloff < fb.D; coloff += 64) spmm_small_windows(fb, lin * wpb + wave, total, coloff, (int)(threadIdx.x & 63));
}

struct SpmmLdsArgs {
    const uint32_t* cell_ptr;   // [(nwg * nranges * 16 + wave) * 4 + j] tile offset of cell (wg, range, wave, j); +1 entry
    const uint32_t* tiles;      // [tiles][kCellWords]
    const int32_t* order;       // the stream's window slots: order[cell_position(wg, wave, j)] = window id or -1
    const _Float16* x16;
    const uint32_t* hdr;
    float* y;
    int32_t N, D, stride /* planes of the planar image */, chunk0, xrows, nranges, nw, nwg;
    int32_t dbg, relu;   // relu: fused epilogue Y = max(A X, 0).  dbg: measurement only (TCGNN_LDS_DBG): 1 no range fill, 2 no multiply, 4 no metadata DMA, 8 no barrier, 16 report phase cycles
    const int32_t* rbase;   // [nwg + 1] first hot (workgroup, range) pair of every workgroup in the compact cell table
    const int32_t* rlist;   // [pairs] column range of every hot pair: the ranges a workgroup streams, in order
    const float* w;      // f3: Y[N, dout] = (A X) W, W [D, dout] fp32 row-major (nullptr: Y = A X)
    int32_t dout, accumulate;   // accumulate: this pass covers only some input columns - its product is ADDED into a zeroed Y
    const uint32_t* parts;      // [slots] split hub windows (lds_split_parts): part | parts << 8 | LDS scratch index << 16; nullptr: none
    SpmmSmallArgs fb;           // fb.guard != nullptr: this launch is its own range-guard fallback (lds_own_fallback)
    Epi epi;                    // tcgnn_spmm_scaled: row scale / bias in the final store (null when a cold remainder follows: its kernel applies them)
};

// Window slot p = (workgroup, wavefront, window slot j) of a cell stream's own order array (CellStream::d_order: window id or -1;
// filled on the host by lds_place_windows).  Workgroups own CONTIGUOUS blocks of windows of about equal weight: windows next to
// each other tend to share their neighbourhoods (communities, R-MAT blocks), so the column ranges in which a workgroup's
// wavefronts have work coincide - every range ends at the barrier of its slowest wavefront - and whole (workgroup, range) pairs
// that hold too few columns can leave the LDS-resident walk altogether (the "cold" remainder, see build_lds_cells).  Inside a
// workgroup the windows are dealt heaviest-first to the least loaded wavefront with a free slot.
__host__ __device__ inline void cell_place(int p, int maxw, int& wg, int& wave, int& j) {
    j = p % maxw;
    wave = (p / maxw) % kLdsWaves;
    wg = p / (maxw * kLdsWaves);
}
__host__ __device__ inline int cell_position(int wg, int wave, int j, int maxw) { return (wg * kLdsWaves + wave) * maxw + j; }

__device__ __forceinline__ int64_t cell_lower_bound(const int32_t* base, int64_t n, int32_t x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (base[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// tiles window w costs a stream with `rows`-row ranges: sum over the ranges of ceil(columns in the range / 32).  The exact weight
// the placement balances (a model by column count alone misjudges graphs whose columns crowd into few ranges).
__global__ __launch_bounds__(256) void window_tiles_kernel(const int64_t* __restrict__ wb_ptr, const int32_t* __restrict__ cols, int32_t nw, int32_t nranges,
                                                           int32_t Nc, int32_t rows, uint32_t* __restrict__ tiles_of) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)nw * nranges) return;
    const int w = (int)(idx / nranges), r = (int)(idx % nranges);
    const int32_t* base = cols + wb_ptr[w] * kWbCols;
    const int64_t n = (wb_ptr[w + 1] - wb_ptr[w]) * kWbCols;
    const int64_t x0 = (int64_t)r * rows, x1 = x0 + rows;
    const int64_t lo = cell_lower_bound(base, n, (int32_t)(x0 < Nc ? x0 : Nc));
    const int64_t hi = cell_lower_bound(base, n, (int32_t)(x1 < Nc ? x1 : Nc));
    if (hi > lo) atomicAdd(&tiles_of[w], (uint32_t)((hi - lo + 31) / 32));
}

// condensed columns of every cell (window slot p, range r) and the condensed index of the cell's first column
__global__ __launch_bounds__(256) void cell_count_kernel(const int64_t* __restrict__ wb_ptr, const int32_t* __restrict__ order,
                                                         const int32_t* __restrict__ cols, int32_t nw, int32_t nwg, int32_t nranges,
                                                         int32_t Nc, int32_t maxw, int32_t rows, uint32_t* __restrict__ cnt, uint32_t* __restrict__ firstq,
                                                         const uint32_t* __restrict__ parts) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)nw * nranges) return;   // nw: window SLOTS of the stream (workgroups x wavefronts x slots)
    const int p = (int)(idx / nranges), r = (int)(idx % nranges);
    const int w = order[p];
    if (w < 0) { firstq[idx] = 0u; return; }    // (cnt stays 0: the table is zeroed)
    const int32_t* base = cols + wb_ptr[w] * kWbCols;
    const int64_t n = (wb_ptr[w + 1] - wb_ptr[w]) * kWbCols;
    const int64_t x0 = (int64_t)r * rows, x1 = x0 + rows;
    int64_t lo = cell_lower_bound(base, n, (int32_t)(x0 < Nc ? x0 : Nc));
    int64_t hi = cell_lower_bound(base, n, (int32_t)(x1 < Nc ? x1 : Nc));
    if (parts) {   // a split window: part q of k takes the q-th run of the cell's tiles (whole tiles, so no part pads more than the window would)
        const uint32_t pi = parts[p], k = (pi >> 8) & 0xffu;
        if (k > 1u) {
            const int64_t q = pi & 0xffu, nt = (hi - lo + 31) / 32;
            const int64_t a = lo + 32 * (nt * q / k), b = lo + 32 * (nt * (q + 1) / k);
            lo = a < hi ? a : hi;
            hi = b < hi ? b : hi;
        }
    }
    int wg, wave, j;
    cell_place(p, maxw, wg, wave, j);
    cnt[(((int64_t)wg * nranges + r) * kLdsWaves + wave) * maxw + j] = (uint32_t)(hi - lo);
    firstq[idx] = (uint32_t)lo;
}

// columns of every (workgroup, range) pair: what decides whether the pair is worth a 48 KB range fill (hot) or its columns go
// to the gather walk (cold)
// (pairmax: tiles of the pair's busiest wavefront - what the range lasts, every range ends at a barrier; feeds the plan-time estimate
// that chooses between placements)
// (pairover: [2][npairs] columns beyond 32 / 64 per cell - what a flat stream with one / two tiles per cell would leave to the cold
//  remainder; pairtiles: the pair's tiles in the ordinary stream)
__global__ __launch_bounds__(256) void cell_pair_cols_kernel(const uint32_t* __restrict__ cellcols, int64_t npairs, int32_t per_wg, int32_t maxw,
                                                             uint32_t* __restrict__ paircols, uint32_t* __restrict__ pairmax,
                                                             uint32_t* __restrict__ pairover, uint32_t* __restrict__ pairtiles) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= npairs) return;
    uint32_t s = 0, mx = 0, o1 = 0, o2 = 0, tt = 0;
    for (int v = 0; v < per_wg / maxw; ++v) {
        uint32_t t = 0;
        for (int j = 0; j < maxw; ++j) {
            const uint32_t c = cellcols[k * per_wg + v * maxw + j];
            s += c; t += (c + 31u) / 32u;
            o1 += c > 32u ? c - 32u : 0u; o2 += c > 64u ? c - 64u : 0u;
        }
        mx = t > mx ? t : mx;
        tt += t;
    }
    paircols[k] = s;
    pairmax[k] = mx;
    if (pairover) { pairover[k] = o1; pairover[npairs + k] = o2; }
    if (pairtiles) pairtiles[k] = tt;
}
// tiles of the cells of the hot pairs, in execution order: kmap[(wg, r)] = index of the pair in the compact cell table, or -1
__global__ __launch_bounds__(256) void cell_compact_kernel(const uint32_t* __restrict__ cellcols, const int32_t* __restrict__ kmap, int64_t npairs, int32_t per_wg,
                                                           uint32_t* __restrict__ cnt) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npairs * per_wg) return;
    const int64_t pair = idx / per_wg;
    const int k = kmap[pair];
    if (k >= 0) cnt[(int64_t)k * per_wg + (idx - pair * per_wg)] = (cellcols[idx] + 31u) / 32u;
}
// what cells_dense_pairs asks of every hot pair, from the compact tile counts: the extra tiles (beyond each cell's first) of its busiest
// wavefront and the tiles of its fullest cell - so that the 4-bytes-per-cell table itself goes to the host only for the stream that is built
__global__ __launch_bounds__(256) void cell_dense_stats_kernel(const uint32_t* __restrict__ cnt, int64_t npairs, int32_t maxw, uint32_t* __restrict__ extra_mx, uint32_t* __restrict__ cell_mx) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= npairs) return;
    uint32_t mx = 0, cmx = 0;
    for (int v = 0; v < kLdsWaves; ++v) {
        uint32_t ex = 0;
        for (int j = 0; j < maxw; ++j) { const uint32_t c = cnt[(k * kLdsWaves + v) * maxw + j]; ex += c > 1u ? c - 1u : 0u; cmx = c > cmx ? c : cmx; }
        mx = ex > mx ? ex : mx;
    }
    extra_mx[k] = mx; cell_mx[k] = cmx;
}
// cold remainder: condensed columns of window slot p that fall into cold pairs -> coldcols[window]
// (cap: columns a hot cell keeps - a flat stream's cells hold cap = 32 x tiles-per-cell, what lies beyond is cold too; 0: no cap)
// (ent: entry table of a flat stream with dense entries, or nullptr - ent[2 k] = normal entry of hot pair k, ent[2 k + 1] = its first
//  dense entry, -1: none; a DENSE pair keeps what its cells hold beyond the cap in its dense entries: not cold)
__device__ __forceinline__ bool pair_is_dense(const int32_t* ent, int32_t k) { return ent && ent[2 * k + 1] >= 0; }
__global__ __launch_bounds__(256) void cell_cold_count_kernel(const uint32_t* __restrict__ cellcols, const int32_t* __restrict__ kmap, const int32_t* __restrict__ order,
                                                              int32_t nslots, int32_t nranges, int32_t maxw, uint32_t* __restrict__ coldcols, uint32_t cap,
                                                              const int32_t* __restrict__ ent = nullptr) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nslots) return;
    const int w = order[p];
    if (w < 0) return;
    int wg, wave, j;
    cell_place(p, maxw, wg, wave, j);
    uint32_t s = 0;
    for (int r = 0; r < nranges; ++r) {
        const uint32_t c = cellcols[(((int64_t)wg * nranges + r) * kLdsWaves + wave) * maxw + j];
        const int32_t kp = kmap[(int64_t)wg * nranges + r];
        if (kp < 0) s += c;
        else if (cap && c > cap && !pair_is_dense(ent, kp)) s += c - cap;
    }
    if (s) atomicAdd(&coldcols[w], s);   // (the parts of a split window each hold a share of its columns; the table starts zeroed)
}
// One workgroup per window slot: the window's cold columns, in order, re-condensed into 16 x 32 tiles of the gather walks' packed
// format (cols / mask; binary SpMM needs no edge offsets).  A block scan ranks the cold columns of each 256-column chunk.
__global__ __launch_bounds__(256) void cell_cold_fill_kernel(const int64_t* __restrict__ wb_ptr, const int32_t* __restrict__ order, const int32_t* __restrict__ cols,
                                                             const uint32_t* __restrict__ mask, const int32_t* __restrict__ kmap, int32_t nranges, int32_t Nc,
                                                             int32_t maxw, int32_t rows, const int64_t* __restrict__ cold_ptr, int32_t* __restrict__ ccols,
                                                             uint32_t* __restrict__ cmask, const uint32_t* __restrict__ parts,
                                                             const uint32_t* __restrict__ firstq, uint32_t cap,
                                                             const int32_t* __restrict__ eidx_src = nullptr, int32_t* __restrict__ ceidx = nullptr,
                                                             const int32_t* __restrict__ ent = nullptr) {
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t base_s;
    const int p = blockIdx.x;
    const int w = order[p];
    if (w < 0) return;
    if (parts && ((parts[p] >> 8) & 0xffu) > 1u && (parts[p] & 0xffu) != 0u) return;   // a split window: part 0 (same workgroup, same cold ranges) emits the whole window's cold columns
    int wg, wave, j;
    cell_place(p, maxw, wg, wave, j);
    const int64_t tb = wb_ptr[w];
    const int64_t n = (wb_ptr[w + 1] - tb) * kWbCols;
    const int64_t cb = cold_ptr[w];
    if (cold_ptr[w + 1] == cb) return;
    if (threadIdx.x == 0) base_s = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int64_t q0 = 0; q0 < n; q0 += blockDim.x) {
        const int64_t q = q0 + threadIdx.x;
        int32_t c = Nc;
        if (q < n) c = cols[tb * kWbCols + q];
        // cold: the column's (workgroup, range) pair is, or (flat streams) it lies beyond the cap of its hot cell
        const int32_t kpc = c < Nc ? kmap[(int64_t)wg * nranges + c / rows] : 0;
        const bool cold = c < Nc && (kpc < 0 || (cap && (uint32_t)q - firstq[(int64_t)p * nranges + c / rows] >= cap && !pair_is_dense(ent, kpc)));
        const uint64_t bal = __ballot(cold);
        const uint32_t before = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wv] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t off = base_s;
        for (int k = 0; k < wv; ++k) off += wsum[k];
        if (cold) {
            const uint32_t pos = off + before;                       // rank among the window's cold columns
            const int64_t t = cb + (pos >> 5);
            const uint32_t k = pos & 31u;
            ccols[t * kWbCols + k] = c;
            if (ceidx) ceidx[t * 32 + k] = eidx_src[tb * kWbCols + q];
            const uint32_t* m = mask + (tb + (q >> 5)) * kWinRows;
            const uint32_t b = (uint32_t)(q & 31);
#pragma unroll
            for (int rr = 0; rr < kWinRows; ++rr)
                if ((m[rr] >> b) & 1u) atomicOr(&cmask[t * kWinRows + rr], 1u << k);
        }
        __syncthreads();
        if (threadIdx.x == 0) base_s += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
}

// K slot <-> (pass group q, home h): a 32-lane pass of ds_read_b64_tr_b16 reads the rows of K slots {0-3, 8-11},
// {4-7, 12-15}, {16-19, 24-27} or {20-23, 28-31}; it is conflict-free when the eight rows differ in the low 3 bits
// (their 32-byte pieces then fall into the eight bank groups).  Slot (q, h) is the HOME of a row with number % 8 == h.
__host__ __device__ constexpr int cell_slot(int q, int h) { return ((q >> 1) * 2 + (h >> 2)) * 8 + (q & 1) * 4 + (h & 3); }
__host__ __device__ constexpr int cell_home(int k) { return ((k >> 3) & 1) * 4 + (k & 3); }
__global__ __launch_bounds__(256) void cell_init_kernel(uint32_t* __restrict__ tiles, int64_t nwords, int32_t rows) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nwords) return;
    const int w = (int)(k & 31);
    tiles[k] = w >= 16 ? 0u : ((uint32_t)(rows + cell_home(2 * w)) | ((uint32_t)(rows + cell_home(2 * w + 1)) << 16));
}

// one workgroup per window position p: every condensed column of the window goes to its cell's tile
__global__ __launch_bounds__(256) void cell_fill_kernel(const int64_t* __restrict__ wb_ptr, const int32_t* __restrict__ order,
                                                        const int32_t* __restrict__ cols, const uint32_t* __restrict__ mask, int32_t nwg,
                                                        int32_t nranges, int32_t Nc, int32_t maxw, int32_t rows, const uint32_t* __restrict__ cell_ptr,
                                                        const uint32_t* __restrict__ firstq, uint32_t* __restrict__ tiles, const int32_t* __restrict__ kmap,
                                                        const uint32_t* __restrict__ parts, const uint32_t* __restrict__ cellcols, int32_t tpc,
                                                        const int32_t* __restrict__ eidx_src = nullptr, int32_t* __restrict__ eidx_out = nullptr,
                                                        const int32_t* __restrict__ ent = nullptr, const uint32_t* __restrict__ xbase = nullptr) {
    const int p = blockIdx.x;
    const int w = order[p];
    if (w < 0) return;
    const bool split = parts && ((parts[p] >> 8) & 0xffu) > 1u;
    const int64_t tb = wb_ptr[w];
    const int64_t n = (wb_ptr[w + 1] - tb) * kWbCols;
    int wg, wave, j;
    cell_place(p, maxw, wg, wave, j);
    for (int64_t q = threadIdx.x; q < n; q += blockDim.x) {
        const int32_t c = cols[tb * kWbCols + q];
        if (c >= Nc) continue;   // padding of the window's last wide block
        const int r = c / rows;
        const int kp = kmap[(int64_t)wg * nranges + r];
        if (kp < 0) continue;    // a cold (workgroup, range) pair: the column belongs to the gather walk's remainder
        const uint32_t first = firstq[(int64_t)p * nranges + r];
        if (split && ((uint32_t)q < first || (uint32_t)q >= first + cellcols[(((int64_t)wg * nranges + r) * kLdsWaves + wave) * maxw + j])) continue;   // another part's run
        const uint32_t pos = (uint32_t)q - first;
        const int64_t cell = ((int64_t)kp * kLdsWaves + wave) * maxw + j;
        int64_t t;
        if (!tpc) t = (int64_t)cell_ptr[cell] + (pos >> 5);
        else {   // flat stream: tile positions are computed, no cell table.  Pair kp's normal entry is entry e (ent, or kp itself)
            const int64_t e = ent ? ent[2 * kp] : kp;
            if (pos < 32u * (uint32_t)tpc) t = (((int64_t)e * kLdsWaves + wave) * maxw + j) * tpc + (pos >> 5);
            else if (pair_is_dense(ent, kp)) {   // beyond the cell's tile, dense pair: extra tile P of this wavefront's list -> dense entry P / maxw, tile P % maxw
                const int64_t P = (int64_t)xbase[cell] + (pos >> 5) - 1;
                t = ((int64_t)(ent[2 * kp + 1] + P / maxw) * kLdsWaves + wave) * maxw + P % maxw;
            } else continue;                     // -> the cold remainder
        }
        const uint32_t k = pos & 31u;
        reinterpret_cast<uint16_t*>(tiles + t * kCellWords)[k] = (uint16_t)(c - r * rows);
        if (eidx_out) eidx_out[t * 32 + k] = eidx_src[tb * kWbCols + q];   // (single-edge source stream: the slot's edge travels with it)
        const uint32_t* m = mask + (tb + (q >> 5)) * kWinRows;
        const uint32_t b = (uint32_t)(q & 31);
#pragma unroll
        for (int rr = 0; rr < kWinRows; ++rr)
            if ((m[rr] >> b) & 1u) atomicOr(&tiles[t * kCellWords + 16 + rr], 1u << k);
    }
}

// One thread per tile: move every row id to a home slot of its bank group where one is free (greedy over the four
// pass groups), leftovers to any free slot; permute the mask bits with it and store mask BYTES as A-table positions.
__global__ __launch_bounds__(256) void cell_optimize_kernel(uint32_t* __restrict__ tiles, int64_t ntiles, int32_t rows, int32_t* __restrict__ eidx = nullptr) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntiles) return;
    uint32_t* tile = tiles + t * kCellWords;
    uint32_t idw[16], mk[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) { idw[k] = tile[k]; mk[k] = tile[16 + k]; }
    uint32_t taken = 0u, placed = 0u;        // new slots in use; old slots already placed
    uint8_t dst[32];
    for (int k = 0; k < 32; ++k) {
        const uint32_t id = (idw[k >> 1] >> (16 * (k & 1))) & 0xffffu;
        dst[k] = 255;
        if (id >= (uint32_t)rows) { placed |= 1u << k; continue; }   // empty slot
        for (int q = 0; q < 4; ++q) {
            const int ns = cell_slot(q, (int)(id & 7u));
            if (!((taken >> ns) & 1u)) { taken |= 1u << ns; dst[k] = (uint8_t)ns; placed |= 1u << k; break; }
        }
    }
    for (int k = 0; k < 32; ++k) {
        if ((placed >> k) & 1u) continue;
        const int ns = __ffs((int)~taken) - 1;   // a real id never outnumbers the free slots
        taken |= 1u << ns;
        dst[k] = (uint8_t)ns;
    }
    uint16_t nid[32];
    for (int ns = 0; ns < 32; ++ns) nid[ns] = (uint16_t)(rows + cell_home(ns));
    uint32_t nm[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) nm[r] = 0u;
    for (int k = 0; k < 32; ++k) {
        if (dst[k] == 255) continue;
        nid[dst[k]] = (uint16_t)((idw[k >> 1] >> (16 * (k & 1))) & 0xffffu);
#pragma unroll
        for (int r = 0; r < 16; ++r) nm[r] |= ((mk[r] >> k) & 1u) << dst[k];
    }
    // final layout: word 4g + c = byte offsets (32 x row) of K rows 8g + c (low half) and 8g + 4 + c (high half) - the pair a
    // lane with i >> 2 == c points its two transposed reads at; word 16 + r = adjacency bits of window row r (lane (g, r)
    // reads byte g)
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int g = k >> 2, c = k & 3;
        tile[k] = ((uint32_t)nid[8 * g + c] << 5) | ((uint32_t)nid[8 * g + 4 + c] << 21);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) tile[16 + r] = nm[r];
    if (eidx) {   // the edges move with their slots
        int32_t* ei = eidx + t * 32;
        int32_t old[32], neu[32];
        for (int k = 0; k < 32; ++k) { old[k] = ei[k]; neu[k] = -1; }
        for (int k = 0; k < 32; ++k) if (dst[k] != 255) neu[dst[k]] = old[k];
        for (int k = 0; k < 32; ++k) ei[k] = neu[k];
    }
}

// A fragment of a tile from this lane's adjacency byte (bit k = edge to K row 8g + k): register j holds K rows 2j, 2j+1 as
// fp16 2.0 or 0 (0x4000: one bit per half, so two packed 16-bit shifts and a mask make a register; the factor 2 comes
// out with the power-of-two scale at the end).  Nine VALU instructions instead of a 1 KB table read: the LDS pipeline is
// what this kernel queues on.
// (s_setprio takes an immediate: the switch folds once the caller's loop is unrolled)
__device__ __forceinline__ void set_wave_priority(int p) {
    switch (p) {
        case 0: __builtin_amdgcn_s_setprio(0); break;
        case 1: __builtin_amdgcn_s_setprio(1); break;
        case 2: __builtin_amdgcn_s_setprio(2); break;
        default: __builtin_amdgcn_s_setprio(3); break;
    }
}
typedef unsigned short ushort2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ half8 afrag_from_byte(uint32_t mb) {
    const uint32_t mm = mb | (mb << 16);
    uintx4 q;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const ushort2v k = {(unsigned short)(1u << (14 - 2 * j)), (unsigned short)(1u << (13 - 2 * j))};
        q[j] = __builtin_bit_cast(uint32_t, (ushort2v)(__builtin_bit_cast(ushort2v, mm) * k)) & 0x40004000u;
    }
    return __builtin_bit_cast(half8, q);
}

template <int NT, int PLANE> __device__ __forceinline__ void lds_cell_block(uint32_t ad0, uint32_t ad1, uint32_t idaddr, uint32_t maddr,
                                                                            half4* lo, half4* hi, uint32_t& idw, uint32_t& m) {
    if constexpr (NT == 1) lds_cell_block1<PLANE>(ad0, ad1, idaddr, maddr, lo, hi, idw, m);
    else if constexpr (NT == 2) lds_cell_block2<PLANE>(ad0, ad1, idaddr, maddr, lo, hi, idw, m);
    else if constexpr (NT == 3) lds_cell_block3<PLANE>(ad0, ad1, idaddr, maddr, lo, hi, idw, m);
    else lds_cell_block4<PLANE>(ad0, ad1, idaddr, maddr, lo, hi, idw, m);
}

// LDS-DMA of one column range: NT planes x (BR / 32) instructions of 1 KB (rows 32b .. 32b+31 of a plane; lane l: row l/2,
// half l%2: 1 KB of consecutive source bytes -> 1 KB of consecutive LDS), dealt round-robin to the 16 wavefronts (wavefront
// w issues instructions w, w + 16, w + 32 ...; four dedicated loaders measured slower: 0.58 vs 0.49 ms of fill alone).
// The planar image is a structured buffer of 32-byte records; rows past the matrix and the eight zero rows of the buffer
// read the all-zero sentinel row.
template <int NT, int BR>
struct RangeFiller {
    static constexpr int IPP = BR / 32;                                   // instructions per plane
    static constexpr int TOTAL = NT * IPP;
    static constexpr int MAXC = (TOTAL + kLdsWaves - 1) / kLdsWaves;      // most instructions any wavefront issues
    __amdgpu_buffer_rsrc_t xrsrc;
    uint32_t frow[MAXC];   // this lane's row of the range buffer per instruction (0x40000000: one of the zero rows)
    int pbase[MAXC];       // record index of row 0 of the instruction's plane
    uint32_t dst[MAXC];    // LDS offset of the instruction's kilobyte inside a buffer
    uint32_t zrow;         // the sentinel row of the image
    int hoff, count;
    __device__ __forceinline__ RangeFiller(const _Float16* x16p, int xrows, int plane0, int nplanes, int wave, int lane) {
        xrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)x16p, (short)32, nplanes * xrows, 0x00020000);
        zrow = (uint32_t)(xrows - 1);
        hoff = (lane & 1) * 16;
        count = 0;
#pragma unroll
        for (int q = 0; q < MAXC; ++q) {
            const int k = wave + kLdsWaves * q;
            const int plane = k < TOTAL ? k / IPP : 0, blk = k % IPP;
            const int row = blk * 32 + (lane >> 1);
            const bool real_plane = plane0 + plane < nplanes;   // (a pass whose last plane lies beyond the matrix: all zeros)
            frow[q] = (row < BR - 8 && real_plane) ? (uint32_t)row : 0x40000000u;
            pbase[q] = real_plane ? (plane0 + plane) * xrows : 0;
            dst[q] = (uint32_t)plane * (BR * 32u) + (uint32_t)blk * 1024u;
            if (k < TOTAL) ++count;
        }
    }
    __device__ __forceinline__ void fill(int r0, uint32_t buf) const {
#pragma unroll
        for (int q = 0; q < MAXC; ++q) {
            if (q < count) {
                const uint32_t want = (uint32_t)r0 + frow[q];
                const int srow = (int)(want < zrow ? want : zrow);
                __builtin_amdgcn_struct_ptr_buffer_load_lds(xrsrc, (LDS_AS void*)(uintptr_t)(buf + dst[q]), 16, pbase[q] + srow, hoff, 0, 0, 0);
            }
        }
    }
};

// NT = 16-column slices (planes) of this pass (1 .. 16 / MAXW), MAXW = windows per wavefront (4 or 8).
// DBG: the timing switches of SpmmLdsArgs::dbg are compiled in (TCGNN_LDS_DBG set; never in the product path - their
// scalar tests sit in the tile loop, which is bound by instruction issue)
template <int NT, int MAXW, bool DBG>
__global__ __launch_bounds__(kLdsWaves * 64) void spmm_lds_kernel(const SpmmLdsArgs a) {
    if (range_is_wide(a.hdr, 0)) { lds_own_fallback(a.fb); return; }   // (range guard: the fp32 walk does the work - here, or in a launch behind this one)
    const int dbg = DBG ? a.dbg : 0;
    constexpr int kLdsBufRows = lds_buf_rows(NT, MAXW), kLdsRows = kLdsBufRows - 8;
    constexpr int kLdsPadTiles = lds_pad_tiles(MAXW, kLdsBufRows), kLdsPadB = kLdsPadTiles * 128, kLdsChunkDims = lds_chunk_dims(MAXW);
    static_assert(NT * MAXW <= 16, "accumulators: NT * MAXW * 4 VGPRs");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int PLANEB = kLdsBufRows * 32;                // one plane of a range buffer
    constexpr int BUFB = NT * PLANEB;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, i = lane & 15;
    const int wg = blockIdx.x;
    const int chunk_id = a.chunk0 + (int)blockIdx.y;
    const int coloff = chunk_id * kLdsChunkDims;   // first feature column of this pass
    const uint32_t lds0 = (uint32_t)(uintptr_t)((LDS_AS char*)smem);
    const uint32_t pad0 = lds0 + 2 * BUFB + (uint32_t)wave * (2 * kLdsPadB);
    const int kx = scale_exp_from_bits(a.hdr[kHdrMaxX]);

    int wj[MAXW];
    uint32_t pj[MAXW];   // split hub windows: part | parts << 8 | scratch index << 16 (0: a whole window)
    floatx4 acc[MAXW][NT];
#pragma unroll
    for (int j = 0; j < MAXW; ++j) {
        wj[j] = __builtin_amdgcn_readfirstlane(a.order[cell_position(wg, wave, j, MAXW)]);   // (-1: an empty slot)
        pj[j] = a.parts ? (uint32_t)__builtin_amdgcn_readfirstlane((int)a.parts[cell_position(wg, wave, j, MAXW)]) : 0u;
#pragma unroll
        for (int s = 0; s < NT; ++s) acc[j][s] = floatx4{0.f, 0.f, 0.f, 0.f};
    }

    // ---- per-lane constants
    // lane (g, i) receives K = 8g + 4h + {0..3} of column 16s + i when it points the transpose read at row
    // 8g + 4h + (i >> 2) of plane s, halves 4(i & 3) .. +3 of the 32-byte record
    const uint32_t lanebase = lds0 + (uint32_t)(i & 3) * 8u;
    const uint32_t idoff = (uint32_t)(4 * g + (i >> 2)) * 4u;   // this lane's pair of K rows: one word of byte offsets (K row 8g + (i >> 2) | that + 4)
    const uint32_t moff = 64u + (uint32_t)i * 4u + (uint32_t)g; // adjacency byte of window row i, K rows 8g .. 8g + 7
    const RangeFiller<NT, kLdsBufRows> filler(a.x16, a.xrows, chunk_id * (kLdsChunkDims / 16), a.stride, wave, lane);
    // tile metadata: up to kLdsPadTiles tiles starting at stream tile t0 -> this wavefront's pad
    // (tried: one shared pad per workgroup filled by ceil(tiles / 8) full 1 KB DMAs, and the 65 cell offsets of a range
    // loaded by two wavefronts and handed round through LDS - 75 instead of 96 vector memory instructions per range, but
    // the LDS round trip it puts in front of the DMAs costs more than the instructions saved: 0.97 ms instead of 0.83)
    const char* const tb = reinterpret_cast<const char*>(a.tiles);
    const uint32_t lane16 = (uint32_t)lane * 16u;
    auto meta_dma = [&](uint32_t t0, uint32_t nt, uint32_t padaddr) {
        const uint32_t n16 = (nt < (uint32_t)kLdsPadTiles ? nt : (uint32_t)kLdsPadTiles) * 128u;
        if (lane16 < n16)
            __builtin_amdgcn_global_load_lds((GLB_AS const void*)((tb + (int64_t)t0 * 128) + lane16), (LDS_AS void*)(uintptr_t)padaddr, 16, 0, 0);
        if constexpr (kLdsPadTiles > 8) {
            if (lane16 + 1024u < n16)
                __builtin_amdgcn_global_load_lds((GLB_AS const void*)((tb + (int64_t)t0 * 128 + 1024) + lane16), (LDS_AS void*)(uintptr_t)(padaddr + 1024u), 16, 0, 0);
        }
    };
    // Cell offsets of a range: lanes 0..MAXW load the words with an ORDINARY vector load, issued with the metadata request at
    // the end of a range and read at the end of the next (scalar loads stalled every range: the in-asm lgkmcnt(0) of the first
    // LDS block waits for them too).
    // This workgroup's hot (workgroup, range) pairs: pair rb + k of the compact cell table is column range rlist[rb + k] (every
    // range of the matrix, in order, where the graph has no locality to exploit; only a handful on a community graph).
    const int rb = a.rbase[wg], nr = a.rbase[wg + 1] - rb;
    // Lane MAXW + 1 of the same load fetches the pair's column range from rlist: one ordinary load per range carries both.
    const uint32_t* const cpl = a.cell_ptr + ((int64_t)rb * kLdsWaves + wave) * MAXW + (lane < MAXW + 1 ? lane : 0);
    const uint32_t* const rlp = reinterpret_cast<const uint32_t*>(a.rlist) + rb;
    const uint32_t* const lbase = lane == MAXW + 1 ? rlp : cpl;
    const int lstride = lane == MAXW + 1 ? 1 : kLdsWaves * MAXW;
    auto load_ov = [&](int r) -> uint32_t { return lbase[(int64_t)r * lstride]; };
    auto spread = [&](uint32_t ov, uint32_t (&o)[MAXW + 1]) {
#pragma unroll
        for (int j = 0; j <= MAXW; ++j) o[j] = (uint32_t)__builtin_amdgcn_readlane((int)ov, j);
    };

    // multiply the tiles [clo, chi) of the stream, whose metadata sits in the pad at `padaddr`, out of the buffer whose
    // lane base address is `bb`
    // (tried: issuing the next range's DMAs between the tiles instead of all at the top - the data then lands later
    // and the multiply stalls on the queue: 0.91 ms instead of 0.83 at Reddit D = 64)
    auto chunk = [&](const uint32_t (&o)[MAXW + 1], uint32_t clo, uint32_t chi, uint32_t padaddr, uint32_t bb) {
        if (clo >= chi) return;
        uint32_t idaddr = padaddr + idoff, maddr = padaddr + moff;
        uint32_t idw, m;
        lds_cell_ids(idaddr, maddr, idw, m);
        // (tried: a software-pipelined walk - tile t+1's reads issued, tile t's A fragment and MFMAs run under them, then the
        // wait: 0.80 ms instead of 0.66 at Reddit D = 64.  The four wavefronts of a SIMD already cover each other's LDS
        // round trips; what the walk queues on is the SIMD's issue slots, and the register copies that rotate the two
        // tile buffers add five instructions to a 30-instruction step)
#pragma unroll
        for (int j = 0; j < MAXW; ++j) {
            const uint32_t lo_ = o[j] > clo ? o[j] : clo, hi_ = o[j + 1] < chi ? o[j + 1] : chi;
            // The four wavefronts of a SIMD queue on its issue slots and the arbiter serves the oldest first: left alone, the
            // youngest runs its range at half speed and then finishes alone with nothing to hide its LDS latency, while the
            // other fifteen wait at the barrier.  Priority falls as a wavefront advances through its windows, so whoever is
            // behind goes first and the four arrive together.
            if (!(dbg & 32)) set_wave_priority(3 - j * 4 / MAXW);
            for (uint32_t t = lo_; t < hi_; ++t) {
                const uint32_t ad0 = bb + (idw & 0xffffu), ad1 = bb + (idw >> 16);
                // (tried: the A fragment read from a 4 KB LDS table, permuted so the nine common entries miss each other's
                // banks - 8 VALU instructions fewer, one 16-byte LDS read more: the same 0.60 ms)
                const half8 af = afrag_from_byte(m);
                half4 lo[NT], hi[NT];
                uint32_t nw_, nm;
                lds_cell_block<NT, PLANEB>(ad0, ad1, idaddr, maddr, lo, hi, nw_, nm);
#pragma unroll
                for (int s = 0; s < NT; ++s) {
                    const half8 bf = __builtin_shufflevector(lo[s], hi[s], 0, 1, 2, 3, 4, 5, 6, 7);
                    acc[j][s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf, acc[j][s], 0, 0, 0);
                }
                idw = nw_; m = nm;
                idaddr += 128u; maddr += 128u;
            }
        }
    };

    // The metadata stream is read once from HBM: a miss costs ~2500 cycles under this load, and a DMA issued at the top of a range
    // and waited for at its end put that latency on the critical path of EVERY range (with the multiply off: 0.73 ms against
    // 0.51 for the range fill alone; 0.56 once the metadata came from a cache-resident window).  So the metadata of range r+2 is
    // requested at the END of range r - after the multiply, into the pad range r has just finished with, behind the end-of-range
    // wait - and has the whole of range r+1 to arrive; only the range fill is issued at the top.  It crosses the barrier in
    // flight, hence the raw s_barrier (__syncthreads carries a fence for which hipcc drains vmcnt to 0).
    uint32_t o[MAXW + 1], on[MAXW + 1], onn[MAXW + 1];
    int rnext = 0;                                                           // column range of pair k + 1
    if (nr > 0) {
        const uint32_t ov0 = load_ov(0), ov1 = load_ov(nr > 1 ? 1 : 0);
        spread(ov0, o);
        spread(ov1, on);
        rnext = __builtin_amdgcn_readlane((int)ov1, MAXW + 1);
        meta_dma(o[0], o[MAXW] - o[0], pad0);
        if (nr > 1) meta_dma(on[0], on[MAXW] - on[0], pad0 + kLdsPadB);
        filler.fill(__builtin_amdgcn_readlane((int)ov0, MAXW + 1) * kLdsRows, lds0);
    }
    uint32_t ov = nr > 0 ? load_ov(nr > 2 ? 2 : 0) : 0u;
    wait_vm0();
    __syncthreads();
    uint64_t ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // dbg & 16: cycles in DMA issue / multiply / DMA wait / barrier; pad refills; longest multiply, wait; tiles
    for (int r = 0; r < nr; ++r) {
        const uint32_t buf = (uint32_t)(r & 1);
        const uint64_t t0 = (dbg & 16) ? __builtin_readcyclecounter() : 0;
        if (r + 1 < nr && !(dbg & 1)) filler.fill(rnext * kLdsRows, lds0 + (buf ^ 1u) * BUFB);
        const uint64_t t1 = (dbg & 16) ? __builtin_readcyclecounter() : 0;
        const uint32_t padaddr = pad0 + buf * kLdsPadB, bb = lanebase + buf * BUFB;
        const uint32_t tend = o[MAXW];
        uint32_t c0 = o[0];
        if (!(dbg & 2)) {
            for (;;) {   // (more than once only for a wavefront with more tiles in this range than its pad holds)
                const uint32_t left = tend - c0;
                const uint32_t c1 = c0 + (left < (uint32_t)kLdsPadTiles ? left : (uint32_t)kLdsPadTiles);
                chunk(o, c0, c1, padaddr, bb);
                c0 = c1;
                if (c0 >= tend) break;
                if (dbg & 16) ++ph[4];
                meta_dma(c0, tend - c0, padaddr);
                wait_vm0();
            }
        }
        const uint64_t t2 = (dbg & 16) ? __builtin_readcyclecounter() : 0;
        wait_vm0();   // range r+1 has landed (this wavefront's share), and its metadata and offsets, requested a range ago
        if (r + 2 < nr) {
            spread(ov, onn);
            rnext = __builtin_amdgcn_readlane((int)ov, MAXW + 1);           // (pair r + 2: filled at the top of the next range)
            ov = load_ov(r + 3 < nr ? r + 3 : r);
            if (!(dbg & 4)) meta_dma(onn[0], onn[MAXW] - onn[0], padaddr);
        }
        const uint64_t t3 = (dbg & 16) ? __builtin_readcyclecounter() : 0;
        if (!(dbg & 8)) __builtin_amdgcn_s_barrier();
        if (dbg & 16) { const uint64_t t4 = __builtin_readcyclecounter(); ph[0] += t1 - t0; ph[1] += t2 - t1; ph[2] += t3 - t2; ph[3] += t4 - t3;
                          if (t2 - t1 > ph[5]) ph[5] = t2 - t1; if (t3 - t2 > ph[6]) ph[6] = t3 - t2; ph[7] += tend - o[0]; }
#pragma unroll
        for (int j = 0; j <= MAXW; ++j) { o[j] = on[j]; on[j] = onn[j]; }
    }
    if (dbg & 16) {   // measurement run: no results, the wavefronts of workgroup 0 report their phase totals
        if (wg == 0 && blockIdx.y == 0 && lane == 0) {
#pragma unroll
            for (int k = 0; k < 8; ++k) a.y[wave * 8 + k] = (float)ph[k];
        }
        return;
    }

    const float inv1 = pow2f(-kx - 1);   // (the A fragment holds 2.0 per edge)
    if (a.parts) {
        // Split hub windows: the follower parts hand their partial sums to part 0 through LDS (the range buffers are free now),
        // which adds them in part order - the same sum on every run.
        __syncthreads();
        floatx4* const scr = reinterpret_cast<floatx4*>(smem);
#pragma unroll
        for (int j = 0; j < MAXW; ++j) {
            const uint32_t k = (pj[j] >> 8) & 0xffu, part = pj[j] & 0xffu, sidx = pj[j] >> 16;
            if (wj[j] >= 0 && k > 1u && part > 0u) {
#pragma unroll
                for (int s = 0; s < NT; ++s) scr[((int)sidx * NT + s) * 64 + lane] = acc[j][s];
                wj[j] = -1;   // (nothing more to do for this slot)
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < MAXW; ++j) {
            const uint32_t k = (pj[j] >> 8) & 0xffu, part = pj[j] & 0xffu, sidx = pj[j] >> 16;
            if (wj[j] >= 0 && k > 1u && part == 0u) {
                for (uint32_t q = 0; q + 1u < k; ++q)
#pragma unroll
                    for (int s = 0; s < NT; ++s) acc[j][s] += scr[((int)(sidx + q) * NT + s) * 64 + lane];
            }
        }
    }
    if (a.w) {
        // f3: the dense update behind the aggregation.  The range buffers are free now: every wavefront takes a 16 x (16 NT + 1)
        // float scratch, lays each window's aggregated rows out row-major and multiplies them by its columns' rows of W.
        __syncthreads();
        constexpr int DIN = NT * 16, LDP = DIN + 1;
        float* scratch = reinterpret_cast<float*>(smem) + wave * (16 * LDP);
        const int din = a.D - coloff < DIN ? a.D - coloff : DIN;        // real input columns of this pass
        const int tiles = (a.dout + 15) >> 4;
#pragma unroll
        for (int j = 0; j < MAXW; ++j) {
            if (wj[j] < 0) continue;
            // (the scratch is per wavefront, but lanes read what OTHER lanes stored: the stores must be done before the tile loop reads
            //  them, and its reads before the next window slot overwrites them - r2 ADVICE)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int s = 0; s < NT; ++s)
#pragma unroll
                for (int ii = 0; ii < 4; ++ii) scratch[(4 * g + ii) * LDP + 16 * s + i] = acc[j][s][ii] * inv1;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();
            const int64_t row0 = (int64_t)wj[j] * kWinRows + 4 * g;
            for (int t = 0; t < tiles; ++t) {
                const floatx4 c = dense_update_tile(scratch, LDP, din, a.w, coloff, a.dout, t, g, i);
                const int colg = 16 * t + i;
                if (colg < a.dout) {
#pragma unroll
                    for (int ii = 0; ii < 4; ++ii) {
                        if (row0 + ii >= a.N) continue;
                        float* dst = a.y + (row0 + ii) * (int64_t)a.dout + colg;
                        if (a.accumulate) atomicAdd(dst, c[ii]);
                        else *dst = relu_if(a.relu, c[ii]);
                    }
                }
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < MAXW; ++j) {
        if (wj[j] < 0) continue;
        const int64_t row0 = (int64_t)wj[j] * kWinRows + 4 * g;
#pragma unroll
        for (int s = 0; s < NT; ++s) {
            const int colg = coloff + 16 * s + i;
            if (colg < a.D) {
#pragma unroll
                for (int ii = 0; ii < 4; ++ii)
                    if (row0 + ii < a.N) a.y[(row0 + ii) * a.D + colg] = epi_apply(a.relu, a.epi, row0 + ii, colg, acc[j][s][ii] * inv1);
            }
        }
    }
}

// (explicit instantiations: with implicit ones hipcc 7.2 left one of the host stubs undefined)
template __global__ void spmm_lds_kernel<1, 4, false>(const SpmmLdsArgs);
template __global__ void spmm_lds_kernel<2, 4, false>(const SpmmLdsArgs);
template __global__ void spmm_lds_kernel<3, 4, false>(const SpmmLdsArgs);
template __global__ void spmm_lds_kernel<4, 4, false>(const SpmmLdsArgs);
template __global__ void spmm_lds_kernel<1, 8, false>(const SpmmLdsArgs);
template __global__ void spmm_lds_kernel<2, 8, false>(const SpmmLdsArgs);
#ifdef TCGNN_DEBUG_TIMERS
template __global__ void spmm_lds_kernel<1, 4, true>(const SpmmLdsArgs);
template __global__ void spmm_lds_kernel<2, 4, true>(const SpmmLdsArgs);
template __global__ void spmm_lds_kernel<3, 4, true>(const SpmmLdsArgs);
template __global__ void spmm_lds_kernel<4, 4, true>(const SpmmLdsArgs);
template __global__ void spmm_lds_kernel<1, 8, true>(const SpmmLdsArgs);
template __global__ void spmm_lds_kernel<2, 8, true>(const SpmmLdsArgs);
#endif

static constexpr int lds_spmm_bytes(int nt, int maxw) { return 2 * nt * lds_buf_rows(nt, maxw) * 32 + kLdsWaves * 2 * lds_pad_tiles(maxw, lds_buf_rows(nt, maxw)) * 128; }

static constexpr LaunchGeom lds_geom(int nt, int maxw) { return {kLdsWaves * 64, lds_spmm_bytes(nt, maxw), kLdsWaves / 4, maxw}; }   // (one workgroup per CU; the kernel's bound is the same kLdsWaves * 64)

template <int NT, int MAXW, bool DBG>
static hipError_t launch_lds_dbg(const SpmmLdsArgs& args, int nchunks, hipStream_t stream) {
    constexpr LaunchGeom g = lds_geom(NT, MAXW);
    return launch_kernel<spmm_lds_kernel<NT, MAXW, DBG>, g.lds_bytes>(dim3((unsigned)args.nwg, (unsigned)nchunks), g, stream, args);
}
template <int NT, int MAXW>
static hipError_t launch_lds_one(const SpmmLdsArgs& args, int nchunks, hipStream_t stream) {
#ifdef TCGNN_DEBUG_TIMERS   // (the phase-timer instantiations: make DEBUG_TIMERS=1)
    if (args.dbg) return launch_lds_dbg<NT, MAXW, true>(args, nchunks, stream);
#endif
    return launch_lds_dbg<NT, MAXW, false>(args, nchunks, stream);
}
static hipError_t launch_lds_any(int maxw, int nt, const SpmmLdsArgs& args, int nchunks, hipStream_t stream) {
    if (maxw == kLdsMaxW2) return with_width<2>(nt, [&](auto NT) { return launch_lds_one<NT, kLdsMaxW2>(args, nchunks, stream); });
    return with_width<4>(nt, [&](auto NT) { return launch_lds_one<NT, kLdsMaxW>(args, nchunks, stream); });
}
