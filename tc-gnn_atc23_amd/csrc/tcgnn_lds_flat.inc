// tcgnn_lds_flat.inc - the LDS-resident column-range SpMM over a FLAT cell stream (r03).  Included by tcgnn_device.hip after
// tcgnn_lds_spmm.inc, whose layouts, range filler, placement and hot / cold machinery it shares.
//
// Why: spmm_lds_kernel gives a cell (window slot, column range) as many 32-column tiles as it has columns.  On the Reddit shape
// a 760-row cell holds 25.7 columns on average - one tile - and two with probability 0.08, so (i) the sixteen wavefronts of a
// workgroup arrive at the barrier that ends every range with 8, 9 or 10 tile steps behind them and the range lasts as long as
// the slowest (PMC r01/r02: 900 of 4 000 cycles per range at the barrier), and (ii) every tile step drags a run-time cell
// walk along: offsets fetched per range and spread over SGPRs by readlane, bounds clamped per window slot, loop tests, pad
// pointers advanced, the next tile's ids read inside the step - 39 instructions per tile step of which 13.7 scalar.
//
// Here every cell has EXACTLY `TPC` tiles (1 where the mean cell is below a tile, 2 for the long single-plane ranges).  Columns
// beyond 32 TPC in a cell - about 1 % of them on the Reddit shape - leave the LDS-resident walk for the cold remainder, which
// spmm_cold_planar_kernel adds afterwards straight from the planar image.  What that buys:
//   * the tile of (pair k, wavefront v, slot j, t) sits at a COMPUTED position: no cell table, no offsets, no readlanes;
//   * every wavefront multiplies MAXW x TPC tiles in every range: they reach the barrier together;
//   * the range body is straight-line code: pad offsets are immediates, the metadata of a whole range is one contiguous block
//     per wavefront that lands with one LDS-DMA instruction (MAXW x TPC = 8) and is read into registers with three wide LDS
//     reads (ids of the 16 lane classes, 8 mask bytes per lane) instead of two narrow reads per tile;
//   * 7 % fewer tile steps (one per cell instead of 1.08).
// Per tile step: 2 address adds, the NEXT tile's 2 NT transposed reads + a counted wait for this tile's, 9 VALU for the A
// fragment, NT MFMAs, s_setprio (two register sets: tcgnn_lds_blocks.inc lds_flat_issue / step / drain).
//
// Block layout (T = MAXW x TPC tiles, 128 T bytes per (pair, wavefront)), built by flat_transpose_kernel from ordinary tiles:
//   words [c][x], c = 0..15, x = 0..T-1 : tile x's row-offset pair of lane class c = 4 g + (i >> 2)   (word c of the tile)
//   bytes [64 T + lane * T + x]         : tile x's adjacency byte of lane (g, i) = byte g of mask word i

// DENSE ENTRIES (r05).  A graph with communities (the SBM calibrated to real Reddit's block count: 22.5 % of a window's edges inside
// its own community of ~6 column ranges) has a handful of (workgroup, range) pairs whose cells hold ~240 columns - eight tiles -
// among 300 pairs whose cells hold ~20.  One tile per cell would send 17 % of the columns to the cold remainder, so such graphs kept
// the ordinary stream (run-time cell walk, 31 instructions per tile step against 19: 0.64 ms against the uniform graph's 0.46).
// Now the workgroup's walk is a list of ENTRIES: a normal entry = one range fill + the straight-line flat block as before; behind
// the normal entry of a pair whose cells overflow by much come DENSE entries - same range, no fill, same 1 KB block per wavefront,
// but the block holds up to T tiles in the ORDINARY tile format (16 id words + 16 mask words each: the cells' tiles beyond their
// first, in window-slot order) and a descriptor word counts them per window slot, so that the walk is MAXW compile-time slots x a
// run-time loop into a scratch accumulator that is added to the slot's own (no second set of MFMA sites on the 64 accumulators:
// r04 found hipcc copying them between two copies of a walk).  A workgroup that straddles two communities walks either one's dense
// entries with exactly the tiles it has there - the repeat-walk variant of r03 walked both at full length.
// A workgroup walks its normal entries first and its dense entries behind them, grouped by pair (their ranges are fetched again -
// a dozen fills, overlapped with the group before).  Per (entry, wavefront) four words, read ahead with one 16-byte load.
struct SpmmFlatArgs {
    const uint32_t* blocks;     // [entries][16 wavefronts][32 T words]
    const int32_t* order;       // window slots of the stream (as SpmmLdsArgs::order)
    const _Float16* x16;
    const uint32_t* hdr;
    float* y;
    int32_t N, D, stride /* planes of the planar image */, chunk0, xrows, nw, nwg;
    int32_t dbg, relu;
    const int32_t* rbase;       // [nwg + 1] first entry of every workgroup
    const uint32_t* rl2;        // [entries][4] entry records (w0, fetch range, normal entries of the workgroup, 0), then [entries][16 wavefronts] descriptor words (spmm_lds_flat_kernel has the bit layout)
    int32_t nent;               // entries of the stream (the descriptor words start at rl2 + 4 nent)
    const float* w;             // f3 (as SpmmLdsArgs::w)
    int32_t dout, accumulate;
    int32_t fill_quota;         // 1: the wavefronts whose last window slot is empty do the range fills (TCGNN_LDS_FILL_QUOTA=0: everybody fills)
    // the cold remainder INSIDE the kernel (layouts with 16 x NT KB of LDS to spare): per wavefront a list of cold tiles in
    // 256-byte records - 32 column ids (window slot in the top four bits), 16 mask words - of which it multiplies one per range (see cold_step)
    const int32_t* wcold_ptr;   // [nwg * 16 + 1] first record of every (workgroup, wavefront); nullptr: no in-kernel remainder
    const uint32_t* wcold;      // [records][64 words]
    SpmmSmallArgs fb;           // fb.guard != nullptr: this launch is its own range-guard fallback (lds_own_fallback)
};

typedef uint32_t uintx2 __attribute__((ext_vector_type(2)));

// the metadata of one range, all tiles of this wavefront: T id words of this lane's class, T mask bytes of this lane
template <int T> struct FlatMeta { uint32_t idw[T]; uint32_t mk[(T + 3) / 4]; };
template <int T> __device__ __forceinline__ void flat_meta_block(uint32_t idaddr, uint32_t maddr, FlatMeta<T>& m) {
    if constexpr (T == 8) {
        uintx4 q0, q1; uintx2 b;
        asm volatile("ds_read_b128 %0, %3\n\t"
                     "ds_read_b128 %1, %3 offset:16\n\t"
                     "ds_read_b64 %2, %4\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&v"(q0), "=&v"(q1), "=&v"(b) : "v"(idaddr), "v"(maddr) : "memory");
#pragma unroll
        for (int k = 0; k < 4; ++k) { m.idw[k] = q0[k]; m.idw[4 + k] = q1[k]; }
        m.mk[0] = b[0]; m.mk[1] = b[1];
    } else if constexpr (T == 4) {
        uintx4 q0; uint32_t b;
        asm volatile("ds_read_b128 %0, %2\n\t"
                     "ds_read_b32 %1, %3\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&v"(q0), "=&v"(b) : "v"(idaddr), "v"(maddr) : "memory");
#pragma unroll
        for (int k = 0; k < 4; ++k) m.idw[k] = q0[k];
        m.mk[0] = b;
    } else {
        static_assert(T == 16, "flat streams: 4, 8 or 16 tiles per wavefront and range");
        uintx4 q0, q1, q2, q3, b;
        asm volatile("ds_read_b128 %0, %5\n\t"
                     "ds_read_b128 %1, %5 offset:16\n\t"
                     "ds_read_b128 %2, %5 offset:32\n\t"
                     "ds_read_b128 %3, %5 offset:48\n\t"
                     "ds_read_b128 %4, %6\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&v"(q0), "=&v"(q1), "=&v"(q2), "=&v"(q3), "=&v"(b) : "v"(idaddr), "v"(maddr) : "memory");
#pragma unroll
        for (int k = 0; k < 4; ++k) { m.idw[k] = q0[k]; m.idw[4 + k] = q1[k]; m.idw[8 + k] = q2[k]; m.idw[12 + k] = q3[k]; m.mk[k] = b[k]; }
    }
}

template <int NT, int PLANE> __device__ __forceinline__ void flat_issue(uint32_t ad0, uint32_t ad1, half4* nlo, half4* nhi) {
    if constexpr (NT == 1) lds_flat_issue1<PLANE>(ad0, ad1, nlo, nhi);
    else if constexpr (NT == 2) lds_flat_issue2<PLANE>(ad0, ad1, nlo, nhi);
    else if constexpr (NT == 3) lds_flat_issue3<PLANE>(ad0, ad1, nlo, nhi);
    else lds_flat_issue4<PLANE>(ad0, ad1, nlo, nhi);
}
template <int NT, int PLANE> __device__ __forceinline__ void flat_step(uint32_t ad0, uint32_t ad1, half4* nlo, half4* nhi, half4* clo, half4* chi) {
    if constexpr (NT == 1) lds_flat_step1<PLANE>(ad0, ad1, nlo, nhi, clo, chi);
    else if constexpr (NT == 2) lds_flat_step2<PLANE>(ad0, ad1, nlo, nhi, clo, chi);
    else if constexpr (NT == 3) lds_flat_step3<PLANE>(ad0, ad1, nlo, nhi, clo, chi);
    else lds_flat_step4<PLANE>(ad0, ad1, nlo, nhi, clo, chi);
}
template <int NT, int PLANE> __device__ __forceinline__ void flat_step_if(uint32_t on, uint32_t ad0, uint32_t ad1, half4* nlo, half4* nhi, half4* clo, half4* chi) {
    if constexpr (NT == 1) lds_flat_step_if1<PLANE>(on, ad0, ad1, nlo, nhi, clo, chi);
    else if constexpr (NT == 2) lds_flat_step_if2<PLANE>(on, ad0, ad1, nlo, nhi, clo, chi);
    else if constexpr (NT == 3) lds_flat_step_if3<PLANE>(on, ad0, ad1, nlo, nhi, clo, chi);
    else lds_flat_step_if4<PLANE>(on, ad0, ad1, nlo, nhi, clo, chi);
}
template <int NT> __device__ __forceinline__ void flat_drain(half4* clo, half4* chi) {
    if constexpr (NT == 1) lds_flat_drain1(clo, chi);
    else if constexpr (NT == 2) lds_flat_drain2(clo, chi);
    else if constexpr (NT == 3) lds_flat_drain3(clo, chi);
    else lds_flat_drain4(clo, chi);
}

// A fragment from byte `b` (compile-time) of a packed mask word: v_perm_b32 puts the byte into both halves, then afrag's shifts
template <int B> __device__ __forceinline__ half8 flat_afrag(uint32_t mkw) {
    const uint32_t mm = __builtin_amdgcn_perm(mkw, mkw, 0x0c000c00u | (uint32_t)B | ((uint32_t)B << 16));
    uintx4 q;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const ushort2v k = {(unsigned short)(1u << (14 - 2 * j)), (unsigned short)(1u << (13 - 2 * j))};
        q[j] = __builtin_bit_cast(uint32_t, (ushort2v)(__builtin_bit_cast(ushort2v, mm) * k)) & 0x40004000u;
    }
    return __builtin_bit_cast(half8, q);
}

// The same as a SELECT mask (edge-valued walk, tcgnn_lds_val.inc): the bit goes to bit 15 of its half and an arithmetic shift spreads
// it - all ones or 0 - so that `mask & slot values` is the value itself.  Same three instructions per register as "2.0 or 0, times
// the value", without the factor 2 that overflowed fp16 for a maximum that rounds up to 2^15 (ADVICE r04).
typedef short short2v __attribute__((ext_vector_type(2)));
template <int B> __device__ __forceinline__ half8 flat_amask(uint32_t mkw) {
    const uint32_t mm = __builtin_amdgcn_perm(mkw, mkw, 0x0c000c00u | (uint32_t)B | ((uint32_t)B << 16));
    uintx4 q;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const ushort2v k = {(unsigned short)(1u << (15 - 2 * j)), (unsigned short)(1u << (14 - 2 * j))};
        const short2v sh = __builtin_bit_cast(short2v, (ushort2v)(__builtin_bit_cast(ushort2v, mm) * k)) >> (short2v){15, 15};
        q[j] = __builtin_bit_cast(uint32_t, sh);
    }
    return __builtin_bit_cast(half8, q);
}

// ordinary tiles [(pair, wavefront)][T][32 words] -> blocks; one thread per output word
// (the block of a DENSE entry - bit 31 of its first entry word - keeps the ordinary tile format: copied)
__global__ __launch_bounds__(256) void flat_transpose_kernel(const uint32_t* __restrict__ tiles, uint32_t* __restrict__ blocks, int64_t nblocks, int32_t T,
                                                             const uint32_t* __restrict__ rl2 = nullptr) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int words = 32 * T;
    if (k >= nblocks * words) return;
    const int64_t blk = k / words;
    if (rl2 && (rl2[(blk / kLdsWaves) * 4] >> 31)) { blocks[k] = tiles[k]; return; }
    const int o = (int)(k - blk * words);
    const uint32_t* src = tiles + blk * words;
    uint32_t v;
    if (o < 16 * T) {                       // ids: [class c][tile x] <- word c of tile x
        const int c = o / T, x = o % T;
        v = src[x * 32 + c];
    } else {                                // mask bytes: byte (lane * T + x) <- byte g of mask word i of tile x
        v = 0u;
        const int b0 = (o - 16 * T) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int b = b0 + q, lane = b / T, x = b % T;
            const int g = lane >> 4, i = lane & 15;
            v |= ((src[x * 32 + 16 + i] >> (8 * g)) & 0xffu) << (8 * q);
        }
    }
    blocks[k] = v;
}

// cold tiles -> the per-wavefront records the flat kernel multiplies itself: entry = tile | slot << 28; one thread per record word
__global__ __launch_bounds__(256) void flat_cold_records_kernel(const uint32_t* __restrict__ list, int64_t n, const int32_t* __restrict__ ccols, const uint32_t* __restrict__ cmask,
                                                                uint32_t* __restrict__ rec) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n * 64) return;
    const uint32_t e = list[k >> 6];
    const int64_t t = e & 0x0fffffffu;
    const int o = (int)(k & 63);
    // (row ids stay below 2^27 - the planar image is addressed through one 4 GB descriptor - so the window slot rides in their top bits)
    rec[k] = o < 32 ? ((uint32_t)ccols[t * kWbCols + o] | (e & 0xf0000000u)) : (o < 48 ? cmask[t * kWinRows + (o - 32)] : 0u);
}

// This lane's number, re-derived WHERE IT IS USED: a volatile statement, so that nothing computed from it is hoisted out of the entry
// loops and kept alive - or spilled - through the tile walk (the kernel has exactly the 128 registers sixteen wavefronts per CU leave;
// hipcc answered hoisted per-lane constants of the fills and of the cold remainder with scratch reloads behind a vmcnt(0))
__device__ __forceinline__ uint32_t lane_id_now() {
    uint32_t l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

// RangeFiller (tcgnn_lds_spmm.inc) with the per-instruction row numbers recomputed from one register (lane / 2) instead of kept in
// MAXC registers: the flat kernel needs those for the second register set of its tile walk and the cold remainder's state.
template <int NT, int BR>
struct FlatRangeFiller {
    // The instructions of a range are dealt to `nfill` of the sixteen wavefronts (rank 0 .. nfill - 1; rank < 0: this wavefront
    // issues none).  All sixteen by default; where most wavefronts hold one window fewer than the fullest ones (7 against 8 on
    // the Reddit shape) those - at least kMinFillers of them - take the fills, so the full wavefronts, which every range waits for,
    // spend their time on tile steps only (a fill instruction costs its issuer 100-180 cycles of queueing).
    static constexpr int IPP = BR / 32, TOTAL = NT * IPP, kMinFillers = 12, MAXC = (TOTAL + kMinFillers - 1) / kMinFillers;
    __amdgpu_buffer_rsrc_t xrsrc;
    uint32_t zrow;
    int rank, nfill, plane0, nplanes, xrows;
    __device__ __forceinline__ FlatRangeFiller(const _Float16* x16p, int xrows_, int plane0_, int nplanes_, int rank_, int nfill_, int lane) {
        xrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)x16p, (short)32, nplanes_ * xrows_, 0x00020000);
        zrow = (uint32_t)(xrows_ - 1);
        (void)lane;
        rank = rank_; nfill = nfill_; plane0 = plane0_; nplanes = nplanes_; xrows = xrows_;
    }
    __device__ __forceinline__ void fill(int r0, uint32_t buf) const {
        if (rank < 0) return;
        // (lane / 2 and lane % 2 are re-derived per call - mbcnt - instead of kept: the kernel has no register to spare, and hipcc
        //  answered one more live value with a scratch reload and a vmcnt(0) in front of every fill)
        const uint32_t l2 = lane_id_now();
        const uint32_t lrow = l2 >> 1;
        const int hoff = (int)(l2 & 1u) * 16;
#pragma unroll
        for (int q = 0; q < MAXC; ++q) {
            const int k = rank + nfill * q;                         // (wave-uniform)
            if (k < TOTAL) {
                const int plane = k / IPP, blk = k - plane * IPP;
                const bool real_plane = plane0 + plane < nplanes;   // (a pass whose last plane lies beyond the matrix: all zeros)
                const uint32_t row = (uint32_t)(blk * 32) + lrow;
                const uint32_t want = (uint32_t)r0 + row;
                const uint32_t srow = (row < (uint32_t)(BR - 8) && real_plane && want < zrow) ? want : zrow;
                const int pbase = real_plane ? (plane0 + plane) * xrows : 0;
                __builtin_amdgcn_struct_ptr_buffer_load_lds(xrsrc, (LDS_AS void*)(uintptr_t)(buf + (uint32_t)plane * (BR * 32u) + (uint32_t)blk * 1024u), 16,
                                                            pbase + (int)srow, hoff, 0, 0, 0);
            }
        }
    }
};

static constexpr bool flat_dense_ok(int nt, int maxw, int tpc) { return tpc == 1 && nt <= 2 && maxw * tpc <= 15; }
// (lng: the long walk - 960-row buffers, lds_stream_of's slot 7 - whose cold remainder shares kLongPoolTiles gather tiles)
static constexpr int kLongPoolTiles = 4;
static constexpr int kLongTurn = 8;       // a wavefront of the long walk may issue a cold gather in one entry of eight (tcgnn_lds_flat_kernel.inc)
static constexpr int flat_cold_tiles(bool lng) { return lng ? kLongPoolTiles : kLdsWaves; }
static constexpr int flat_lds_main(int nt, int maxw, int tpc, bool lng = false) { return 2 * nt * lds_buf_rows(nt, maxw, lng) * 32 + kLdsWaves * 2 * (maxw * tpc * 128); }
// the in-kernel cold remainder needs one gathered tile (32 rows x NT planes x 32 bytes) per wavefront
static constexpr bool flat_cold_fits(int nt, int maxw, int tpc, bool lng = false) { return flat_lds_main(nt, maxw, tpc, lng) + flat_cold_tiles(lng) * nt * 1024 <= 160 * 1024; }
// (+ 128 bytes: the walk of a dense entry reads the id word / mask byte of "the next tile" behind its last one)
static constexpr int flat_lds_bytes(int nt, int maxw, int tpc, bool lng = false) { return flat_lds_main(nt, maxw, tpc, lng) + (flat_cold_fits(nt, maxw, tpc, lng) ? flat_cold_tiles(lng) * nt * 1024 : (flat_dense_ok(nt, maxw, tpc) ? 128 : 0)); }
static_assert(flat_lds_bytes(2, 8, 1, true) == 160 * 1024 && flat_cold_fits(2, 8, 1, true), "the long walk: 2 x 2 planes x 960 rows, 32 KB of pads, four 2 KB gather tiles");
static_assert(flat_lds_bytes(2, 8, 1) == 160 * 1024 && flat_lds_bytes(1, 8, 1) == 80 * 1024, "the shipped 8-window layouts keep their LDS");
static_assert(lds_buf_rows(2, 8, true) * 32 < 32768 && kLongPoolTiles * 4 == kLdsWaves && kLongTurn == 2 * 4, "plane offsets as immediates, 16-bit row offsets; four wavefronts per pool tile, a turn every two entries");
// (measured and not kept, r03: an L2 warm-up - one 4-byte-per-lane LDS-DMA per workgroup and range touching every 16th line of
//  the range after next, shared between the workgroups of an XCD: with the multiply switched off a range lasts ~2 900 cycles, but
//  that is not an L2 miss the warm-up could take - 0.602 ms with it, 0.607 without)

// WITH_DENSE = false: the instantiation for streams WITHOUT dense entries (the launcher knows: CellStream::dense_entries).  The dense
// walk is dead code there, and merely having it in the kernel costs the normal entries 5.5 % (r05, uniform Reddit shape, same box:
// 0.477 ms with it, 0.451 without - r04's kernel 0.457): the second loop's live ranges push the first one's registers around.
#define TCGNN_KERNEL_LONG false
#define TCGNN_KERNEL_NAME spmm_lds_flat_kernel
#define TCGNN_KERNEL_PARAM const SpmmFlatArgs a
#define TCGNN_KERNEL_PROLOGUE
#define TCGNN_KERNEL_STORE(relu, row, col, v) relu_if(relu, v)
#include "tcgnn_lds_flat_kernel.inc"
#undef TCGNN_KERNEL_NAME
#undef TCGNN_KERNEL_PARAM
#undef TCGNN_KERNEL_PROLOGUE
#undef TCGNN_KERNEL_STORE
// tcgnn_spmm_scaled on the flat stream (binary A, no fused dense update): the final store applies row scale, bias and ReLU - also
// on the headline graph, whose cold remainder this kernel multiplies itself
struct SpmmFlatEpiArgs { SpmmFlatArgs a; Epi epi; };
#define TCGNN_KERNEL_NAME spmm_lds_flat_epi_kernel
#define TCGNN_KERNEL_PARAM const SpmmFlatEpiArgs e
#define TCGNN_KERNEL_PROLOGUE const SpmmFlatArgs& a = e.a;
#define TCGNN_KERNEL_STORE(relu, row, col, v) epi_apply(relu, e.epi, row, col, v)
#include "tcgnn_lds_flat_kernel.inc"
#undef TCGNN_KERNEL_NAME
#undef TCGNN_KERNEL_PARAM
#undef TCGNN_KERNEL_PROLOGUE
#undef TCGNN_KERNEL_STORE
#undef TCGNN_KERNEL_LONG
// the LONG walk (952-row ranges, cell stream slot kLdsLongSlot) and its twin: <2, 8, 1> only
#define TCGNN_KERNEL_LONG true
#define TCGNN_KERNEL_NAME spmm_lds_flat_long_kernel
#define TCGNN_KERNEL_PARAM const SpmmFlatArgs a
#define TCGNN_KERNEL_PROLOGUE
#define TCGNN_KERNEL_STORE(relu, row, col, v) relu_if(relu, v)
#include "tcgnn_lds_flat_kernel.inc"
#undef TCGNN_KERNEL_NAME
#undef TCGNN_KERNEL_PARAM
#undef TCGNN_KERNEL_PROLOGUE
#undef TCGNN_KERNEL_STORE
#define TCGNN_KERNEL_NAME spmm_lds_flat_long_epi_kernel
#define TCGNN_KERNEL_PARAM const SpmmFlatEpiArgs e
#define TCGNN_KERNEL_PROLOGUE const SpmmFlatArgs& a = e.a;
#define TCGNN_KERNEL_STORE(relu, row, col, v) epi_apply(relu, e.epi, row, col, v)
#include "tcgnn_lds_flat_kernel.inc"
#undef TCGNN_KERNEL_NAME
#undef TCGNN_KERNEL_PARAM
#undef TCGNN_KERNEL_PROLOGUE
#undef TCGNN_KERNEL_STORE
#undef TCGNN_KERNEL_LONG

// (explicit instantiations: with implicit ones hipcc 7.2 leaves some host stubs undefined)
template __global__ void spmm_lds_flat_kernel<1, 4, 1, false, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<1, 4, 1, false, true>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<2, 4, 1, false, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<2, 4, 1, false, true>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<3, 4, 1, false, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<4, 4, 1, false, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<1, 8, 1, false, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<1, 8, 1, false, true>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<2, 8, 1, false, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<2, 8, 1, false, true>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<1, 4, 2, false, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<2, 4, 2, false, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<3, 4, 2, false, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<4, 4, 2, false, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<1, 8, 2, false, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<2, 8, 2, false, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_long_kernel<2, 8, 1, false, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_long_kernel<2, 8, 1, false, true>(const SpmmFlatArgs);
#ifdef TCGNN_DEBUG_TIMERS
template __global__ void spmm_lds_flat_long_kernel<2, 8, 1, true, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_long_kernel<2, 8, 1, true, true>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<1, 4, 1, true, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<1, 4, 1, true, true>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<2, 4, 1, true, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<2, 4, 1, true, true>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<3, 4, 1, true, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<4, 4, 1, true, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<1, 8, 1, true, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<1, 8, 1, true, true>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<2, 8, 1, true, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<2, 8, 1, true, true>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<1, 4, 2, true, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<2, 4, 2, true, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<3, 4, 2, true, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<4, 4, 2, true, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<1, 8, 2, true, false>(const SpmmFlatArgs);
template __global__ void spmm_lds_flat_kernel<2, 8, 2, true, false>(const SpmmFlatArgs);
#endif

// (the twin: the phase-timer instantiations are not needed)
template __global__ void spmm_lds_flat_epi_kernel<1, 4, 1, false, false>(const SpmmFlatEpiArgs);
template __global__ void spmm_lds_flat_epi_kernel<1, 4, 1, false, true>(const SpmmFlatEpiArgs);
template __global__ void spmm_lds_flat_epi_kernel<2, 4, 1, false, false>(const SpmmFlatEpiArgs);
template __global__ void spmm_lds_flat_epi_kernel<2, 4, 1, false, true>(const SpmmFlatEpiArgs);
template __global__ void spmm_lds_flat_epi_kernel<3, 4, 1, false, false>(const SpmmFlatEpiArgs);
template __global__ void spmm_lds_flat_epi_kernel<4, 4, 1, false, false>(const SpmmFlatEpiArgs);
template __global__ void spmm_lds_flat_epi_kernel<1, 8, 1, false, false>(const SpmmFlatEpiArgs);
template __global__ void spmm_lds_flat_epi_kernel<1, 8, 1, false, true>(const SpmmFlatEpiArgs);
template __global__ void spmm_lds_flat_epi_kernel<2, 8, 1, false, false>(const SpmmFlatEpiArgs);
template __global__ void spmm_lds_flat_epi_kernel<2, 8, 1, false, true>(const SpmmFlatEpiArgs);
template __global__ void spmm_lds_flat_epi_kernel<1, 4, 2, false, false>(const SpmmFlatEpiArgs);
template __global__ void spmm_lds_flat_epi_kernel<2, 4, 2, false, false>(const SpmmFlatEpiArgs);
template __global__ void spmm_lds_flat_epi_kernel<3, 4, 2, false, false>(const SpmmFlatEpiArgs);
template __global__ void spmm_lds_flat_epi_kernel<4, 4, 2, false, false>(const SpmmFlatEpiArgs);
template __global__ void spmm_lds_flat_epi_kernel<1, 8, 2, false, false>(const SpmmFlatEpiArgs);
template __global__ void spmm_lds_flat_epi_kernel<2, 8, 2, false, false>(const SpmmFlatEpiArgs);
template __global__ void spmm_lds_flat_long_epi_kernel<2, 8, 1, false, false>(const SpmmFlatEpiArgs);
template __global__ void spmm_lds_flat_long_epi_kernel<2, 8, 1, false, true>(const SpmmFlatEpiArgs);

static constexpr LaunchGeom flat_geom(int nt, int maxw, int tpc, bool lng = false) { return {kLdsWaves * 64, flat_lds_bytes(nt, maxw, tpc, lng), kLdsWaves / 4, maxw}; }   // (as lds_geom)

template <int NT, int MAXW, int TPC, bool DBG, bool WITH_DENSE>
static hipError_t launch_flat_dbg(const SpmmFlatArgs& args, int nchunks, hipStream_t stream, const Epi& epi) {
    constexpr LaunchGeom g = flat_geom(NT, MAXW, TPC);
    const dim3 grid((unsigned)args.nwg, (unsigned)nchunks);
    // (tcgnn_spmm_scaled: the twin with the epilogue in its store; it has no phase-timer instantiations)
    if constexpr (DBG) return launch_kernel<spmm_lds_flat_kernel<NT, MAXW, TPC, true, WITH_DENSE>, g.lds_bytes>(grid, g, stream, args);
    else return launch_plain_or_twin<spmm_lds_flat_kernel<NT, MAXW, TPC, false, WITH_DENSE>, spmm_lds_flat_epi_kernel<NT, MAXW, TPC, false, WITH_DENSE>, g.lds_bytes>(grid, g, stream, args, epi);
}
template <int NT, int MAXW, int TPC, bool DBG>
static hipError_t launch_flat_dense(const SpmmFlatArgs& args, int nchunks, hipStream_t stream, bool dense, const Epi& epi) {
    if constexpr (flat_dense_ok(NT, MAXW, TPC)) {
        if (dense) return launch_flat_dbg<NT, MAXW, TPC, DBG, true>(args, nchunks, stream, epi);
    }
    return launch_flat_dbg<NT, MAXW, TPC, DBG, false>(args, nchunks, stream, epi);   // (build_lds_cells makes dense entries only for layouts whose kernel walks them)
}
template <int NT, int MAXW, int TPC>
static hipError_t launch_flat_one(const SpmmFlatArgs& args, int nchunks, hipStream_t stream, bool dense, const Epi& epi) {
#ifdef TCGNN_DEBUG_TIMERS   // (the phase-timer instantiations: make DEBUG_TIMERS=1)
    if (args.dbg) return launch_flat_dense<NT, MAXW, TPC, true>(args, nchunks, stream, dense, epi);
#endif
    return launch_flat_dense<NT, MAXW, TPC, false>(args, nchunks, stream, dense, epi);
}
template <int TPC>
static hipError_t launch_flat_tpc(int maxw, int nt, const SpmmFlatArgs& args, int nchunks, hipStream_t stream, bool dense, const Epi& epi) {
    if (maxw == kLdsMaxW2) return with_width<2>(nt, [&](auto NT) { return launch_flat_one<NT, kLdsMaxW2, TPC>(args, nchunks, stream, dense, epi); });
    return with_width<4>(nt, [&](auto NT) { return launch_flat_one<NT, kLdsMaxW, TPC>(args, nchunks, stream, dense, epi); });
}
// dense: the stream has dense entries (CellStream::dense_entries > 0) - the instantiation that walks them
// the long walk: one layout, with / without dense entries, plain or twin (+ the phase-timer pair)
template <bool DBG, bool WITH_DENSE>
static hipError_t launch_flat_long_dbg(const SpmmFlatArgs& args, int nchunks, hipStream_t stream, const Epi& epi) {
    constexpr LaunchGeom g = flat_geom(2, kLdsMaxW2, 1, true);
    const dim3 grid((unsigned)args.nwg, (unsigned)nchunks);
    if constexpr (DBG) return launch_kernel<spmm_lds_flat_long_kernel<2, kLdsMaxW2, 1, true, WITH_DENSE>, g.lds_bytes>(grid, g, stream, args);
    else return launch_plain_or_twin<spmm_lds_flat_long_kernel<2, kLdsMaxW2, 1, false, WITH_DENSE>, spmm_lds_flat_long_epi_kernel<2, kLdsMaxW2, 1, false, WITH_DENSE>, g.lds_bytes>(grid, g, stream, args, epi);
}
static hipError_t launch_flat_long(const SpmmFlatArgs& args, int nchunks, hipStream_t stream, bool dense, const Epi& epi) {
#ifdef TCGNN_DEBUG_TIMERS
    if (args.dbg) return dense ? launch_flat_long_dbg<true, true>(args, nchunks, stream, epi) : launch_flat_long_dbg<true, false>(args, nchunks, stream, epi);
#endif
    return dense ? launch_flat_long_dbg<false, true>(args, nchunks, stream, epi) : launch_flat_long_dbg<false, false>(args, nchunks, stream, epi);
}
static hipError_t launch_flat_any(int maxw, int nt, int tpc, const SpmmFlatArgs& args, int nchunks, hipStream_t stream, bool dense,
                                  const Epi& epi = Epi{nullptr, nullptr}, bool long_ranges = false) {
    if (long_ranges) return (maxw == kLdsMaxW2 && nt == 2 && tpc == 1) ? launch_flat_long(args, nchunks, stream, dense, epi) : hipErrorInvalidValue;
    return tpc == 2 ? launch_flat_tpc<2>(maxw, nt, args, nchunks, stream, dense, epi) : launch_flat_tpc<1>(maxw, nt, args, nchunks, stream, dense, epi);
}

// ------------------------------------------------------------------------------------------------------------------------------
// The cold remainder of a flat stream, added straight from the PLANAR image (no second, row-major image and no second staging
// pass): one wavefront per window, lane = (window row, 16-column quarter of this launch's 64-column group) - a lane owns 16
// accumulators of ONE row.  Per cold tile a lane walks the set bits of its row's mask word (column ids broadcast by ds_bpermute)
// four edges at a time and fetches its 32-byte record of each neighbour row: eight 16-byte loads in flight per lane.
// ~1 % of the edges on the Reddit shape (3 tiles per window): latency-bound by construction (the first version - lane = feature
// column, accumulators in LDS - took 105 us there).
// Y += sum (x 2^-kx), with the ReLU of a fused call applied here (the LDS-resident kernel then stored the raw sums).
// ------------------------------------------------------------------------------------------------------------------------------
struct ColdPlanarArgs {
    const int64_t* cold_ptr;    // [nw + 1]
    const int32_t* ccols;       // [tiles][32]
    const uint32_t* cmask;      // [tiles][16]
    const _Float16* x16;        // planar image
    const uint32_t* hdr;
    float* y;
    int32_t N, D, xrows, nw, col0, ncols, relu;   // columns [col0, col0 + ncols) of Y (whole planes)
    Epi epi;                                      // tcgnn_spmm_scaled's row scale / bias: applied here, like the ReLU
};
__global__ __launch_bounds__(256, 2) void spmm_cold_planar_kernel(const ColdPlanarArgs a) {   // (8 wavefronts per SIMD: a wavefront is a chain of ~8 memory round trips)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int w = blockIdx.x * 4 + wave;
    if (w >= a.nw) return;
    const int64_t t0 = a.cold_ptr[w], t1 = a.cold_ptr[w + 1];
    if (t0 == t1 && !a.relu && !a.epi.rs && !a.epi.bias) return;   // (a fused ReLU is applied here for every window: the LDS-resident kernel stored raw sums)
    const int r = lane >> 2, q = lane & 3;                          // window row, 16-column quarter of this launch's 64-column group
    const int plane = (a.col0 >> 4) + (int)blockIdx.y * 4 + q;
    const bool live = plane * 16 < a.col0 + a.ncols && plane * 16 < ((a.D + 15) & ~15);
    float acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
    const int zrow = a.xrows - 1;                                   // the all-zero record
    const half8* xp = reinterpret_cast<const half8*>(a.x16 + (int64_t)(live ? plane : 0) * a.xrows * 16);
    int32_t cv = 0; uint32_t mv = 0u;
    if (t0 < t1) { cv = a.ccols[t0 * kWbCols + (lane & 31)]; mv = a.cmask[t0 * kWinRows + r]; }
    for (int64_t t = t0; t < t1; ++t) {
    if (range_is_wide(a.hdr, 0)) return;   // (range guard: the fp32 fallback launched behind this kernel does the work)
        int32_t cvn = 0; uint32_t mvn = 0u;                           // the next tile's ids and mask word: requested before this tile's rows
        if (t + 1 < t1) { cvn = a.ccols[(t + 1) * kWbCols + (lane & 31)]; mvn = a.cmask[(t + 1) * kWinRows + r]; }
        while (__any(mv != 0u)) {   // rounds of up to two edges per row: four 16-byte loads in flight per lane
            int c[2];
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const bool v = mv != 0u;
                const int k = v ? __builtin_ctz(mv) : 0;
                mv &= mv - 1u;
                const int cc = __shfl(cv, k);
                c[it] = (v && live && cc < zrow) ? cc : zrow;
            }
            half8 x[2][2];
#pragma unroll
            for (int it = 0; it < 2; ++it) { x[it][0] = xp[(int64_t)c[it] * 2]; x[it][1] = xp[(int64_t)c[it] * 2 + 1]; }
#pragma unroll
            for (int it = 0; it < 2; ++it)
#pragma unroll
                for (int e = 0; e < 8; ++e) { acc[e] += (float)x[it][0][e]; acc[8 + e] += (float)x[it][1][e]; }
        }
        cv = cvn; mv = mvn;
    }
    const int64_t row = (int64_t)w * kWinRows + r;
    if (!live || row >= a.N) return;
    const float inv = pow2f(-scale_exp_from_bits(a.hdr[kHdrMaxX]));
    float* dst = a.y + row * a.D + plane * 16;
    if (plane * 16 + 16 <= a.D && (a.D & 3) == 0) {
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4) {
            float4 v = reinterpret_cast<float4*>(dst)[e4];
            const int c0 = plane * 16 + 4 * e4;
            v.x = epi_apply(a.relu, a.epi, row, c0, v.x + acc[4 * e4] * inv); v.y = epi_apply(a.relu, a.epi, row, c0 + 1, v.y + acc[4 * e4 + 1] * inv);
            v.z = epi_apply(a.relu, a.epi, row, c0 + 2, v.z + acc[4 * e4 + 2] * inv); v.w = epi_apply(a.relu, a.epi, row, c0 + 3, v.w + acc[4 * e4 + 3] * inv);
            reinterpret_cast<float4*>(dst)[e4] = v;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 16; ++e)
            if (plane * 16 + e < a.D) dst[e] = epi_apply(a.relu, a.epi, row, plane * 16 + e, dst[e] + acc[e] * inv);
    }
}
