// tcgnn_sddmm.inc - SDDMM (forward_ef): sddmm_kernel, sddmm_wide_kernel.  Included by tcgnn_device.hip.
// ------------------------------------------------------------------------------------------
// SDDMM:  ef[e] = <X16[row e], X16[col e]>
// ------------------------------------------------------------------------------------------
struct SddmmArgs {
    const int64_t* wb_ptr;
    const int32_t* order;
    const int32_t* cols;
    const uint32_t* mask;
    const int32_t* ebase;
    const _Float16* x16;
    const uint32_t* hdr;
    float* ef;
    int32_t N, Nc, row_off, Dpad, stride;
    const int32_t* rowptr;
    const uint32_t* bptr;       // range-blocked walk (nranges > 0)
    int32_t nbuckets, gsel, nranges, nw;
    int32_t big;                // fp16 image >= 4 GB: 64-bit lane addresses instead of the buffer descriptor
    int32_t xcd;                // range-major walk with XCD affinity: workgroup b (on XCD b % 8) takes the ranges r = b % 8, b % 8 + 8, ... only
    int32_t ident;              // range-major walk: item q is window q itself, not order[q] (r06).  `order` in its XCD-contiguous form puts the
                                // x-th eighth of the graph at the positions = x mod 8, and a persistent wavefront's stride is a multiple of 8: it
                                // would draw all its windows from ONE eighth - on a graph with communities the wavefronts of the eighth that holds
                                // a range's communities carry 3x the tiles of the others in that range and the walk falls out of step
    int32_t use_sync;           // the slice-synchronised range walk (tcgnn_sync_walk.inc): this launch covers slice `sync.round` of every XCD's share
    SyncArgs sync;
    // tcgnn_sddmm2 (the TWO instantiations only; behind every field the single-operand kernels read, whose offsets stay): the WINDOW operand's
    // own image and header - same pitch and row count as x16, its own power-of-two scale.  x16 / hdr are then the gathered operand's
    const _Float16* xa16;
    const uint32_t* hdr_a;
    // tcgnn_sddmm_heads (the HF > 0 instantiations only, behind everything above): ef is [H][E] head-major, E floats a head; pass
    // blockIdx.y of a launch takes the G heads from head0 + blockIdx.y G on - columns (head0 + blockIdx.y G) HF .. of both images
    int64_t E;
    int32_t head0;
};
// tcgnn_sddmm2's range guard (level >= 2: Z's kHdrCapX = 2 D, else 0): the whole call goes the fp32 way when either operand holds elements
// that lose bits in its image (range_spread, counted in kHdrTiny) and k max|X| max|Z| 2^-39 could leave 2^-10 - range_is_wide's rule for
// SDDMM with the product of the two maxima in place of the square of one
__device__ __forceinline__ bool sddmm2_wide(const uint32_t* hx, const uint32_t* hz) {
    int ex, ez;
    const bool sx = range_spread(hx, 0, ex) && hx[kHdrTiny] != 0u, sz = range_spread(hz, 0, ez) && hz[kHdrTiny] != 0u;
    const uint32_t cap = hz[kHdrCapX];
    if (!(sx || sz) || cap == 0u || hx[kHdrMaxX] == 0u || hz[kHdrMaxX] == 0u) return false;
    const uint32_t n = (sx ? hx[kHdrTiny] : 0u) + (sz ? hz[kHdrTiny] : 0u);
    return (ex - 127) + (ez - 127) >= 29 - ceil_log2_u32(n < cap ? n : cap);
}

// LDS of one SDDMM wavefront: two operand buffers, the metadata pad, the output staging area
// (16 rows x kSddmmStageCap floats) and 256 bytes of junk slots for lanes that have nothing to stage.
static constexpr int kSddmmStageCap = 64;
#ifndef TCGNN_SDDMM_NBUF
#define TCGNN_SDDMM_NBUF(ks) ((ks) <= 2 ? 2 : 1)
#endif
// Operand buffers: two (gather of the next tile under the multiply of this one) up to D = 64; one beyond,
// where LDS would otherwise allow a single workgroup per CU (latency is then hidden by wavefront count only).
static constexpr int sddmm_nbuf(int ks) { return TCGNN_SDDMM_NBUF(ks); }
static constexpr int sddmm_wave_lds(int ks) { return sddmm_nbuf(ks) * (2 * ks * 1024) + kPadBytes + 16 * kSddmmStageCap * 4 + 256; }
// The multi-head form (tcgnn_sddmm_heads; HF = columns of a head, G = heads of a pass): one staging area PER HEAD, so the cap is the
// smallest a tile allows - a tile adds at most 32 results to a row - and the flush is decided from the tile's masks BEFORE it is
// staged (a row that could overflow flushes first) instead of after it with 32 slots kept free.  At most kSddmmMaxHeadsPerPass heads
// and 128 columns a pass: 2 x 4 KB or 8 KB of operand buffers + 4 x 2 KB of staging = 16.8 KB a wavefront, two four-wavefront
// workgroups per CU at the worst shapes (4 x 16, 4 x 32), three at 4 x 8 (DESIGN.md 4.11 has the table).
static constexpr int kSddmmHeadsStageCap = 32, kSddmmMaxHeadsPerPass = 4;
static constexpr int sddmm_heads_ks(int hf, int g) { return (hf * g + 31) / 32; }
static constexpr int sddmm_heads_wave_lds(int hf, int g) {
    return sddmm_nbuf(sddmm_heads_ks(hf, g)) * (2 * sddmm_heads_ks(hf, g) * 1024) + kPadBytes + g * 16 * kSddmmHeadsStageCap * 4 + 256;
}
// Launch geometry of sddmm_kernel and of its multi-head form.  The persistent walks (range-major, slice-synchronised) take one window per
// wavefront at a time; four wavefronts per SIMD up to 64 columns, three beyond - the multi-head form three at one K-step, else two.
static constexpr LaunchGeom sddmm_geom(int ks, int waves) { return {waves * 64, waves * sddmm_wave_lds(ks), ks <= 2 ? 4 : 3, 1}; }
static constexpr LaunchGeom sddmm_heads_geom(int hf, int g, int waves) { return {waves * 64, waves * sddmm_heads_wave_lds(hf, g), sddmm_heads_ks(hf, g) <= 1 ? 3 : 2, 1}; }
// (pinned: resident four-wavefront workgroups per CU at 1 .. 4 K-steps, and for every instantiated pass of 2 .. 4 heads - index g - 1)
static_assert(widths_give([](int ks) { return sddmm_geom(ks, 4).wgs_per_cu(); }, {4, 3, 3, 3}), "sddmm_kernel");
static_assert(widths_give([](int g) { return g < 2 ? 0 : sddmm_heads_geom(8, g, 4).wgs_per_cu(); }, {0, 3, 3, 3}), "sddmm_kernel, heads of 8 columns");
static_assert(widths_give([](int g) { return g < 2 ? 0 : sddmm_heads_geom(16, g, 4).wgs_per_cu(); }, {0, 3, 2, 2}), "sddmm_kernel, heads of 16 columns");
static_assert(widths_give([](int g) { return g < 2 ? 0 : sddmm_heads_geom(32, g, 4).wgs_per_cu(); }, {0, 2, 2, 2}), "sddmm_kernel, heads of 32 columns");
static_assert(widths_give([](int g) { return g < 2 ? 0 : sddmm_heads_geom(64, g, 4).wgs_per_cu(); }, {0, 2}), "sddmm_kernel, heads of 64 columns");

// KS = number of 32-wide k steps (D <= 32*KS <= 128).  The 16 window rows (MFMA A operand) stay in
// registers.  Neighbour rows are the B operand, which for X * X^T is contiguous per lane: lane
// (i, g) needs halves 32*ks + 8g .. +7 of neighbour row i.  Each lane DMAs exactly those 16 bytes
// (structured-buffer addressing: row id * pitch + offset formed by the hardware) into its own LDS
// slot and reads the slot back - LDS is a per-lane landing pad, trivially conflict-free - so the
// gather of the NEXT tile (both 16-column halves) is in flight while the current one is multiplied
// and scattered, without any VGPR holding a load in flight (see "memory pipeline discipline").
// TWO (tcgnn_sddmm2): the window rows come from a second image, a.xa16, scaled by its own header word; everything else is the same code
// HF > 0 (tcgnn_sddmm_heads, with TWO; reported as "sddmm_heads_kernel"): the KS K-steps are the G HF columns of one pass of G heads,
// HF columns each, and every head has its own accumulator, staging area and row of ef.  Lane (i, g) of K-step ks holds the pass's
// columns 32 ks + 8 g .. + 7, which belong to ONE head: a head's accumulator takes the K-steps its columns touch - HF = 64 two, HF = 32
// one; HF = 8 / 16: four / two heads share a K-step, which is then issued once per head with an A fragment whose lanes outside that
// head's column groups are zero (built once per window in load_a: the tile loop gains MFMA issues and the staging writes of G times
// the outputs, no other VALU work).  Gather, metadata DMA, LDS landing layout and the three walks are the single-head kernel's.
template <int KS, int WAVES, bool BLOCKED, bool TWO = false, int HF = 0, int G = 1>
__global__ __launch_bounds__(WAVES * 64, (HF > 0 ? sddmm_heads_geom(HF, G, WAVES) : sddmm_geom(KS, WAVES)).waves_per_simd) void sddmm_kernel(const SddmmArgs a) {
    static_assert(HF == 0 || (TWO && (HF == 8 || HF == 16 || HF == 32 || HF == 64) && G >= 1 && G <= kSddmmMaxHeadsPerPass && KS == sddmm_heads_ks(HF, G) && KS <= 4),
                  "a pass of the multi-head form: G heads of HF columns in KS K-steps");
    if constexpr (TWO) { if (sddmm2_wide(a.hdr_a, a.hdr)) return; }   // (sddmm2_csr_kernel, launched behind this kernel, does the work)
    else if (wide2_dense(a.hdr)) return;   // (range guard: the fp32 fallback launched behind this kernel does the work)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int BUF_BYTES = 2 * KS * 1024;               // both halves of one tile
    constexpr int WAVE_LDS = HF > 0 ? sddmm_heads_wave_lds(HF, G) : sddmm_wave_lds(KS);
    constexpr int CAP = HF > 0 ? kSddmmHeadsStageCap : kSddmmStageCap;   // staged outputs per row before a flush
    constexpr int KPH = HF > 32 ? HF / 32 : 1;             // HF > 0: K-steps a head's accumulator takes
    constexpr int NA = HF > 0 ? G * KPH : KS;              // A fragments a window keeps: one per K-step; HF > 0: one per (head, K-step of the head)
    constexpr int STG_HEAD = 16 * CAP * 4;                 // staging bytes of one head
    const int head0 = HF > 0 ? a.head0 + (int)blockIdx.y * G : 0;
    const int coloff = head0 * HF;                         // first column of this pass in both images (a multiple of 8)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, i = lane & 15;
    const int64_t stride = a.stride;
    const int kx = scale_exp_from_bits(a.hdr[kHdrMaxX]);
    // ef = acc * 2^(-2kx); one multiply unless 2kx leaves the fp32 exponent range (then two)
    bool two_step = kx > 63 || kx < -63;
    float inv_a = two_step ? pow2f(-kx) : pow2f(-2 * kx), inv_b = two_step ? pow2f(-kx) : 1.0f;
    if constexpr (TWO) {   // ef = acc * 2^-(ka + kx); with ka = kx exactly the factors above
        const int ka = scale_exp_from_bits(a.hdr_a[kHdrMaxX]);
        two_step = ka + kx > 126 || ka + kx < -126;
        inv_a = two_step ? pow2f(-ka) : pow2f(-(ka + kx));
        inv_b = two_step ? pow2f(-kx) : 1.0f;
    }
    const half8 hz = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t below[2] = {(1u << i) - 1u, (1u << (16 + i)) - 1u};   // condensed columns left of mine, per half

    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a.x16, (short)(a.stride * 2), a.Nc + 1, 0x00020000);
    const MetaSource meta(a.cols, a.mask, a.ebase, lane);
    const uint32_t ring = (uint32_t)(uintptr_t)((LDS_AS char*)(smem + wave * WAVE_LDS));
    const uint32_t pad = ring + sddmm_nbuf(KS) * BUF_BYTES;
    // a lane whose k slice lies past Dpad fetches slice 0 instead (valid memory) and is zeroed at use
    uint32_t boff[KS];
    bool bok[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) { bok[ks] = coloff + ks * 32 + 8 * g < a.Dpad; boff[ks] = (uint32_t)(coloff + (bok[ks] ? ks * 32 + 8 * g : 0)) * 2u; }
    // WL (KS = 2, rows of one 128-byte line; r03): whole-line gathers, as in agnn_kernel - instruction q takes the eight rows of tile
    // columns 8q .. 8q+7 (lane L: row slot L >> 3, the chunk that belongs at position L & 7) into block q, row-major; chunk c of row
    // slot rho lies at position c ^ 2 (rho >> 1), which spreads the sixteen lanes of every ds_read_b128 lane group of the operand
    // reads (row i of half sub = row slot i & 7 of block 2 sub + (i >> 3), chunk 4 ks + g) over the sixteen 16-byte bank slots.
    // KS = 4 (256-byte rows): four rows per instruction, eight instructions, tile column tau in row slot tau & 3 of block tau >> 2,
    // chunk c at position c ^ (4 (q & 3) + rho).  (KS = 3: the layout above, see agnn_kernel.)
    constexpr bool WL = KS == 2 || KS == 4;
    constexpr int RB = KS == 2 ? 128 : 256, RPI = 1024 / RB, NI = WL ? 32 / RPI : 2, CPR = RB / 16;
    constexpr int NIDR = NI;                                                                      // row ids this lane reads per tile
    auto wl_sw = [](uint32_t rho, uint32_t q) -> uint32_t {
        if constexpr (KS == 2) return 2u * (rho >> 1);
        else return 4u * (q & 3u) + rho;
    };
    uint32_t idaddr[NIDR];
    if constexpr (WL) {
#pragma unroll
        for (int q = 0; q < NI; ++q) idaddr[q] = pad + (uint32_t)(RPI * q + lane / CPR) * 4u;
    } else { idaddr[0] = pad + (uint32_t)i * 4u; idaddr[1] = pad + 64u + (uint32_t)i * 4u; }      // row ids of both halves
    [[maybe_unused]] uint32_t choff[WL ? NI : 1];                                                 // WL: byte offset of my chunk inside the rows instruction q fetches
    if constexpr (WL) {
#pragma unroll
        for (int q = 0; q < NI; ++q) {
            const uint32_t c = (uint32_t)(lane % CPR) ^ wl_sw((uint32_t)(lane / CPR), (uint32_t)q);
            choff[q] = (uint32_t)coloff * 2u + ((coloff + (int)(c * 8u) < a.Dpad) ? c * 16u : 0u);
        }
    }
    uint32_t qaddr[1 + 2 * KS];                                                                   // edge offsets, then my landing slots
    qaddr[0] = pad + 192u + 16u * (uint32_t)g;
#pragma unroll
    for (int k = 0; k < 2 * KS; ++k) {
        if constexpr (WL) {   // row i of half sub = tile column 16 sub + i
            const uint32_t sub = (uint32_t)(k / KS), ks = (uint32_t)(k % KS), tau = 16u * sub + (uint32_t)i, q = tau / RPI, rho = tau % RPI;
            qaddr[1 + k] = ring + q * 1024u + rho * (uint32_t)RB + (((4u * ks + (uint32_t)g) ^ wl_sw(rho, q)) * 16u);
        } else qaddr[1 + k] = ring + (uint32_t)k * 1024u + (uint32_t)lane * 16u;
    }
    const uint32_t m4addr = pad + 128u + 16u * (uint32_t)g;
    // Output staging.  PMC (profiles/r01): scattering every result with its own 4-byte store costs
    // 7.6e7 L2 write requests per launch on top of the 1.25e8 gather reads, and the kernel runs at the
    // L2 request-rate ceiling.  A wavefront walks CONSECUTIVE tiles, and a row's edges in consecutive
    // tiles are consecutive in ef, so results are staged per row in LDS and each row is flushed as one
    // contiguous store (about one store per tile instead of eight, ~10x fewer write requests).
    const uint32_t stg = pad + kPadBytes;
    const uint32_t junk = stg + (uint32_t)(HF > 0 ? G : 1) * STG_HEAD + (uint32_t)lane * 4u;
    const uint32_t stg_row[4] = {stg + (uint32_t)(4 * g + 0) * CAP * 4u, stg + (uint32_t)(4 * g + 1) * CAP * 4u,
                                 stg + (uint32_t)(4 * g + 2) * CAP * 4u, stg + (uint32_t)(4 * g + 3) * CAP * 4u};
    const uint32_t flush_base = stg + (uint32_t)lane * 4u;        // lane j reads the j-th staged result of every row

  // A operand of window w: row i, halves 32*ks + 8g .. +7 (rows past N read the zero sentinel row)
  // (HF > 0: fragment k KPH + j is head k's j-th K-step; where heads share a K-step, the lanes of the other heads' column groups are zero)
  auto load_a = [&](const int w, half8 (&af)[NA]) __attribute__((always_inline)) {
    int64_t arow = (int64_t)w * kWinRows + i;
    arow = arow < a.N ? arow + a.row_off : a.Nc;
    const _Float16* ap = (TWO ? a.xa16 : a.x16) + arow * stride + coloff + 8 * g;
    if constexpr (HF > 0) {
#pragma unroll
        for (int k = 0; k < G; ++k)
#pragma unroll
            for (int j = 0; j < KPH; ++j) {
                const int ks = (k * HF) / 32 + j;
                af[k * KPH + j] = ((32 * ks + 8 * g) / HF == k && coloff + ks * 32 + 8 * g < a.Dpad) ? *reinterpret_cast<const half8*>(ap + ks * 32) : hz;
            }
        return;
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) af[ks] = (ks * 32 + 8 * g < a.Dpad) ? *reinterpret_cast<const half8*>(ap + ks * 32) : hz;
  };
  // one run: CONSECUTIVE tiles t .. te-1 of window w (step must be 1: the staging relies on it); af = load_a(w)
  auto run_a = [&](const int w, const half8 (&af)[NA], int64_t t, const int64_t te, const int64_t step) __attribute__((always_inline)) {
    if (t >= te) return;
    // edges of this window live in ef[e_w0 .. ): 32-bit offsets from a wave-uniform base
    const int64_t wrow = (int64_t)w * kWinRows;
    const int64_t e_w0 = a.rowptr[wrow < a.N ? wrow : a.N];
    char* const ef_w = reinterpret_cast<char*>(a.ef + e_w0);
    bool flush_pending = false;
    uint32_t cnt[4] = {0u, 0u, 0u, 0u};                          // staged results of rows 4g .. 4g+3
    uint32_t rstart[4] = {~0u, ~0u, ~0u, ~0u};                   // window-relative ef position of each row's first staged result
    auto flush = [&]() {
        uint32_t vals[16];
        if constexpr (HF > 0) {   // every head's runs: the same counts and positions, head k's staging area into its row of ef
#pragma unroll
            for (int k = 0; k < G; ++k) {
                lds_rows_block8<CAP * 4, 0>(flush_base + (uint32_t)(k * STG_HEAD), vals);
                lds_rows_block8<CAP * 4, 8>(flush_base + (uint32_t)(k * STG_HEAD), vals + 8);
                char* const ef_h = ef_w + (int64_t)(head0 + k) * a.E * 4;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint32_t c_r = (uint32_t)__builtin_amdgcn_readlane((int)cnt[r & 3], 16 * (r >> 2));
                    const uint32_t s_r = (uint32_t)__builtin_amdgcn_readlane((int)rstart[r & 3], 16 * (r >> 2));
                    if ((uint32_t)lane < c_r) *reinterpret_cast<uint32_t*>(ef_h + ((s_r + (uint32_t)lane) << 2)) = vals[r];
                }
            }
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) { cnt[ii] = 0u; rstart[ii] = ~0u; }
            return;
        }
        lds_rows_block8<CAP * 4, 0>(flush_base, vals);
        lds_rows_block8<CAP * 4, 8>(flush_base, vals + 8);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t c_r = (uint32_t)__builtin_amdgcn_readlane((int)cnt[r & 3], 16 * (r >> 2));
            const uint32_t s_r = (uint32_t)__builtin_amdgcn_readlane((int)rstart[r & 3], 16 * (r >> 2));
            if ((uint32_t)lane < c_r) *reinterpret_cast<uint32_t*>(ef_w + ((s_r + (uint32_t)lane) << 2)) = vals[r];
        }
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) { cnt[ii] = 0u; rstart[ii] = ~0u; }
    };

    auto dma_b = [&](const uint32_t* cid, int bufbase) {
        if constexpr (WL) {
            if (a.big) {
                const char* const xb = reinterpret_cast<const char*>(a.x16);
#pragma unroll
                for (int q = 0; q < NI; ++q)
                    __builtin_amdgcn_global_load_lds((GLB_AS const void*)(xb + (uint64_t)cid[q] * (uint64_t)(stride * 2) + choff[q]),
                                                     (LDS_AS void*)(uintptr_t)(ring + bufbase + q * 1024), 16, 0, 0);
                return;
            }
#pragma unroll
            for (int q = 0; q < NI; ++q)
                __builtin_amdgcn_struct_ptr_buffer_load_lds(xrsrc, (LDS_AS void*)(uintptr_t)(ring + bufbase + q * 1024), 16, (int)cid[q], (int)choff[q], 0, 0, 0);
            return;
        }
        if (a.big) {
            const char* const xb = reinterpret_cast<const char*>(a.x16);
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
                    __builtin_amdgcn_global_load_lds((GLB_AS const void*)(xb + (uint64_t)cid[sub] * (uint64_t)(stride * 2) + boff[ks]),
                                                     (LDS_AS void*)(uintptr_t)(ring + bufbase + (sub * KS + ks) * 1024), 16, 0, 0);
            return;
        }
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
                __builtin_amdgcn_struct_ptr_buffer_load_lds(xrsrc, (LDS_AS void*)(uintptr_t)(ring + bufbase + (sub * KS + ks) * 1024), 16,
                                                            (int)cid[sub], (int)boff[ks], 0, 0, 0);
    };
    struct Cur { uintx4 m4, eb4; };
    auto stage = [&](auto BUFC, Cur& cur, int64_t& tcur, int64_t& tn) -> bool {
        constexpr int BUF = decltype(BUFC)::value;
        wait_vm0();
        uint32_t cid[NIDR];
        uintx4 m4n, q[1 + 2 * KS];
        lds_ids_block<NIDR>(idaddr, cid, m4addr, m4n);             // ids + masks of the next tile
        constexpr int NB = sddmm_nbuf(KS);
        lds_q_block<1 + 2 * KS, (NB == 2 ? BUF : 0) * BUF_BYTES>(qaddr, q);   // its edge offsets, and this tile's operands
        const bool more = tn < te;
        const int64_t tnn = tn + step;
        if (more) {
            dma_b(cid, (NB == 2 ? (BUF ^ 1) : 0) * BUF_BYTES);   // (single buffer: its reads above have completed)
            if (tnn < te) meta.dma(tnn, pad);
        }
        // A flush decided at the end of the previous tile is issued HERE, right behind the gather: its stores then have as
        // long to complete as the gather before the next wait (issued after the multiply they held that wait up).
        if (flush_pending) { flush(); flush_pending = false; }
        // ---- tile tcur
        const uint32_t mm[4] = {cur.m4[0], cur.m4[1], cur.m4[2], cur.m4[3]};
        if constexpr (HF > 0) {   // (CAP = 32: the masks say before the multiply whether every row has room for this tile)
            const uint32_t fill = max(max(cnt[0] + (uint32_t)__popc(mm[0]), cnt[1] + (uint32_t)__popc(mm[1])), max(cnt[2] + (uint32_t)__popc(mm[2]), cnt[3] + (uint32_t)__popc(mm[3])));
            if (__any(fill > (uint32_t)CAP)) flush();
        }
        const uint32_t e0 = (uint32_t)e_w0;   // window-relative edge positions (a window holds far fewer than 2^32 edges)
        const uint32_t rbase[4] = {cur.eb4[0] - e0, cur.eb4[1] - e0, cur.eb4[2] - e0, cur.eb4[3] - e0};
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const uint32_t anyrow = ((mm[0] | mm[1] | mm[2] | mm[3]) >> (16 * sub)) & 0xffffu;
            if constexpr (HF > 0) {
              if (__any(anyrow != 0u)) {
                floatx4 acch[G];
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    acch[k] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int j = 0; j < KPH; ++j)
                        acch[k] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[k * KPH + j], __builtin_bit_cast(half8, q[1 + sub * KS + (k * HF) / 32 + j]), acch[k], 0, 0, 0);
                }
                const int bit = 16 * sub + i;
#pragma unroll
                for (int ii = 0; ii < 4; ++ii) {
                    const bool on = (mm[ii] >> bit) & 1u;
                    const uint32_t slot = on ? stg_row[ii] + ((cnt[ii] + (uint32_t)__popc(mm[ii] & below[sub])) << 2) : junk;
#pragma unroll
                    for (int k = 0; k < G; ++k) {
                        float v = acch[k][ii] * inv_a;
                        if (two_step) v *= inv_b;
                        lds_write_b32(on ? slot + (uint32_t)(k * STG_HEAD) : junk, v);
                    }
                }
              }
            } else
            if (__any(anyrow != 0u)) {              // skip a 16-column half no edge lands in
                floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    // (a lane whose k slice lies past Dpad holds zeros in af: whatever it fetched for B is multiplied away)
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[ks], __builtin_bit_cast(half8, q[1 + sub * KS + ks]), acc, 0, 0, 0);
                }
                // C[row 4g+ii][col i] -> staged at the row's next free slot if the edge exists
                const int bit = 16 * sub + i;
#pragma unroll
                for (int ii = 0; ii < 4; ++ii) {
                    const bool on = (mm[ii] >> bit) & 1u;
                    const uint32_t pos = cnt[ii] + (uint32_t)__popc(mm[ii] & below[sub]);
                    float v = acc[ii] * inv_a;
                    if (two_step) v *= inv_b;
                    lds_write_b32(on ? stg_row[ii] + (pos << 2) : junk, v);
                }
            }
        }
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            if (rstart[ii] == ~0u && mm[ii] != 0u) rstart[ii] = rbase[ii];
            cnt[ii] += (uint32_t)__popc(mm[ii]);
        }
        // a tile adds at most 32 results to a row: flush while every row still has room for one more tile
        const uint32_t fullest = max(max(cnt[0], cnt[1]), max(cnt[2], cnt[3]));
        if (!more) flush();
        else if constexpr (HF == 0) flush_pending = __any(fullest > (uint32_t)(CAP - 32));
        cur.m4 = m4n;
        cur.eb4 = q[0];
        tcur = tn;
        tn = tnn;
        return more;
    };

    // prologue: metadata of the first tile, its operands, metadata of the second
    meta.dma(t, pad);
    wait_vm0();
    Cur cur;
    {
        uint32_t cid[NIDR];
        uintx4 e4[1];
        lds_ids_block<NIDR>(idaddr, cid, m4addr, cur.m4);
        lds_q_block<1, 0>(qaddr, e4);
        cur.eb4 = e4[0];
        dma_b(cid, 0);
    }
    int64_t tn = t + step;
    if (tn < te) meta.dma(tn, pad);
    for (;;) {
        if (!stage(std::integral_constant<int, 0>{}, cur, t, tn)) break;
        if (!stage(std::integral_constant<int, 1>{}, cur, t, tn)) break;
    }
    wait_vm0();   // the run's last stores are retired before the next run reuses pad and slots
  };
  auto run = [&](const int w, int64_t t, const int64_t te, const int64_t step) __attribute__((always_inline)) {
    if (t >= te) return;
    half8 af[NA];
    load_a(w, af);
    run_a(w, af, t, te, step);
  };

    if constexpr (BLOCKED) {
        if (a.use_sync) {
            // slice-synchronised walk (r06): the wavefronts of XCD x take (phase, window) items of ONE slice of that XCD's share, phase-major.
            // No state crosses a phase, so a wavefront simply runs every nwv-th window of the slice in each phase; the windows of a slice are
            // alike, the launch started every wavefront together, and the phase's rows (~2 MB) are what the XCD's L2 holds meanwhile.
            int x, w_lo, w_hi, nph;
            sync_slice_of(a.sync, x, w_lo, w_hi, nph);
            const int nwv = (int)(gridDim.x / (unsigned)kXcds) * WAVES, wid = (int)(blockIdx.x / (unsigned)kXcds) * WAVES + wave;
            const int ts = a.sync.kmax + 1;
            // (a wavefront keeps ONE window through all phases, its rows in registers, then takes the next: reloading the A operand per
            //  (window, phase) run cost 4 KB of mostly missing lines and a round trip in front of each of the ~5-tile runs - 4.4 GB per call on
            //  the products shape; every trip walks the phases again, the wavefronts still together)
            for (int w = w_lo + wid; w < w_hi; w += nwv) {
                half8 af[NA];
                load_a(w, af);
                const uint32_t* Tw = a.sync.T + (int64_t)w * ts;
                const int64_t tb = a.wb_ptr[w];
                for (int r = 0; r < nph; ++r) {
                    const int k0 = r * a.sync.m < a.sync.kmax ? r * a.sync.m : a.sync.kmax, k1 = (r + 1) * a.sync.m < a.sync.kmax ? (r + 1) * a.sync.m : a.sync.kmax;
                    run_a(w, af, tb + Tw[k0], tb + Tw[k1], 1);
                }
            }
            return;
        }
        // persistent wavefronts take (column range, window) items in range-major order: at any moment
        // the whole chip gathers from one or two ranges of X16, which stay L2-resident
        if (a.xcd) {
            // XCD affinity (r03, after the whole-line gathers made an L2 hit worth twice a miss): the workgroups of XCD x gather from
            // the ranges x, x + 8, ... only, one after the other - that XCD's L2 is asked for an eighth of the image, a range or two of
            // it at a time, instead of every range every other XCD is walking as well.  Every edge lies in exactly one range, so
            // nothing is added up afterwards and the scores are bit for bit those of the other walks.
            const int x = (int)(blockIdx.x % (unsigned)kXcds);
            const int64_t items_x = (int64_t)(a.nranges / kXcds) * a.nw, lstride = (int64_t)(gridDim.x / (unsigned)kXcds) * WAVES;
            for (int64_t q = (int64_t)(blockIdx.x / (unsigned)kXcds) * WAVES + wave; q < items_x; q += lstride) {
                const int rr = (int)(q / a.nw), r = x + kXcds * rr;
                const int wq = (int)(q - (int64_t)rr * a.nw);
                const int w = a.ident ? wq : __builtin_amdgcn_readfirstlane(a.order[wq]);
                const int64_t tb = a.wb_ptr[w];
                const uint32_t* bp = a.bptr + (int64_t)w * (a.nbuckets + 1);
                run(w, tb + bp[r * a.gsel], tb + bp[(r + 1) * a.gsel], 1);
            }
            return;
        }
        const int64_t items = (int64_t)a.nranges * a.nw;
        for (int64_t q = (int64_t)blockIdx.x * WAVES + wave; q < items; q += (int64_t)gridDim.x * WAVES) {
            const int r = (int)(q / a.nw);
            const int wq = (int)(q - (int64_t)r * a.nw);
            const int w = a.ident ? wq : __builtin_amdgcn_readfirstlane(a.order[wq]);
            const int64_t tb = a.wb_ptr[w];
            const uint32_t* bp = a.bptr + (int64_t)w * (a.nbuckets + 1);
            run(w, tb + bp[r * a.gsel], tb + bp[(r + 1) * a.gsel], 1);
        }
    } else {
        const int w = a.order[blockIdx.x];
        const int64_t tb = a.wb_ptr[w], te = a.wb_ptr[w + 1];
        const int64_t chunk = (te - tb + WAVES - 1) / WAVES;       // contiguous share of this wavefront
        const int64_t t0 = tb + wave * chunk;
        run(w, t0, t0 + chunk < te ? t0 + chunk : te, 1);
    }
}

// Run-time-K variant for D > 128: window rows are re-read per tile (L1-resident), ordinary loads.
template <int WAVES, bool TWO = false>
__global__ __launch_bounds__(WAVES * 64) void sddmm_wide_kernel(const SddmmArgs a) {
    if constexpr (TWO) { if (sddmm2_wide(a.hdr_a, a.hdr)) return; }
    else if (wide2_dense(a.hdr)) return;   // (range guard: the fp32 fallback launched behind this kernel does the work)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, i = lane & 15;
    const int w = a.order[blockIdx.x];
    const int64_t tb = a.wb_ptr[w], te = a.wb_ptr[w + 1];
    const int64_t stride = a.stride;
    const float inv = pow2f(-scale_exp_from_bits(a.hdr[kHdrMaxX]));
    const float inv_w = TWO ? pow2f(-scale_exp_from_bits(a.hdr_a[kHdrMaxX])) : inv;   // (the window operand's scale)
    const int ksteps = (a.Dpad + 31) >> 5;
    const half8 hz = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t arow = (int64_t)w * kWinRows + i;
    arow = arow < a.N ? arow + a.row_off : a.Nc;
    const _Float16* ap = (TWO ? a.xa16 : a.x16) + arow * stride + 8 * g;
    for (int64_t t = tb + wave; t < te; t += WAVES) {
        const uint4 m4 = *reinterpret_cast<const uint4*>(a.mask + t * kWinRows + 4 * g);
        const int4 eb4 = *reinterpret_cast<const int4*>(a.ebase + t * kWinRows + 4 * g);
        const uint32_t mm[4] = {m4.x, m4.y, m4.z, m4.w};
        const int ee[4] = {eb4.x, eb4.y, eb4.z, eb4.w};
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const uint32_t anyrow = ((m4.x | m4.y | m4.z | m4.w) >> (16 * sub)) & 0xffffu;
            if (!__any(anyrow != 0u)) continue;
            const int cid = a.cols[t * kWbCols + 16 * sub + i];
            const _Float16* bp = a.x16 + (int64_t)cid * stride + 8 * g;
            floatx4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int ks = 0; ks < ksteps; ++ks) {
                const bool ok = ks * 32 + 8 * g < a.Dpad;
                const half8 av = ok ? *reinterpret_cast<const half8*>(ap + ks * 32) : hz;
                const half8 bf = ok ? *reinterpret_cast<const half8*>(bp + ks * 32) : hz;
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bf, acc, 0, 0, 0);
            }
            const int bit = 16 * sub + i;
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) {
                if ((mm[ii] >> bit) & 1u) {
                    const int64_t e = (int64_t)ee[ii] + __popc(mm[ii] & ((1u << bit) - 1u));
                    a.ef[e] = acc[ii] * inv * inv_w;
                }
            }
        }
    }
}

// tcgnn_sddmm2 in plain fp32, CSR order, operands rounded like the reference's - sddmm_csr_kernel with two matrices (the same sums in
// the same order: X = Z gives its scores bit for bit).  The path of non-canonical plans (hx == nullptr) and the range guard's way
// through a wide operand: launched behind the MFMA kernel, it returns at once unless sddmm2_wide holds.  A wavefront per row.
__global__ __launch_bounds__(256) void sddmm2_csr_kernel(const uint32_t* __restrict__ hx, const uint32_t* __restrict__ hz, const int32_t* __restrict__ rowptr,
                                                         const int32_t* __restrict__ col, const float* __restrict__ X, const float* __restrict__ Z, float* ef,
                                                         int32_t N, int32_t D, int32_t row_off) {
    if (hx && !sddmm2_wide(hx, hz)) return;
    const int lane = threadIdx.x & 63;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < N; row += (int64_t)gridDim.x * 4) {
        const float* xr = X + (row + row_off) * D;
        for (int64_t e = rowptr[row]; e < rowptr[row + 1]; ++e) {
            const float* xc = Z + (int64_t)col[e] * D;
            float s = 0.f;
            for (int d = lane; d < D; d += 64) s += round_rna10(xr[d]) * round_rna10(xc[d]);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
            if (lane == 0) ef[e] = s;
        }
    }
}

// tcgnn_sddmm_heads in plain fp32: sddmm2_csr_kernel's body per head - head h reads columns h F .. of X and Z (row stride ld = H F)
// and writes ef + h E, the same sums in the same order as the single-head kernel on that head's columns.  ONE launch for all heads
// (heads from blockIdx.y in steps of grid.y, rows from blockIdx.x in steps of grid.x: any H and N under a capped grid): the path of
// non-canonical plans and of fewer than four edges (hx == nullptr), and the range guard's way behind the MFMA kernels of the fused
// and of the head-by-head route (returns at once unless sddmm2_wide holds on the two headers, which decide for the whole call).
__global__ __launch_bounds__(256) void sddmm_heads_csr_kernel(const uint32_t* __restrict__ hx, const uint32_t* __restrict__ hz, const int32_t* __restrict__ rowptr,
                                                              const int32_t* __restrict__ col, const float* __restrict__ X, const float* __restrict__ Z, float* ef,
                                                              int32_t N, int32_t H, int32_t F, int64_t ld, int64_t E, int32_t row_off) {
    if (hx && !sddmm2_wide(hx, hz)) return;
    const int lane = threadIdx.x & 63;
    for (int64_t h = blockIdx.y; h < H; h += gridDim.y) {
        const float* const Xh = X + h * F;
        const float* const Zh = Z + h * F;
        float* const efh = ef + h * E;
        for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < N; row += (int64_t)gridDim.x * 4) {
            const float* xr = Xh + (row + row_off) * ld;
            for (int64_t e = rowptr[row]; e < rowptr[row + 1]; ++e) {
                const float* xc = Zh + (int64_t)col[e] * ld;
                float s = 0.f;
                for (int d = lane; d < F; d += 64) s += round_rna10(xr[d]) * round_rna10(xc[d]);
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
                if (lane == 0) efh[e] = s;
            }
        }
    }
}

// (TWO: tcgnn_sddmm2's instantiations, the window operand from its own image.  Beyond 128 columns - ks > 4 - only sddmm_wide_kernel exists)
template <int WAVES, bool BLOCKED, bool TWO>
static hipError_t launch_sddmm_two(int ks, const SddmmArgs& args, int nwg, hipStream_t stream) {
    const dim3 grid((unsigned)nwg);
    if (ks > 4) return launch_kernel<sddmm_wide_kernel<WAVES, TWO>>(grid, LaunchGeom{WAVES * 64, 0, 0, 0}, stream, args);
    return with_width<4>(ks, [&](auto KS) { return launch_kernel<sddmm_kernel<KS, WAVES, BLOCKED, TWO>>(grid, sddmm_geom(KS, WAVES), stream, args); });
}
template <int WAVES, bool BLOCKED>
static hipError_t launch_sddmm_ks(int ks, const SddmmArgs& args, int nwg, hipStream_t stream) {
    return args.xa16 ? launch_sddmm_two<WAVES, BLOCKED, true>(ks, args, nwg, stream) : launch_sddmm_two<WAVES, BLOCKED, false>(ks, args, nwg, stream);
}

// tcgnn_sddmm_heads: npass passes (grid.y) of g heads of hf columns each, from args.head0 on.  The instantiated (hf, g): every pass
// sddmm_heads_passes forms - hf = 8, 16, 32 with 2, 3 or 4 heads, hf = 64 with 2
template <int WAVES, bool BLOCKED>
static hipError_t launch_sddmm_heads(int hf, int g, const SddmmArgs& args, int nwg, int npass, hipStream_t stream) {
    const dim3 grid((unsigned)nwg, (unsigned)npass);
#define TCGNN_SDDMM_HEADS_CASE(f, n) \
    if (hf == f && g == n) return launch_kernel<sddmm_kernel<sddmm_heads_ks(f, n), WAVES, BLOCKED, true, f, n>>(grid, sddmm_heads_geom(f, n, WAVES), stream, args);
    TCGNN_SDDMM_HEADS_CASE(8, 2) TCGNN_SDDMM_HEADS_CASE(8, 3) TCGNN_SDDMM_HEADS_CASE(8, 4)
    TCGNN_SDDMM_HEADS_CASE(16, 2) TCGNN_SDDMM_HEADS_CASE(16, 3) TCGNN_SDDMM_HEADS_CASE(16, 4)
    TCGNN_SDDMM_HEADS_CASE(32, 2) TCGNN_SDDMM_HEADS_CASE(32, 3) TCGNN_SDDMM_HEADS_CASE(32, 4)
    TCGNN_SDDMM_HEADS_CASE(64, 2)
#undef TCGNN_SDDMM_HEADS_CASE
    return hipErrorInvalidValue;
}
