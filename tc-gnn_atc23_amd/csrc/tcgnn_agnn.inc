// tcgnn_agnn.inc - the fused AGNN pair (agnn_kernel forward / backward, the slice sum, the d_w reduction).  Included by tcgnn_device.hip.
// ------------------------------------------------------------------------------------------
// Fused AGNN products: one gather of a tile's 32 neighbour rows feeds BOTH the edge scores
// (SDDMM) and the edge-weighted aggregation (SpMM), which the AGNN layer always wants together.
//
// Per tile:   S^T = Xc * Xw^T   (MFMA #1, once per half: 16 tile columns as rows m, the 16 window rows as
//             columns n, K = D).  Row m of half `sub` is tile column 8(m>>2) + 4sub + (m&3), so lane (g, i)
//             ends up holding, for window row i, the scores of tile columns 8g .. 8g+7 - exactly an A
//             fragment of MFMA #2 (k slot j <-> tile column 8g + j), and row i's edges inside those eight
//             columns are ONE run of ef.  No data moves between lanes:
//             Y  += att * Xc    (MFMA #2)
// The gathered rows land lane-linear in LDS (lane (g, i) DMAs halves 32ks + 8g.. of row m = i of half
// sub to slot lane*16 of block (sub, ks)); MFMA #1 reads each lane's own slot back, MFMA #2 reads the
// same bytes through ds_read_b64_tr_b16.  One buffer is
// enough: every LDS read of tile t completes before the gather of tile t+1 is issued, and that
// gather is in flight while tile t is multiplied.
//   forward  (BWD = false): ef = scores (staged per row, flushed as contiguous runs, as in
//            sddmm_kernel), att = fl32(w * ef), max |ef| recorded for the backward call's scale.
//   backward (BWD = true):  att = fl32(w * ef_saved) (edge values DMA'd one tile ahead),
//            scores of dY are only reduced against the column ids: sum_e s[e] * (float)col(e).
// ------------------------------------------------------------------------------------------
struct AgnnArgs {
    const int64_t* wb_ptr;
    const int32_t* order;
    const int32_t* cols;
    const uint32_t* mask;
    const int32_t* ebase;
    const _Float16* x16;
    const uint32_t* hdr;
    const float* w;            // attention weight, device scalar
    float* ef;                 // forward: out [E]; backward: the saved scores (read only)
    uint32_t* ef_absmax;       // bit pattern of max |ef|: forward accumulates, backward reads
    float* y;                  // [N, D]
    double* partial;           // backward: one slot per workgroup
    int32_t N, Nc, row_off, Dpad, D, stride;
    int64_t E;
    const int32_t* rowptr;
    const uint32_t* bptr;      // range-major walk (MAXW > 0): per-window tile offsets of the column buckets
    int32_t nbuckets, gsel, nranges, nw, ngroups;
    int32_t big;               // fp16 image >= 4 GB: 64-bit lane addresses instead of the buffer descriptor
    int32_t nslices;           // > 0 (MAXW = 0 only): the XCD-sliced walk, see agnn_kernel
    int32_t valonly;           // backward kernel as an edge-valued SpMM (tcgnn_spmm_val on the sliced walk): Y = sum ef[e] X[col(e)], no scores, w = 1
    int32_t* rowka;            // [N] per-row power-of-two exponent of the edge weights' fp16 image: forward writes, backward reads (nullptr: values only - one scale)
    int32_t rot;               // XCD-sliced walk (r06): windows in their OWN order, the XCD of slice s starting s eighths into the graph.  With `order`
                               // (XCD-contiguous: position q holds a window of eighth q % 8) the four wavefronts of a workgroup belong to four different
                               // eighths, and on a graph with communities the one whose community lies in the workgroup's slice carries 3x the tiles of the
                               // other three - every other workgroup waits for one wavefront.  In the graph's own order the four windows are neighbours
                               // (heavy or light together), and the rotation makes every XCD meet its own communities at the same time
    int32_t use_sync;          // MAXW > 0: the slice-synchronised range walk (tcgnn_sync_walk.inc) - this launch covers slice `sync.round` of every XCD's share
    SyncArgs sync;
};

static constexpr int agnn_wave_lds(int ks, bool bwd) {
    return 2 * ks * 1024 + kPadBytes + (bwd ? 2048 : 16 * kSddmmStageCap * 4 + 256);   // backward: two 1 KB edge-value blocks
}

// MAXW = 0: one workgroup per window, each wavefront a contiguous quarter of its tiles.
// MAXW > 0: persistent wavefronts that own MAXW windows (accumulators in registers) and walk the column
//           ranges in step, as spmm_blocked_kernel does, so the gathered rows stay L2-resident.
static constexpr int kAgnnMaxW = 2;   // windows owned by a wavefront of the range-major fused kernel
// (the backward pass of the range-major walk beyond 96 columns - taken on request only, tcgnn_set_spmm_mode(2) - needs more than the 256
//  registers two wavefronts per SIMD leave once the per-row exponents are live: one wavefront per SIMD there)
static constexpr LaunchGeom agnn_geom(int nt, int waves, bool bwd, int maxw) {
    return {waves * 64, waves * agnn_wave_lds((nt + 1) / 2, bwd), nt <= 4 ? 3 : ((bwd && maxw > 1 && nt > 6) ? 1 : 2), maxw};
}
// EXCEPTION kept from before the geometry was stated once: a forced range-major backward pass beyond 96 columns sizes its persistent
// grid for TWO workgroups per CU although its launch bound lets one be resident (material for a performance issue, not measured)
static constexpr int agnn_range_major_wgs_per_cu(int nt, bool bwd) {
    return (bwd && nt > 6) ? 2 : agnn_geom(nt, 4, bwd, kAgnnMaxW).wgs_per_cu();
}
// (pinned: resident four-wavefront workgroups per CU at 1 .. 8 tiles of width, as the persistent grids are sized)
static_assert(widths_give([](int nt) { return agnn_range_major_wgs_per_cu(nt, false); }, {3, 3, 3, 3, 2, 2, 2, 2}), "agnn_kernel range-major, forward");
static_assert(widths_give([](int nt) { return agnn_range_major_wgs_per_cu(nt, true); }, {3, 3, 3, 3, 2, 2, 2, 2}), "agnn_kernel range-major, backward");
static_assert(widths_give([](int nt) { return agnn_geom(nt, 4, false, kAgnnMaxW).wgs_per_cu(); }, {3, 3, 3, 3, 2, 2, 2, 2}), "agnn_kernel slice-synchronised, forward");
static_assert(widths_give([](int nt) { return agnn_geom(nt, 4, true, nt > 6 ? 1 : kAgnnMaxW).wgs_per_cu(); }, {3, 3, 3, 3, 2, 2, 2, 2}), "agnn_kernel slice-synchronised, backward");
template <int NT, int WAVES, bool BWD, int MAXW>
__global__ __launch_bounds__(agnn_geom(NT, WAVES, BWD, MAXW).threads, agnn_geom(NT, WAVES, BWD, MAXW).waves_per_simd) void agnn_kernel(const AgnnArgs a) {
    const bool valonly = BWD && a.valonly != 0;   // (kernel-uniform)
    if (valonly ? range_is_wide_val(a.hdr) : wide2_dense(a.hdr)) return;   // (range guard: the fp32 fallback launched behind this kernel does the work; a few dirty rows: wide_patch_kernel)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int KS = (NT + 1) / 2;
    constexpr int WAVE_LDS = agnn_wave_lds(KS, BWD);
    constexpr int CAP = kSddmmStageCap;
    constexpr int NQ = 2 * KS;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, i = lane & 15;
    const int64_t stride = a.stride;
    const int kx = scale_exp_from_bits(a.hdr[kHdrMaxX]);
    const bool two_step = kx > 63 || kx < -63;                     // score = acc * 2^(-2kx), in two factors if needed
    const float inv_a = two_step ? pow2f(-kx) : pow2f(-2 * kx), inv_b = two_step ? pow2f(-kx) : 1.0f;
    const float wv = a.w ? a.w[0] : 1.0f;
    // power-of-two scale of the edge weights att = w * ef.  forward: |ef| <= Dpad * max|x|^2 (no pass over E);
    // backward: the recorded max |ef|.  Rounding to a 10-bit mantissa does not depend on the scale.
    float att_bound;
    if constexpr (BWD) att_bound = fabsf(wv) * __uint_as_float(a.ef_absmax[0]);
    else { const float xm = __uint_as_float(a.hdr[kHdrMaxX]); att_bound = fabsf(wv) * (float)a.Dpad * xm * xm; }
    const int ka = scale_exp_from_bits(__float_as_uint(att_bound));
    // r05: ONE scale per ROW of A.  The edge weights of a power-law graph under the reference's unscaled weights spread over 2^30 and
    // more ACROSS the matrix (hub x hub scores against leaf x leaf), and with one scale for all of them the small rows' weights fell
    // below fp16's normal range: their aggregate came out wrong by its whole value (tests: R-MAT at scale 0.05).  Inside one row
    // att[i][c] = w <x_i, x_c> only varies with the neighbours' magnitudes, so row i gets its own power of two from the bound
    // |att[i][.]| <= |w| Dpad max|x_i| max|X| - the forward pass stores the exponent (rowka, behind the ef_absmax word), the
    // backward pass reads it - and the epilogue undoes it per row.  Rounding to a 10-bit mantissa does not depend on the scale.
    // (a row whose neighbours' magnitudes spread over more than ~2^20 still loses bits of its smallest weights: documented)
    auto row_ka = [&](const int w) -> int {
        if (valonly || !a.rowka) return ka;
        int64_t row = (int64_t)w * kWinRows + i;
        if constexpr (BWD) return row < a.N ? a.rowka[row] : 0;
        const int64_t arow = row < a.N ? row + a.row_off : a.Nc;
        const _Float16* ap = a.x16 + arow * stride;
        float m = 0.f;
        for (int d = 8 * g; d < a.Dpad; d += 32) {
            const half8 v = *reinterpret_cast<const half8*>(ap + d);
#pragma unroll
            for (int q = 0; q < 8; ++q) m = fmaxf(m, fabsf((float)v[q]));
        }
        m = fmaxf(m, __shfl_xor(m, 16)); m = fmaxf(m, __shfl_xor(m, 32));
        const float xm = __uint_as_float(a.hdr[kHdrMaxX]);
        const float bound = fabsf(wv) * (float)a.Dpad * xm * (m * pow2f(-kx));
        const int k = scale_exp_from_bits(__float_as_uint(bound));
        if (g == 0 && row < a.N) a.rowka[row] = k;
        return k;
    };
    const half8 hz = {0, 0, 0, 0, 0, 0, 0, 0};

    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a.x16, (short)(a.stride * 2), a.Nc + 1, 0x00020000);
    const MetaSource meta(a.cols, a.mask, a.ebase, lane);
    const uint32_t ring = (uint32_t)(uintptr_t)((LDS_AS char*)(smem + wave * WAVE_LDS));
    const uint32_t pad = ring + 2 * KS * 1024;
    const uint32_t aux = pad + kPadBytes;                          // forward: output staging; backward: edge-value pad
    uint32_t boff[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) boff[ks] = (ks * 32 + 8 * g < a.Dpad) ? (uint32_t)(ks * 32 + 8 * g) * 2u : 0u;
    // pad: cols[32] | mask[16] | ebase[16]; this lane: ids of the tile columns it gathers for the two halves
    // (row m = i of half sub is tile column 8(i>>2) + 4sub + (i&3)), mask and edge offset of ROW i
    //
    // WL (KS = 2, rows of one 128-byte line; r03): WHOLE-LINE gathers.  The layout above makes an instruction take 64 bytes of each
    // of sixteen rows, so every line is asked for twice, and tools/gather_bench.hip measures what that costs once the rows come out
    // of L2: 9.2 TB/s at any depth against 14-18 TB/s for instructions that take eight whole rows.  Here instruction q takes the
    // rows of tile columns 8q .. 8q+7 - lane L the 16-byte chunk of row slot rho = L >> 3 that belongs at position p = L & 7 - into
    // block q, row-major.  Chunk c of row slot rho lies at position c ^ sw(rho, q), sw = 4 ((rho >> 1) & 1) + sigma(q),
    // sigma = (0, 2, 3, 1): with it the sixteen lanes of every ds_read_b128 lane group of MFMA #1's operand reads (row i, chunk
    // 4 ks + g) fall into the sixteen 16-byte bank slots, and so do the eight rows x two chunks a 32-lane group of the transposed
    // reads of MFMA #2 addresses.  All of it is per-lane constants: the tile loop issues the same instructions as before, plus two
    // more row ids read from the pad.
    // KS = 4 (rows of two lines, D = 97 .. 128): the same with four 256-byte rows per instruction, eight instructions, tile column tau in
    // row slot tau & 3 of block tau >> 2, sw = 8 ((q >> 1) & 1) + 2 rho.  (KS = 3 keeps the layout above: its 192-byte rows are
    // gathered at a 256-byte pitch, which a row-major image of the tile would have to be sized for.)
    constexpr bool WL = KS == 2 || KS == 4;
    constexpr int RB = KS == 2 ? 128 : 256, RPI = 1024 / RB, NI = WL ? 32 / RPI : 2, CPR = RB / 16;   // row bytes, rows per instruction, instructions, chunks per row
    constexpr int NV = WL ? NI + 2 : 4;                              // words read from the pad per tile: row ids, mask, edge offset
    auto wl_sw = [](uint32_t rho, uint32_t q) -> uint32_t {
        if constexpr (KS == 2) return 4u * ((rho >> 1) & 1u) + ((0x1320u >> (4u * q)) & 3u);
        else return 8u * ((q >> 1) & 1u) + 2u * rho;
    };
    auto wl_pos = [&](uint32_t tau, uint32_t c) -> uint32_t {        // byte position of chunk c of tile column tau inside the tile image
        const uint32_t q = tau / RPI, rho = tau % RPI;
        return q * 1024u + rho * (uint32_t)RB + ((c ^ wl_sw(rho, q)) * 16u);
    };
    const uint32_t pcol = (uint32_t)(8 * (i >> 2) + (i & 3));
    uint32_t idaddr[NV];
    if constexpr (WL) {
#pragma unroll
        for (int q = 0; q < NI; ++q) idaddr[q] = pad + (uint32_t)(RPI * q + lane / CPR) * 4u;
    } else { idaddr[0] = pad + pcol * 4u; idaddr[1] = pad + (pcol + 4u) * 4u; }
    idaddr[NV - 2] = pad + 128u + (uint32_t)i * 4u;
    idaddr[NV - 1] = pad + 192u + (uint32_t)i * 4u;
    [[maybe_unused]] uint32_t choff[WL ? NI : 1];                   // WL: byte offset inside the row this lane fetches with instruction q
    if constexpr (WL) {
#pragma unroll
        for (int q = 0; q < NI; ++q) {
            const uint32_t c = (uint32_t)(lane % CPR) ^ wl_sw((uint32_t)(lane / CPR), (uint32_t)q);
            choff[q] = ((int)(c * 8u) < a.Dpad) ? c * 16u : 0u;      // (a chunk past Dpad: chunk 0 instead - valid memory, multiplied by zeros)
        }
    }
    uint32_t qaddr[NQ];
#pragma unroll
    for (int k = 0; k < 2 * KS; ++k) {
        if constexpr (WL) {   // operand (sub, ks) of MFMA #1: row m = i of half sub (tile column 8 (i >> 2) + 4 sub + (i & 3)), chunk 4 ks + g
            const uint32_t sub = (uint32_t)(k / KS), ks = (uint32_t)(k % KS);
            qaddr[k] = ring + wl_pos(8u * (uint32_t)(i >> 2) + 4u * sub + (uint32_t)(i & 3), 4u * ks + (uint32_t)g);
        } else qaddr[k] = ring + (uint32_t)k * 1024u + (uint32_t)lane * 16u;
    }
    [[maybe_unused]] const uint32_t vaddr0 = aux + (uint32_t)lane * 16u;   // backward: this lane's run of saved scores (second block: + 1024)
    const uint32_t caddr[2] = {pad + 32u * (uint32_t)g, pad + 32u * (uint32_t)g + 16u};   // ids of my eight tile columns (backward)
    // transpose reads: this lane addresses k row j = i >> 2 (row m = 4g + j of half h), feature quad q = i & 3 of slice s
    uint32_t raddr[NT][2];
#pragma unroll
    for (int s = 0; s < NT; ++s)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if constexpr (WL) {   // row m = 4g + (i >> 2) of half h = tile column 8g + 4h + (i >> 2); features 16 s + 4 (i & 3) ..
                raddr[s][h] = ring + wl_pos(8u * (uint32_t)g + 4u * (uint32_t)h + (uint32_t)(i >> 2), 2u * (uint32_t)s + (uint32_t)((i & 3) >> 1)) + 8u * (uint32_t)(i & 1);
            } else
                raddr[s][h] = ring + (uint32_t)((h * KS + (s >> 1)) * 1024 + ((2 * (s & 1) + ((i & 3) >> 1)) * 16 + 4 * g + (i >> 2)) * 16 + 8 * (i & 1));
        }
    const uint32_t stg_i = aux + (uint32_t)i * CAP * 4u;
    const uint32_t junk = aux + 16u * CAP * 4u + (uint32_t)lane * 4u;
    const uint32_t flush_base = aux + (uint32_t)lane * 4u;
    const uint32_t low8 = (1u << (8 * g)) - 1u;                                         // condensed columns left of my eight
    const uint32_t halfbits[2] = {0x0f0f0f0fu, 0xf0f0f0f0u};                            // tile columns of each half

    uint32_t emax = 0u;
    float dsum = 0.f;

    // one run: consecutive tiles t .. te-1 of window w, accumulated into acc
    auto run = [&](const int w, int64_t t, const int64_t te, floatx4 (&acc)[NT], const int ka_i) {
        if (t >= te) return;
        const float c_val = wv * pow2f(ka_i);   // power-of-two scaling commutes with rounding: fl(x * w) * 2^ka == fl(x * (w * 2^ka))
        // B operand of MFMA #1: window row i, halves 32*ks + 8g .. +7 (rows past N read the zero sentinel row)
        int64_t arow = (int64_t)w * kWinRows + i;
        arow = arow < a.N ? arow + a.row_off : a.Nc;
        const _Float16* ap = a.x16 + arow * stride + 8 * g;
        half8 af[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) af[ks] = (ks * 32 + 8 * g < a.Dpad) ? *reinterpret_cast<const half8*>(ap + ks * 32) : hz;
        const int64_t wrow = (int64_t)w * kWinRows;
        const int64_t e_w0 = a.rowptr[wrow < a.N ? wrow : a.N];
        char* const ef_w = reinterpret_cast<char*>(a.ef + e_w0);
        uint32_t cnt = 0u, rstart = ~0u;                           // staged results of row i / window-relative position of the first
        [[maybe_unused]] bool flush_pending = false;

        auto flush = [&]() {
            uint32_t vals[16];
            lds_rows_block8<CAP * 4, 0>(flush_base, vals);
            lds_rows_block8<CAP * 4, 8>(flush_base, vals + 8);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t c_r = (uint32_t)__builtin_amdgcn_readlane((int)cnt, r);
                const uint32_t s_r = (uint32_t)__builtin_amdgcn_readlane((int)rstart, r);
                if ((uint32_t)lane < c_r) {
                    st_stream(reinterpret_cast<uint32_t*>(ef_w + ((s_r + (uint32_t)lane) << 2)), vals[r]);
                    const uint32_t ab = vals[r] & 0x7fffffffu;           // max |ef| for the backward call's scale
                    emax = ab > emax ? ab : emax;
                }
            }
            cnt = 0u; rstart = ~0u;
        };
        auto dma_b = [&](const uint32_t* cid) {
            if constexpr (WL) {   // NI instructions of RPI whole rows each
                if (MAXW == 0 && a.big) {
                    const char* const xb = reinterpret_cast<const char*>(a.x16);
#pragma unroll
                    for (int q = 0; q < NI; ++q)
                        __builtin_amdgcn_global_load_lds((GLB_AS const void*)(xb + (uint64_t)cid[q] * (uint64_t)(stride * 2) + choff[q]),
                                                         (LDS_AS void*)(uintptr_t)(ring + q * 1024), 16, 0, 0);
                    return;
                }
#pragma unroll
                for (int q = 0; q < NI; ++q)
                    __builtin_amdgcn_struct_ptr_buffer_load_lds(xrsrc, (LDS_AS void*)(uintptr_t)(ring + q * 1024), 16, (int)cid[q], (int)choff[q], 0, 0, 0);
                return;
            }
            if (MAXW == 0 && a.big) {   // (the range-major variant, on request only, is at its register limit: the launcher keeps big images off it)
                const char* const xb = reinterpret_cast<const char*>(a.x16);
#pragma unroll
                for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks)
                        __builtin_amdgcn_global_load_lds((GLB_AS const void*)(xb + (uint64_t)cid[sub] * (uint64_t)(stride * 2) + boff[ks]),
                                                         (LDS_AS void*)(uintptr_t)(ring + (sub * KS + ks) * 1024), 16, 0, 0);
                return;
            }
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
                    __builtin_amdgcn_struct_ptr_buffer_load_lds(xrsrc, (LDS_AS void*)(uintptr_t)(ring + (sub * KS + ks) * 1024), 16,
                                                                (int)cid[sub], (int)boff[ks], 0, 0, 0);
        };
        struct Cur { uint32_t m, eb; int sh; bool wide; uintx4 c[2]; };
        // saved scores of row i inside my eight tile columns: one run of ef.  Four floats (clamped to stay inside ef)
        // cover it almost always; a second DMA fetches the next four when some lane's run is longer.
        auto dma_vals = [&](Cur& c) {
            // (32-bit arithmetic: edge offsets are int32 by the CSR's type)
            const int32_t e0 = (int32_t)c.eb + __popc(c.m & low8);
            int32_t lo = min(e0, (int32_t)a.E - 8);
            lo = max(lo, 0);
            c.sh = e0 - lo;
            c.wide = __any(__popc((c.m >> (8 * g)) & 0xffu) + c.sh > 4);
            __builtin_amdgcn_global_load_lds((GLB_AS const void*)(a.ef + lo), (LDS_AS void*)(uintptr_t)aux, 16, 0, 0);
            if (c.wide) __builtin_amdgcn_global_load_lds((GLB_AS const void*)(a.ef + lo + 4), (LDS_AS void*)(uintptr_t)(aux + 1024), 16, 0, 0);
        };
        auto stage = [&](Cur& cur, int64_t& tcur, int64_t& tn) -> bool {
            wait_vm0();
            uint32_t v[NV];
            uintx4 q[NQ];
            lds_ids_block<NV>(idaddr, v, qaddr[0], q[0]);         // next tile: its row ids for my lane, my row's mask and edge offset; + operand 0
            if (!valonly) lds_q_block<NQ - 1, 0>(qaddr + 1, q + 1);   // the other operands (values only: no scores, nothing reads them)
            // backward: the saved score of tile column j of my eight is word (edges of row i left of it in my run) of the run the
            // DMA fetched - read by ADDRESS (r03; a cascade of selects over eight registers cost ten VALU instructions per column
            // in a loop that is VALU-bound: 265 per tile, SQ_INSTS_VALU of profiles/r02).  Lanes without the edge read a
            // neighbouring word that the mask removes below.
            [[maybe_unused]] uint32_t sv[8];
            if constexpr (BWD) {
                const uint32_t byte0 = (cur.m >> (8 * g)) & 0xffu;
                uint32_t va = vaddr0 + ((uint32_t)cur.sh << 2), ad[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    ad[j] = va;
                    va -= (uint32_t)((int32_t)(byte0 << (31 - j)) >> 31) << 2;        // + 4 where the edge exists
                }
                if (cur.wide) {   // (wave-uniform, rare: some lane's run crosses into the second block of four)
#pragma unroll
                    for (int j = 0; j < 8; ++j) ad[j] += (((ad[j] - vaddr0) >> 4) & 1u) * 1008u;
                }
                lds_read8_b32(ad, sv);
            }
            Cur nx;
            nx.m = v[NV - 2]; nx.eb = v[NV - 1]; nx.sh = 0; nx.wide = false;
            if constexpr (BWD) lds_q_block<2, 0>(caddr, nx.c);
            half4 lo[NT], hi[NT];
            lds_tr_block<NT, 0>(raddr, lo, hi);
            const bool more = tn < te;
            const int64_t tnn = tn + 1;
            if (more) {
                dma_b(v);
                if constexpr (BWD) dma_vals(nx);
                if (tnn < te) meta.dma(tnn, pad);
            }
            if constexpr (!BWD) {   // (see sddmm_kernel: a pending flush goes right behind the gather)
                if (flush_pending) { flush(); flush_pending = false; }
            }
            // ---- tile tcur: scores
            floatx4 S[2];
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                S[sub] = floatx4{0.f, 0.f, 0.f, 0.f};
                if (!valonly && __any((cur.m & halfbits[sub]) != 0u)) {
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks)
                        S[sub] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, q[sub * KS + ks]), af[ks], S[sub], 0, 0, 0);
                }
            }
            // ---- edge weights of row i for my eight tile columns (branch-free; 10-bit RNA rounding done in integer
            //      arithmetic, after which the round-toward-zero pack conversion is exact)
            const uint32_t byte = (cur.m >> (8 * g)) & 0xffu;
            // (the tile loop is VALU-bound - 160 VALU instructions per tile before this form - so the eight columns are
            // handled with masks instead of compares and selects: mk = all-ones where the edge exists; the second scale
            // factor is 1.0 unless the exponent needs two steps, and multiplying by it is exact)
            [[maybe_unused]] uint32_t wpos = stg_i + ((cnt + (uint32_t)__popc(cur.m & low8)) << 2);   // forward: its staging slot
            uint32_t rb[8];
            [[maybe_unused]] float scv[8];
            if constexpr (!BWD) {
#pragma unroll
                for (int j = 0; j < 8; ++j) scv[j] = S[j >> 2][j & 3] * inv_a;
                if (__builtin_expect(two_step, 0)) {   // (kernel-uniform, almost never taken; the empty asm keeps it a branch - if-converted
                                                       //  it costs a multiply and a select per column)
                    asm volatile("; second scale factor");
#pragma unroll
                    for (int j = 0; j < 8; ++j) scv[j] *= inv_b;
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t mk = (uint32_t)((int32_t)(byte << (31 - j)) >> 31);   // (one v_bfe_i32)
                [[maybe_unused]] const float sraw = S[j >> 2][j & 3];
                [[maybe_unused]] float sc = 0.f;
                if constexpr (!BWD) sc = scv[j];
                float att_s;
                if constexpr (BWD) {
                    att_s = __uint_as_float(sv[j]) * c_val;                          // = fl32(w * ef) * 2^ka
                } else {
                    lds_write_b32(bitfield_select(mk, wpos, junk), sc);
                    asm("v_mad_i32_i24 %0, %1, -4, %0" : "+v"(wpos) : "v"(mk));           // wpos += 4 where the edge exists (mk = -1)
                    att_s = sc * c_val;                                              // = fl32(w * ef) * 2^ka
                }
                // (+ half an ulp of the 10-bit mantissa; the 13 bits below it are cut by the round-toward-zero pack conversion itself -
                //  in fp16's normal range exactly the bits `& 0xffffe000` would clear, below it a coarser cut toward zero of the same value)
                rb[j] = (__float_as_uint(att_s) & mk) + 0x1000u;
            }
            if constexpr (BWD) {
                if (!valonly) {   // sum_e s[e] * col(e) (the raw accumulators: their power-of-two scale is applied once, to the workgroup's sum)
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const uint32_t mk = (uint32_t)((int32_t)(byte << (31 - j)) >> 31);
                        dsum += __uint_as_float(__float_as_uint(S[j >> 2][j & 3]) & mk) * (float)(int32_t)cur.c[j >> 2][j & 3];
                    }
                }
            }
            half8 a16;
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
                const auto pk = __builtin_amdgcn_cvt_pkrtz(__uint_as_float(rb[j]), __uint_as_float(rb[j + 1]));
                a16[j] = (_Float16)pk[0];
                a16[j + 1] = (_Float16)pk[1];
            }
            // ---- aggregation
#pragma unroll
            for (int s = 0; s < NT; ++s) {
                const half8 bf = __builtin_shufflevector(lo[s], hi[s], 0, 1, 2, 3, 4, 5, 6, 7);
                acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a16, bf, acc[s], 0, 0, 0);
            }
            if constexpr (!BWD) {
                if (rstart == ~0u && cur.m != 0u) rstart = cur.eb - (uint32_t)e_w0;
                cnt += (uint32_t)__popc(cur.m);
                // a tile adds at most 32 results to a row: flush while every row still has room for one more tile
                if (!more) flush();
                else flush_pending = __any(cnt > (uint32_t)(CAP - 32));
            }
            cur = nx;
            tcur = tn;
            tn = tnn;
            return more;
        };

        // prologue: metadata of the first tile, its operands [and saved scores], metadata of the second
        meta.dma(t, pad);
        wait_vm0();
        Cur cur;
        {
            uint32_t v[NV];
            uintx4 dummy;
            lds_ids_block<NV>(idaddr, v, qaddr[0], dummy);
            cur.m = v[NV - 2]; cur.eb = v[NV - 1]; cur.sh = 0; cur.wide = false;
            if constexpr (BWD) lds_q_block<2, 0>(caddr, cur.c);
            dma_b(v);
            if constexpr (BWD) dma_vals(cur);
        }
        int64_t tn = t + 1;
        if (tn < te) meta.dma(tn, pad);
        while (stage(cur, t, tn)) {}
        wait_vm0();
    };

    const float inv1 = pow2f(-kx);
    // (lane (g, i) holds rows 4g .. 4g + 3 of output column i; row r's exponent sits in the lanes with i == r)
    auto row_inv = [&](const int ka_i, float (&inv2)[4]) {
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) inv2[ii] = pow2f(-__shfl(ka_i, 4 * g + ii));
    };
    auto store_rows = [&](const int w, const int s, const floatx4& v, const int ka_i) {
        const int64_t row0 = (int64_t)w * kWinRows + 4 * g;
        const int colg = 16 * s + i;
        float inv2[4];
        row_inv(ka_i, inv2);
        if (colg < a.D) {
#pragma unroll
            for (int ii = 0; ii < 4; ++ii)
                if (row0 + ii < a.N) a.y[(row0 + ii) * a.D + colg] = v[ii] * inv1 * inv2[ii];
        }
    };

    [[maybe_unused]] int w0 = 0, ka0 = 0;
    [[maybe_unused]] floatx4 acc0[NT];
    if constexpr (MAXW == 0) {
#pragma unroll
        for (int s = 0; s < NT; ++s) acc0[s] = floatx4{0.f, 0.f, 0.f, 0.f};
        if (a.nslices > 0) {
            // XCD-sliced walk (r03).  Workgroups are dealt to the eight XCDs round-robin (workgroup b runs on XCD b % 8), and here
            // workgroup b only ever gathers rows of column slice b % nslices: an XCD's 4 MB L2 then holds the one slice of the fp16
            // image it is asked for (Reddit shape, D = 64: 29.8 MB / 8) instead of seeing all of it - tools/gather_bench.hip: rows out
            // of an L2-resident slice arrive at 14-17 TB/s against 8.3 TB/s for rows of the whole image, which is what the
            // per-window walk runs at.  Every wavefront takes the tiles of ONE window inside the slice (bptr: the plan's bucket
            // table) and stores its sums as that slice's addend of Y (a.y = nslices buffers), which agnn_slice_sum_kernel adds in
            // slice order: deterministic, and nothing depends on the placement being what is assumed here.
            // (more than eight slices - an image of 16 .. 32 MB - go in ROUNDS of eight: the grid's first 1 / rounds takes slices
            //  0 .. 7, the next one slices 8 .. 15, and workgroups start in grid order, so an XCD is asked for one slice at a time)
            const unsigned per_round = gridDim.x / (unsigned)(a.nslices / kXcds), b2 = blockIdx.x % per_round;
            const int slice = (int)(blockIdx.x / per_round) * kXcds + (int)(b2 % (unsigned)kXcds);
            const int wi = (int)(b2 / (unsigned)kXcds) * WAVES + wave;
            if (a.rot) {
                const int span = (int)(per_round / (unsigned)kXcds) * WAVES;   // window positions of one round (>= nw)
                int wr = wi + (int)(((int64_t)(slice % kXcds) * a.nw) / kXcds);
                if (wr >= span) wr -= span;
                w0 = wr < a.nw ? wr : -1;
            } else
            w0 = wi < a.nw ? __builtin_amdgcn_readfirstlane(a.order[wi]) : -1;
            if (w0 >= 0) {
                const int64_t tb = a.wb_ptr[w0];
                const uint32_t* bp = a.bptr + (int64_t)w0 * (a.nbuckets + 1);
                ka0 = row_ka(w0);
                run(w0, tb + bp[slice * a.gsel], tb + bp[(slice + 1) * a.gsel], acc0, ka0);
            }
        } else {
            w0 = a.order[blockIdx.x];
            const int64_t tb = a.wb_ptr[w0], te_w = a.wb_ptr[w0 + 1];
            const int64_t chunk = (te_w - tb + WAVES - 1) / WAVES;         // contiguous share of this wavefront
            const int64_t t0 = tb + wave * chunk;
            ka0 = row_ka(w0);
            run(w0, t0, t0 + chunk < te_w ? t0 + chunk : te_w, acc0, ka0);
        }
    } else if (a.use_sync) {
        // slice-synchronised walk (r06): the wavefronts of XCD x own MAXW windows each of ONE slice of that XCD's share and walk its phases
        // (a few hot column buckets each, ~3 MB of rows) together - spmm_sync_kernel's schedule with this kernel's run
        int x, w_lo, w_hi, nph;
        sync_slice_of(a.sync, x, w_lo, w_hi, nph);
        const int nwv = (int)(gridDim.x / (unsigned)kXcds) * WAVES, wid = (int)(blockIdx.x / (unsigned)kXcds) * WAVES + wave;
        const int ts = a.sync.kmax + 1;
        for (int base = w_lo + wid; base < w_hi; base += nwv * MAXW) {
            int wj[MAXW], kaj[MAXW];
            int64_t tbj[MAXW];
            floatx4 acc[MAXW][NT];
#pragma unroll
            for (int j = 0; j < MAXW; ++j) {
                const int w = base + j * nwv;
                wj[j] = w < w_hi ? w : -1;
                tbj[j] = wj[j] >= 0 ? a.wb_ptr[wj[j]] : 0;
                kaj[j] = wj[j] >= 0 ? row_ka(wj[j]) : 0;
#pragma unroll
                for (int s = 0; s < NT; ++s) acc[j][s] = floatx4{0.f, 0.f, 0.f, 0.f};
            }
            for (int r = 0; r < nph; ++r) {
                const int k0 = r * a.sync.m < a.sync.kmax ? r * a.sync.m : a.sync.kmax, k1 = (r + 1) * a.sync.m < a.sync.kmax ? (r + 1) * a.sync.m : a.sync.kmax;
#pragma unroll
                for (int j = 0; j < MAXW; ++j) {
                    if (wj[j] < 0) continue;
                    const uint32_t* Tw = a.sync.T + (int64_t)wj[j] * ts;
                    run(wj[j], tbj[j] + Tw[k0], tbj[j] + Tw[k1], acc[j], kaj[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < MAXW; ++j) {
                if (wj[j] < 0) continue;
#pragma unroll
                for (int s = 0; s < NT; ++s) store_rows(wj[j], s, acc[j][s], kaj[j]);
            }
        }
    } else {
        const int gw = blockIdx.x * WAVES + wave, gwn = gridDim.x * WAVES;
        for (int grp = gw; grp < a.ngroups; grp += gwn) {
            int wj[MAXW], kaj[MAXW];
            int64_t tbj[MAXW];
            floatx4 acc[MAXW][NT];
#pragma unroll
            for (int j = 0; j < MAXW; ++j) {
                const int idx = grp + j * a.ngroups;   // strided picks from the heaviest-first order: balanced groups
                wj[j] = idx < a.nw ? __builtin_amdgcn_readfirstlane(a.order[idx]) : -1;
                tbj[j] = wj[j] >= 0 ? a.wb_ptr[wj[j]] : 0;
                kaj[j] = wj[j] >= 0 ? row_ka(wj[j]) : 0;
#pragma unroll
                for (int s = 0; s < NT; ++s) acc[j][s] = floatx4{0.f, 0.f, 0.f, 0.f};
            }
            for (int r = 0; r < a.nranges; ++r) {
#pragma unroll
                for (int j = 0; j < MAXW; ++j) {
                    if (wj[j] < 0) continue;
                    const uint32_t* bp = a.bptr + (int64_t)wj[j] * (a.nbuckets + 1);
                    run(wj[j], tbj[j] + bp[r * a.gsel], tbj[j] + bp[(r + 1) * a.gsel], acc[j], kaj[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < MAXW; ++j) {
                if (wj[j] < 0) continue;
#pragma unroll
                for (int s = 0; s < NT; ++s) store_rows(wj[j], s, acc[j][s], kaj[j]);
            }
        }
    }

    if constexpr (BWD) {
        // sum_e score(e) * col(e): per-wavefront double, then one slot per workgroup (fixed order -> deterministic)
        double d = (double)dsum * (double)inv_a * (double)inv_b;   // (dsum holds raw MFMA sums: scores * 2^(2 kx))
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) d += __shfl_xor(d, off, 64);
        __syncthreads();
        double* dred = reinterpret_cast<double*>(smem);
        if (lane == 0) dred[wave] = d;
        __syncthreads();
        if (threadIdx.x == 0) {
            double tot = 0.0;
            for (int ww = 0; ww < WAVES; ++ww) tot += dred[ww];
            a.partial[blockIdx.x] = tot;
        }
    } else {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)emax, off, 64); emax = o > emax ? o : emax; }
        // one word for the whole launch: 600k same-address atomics serialise in one L2 channel (12 ns each - they cost
        // 3 ms on the ogbn-products shape).  The running maximum stops growing after a handful of wavefronts, so look first.
        if (lane == 0 && emax != 0u && emax > __hip_atomic_load(a.ef_absmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(a.ef_absmax, emax);
    }

    // ---- per-window workgroups: combine the wavefronts' partial sums in a fixed order and store
    if constexpr (MAXW == 0) {
        if (a.nslices > 0) {   // a wavefront = a window: its sums are one slice's addend
            if (w0 >= 0) {
                const unsigned per_round = gridDim.x / (unsigned)(a.nslices / kXcds);
                const int slice = (int)(blockIdx.x / per_round) * kXcds + (int)((blockIdx.x % per_round) % (unsigned)kXcds);
                const int64_t row0 = (int64_t)w0 * kWinRows + 4 * g;
                float* const yp = a.y + (int64_t)slice * a.N * a.D;
                float inv2[4];
                row_inv(ka0, inv2);
#pragma unroll
                for (int s = 0; s < NT; ++s) {
                    const int colg = 16 * s + i;
                    if (colg < a.D) {
#pragma unroll
                        for (int ii = 0; ii < 4; ++ii)
                            if (row0 + ii < a.N) st_stream(&yp[(row0 + ii) * a.D + colg], acc0[s][ii] * inv1 * inv2[ii]);
                    }
                }
            }
        } else if constexpr (WAVES > 1) {
            __syncthreads(); // every wave is done with its LDS
            floatx4* red = reinterpret_cast<floatx4*>(smem);
#pragma unroll
            for (int s = 0; s < NT; ++s) red[(wave * NT + s) * 64 + lane] = acc0[s];
            __syncthreads();
            for (int s = wave; s < NT; s += WAVES) {
                floatx4 v = red[s * 64 + lane];
#pragma unroll
                for (int ww = 1; ww < WAVES; ++ww) {
                    const floatx4 o = red[(ww * NT + s) * 64 + lane];
                    v[0] += o[0]; v[1] += o[1]; v[2] += o[2]; v[3] += o[3];
                }
                store_rows(w0, s, v, ka0);
            }
        } else {
#pragma unroll
            for (int s = 0; s < NT; ++s) store_rows(w0, s, acc0[s], ka0);
        }
    }
}

// Y = sum of the XCD-sliced walk's addends, in slice order (float4 where the pointers allow)
__global__ __launch_bounds__(256) void agnn_slice_sum_kernel(const float* __restrict__ part, float* __restrict__ y, int64_t n, int64_t stride, int32_t nslices) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gsz = (int64_t)gridDim.x * blockDim.x;
    if (((reinterpret_cast<uintptr_t>(part) | reinterpret_cast<uintptr_t>(y)) & 15) == 0 && ((n | stride) & 3) == 0) {
        const int64_t n4 = n >> 2, s4 = stride >> 2;
        const float4* p4 = reinterpret_cast<const float4*>(part);
        for (int64_t k = gid; k < n4; k += gsz) {
            float4 v = p4[k];
            for (int s = 1; s < nslices; ++s) { const float4 o = p4[(int64_t)s * s4 + k]; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
            reinterpret_cast<float4*>(y)[k] = v;
        }
    } else {
        for (int64_t k = gid; k < n; k += gsz) {
            float v = part[k];
            for (int s = 1; s < nslices; ++s) v += part[(int64_t)s * stride + k];
            y[k] = v;
        }
    }
}

// partial[0..n) -> out[0], fixed order.  One workgroup of 1024, four independent loads per thread and step: the sliced walk leaves
// 29 k partials on the Reddit shape, and 256 threads taking one dependent load per step spent 47 us on them (a memory round trip
// per step) - 2 x 47 us of an AGNN epoch.
static constexpr int kReduceThreads = 1024;
__global__ __launch_bounds__(kReduceThreads) void agnn_reduce_kernel(const double* __restrict__ partial, int32_t n, float* __restrict__ out, const double* __restrict__ extra = nullptr) {
    __shared__ double sh[kReduceThreads];
    double s = 0.0;
    int k = (int)threadIdx.x;
    for (; k + 3 * kReduceThreads < n; k += 4 * kReduceThreads) {
        const double a = partial[k], b = partial[k + kReduceThreads], c = partial[k + 2 * kReduceThreads], d = partial[k + 3 * kReduceThreads];
        s += (a + b) + (c + d);
    }
    for (; k < n; k += kReduceThreads) s += partial[k];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = kReduceThreads / 2; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)(sh[0] + (extra ? extra[0] : 0.0));   // (extra: wide_patch_kernel's correction, the double at header word kHdrDwExtra; zero unless the call was patched)
}

template <int WAVES, bool BWD, int MAXW>
static hipError_t launch_agnn(int nt, const AgnnArgs& args, int nwg, hipStream_t stream) {
    return with_width<8>(nt, [&](auto NT) { return launch_kernel<agnn_kernel<NT, WAVES, BWD, MAXW>>(dim3((unsigned)nwg), agnn_geom(NT, WAVES, BWD, MAXW), stream, args); });
}
// the fused backward kernel beyond 96 columns on the slice-synchronised walk: one window per wavefront (MAXW = 1)
static hipError_t launch_agnn_wide_one(int nt, const AgnnArgs& args, int nwg, hipStream_t stream) {
    const dim3 grid((unsigned)nwg);
    if (nt == 7) return launch_kernel<agnn_kernel<7, 4, true, 1>>(grid, agnn_geom(7, 4, true, 1), stream, args);
    if (nt == 8) return launch_kernel<agnn_kernel<8, 4, true, 1>>(grid, agnn_geom(8, 4, true, 1), stream, args);
    return hipErrorInvalidValue;
}
