// tcgnn_lds_val.inc - the EDGE-VALUED SpMM (forward_AGNN, TCGNN_kernel.cu:459-578) on the LDS-resident flat walk (r04).
// Included by tcgnn_device.hip after tcgnn_lds_flat.inc, whose range filler, metadata blocks and A-fragment expansion it shares.
//
// Why: until r04 the edge-valued operator only had gather walks (one fp16 row per EDGE through an L2 channel: 14.5 GB at D = 64,
// 1.6 ms on the Reddit shape, DESIGN.md 4.3b "the roofline that binds a gather formulation is the L2's") while the binary SpMM
// streams column ranges through LDS (0.46 ms).  What kept the values out of that walk (DESIGN.md 4.2e) was their position: a K
// slot of a cell-stream tile is a condensed COLUMN, which may hold several edges of the window, so a value per slot is not enough
// and a value per (row, slot) is 16 x the metadata.
//
// Here the stream is cut from a SINGLE-EDGE tile stream (expand_edges_kernel: every condensed column repeated once per edge - 1.02
// to 1.05 slots per column on the Reddit shapes), so a K slot carries exactly one edge:
//   A[i][k] = (mask bit (i, k)) ? value of slot k : 0  =  (binary A fragment, 2.0 or 0) x (the tile's 32 slot values),
// the nine-instruction expansion of the binary kernel plus four packed multiplies; the values are one more 64-byte block per tile
// beside the 128 bytes of ids and masks.  Per call the caller's edge values (CSR order) are brought into stream order by
// val_permute_kernel: one workgroup per window slot stages the window's run of the CSR in LDS (coalesced) and writes the window's
// tiles 64 bytes at a time - scattered 4-byte requests would run at the L2's request rate (~1e11 / s: 1.6 ms for 160 M slots).
// Cells hold at most 32 edges (flat stream, one tile per cell); what lies beyond, and the (workgroup, range) pairs too thin for a
// range fill, is the cold remainder, added from the planar image by spmm_cold_val_kernel.
//
// Numerics: values are rounded to a 10-bit mantissa with the reference's rule and scaled by the power of two of max |value|
// (header word kHdrMaxVal), exactly as the gather walks' TileWalker<NT, true> does; products are exact in fp32; sums run in range order.

struct SpmmValArgs {
    const uint32_t* blocks;     // plan: [npairs][16 wavefronts][32 T words] ids + masks (as SpmmFlatArgs::blocks)
    const _Float16* vals;       // per call: [npairs][16 wavefronts][T][32] slot values, scaled fp16
    const int32_t* order;
    const _Float16* x16;        // planar image
    const uint32_t* hdr;
    float* y;
    int32_t N, D, stride, chunk0, xrows, nw, nwg;
    const int32_t* rbase;
    const uint32_t* rl2;        // entry records + descriptor words of the stream (tcgnn_lds_flat.inc)
    int32_t nent;
};

// per-window edge counts -> the single-edge stream's wide blocks (host prefix sum)
__global__ __launch_bounds__(256) void window_edges_kernel(const int32_t* __restrict__ rowptr, int32_t N, int32_t nw, int32_t* __restrict__ out) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    const int64_t r0 = (int64_t)w * kWinRows, r1 = r0 + kWinRows < N ? r0 + kWinRows : N;
    out[w] = r0 < N ? rowptr[r1] - rowptr[r0] : 0;
}

// packed tile stream (cols / mask / ebase) -> single-edge stream: column q of a window with p edges becomes p consecutive slots,
// each with one mask bit and the CSR position of its edge (ebase + rank inside the tile row, as the gather walks compute it).
// One workgroup per window; a block scan ranks the edges of each 256-column chunk.  Columns stay in non-decreasing order.
__global__ __launch_bounds__(256) void expand_edges_kernel(const int64_t* __restrict__ wb_ptr, const int32_t* __restrict__ cols, const uint32_t* __restrict__ mask,
                                                           const int32_t* __restrict__ ebase, const int64_t* __restrict__ xwb_ptr, int32_t* __restrict__ xcols,
                                                           uint32_t* __restrict__ xmask, int32_t* __restrict__ xeidx, int32_t Nc, int32_t* __restrict__ flags) {
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t base_s;
    const int w = blockIdx.x;
    const int64_t tb = wb_ptr[w], n = (wb_ptr[w + 1] - tb) * kWbCols;
    const int64_t xb = xwb_ptr[w], xcap = (xwb_ptr[w + 1] - xb) * kWbCols;
    if (threadIdx.x == 0) base_s = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int64_t q0 = 0; q0 < n; q0 += blockDim.x) {
        const int64_t q = q0 + threadIdx.x;
        uint32_t rowsmask = 0u;
        int32_t c = Nc;
        const uint32_t b = (uint32_t)(q & 31);
        if (q < n) {
            c = cols[tb * kWbCols + q];
            if (c < Nc) {
                const uint32_t* m = mask + (tb + (q >> 5)) * kWinRows;
#pragma unroll
                for (int r = 0; r < kWinRows; ++r) rowsmask |= ((m[r] >> b) & 1u) << r;
            }
        }
        const uint32_t pc = (uint32_t)__builtin_popcount(rowsmask);
        uint32_t incl = pc;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)incl, o); if (lane >= o) incl += t; }
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        uint32_t s = base_s + incl - pc;
        for (int k = 0; k < wv; ++k) s += wsum[k];
        while (rowsmask) {
            const int r = __builtin_ctz(rowsmask);
            rowsmask &= rowsmask - 1u;
            if ((int64_t)s >= xcap) { flags[0] = 1; break; }   // (more set bits than CSR edges: the plan is inconsistent)
            const uint32_t mrow = mask[(tb + (q >> 5)) * kWinRows + r];
            xcols[xb * kWbCols + s] = c;
            atomicOr(&xmask[(xb + (s >> 5)) * kWinRows + r], 1u << (s & 31u));
            xeidx[xb * kWbCols + s] = ebase[(tb + (q >> 5)) * kWinRows + r] + __builtin_popcount(mrow & ((1u << b) - 1u));
            ++s;
        }
        __syncthreads();
        if (threadIdx.x == 0) base_s += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
}

// Edge values (fp32, CSR order) -> the stream's slot values (scaled fp16, stream order) and the cold tiles' values.  One workgroup
// per window slot p = (workgroup, wavefront, slot j): the window's edges are ONE run of the CSR (16 consecutive rows), converted
// once and staged in LDS with coalesced loads when it fits (kValSpan halves; a longer window converts per slot from global memory);
// the window's tiles - entry j of block (pair k, wavefront) for every hot pair k of its workgroup - are written 64 bytes each, their
// edges looked up through 16-bit offsets into the window's run (eidx16; 0xffff: no edge).  Eight tiles per 32 lanes are in flight
// at a time (the first version walked them one dependent round trip after the other: 0.93 ms on the Reddit shape).
// int32 CSR positions -> 16-bit offsets from the window's first edge; `bad` is raised by a window with 65 535 edges or more
// window slot of tile x of a DENSE entry's block (descriptor: tiles per window slot, four bits each, in slot order); -1: an empty tile
__device__ __forceinline__ int dense_tile_slot(uint32_t desc, int x, int maxw) {
    int run = 0;
    for (int j = 0; j < maxw; ++j) { run += (int)((desc >> (4 * j)) & 15u); if (x < run) return j; }
    return -1;
}
__global__ __launch_bounds__(256) void val_index16_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ order, const int32_t* __restrict__ eidx,
                                                          const int32_t* __restrict__ rbase, uint16_t* __restrict__ out, int32_t N, int32_t maxw,
                                                          const int64_t* __restrict__ cold_ptr, const int32_t* __restrict__ cold_eidx, uint16_t* __restrict__ cout,
                                                          int32_t* __restrict__ bad, const uint32_t* __restrict__ rl2, int32_t nent) {
    const int p = blockIdx.x;
    int wg, wave, j;
    cell_place(p, maxw, wg, wave, j);
    const int w = order[p];
    int64_t e0 = 0, e1 = 0;
    if (w >= 0) {
        const int64_t r0 = (int64_t)w * kWinRows, r1 = r0 + kWinRows < N ? r0 + kWinRows : N;
        e0 = rowptr[r0]; e1 = rowptr[r1];
    }
    if (e1 - e0 >= 65535 && threadIdx.x == 0) bad[0] = 1;
    auto conv = [&](int32_t e) -> uint16_t { return (e < 0 || e < e0 || e - e0 >= 65535) ? (uint16_t)0xffffu : (uint16_t)(e - e0); };
    const int k0 = rbase[wg], k1 = rbase[wg + 1];
    const int sub = threadIdx.x >> 5, sl = threadIdx.x & 31;
    for (int64_t i = sub; i < k1 - k0; i += 8) {
        const int64_t t0 = ((k0 + i) * kLdsWaves + wave) * maxw;
        if (!(rl2[(k0 + i) * 4] >> 31)) { out[(t0 + j) * 32 + sl] = conv(eidx[(t0 + j) * 32 + sl]); continue; }   // a normal entry: tile j is slot j's
        const uint32_t desc = rl2[(int64_t)nent * 4 + (k0 + i) * kLdsWaves + wave];
        for (int x = 0; x < maxw; ++x)                                                                 // a dense entry: the tiles its descriptor gives slot j
            if (dense_tile_slot(desc, x, maxw) == j) out[(t0 + x) * 32 + sl] = conv(eidx[(t0 + x) * 32 + sl]);
    }
    if (w >= 0 && cold_ptr)
        for (int64_t t = cold_ptr[w] + sub; t < cold_ptr[w + 1]; t += 8) cout[t * 32 + sl] = conv(cold_eidx[t * 32 + sl]);
}
// (second version.  A workgroup is one (stream workgroup, stream wavefront): its eight windows' runs are staged together - ~63 k
//  halves on the Reddit shape - because the eight tiles of a (pair, wavefront) block are CONTIGUOUS in the index and value arrays:
//  512 bytes per block, one 8-byte piece per lane, whole 128-byte lines - where a workgroup per window moved 64-byte pieces 8 KB
//  apart, 41 M of them, at the L2's request rate: 0.63 ms.)
// (third version: half a wavefront's windows per workgroup - 72 KB of LDS, two workgroups per CU, so that one stages while the
//  other permutes - and eight 8-byte pieces in flight per lane: 0.46 -> see DESIGN.md 4.2e.)
// (fourth version, r05: a QUARTER of a wavefront's windows per workgroup - 36 KB, four workgroups per CU; the runs staged as one
//  index space with sixteen loads per thread in flight instead of window by window, four at a time; the normal entries one batch
//  of eight pieces per lane, the dense entries four blocks per 32 lanes at a time: 0.347 -> 0.25 ms on the calibrated SBM graph.)
static constexpr int kValWpb = 2;                  // windows per workgroup
static constexpr int kValSpanHalves = 9216 * kValWpb;   // 18 KB of LDS per window (Reddit shape: ~7 900 edges per window)
static constexpr int kValThreads = 512;
__global__ __launch_bounds__(kValThreads) void val_permute_kernel(const float* __restrict__ att, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ order,
                                                           const uint16_t* __restrict__ eidx16, const int32_t* __restrict__ rbase, const uint32_t* __restrict__ hdr,
                                                           _Float16* __restrict__ vals, int32_t N,
                                                           const int64_t* __restrict__ cold_ptr, const uint16_t* __restrict__ cold_eidx16, _Float16* __restrict__ cvals,
                                                           const uint32_t* __restrict__ rl2, int32_t has_dense, int32_t nent) {
    extern __shared__ __attribute__((aligned(16))) _Float16 vspan[];
    __shared__ int64_t e0s[kValWpb];
    __shared__ int32_t wins[kValWpb], lens[kValWpb], offs[kValWpb + 1];
    constexpr int MAXW = kLdsMaxW2, PARTS = MAXW / kValWpb;
    const int part = blockIdx.x % PARTS, bw = blockIdx.x / PARTS;
    const int wg = bw / kLdsWaves, wave = bw % kLdsWaves;
    const int j0 = part * kValWpb;
    if (threadIdx.x < kValWpb) {
        const int w = order[cell_position(wg, wave, j0 + (int)threadIdx.x, MAXW)];
        int64_t e0 = 0, e1 = 0;
        if (w >= 0) {
            const int64_t r0 = (int64_t)w * kWinRows, r1 = r0 + kWinRows < N ? r0 + kWinRows : N;
            e0 = rowptr[r0]; e1 = rowptr[r1];
        }
        wins[threadIdx.x] = w; e0s[threadIdx.x] = e0; lens[threadIdx.x] = (int32_t)(e1 - e0 < 65535 ? e1 - e0 : 65535);
    }
    __syncthreads();
    if (threadIdx.x == 0) { int32_t a = 0; for (int j = 0; j < kValWpb; ++j) { offs[j] = a; a += lens[j]; } offs[kValWpb] = a; }
    __syncthreads();
    const float s = pow2f(scale_exp_from_bits(hdr[kHdrMaxVal]));
    const bool staged = offs[kValWpb] <= kValSpanHalves;
    if (staged) {
        // The four runs as ONE index space (element t of the span lies in window j = the number of run starts at or below t): sixteen
        // loads per thread are in flight before the first is converted - two batches stage the ~31 k values of four Reddit-shape
        // windows.  (r04's form walked window by window, four loads at a time: sixteen dependent round trips per workgroup, which
        // is what the kernel's 0.35 ms were - 78 % of its wave cycles parked, profiles/r04.)
        constexpr int LU = 16;
        const int total = offs[kValWpb];

        for (int t0 = 0; t0 < total; t0 += LU * kValThreads) {
            float a[LU];
#pragma unroll
            for (int u = 0; u < LU; ++u) {
                const int t = t0 + u * kValThreads + (int)threadIdx.x;
                int j = 0;
#pragma unroll
                for (int q = 1; q < kValWpb; ++q) j += t >= offs[q];
                a[u] = t < total ? att[e0s[j] + (t - offs[j])] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < LU; ++u) {
                const int t = t0 + u * kValThreads + (int)threadIdx.x;
                if (t < total) vspan[t] = to_half_rna(a[u] * s);
            }
        }
    }
    __syncthreads();
    auto value = [&](uint32_t o, int j) -> uint32_t {   // -> the half's bit pattern
        if (o == 0xffffu) return 0u;
        const _Float16 h = staged ? vspan[offs[j] + (int)o] : to_half_rna(att[e0s[j] + o] * s);
        return (uint32_t)__builtin_bit_cast(unsigned short, h);
    };
    constexpr int LPB = kValWpb * 8;                            // lanes per block: 8 bytes (four slots) each = this workgroup's 64 kValWpb bytes of a block
    const int lb = threadIdx.x % LPB, grp = threadIdx.x / LPB;
    const int k0 = rbase[wg];
    const int wgent = rbase[wg + 1] - k0;   // entries of this stream workgroup (nent: of the whole stream)
    const int npair = (has_dense && wgent > 0) ? (int)rl2[(int64_t)k0 * 4 + 2] : wgent;   // the workgroup's NORMAL entries come first (record word 2 counts them), its dense entries behind them
    const int j = lb >> 3;                                      // local window of this lane's four slots
    constexpr int GRPS = kValThreads / LPB, U = 256 / GRPS > 4 ? 256 / GRPS : 4;   // (pieces in flight per lane: the ~170 normal entries of a Reddit-shape workgroup are one batch)
    const int64_t lane_off = (int64_t)j0 * 32 + lb * 4;         // halves into a block
    for (int i0 = 0; i0 < npair; i0 += GRPS * U) {
        uintx2 o[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + grp + GRPS * u;
            o[u] = uintx2{0xffffffffu, 0xffffffffu};
            if (i < npair) o[u] = *reinterpret_cast<const uintx2*>(eidx16 + (((int64_t)(k0 + i) * kLdsWaves + wave) * MAXW) * 32 + lane_off);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + grp + GRPS * u;
            if (i >= npair) continue;
            uintx2 v;
            v[0] = value(o[u][0] & 0xffffu, j) | (value(o[u][0] >> 16, j) << 16);
            v[1] = value(o[u][1] & 0xffffu, j) | (value(o[u][1] >> 16, j) << 16);
            *reinterpret_cast<uintx2*>(vals + (((int64_t)(k0 + i) * kLdsWaves + wave) * MAXW) * 32 + lane_off) = v;
        }
    }
    // dense entries (tcgnn_lds_flat.inc): the eight tiles of a block belong to the window slots its descriptor names; 32 lanes take
    // a block, lane = (tile, 16-byte piece), and this workgroup writes the tiles of ITS kValWpb windows
    if (has_dense) {
        constexpr int UD = 4;   // blocks in flight per 32 lanes (descriptor word, then the 16-byte piece: two round trips per batch)
        const int l32 = threadIdx.x & 31, grp = threadIdx.x >> 5;   // (this part's own mapping: 32 lanes per block whatever kValWpb)
        constexpr int GRPS = kValThreads / 32;
        const int x = l32 >> 2, piece = l32 & 3;
        for (int i0 = npair; i0 < wgent; i0 += GRPS * UD) {
            uint32_t desc[UD];
#pragma unroll
            for (int u = 0; u < UD; ++u) {
                const int i = i0 + grp + GRPS * u;
                desc[u] = i < wgent ? rl2[(int64_t)nent * 4 + (int64_t)(k0 + i) * kLdsWaves + wave] : 0u;   // (0: every tile empty - slot -1)
            }
            int sl[UD];
            uintx4 oo[UD];
#pragma unroll
            for (int u = 0; u < UD; ++u) {
                const int i = i0 + grp + GRPS * u;
                sl[u] = dense_tile_slot(desc[u], x, MAXW) - j0;
                if (sl[u] < 0 || sl[u] >= kValWpb || i >= wgent) { sl[u] = -1; continue; }
                oo[u] = *reinterpret_cast<const uintx4*>(eidx16 + ((((int64_t)(k0 + i) * kLdsWaves + wave) * MAXW + x) * 32) + piece * 8);
            }
#pragma unroll
            for (int u = 0; u < UD; ++u) {
                if (sl[u] < 0) continue;
                const int i = i0 + grp + GRPS * u;
                uintx4 v;
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = value(oo[u][q] & 0xffffu, sl[u]) | (value(oo[u][q] >> 16, sl[u]) << 16);
                *reinterpret_cast<uintx4*>(vals + ((((int64_t)(k0 + i) * kLdsWaves + wave) * MAXW + x) * 32) + piece * 8) = v;
            }
        }
    }
    if (cold_ptr) {
        const int l32 = threadIdx.x & 31, grp = threadIdx.x >> 5;
        constexpr int GRPS = kValThreads / 32;
        for (int jj = 0; jj < kValWpb; ++jj) {
            const int w = wins[jj];
            if (w < 0) continue;
            for (int64_t t = cold_ptr[w] + grp; t < cold_ptr[w + 1]; t += GRPS)
                cvals[t * 32 + l32] = __builtin_bit_cast(_Float16, (unsigned short)value((uint32_t)cold_eidx16[t * 32 + l32], jj));
        }
    }
}

// One tile of the walk = its 2 NT transposed reads and the 16 bytes of slot values of this lane's K group.  Two register sets, as
// in the flat kernel (tcgnn_lds_blocks.inc lds_flat_issue / step / step_if / drain, whose rules these follow: the set in flight
// is an early-clobber OUTPUT of the statement that issues it and a "+v" operand of the statement that waits for it; the wait is
// counted - lgkmcnt(5) retires everything but the five reads just issued; tools/audit_hidden_loads.py checks every touch).
template <int PLANE> __device__ __forceinline__ void lds_val_issue2(uint32_t ad0, uint32_t ad1, uint32_t vaddr, half4* nlo, half4* nhi, uintx4& nv) {
    asm volatile("ds_read_b64_tr_b16 %0, %5\n\t"
                 "ds_read_b64_tr_b16 %1, %6\n\t"
                 "ds_read_b64_tr_b16 %2, %5 offset:%8\n\t"
                 "ds_read_b64_tr_b16 %3, %6 offset:%8\n\t"
                 "ds_read_b128 %4, %7"
                 : "=&v"(nlo[0]), "=&v"(nhi[0]), "=&v"(nlo[1]), "=&v"(nhi[1]), "=&v"(nv)
                 : "v"(ad0), "v"(ad1), "v"(vaddr), "i"(PLANE)
                 : "memory");
}
template <int PLANE> __device__ __forceinline__ void lds_val_step2(uint32_t ad0, uint32_t ad1, uint32_t vaddr, half4* nlo, half4* nhi, uintx4& nv,
                                                                   half4* clo, half4* chi, uintx4& cv) {
    asm volatile("ds_read_b64_tr_b16 %0, %10\n\t"
                 "ds_read_b64_tr_b16 %1, %11\n\t"
                 "ds_read_b64_tr_b16 %2, %10 offset:%13\n\t"
                 "ds_read_b64_tr_b16 %3, %11 offset:%13\n\t"
                 "ds_read_b128 %4, %12\n\t"
                 "s_waitcnt lgkmcnt(5)"
                 : "=&v"(nlo[0]), "=&v"(nhi[0]), "=&v"(nlo[1]), "=&v"(nhi[1]), "=&v"(nv), "+v"(clo[0]), "+v"(chi[0]), "+v"(clo[1]), "+v"(chi[1]), "+v"(cv)
                 : "v"(ad0), "v"(ad1), "v"(vaddr), "i"(PLANE)
                 : "memory");
}
// ... the same where the next tile may be switched off (a wavefront whose last window slot is empty): one statement, no
// compiler-made branch between a set's issue and its wait.  on == 0: nothing is issued, everything older is waited for.
template <int PLANE> __device__ __forceinline__ void lds_val_step_if2(uint32_t on, uint32_t ad0, uint32_t ad1, uint32_t vaddr, half4* nlo, half4* nhi, uintx4& nv,
                                                                      half4* clo, half4* chi, uintx4& cv) {
    asm volatile("v_cmp_eq_u32 vcc, 0, %14\n\t"
                 "s_cbranch_vccnz 1f\n\t"
                 "ds_read_b64_tr_b16 %0, %10\n\t"
                 "ds_read_b64_tr_b16 %1, %11\n\t"
                 "ds_read_b64_tr_b16 %2, %10 offset:%13\n\t"
                 "ds_read_b64_tr_b16 %3, %11 offset:%13\n\t"
                 "ds_read_b128 %4, %12\n\t"
                 "s_waitcnt lgkmcnt(5)\n\t"
                 "s_branch 2f\n\t"
                 "1:\n\t"
                 "s_waitcnt lgkmcnt(0)\n\t"
                 "2:"
                 : "=&v"(nlo[0]), "=&v"(nhi[0]), "=&v"(nlo[1]), "=&v"(nhi[1]), "=&v"(nv), "+v"(clo[0]), "+v"(chi[0]), "+v"(clo[1]), "+v"(chi[1]), "+v"(cv)
                 : "v"(ad0), "v"(ad1), "v"(vaddr), "i"(PLANE), "v"(on)
                 : "memory", "vcc");
}
__device__ __forceinline__ void lds_val_drain2(half4* clo, half4* chi, uintx4& cv) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(clo[0]), "+v"(chi[0]), "+v"(clo[1]), "+v"(chi[1]), "+v"(cv)
                 :
                 : "memory");
}

// a dense entry's tile (ordinary format): the four transposed reads, the next tile's id word and mask byte, this tile's 16 bytes of slot values
template <int PLANE> __device__ __forceinline__ void lds_val_cell_block2(uint32_t ad0, uint32_t ad1, uint32_t idaddr, uint32_t maddr, uint32_t vaddr,
                                                                         half4* lo, half4* hi, uint32_t& idw, uint32_t& m, uintx4& vv) {
    asm volatile("ds_read_b64_tr_b16 %0, %7\n\t"
                 "ds_read_b64_tr_b16 %1, %8\n\t"
                 "ds_read_b64_tr_b16 %2, %7 offset:%12\n\t"
                 "ds_read_b64_tr_b16 %3, %8 offset:%12\n\t"
                 "ds_read_b32 %4, %9 offset:128\n\t"
                 "ds_read_u8 %5, %10 offset:128\n\t"
                 "ds_read_b128 %6, %11\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(lo[0]), "=&v"(hi[0]), "=&v"(lo[1]), "=&v"(hi[1]), "=&v"(idw), "=&v"(m), "=&v"(vv)
                 : "v"(ad0), "v"(ad1), "v"(idaddr), "v"(maddr), "v"(vaddr), "i"(PLANE)
                 : "memory");
}
// afrag_from_byte as a select mask (all ones or 0 per half; flat_amask's arithmetic on a byte in a register)
__device__ __forceinline__ half8 amask_from_byte(uint32_t mb) {
    const uint32_t mm = mb | (mb << 16);
    uintx4 q;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const ushort2v k = {(unsigned short)(1u << (15 - 2 * j)), (unsigned short)(1u << (14 - 2 * j))};
        const short2v sh = __builtin_bit_cast(short2v, (ushort2v)(__builtin_bit_cast(ushort2v, mm) * k)) >> (short2v){15, 15};
        q[j] = __builtin_bit_cast(uint32_t, sh);
    }
    return __builtin_bit_cast(half8, q);
}

static constexpr int val_lds_bytes(int nt, int maxw) { return 2 * nt * lds_buf_rows(nt, maxw) * 32 + kLdsWaves * 2 * (maxw * 128) + kLdsWaves * 2 * (maxw * 64); }   // (the id / mask pads lie in FRONT of the value pads: the read behind the last id pad stays inside)

// spmm_lds_flat_kernel<2, 8, 1> with a value block per (pair, wavefront) beside the metadata block
__global__ __launch_bounds__(kLdsWaves * 64) void spmm_lds_val_kernel(const SpmmValArgs a) {
    if (range_is_wide_val(a.hdr)) return;   // (range guard: the fp32 fallback launched behind this kernel does the work)
    constexpr int NT = 2, MAXW = kLdsMaxW2, T = MAXW;
    constexpr int kLdsBufRows = lds_buf_rows(NT, MAXW), kLdsRows = kLdsBufRows - 8;
    constexpr int PADB = T * 128, PADV = T * 64, kLdsChunkDims = lds_chunk_dims(MAXW);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int PLANEB = kLdsBufRows * 32, BUFB = NT * PLANEB;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, i = lane & 15;
    const int wg = blockIdx.x;
    const int chunk_id = a.chunk0 + (int)blockIdx.y;
    const int coloff = chunk_id * kLdsChunkDims;
    const uint32_t lds0 = (uint32_t)(uintptr_t)((LDS_AS char*)smem);
    const uint32_t pad0 = lds0 + 2 * BUFB + (uint32_t)wave * (2 * PADB);
    const uint32_t vpad0 = lds0 + 2 * BUFB + kLdsWaves * 2 * PADB + (uint32_t)wave * (2 * PADV);
    const int kx = scale_exp_from_bits(a.hdr[kHdrMaxX]), ka = scale_exp_from_bits(a.hdr[kHdrMaxVal]);

    int wj[MAXW];
    floatx4 acc[MAXW][NT];
#pragma unroll
    for (int j = 0; j < MAXW; ++j) {
        wj[j] = __builtin_amdgcn_readfirstlane(a.order[cell_position(wg, wave, j, MAXW)]);
#pragma unroll
        for (int s = 0; s < NT; ++s) acc[j][s] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    const bool last_valid = wj[MAXW - 1] >= 0;
    const uint32_t last_on = (uint32_t)__builtin_amdgcn_readfirstlane(last_valid ? 1 : 0);
    const uint32_t lanebase = lds0 + (uint32_t)(i & 3) * 8u;
    const uint32_t idoff = (uint32_t)(4 * g + (i >> 2)) * (uint32_t)(T * 4);
    const uint32_t moff = (uint32_t)(64 * T) + (uint32_t)lane * (uint32_t)T;
    const uint32_t voff = (uint32_t)g * 16u;                            // this lane's K group inside a tile's 64 bytes of values
    // (the fill quota of spmm_lds_flat_kernel - the wavefronts with an empty last slot take the fills - measured here in r05: 822 -> 827 us, not kept)
    const FlatRangeFiller<NT, kLdsBufRows> filler(a.x16, a.xrows, chunk_id * (kLdsChunkDims / 16), a.stride, wave, kLdsWaves, lane);
    const int rb = a.rbase[wg], nr = a.rbase[wg + 1] - rb;
    const char* const bb0 = reinterpret_cast<const char*>(a.blocks) + ((int64_t)rb * kLdsWaves + wave) * PADB;
    const char* const vb0 = reinterpret_cast<const char*>(a.vals) + ((int64_t)rb * kLdsWaves + wave) * PADV;
    const uint32_t lane16 = (uint32_t)lane * 16u;
    auto meta_dma = [&](int r, uint32_t padaddr, uint32_t vpadaddr) {   // metadata block (1 KB) and value block (512 B) of pair rb + r
        __builtin_amdgcn_global_load_lds((GLB_AS const void*)(bb0 + (int64_t)r * (kLdsWaves * PADB) + lane16), (LDS_AS void*)(uintptr_t)padaddr, 16, 0, 0);
        if (lane16 < (uint32_t)PADV)
            __builtin_amdgcn_global_load_lds((GLB_AS const void*)(vb0 + (int64_t)r * (kLdsWaves * PADV) + lane16), (LDS_AS void*)(uintptr_t)vpadaddr, 16, 0, 0);
    };
    const uint32_t* const rlp = a.rl2 + (int64_t)rb * 4;   // (entry records and descriptor words: as spmm_lds_flat_kernel)
    auto load_info = [&](int r_) -> uintx2 { return *reinterpret_cast<const uintx2*>(rlp + (int64_t)r_ * 4); };   // (both words are read: see spmm_lds_flat_kernel)
    const uint32_t* const dscp = a.rl2 + (int64_t)a.nent * 4 + ((int64_t)rb * kLdsWaves + wave);
    auto load_desc = [&](int r_) -> uint32_t { return dscp[(int64_t)r_ * kLdsWaves]; };
    uint32_t ew0 = 0u, ew1 = 0u, ew2 = ~0u;     // the current entry's words; the next entry's in flight (as spmm_lds_flat_kernel)
    uintx2 einfo = {0u, ~0u};
    if (nr > 0) {
        const uintx2 e0 = load_info(0);
        ew0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)e0[0]);
        ew2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)e0[1]);
        meta_dma(0, pad0, vpad0);
        if (nr > 1) meta_dma(1, pad0 + PADB, vpad0 + PADV);
        filler.fill((int)(ew0 & 0x3fffffffu) * kLdsRows, lds0);
        einfo = load_info(nr > 1 ? 1 : 0);
    }
    wait_vm0();
    __syncthreads();
    uint32_t buf = 0u;
    int r = 0;
    uint32_t dnext = 0u;
    auto entry_end = [&](uint32_t padaddr, uint32_t vpadaddr, bool dense_phase) {
        wait_vm0();   // the range fetched at the top has landed (this wavefront's share), the blocks of entry r + 1 and its words
        const bool more = r + 2 < nr;
        ew0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)einfo[0]);
        ew2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)einfo[1]);
        if (dense_phase) ew1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)dnext);
        if (ew0 & 0x40000000u) buf ^= 1u;
        if (more) {
            einfo = load_info(r + 2);
            if (dense_phase) dnext = load_desc(r + 2);
            meta_dma(r + 2, padaddr, vpadaddr);            // into the pads this entry has just finished with
        }
        __builtin_amdgcn_s_barrier();
    };
    for (; r < nr && !(ew0 >> 31); ++r) {   // ---- normal entries (as spmm_lds_flat_kernel: normal entries first, then the dense ones)
        if (ew2 != ~0u) filler.fill((int)ew2 * kLdsRows, lds0 + (buf ^ 1u) * BUFB);
        const uint32_t padaddr = pad0 + (uint32_t)(r & 1) * PADB, vpadaddr = vpad0 + (uint32_t)(r & 1) * PADV, bb = lanebase + buf * BUFB;
        {
            FlatMeta<T> m;
            flat_meta_block<T>(padaddr + idoff, padaddr + moff, m);
            half4 lo[2][NT], hi[2][NT];
            uintx4 vv[2];
            const uint32_t vbase = vpadaddr + voff;
            lds_val_issue2<PLANEB>(bb + (m.idw[0] & 0xffffu), bb + (m.idw[0] >> 16), vbase, lo[0], hi[0], vv[0]);
#pragma unroll
            for (int x = 0; x < T; ++x) {
                if (x == MAXW - 1 && !last_valid) break;           // (slots fill in order: an empty one is the last; nothing is in flight here: lds_val_step_if2)
                set_wave_priority(3 - x * 4 / MAXW);
                const int cs = x & 1, ns = (x + 1) & 1;
                if (x + 1 < T && x + 1 == MAXW - 1)                // the step in front of the last slot: its reads only if the slot holds a window
                    lds_val_step_if2<PLANEB>(last_on, bb + (m.idw[x + 1] & 0xffffu), bb + (m.idw[x + 1] >> 16), vbase + (uint32_t)(x + 1) * 64u, lo[ns], hi[ns], vv[ns], lo[cs], hi[cs], vv[cs]);
                else if (x + 1 < T)
                    lds_val_step2<PLANEB>(bb + (m.idw[x + 1] & 0xffffu), bb + (m.idw[x + 1] >> 16), vbase + (uint32_t)(x + 1) * 64u, lo[ns], hi[ns], vv[ns], lo[cs], hi[cs], vv[cs]);
                else lds_val_drain2(lo[cs], hi[cs], vv[cs]);
                half8 af;
                switch (x & 3) {
                    case 0: af = flat_amask<0>(m.mk[x >> 2]); break;
                    case 1: af = flat_amask<1>(m.mk[x >> 2]); break;
                    case 2: af = flat_amask<2>(m.mk[x >> 2]); break;
                    default: af = flat_amask<3>(m.mk[x >> 2]); break;
                }
                af = __builtin_bit_cast(half8, __builtin_bit_cast(uintx4, af) & vv[cs]);   // all-ones or 0 AND the slot values: the value itself, any magnitude
#pragma unroll
                for (int s = 0; s < NT; ++s) {
                    const half8 bf = __builtin_shufflevector(lo[cs][s], hi[cs][s], 0, 1, 2, 3, 4, 5, 6, 7);
                    acc[x][s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf, acc[x][s], 0, 0, 0);
                }
            }
        }
        entry_end(padaddr, vpadaddr, false);
    }
    if (r < nr) {   // the descriptor words of the first two dense entries
        const uint32_t d0 = load_desc(r), d1 = load_desc(r + 1 < nr ? r + 1 : r);
        wait_vm0();
        ew1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)d0);
        dnext = d1;
    }
    for (; r < nr; ++r) {                   // ---- dense entries: ordinary-format tiles, ew1 = tiles per window slot; a tile's 64 bytes of slot values beside it
        if (ew2 != ~0u) filler.fill((int)ew2 * kLdsRows, lds0 + (buf ^ 1u) * BUFB);
        const uint32_t padaddr = pad0 + (uint32_t)(r & 1) * PADB, vpadaddr = vpad0 + (uint32_t)(r & 1) * PADV, bb = lanebase + buf * BUFB;
        {
            const uint32_t l2 = lane_id_now();
            const uint32_t gd = l2 >> 4, id_ = l2 & 15u;
            uint32_t idaddr = padaddr + (4u * gd + (id_ >> 2)) * 4u, maddr = padaddr + 64u + id_ * 4u + gd, vaddr = vpadaddr + gd * 16u, idw, mb;
            lds_cell_ids(idaddr, maddr, idw, mb);
#pragma unroll
            for (int j = 0; j < MAXW; ++j) {
                const int nj = (int)((ew1 >> (4 * j)) & 15u);
                if (nj) {
                    floatx4 cacc[NT];
#pragma unroll
                    for (int s = 0; s < NT; ++s) cacc[s] = floatx4{0.f, 0.f, 0.f, 0.f};
                    for (int t = 0; t < nj; ++t) {
                        const uint32_t ad0 = bb + (idw & 0xffffu), ad1 = bb + (idw >> 16);
                        const half8 am = amask_from_byte(mb);
                        half4 lo[NT], hi[NT];
                        uint32_t nidw, nmb;
                        uintx4 vv;
                        lds_val_cell_block2<PLANEB>(ad0, ad1, idaddr, maddr, vaddr, lo, hi, nidw, nmb, vv);
                        const half8 af = __builtin_bit_cast(half8, __builtin_bit_cast(uintx4, am) & vv);
#pragma unroll
                        for (int s = 0; s < NT; ++s) {
                            const half8 bf = __builtin_shufflevector(lo[s], hi[s], 0, 1, 2, 3, 4, 5, 6, 7);
                            cacc[s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf, cacc[s], 0, 0, 0);
                        }
                        idw = nidw; mb = nmb;
                        idaddr += 128u; maddr += 128u; vaddr += 64u;
                    }
#pragma unroll
                    for (int s = 0; s < NT; ++s) acc[j][s] += cacc[s];
                }
            }
        }
        entry_end(padaddr, vpadaddr, true);
    }
    __builtin_amdgcn_s_setprio(0);
    // (ADVICE r04: the A fragment used to be 2.0 x value in fp16 - a maximum whose mantissa rounds up to 2^15 became 65536 = inf, about
    //  one call in 2048; it is now the value itself, selected by an all-ones mask.  And |kx + ka| may exceed 126: two factors, like
    //  the gather walks' epilogue, tcgnn_gather_spmm.inc)
    const float inv1 = pow2f(-kx), inv2 = pow2f(-ka);
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
                    if (row0 + ii < a.N) a.y[(row0 + ii) * a.D + colg] = acc[j][s][ii] * inv1 * inv2;
            }
        }
    }
}

// (as lds_geom: eight windows a wavefront, two planes a pass)
static constexpr LaunchGeom val_geom() { return {kLdsWaves * 64, val_lds_bytes(2, kLdsMaxW2), kLdsWaves / 4, kLdsMaxW2}; }
static_assert(val_geom().lds_bytes <= 160 * 1024, "LDS of the edge-valued flat walk");
static hipError_t launch_lds_val(const SpmmValArgs& args, int nchunks, hipStream_t stream) {
    return launch_kernel<spmm_lds_val_kernel, val_geom().lds_bytes>(dim3((unsigned)args.nwg, (unsigned)nchunks), val_geom(), stream, args);
}

// The cold remainder of the edge-valued walk: spmm_cold_planar_kernel with a value per tile slot (lane k & 31 holds slot k's value,
// handed round like the column ids).  Y += sum (x 2^-(kx + ka)).
struct ColdValArgs {
    const int64_t* cold_ptr;
    const int32_t* ccols;
    const uint32_t* cmask;
    const _Float16* cvals;      // [tiles][32]
    const _Float16* x16;
    const uint32_t* hdr;
    float* y;
    int32_t N, D, xrows, nw, col0, ncols;
};
__global__ __launch_bounds__(256, 2) void spmm_cold_val_kernel(const ColdValArgs a) {
    if (range_is_wide_val(a.hdr)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int w = blockIdx.x * 4 + wave;
    if (w >= a.nw) return;
    const int64_t t0 = a.cold_ptr[w], t1 = a.cold_ptr[w + 1];
    if (t0 == t1) return;
    const int r = lane >> 2, q = lane & 3;
    const int plane = (a.col0 >> 4) + (int)blockIdx.y * 4 + q;
    const bool live = plane * 16 < a.col0 + a.ncols && plane * 16 < ((a.D + 15) & ~15);
    float acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
    const int zrow = a.xrows - 1;
    const half8* xp = reinterpret_cast<const half8*>(a.x16 + (int64_t)(live ? plane : 0) * a.xrows * 16);
    for (int64_t t = t0; t < t1; ++t) {
        const int32_t cv = a.ccols[t * kWbCols + (lane & 31)];
        const float vv = (float)a.cvals[t * 32 + (lane & 31)];
        uint32_t mv = a.cmask[t * kWinRows + r];
        while (__any(mv != 0u)) {
            const bool v = mv != 0u;
            const int k = v ? __builtin_ctz(mv) : 0;
            mv &= mv - 1u;
            const int cc = __shfl(cv, k);
            const float sv = __shfl(vv, k);
            const float av = v ? sv : 0.0f;
            const int c = (v && live && cc < zrow) ? cc : zrow;
            const half8 x0 = xp[(int64_t)c * 2], x1 = xp[(int64_t)c * 2 + 1];
#pragma unroll
            for (int e = 0; e < 8; ++e) { acc[e] += av * (float)x0[e]; acc[8 + e] += av * (float)x1[e]; }
        }
    }
    const int64_t row = (int64_t)w * kWinRows + r;
    if (!live || row >= a.N) return;
    const float inv = pow2f(-scale_exp_from_bits(a.hdr[kHdrMaxX])), inv2 = pow2f(-scale_exp_from_bits(a.hdr[kHdrMaxVal]));   // (|kx + ka| may exceed 126: two factors)
    float* dst = a.y + row * a.D + plane * 16;
    if (plane * 16 + 16 <= a.D && (a.D & 3) == 0) {
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4) {
            float4 v = reinterpret_cast<float4*>(dst)[e4];
            v.x += acc[4 * e4] * inv * inv2; v.y += acc[4 * e4 + 1] * inv * inv2; v.z += acc[4 * e4 + 2] * inv * inv2; v.w += acc[4 * e4 + 3] * inv * inv2;
            reinterpret_cast<float4*>(dst)[e4] = v;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 16; ++e)
            if (plane * 16 + e < a.D) dst[e] += acc[e] * inv * inv2;
    }
}
