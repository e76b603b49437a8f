// tcgnn_heads.inc - the multi-head edge-valued SpMM (tcgnn_spmm_heads): Y[:, hF:(h+1)F] = A_val(edge_val[h, :]) X[:, hF:(h+1)F], one
// gather of the neighbour rows and one metadata DMA per tile feeding every head of a pass.  Included by tcgnn_device.hip behind
// tcgnn_gather_spmm.inc (and tcgnn_small_fallback.inc), whose TileWalker it is built on and whose pipeline discipline it keeps (no VGPR has a load in flight
// outside one asm statement).  Host side: route_heads / run_spmm_heads in tcgnn_spmm_dispatch.inc.
//
// A PASS (blockIdx.y) takes G whole heads of F = 8 FB columns each: the gather fetches only those G F columns of every source row,
// as NT = ceil(G F / 16) 16-column slices.  The B side is TileWalker's, unchanged.  The A side is one fragment per head, built from
// that head's row of edge_val; slice s is multiplied by the fragment of the head that owns its columns.  Where F is not a multiple
// of 16 a slice can hold the columns of two heads (lanes i < 8: one head, i >= 8: the next).  In v_mfma_f32_16x16x32_f16 lane
// (g, i) holds B column i and C column i, so an output column depends only on its own B lanes: such a slice is multiplied TWICE,
// once per head, into two accumulators, and the store takes columns i < 8 from the first and i >= 8 from the second.  (The other
// way - zeroing the other head's B lanes and adding into one accumulator - costs eight VALU instructions per mixed slice and tile
// in a loop that is VALU-bound; this way costs four accumulator registers per mixed slice, at most two slices, and nothing in the loop.)
//
// Edge values: per lane the run of its byte of row i, fetched by LDS-DMA one tile ahead exactly as TileWalker::dma_vals does - the
// run starts at the same CSR offset in every head's row, so the offsets, the clamp, the "second DMA" decision and the eight LDS
// read addresses are computed once per tile and the heads differ by an immediate offset (2 KB per head and wavefront).
//
// What bounds a pass (DESIGN.md 4.11): G <= kMaxHeadsPerPass = 4 and G F <= kMaxHeadsPassDims = 64, so a wavefront holds at most
// 2 x 4 KB of tile buffers + 256 B + 4 x 2 KB of values = 16.25 KB and a four-wavefront workgroup 65 KB: two workgroups per CU at
// the worst shape (4 x 16), three at 8 heads of 8 (two passes of 4: 49 KB).  One pass of all eight heads would be 97 KB - one
// workgroup per CU.  A pass of ONE head (a remainder: 9 x 16 = 4 + 4 + 1) exists; widths at which every pass would be one - F > 32 -
// are not routed here (heads_per_pass): nothing would be shared.
struct SpmmHeadsArgs {
    SpmmArgs base;   // D = H F (= ldy), edge_val = [H][E] head-major; chunk0, relu, w, accumulate, unguarded unused (0)
    int32_t head0;   // first head of pass 0 of this launch (pass p: head0 + p G)
};

static constexpr int kMaxHeadsPerPass = 4, kMaxHeadsPassDims = 64, kHeadValBytes = 2048;

// eight 4-byte LDS reads at per-lane addresses + an immediate offset (the head's value pad), retired inside the statement
template <int OFF>
__device__ __forceinline__ void lds_read8_b32_at(const uint32_t (&ad)[8], uint32_t (&v)[8]) {
    asm volatile("ds_read_b32 %0, %8 offset:%16\n\t"
                 "ds_read_b32 %1, %9 offset:%16\n\t"
                 "ds_read_b32 %2, %10 offset:%16\n\t"
                 "ds_read_b32 %3, %11 offset:%16\n\t"
                 "ds_read_b32 %4, %12 offset:%16\n\t"
                 "ds_read_b32 %5, %13 offset:%16\n\t"
                 "ds_read_b32 %6, %14 offset:%16\n\t"
                 "ds_read_b32 %7, %15 offset:%16\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7])
                 : "v"(ad[0]), "v"(ad[1]), "v"(ad[2]), "v"(ad[3]), "v"(ad[4]), "v"(ad[5]), "v"(ad[6]), "v"(ad[7]), "i"(OFF)
                 : "memory");
}

template <int G, int FB>
struct HeadsWalker : TileWalker<(G * FB + 1) / 2, true, 2> {
    static constexpr int HALVES = G * FB;            // 8-column half slices of the pass
    static constexpr int NT = (HALVES + 1) / 2;
    using Base = TileWalker<NT, true, 2>;
    using Cur = typename Base::Cur;
    static constexpr int NIDS = Base::NIDS;
    static constexpr int WAVE_LDS = 2 * Base::TILE_BYTES + kPadBytes + G * kHeadValBytes;   // tile buffers, metadata pad, one value pad per head
    // head (of the pass) that owns half slice j; the half slice behind the last one (HALVES odd) holds padding columns only
    static constexpr int head_of(int j) { return (j < HALVES ? j : HALVES - 1) / FB; }
    static constexpr bool mixed(int s) { return 2 * s + 1 < HALVES && head_of(2 * s) != head_of(2 * s + 1); }
    const float* val0;   // first head of the pass: its row of edge_val
    int64_t E;

    __device__ __forceinline__ HeadsWalker(const SpmmArgs& args, char* wave_lds, int coloff, float sa_, int head0)
        : Base(args, wave_lds, wave_lds, coloff, sa_), val0(args.edge_val + (int64_t)head0 * args.E), E(args.E) {}

    // TileWalker::dma_vals for every head of the pass: one run offset, G (2 G) DMAs
    __device__ __forceinline__ void dma_vals(Cur& c) const {
        const int g = this->g;
        const int64_t e0 = (int64_t)c.eb + __popc(c.m & ((1u << (8 * g)) - 1u));
        int64_t lo = e0 < E - 8 ? e0 : E - 8;
        if (lo < 0) lo = 0;
        c.shift = (int)(e0 - lo);
        c.wide = E >= 8 && __any(__popc((c.m >> (8 * g)) & 0xffu) + c.shift > 4);
#pragma unroll
        for (int k = 0; k < G; ++k) {
            const float* src = val0 + (int64_t)k * E + lo;
            __builtin_amdgcn_global_load_lds((GLB_AS const void*)src, (LDS_AS void*)(uintptr_t)(this->vpad + (uint32_t)(k * kHeadValBytes)), 16, 0, 0);
            if (c.wide) __builtin_amdgcn_global_load_lds((GLB_AS const void*)(src + 4), (LDS_AS void*)(uintptr_t)(this->vpad + (uint32_t)(k * kHeadValBytes) + 1024u), 16, 0, 0);
        }
    }
    // head k's A fragment from the eight values read by address (slow: fewer than eight edges in the whole matrix - ordinary loads)
    __device__ __forceinline__ half8 a_fragment(const Cur& cur, const uint32_t (&sv)[8], int k, bool slow) const {
        half8 af;
        const int g = this->g;
        const uint32_t mb = (cur.m >> (8 * g)) & 0xffu;
        if (__builtin_expect(slow, 0)) {
            const float* val = val0 + (int64_t)k * E + (int64_t)cur.eb + __popc(cur.m & ((1u << (8 * g)) - 1u));
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool on = (mb >> j) & 1u;
                const float v = on ? val[__popc(mb & ((1u << j) - 1u))] * this->sa : 0.0f;
                af[j] = to_half_rna(v);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) af[j] = ((mb >> j) & 1u) ? to_half_rna(__uint_as_float(sv[j]) * this->sa) : (_Float16)0.0f;
        }
        return af;
    }
    template <int K> __device__ __forceinline__ void read_heads(const uint32_t (&ad)[8], uint32_t (&sv)[G][8]) const {
        if constexpr (K < G) {
            lds_read8_b32_at<K * kHeadValBytes>(ad, sv[K]);
            read_heads<K + 1>(ad, sv);
        }
    }
    // slice S by the fragment of the head that owns it - by both heads' where it holds columns of two
    template <int S> __device__ __forceinline__ void mfma_heads(const half8 (&af)[G], const half4 (&lo)[NT], const half4 (&hi)[NT], floatx4 (&acc)[NT], floatx4 (&acc2)[NT]) const {
        if constexpr (S < NT) {
            const half8 bf = __builtin_shufflevector(lo[S], hi[S], 0, 1, 2, 3, 4, 5, 6, 7);
            acc[S] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[head_of(2 * S)], bf, acc[S], 0, 0, 0);
            if constexpr (mixed(S)) acc2[S] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[head_of(2 * S + 1)], bf, acc2[S], 0, 0, 0);
            mfma_heads<S + 1>(af, lo, hi, acc, acc2);
        }
    }

    // TileWalker::stage with G value pads: after ONE wait the ids of the next tile and every head's values of this one are read from
    // LDS, the next gather, the next values and the metadata of the tile after that are issued, and tile t is multiplied underneath.
    template <int BUF>
    __device__ __forceinline__ bool stage(int64_t& t, int64_t& tn, const int64_t te, const int64_t step, Cur& cur, floatx4 (&acc)[NT], floatx4 (&acc2)[NT]) const {
        wait_vm0();
        uint32_t v[NIDS];
        uintx4 q;
        const uint32_t vbase = this->vpad + (uint32_t)this->lane * 16u;
        lds_ids_block<NIDS>(this->idaddr, v, vbase, q);   // (the 16-byte read is a dummy here)
        const uint32_t mb = (cur.m >> (8 * this->g)) & 0xffu;
        uint32_t va = vbase + ((uint32_t)cur.shift << 2), ad[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            ad[j] = va;
            va -= (uint32_t)((int32_t)(mb << (31 - j)) >> 31) << 2;                 // + 4 where the edge exists
        }
        if (cur.wide) {   // (wave-uniform: some lane's run crosses into the second block of four)
#pragma unroll
            for (int j = 0; j < 8; ++j) ad[j] += (((ad[j] - vbase) >> 4) & 1u) * 1008u;
        }
        uint32_t sv[G][8];
        read_heads<0>(ad, sv);                            // (before the next tile's values overwrite the pads)
        const bool slow = !cur.wide && __any(__popc(mb) + cur.shift > 4);
        const bool more = tn < te;
        Cur nx;
        nx.m = v[NT];
        nx.eb = v[NT + 1];
        nx.shift = 0;
        nx.wide = false;
        const int64_t tnn = tn + step;
        if (more) {
            this->template dma_gather<BUF ^ 1>(v);
            dma_vals(nx);
            if (tnn < te) this->meta.dma(tnn, this->pad);   // metadata two tiles ahead
        }
        half8 af[G];
#pragma unroll
        for (int k = 0; k < G; ++k) af[k] = a_fragment(cur, sv[k], k, slow);
        half4 lo[NT], hi[NT];
        lds_tr_block<NT, BUF * Base::TILE_BYTES>(this->raddr, lo, hi);
        mfma_heads<0>(af, lo, hi, acc, acc2);
        cur = nx;
        t = tn;
        tn = tnn;
        return more;
    }

    // acc (+ acc2 for the mixed slices) += A_h(tiles t, t + step, ... < te) * X16 rows, for every head h of the pass
    __device__ __forceinline__ void walk(int64_t t, const int64_t te, const int64_t step, floatx4 (&acc)[NT], floatx4 (&acc2)[NT]) const {
        if (t >= te) return;
        this->meta.dma(t, this->pad);
        wait_vm0();
        uint32_t v[NIDS];
        uintx4 q;
        lds_ids_block<NIDS>(this->idaddr, v, this->ring, q);   // (the 16-byte read is a dummy here)
        Cur cur;
        cur.m = v[NT];
        cur.eb = v[NT + 1];
        cur.shift = 0;
        cur.wide = false;
        this->template dma_gather<0>(v);
        dma_vals(cur);
        int64_t tn = t + step;
        if (tn < te) this->meta.dma(tn, this->pad);
        for (;;) {   // ping-pong over the two tile buffers: static LDS offsets, no register rotation
            if (!stage<0>(t, tn, te, step, cur, acc, acc2)) break;
            if (!stage<1>(t, tn, te, step, cur, acc, acc2)) break;
        }
    }
};

// One workgroup per (window, pass); 1 or 4 wavefronts (blockDim.x / 64: the plan's workgroup shape) share the window's tiles round-robin
// and their partial sums are combined through LDS in wavefront order.  (second launch-bound argument: as spmm_kernel's)
template <int G, int FB>
static constexpr LaunchGeom heads_geom(int waves) { return {waves * 64, waves * HeadsWalker<G, FB>::WAVE_LDS, HeadsWalker<G, FB>::NT <= 4 ? 4 : 2, 0}; }
template <int G, int FB>
__global__ __launch_bounds__((heads_geom<G, FB>(4).threads), (heads_geom<G, FB>(4).waves_per_simd)) void spmm_heads_kernel(const SpmmHeadsArgs h) {
    const SpmmArgs& a = h.base;
    if (range_is_wide_val(a.hdr)) return;   // (range guard, the whole call: spmm_heads_wide_fallback_kernel, launched behind this kernel, does the work)
    using HW = HeadsWalker<G, FB>;
    constexpr int NT = HW::NT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nwaves = (int)(blockDim.x >> 6);
    const int g = lane >> 4, i = lane & 15;
    const int w = a.order[blockIdx.x];
    const int head0 = h.head0 + (int)blockIdx.y * G;
    const int coloff = head0 * (FB * 8);   // first feature column of this pass (a multiple of 16: route_heads only forms such passes)
    const int64_t tb = a.wb_ptr[w], te = a.wb_ptr[w + 1];
    const int kx = scale_exp_from_bits(a.hdr[kHdrMaxX]);
    const int ka = scale_exp_from_bits(a.hdr[kHdrMaxVal]);

    floatx4 acc[NT], acc2[NT];
#pragma unroll
    for (int s = 0; s < NT; ++s) acc[s] = acc2[s] = floatx4{0.f, 0.f, 0.f, 0.f};
    {
        const HW hw(a, smem + wave * HW::WAVE_LDS, coloff, pow2f(ka), head0);
        hw.walk(tb + wave, te, nwaves, acc, acc2);
    }
#pragma unroll
    for (int s = 0; s < NT; ++s)
        if (HW::mixed(s) && i >= 8) acc[s] = acc2[s];

    // ---- combine the wavefronts' partial sums in a fixed order and store (every row of the window: an empty sum stores 0)
    const float inv1 = pow2f(-kx), inv2 = pow2f(-ka);   // |kx + ka| may exceed 126: two factors
    const int64_t row0 = (int64_t)w * kWinRows + 4 * g;
    if (nwaves > 1) {
        __syncthreads();   // every wave is done with its tile buffers
        floatx4* red = reinterpret_cast<floatx4*>(smem);
#pragma unroll
        for (int s = 0; s < NT; ++s) red[(wave * NT + s) * 64 + lane] = acc[s];
        __syncthreads();
        for (int s = wave; s < NT; s += nwaves) {
            floatx4 v = red[s * 64 + lane];
            for (int ww = 1; ww < nwaves; ++ww) {
                const floatx4 o = red[(ww * NT + s) * 64 + lane];
                v[0] += o[0]; v[1] += o[1]; v[2] += o[2]; v[3] += o[3];
            }
            const int colg = coloff + 16 * s + i;
            if (colg < a.D) {
#pragma unroll
                for (int ii = 0; ii < 4; ++ii)
                    if (row0 + ii < a.N) a.y[(row0 + ii) * a.ldy + colg] = v[ii] * inv1 * inv2;
            }
        }
    } else {
#pragma unroll
        for (int s = 0; s < NT; ++s) {
            const int colg = coloff + 16 * s + i;
            if (colg < a.D) {
#pragma unroll
                for (int ii = 0; ii < 4; ++ii)
                    if (row0 + ii < a.N) a.y[(row0 + ii) * a.ldy + colg] = acc[s][ii] * inv1 * inv2;
            }
        }
    }
}

// every head of a plan the tile stream cannot serve with edge values (rows not strictly increasing, or fewer than four edges): plain
// fp32 in CSR order with the reference's operand rounding, as spmm_val_csr_kernel does for one head - here all of them in one launch
__global__ __launch_bounds__(256) void spmm_heads_csr_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ val,
                                                             const float* __restrict__ X, float* __restrict__ Y, int32_t N, int32_t H, int32_t F, int64_t E) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const int lane = threadIdx.x & 63;
    const int64_t D = (int64_t)H * F;
    const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
    for (int64_t d = lane; d < D; d += 64) {
        const float* v = val + (d / F) * E;
        float s = 0.f;
        for (int64_t e = e0; e < e1; ++e) s += round_rna10(v[e]) * round_rna10(X[(int64_t)col[e] * D + d]);
        Y[row * D + d] = s;
    }
}

// the range guard's fp32 way for every head in ONE launch behind spmm_heads_kernel (grid.y = head): spmm_wide_fallback_kernel's body on
// the head's columns of X and Y (row stride ld = H F) and its row of edge values; returns at once unless the call is "wide"
__global__ __launch_bounds__(256) void spmm_heads_wide_fallback_kernel(const uint32_t* __restrict__ hdr, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                       const float* __restrict__ val, const float* __restrict__ X, float* __restrict__ Y, int32_t N, int32_t F,
                                                                       int64_t E, int64_t ld) {
    const int64_t h = blockIdx.y;
    spmm_wide_fallback_body<false>(hdr, 1, rowptr, col, val + h * E, nullptr, X + h * F, nullptr, Y + h * F, N, F, ld, ld, 0, 0, nullptr, Epi{nullptr, nullptr});
}

// spmm_heads_kernel: G whole heads of 8 FB columns per pass - the shapes heads_per_pass (tcgnn_spmm_dispatch.inc) forms, full passes and remainders
template <int G, int FB>
static hipError_t launch_heads_one(const SpmmHeadsArgs& args, int waves, int nwin, int npass, hipStream_t stream) {
    // (four wavefronts of a 4 x 16 pass hold 65 KB: the ceiling is raised to what four need, whatever this plan's workgroup shape)
    return launch_kernel<spmm_heads_kernel<G, FB>, heads_geom<G, FB>(4).lds_bytes>(dim3((unsigned)nwin, (unsigned)npass), heads_geom<G, FB>(waves), stream, args);
}
static hipError_t launch_heads_any(int g, int fb, const SpmmHeadsArgs& args, int waves, int nwin, int npass, hipStream_t stream) {
#define TCGNN_HEADS_CASE(G, FB) case (G) * 100 + (FB): return launch_heads_one<G, FB>(args, waves, nwin, npass, stream)
    switch (g * 100 + fb) {
        TCGNN_HEADS_CASE(1, 1); TCGNN_HEADS_CASE(2, 1); TCGNN_HEADS_CASE(3, 1); TCGNN_HEADS_CASE(4, 1);   // F = 8
        TCGNN_HEADS_CASE(1, 2); TCGNN_HEADS_CASE(2, 2); TCGNN_HEADS_CASE(3, 2); TCGNN_HEADS_CASE(4, 2);   // F = 16
        TCGNN_HEADS_CASE(1, 3); TCGNN_HEADS_CASE(2, 3);                                                   // F = 24
        TCGNN_HEADS_CASE(1, 4); TCGNN_HEADS_CASE(2, 4);                                                   // F = 32
        default: return hipErrorInvalidValue;
    }
#undef TCGNN_HEADS_CASE
}
