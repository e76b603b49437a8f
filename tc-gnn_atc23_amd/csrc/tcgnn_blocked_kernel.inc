// tcgnn_blocked_kernel.inc - the body of spmm_blocked_kernel (tcgnn_gather_spmm.inc), included twice: as the plain kernel and as
// spmm_blocked_epi_kernel, the same walk with tcgnn_spmm_scaled's row scale / bias in the final store.  The macros expand, for the
// plain kernel, to exactly the tokens it was written with, so its code does not change.
template <int NT, int MAXW, bool VAL>
__global__ __launch_bounds__(blocked_geom(NT, VAL).threads, blocked_geom(NT, VAL).waves_per_simd) void TCGNN_KERNEL_NAME(TCGNN_KERNEL_PARAM) {
    TCGNN_KERNEL_PROLOGUE
    if (!b.base.unguarded && (VAL ? range_is_wide_val(b.base.hdr) : range_is_wide(b.base.hdr, 0))) return;   // (range guard: the fp32 fallback launched behind this kernel does the work)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const SpmmArgs& a = b.base;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, i = lane & 15;
    const int coloff = (a.chunk0 + (int)blockIdx.y) * kMaxChunkDims;
    const int kx = scale_exp_from_bits(a.hdr[kHdrMaxX]);
    const int ka = VAL ? scale_exp_from_bits(a.hdr[kHdrMaxVal]) : 0;
    const float inv1 = pow2f(-kx), inv2 = VAL ? pow2f(-ka) : 1.0f;
    using TW = TileWalker<NT, VAL>;
    char* atab = smem + 4 * TW::WAVE_LDS;
    fill_afrag_table(atab);
    __syncthreads();
    const TW tw(a, smem + wave * TW::WAVE_LDS, atab, coloff, pow2f(ka));

    const int gw = blockIdx.x * 4 + wave, gwn = gridDim.x * 4;
    for (int grp = gw; grp < b.ngroups; grp += gwn) {
        int wj[MAXW];
        int64_t tbj[MAXW];
        uint32_t done[MAXW];
        floatx4 acc[MAXW][NT];
#pragma unroll
        for (int j = 0; j < MAXW; ++j) {
            const int idx = grp + j * b.ngroups;   // strided picks from the heaviest-first order: balanced groups
            wj[j] = idx < b.nw ? __builtin_amdgcn_readfirstlane(a.order[idx]) : -1;
            tbj[j] = wj[j] >= 0 ? a.wb_ptr[wj[j]] : 0;
            done[j] = 0;
#pragma unroll
            for (int s = 0; s < NT; ++s) acc[j][s] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
        int64_t pad_tile = -1;
        // run q = (range r, window j); its bounds are looked up one run ahead so the walk can prefetch
        // the ids of the next run's first tile while it finishes the current one
        uint32_t nend[MAXW];
#pragma unroll
        for (int j = 0; j < MAXW; ++j) nend[j] = wj[j] >= 0 ? b.bptr[(int64_t)wj[j] * (b.nbuckets + 1) + b.gsel] : 0u;
        for (int r = 0; r < b.nranges; ++r) {
            uint32_t end[MAXW], after[MAXW];
#pragma unroll
            for (int j = 0; j < MAXW; ++j) {
                end[j] = nend[j];
                after[j] = (wj[j] >= 0 && r + 1 < b.nranges) ? b.bptr[(int64_t)wj[j] * (b.nbuckets + 1) + (int64_t)(r + 2) * b.gsel] : end[j];
                nend[j] = after[j];
            }
#pragma unroll
            for (int j = 0; j < MAXW; ++j) {
                if (wj[j] < 0) continue;
                // first tile of the next non-empty run: window j+1.. of this range, else window 0.. of the next
                int64_t t_after = -1;
#pragma unroll
                for (int jj = MAXW - 1; jj >= 0; --jj)
                    if (wj[jj] >= 0 && after[jj] > end[jj]) t_after = tbj[jj] + end[jj];
#pragma unroll
                for (int jj = MAXW - 1; jj > j; --jj)
                    if (wj[jj] >= 0 && end[jj] > done[jj]) t_after = tbj[jj] + done[jj];
                tw.walk(tbj[j] + done[j], tbj[j] + end[j], 1, acc[j], pad_tile, t_after);
                done[j] = end[j];
            }
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
                        if (row0 + ii < a.N) a.y[(row0 + ii) * a.ldy + colg] = TCGNN_KERNEL_STORE(a.relu, row0 + ii, colg, acc[j][s][ii] * inv1 * inv2);
                }
            }
        }
    }
}
