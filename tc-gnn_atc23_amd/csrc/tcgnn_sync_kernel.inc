// tcgnn_sync_kernel.inc - the body of spmm_sync_kernel (tcgnn_sync_walk.inc), included twice: as the plain kernel and as
// spmm_sync_epi_kernel, the same walk with tcgnn_spmm_scaled's row scale / bias in the final store.  The macros expand, for the
// plain kernel, to exactly the tokens it was written with, so its code does not change.
template <int NT, int MAXW, bool VAL, int NBUF>
__global__ __launch_bounds__(sync_geom(NT, VAL).threads, sync_geom(NT, VAL).waves_per_simd) void TCGNN_KERNEL_NAME(TCGNN_KERNEL_PARAM) {
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
    using TW = TileWalker<NT, VAL, NBUF>;
    char* atab = smem + 4 * TW::WAVE_LDS;
    fill_afrag_table(atab);
    __syncthreads();
    const TW tw(a, smem + wave * TW::WAVE_LDS, atab, coloff, pow2f(ka));

    int x, w_lo, w_hi, nph;
    sync_slice_of(b.s, x, w_lo, w_hi, nph);
    const int nwv = (int)(gridDim.x / (unsigned)kXcds) * 4, wid = (int)(blockIdx.x / (unsigned)kXcds) * 4 + wave;
    const int tstride = b.s.kmax + 1;
    for (int base = w_lo + wid; base < w_hi; base += nwv * MAXW) {   // (one trip when the grid holds the slice)
        int wj[MAXW];
        int64_t tbj[MAXW];
        uint32_t done[MAXW], nend[MAXW];
        floatx4 acc[MAXW][NT];
#pragma unroll
        for (int j = 0; j < MAXW; ++j) {
            const int w = base + j * nwv;           // co-resident wavefronts hold neighbouring windows
            wj[j] = w < w_hi ? w : -1;
            tbj[j] = wj[j] >= 0 ? a.wb_ptr[wj[j]] : 0;
            done[j] = 0;
            nend[j] = wj[j] >= 0 ? b.s.T[(int64_t)wj[j] * tstride + (b.s.m < b.s.kmax ? b.s.m : b.s.kmax)] : 0u;
#pragma unroll
            for (int s = 0; s < NT; ++s) acc[j][s] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
        if constexpr (NBUF == 1) {
            // one pipeline over the wavefront's runs, phase-major (TileWalker::walk_list): the (window, phase) runs are ~5 tiles here, and
            // walk() starts each behind two exposed round trips.  The list goes to the wavefront's own LDS first - nothing is in flight
            // then; a list that would not fit (tiny phases: tests) is walked in pieces of kMaxRuns / MAXW phases.
            for (int r0 = 0; r0 < nph; r0 += TW::kMaxRuns / MAXW) {
                const int r1 = r0 + TW::kMaxRuns / MAXW < nph ? r0 + TW::kMaxRuns / MAXW : nph;
                int nruns = 0;
                for (int r = r0; r < r1; ++r) {
                    const int k1 = (r + 1) * b.s.m < b.s.kmax ? (r + 1) * b.s.m : b.s.kmax;
#pragma unroll
                    for (int j = 0; j < MAXW; ++j) {
                        if (wj[j] < 0) continue;
                        const uint32_t e = b.s.T[(int64_t)wj[j] * tstride + k1];
                        if (e > done[j]) { tw.run_put(nruns++, tbj[j] + done[j], e - done[j], j); done[j] = e; }
                    }
                }
                tw.template walk_list<MAXW>(nruns, acc);
            }
        } else {
        int64_t pad_tile = -1;
        for (int r = 0; r < nph; ++r) {
            uint32_t end[MAXW], after[MAXW];
            const int kn = (r + 2) * b.s.m < b.s.kmax ? (r + 2) * b.s.m : b.s.kmax;
#pragma unroll
            for (int j = 0; j < MAXW; ++j) {
                end[j] = nend[j];
                after[j] = (wj[j] >= 0 && r + 1 < nph) ? b.s.T[(int64_t)wj[j] * tstride + kn] : end[j];
                nend[j] = after[j];
            }
#pragma unroll
            for (int j = 0; j < MAXW; ++j) {
                if (wj[j] < 0) continue;
                // first tile of the next non-empty run (window j+1.. of this phase, else window 0.. of the next): its ids are prefetched
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
