// tcgnn_small_fallback.inc - the CSR kernels of non-canonical plans, the range guard's fallbacks and wide_patch_kernel (the single-launch
// fp32-MFMA kernel of small graphs, which is also the binary SpMM's fallback: tcgnn_small_spmm.inc).  Included by tcgnn_device.hip.
static constexpr int64_t kSmallMaxTiles = 8192;   // wide blocks up to which the single-launch kernel is used (mode 0)

// ------------------------------------------------------------------------------------------
// fallbacks for non-canonical CSR rows (unsorted or duplicated column ids)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void spmm_val_csr_kernel(const int32_t* __restrict__ rowptr,
                                                           const int32_t* __restrict__ col,
                                                           const float* __restrict__ val,
                                                           const float* __restrict__ X, float* Y,
                                                           int32_t N, int32_t D) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const int lane = threadIdx.x & 63;
    const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
    for (int d = lane; d < D; d += 64) {
        float s = 0.f;
        for (int64_t e = e0; e < e1; ++e) s += round_rna10(val[e]) * round_rna10(X[(int64_t)col[e] * D + d]);
        Y[row * D + d] = s;
    }
}

__global__ __launch_bounds__(256) void sddmm_csr_kernel(const int32_t* __restrict__ rowptr,
                                                        const int32_t* __restrict__ col,
                                                        const float* __restrict__ X, float* ef,
                                                        int32_t N, int32_t D, int32_t row_off) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const int lane = threadIdx.x & 63;
    const float* xr = X + (row + row_off) * D;
    for (int64_t e = rowptr[row]; e < rowptr[row + 1]; ++e) {
        const float* xc = X + (int64_t)col[e] * D;
        float s = 0.f;
        for (int d = lane; d < D; d += 64) s += round_rna10(xr[d]) * round_rna10(xc[d]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        if (lane == 0) ef[e] = s;
    }
}

// ---- fallbacks behind the range guard (range_is_wide): launched behind every fp16-path kernel, they return at once unless the
//      staged matrix is "wide".  Plain fp32, CSR order, operands rounded to a 10-bit mantissa exactly like the reference's
//      (round_rna10) with fp32's full exponent: correct for any magnitudes, far from fast - a wide matrix is a rare input.
// Y[row] = [relu] sum_e v_e * rna(X'[col e]) with v_e = 1 (binary), rna(val[e]) or rna(fl32(w * val[e])) (the AGNN edge weights);
// X' = X where gate > 0 (the fused ReLU backward mask).  ldx / ldy: row strides (column blocks of wider matrices).
// (SC: tcgnn_spmm_scaled - X'[c] is multiplied by cs[c] before the rounding, the store applies the row scale / bias epilogue)
template <bool SC>
__device__ __forceinline__ void spmm_wide_fallback_body(const uint32_t* __restrict__ hdr, int use_val_word, const int32_t* __restrict__ rowptr,
                                                        const int32_t* __restrict__ col, const float* __restrict__ val, const float* __restrict__ wscale,
                                                        const float* __restrict__ X, const float* __restrict__ gate, float* __restrict__ Y, int32_t N, int32_t D,
                                                        int64_t ldx, int64_t ldy, int32_t relu, int32_t dedupe, const float* __restrict__ cs, const Epi& epi) {
    if (!(use_val_word ? range_is_wide_val(hdr) : range_is_wide(hdr, 0))) return;
    const int lane = threadIdx.x & 63;
    const float w = wscale ? wscale[0] : 1.0f;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < N; row += (int64_t)gridDim.x * 4) {   // (a small grid: the usual launch returns above)
    const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
    for (int d = lane; d < D; d += 64) {
        float s = 0.f;
        for (int64_t e = e0; e < e1; ++e) {
            if (dedupe) {   // binary A on a non-canonical row: an edge listed twice counts once (TCGNN_kernel.cu:405)
                bool dup = false;
                for (int64_t e2 = e0; e2 < e; ++e2) dup = dup || col[e2] == col[e];
                if (dup) continue;
            }
            const int64_t xi = (int64_t)col[e] * ldx + d;
            float x = X[xi];
            if (gate && !(gate[xi] > 0.0f)) x = 0.0f;
            if constexpr (SC) {
                if (cs) x = cs[col[e]] * x;
            }
            const float v = val ? round_rna10(wscale ? w * val[e] : val[e]) : 1.0f;
            s += v * round_rna10(x);
        }
        Y[row * ldy + d] = SC ? epi_apply(relu, epi, row, d, s) : relu_if(relu, s);
    }
    }
}
__global__ __launch_bounds__(256) void spmm_wide_fallback_kernel(const uint32_t* __restrict__ hdr, int use_val_word, const int32_t* __restrict__ rowptr,
                                                                 const int32_t* __restrict__ col, const float* __restrict__ val, const float* __restrict__ wscale,
                                                                 const float* __restrict__ X, const float* __restrict__ gate, float* __restrict__ Y, int32_t N, int32_t D,
                                                                 int64_t ldx, int64_t ldy, int32_t relu, int32_t dedupe) {
    spmm_wide_fallback_body<false>(hdr, use_val_word, rowptr, col, val, wscale, X, gate, Y, N, D, ldx, ldy, relu, dedupe, nullptr, Epi{nullptr, nullptr});
}
// binary A only (tcgnn_spmm_scaled)
__global__ __launch_bounds__(256) void spmm_wide_fallback_scaled_kernel(const uint32_t* __restrict__ hdr, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                        const float* __restrict__ X, const float* __restrict__ gate, const float* __restrict__ cs, const Epi epi,
                                                                        float* __restrict__ Y, int32_t N, int32_t D, int64_t ldx, int64_t ldy, int32_t relu, int32_t dedupe) {
    spmm_wide_fallback_body<true>(hdr, 0, rowptr, col, nullptr, nullptr, X, gate, Y, N, D, ldx, ldy, relu, dedupe, cs, epi);
}
// rows beyond the windows the caller described (zero in tcgnn_spmm): the epilogue of an empty sum
__global__ __launch_bounds__(256) void epi_fill_kernel(float* __restrict__ Y, int64_t row0, int32_t N, int32_t D, int32_t relu, const Epi epi) {
    const int64_t n = ((int64_t)N - row0) * D;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = row0 + k / D;
        const int d = (int)(k % D);
        Y[row * D + d] = epi_apply(relu, epi, row, d, 0.0f);
    }
}
// Y[row] = [relu] ((A X)[row]) W: the aggregated row goes through LDS, then every lane takes output columns (D_in, D_out <= 128)
__global__ __launch_bounds__(256) void spmm_gemm_wide_fallback_kernel(const uint32_t* __restrict__ hdr, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                      const float* __restrict__ X, const float* __restrict__ W, float* __restrict__ Y, int32_t N,
                                                                      int32_t Din, int32_t Dout, int32_t relu) {
    if (!range_is_wide(hdr, 0)) return;
    __shared__ float agg[4][128];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t row0 = (int64_t)blockIdx.x * 4; row0 < N; row0 += (int64_t)gridDim.x * 4) {
    const int64_t row = row0 + wv;
    __syncthreads();
    if (row < N) {
        const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
        for (int d = lane; d < Din; d += 64) {
            float s = 0.f;
            for (int64_t e = e0; e < e1; ++e) s += round_rna10(X[(int64_t)col[e] * Din + d]);
            agg[wv][d] = s;
        }
    }
    __syncthreads();
    if (row < N)
    for (int o = lane; o < Dout; o += 64) {
        float s = 0.f;
        for (int k = 0; k < Din; ++k) s = fmaf(agg[wv][k], W[(int64_t)k * Dout + o], s);
        Y[row * Dout + o] = relu_if(relu, s);
    }
    }
}
// ---- the way through a wide matrix at the default guard level (see wide2_dense in tcgnn_device.hip): every edge (r, c) whose row of
//      X or whose column's row of X is DIRTY (bitmap written by the conversion pass) is recomputed in fp32 with the reference's
//      operand rounding.
//   mode 0 (SDDMM):          ef[e] = <rna(x_r), rna(x_c)>
//   mode 1 (fused forward):  the same, max |ef| kept up to date, and Y[r] += rna(w ef_new) rna(x_c) - rna(w ef_old) img(x_c): the
//                            edge's contribution as the reference computes it minus what the MFMA kernel added (img = the fp16 image)
//   mode 2 (fused backward): X = dY, ef = the saved scores: G[r] += rna(w ef) (rna(x_c) - img(x_c)) and the edge's term of d_w,
//                            (<rna(x_r), rna(x_c)> - <img(x_r), img(x_c)>) col(e), into one extra double behind the partial sums
// r05: ONE scan over the edges (a lane tests an edge: its row's bit through edgeToRow, its column's bit), and every hit is recomputed
// by the whole wavefront (lane = feature column: coalesced rows, one reduction) - so the cost follows the dirty EDGES, however many
// rows they belong to and however long those rows are (a hub row's edges spread over all wavefronts).  Atomic adds: the order of
// the corrections of one row is not fixed.
struct PatchArgs {
    const uint32_t* hdr; const uint32_t* bitmap;
    const int32_t* rowptr; const int32_t* col; const int32_t* e2r;
    const float* X; const _Float16* x16; int32_t pitch;
    float* ef; const float* w; float* Y; uint32_t* efmax; double* dw_extra;
    int32_t N, Nc, D, row_off, mode; int64_t E;
    const int32_t* sym;   // device word: 1 = the plan's graph is structurally symmetric (symmetry_kernel, plan creation); nullptr: not known
    int32_t rows;         // min(N, nw_eff * 16): the rows of the windows the plan was given.  Behind them ef, Y / G and d_w keep the caller's zeros
};
// one thread per edge (r, c): is (c, r) an edge too?  (canonical CSR: column ids sorted inside a row - a binary search.)  sym[0] starts at 1.
// r06: only the edges ABOVE the diagonal search for their mirror; sym[1] collects (edges above) - (edges below).  Mirrors of distinct
// edges are distinct, so "every upper edge has a mirror" and "as many below as above" together say every lower edge is one: the same
// answer for half the searches (114.6 M edges: 13 -> 7 ms of plan creation).  symmetry_finish_kernel folds the balance into sym[0].
__global__ __launch_bounds__(256) void symmetry_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int32_t* __restrict__ e2r,
                                                       int64_t E, int32_t N, int32_t* __restrict__ sym) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int bal = 0;
    if (e < E) {
        const int32_t r = e2r[e], c = col[e];
        if (r < 0 || r >= N || c < 0 || c >= N) sym[0] = 0;
        else if (r < c) {
            bal = 1;
            int32_t lo = rowptr[c], hi = rowptr[c + 1];
            const int32_t end = hi;
            while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if (col[mid] < r) lo = mid + 1; else hi = mid; }
            if (!(lo < end && col[lo] == r)) sym[0] = 0;
        } else if (r > c) bal = -1;
    }
    const int up = __popcll(__ballot(bal > 0)), down = __popcll(__ballot(bal < 0));
    if ((threadIdx.x & 63) == 0 && up != down) atomicAdd(sym + 1, up - down);
}
__global__ void symmetry_finish_kernel(int32_t* sym) { if (sym[1] != 0) sym[0] = 0; }
// One dirty edge per GROUP OF EIGHT LANES (eight edges of a chunk at a time): the edges of a dirty row are consecutive in the CSR, so
// its hits come sixty-four to a chunk - one wavefront taking them one after the other was a chain of ~200 memory round trips per
// chunk (a 500-edge row: 0.2 ms on eight wavefronts while 8 000 others idled).  Lane `sub` of a group takes the feature columns
// sub, sub + 8, ...: the group reads 32 consecutive bytes of a row per step and adds its corrections to consecutive words.
__device__ __forceinline__ void patch_edge_group(const PatchArgs& a, bool on, int64_t e, int64_t r, int32_t c, bool c_dirty, int sub, float inv) {
    const float* xr = a.X + (on ? (r + a.row_off) * a.D : 0);
    const float* xc = a.X + (on ? (int64_t)c * a.D : 0);
    const _Float16* ir = a.x16 + (on ? (r + a.row_off) * a.pitch : 0);
    const _Float16* ic = a.x16 + (on ? (int64_t)c * a.pitch : 0);
    float exact = 0.f, dimg = 0.f;
    if (on) {
        int d = sub;
        for (; d + 24 < a.D; d += 32) {   // (four steps' loads in flight)
            const float x0 = xr[d], x1 = xr[d + 8], x2 = xr[d + 16], x3 = xr[d + 24], y0 = xc[d], y1 = xc[d + 8], y2 = xc[d + 16], y3 = xc[d + 24];
            const float i0 = (float)ir[d], i1 = (float)ir[d + 8], i2 = (float)ir[d + 16], i3 = (float)ir[d + 24], j0 = (float)ic[d], j1 = (float)ic[d + 8], j2 = (float)ic[d + 16], j3 = (float)ic[d + 24];
            exact += round_rna10(x0) * round_rna10(y0); exact += round_rna10(x1) * round_rna10(y1); exact += round_rna10(x2) * round_rna10(y2); exact += round_rna10(x3) * round_rna10(y3);
            dimg += (i0 * inv) * (j0 * inv); dimg += (i1 * inv) * (j1 * inv); dimg += (i2 * inv) * (j2 * inv); dimg += (i3 * inv) * (j3 * inv);
        }
        for (; d < a.D; d += 8) { exact += round_rna10(xr[d]) * round_rna10(xc[d]); dimg += ((float)ir[d] * inv) * ((float)ic[d] * inv); }
    }
#pragma unroll
    for (int off = 4; off > 0; off >>= 1) { exact += __shfl_xor(exact, off); dimg += __shfl_xor(dimg, off); }   // (inside the group of eight; every lane takes part)
    if (!on) return;
    if (a.mode == 0) { if (sub == 0) a.ef[e] = exact; return; }
    const float w = a.w[0];
    const float ef_old = a.ef[e];
    if (a.mode == 1) {
        const float a_old = round_rna10(w * ef_old), a_new = round_rna10(w * exact);
        for (int d = sub; d < a.D; d += 8) {
            const float v = a_new * round_rna10(xc[d]) - a_old * ((float)ic[d] * inv);
            if (v != 0.f) atomicAdd(&a.Y[r * a.D + d], v);
        }
        if (sub == 0) { a.ef[e] = exact; atomicMax(a.efmax, __float_as_uint(exact) & 0x7fffffffu); }
        return;
    }
    const float att = round_rna10(w * ef_old);
    if (c_dirty)
        for (int d = sub; d < a.D; d += 8) {   // (the image of an element that lost no bits IS its 10-bit rounding: the difference is exactly zero except at the
            const float v = att * (round_rna10(xc[d]) - (float)ic[d] * inv);   //  column's few lost elements - one or two atomics per edge instead of D; R-MAT backward calls: 1.4 M dirty edges)
            if (v != 0.f) atomicAdd(&a.Y[r * a.D + d], v);
        }
    if (sub == 0) atomicAdd(a.dw_extra, ((double)exact - (double)dimg) * (double)(float)c);
}
// the dense way through a wide matrix, inside the same launch (more than kSparseRows dirty rows: the MFMA kernel returned at once):
// plain fp32 in CSR order with the reference's operand rounding (as spmm_wide_fallback_kernel), a wavefront per row - every row's
// scores, then its aggregate from them, then (backward) its share of d_w into this workgroup's partial sum.
__device__ __forceinline__ void wide_dense_body(const PatchArgs& a, double* partial, int32_t npartial) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nb = a.mode == 2 ? (int)min((uint32_t)gridDim.x, (uint32_t)npartial) : (int)gridDim.x;
    __shared__ double wsum[4];
    double acc = 0.0;
    uint32_t m = 0u;
    const float w = a.w ? a.w[0] : 1.0f;
    if ((int)blockIdx.x < nb)
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < a.rows; row += (int64_t)nb * 4) {   // (rows behind the windows: the caller's zeros stay)
        const float* xr = a.X + (row + a.row_off) * a.D;
        const int64_t e0 = a.rowptr[row], e1 = a.rowptr[row + 1];
        if (a.mode != 2 || a.dw_extra)
            for (int64_t e = e0; e < e1; ++e) {
                const float* xc = a.X + (int64_t)a.col[e] * a.D;
                float s = 0.f;
                for (int d = lane; d < a.D; d += 64) s += round_rna10(xr[d]) * round_rna10(xc[d]);
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
                if (a.mode == 2) acc += (double)s * (double)(float)a.col[e];
                else if (lane == 0) { a.ef[e] = s; m = max(m, __float_as_uint(s) & 0x7fffffffu); }
            }
        if (a.mode == 0) continue;
        __threadfence_block();            // (mode 1: this wavefront reads back the scores its lane 0 has just written)
        for (int d = lane; d < a.D; d += 64) {
            float s = 0.f;
            for (int64_t e = e0; e < e1; ++e) s += round_rna10(w * a.ef[e]) * round_rna10(a.X[(int64_t)a.col[e] * a.D + d]);
            a.Y[row * a.D + d] = s;
        }
    }
    if (a.mode == 1 && a.efmax && lane == 0 && m) atomicMax(a.efmax, m);
    if (a.mode == 2) {
        if (lane == 0) wsum[wave] = acc;
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = (int)blockIdx.x; k < npartial; k += (int)gridDim.x) partial[k] = (k == (int)blockIdx.x && (int)blockIdx.x < nb) ? (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]) : 0.0;
    }
}
// (the bitmap is copied into LDS when it fits - 60 KB = 491 520 rows of X - so that the per-edge test is an LDS read; every wavefront
//  keeps four 64-edge chunks in flight and QUEUES its hits in LDS, recomputing them eight at a time, one per group of eight lanes:
//  on R-MAT a backward call has 16 000 dirty rows and 1.4 M dirty edges spread one or two to a chunk, and taking each chunk's
//  hits on their own was a chain of memory round trips per hit - 1.9 ms per call; sparse hits now fill whole batches)
// ROW-DRIVEN (r05, late): what training usually produces is ONE to a few dozen dirty rows (the calibrated SBM graph: one row of ~1 000
// edges in two of an epoch's four calls), and the scan reads all 458 MB of column ids to find their ~2 000 edges: 0.15 ms per wide
// call.  On a structurally symmetric graph (PatchArgs::sym) the edges that touch dirty row d are its own CSR row and, for every
// neighbour n of d, the mirror edge (n, d) - a binary search in row n: up to kPatchRowDriven dirty rows are patched that way, every
// wavefront of the grid taking eight edges of a row at a time (both sides), in ~10 us.  More rows, an asymmetric or rectangular
// plan, a bitmap beyond LDS: the scan.
// r15: which wavefront takes which eight edges of a dirty row is a function of the ROW ID.  It was a function of the row's position in
// dlist, and dlist is filled in the order this workgroup's wavefronts won an LDS atomic: two workgroups that numbered the rows
// differently left a chunk to no wavefront or to several (modes 1 and 2 then add the correction twice).  dlist's order now decides
// nothing but the order of the loop.  Rows behind the windows the plan was given (PatchArgs::rows) keep their zeros on every way:
// a dirty row there is patched on the mirror side only - the edges (n, d) of covered rows n.
static constexpr int kPatchBitmapWords = 15360, kPatchUnroll = 4, kPatchQueue = 128, kPatchRowDriven = 256;
__global__ __launch_bounds__(256) void wide_patch_kernel(const PatchArgs a, double* partial, int32_t npartial) {
    if (!range_is_wide(a.hdr, 0)) return;
    if (a.hdr[kHdrStrict]) { wide_dense_body(a, partial, npartial); return; }   // (the strict level: the MFMA kernel returned at once, everything in plain fp32)
    if (!a.hdr[kHdrDirtyRows]) return;                                             // (lost elements in no row that was marked: nothing to patch)
    __shared__ uint32_t sbm[kPatchBitmapWords];
    __shared__ int32_t q_elo[4][kPatchQueue], q_ehi[4][kPatchQueue], q_r[4][kPatchQueue], q_c[4][kPatchQueue];   // per wavefront: edge, row (-2: read it), column | dirty-column flag << 31
    const int nwords = (a.Nc + 1 + 31) >> 5;
    const bool in_lds = nwords <= kPatchBitmapWords;
    if (in_lds) {
        for (int k = threadIdx.x; k < nwords; k += blockDim.x) sbm[k] = a.bitmap[k];
        __syncthreads();
    }
    const uint32_t* const bm = in_lds ? sbm : a.bitmap;   // (generic pointer: the branch is kernel-uniform)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t gw = (int64_t)blockIdx.x * 4 + wv, nwaves = (int64_t)gridDim.x * 4;
    const float inv = pow2f(-scale_exp_from_bits(a.hdr[kHdrMaxX]));
    auto dirty = [&](int64_t x) -> bool { return x >= 0 && x <= a.Nc && ((bm[x >> 5] >> (x & 31)) & 1u); };
    if (in_lds && a.sym && a.row_off == 0 && a.N == a.Nc && a.hdr[kHdrDirtyRows] <= (uint32_t)kPatchRowDriven && a.sym[0] == 1) {   // (kernel-uniform)
        __shared__ int32_t dlist[kPatchRowDriven];
        __shared__ int32_t dcount;
        if (threadIdx.x == 0) dcount = 0;
        __syncthreads();
        for (int k = threadIdx.x; k < nwords; k += blockDim.x) {
            uint32_t wbits = sbm[k];
            while (wbits) {
                const int b = __builtin_ctz(wbits); wbits &= wbits - 1u;
                const int32_t row = k * 32 + b;
                if (row < a.N) { const int pos = atomicAdd(&dcount, 1); if (pos < kPatchRowDriven) dlist[pos] = row; }
            }
        }
        __syncthreads();
        const int nd = dcount < kPatchRowDriven ? dcount : kPatchRowDriven;   // (hdr[kHdrDirtyRows] counted every marked row once: dcount <= hdr[kHdrDirtyRows])
        const int g8 = lane >> 3;
        for (int i = 0; i < nd; ++i) {
            const int32_t d = dlist[i];
            const int64_t e0 = a.rowptr[d], deg = (int64_t)a.rowptr[d + 1] - e0;
            const int64_t first = (gw + (int64_t)d * 257) % nwaves;          // (by the row id, the same in every workgroup; neighbouring dirty rows start at different wavefronts)
            for (int64_t j0 = first * 8; j0 < 2 * deg; j0 += nwaves * 8) {   // (wave-uniform trip count: patch_edge_group shuffles inside its groups of eight)
                const int64_t j = j0 + g8;
                const bool valid = j < 2 * deg, mirror = j >= deg;
                const int64_t erow = e0 + (valid ? (mirror ? j - deg : j) : 0);
                const int32_t n = valid ? a.col[erow] : 0;
                const bool ndirty = dirty(n);
                int64_t e = erow; int64_t r = d; int32_t c = n; bool cd = ndirty, on = valid && d < a.rows;
                if (mirror) {   // the edge (n, d): where d sits in row n.  Row n dirty as well: its own row side takes that edge
                    int32_t lo = valid ? a.rowptr[n] : 0, hi = valid ? a.rowptr[n + 1] : 0;
                    const int32_t end = hi;
                    while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if (a.col[mid] < d) lo = mid + 1; else hi = mid; }
                    on = valid && !ndirty && n < a.rows && lo < end && a.col[lo] == d;
                    e = lo; r = n; c = d; cd = true;
                }
                patch_edge_group(a, on, e, r, c, cd, lane & 7, inv);
            }
        }
        return;
    }
    int cnt = 0;                                          // entries in this wavefront's queue (wave-uniform)
    auto process8 = [&](int first, int n) {               // queue entries first .. first + n - 1 (n <= 8), one per group of eight lanes
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();
        const int g8 = lane >> 3;
        const bool mine = g8 < n;
        const int k = first + (mine ? g8 : 0);
        const int64_t e = ((int64_t)q_ehi[wv][k] << 32) | (uint32_t)q_elo[wv][k];
        int32_t r = q_r[wv][k];
        const uint32_t cw = (uint32_t)q_c[wv][k];
        if (mine && r == -2) r = a.e2r[e];                // (a hit by its column alone: its row is read now)
        const bool on = mine && r >= 0 && r < a.rows;
        patch_edge_group(a, on, e, (int64_t)r, (int32_t)(cw & 0x7fffffffu), (cw >> 31) != 0u, lane & 7, inv);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();
    };
    // (the edges of a 64-edge chunk are consecutive in the CSR: their rows are the interval [edgeToRow[first], edgeToRow[last]] - two
    //  words per chunk tell whether any of them can be dirty at all; only then is edgeToRow read per edge)
    constexpr int U = kPatchUnroll;
    for (int64_t base = gw * (64 * U); base < a.E; base += nwaves * (64 * U)) {
        int32_t c[U], ra[U], rb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t e0 = base + 64 * u, e = e0 + lane;
            c[u] = e < a.E ? a.col[e] : -1;
            ra[u] = e0 < a.E ? a.e2r[e0] : 0;
            rb[u] = e0 < a.E ? a.e2r[e0 + 63 < a.E ? e0 + 63 : a.E - 1] : -1;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t e0 = base + 64 * u, e = e0 + lane;
            if (e0 >= a.E) break;
            bool rows_dirty = rb[u] - ra[u] > 64 || ra[u] < 0 || rb[u] >= a.N;    // (a chunk that spans many rows - or inconsistent metadata: the per-edge test decides)
            for (int32_t q = ra[u]; q <= rb[u] && !rows_dirty; ++q) rows_dirty = dirty((int64_t)q + a.row_off);
            int32_t r = -2;
            const bool cd = dirty(c[u]);
            bool hit = e < a.E && cd;
            if (rows_dirty && e < a.E) { r = a.e2r[e]; hit = r >= 0 && r < a.rows && (cd || dirty((int64_t)r + a.row_off)); }
            const uint64_t m = __ballot(hit);
            if (!m) continue;
            if (hit) {
                const int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
                q_elo[wv][pos] = (int32_t)(uint32_t)e; q_ehi[wv][pos] = (int32_t)(e >> 32); q_r[wv][pos] = r; q_c[wv][pos] = (int32_t)((uint32_t)c[u] | (cd ? 0x80000000u : 0u));
            }
            cnt += __popcll(m);
            while (cnt >= 8 && (cnt > kPatchQueue - 64 || cnt >= 64)) { cnt -= 8; process8(cnt, 8); }   // (whole batches; room for the next chunk's sixty-four)
        }
        while (cnt >= 8) { cnt -= 8; process8(cnt, 8); }
    }
    if (cnt > 0) process8(0, cnt);
}
static hipError_t launch_wide_patch(const PatchArgs& a, hipStream_t stream, double* partial = nullptr, int32_t npartial = 0) {
    hipLaunchKernelGGL(wide_patch_kernel, dim3(2048), dim3(256), 0, stream, a, partial, npartial);
    return hipGetLastError();
}
