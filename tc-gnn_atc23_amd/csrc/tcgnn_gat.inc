// tcgnn_gat.inc - multi-head GAT attention: the additive scores, their softmax over a node's incoming edges and its backward in ONE
// kernel each, the per-source-node sum of per-edge values, and their C ABI.  Included by tcgnn_device.hip behind
// tcgnn_edge_softmax.inc, whose building blocks (es_*: length binning, fixed-order reductions) it uses as they are.
//
//   forward   s[h,e] = lrelu(fl32(el[col e, h] + er[row e, h])),  lrelu(x) = x > 0 ? x : fl32(x slope);   p[h,.] = softmax of s[h,.] over each row
//   backward  g = p (dp - sum_row p dp);  ds[h,e] = g (raw > 0 ? 1 : slope);  d_er[r,h] = sum_{e in row r} ds[h,e]
//   colsum    out[c,h] = sum_{eT in row c of A^T} val[h, perm[eT]]                                  (val = ds: d_el)
//
// Per-node terms are [N, H] row-major, per-edge arrays head-major [H, E] (a head's row is what tcgnn_spmm_val takes).  The scores never
// reach memory: they are formed from the two gathers where they are used, in backward again.
// Scheduling is tcgnn_edge_softmax.inc's: a workgroup of four wavefronts owns 32 consecutive rows and bins them by length; ALL heads
// of a row stay in that workgroup.  Rows of up to 1024 edges read their column ids once and keep them in registers while the heads
// are taken one after the other (a node's H values of el share a 4H-byte line); longer rows take kGatHc heads per strided pass, so
// that one read of a column id and one line of el feed kGatHc scores.
// The score is rounded to fp32 BEFORE the maximum is taken and subtracted (gat_mul_rn: the product x slope must not be contracted
// with the subtraction into one fma) - p is the softmax of the score a composition of separate operators would form; at |s| ~ 1e4 a
// contracted product moves p by ~6e-4 relative.  Row sums and quotients are fp64 as in tcgnn_edge_softmax.inc, d_er and the column
// sums as well (fp32 terms, fp64 fixed-order sums, one rounding).  No atomics: every result is bit-identical on repetition.
// Row pointers are clamped to [0, E] (es_load_rows), column ids to [0, N), perm entries to [0, E): nothing outside [0, E) of a head's
// row of p / ds and nothing outside [0, N H) of d_er / out is written, whatever the arrays hold.  ds may alias dp (a thread reads
// position e of dp before it writes position e of ds; the workgroup passes are separated by barriers).

namespace {

constexpr int kGatHc = 4;   // heads carried through one strided pass over a long row

__device__ __forceinline__ float gat_mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float gat_score(float l, float r, float slope) {
    const float x = l + r;
    return x > 0.f ? x : gat_mul_rn(x, slope);
}
__device__ __forceinline__ int32_t gat_node(int32_t c, int32_t N) { return c < 0 ? 0 : (c >= N ? N - 1 : c); }
__device__ __forceinline__ int64_t gat_edge(int32_t q, int64_t E) { return (uint64_t)(uint32_t)q >= (uint64_t)E ? 0 : (int64_t)(uint32_t)q; }

// ---- forward ------------------------------------------------------------------------------------------------------------------
// W lanes per row, NK edges per lane (W * NK >= the row's length); err = er + row * H.  FULL: the row is longer than W * NK / 2, so the
// lower half of a lane's edges needs no bounds test (half as many lane masks stay live across the loop over the heads)
template <int W, int NK, bool FULL>
__device__ __forceinline__ void gat_fwd_row(const int32_t* __restrict__ col, const float* __restrict__ el, const float* __restrict__ err, int32_t N,
                                            int32_t H, int64_t E, float slope, float* __restrict__ p, int64_t lo, int64_t hi, int sub) {
    const float* lp[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int64_t e = lo + k * W + sub;
        const bool in = (FULL && k < NK / 2) || e < hi;
        lp[k] = el + (int64_t)gat_node(in ? col[e] : 0, N) * H;
    }
    for (int32_t h = 0; h < H; ++h) {
        const float r = err[h];
        float v[NK], ex[NK];
        double t[NK];
        float m = -INFINITY;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int64_t e = lo + k * W + sub;
            const bool in = (FULL && k < NK / 2) || e < hi;
            v[k] = in ? gat_score(lp[k][h], r, slope) : 0.f;
            if (in) m = fmaxf(m, v[k]);
        }
        m = es_max<W>(m);
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int64_t e = lo + k * W + sub;
            const bool in = (FULL && k < NK / 2) || e < hi;
            ex[k] = in ? es_exp(v[k] - m) : 0.f;
            t[k] = ex[k];
        }
        const double inv = 1.0 / es_sum<W>(es_pairwise<NK>(t));
        float* ph = p + (int64_t)h * E;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int64_t e = lo + k * W + sub;
            const bool in = (FULL && k < NK / 2) || e < hi;
            if (in) ph[e] = (float)((double)ex[k] * inv);
        }
    }
}

__global__ __launch_bounds__(256) void gat_softmax_fwd_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int32_t N, int64_t E,
                                                              int32_t H, const float* __restrict__ el, const float* __restrict__ er, float slope,
                                                              float* __restrict__ p) {
    __shared__ int64_t sp[kEsRowsPerWg + 1];
    __shared__ float redf[4];
    __shared__ double redd[4];
    es_load_rows(rowptr, N, E, sp);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t row0 = (int64_t)blockIdx.x * kEsRowsPerWg;
    const auto er_of = [&](int r) { const int64_t g = row0 + r; return er + (g < N ? g : (int64_t)N - 1) * H; };   // (rows behind N are empty)
    {   // rows of 1 .. 16 edges: eight lanes each
        const int r = wave * kEsRowsPerWave + (lane >> 3);
        const int64_t lo = sp[r], len = sp[r + 1] - lo;
        const bool mine = len >= 1 && len <= kEsShort;
        gat_fwd_row<8, 2, false>(col, el, er_of(r), N, H, E, slope, p, lo, mine ? lo + len : lo, lane & 7);
    }
    for (int q = 0; q < kEsRowsPerWave; ++q) {   // rows of 17 .. 1024 edges: this wavefront's, one after the other
        const int r = wave * kEsRowsPerWave + q;
        const int64_t lo = sp[r], hi = sp[r + 1];
        const int len = __builtin_amdgcn_readfirstlane((int)(hi - lo));
        if (len <= kEsShort || len > kEsMedium) continue;
        const float* err = er_of(r);
        if (len <= 64) gat_fwd_row<64, 1, false>(col, el, err, N, H, E, slope, p, lo, hi, lane);
        else if (len <= 128) gat_fwd_row<64, 2, true>(col, el, err, N, H, E, slope, p, lo, hi, lane);
        else if (len <= 256) gat_fwd_row<64, 4, true>(col, el, err, N, H, E, slope, p, lo, hi, lane);
        else if (len <= 512) gat_fwd_row<64, 8, true>(col, el, err, N, H, E, slope, p, lo, hi, lane);
        else gat_fwd_row<64, 16, true>(col, el, err, N, H, E, slope, p, lo, hi, lane);
    }
    for (int r = 0; r < kEsRowsPerWg; ++r) {     // longer rows: the whole workgroup, kGatHc heads per pass (the trip tests are workgroup-uniform)
        const int64_t lo = sp[r], hi = sp[r + 1];
        if (hi - lo <= kEsMedium) continue;
        const float* err = er_of(r);
        for (int32_t h0 = 0; h0 < H; h0 += kGatHc) {
            const int nh = H - h0 < kGatHc ? H - h0 : kGatHc;
            float rr[kGatHc], m[kGatHc];
            double inv[kGatHc];
#pragma unroll
            for (int j = 0; j < kGatHc; ++j) {
                rr[j] = j < nh ? err[h0 + j] : 0.f;
                m[j] = -INFINITY;
            }
#pragma unroll 2
            for (int64_t e = lo + threadIdx.x; e < hi; e += 256) {
                const float* l = el + (int64_t)gat_node(col[e], N) * H + h0;
#pragma unroll
                for (int j = 0; j < kGatHc; ++j)
                    if (j < nh) m[j] = fmaxf(m[j], gat_score(l[j], rr[j], slope));
            }
#pragma unroll
            for (int j = 0; j < kGatHc; ++j) m[j] = es_block_max(m[j], redf);
            double acc[kGatHc] = {};
#pragma unroll 2
            for (int64_t e = lo + threadIdx.x; e < hi; e += 256) {
                const float* l = el + (int64_t)gat_node(col[e], N) * H + h0;
#pragma unroll
                for (int j = 0; j < kGatHc; ++j)
                    if (j < nh) acc[j] += (double)es_exp(gat_score(l[j], rr[j], slope) - m[j]);
            }
#pragma unroll
            for (int j = 0; j < kGatHc; ++j) inv[j] = 1.0 / es_block_sum(acc[j], redd);
#pragma unroll 2
            for (int64_t e = lo + threadIdx.x; e < hi; e += 256) {
                const float* l = el + (int64_t)gat_node(col[e], N) * H + h0;
#pragma unroll
                for (int j = 0; j < kGatHc; ++j)
                    if (j < nh) p[(int64_t)(h0 + j) * E + e] = (float)((double)es_exp(gat_score(l[j], rr[j], slope) - m[j]) * inv[j]);
            }
        }
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
// dst = d_er + row * H, or null where the lane group's row lies behind N
template <int W, int NK, bool FULL>
__device__ __forceinline__ void gat_bwd_row(const int32_t* __restrict__ col, const float* __restrict__ el, const float* __restrict__ err, int32_t N,
                                            int32_t H, int64_t E, float slope, const float* __restrict__ p, const float* dp, float* ds, float* dst,
                                            int64_t lo, int64_t hi, int sub) {
    const float* lp[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int64_t e = lo + k * W + sub;
        const bool in = (FULL && k < NK / 2) || e < hi;
        lp[k] = el + (int64_t)gat_node(in ? col[e] : 0, N) * H;
    }
    for (int32_t h = 0; h < H; ++h) {
        const float r = err[h];
        const float* ph = p + (int64_t)h * E;
        const float* dph = dp + (int64_t)h * E;
        float* dsh = ds + (int64_t)h * E;
        float pv[NK], dv[NK], raw[NK];
        double t[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int64_t e = lo + k * W + sub;
            const bool in = (FULL && k < NK / 2) || e < hi;
            pv[k] = in ? ph[e] : 0.f;
            dv[k] = in ? dph[e] : 0.f;
            raw[k] = in ? lp[k][h] + r : 0.f;
            t[k] = (double)pv[k] * (double)dv[k];
        }
        const double dot = es_sum<W>(es_pairwise<NK>(t));   // (fp64, and the difference below: tcgnn_edge_softmax.inc says why)
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int64_t e = lo + k * W + sub;
            const bool in = (FULL && k < NK / 2) || e < hi;
            const float g = pv[k] * (float)((double)dv[k] - dot);
            const float d = raw[k] > 0.f ? g : g * slope;
            if (in) dsh[e] = d;
            t[k] = in ? (double)d : 0.0;
        }
        const double total = es_sum<W>(es_pairwise<NK>(t));
        if (sub == 0 && dst) dst[h] = (float)total;
    }
}

__global__ __launch_bounds__(256) void gat_softmax_bwd_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int32_t N, int64_t E,
                                                              int32_t H, const float* __restrict__ el, const float* __restrict__ er, float slope,
                                                              const float* __restrict__ p, const float* dp, float* ds, float* __restrict__ d_er) {
    __shared__ int64_t sp[kEsRowsPerWg + 1];
    __shared__ double redd[4];
    es_load_rows(rowptr, N, E, sp);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t row0 = (int64_t)blockIdx.x * kEsRowsPerWg;
    const auto er_of = [&](int r) { const int64_t g = row0 + r; return er + (g < N ? g : (int64_t)N - 1) * H; };
    {   // rows of 0 .. 16 edges (an empty row's d_er is written here: 0)
        const int r = wave * kEsRowsPerWave + (lane >> 3);
        const int64_t lo = sp[r], len = sp[r + 1] - lo;
        const bool mine = len <= kEsShort;
        gat_bwd_row<8, 2, false>(col, el, er_of(r), N, H, E, slope, p, dp, ds, mine && row0 + r < N ? d_er + (row0 + r) * H : nullptr, lo,
                          mine ? lo + len : lo, lane & 7);
    }
    for (int q = 0; q < kEsRowsPerWave; ++q) {
        const int r = wave * kEsRowsPerWave + q;
        const int64_t lo = sp[r], hi = sp[r + 1];
        const int len = __builtin_amdgcn_readfirstlane((int)(hi - lo));
        if (len <= kEsShort || len > kEsMedium) continue;
        const float* err = er_of(r);
        float* dst = d_er + (row0 + r) * H;   // (a row with edges lies in front of N)
        if (len <= 64) gat_bwd_row<64, 1, false>(col, el, err, N, H, E, slope, p, dp, ds, dst, lo, hi, lane);
        else if (len <= 128) gat_bwd_row<64, 2, true>(col, el, err, N, H, E, slope, p, dp, ds, dst, lo, hi, lane);
        else if (len <= 256) gat_bwd_row<64, 4, true>(col, el, err, N, H, E, slope, p, dp, ds, dst, lo, hi, lane);
        else if (len <= 512) gat_bwd_row<64, 8, true>(col, el, err, N, H, E, slope, p, dp, ds, dst, lo, hi, lane);
        else gat_bwd_row<64, 16, true>(col, el, err, N, H, E, slope, p, dp, ds, dst, lo, hi, lane);
    }
    for (int r = 0; r < kEsRowsPerWg; ++r) {
        const int64_t lo = sp[r], hi = sp[r + 1];
        if (hi - lo <= kEsMedium) continue;
        const float* err = er_of(r);
        for (int32_t h0 = 0; h0 < H; h0 += kGatHc) {
            const int nh = H - h0 < kGatHc ? H - h0 : kGatHc;
            float rr[kGatHc];
            double dot[kGatHc], acc[kGatHc] = {};
#pragma unroll
            for (int j = 0; j < kGatHc; ++j) rr[j] = j < nh ? err[h0 + j] : 0.f;
#pragma unroll 2
            for (int64_t e = lo + threadIdx.x; e < hi; e += 256) {
#pragma unroll
                for (int j = 0; j < kGatHc; ++j)
                    if (j < nh) acc[j] += (double)p[(int64_t)(h0 + j) * E + e] * (double)dp[(int64_t)(h0 + j) * E + e];
            }
#pragma unroll
            for (int j = 0; j < kGatHc; ++j) {
                dot[j] = es_block_sum(acc[j], redd);
                acc[j] = 0.0;
            }
#pragma unroll 2
            for (int64_t e = lo + threadIdx.x; e < hi; e += 256) {
                const float* l = el + (int64_t)gat_node(col[e], N) * H + h0;
#pragma unroll
                for (int j = 0; j < kGatHc; ++j)
                    if (j < nh) {
                        const int64_t at = (int64_t)(h0 + j) * E + e;
                        const float g = p[at] * (float)((double)dp[at] - dot[j]);
                        const float d = l[j] + rr[j] > 0.f ? g : g * slope;
                        ds[at] = d;
                        acc[j] += (double)d;
                    }
            }
#pragma unroll
            for (int j = 0; j < kGatHc; ++j) {
                const double total = es_block_sum(acc[j], redd);
                if (threadIdx.x == 0 && j < nh) d_er[(row0 + r) * H + h0 + j] = (float)total;
            }
        }
    }
}

// ---- per-source-node sums of per-edge values (rows of A^T; the values in A's order, found through perm) ---------------------------
// kGatHc heads of one row of A^T, a strided walk of W lanes: fp64 partial sums in the walk's order, then the fixed tree
template <int W>
__device__ __forceinline__ void colsum_strided(const int32_t* __restrict__ perm, const float* __restrict__ val, int64_t E, int32_t h0, int nh,
                                               int64_t lo, int64_t hi, int sub, double (&acc)[kGatHc]) {
#pragma unroll
    for (int j = 0; j < kGatHc; ++j) acc[j] = 0.0;
#pragma unroll 2
    for (int64_t e = lo + sub; e < hi; e += W) {
        const float* v = val + (int64_t)h0 * E + gat_edge(perm[e], E);
#pragma unroll
        for (int j = 0; j < kGatHc; ++j)
            if (j < nh) acc[j] += (double)v[(int64_t)j * E];
    }
}

__global__ __launch_bounds__(256) void edge_colsum_kernel(const int32_t* __restrict__ rowptr_t, const int32_t* __restrict__ perm, int32_t N, int64_t E,
                                                          int32_t H, const float* __restrict__ val, float* __restrict__ out) {
    __shared__ int64_t sp[kEsRowsPerWg + 1];
    __shared__ double redd[4];
    es_load_rows(rowptr_t, N, E, sp);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t row0 = (int64_t)blockIdx.x * kEsRowsPerWg;
    {   // rows of 0 .. 16 entries: eight lanes each, two entries per lane
        const int r = wave * kEsRowsPerWave + (lane >> 3);
        const int64_t lo = sp[r], len = sp[r + 1] - lo;
        const bool mine = len <= kEsShort && row0 + r < N;
        const int64_t hi = mine ? lo + len : lo, e0 = lo + (lane & 7), e1 = e0 + 8;
        const int64_t q0 = e0 < hi ? gat_edge(perm[e0], E) : 0, q1 = e1 < hi ? gat_edge(perm[e1], E) : 0;
        for (int32_t h = 0; h < H; ++h) {
            const float* v = val + (int64_t)h * E;
            const double t = (e0 < hi ? (double)v[q0] : 0.0) + (e1 < hi ? (double)v[q1] : 0.0);
            const double total = es_sum<8>(t);
            if (mine && (lane & 7) == 0) out[(row0 + r) * H + h] = (float)total;
        }
    }
    for (int q = 0; q < kEsRowsPerWave; ++q) {   // rows of 17 .. 1024 entries: a wavefront each
        const int r = wave * kEsRowsPerWave + q;
        const int64_t lo = sp[r], hi = sp[r + 1];
        const int len = __builtin_amdgcn_readfirstlane((int)(hi - lo));
        if (len <= kEsShort || len > kEsMedium) continue;
        for (int32_t h0 = 0; h0 < H; h0 += kGatHc) {
            const int nh = H - h0 < kGatHc ? H - h0 : kGatHc;
            double acc[kGatHc];
            colsum_strided<64>(perm, val, E, h0, nh, lo, hi, lane, acc);
#pragma unroll
            for (int j = 0; j < kGatHc; ++j) {
                const double total = es_sum<64>(acc[j]);
                if (lane == 0 && j < nh) out[(row0 + r) * H + h0 + j] = (float)total;
            }
        }
    }
    for (int r = 0; r < kEsRowsPerWg; ++r) {     // longer rows: the whole workgroup
        const int64_t lo = sp[r], hi = sp[r + 1];
        if (hi - lo <= kEsMedium) continue;
        for (int32_t h0 = 0; h0 < H; h0 += kGatHc) {
            const int nh = H - h0 < kGatHc ? H - h0 : kGatHc;
            double acc[kGatHc];
            colsum_strided<256>(perm, val, E, h0, nh, lo, hi, threadIdx.x, acc);
#pragma unroll
            for (int j = 0; j < kGatHc; ++j) {
                const double total = es_block_sum(acc[j], redd);
                if (threadIdx.x == 0 && j < nh) out[(row0 + r) * H + h0 + j] = (float)total;
            }
        }
    }
}

inline int gat_sizes_ok(int32_t N, int64_t E, int32_t H) { return N >= 0 && E >= 0 && E <= 0x7fffffffLL && H >= 1; }

} // namespace

extern "C" int tcgnn_gat_softmax(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges, int32_t num_heads,
                                 const float* d_el, const float* d_er, float negative_slope, float* d_p, void* stream) {
    if (!gat_sizes_ok(num_nodes, num_edges, num_heads)) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_gat_softmax: bad size (num_heads >= 1, int32 CSR positions only)");
    if (num_nodes == 0 || num_edges == 0) return TCGNN_OK;
    if (!d_nodePointer || !d_edgeList || !d_el || !d_er || !d_p) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_gat_softmax: null array");
    hipLaunchKernelGGL(gat_softmax_fwd_kernel, dim3(es_grid(num_nodes)), dim3(256), 0, static_cast<hipStream_t>(stream), d_nodePointer, d_edgeList,
                       num_nodes, num_edges, num_heads, d_el, d_er, negative_slope, d_p);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}

extern "C" int tcgnn_gat_softmax_backward(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges,
                                          int32_t num_heads, const float* d_el, const float* d_er, float negative_slope, const float* d_p,
                                          const float* d_dp, float* d_ds, float* d_der, void* stream_v) {
    if (!gat_sizes_ok(num_nodes, num_edges, num_heads)) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_gat_softmax_backward: bad size (num_heads >= 1, int32 CSR positions only)");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_nodes == 0 || num_edges == 0) {
        if (num_nodes > 0 && d_der) HIP_TRY(hipMemsetAsync(d_der, 0, sizeof(float) * (size_t)num_nodes * (size_t)num_heads, stream));
        return TCGNN_OK;
    }
    if (!d_nodePointer || !d_edgeList || !d_el || !d_er || !d_p || !d_dp || !d_ds || !d_der) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_gat_softmax_backward: null array");
    hipLaunchKernelGGL(gat_softmax_bwd_kernel, dim3(es_grid(num_nodes)), dim3(256), 0, stream, d_nodePointer, d_edgeList, num_nodes, num_edges, num_heads,
                       d_el, d_er, negative_slope, d_p, d_dp, d_ds, d_der);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}

extern "C" int tcgnn_edge_colsum(const int32_t* d_nodePointer_t, const int32_t* d_perm, int32_t num_nodes, int64_t num_edges, int32_t num_heads,
                                 const float* d_val, float* d_out, void* stream_v) {
    if (!gat_sizes_ok(num_nodes, num_edges, num_heads)) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_edge_colsum: bad size (num_heads >= 1, int32 CSR positions only)");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_nodes == 0 || num_edges == 0) {
        if (num_nodes > 0 && d_out) HIP_TRY(hipMemsetAsync(d_out, 0, sizeof(float) * (size_t)num_nodes * (size_t)num_heads, stream));
        return TCGNN_OK;
    }
    if (!d_nodePointer_t || !d_perm || !d_val || !d_out) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_edge_colsum: null array");
    hipLaunchKernelGGL(edge_colsum_kernel, dim3(es_grid(num_nodes)), dim3(256), 0, stream, d_nodePointer_t, d_perm, num_nodes, num_edges, num_heads, d_val,
                       d_out);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}
