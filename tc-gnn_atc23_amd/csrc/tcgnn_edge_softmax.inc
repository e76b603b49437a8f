// tcgnn_edge_softmax.inc - softmax over a node's incoming edges (DGL's edge_softmax: by CSR row), forward and backward, and their
// C ABI.  Included by tcgnn_device.hip so that `make audit` lists the kernels with every other kernel of the library.
//
//   forward   p[e] = exp(b s[e] - m_r) / sum_{row r} exp(b s[e'] - m_r),  m_r = max over row r of b s      (b = *beta, 1 when null)
//   backward  g[e] = p[e] (dp[e] - sum_{row} p dp),  ds[e] = b g[e],  *dbeta = sum_e s[e] g[e]
//
// Scheduling (DESIGN.md 4.10).  A workgroup of four wavefronts owns 32 consecutive rows and bins them by length, read from
// nodePointer inside the kernel (no list, no scratch, one launch):
//   1 .. 16 edges      a group of EIGHT lanes per row, two values per lane: the 32 rows of the workgroup at once;
//   17 .. 1024 edges   a wavefront per row, up to sixteen values per lane IN REGISTERS across max, exp, sum and divide - every value is
//                      read once and written once (a wavefront takes those of its eight rows one after the other);
//   beyond             the whole workgroup per row, three strided read passes (max; sum, accumulated in fp64; the quotients) - the
//                      second and third find the row in L2.  A hub row of 300 000 edges is 1 172 trips of 256 lanes, not 4 700 of 64.
// Every reduction has a fixed order - the lane's own values pairwise, a butterfly over the lanes (in fp64), the four wavefronts through LDS -
// and nothing is accumulated with atomics: results are bit-identical on repetition.  d_beta's sum leaves each workgroup as one fp64
// partial in the caller's scratch; a second, single-workgroup kernel adds them in index order.
// The exponent is formed as fma(b, s, -m): the product is not rounded before the maximum is subtracted, so the error of p follows
// |b s - m|, not |b s| (scores of 1e4 stay within the bound of tests/edge_ops_ref.py).
// Row pointers are clamped to [0, E] and a descending pair is an empty row: whatever the array holds, nothing outside [0, E) is touched.
// d_p may alias d_score and d_ds may alias d_dp: a thread reads position e of every input before it writes position e, and no other
// thread reads that position afterwards (the workgroup passes are separated by barriers).

namespace {

constexpr int kEsRowsPerWg = 32, kEsRowsPerWave = 8, kEsShort = 16, kEsMedium = 1024;
constexpr float kEsLog2e = 1.4426950408889634f;

__device__ __forceinline__ float es_exp(float d) { return __builtin_amdgcn_exp2f(d * kEsLog2e); }   // v_exp_f32

template <int W>
__device__ __forceinline__ float es_max(float v) {
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}
template <int W, typename T>
__device__ __forceinline__ T es_sum(T v) {
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
template <int NK, typename T>
__device__ __forceinline__ T es_pairwise(T (&t)[NK]) {   // (destroys t)
#pragma unroll
    for (int w = 1; w < NK; w <<= 1)
#pragma unroll
        for (int k = 0; k + w < NK; k += 2 * w) t[k] += t[k + w];
    return t[0];
}
// the workgroup's 33 row pointers, clamped
__device__ __forceinline__ void es_load_rows(const int32_t* __restrict__ rowptr, int32_t N, int64_t E, int64_t* sp) {
    if (threadIdx.x <= kEsRowsPerWg) {
        const int64_t r = (int64_t)blockIdx.x * kEsRowsPerWg + threadIdx.x;
        int64_t v = rowptr[r < N ? r : N];
        v = v < 0 ? 0 : (v > E ? E : v);
        sp[threadIdx.x] = v;
    }
    __syncthreads();
}
__device__ __forceinline__ float es_block_max(float v, float* red) {
    v = es_max<64>(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    return v;
}
__device__ __forceinline__ double es_block_sum(double v, double* red) {
    v = es_sum<64>(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return v;
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
// W lanes per row, NK values per lane (W * NK >= the row's length): the row lives in registers from its one read to its one write
template <int W, int NK>
__device__ __forceinline__ void es_fwd_row(const float* s, float* p, int64_t lo, int64_t hi, float b, int sub) {
    float v[NK], ex[NK];
    double t[NK];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int64_t e = lo + k * W + sub;
        v[k] = e < hi ? s[e] : 0.f;
        if (e < hi) m = fmaxf(m, b * v[k]);
    }
    m = es_max<W>(m);
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int64_t e = lo + k * W + sub;
        ex[k] = e < hi ? es_exp(__builtin_fmaf(b, v[k], -m)) : 0.f;
        t[k] = ex[k];
    }
    // the row sum and the quotient in fp64: an fp32 sum drops what lies below half an ulp of its largest term, which alone costs a p
    // near 1 more than the 1e-7 it is allowed (a row of 65 536 edges under one dominant score); p = ex / sum then rounds once
    const double inv = 1.0 / es_sum<W>(es_pairwise<NK>(t));
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int64_t e = lo + k * W + sub;
        if (e < hi) p[e] = (float)((double)ex[k] * inv);
    }
}

// every row of the workgroup (sp: its 33 clamped row pointers), binned by length as the header says; score may be p itself
__device__ __forceinline__ void es_fwd_rows(const int64_t* sp, const float* score, float* p, float b, float* redf, double* redd) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    {   // rows of 1 .. 16 edges: eight lanes each
        const int r = wave * kEsRowsPerWave + (lane >> 3);
        const int64_t lo = sp[r], len = sp[r + 1] - lo;
        const bool mine = len >= 1 && len <= kEsShort;
        es_fwd_row<8, 2>(score, p, lo, mine ? lo + len : lo, b, lane & 7);
    }
    for (int q = 0; q < kEsRowsPerWave; ++q) {   // rows of 17 .. 1024 edges: this wavefront's, one after the other
        const int r = wave * kEsRowsPerWave + q;
        const int64_t lo = sp[r], hi = sp[r + 1];
        const int len = __builtin_amdgcn_readfirstlane((int)(hi - lo));
        if (len <= kEsShort || len > kEsMedium) continue;
        if (len <= 64) es_fwd_row<64, 1>(score, p, lo, hi, b, lane);
        else if (len <= 128) es_fwd_row<64, 2>(score, p, lo, hi, b, lane);
        else if (len <= 256) es_fwd_row<64, 4>(score, p, lo, hi, b, lane);
        else if (len <= 512) es_fwd_row<64, 8>(score, p, lo, hi, b, lane);
        else es_fwd_row<64, 16>(score, p, lo, hi, b, lane);
    }
    for (int r = 0; r < kEsRowsPerWg; ++r) {     // longer rows: the whole workgroup (the trip test is workgroup-uniform)
        const int64_t lo = sp[r], hi = sp[r + 1];
        if (hi - lo <= kEsMedium) continue;
        float m = -INFINITY;
#pragma unroll 4
        for (int64_t e = lo + threadIdx.x; e < hi; e += 256) m = fmaxf(m, b * score[e]);
        m = es_block_max(m, redf);
        double acc = 0.0;
#pragma unroll 4
        for (int64_t e = lo + threadIdx.x; e < hi; e += 256) acc += (double)es_exp(__builtin_fmaf(b, score[e], -m));
        const double inv = 1.0 / es_block_sum(acc, redd);
#pragma unroll 4
        for (int64_t e = lo + threadIdx.x; e < hi; e += 256) p[e] = (float)((double)es_exp(__builtin_fmaf(b, score[e], -m)) * inv);
    }
}

__global__ __launch_bounds__(256) void edge_softmax_fwd_kernel(const int32_t* __restrict__ rowptr, int32_t N, int64_t E, const float* score,
                                                               const float* __restrict__ beta, float* p) {
    __shared__ int64_t sp[kEsRowsPerWg + 1];
    __shared__ float redf[4];
    __shared__ double redd[4];
    es_load_rows(rowptr, N, E, sp);
    es_fwd_rows(sp, score, p, beta ? beta[0] : 1.0f, redf, redd);
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
template <int W, int NK, bool DB>
__device__ __forceinline__ void es_bwd_row(const float* __restrict__ p, const float* dp, const float* __restrict__ s, float* ds, int64_t lo,
                                           int64_t hi, float b, int sub, double& dbeta) {
    float pv[NK], dv[NK];
    double t[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int64_t e = lo + k * W + sub;
        pv[k] = e < hi ? p[e] : 0.f;
        dv[k] = e < hi ? dp[e] : 0.f;
        t[k] = (double)pv[k] * (double)dv[k];
    }
    // sum_row p dp and the difference dp - sum in fp64: where one p is close to 1 the sum is close to that edge's dp, and an fp32 sum
    // would leave the difference - g, and with it d_beta = sum s g, whose terms cancel - with the rounding error of the SUM
    const double dot = es_sum<W>(es_pairwise<NK>(t));
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int64_t e = lo + k * W + sub;
        const float g = pv[k] * (float)((double)dv[k] - dot);
        if (e < hi) {
            ds[e] = b * g;
            if constexpr (DB) dbeta += (double)s[e] * (double)g;
        }
    }
}

// every row of the workgroup, binned as in forward; dbeta: this thread's share of sum s g (DB only).  score is read where DB
template <bool DB>
__device__ __forceinline__ void es_bwd_rows(const int64_t* sp, const float* __restrict__ p, const float* dp, const float* __restrict__ score, float* ds,
                                            float b, double* redd, double& dbeta) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    {
        const int r = wave * kEsRowsPerWave + (lane >> 3);
        const int64_t lo = sp[r], len = sp[r + 1] - lo;
        const bool mine = len >= 1 && len <= kEsShort;
        es_bwd_row<8, 2, DB>(p, dp, score, ds, lo, mine ? lo + len : lo, b, lane & 7, dbeta);
    }
    for (int q = 0; q < kEsRowsPerWave; ++q) {
        const int r = wave * kEsRowsPerWave + q;
        const int64_t lo = sp[r], hi = sp[r + 1];
        const int len = __builtin_amdgcn_readfirstlane((int)(hi - lo));
        if (len <= kEsShort || len > kEsMedium) continue;
        if (len <= 64) es_bwd_row<64, 1, DB>(p, dp, score, ds, lo, hi, b, lane, dbeta);
        else if (len <= 128) es_bwd_row<64, 2, DB>(p, dp, score, ds, lo, hi, b, lane, dbeta);
        else if (len <= 256) es_bwd_row<64, 4, DB>(p, dp, score, ds, lo, hi, b, lane, dbeta);
        else if (len <= 512) es_bwd_row<64, 8, DB>(p, dp, score, ds, lo, hi, b, lane, dbeta);
        else es_bwd_row<64, 16, DB>(p, dp, score, ds, lo, hi, b, lane, dbeta);
    }
    for (int r = 0; r < kEsRowsPerWg; ++r) {
        const int64_t lo = sp[r], hi = sp[r + 1];
        if (hi - lo <= kEsMedium) continue;
        double acc = 0.0;
#pragma unroll 4
        for (int64_t e = lo + threadIdx.x; e < hi; e += 256) acc += (double)p[e] * (double)dp[e];
        const double dot = es_block_sum(acc, redd);
#pragma unroll 4
        for (int64_t e = lo + threadIdx.x; e < hi; e += 256) {
            const float g = p[e] * (float)((double)dp[e] - dot);
            ds[e] = b * g;
            if constexpr (DB) dbeta += (double)score[e] * (double)g;
        }
    }
}

template <bool DB>
__global__ __launch_bounds__(256) void edge_softmax_bwd_kernel(const int32_t* __restrict__ rowptr, int32_t N, int64_t E, const float* __restrict__ p,
                                                               const float* dp, const float* __restrict__ score, const float* __restrict__ beta,
                                                               float* ds, double* __restrict__ partial) {
    __shared__ int64_t sp[kEsRowsPerWg + 1];
    __shared__ double redd[4];
    es_load_rows(rowptr, N, E, sp);
    double dbeta = 0.0;
    es_bwd_rows<DB>(sp, p, dp, score, ds, beta ? beta[0] : 1.0f, redd, dbeta);
    if constexpr (DB) {
        const double total = es_block_sum(dbeta, redd);
        if (threadIdx.x == 0) partial[blockIdx.x] = total;
    }
}

// *out = the workgroups' partial sums, added in index order per thread and then in the fixed tree: one workgroup
__global__ __launch_bounds__(256) void edge_softmax_dbeta_kernel(const double* __restrict__ partial, int32_t n, float* __restrict__ out) {
    __shared__ double redd[4];
    double acc = 0.0;
    for (int32_t k = threadIdx.x; k < n; k += 256) acc += partial[k];
    const double total = es_block_sum(acc, redd);
    if (threadIdx.x == 0) out[0] = (float)total;
}

inline unsigned es_grid(int32_t N) { return (unsigned)(((int64_t)N + kEsRowsPerWg - 1) / kEsRowsPerWg); }
inline size_t es_partial_bytes(int32_t N) { return ((size_t)es_grid(N) * sizeof(double) + 255) / 256 * 256; }

} // namespace

extern "C" size_t tcgnn_edge_softmax_workspace_bytes(int32_t num_nodes, int64_t num_edges) {
    return num_nodes > 0 && num_edges >= 0 ? es_partial_bytes(num_nodes) : 0;
}

extern "C" int tcgnn_edge_softmax(const int32_t* d_nodePointer, int32_t num_nodes, int64_t num_edges, const float* d_score, const float* d_beta,
                                  float* d_p, void* stream) {
    if (num_nodes < 0 || num_edges < 0 || num_edges > 0x7fffffffLL) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_edge_softmax: bad size (int32 CSR positions only)");
    if (num_nodes == 0 || num_edges == 0) return TCGNN_OK;
    if (!d_nodePointer || !d_score || !d_p) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_edge_softmax: null array");
    hipLaunchKernelGGL(edge_softmax_fwd_kernel, dim3(es_grid(num_nodes)), dim3(256), 0, static_cast<hipStream_t>(stream), d_nodePointer, num_nodes,
                       num_edges, d_score, d_beta, d_p);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}

extern "C" int tcgnn_edge_softmax_backward(const int32_t* d_nodePointer, int32_t num_nodes, int64_t num_edges, const float* d_p, const float* d_dp,
                                           const float* d_score, const float* d_beta, float* d_ds, float* d_dbeta, void* d_scratch,
                                           size_t scratch_bytes, void* stream_v) {
    if (num_nodes < 0 || num_edges < 0 || num_edges > 0x7fffffffLL) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_edge_softmax_backward: bad size (int32 CSR positions only)");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_nodes == 0 || num_edges == 0) {
        if (d_dbeta) HIP_TRY(hipMemsetAsync(d_dbeta, 0, sizeof(float), stream));
        return TCGNN_OK;
    }
    if (!d_nodePointer || !d_p || !d_dp || !d_ds) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_edge_softmax_backward: null array");
    const dim3 grid(es_grid(num_nodes)), block(256);
    if (!d_dbeta) {
        hipLaunchKernelGGL(edge_softmax_bwd_kernel<false>, grid, block, 0, stream, d_nodePointer, num_nodes, num_edges, d_p, d_dp, (const float*)nullptr, d_beta,
                           d_ds, (double*)nullptr);
        HIP_TRY(hipGetLastError());
        return TCGNN_OK;
    }
    if (!d_score) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_edge_softmax_backward: d_dbeta needs d_score");
    const size_t need = es_partial_bytes(num_nodes);
    if (!d_scratch || scratch_bytes < need || (reinterpret_cast<uintptr_t>(d_scratch) & 7))
        return fail(TCGNN_ERR_WORKSPACE, "tcgnn_edge_softmax_backward: scratch needs %zu bytes 8-aligned (tcgnn_edge_softmax_workspace_bytes), got %zu at %p", need,
                    scratch_bytes, d_scratch);
    double* const partial = static_cast<double*>(d_scratch);
    hipLaunchKernelGGL(edge_softmax_bwd_kernel<true>, grid, block, 0, stream, d_nodePointer, num_nodes, num_edges, d_p, d_dp, d_score, d_beta, d_ds, partial);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(edge_softmax_dbeta_kernel, dim3(1), dim3(256), 0, stream, (const double*)partial, (int32_t)grid.x, d_dbeta);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}
