// tcgnn_gated.inc - gated aggregation (Bresson & Laurent's residual gated graph convolution; PyG's ResGatedGraphConv, the core of DGL's
// GatedGCNConv): a sum over a node's incoming edges whose per-edge, per-channel weight is a sigmoid gate of BOTH endpoints, its backward
// over A^T, and their C ABI.  Included by tcgnn_device.hip behind tcgnn_edge_project.inc; it uses tcgnn_segment_max.inc's scheduling
// and helpers (seg_chunk, seg_load_rows, seg_bwd_groups, seg_lg_group, seg_grid, seg_rows_aligned), tcgnn_gatv2.inc's gv2_load4,
// tcgnn_edge_softmax.inc's es_exp and tcgnn_gat.inc's gat_node clamp.
//
//   gate      z = fl32(k[row e, d] + q[col e, d]);  t = es_exp(-|z|);  r = fl32(1 + t);  (eta, c) = z >= 0 ? (1 / r, t / r) : (t / r, 1 / r)
//             eta = sigmoid(z) and c = 1 - eta from ONE exponential and two true divisions: both carry a relative error, eta c never cancels
//   forward   Y[i, d] = fl32(sum over e in row i of (double)fl32(eta v[col e, d]))                                       (empty row: 0)
//             S[i, d] = fl32(sum over e in row i of (double)fl32(fl32(eta c) v[col e, d]))     optional: dk = dY (.) S, formed by the caller
//   source    over the rows of A^T, i = col_t[eT]:  dv[j, d] = fl32(sum (double)fl32(eta dY[i, d]))
//             dq[j, d] = fl32((double)v[j, d] sum (double)fl32(fl32(eta c) dY[i, d]))                              (nobody reads j: 0)
//
// ONE walk serves both directions (gated_kernel): a row owns a FIXED operand that stays in registers (k[i] going forward; q[j], and v[j]
// for the final product, on the source side) and every edge gathers TWO neighbour rows (q and v; k and dY).  z is the sum of the fixed
// and the first gathered word - fp32 addition commutes, so the source side forms the forward's z bit for bit - and the second gathered
// word is multiplied by eta into the first fp64 accumulator set and by fl32(eta c) into the second.  Because S leaves the forward walk,
// training needs no row-side backward kernel and no second gather over A.
// Scheduling (DESIGN.md 4.21): segment_max's - a group of G lanes per edge, four columns a lane (one 16-byte load per gathered row),
// kGtUnroll steps in flight (2 kGtUnroll loads a lane), the column ids of the next steps read before the rows of these are used,
// kSegRowsPerWg rows a workgroup of four wavefronts, a row of up to kSegWaveRow edges on one wavefront and a longer one on all four,
// whose two sets of fp64 partial sums meet in LDS in wavefront order; D > 256 as column blocks, the XCD row mapping under
// TCGNN_SEGMAX_XCD_MAP.  SENS = false (forward without S) drops the second set and its arithmetic; Y's operations are the same.
// VEC = false is the dword form (D % 4 != 0 or an operand off 16 bytes): the same lanes, the same order, the same bits.
// No atomics, every order fixed.  Row pointers are clamped to [0, E] and a descending pair is an empty row; a column id is clamped to
// [0, N); perm is not read.  Every element of the outputs is written and nothing else.  A hub row stays on one workgroup.

namespace {

constexpr int kGtUnroll = kSegUnroll;
enum : int { kGtFwd = 0, kGtFwdSens = 1, kGtSource = 2 };

// eta = sigmoid(z) and c = 1 - eta (see the header); a NaN z gives NaN in both
__device__ __forceinline__ void gt_gate(float z, float& eta, float& c) {
#pragma clang fp contract(off)
    const float t = es_exp(-__builtin_fabsf(z));
    const float r = 1.0f + t;
    const float a = 1.0f / r, b = t / r;
    const bool pos = z >= 0.0f;
    eta = pos ? a : b;
    c = pos ? b : a;
}

// this lane's edges lo + slot, lo + slot + stride, ... of one row, four columns from d0 on.  ga: the gathered gate operand (q / k),
// gb: the gathered factor (v / dY); f: the row's own gate operand
template <bool VEC, bool SENS>
__device__ __forceinline__ void gt_walk(const int32_t* __restrict__ col, const float* ga, const float* gb, int32_t N, int32_t D, int64_t lo, int64_t hi,
                                        int slot, int stride, int32_t d0, const float (&f)[4], double (&a0)[4], double (&a1)[4]) {
    int64_t e = lo + slot;
    int32_t c[kGtUnroll];
#pragma unroll
    for (int u = 0; u < kGtUnroll; ++u) {
        const int64_t eu = e + (int64_t)u * stride;
        c[u] = eu < hi ? col[eu] : 0;
    }
    while (e < hi) {
        float x[kGtUnroll][4], w[kGtUnroll][4];
#pragma unroll
        for (int u = 0; u < kGtUnroll; ++u) {
            const int64_t eu = e + (int64_t)u * stride;
            if (eu < hi) {
                const int64_t at = (int64_t)gat_node(c[u], N) * D;
                gv2_load4<VEC>(ga + at, d0, D, x[u]);
                gv2_load4<VEC>(gb + at, d0, D, w[u]);
            } else {
                x[u][0] = x[u][1] = x[u][2] = x[u][3] = 0.f;
                w[u][0] = w[u][1] = w[u][2] = w[u][3] = 0.f;
            }
        }
        const int64_t en = e + (int64_t)kGtUnroll * stride;
#pragma unroll
        for (int u = 0; u < kGtUnroll; ++u) {   // the next steps' column ids, before these steps' rows are waited for
            const int64_t eu = en + (int64_t)u * stride;
            c[u] = eu < hi ? col[eu] : 0;
        }
#pragma unroll
        for (int u = 0; u < kGtUnroll; ++u) {
            const int64_t eu = e + (int64_t)u * stride;
            if (eu < hi) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float eta, cc;
                    gt_gate(f[k] + x[u][k], eta, cc);
                    a0[k] += (double)(eta * w[u][k]);                         // (a conversion follows each product: nothing to contract)
                    if constexpr (SENS) a1[k] += (double)((eta * cc) * w[u][k]);
                }
            }
        }
        e = en;
    }
}

// MODE kGtFwd / kGtFwdSens: rows of A, fixed = k, ga = q, gb = v, o0 = Y, o1 = S (kGtFwdSens only).
// MODE kGtSource: rows of A^T, fixed = q, fixed_v = v, ga = k, gb = dY, o0 = dv, o1 = dq.
template <bool VEC, int MODE>
__global__ __launch_bounds__(256) void gated_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int32_t N, int64_t E,
                                                    const float* fixed, const float* fixed_v, const float* ga, const float* gb, int32_t D, int lgG,
                                                    int xcd_map, float* __restrict__ o0, float* __restrict__ o1) {
    constexpr bool SENS = MODE != kGtFwd;
    __shared__ int64_t sp[kSegRowsPerWg + 1];
    __shared__ double sacc[2][4][64][4];
    const int64_t row0 = seg_chunk(xcd_map) * kSegRowsPerWg;
    if (row0 >= N) return;   // (the grid is rounded up to a multiple of eight under the XCD mapping)
    seg_load_rows(rowptr, row0, N, E, sp);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int G = 1 << lgG, eps = 64 >> lgG, grp = lane >> lgG, sub = lane & (G - 1);
    const int32_t d0 = (int32_t)blockIdx.y * kSegColBlock + 4 * sub;
    const bool active = d0 < D;
    // the row's results from its two sums; only the lanes of group 0 that hold columns come here
    auto store = [&](int64_t r, const double (&a0)[4], const double (&a1)[4], const float (&fv)[4]) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (d0 + k < D) {
                o0[r * D + d0 + k] = (float)a0[k];
                if constexpr (MODE == kGtFwdSens) o1[r * D + d0 + k] = (float)a1[k];
                if constexpr (MODE == kGtSource) o1[r * D + d0 + k] = (float)((double)fv[k] * a1[k]);
            }
    };
    for (int pass = 0; pass < 2; ++pass) {   // 0: rows of up to kSegWaveRow edges, a wavefront each in turn; 1: longer rows, the whole workgroup
        for (int q = pass ? 0 : wave; q < kSegRowsPerWg && row0 + q < N; q += pass ? 1 : 4) {
            const int64_t lo = sp[q], hi = sp[q + 1] > lo ? sp[q + 1] : lo;
            if ((hi - lo > kSegWaveRow) != (pass == 1)) continue;   // (workgroup-uniform in pass 1)
            float f[4] = {0.f, 0.f, 0.f, 0.f}, fv[4] = {0.f, 0.f, 0.f, 0.f};
            if (active) {
                gv2_load4<VEC>(fixed + (row0 + q) * D, d0, D, f);
                if constexpr (MODE == kGtSource) gv2_load4<VEC>(fixed_v + (row0 + q) * D, d0, D, fv);
            }
            double a0[4] = {0.0, 0.0, 0.0, 0.0}, a1[4] = {0.0, 0.0, 0.0, 0.0};
            if (!pass) {
                gt_walk<VEC, SENS>(col, ga, gb, N, D, lo, active ? hi : lo, grp, eps, d0, f, a0, a1);
                seg_bwd_groups(a0, G);
                if constexpr (SENS) seg_bwd_groups(a1, G);
                if (grp == 0 && active) store(row0 + q, a0, a1, fv);
            } else {
                gt_walk<VEC, SENS>(col, ga, gb, N, D, lo, active ? hi : lo, wave * eps + grp, 4 * eps, d0, f, a0, a1);
                seg_bwd_groups(a0, G);
                if constexpr (SENS) seg_bwd_groups(a1, G);
                if (grp == 0) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        sacc[0][wave][sub][k] = a0[k];
                        if constexpr (SENS) sacc[1][wave][sub][k] = a1[k];
                    }
                }
                __syncthreads();
                if (wave == 0 && grp == 0 && active) {   // the four wavefronts' sums, in wavefront order
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        a0[k] = (sacc[0][0][sub][k] + sacc[0][1][sub][k]) + (sacc[0][2][sub][k] + sacc[0][3][sub][k]);
                        if constexpr (SENS) a1[k] = (sacc[1][0][sub][k] + sacc[1][1][sub][k]) + (sacc[1][2][sub][k] + sacc[1][3][sub][k]);
                    }
                    store(row0 + q, a0, a1, fv);
                }
                __syncthreads();
            }
        }
    }
}

// an output of a call without edges: zero, by a kernel (a memset node would not replay in a captured graph everywhere)
__global__ __launch_bounds__(256) void gated_zero_kernel(float* __restrict__ a, float* __restrict__ b, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (a) a[i] = 0.f;
        if (b) b[i] = 0.f;
    }
}

inline int gt_zero(float* a, float* b, int32_t N, int32_t D, hipStream_t stream) {
    const int64_t n = (int64_t)N * D;
    const unsigned blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(gated_zero_kernel, dim3(blocks), dim3(256), 0, stream, a, b, n);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}

inline int gt_sizes_ok(const char* call, int32_t N, int64_t E, int32_t D) {
    if (N < 0 || E < 0 || E > 0x7fffffffLL || D < 0) return fail(TCGNN_ERR_INVALID_ARG, "%s: bad size (int32 CSR positions only)", call);
    return TCGNN_OK;
}

// the family's launch geometry (seg_grid, seg_lg_group); VEC when every gathered and fixed [N, D] operand is 16-byte aligned and D % 4 == 0
template <int MODE>
inline int gt_launch(const int32_t* rowptr, const int32_t* col, int32_t N, int64_t E, const float* fixed, const float* fixed_v, const float* ga,
                     const float* gb, int32_t D, float* o0, float* o1, hipStream_t stream) {
    const int lg = seg_lg_group(D), xcd = g_segmax_xcd_map ? 1 : 0;
    const dim3 grid = seg_grid(N, D, xcd), block(256);
    const bool vec = seg_rows_aligned(fixed, D) && seg_rows_aligned(ga, D) && seg_rows_aligned(gb, D) && (!fixed_v || seg_rows_aligned(fixed_v, D));
    if (vec) hipLaunchKernelGGL((gated_kernel<true, MODE>), grid, block, 0, stream, rowptr, col, N, E, fixed, fixed_v, ga, gb, D, lg, xcd, o0, o1);
    else hipLaunchKernelGGL((gated_kernel<false, MODE>), grid, block, 0, stream, rowptr, col, N, E, fixed, fixed_v, ga, gb, D, lg, xcd, o0, o1);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}

} // namespace

extern "C" int tcgnn_gated_sum(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges, const float* d_k,
                               const float* d_q, const float* d_v, int32_t D, float* d_Y, float* d_S, void* stream_v) {
    if (const int rc = gt_sizes_ok("tcgnn_gated_sum", num_nodes, num_edges, D)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_nodes == 0 || D == 0) return TCGNN_OK;
    if (!d_Y) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_gated_sum: null array");
    if (num_edges == 0) return gt_zero(d_Y, d_S, num_nodes, D, stream);   // every row is empty
    if (!d_nodePointer || !d_edgeList || !d_k || !d_q || !d_v) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_gated_sum: null array");
    return d_S ? gt_launch<kGtFwdSens>(d_nodePointer, d_edgeList, num_nodes, num_edges, d_k, nullptr, d_q, d_v, D, d_Y, d_S, stream)
               : gt_launch<kGtFwd>(d_nodePointer, d_edgeList, num_nodes, num_edges, d_k, nullptr, d_q, d_v, D, d_Y, nullptr, stream);
}

extern "C" int tcgnn_gated_source_grad(const int32_t* d_nodePointer_t, const int32_t* d_edgeList_t, const int32_t* d_perm, int32_t num_nodes,
                                       int64_t num_edges, const float* d_k, const float* d_q, const float* d_v, const float* d_dY, int32_t D,
                                       float* d_dq, float* d_dv, void* stream_v) {
    (void)d_perm;   // (the values do not depend on A's positions)
    if (const int rc = gt_sizes_ok("tcgnn_gated_source_grad", num_nodes, num_edges, D)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_nodes == 0 || D == 0) return TCGNN_OK;
    if (!d_dq || !d_dv) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_gated_source_grad: null array");
    if (num_edges == 0) return gt_zero(d_dv, d_dq, num_nodes, D, stream);   // nobody reads anybody
    if (!d_nodePointer_t || !d_edgeList_t || !d_k || !d_q || !d_v || !d_dY) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_gated_source_grad: null array");
    return gt_launch<kGtSource>(d_nodePointer_t, d_edgeList_t, num_nodes, num_edges, d_q, d_v, d_k, d_dY, D, d_dv, d_dq, stream);
}
