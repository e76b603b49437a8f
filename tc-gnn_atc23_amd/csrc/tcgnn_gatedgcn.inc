// tcgnn_gatedgcn.inc - GatedGCN with edge features (Bresson & Laurent's layer as "Benchmarking GNNs" trains it, DGL's GatedGCNConv, the
// local layer of GraphGPS): the gate of tcgnn_gated.inc with a per-edge term, Z[e] = k[row e] + q[col e] + c[e], which is also the layer's
// new edge feature - an OUTPUT [E, D] -, the gated MEAN sum(eta v) / (sum(eta) + eps), and both sides of its backward.  Included by
// tcgnn_device.hip behind tcgnn_gated.inc; it uses that file's gate (gt_gate), zero fill (gt_zero) and size check, tcgnn_segment_max.inc's
// scheduling and helpers (seg_chunk, seg_load_rows, seg_bwd_groups, seg_lg_group, seg_grid, seg_rows_aligned), tcgnn_gatv2.inc's gv2_load4
// and tcgnn_gat.inc's gat_node / gat_edge clamps.
//
//   forward  z = fl32(fl32(k[i, d] + q[j, d]) + c[e, d]) -> Z[e, d];  (eta, cc) = gt_gate(z)                      i = row e, j = col e
//            num = sum over e in row i of (double)fl32(eta v[j, d]);  den = sum of (double)eta;  s = den + (double)eps
//            Y[i, d] = s == 0 ? 0 : fl32(num / s);  Den[i, d] = fl32(den)                                          (empty row: 0, 0)
//   row side u = gg_u(dY[i, d], Den[i, d]) = s == 0 ? 0 : fl32((double)dY / s) with s = (double)Den + (double)eps, once per row
//            G[e, d] = fl32(dz + fl32(fl32(eta cc) fl32(u fl32(v[j, d] - Y[i, d])))), dz = dZ[e, d] or 0 without dZ; the gate from Z[e, d]
//            dk[i, d] = fl32(sum over e in row i of (double)G[e, d])
//   source   over the rows of A^T, e = perm[t], i = col_t[t]:  dq[j, d] = fl32(sum (double)G[e, d])
//            dv[j, d] = fl32(sum (double)fl32(eta gg_u(dY[i, d], Den[i, d]))), the gate from Z[e, d]               (nobody reads j: 0, 0)
//
// ONE walk (gatedgcn_kernel) in four modes.  Per position it moves rows of two kinds: GATHERED [N, D] rows, found through a column id and
// re-read by other rows (q and v; v; dY and Den), and STREAMED [E, D] rows, each touched once per call (c in and Z out; Z, dZ in and G
// out; on the source side G and Z, found through perm).  A CSR row's streamed rows are contiguous and a workgroup's sixteen rows are one
// span of c / Z, so a wavefront step reads 64 / G consecutive rows.  Interleaving (DESIGN.md 4.22): kGgUnroll = 4 steps are in flight; a
// step's streamed loads are issued FIRST - their addresses need no id -, its gathers behind them, then the ids of the next four steps,
// and only then is anything waited for: up to 12 (forward, row side with dZ) or 16 (source) 16-byte loads a lane.  Every streamed access
// is non-temporal, load and store, so the once-touched [E, D] traffic does not push the gathered rows out of L2; gathers are plain loads.
// The gate is element-wise: nothing here is a matrix product, the matrix pipe is idle.
// Scheduling is segment_max's: a group of G lanes per edge, four columns a lane, kSegRowsPerWg rows a workgroup of four wavefronts, a row
// of up to kSegWaveRow edges on one wavefront and a longer one on all four, whose fp64 partial sums meet in LDS in wavefront order;
// D > 256 as column blocks; the XCD row mapping under TCGNN_SEGMAX_XCD_MAP.  VEC = false is the dword form (D % 4 != 0 or an operand off
// 16 bytes): the same lanes, the same order, the same bits.  No atomics, every order fixed.  Row pointers are clamped to [0, E] and a
// descending pair is an empty row; a column id is clamped to [0, N), a perm entry outside [0, E) reads position 0.  Positions of Z / G
// that no row covers (rowptr[0] > 0 or rowptr[N] < E; none in a canonical CSR) are zeroed by the first and the last chunk.  A hub row
// stays on one workgroup: hub-row splitting is not built, as everywhere in the family.

namespace {

constexpr int kGgUnroll = kSegUnroll;
enum : int { kGgFwd = 0, kGgBwd = 1, kGgBwdDz = 2, kGgSource = 3 };

typedef float gg_float4 __attribute__((ext_vector_type(4)));

struct GgArgs {
    const float *f0, *f1, *f2;   // the row's own [N, D] rows.   forward: k;  row side: dY, Y, Den
    const float *g0, *g1;        // gathered [N, D] rows.        forward: q, v;  row side: v;  source: dY, Den
    const float *s0, *s1;        // streamed [E, D] rows.        forward: c;  row side: Z, dZ;  source (through perm): G, Z
    float* so;                   // streamed out [E, D].         forward: Z;  row side: G
    float *o0, *o1;              // [N, D] results.              forward: Y, Den;  row side: dk;  source: dq, dv
    double eps;
};

// four consecutive floats of an [E, D] row that this call touches once: non-temporal
template <bool VEC>
__device__ __forceinline__ void gg_stream4(const float* __restrict__ row, int32_t d0, int32_t D, float (&x)[4]) {
    if constexpr (VEC) {
        const gg_float4 t = __builtin_nontemporal_load(reinterpret_cast<const gg_float4*>(row + d0));
        x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = d0 + k < D ? __builtin_nontemporal_load(row + d0 + k) : 0.f;
    }
}
template <bool VEC>
__device__ __forceinline__ void gg_store4(float* __restrict__ row, int32_t d0, int32_t D, const float (&x)[4]) {
    if constexpr (VEC) {
        gg_float4 t;
        t.x = x[0]; t.y = x[1]; t.z = x[2]; t.w = x[3];
        __builtin_nontemporal_store(t, reinterpret_cast<gg_float4*>(row + d0));
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (d0 + k < D) __builtin_nontemporal_store(x[k], row + d0 + k);
    }
}

// the mean's quotient and the backward's u: x / (den + eps) in fp64, rounded once; 0 where the denominator is 0 (a row without edges,
// or eps = 0 under gates that all underflowed)
__device__ __forceinline__ float gg_quot(double x, double den, double eps) {
    const double s = den + eps;
    return s == 0.0 ? 0.f : (float)(x / s);
}

__device__ __forceinline__ void gg_zero4(float (&x)[4]) { x[0] = x[1] = x[2] = x[3] = 0.f; }

// this lane's positions lo + slot, lo + slot + stride, ... of one row, four columns from d0 on.  f0 / f1: the row's own words
// (forward: k[i] / -;  row side: u / Y[i];  source: unused).  a0 / a1: forward num / den;  row side dk / -;  source dq / dv
template <bool VEC, int MODE>
__device__ __forceinline__ void gg_walk(const GgArgs& a, const int32_t* __restrict__ col, const int32_t* __restrict__ perm, int32_t N, int64_t E,
                                        int32_t D, int64_t lo, int64_t hi, int slot, int stride, int32_t d0, const float (&f0)[4],
                                        const float (&f1)[4], double (&a0)[4], double (&a1)[4]) {
#pragma clang fp contract(off)
    constexpr bool SRC = MODE == kGgSource, TWO_G = MODE == kGgFwd || SRC, TWO_S = MODE == kGgBwdDz || SRC;
    int64_t e = lo + slot;
    int32_t c[kGgUnroll];
    [[maybe_unused]] int32_t p[kGgUnroll];
#pragma unroll
    for (int u = 0; u < kGgUnroll; ++u) {
        const int64_t eu = e + (int64_t)u * stride;
        c[u] = eu < hi ? col[eu] : 0;
        if constexpr (SRC) p[u] = eu < hi ? perm[eu] : 0;
    }
    while (e < hi) {
        float s[kGgUnroll][4], x[kGgUnroll][4];
        [[maybe_unused]] float t[kGgUnroll][4], w[kGgUnroll][4];
        if constexpr (!SRC) {   // the streams first: their addresses need no id
#pragma unroll
            for (int u = 0; u < kGgUnroll; ++u) {
                const int64_t eu = e + (int64_t)u * stride;
                if (eu < hi) {
                    gg_stream4<VEC>(a.s0 + eu * D, d0, D, s[u]);
                    if constexpr (TWO_S) gg_stream4<VEC>(a.s1 + eu * D, d0, D, t[u]);
                } else {
                    gg_zero4(s[u]);
                    if constexpr (TWO_S) gg_zero4(t[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kGgUnroll; ++u) {
            const int64_t eu = e + (int64_t)u * stride;
            if (eu < hi) {
                if constexpr (SRC) {
                    const int64_t at = gat_edge(p[u], E) * D;
                    gg_stream4<VEC>(a.s0 + at, d0, D, s[u]);
                    gg_stream4<VEC>(a.s1 + at, d0, D, t[u]);
                }
                const int64_t at = (int64_t)gat_node(c[u], N) * D;
                gv2_load4<VEC>(a.g0 + at, d0, D, x[u]);
                if constexpr (TWO_G) gv2_load4<VEC>(a.g1 + at, d0, D, w[u]);
            } else {
                gg_zero4(x[u]);
                if constexpr (TWO_G) gg_zero4(w[u]);
                if constexpr (SRC) {
                    gg_zero4(s[u]);
                    gg_zero4(t[u]);
                }
            }
        }
        const int64_t en = e + (int64_t)kGgUnroll * stride;
#pragma unroll
        for (int u = 0; u < kGgUnroll; ++u) {   // the next steps' ids, before these steps' rows are waited for
            const int64_t eu = en + (int64_t)u * stride;
            c[u] = eu < hi ? col[eu] : 0;
            if constexpr (SRC) p[u] = eu < hi ? perm[eu] : 0;
        }
#pragma unroll
        for (int u = 0; u < kGgUnroll; ++u) {
            const int64_t eu = e + (int64_t)u * stride;
            if (eu < hi) {
                [[maybe_unused]] float out[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float eta, cc;
                    if constexpr (MODE == kGgFwd) {
                        const float kq = f0[k] + x[u][k];
                        const float z = kq + s[u][k];
                        out[k] = z;
                        gt_gate(z, eta, cc);
                        const float m = eta * w[u][k];
                        a0[k] += (double)m;
                        a1[k] += (double)eta;
                    } else if constexpr (SRC) {
                        gt_gate(t[u][k], eta, cc);
                        const float m = eta * gg_quot((double)x[u][k], (double)w[u][k], a.eps);
                        a0[k] += (double)s[u][k];
                        a1[k] += (double)m;
                    } else {
                        gt_gate(s[u][k], eta, cc);
                        const float dv = x[u][k] - f1[k];
                        const float ud = f0[k] * dv;
                        const float ec = eta * cc;
                        const float gm = ec * ud;
                        float g = 0.f;
                        if constexpr (MODE == kGgBwdDz) g = t[u][k];
                        g = g + gm;
                        out[k] = g;
                        a0[k] += (double)g;
                    }
                }
                if constexpr (!SRC) gg_store4<VEC>(a.so + eu * D, d0, D, out);
            }
        }
        e = en;
    }
}

// zero the positions [lo, hi) of the streamed output (see the header: positions no row covers)
template <bool VEC>
__device__ __forceinline__ void gg_clear(float* __restrict__ so, int32_t D, int64_t lo, int64_t hi, int slot, int stride, int32_t d0) {
    const float zero[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t e = lo + slot; e < hi; e += stride) gg_store4<VEC>(so + e * D, d0, D, zero);
}

template <bool VEC, int MODE>
__global__ __launch_bounds__(256) void gatedgcn_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int32_t* __restrict__ perm,
                                                       int32_t N, int64_t E, GgArgs a, int32_t D, int lgG, int xcd_map) {
    constexpr bool SRC = MODE == kGgSource, ROW = MODE == kGgBwd || MODE == kGgBwdDz, TWO = !ROW;   // TWO: a second fp64 set
    __shared__ int64_t sp[kSegRowsPerWg + 1];
    __shared__ double sacc[2][4][64][4];
    const int64_t row0 = seg_chunk(xcd_map) * kSegRowsPerWg;
    if (row0 >= N) return;   // (the grid is rounded up to a multiple of eight under the XCD mapping)
    seg_load_rows(rowptr, row0, N, E, sp);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int G = 1 << lgG, eps = 64 >> lgG, grp = lane >> lgG, sub = lane & (G - 1);
    const int32_t d0 = (int32_t)blockIdx.y * kSegColBlock + 4 * sub;
    const bool active = d0 < D;
    // the row's results from its sums; only the lanes of group 0 that hold columns come here
    auto store = [&](int64_t r, const double (&a0)[4], const double (&a1)[4]) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (d0 + k < D) {
                if constexpr (MODE == kGgFwd) {
                    a.o0[r * D + d0 + k] = gg_quot(a0[k], a1[k], a.eps);
                    a.o1[r * D + d0 + k] = (float)a1[k];
                } else {
                    a.o0[r * D + d0 + k] = (float)a0[k];
                    if constexpr (SRC) a.o1[r * D + d0 + k] = (float)a1[k];
                }
            }
    };
    for (int pass = 0; pass < 2; ++pass) {   // 0: rows of up to kSegWaveRow edges, a wavefront each in turn; 1: longer rows, the whole workgroup
        for (int q = pass ? 0 : wave; q < kSegRowsPerWg && row0 + q < N; q += pass ? 1 : 4) {
            const int64_t lo = sp[q], hi = sp[q + 1] > lo ? sp[q + 1] : lo;
            if ((hi - lo > kSegWaveRow) != (pass == 1)) continue;   // (workgroup-uniform in pass 1)
            float f0[4] = {0.f, 0.f, 0.f, 0.f}, f1[4] = {0.f, 0.f, 0.f, 0.f};
            if (active) {
                if constexpr (MODE == kGgFwd) gv2_load4<VEC>(a.f0 + (row0 + q) * D, d0, D, f0);
                if constexpr (ROW) {   // u, once per row
                    float dy[4], den[4];
                    gv2_load4<VEC>(a.f0 + (row0 + q) * D, d0, D, dy);
                    gv2_load4<VEC>(a.f1 + (row0 + q) * D, d0, D, f1);
                    gv2_load4<VEC>(a.f2 + (row0 + q) * D, d0, D, den);
#pragma unroll
                    for (int k = 0; k < 4; ++k) f0[k] = gg_quot((double)dy[k], (double)den[k], a.eps);
                }
            }
            double a0[4] = {0.0, 0.0, 0.0, 0.0}, a1[4] = {0.0, 0.0, 0.0, 0.0};
            if (!pass) {
                gg_walk<VEC, MODE>(a, col, perm, N, E, D, lo, active ? hi : lo, grp, eps, d0, f0, f1, a0, a1);
                seg_bwd_groups(a0, G);
                if constexpr (TWO) seg_bwd_groups(a1, G);
                if (grp == 0 && active) store(row0 + q, a0, a1);
            } else {
                gg_walk<VEC, MODE>(a, col, perm, N, E, D, lo, active ? hi : lo, wave * eps + grp, 4 * eps, d0, f0, f1, a0, a1);
                seg_bwd_groups(a0, G);
                if constexpr (TWO) seg_bwd_groups(a1, G);
                if (grp == 0) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        sacc[0][wave][sub][k] = a0[k];
                        if constexpr (TWO) sacc[1][wave][sub][k] = a1[k];
                    }
                }
                __syncthreads();
                if (wave == 0 && grp == 0 && active) {   // the four wavefronts' sums, in wavefront order
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        a0[k] = (sacc[0][0][sub][k] + sacc[0][1][sub][k]) + (sacc[0][2][sub][k] + sacc[0][3][sub][k]);
                        if constexpr (TWO) a1[k] = (sacc[1][0][sub][k] + sacc[1][1][sub][k]) + (sacc[1][2][sub][k] + sacc[1][3][sub][k]);
                    }
                    store(row0 + q, a0, a1);
                }
                __syncthreads();
            }
        }
    }
    if constexpr (!SRC) {
        if (active && row0 == 0) gg_clear<VEC>(a.so, D, 0, sp[0], wave * eps + grp, 4 * eps, d0);
        if (active && row0 + kSegRowsPerWg >= N) gg_clear<VEC>(a.so, D, sp[kSegRowsPerWg], E, wave * eps + grp, 4 * eps, d0);
    }
}

// The family's launch geometry: 256 threads, a workgroup per kSegRowsPerWg rows and 256-column block (seg_grid), the lane group of
// seg_lg_group(D); VEC when D % 4 == 0 and every operand the mode touches is 16-byte aligned.
template <int MODE>
inline int gg_launch(const int32_t* rowptr, const int32_t* col, const int32_t* perm, int32_t N, int64_t E, const GgArgs& a, int32_t D, hipStream_t stream) {
    const int lg = seg_lg_group(D), xcd = g_segmax_xcd_map ? 1 : 0;
    const dim3 grid = seg_grid(N, D, xcd), block(256);
    bool vec = D % 4 == 0;
    for (const void* ptr : {(const void*)a.f0, (const void*)a.f1, (const void*)a.f2, (const void*)a.g0, (const void*)a.g1, (const void*)a.s0,
                            (const void*)a.s1, (const void*)a.so})
        vec = vec && (!ptr || seg_rows_aligned(ptr, D));
    if (vec) hipLaunchKernelGGL((gatedgcn_kernel<true, MODE>), grid, block, 0, stream, rowptr, col, perm, N, E, a, D, lg, xcd);
    else hipLaunchKernelGGL((gatedgcn_kernel<false, MODE>), grid, block, 0, stream, rowptr, col, perm, N, E, a, D, lg, xcd);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}

inline int gg_args_ok(const char* call, int32_t N, int64_t E, int32_t D, float eps) {
    if (const int rc = gt_sizes_ok(call, N, E, D)) return rc;
    if (!(eps >= 0.0f) || eps > 3.0e38f) return fail(TCGNN_ERR_INVALID_ARG, "%s: eps must be a finite number >= 0", call);
    return TCGNN_OK;
}

} // namespace

extern "C" int tcgnn_gatedgcn_forward(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges, const float* d_k,
                                      const float* d_q, const float* d_v, const float* d_c, int32_t D, float eps, float* d_Y, float* d_Z, float* d_Den,
                                      void* stream_v) {
    if (const int rc = gg_args_ok("tcgnn_gatedgcn_forward", num_nodes, num_edges, D, eps)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_nodes == 0 || D == 0) return TCGNN_OK;
    if (!d_Y || !d_Den) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_gatedgcn_forward: null array");
    if (num_edges == 0) return gt_zero(d_Y, d_Den, num_nodes, D, stream);   // every row is empty
    if (!d_nodePointer || !d_edgeList || !d_k || !d_q || !d_v || !d_c || !d_Z) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_gatedgcn_forward: null array");
    const GgArgs a{d_k, nullptr, nullptr, d_q, d_v, d_c, nullptr, d_Z, d_Y, d_Den, (double)eps};
    return gg_launch<kGgFwd>(d_nodePointer, d_edgeList, nullptr, num_nodes, num_edges, a, D, stream);
}

extern "C" int tcgnn_gatedgcn_backward(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges, const float* d_dY,
                                       const float* d_dZ, const float* d_Y, const float* d_Den, const float* d_Z, const float* d_v, int32_t D, float eps,
                                       float* d_G, float* d_dk, void* stream_v) {
    if (const int rc = gg_args_ok("tcgnn_gatedgcn_backward", num_nodes, num_edges, D, eps)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_nodes == 0 || D == 0) return TCGNN_OK;
    if (!d_dk) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_gatedgcn_backward: null array");
    if (num_edges == 0) return gt_zero(d_dk, nullptr, num_nodes, D, stream);
    if (!d_nodePointer || !d_edgeList || !d_dY || !d_Y || !d_Den || !d_Z || !d_v || !d_G) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_gatedgcn_backward: null array");
    const GgArgs a{d_dY, d_Y, d_Den, d_v, nullptr, d_Z, d_dZ, d_G, d_dk, nullptr, (double)eps};
    return d_dZ ? gg_launch<kGgBwdDz>(d_nodePointer, d_edgeList, nullptr, num_nodes, num_edges, a, D, stream)
                : gg_launch<kGgBwd>(d_nodePointer, d_edgeList, nullptr, num_nodes, num_edges, a, D, stream);
}

extern "C" int tcgnn_gatedgcn_source_grad(const int32_t* d_nodePointer_t, const int32_t* d_edgeList_t, const int32_t* d_perm, int32_t num_nodes,
                                          int64_t num_edges, const float* d_G, const float* d_Z, const float* d_dY, const float* d_Den, int32_t D, float eps,
                                          float* d_dq, float* d_dv, void* stream_v) {
    if (const int rc = gg_args_ok("tcgnn_gatedgcn_source_grad", num_nodes, num_edges, D, eps)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_nodes == 0 || D == 0) return TCGNN_OK;
    if (!d_dq || !d_dv) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_gatedgcn_source_grad: null array");
    if (num_edges == 0) return gt_zero(d_dq, d_dv, num_nodes, D, stream);   // nobody reads anybody
    if (!d_nodePointer_t || !d_edgeList_t || !d_perm || !d_G || !d_Z || !d_dY || !d_Den)
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_gatedgcn_source_grad: null array");
    const GgArgs a{nullptr, nullptr, nullptr, d_dY, d_Den, d_G, d_Z, nullptr, d_dq, d_dv, (double)eps};
    return gg_launch<kGgSource>(d_nodePointer_t, d_edgeList_t, d_perm, num_nodes, num_edges, a, D, stream);
}
