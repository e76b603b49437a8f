// tcgnn_edge_message.inc - message passing with a feature VECTOR per edge (DGL's u_add_e / sum, PyG's GINEConv message), its backward, the
// sum of per-edge rows into nodes (DGL's copy_e / sum), and their C ABI.  Included by tcgnn_device.hip behind tcgnn_gatv2.inc; it uses
// tcgnn_segment_max.inc's scheduling and helpers (seg_load4, seg_chunk, seg_load_rows, seg_bwd_groups / seg_bwd_store, seg_lg_group,
// seg_grid, seg_rows_aligned; gat_node / gat_edge for the clamps).
//
//   forward   z = fl32(X[col e, d] + Ef[e, d]);  m = act(z);  Y[i, d] = fl32(sum over e in row i of (double)m)         (empty row: 0)
//   backward  dM[e, d] = dY[row e, d] where act is the identity or !(z <= 0), +0.0 otherwise: the BITS of dY or zero
//   edge sum  Y[r, d] = fl32(sum over positions t of row r of (double)M[perm ? perm[t] : t, d])                       (empty row: 0)
//
// Ef, dM and M are [E, D] row-major in CSR position order, so the rows a CSR row needs are ONE contiguous stream: the lane groups of a
// wavefront take consecutive positions, a step of a wavefront reads 64 / G consecutive rows (1 KB where D = 4 G), and those loads are
// issued before the column ids they do not depend on have arrived.  Ef is read once per call and dM written once: both go past the
// caches' retention (non-temporal), X and dY - which are re-read - do not.
// ReLU is torch.relu / threshold_backward: a NaN z stays NaN going forward and PASSES the gradient going back; -0.0 and +0.0 block it.
// Scheduling (DESIGN.md 4.15): segment_max's unchanged - a group of G lanes per edge, four columns a lane, kUeUnroll steps in flight,
// kSegRowsPerWg rows a workgroup of four wavefronts, a row of up to kSegWaveRow edges on one wavefront and a longer one on all four
// (their fp64 partial sums meet in LDS in wavefront order), D > 256 as column blocks, the XCD row mapping under TCGNN_SEGMAX_XCD_MAP.
// VEC = false is the dword form (D % 4 != 0 or a base address off 16 bytes): the same lanes, the same order, the same bits.
// No atomics, every order fixed.  dM has rows no CSR row covers when rowptr[0] > 0 or rowptr[N] < E: the workgroups of the first and
// of the last chunk zero those, so every element of dM is written (a canonical CSR has none).

namespace {

enum : int { kUeSum = 0, kUeAdd = 1, kUeRelu = 2 };   // what a walk forms of a position: M's row / X[col] + Ef / the ReLU of that
constexpr int kUeUnroll = kSegUnroll;

typedef uint32_t uintx4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool ue_pass(float z) { return !(z <= 0.0f); }   // z > 0 or NaN

// four consecutive words of a row that is read once (Ef) - seg_load4 with a non-temporal hint
template <bool VEC>
__device__ __forceinline__ void ue_stream4(const uint32_t* __restrict__ row, int32_t d0, int32_t D, uint32_t (&x)[4]) {
    if constexpr (VEC) {
        const uintx4 t = __builtin_nontemporal_load(reinterpret_cast<const uintx4*>(row + d0));
        x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = d0 + k < D ? __builtin_nontemporal_load(row + d0 + k) : 0u;
    }
}
// ... and of a row that is written once (dM)
template <bool VEC>
__device__ __forceinline__ void ue_store4(uint32_t* __restrict__ row, int32_t d0, int32_t D, const uint32_t (&x)[4]) {
    if constexpr (VEC) {
        uintx4 t;
        t.x = x[0]; t.y = x[1]; t.z = x[2]; t.w = x[3];
        __builtin_nontemporal_store(t, reinterpret_cast<uintx4*>(row + d0));
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (d0 + k < D) __builtin_nontemporal_store(x[k], row + d0 + k);
    }
}

// ---- forward and edge sum --------------------------------------------------------------------------------------------------------
// this lane's positions lo + slot, lo + slot + stride, ... of one row, four columns from d0 on.  ids: col (kUeAdd / kUeRelu) or perm
// (kUeSum; may be null: the identity)
template <bool VEC, int MODE>
__device__ __forceinline__ void ue_fwd_walk(const uint32_t* __restrict__ X, const int32_t* __restrict__ ids, const uint32_t* __restrict__ Ef, int32_t N,
                                            int64_t E, int32_t D, int64_t lo, int64_t hi, int slot, int stride, int32_t d0, double (&acc)[4]) {
    int64_t e = lo + slot;
    int32_t c[kUeUnroll];
#pragma unroll
    for (int u = 0; u < kUeUnroll; ++u) {
        const int64_t eu = e + (int64_t)u * stride;
        c[u] = ids && eu < hi ? ids[eu] : 0;
    }
    while (e < hi) {
        [[maybe_unused]] uint32_t f[kUeUnroll][4];
        uint32_t x[kUeUnroll][4];
        if constexpr (MODE != kUeSum) {   // the stream first: its addresses need no column id
#pragma unroll
            for (int u = 0; u < kUeUnroll; ++u) {
                const int64_t eu = e + (int64_t)u * stride;
                if (eu < hi) ue_stream4<VEC>(Ef + eu * D, d0, D, f[u]);
                else f[u][0] = f[u][1] = f[u][2] = f[u][3] = 0u;
            }
        }
#pragma unroll
        for (int u = 0; u < kUeUnroll; ++u) {
            const int64_t eu = e + (int64_t)u * stride;
            if constexpr (MODE == kUeSum) {
                if (eu < hi) seg_load4<VEC>(Ef + (ids ? gat_edge(c[u], E) : eu) * D, d0, D, x[u]);
                else x[u][0] = x[u][1] = x[u][2] = x[u][3] = 0u;
            } else {
                if (eu < hi) seg_load4<VEC>(X + (int64_t)gat_node(c[u], N) * D, d0, D, x[u]);
                else x[u][0] = x[u][1] = x[u][2] = x[u][3] = 0u;
            }
        }
        const int64_t en = e + (int64_t)kUeUnroll * stride;
#pragma unroll
        for (int u = 0; u < kUeUnroll; ++u) {   // the next steps' ids, before these steps' rows are waited for
            const int64_t eu = en + (int64_t)u * stride;
            c[u] = ids && eu < hi ? ids[eu] : 0;
        }
#pragma unroll
        for (int u = 0; u < kUeUnroll; ++u) {
            const int64_t eu = e + (int64_t)u * stride;
            if (eu < hi) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float m = __uint_as_float(x[u][k]);
                    if constexpr (MODE != kUeSum) m = m + __uint_as_float(f[u][k]);
                    if constexpr (MODE == kUeRelu) m = ue_pass(m) ? m : 0.0f;
                    acc[k] += (double)m;
                }
            }
        }
        e = en;
    }
}

template <bool VEC, int MODE>
__global__ __launch_bounds__(256) void edge_message_fwd_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ ids, int32_t N, int64_t E,
                                                               const uint32_t* __restrict__ X, const uint32_t* __restrict__ Ef, int32_t D, int lgG,
                                                               int xcd_map, float* __restrict__ Y) {
    __shared__ int64_t sp[kSegRowsPerWg + 1];
    __shared__ double sacc[4][64][4];
    const int64_t row0 = seg_chunk(xcd_map) * kSegRowsPerWg;
    if (row0 >= N) return;   // (the grid is rounded up to a multiple of eight under the XCD mapping)
    seg_load_rows(rowptr, row0, N, E, sp);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int G = 1 << lgG, eps = 64 >> lgG, grp = lane >> lgG, sub = lane & (G - 1);
    const int32_t d0 = (int32_t)blockIdx.y * kSegColBlock + 4 * sub;
    const bool active = d0 < D;
    for (int q = wave; q < kSegRowsPerWg && row0 + q < N; q += 4) {   // rows of up to kSegWaveRow edges: a wavefront each, in turn
        const int64_t lo = sp[q], hi = sp[q + 1] > lo ? sp[q + 1] : lo;
        if (hi - lo > kSegWaveRow) continue;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        ue_fwd_walk<VEC, MODE>(X, ids, Ef, N, E, D, lo, active ? hi : lo, grp, eps, d0, acc);
        seg_bwd_groups(acc, G);
        if (grp == 0 && active) seg_bwd_store(acc, Y, row0 + q, D, d0);
    }
    for (int q = 0; q < kSegRowsPerWg && row0 + q < N; ++q) {         // longer rows: the whole workgroup (the trip test is workgroup-uniform)
        const int64_t lo = sp[q], hi = sp[q + 1];
        if (hi - lo <= kSegWaveRow) continue;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        ue_fwd_walk<VEC, MODE>(X, ids, Ef, N, E, D, lo, active ? hi : lo, wave * eps + grp, 4 * eps, d0, acc);
        seg_bwd_groups(acc, G);
        if (grp == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) sacc[wave][sub][k] = acc[k];
        }
        __syncthreads();
        if (wave == 0 && grp == 0 && active) {
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = (sacc[0][sub][k] + sacc[1][sub][k]) + (sacc[2][sub][k] + sacc[3][sub][k]);
            seg_bwd_store(acc, Y, row0 + q, D, d0);
        }
        __syncthreads();
    }
}

// ---- backward: the same walk, a store per position instead of a sum ------------------------------------------------------------
// dy: this lane's four words of dY[row]; RELU: the mask is recomputed from X[col] + Ef, else nothing but dy is read
template <bool VEC, bool RELU>
__device__ __forceinline__ void ue_bwd_walk(const uint32_t* __restrict__ X, const int32_t* __restrict__ col, const uint32_t* __restrict__ Ef, int32_t N,
                                            int32_t D, int64_t lo, int64_t hi, int slot, int stride, int32_t d0, const uint32_t (&dy)[4],
                                            uint32_t* __restrict__ dM) {
    int64_t e = lo + slot;
    if constexpr (!RELU) {
        for (; e < hi; e += stride) ue_store4<VEC>(dM + e * D, d0, D, dy);
    } else {
        int32_t c[kUeUnroll];
#pragma unroll
        for (int u = 0; u < kUeUnroll; ++u) {
            const int64_t eu = e + (int64_t)u * stride;
            c[u] = eu < hi ? col[eu] : 0;
        }
        while (e < hi) {
            uint32_t f[kUeUnroll][4], x[kUeUnroll][4];
#pragma unroll
            for (int u = 0; u < kUeUnroll; ++u) {
                const int64_t eu = e + (int64_t)u * stride;
                if (eu < hi) ue_stream4<VEC>(Ef + eu * D, d0, D, f[u]);
                else f[u][0] = f[u][1] = f[u][2] = f[u][3] = 0u;
            }
#pragma unroll
            for (int u = 0; u < kUeUnroll; ++u) {
                const int64_t eu = e + (int64_t)u * stride;
                if (eu < hi) seg_load4<VEC>(X + (int64_t)gat_node(c[u], N) * D, d0, D, x[u]);
                else x[u][0] = x[u][1] = x[u][2] = x[u][3] = 0u;
            }
            const int64_t en = e + (int64_t)kUeUnroll * stride;
#pragma unroll
            for (int u = 0; u < kUeUnroll; ++u) {
                const int64_t eu = en + (int64_t)u * stride;
                c[u] = eu < hi ? col[eu] : 0;
            }
#pragma unroll
            for (int u = 0; u < kUeUnroll; ++u) {
                const int64_t eu = e + (int64_t)u * stride;
                if (eu < hi) {
                    uint32_t g[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) g[k] = ue_pass(__uint_as_float(x[u][k]) + __uint_as_float(f[u][k])) ? dy[k] : 0u;
                    ue_store4<VEC>(dM + eu * D, d0, D, g);
                }
            }
            e = en;
        }
    }
}

template <bool VEC, bool RELU>
__global__ __launch_bounds__(256) void edge_message_bwd_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int32_t N, int64_t E,
                                                               const uint32_t* __restrict__ X, const uint32_t* __restrict__ Ef,
                                                               const uint32_t* __restrict__ dY, int32_t D, int lgG, int xcd_map, uint32_t* __restrict__ dM) {
    __shared__ int64_t sp[kSegRowsPerWg + 1];
    const int64_t row0 = seg_chunk(xcd_map) * kSegRowsPerWg;
    if (row0 >= N) return;
    seg_load_rows(rowptr, row0, N, E, sp);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int G = 1 << lgG, eps = 64 >> lgG, grp = lane >> lgG, sub = lane & (G - 1);
    const int32_t d0 = (int32_t)blockIdx.y * kSegColBlock + 4 * sub;
    const bool active = d0 < D;
    for (int q = wave; q < kSegRowsPerWg && row0 + q < N; q += 4) {
        const int64_t lo = sp[q], hi = sp[q + 1] > lo ? sp[q + 1] : lo;
        if (hi - lo > kSegWaveRow || !active || hi == lo) continue;
        uint32_t dy[4];
        seg_load4<VEC>(dY + (row0 + q) * D, d0, D, dy);
        ue_bwd_walk<VEC, RELU>(X, col, Ef, N, D, lo, hi, grp, eps, d0, dy, dM);
    }
    for (int q = 0; q < kSegRowsPerWg && row0 + q < N; ++q) {
        const int64_t lo = sp[q], hi = sp[q + 1];
        if (hi - lo <= kSegWaveRow || !active) continue;
        uint32_t dy[4];
        seg_load4<VEC>(dY + (row0 + q) * D, d0, D, dy);
        ue_bwd_walk<VEC, RELU>(X, col, Ef, N, D, lo, hi, wave * eps + grp, 4 * eps, d0, dy, dM);
    }
    // positions in front of the first row and behind the last (none in a canonical CSR): zero, from the chunks that hold those rows
    const uint32_t zero[4] = {0u, 0u, 0u, 0u};
    if (active && row0 == 0) ue_bwd_walk<VEC, false>(X, col, Ef, N, D, 0, sp[0], wave * eps + grp, 4 * eps, d0, zero, dM);
    if (active && row0 + kSegRowsPerWg >= N) ue_bwd_walk<VEC, false>(X, col, Ef, N, D, sp[kSegRowsPerWg], E, wave * eps + grp, 4 * eps, d0, zero, dM);
}

// The family's launch geometry: 256 threads, a workgroup per kSegRowsPerWg rows and 256-column block (seg_grid), the lane group of
// seg_lg_group(D); VEC when every [.., D] operand the kernel touches with 16-byte accesses is aligned.
struct UeGeom {
    dim3 grid, block;
    int lg, xcd;
};
inline UeGeom ue_geom(int32_t N, int32_t D) {
    const int xcd = g_segmax_xcd_map ? 1 : 0;
    return UeGeom{seg_grid(N, D, xcd), dim3(256), seg_lg_group(D), xcd};
}

inline int ue_sizes_ok(const char* call, int32_t N, int64_t E, int32_t D) {
    if (N < 0 || E < 0 || E > 0x7fffffffLL || D < 0) return fail(TCGNN_ERR_INVALID_ARG, "%s: bad size (int32 CSR positions only)", call);
    return TCGNN_OK;
}

template <int MODE>
inline int ue_launch_fwd(const int32_t* rowptr, const int32_t* ids, int32_t N, int64_t E, const float* X, const float* Ef, int32_t D, float* Y,
                         hipStream_t stream) {
    const UeGeom g = ue_geom(N, D);
    const uint32_t* x = reinterpret_cast<const uint32_t*>(X);
    const uint32_t* f = reinterpret_cast<const uint32_t*>(Ef);
    if (seg_rows_aligned(Ef, D) && (MODE == kUeSum || seg_rows_aligned(X, D)))
        hipLaunchKernelGGL((edge_message_fwd_kernel<true, MODE>), g.grid, g.block, 0, stream, rowptr, ids, N, E, x, f, D, g.lg, g.xcd, Y);
    else
        hipLaunchKernelGGL((edge_message_fwd_kernel<false, MODE>), g.grid, g.block, 0, stream, rowptr, ids, N, E, x, f, D, g.lg, g.xcd, Y);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}

} // namespace

extern "C" int tcgnn_edge_message(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges, const float* d_X,
                                  const float* d_Ef, int32_t D, int32_t act, float* d_Y, void* stream_v) {
    if (const int rc = ue_sizes_ok("tcgnn_edge_message", num_nodes, num_edges, D)) return rc;
    if (act != TCGNN_ACT_IDENTITY && act != TCGNN_ACT_RELU) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_edge_message: unknown act %d", act);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_nodes == 0 || D == 0) return TCGNN_OK;
    if (!d_Y) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_edge_message: null array");
    if (num_edges == 0) {   // every row is empty
        HIP_TRY(hipMemsetAsync(d_Y, 0, sizeof(float) * (size_t)num_nodes * (size_t)D, stream));
        return TCGNN_OK;
    }
    if (!d_nodePointer || !d_edgeList || !d_X || !d_Ef) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_edge_message: null array");
    return act == TCGNN_ACT_RELU ? ue_launch_fwd<kUeRelu>(d_nodePointer, d_edgeList, num_nodes, num_edges, d_X, d_Ef, D, d_Y, stream)
                                 : ue_launch_fwd<kUeAdd>(d_nodePointer, d_edgeList, num_nodes, num_edges, d_X, d_Ef, D, d_Y, stream);
}

extern "C" int tcgnn_edge_sum(const int32_t* d_nodePointer, const int32_t* d_perm, int32_t num_nodes, int64_t num_edges, const float* d_M, int32_t D,
                              float* d_Y, void* stream_v) {
    if (const int rc = ue_sizes_ok("tcgnn_edge_sum", num_nodes, num_edges, D)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_nodes == 0 || D == 0) return TCGNN_OK;
    if (!d_Y) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_edge_sum: null array");
    if (num_edges == 0) {
        HIP_TRY(hipMemsetAsync(d_Y, 0, sizeof(float) * (size_t)num_nodes * (size_t)D, stream));
        return TCGNN_OK;
    }
    if (!d_nodePointer || !d_M) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_edge_sum: null array");
    return ue_launch_fwd<kUeSum>(d_nodePointer, d_perm, num_nodes, num_edges, nullptr, d_M, D, d_Y, stream);
}

extern "C" int tcgnn_edge_message_backward(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges, const float* d_X,
                                           const float* d_Ef, const float* d_dY, int32_t D, int32_t act, float* d_dM, void* stream_v) {
    if (const int rc = ue_sizes_ok("tcgnn_edge_message_backward", num_nodes, num_edges, D)) return rc;
    if (act != TCGNN_ACT_IDENTITY && act != TCGNN_ACT_RELU) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_edge_message_backward: unknown act %d", act);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_edges == 0 || D == 0) return TCGNN_OK;
    if (!d_dM) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_edge_message_backward: null array");
    if (num_nodes == 0) {   // no row covers any position
        HIP_TRY(hipMemsetAsync(d_dM, 0, sizeof(float) * (size_t)num_edges * (size_t)D, stream));
        return TCGNN_OK;
    }
    const bool relu = act == TCGNN_ACT_RELU;
    if (!d_nodePointer || !d_dY || (relu && (!d_edgeList || !d_X || !d_Ef))) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_edge_message_backward: null array");
    const UeGeom g = ue_geom(num_nodes, D);
    const uint32_t* x = reinterpret_cast<const uint32_t*>(d_X);
    const uint32_t* f = reinterpret_cast<const uint32_t*>(d_Ef);
    const uint32_t* dy = reinterpret_cast<const uint32_t*>(d_dY);
    uint32_t* dm = reinterpret_cast<uint32_t*>(d_dM);
    const bool vec = seg_rows_aligned(d_dY, D) && seg_rows_aligned(d_dM, D) && (!relu || (seg_rows_aligned(d_X, D) && seg_rows_aligned(d_Ef, D)));
    if (relu) {
        if (vec)
            hipLaunchKernelGGL((edge_message_bwd_kernel<true, true>), g.grid, g.block, 0, stream, d_nodePointer, d_edgeList, num_nodes, num_edges, x, f, dy, D,
                               g.lg, g.xcd, dm);
        else
            hipLaunchKernelGGL((edge_message_bwd_kernel<false, true>), g.grid, g.block, 0, stream, d_nodePointer, d_edgeList, num_nodes, num_edges, x, f, dy, D,
                               g.lg, g.xcd, dm);
    } else {
        if (vec)
            hipLaunchKernelGGL((edge_message_bwd_kernel<true, false>), g.grid, g.block, 0, stream, d_nodePointer, d_edgeList, num_nodes, num_edges, x, f, dy, D,
                               g.lg, g.xcd, dm);
        else
            hipLaunchKernelGGL((edge_message_bwd_kernel<false, false>), g.grid, g.block, 0, stream, d_nodePointer, d_edgeList, num_nodes, num_edges, x, f, dy, D,
                               g.lg, g.xcd, dm);
    }
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}
