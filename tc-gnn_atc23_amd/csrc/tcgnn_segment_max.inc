// tcgnn_segment_max.inc - element-wise maximum over a node's incoming edges (GraphSAGE's max / pool aggregation), its backward over A^T,
// and their C ABI.  Included by tcgnn_device.hip behind tcgnn_gat.inc (whose gat_node / gat_edge clamps it uses), so that `make audit`
// lists the kernels with every other kernel of the library.
//
//   forward   Y[i,d]  = max over e in row i of X[col e, d];   arg[i,d] = the CSR position e that supplied it   (empty row: 0 / -1)
//   backward  dX[j,d] = sum over eT in row j of A^T of dY[i,d] where i = col_t[eT] and arg[i,d] == perm[eT]      (nobody chose j: 0)
//
// The winner of two (value, position) pairs is the greater value; among equal values (-0.0 == +0.0) the smaller position; a NaN beats
// every number, and among NaNs the smaller position wins: numpy.argmax over the row's slice.  The combine is associative and
// commutative, so the lane layout never shows.  Values travel as BIT PATTERNS and are chosen with compare + select: Y has the bits of
// the X element that won (sign of zero, NaN payload), no arithmetic maximum touches them.
// Scheduling (DESIGN.md 4.12).  A group of G lanes owns one neighbour row, four columns a lane (one 16-byte load); G = the smallest
// power of two >= ceil(D / 4), at most 64; a wavefront takes 64 / G edges a step, kSegUnroll steps in flight, the column ids of the next
// steps read before the rows of these are used.  D > 256 goes as column blocks of 256 (blockIdx.y).  A workgroup of four wavefronts
// owns kSegRowsPerWg consecutive rows and bins them in place, as tcgnn_edge_softmax.inc does: a row of up to kSegWaveRow edges takes
// one wavefront (the four take the workgroup's rows in turn), a longer one the whole workgroup, whose four partial results meet in
// LDS in wavefront order.  With the XCD mapping on (TCGNN_SEGMAX_XCD_MAP, default 1) workgroup b takes chunk (b mod 8) * grid / 8 + b / 8:
// the workgroups that share an XCD's L2 (b mod 8) own a contiguous eighth of the rows.
// VEC = false is the dword form, taken when the rows are not 16-byte aligned (D % 4 != 0 or a base address off 16 bytes): the same
// lanes, four 4-byte loads each - the same results.
// No atomics anywhere, every order fixed: results are bit-identical on repetition.  The backward's sums are fp64, rounded once.
// Row pointers are clamped to [0, E] and a descending pair is an empty row; a column id is clamped to [0, N) and a perm entry outside
// [0, E) reads position 0; nothing outside [0, N D) of Y / arg / dX is written, and every element of them is.

namespace {

constexpr int kSegRowsPerWg = 16, kSegWaveRow = 1024, kSegColBlock = 256, kSegUnroll = 4;

static int g_segmax_xcd_map = [] { const char* e = getenv("TCGNN_SEGMAX_XCD_MAP"); return e ? atoi(e) : 1; }();

struct SegBest {
    uint32_t v[4];   // bit patterns
    int32_t p[4];    // CSR positions; -1: no candidate yet (v = 0)
};

__device__ __forceinline__ bool seg_nan(uint32_t b) { return (b & 0x7fffffffu) > 0x7f800000u; }
// does (b1, p1) win over (b2, p2)?  (two candidates never share a position)
__device__ __forceinline__ bool seg_wins(uint32_t b1, int32_t p1, uint32_t b2, int32_t p2) {
    const float v1 = __uint_as_float(b1), v2 = __uint_as_float(b2);
    const bool num = v1 > v2 || (v1 == v2 && p1 < p2);                  // (false when either is a NaN)
    const bool nan = seg_nan(b1) && (!seg_nan(b2) || p1 < p2);
    return p2 < 0 || (p1 >= 0 && (num || nan));
}
// a lane meets its positions in ascending order: the newcomer has to be strictly better
__device__ __forceinline__ void seg_take(uint32_t& bv, int32_t& bp, uint32_t x, int32_t e) {
    const bool better = bp < 0 || __uint_as_float(x) > __uint_as_float(bv) || (seg_nan(x) && !seg_nan(bv));
    bv = better ? x : bv;
    bp = better ? e : bp;
}

// four consecutive 32-bit words of a row from column d0 on; VEC: one 16-byte load (the caller saw to the alignment and D % 4 == 0)
template <bool VEC>
__device__ __forceinline__ void seg_load4(const uint32_t* __restrict__ row, int32_t d0, int32_t D, uint32_t (&x)[4]) {
    if constexpr (VEC) {
        const uint4 t = *reinterpret_cast<const uint4*>(row + d0);
        x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = d0 + k < D ? row[d0 + k] : 0u;
    }
}

// the workgroup's chunk of kSegRowsPerWg rows (see the header: XCD b mod 8 owns a contiguous eighth)
__device__ __forceinline__ int64_t seg_chunk(int xcd_map) {
    const int64_t b = blockIdx.x;
    return xcd_map ? (b & 7) * (int64_t)(gridDim.x >> 3) + (b >> 3) : b;
}
// its kSegRowsPerWg + 1 row pointers, clamped
__device__ __forceinline__ void seg_load_rows(const int32_t* __restrict__ rowptr, int64_t row0, int32_t N, int64_t E, int64_t* sp) {
    if (threadIdx.x <= kSegRowsPerWg) {
        const int64_t r = row0 + threadIdx.x;
        int64_t v = rowptr[r < N ? r : N];
        v = v < 0 ? 0 : (v > E ? E : v);
        sp[threadIdx.x] = v;
    }
    __syncthreads();
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
// this lane's edges lo + slot, lo + slot + stride, ... of one row, four columns from d0 on
template <bool VEC>
__device__ __forceinline__ void seg_fwd_walk(const uint32_t* __restrict__ X, const int32_t* __restrict__ col, int32_t N, int32_t D, int64_t lo,
                                             int64_t hi, int slot, int stride, int32_t d0, SegBest& b) {
    int64_t e = lo + slot;
    int32_t c[kSegUnroll];
#pragma unroll
    for (int u = 0; u < kSegUnroll; ++u) {
        const int64_t eu = e + (int64_t)u * stride;
        c[u] = eu < hi ? col[eu] : 0;
    }
    while (e < hi) {
        uint32_t x[kSegUnroll][4];
#pragma unroll
        for (int u = 0; u < kSegUnroll; ++u) {
            const int64_t eu = e + (int64_t)u * stride;
            if (eu < hi) seg_load4<VEC>(X + (int64_t)gat_node(c[u], N) * D, d0, D, x[u]);
            else x[u][0] = x[u][1] = x[u][2] = x[u][3] = 0u;
        }
        const int64_t en = e + (int64_t)kSegUnroll * stride;
#pragma unroll
        for (int u = 0; u < kSegUnroll; ++u) {   // the next steps' column ids, before these steps' rows are waited for
            const int64_t eu = en + (int64_t)u * stride;
            c[u] = eu < hi ? col[eu] : 0;
        }
#pragma unroll
        for (int u = 0; u < kSegUnroll; ++u) {
            const int64_t eu = e + (int64_t)u * stride;
            if (eu < hi) {
#pragma unroll
                for (int k = 0; k < 4; ++k) seg_take(b.v[k], b.p[k], x[u][k], (int32_t)eu);
            }
        }
        e = en;
    }
}
// the lane groups of a wavefront (lanes off, 2 off, ... apart hold the same columns): every lane ends with the wavefront's winner
__device__ __forceinline__ void seg_fwd_groups(SegBest& b, int G) {
    for (int off = G; off < 64; off <<= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t ov = __shfl_xor(b.v[k], off);
            const int32_t op = __shfl_xor(b.p[k], off);
            const bool keep = seg_wins(b.v[k], b.p[k], ov, op);
            b.v[k] = keep ? b.v[k] : ov;
            b.p[k] = keep ? b.p[k] : op;
        }
    }
}
__device__ __forceinline__ void seg_fwd_store(const SegBest& b, uint32_t* __restrict__ Y, int32_t* __restrict__ arg, int64_t r, int32_t D, int32_t d0) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (d0 + k < D) {
            Y[r * D + d0 + k] = b.v[k];
            if (arg) arg[r * D + d0 + k] = b.p[k];
        }
}

template <bool VEC>
__global__ __launch_bounds__(256) void segment_max_fwd_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int32_t N, int64_t E,
                                                              const uint32_t* __restrict__ X, int32_t D, int lgG, int xcd_map, uint32_t* __restrict__ Y,
                                                              int32_t* __restrict__ arg) {
    __shared__ int64_t sp[kSegRowsPerWg + 1];
    __shared__ uint32_t sv[4][64][4];
    __shared__ int32_t spos[4][64][4];
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
        SegBest b = {{0u, 0u, 0u, 0u}, {-1, -1, -1, -1}};
        seg_fwd_walk<VEC>(X, col, N, D, lo, active ? hi : lo, grp, eps, d0, b);
        seg_fwd_groups(b, G);
        if (grp == 0 && active) seg_fwd_store(b, Y, arg, row0 + q, D, d0);
    }
    for (int q = 0; q < kSegRowsPerWg && row0 + q < N; ++q) {         // longer rows: the whole workgroup (the trip test is workgroup-uniform)
        const int64_t lo = sp[q], hi = sp[q + 1];
        if (hi - lo <= kSegWaveRow) continue;
        SegBest b = {{0u, 0u, 0u, 0u}, {-1, -1, -1, -1}};
        seg_fwd_walk<VEC>(X, col, N, D, lo, active ? hi : lo, wave * eps + grp, 4 * eps, d0, b);
        seg_fwd_groups(b, G);
        if (grp == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                sv[wave][sub][k] = b.v[k];
                spos[wave][sub][k] = b.p[k];
            }
        }
        __syncthreads();
        if (wave == 0 && grp == 0 && active) {
#pragma unroll
            for (int w = 1; w < 4; ++w)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t ov = sv[w][sub][k];
                    const int32_t op = spos[w][sub][k];
                    const bool keep = seg_wins(b.v[k], b.p[k], ov, op);
                    b.v[k] = keep ? b.v[k] : ov;
                    b.p[k] = keep ? b.p[k] : op;
                }
            seg_fwd_store(b, Y, arg, row0 + q, D, d0);
        }
        __syncthreads();
    }
}

// ---- backward: the same walk over A^T -----------------------------------------------------------------------------------------
// VEC: the rows of arg are 16-byte aligned.  dY is read only where arg names this edge.
template <bool VEC>
__device__ __forceinline__ void seg_bwd_walk(const int32_t* __restrict__ col_t, const int32_t* __restrict__ perm, int32_t N, int64_t E,
                                             const uint32_t* __restrict__ arg, const float* __restrict__ dY, int32_t D, int64_t lo, int64_t hi,
                                             int slot, int stride, int32_t d0, double (&acc)[4]) {
    int64_t e = lo + slot;
    int32_t c[kSegUnroll], p[kSegUnroll];
#pragma unroll
    for (int u = 0; u < kSegUnroll; ++u) {
        const int64_t eu = e + (int64_t)u * stride;
        c[u] = eu < hi ? col_t[eu] : 0;
        p[u] = eu < hi ? perm[eu] : 0;
    }
    while (e < hi) {
        uint32_t a[kSegUnroll][4];
        int64_t at[kSegUnroll];
        uint32_t want[kSegUnroll];
#pragma unroll
        for (int u = 0; u < kSegUnroll; ++u) {
            const int64_t eu = e + (int64_t)u * stride;
            at[u] = (int64_t)gat_node(c[u], N) * D;
            want[u] = (uint32_t)gat_edge(p[u], E);
            if (eu < hi) seg_load4<VEC>(arg + at[u], d0, D, a[u]);
            else a[u][0] = a[u][1] = a[u][2] = a[u][3] = 0xffffffffu;   // (-1: no position)
        }
        const int64_t en = e + (int64_t)kSegUnroll * stride;
#pragma unroll
        for (int u = 0; u < kSegUnroll; ++u) {
            const int64_t eu = en + (int64_t)u * stride;
            c[u] = eu < hi ? col_t[eu] : 0;
            p[u] = eu < hi ? perm[eu] : 0;
        }
#pragma unroll
        for (int u = 0; u < kSegUnroll; ++u) {
            const int64_t eu = e + (int64_t)u * stride;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (eu < hi && d0 + k < D && a[u][k] == want[u]) acc[k] += (double)dY[at[u] + d0 + k];
        }
        e = en;
    }
}
__device__ __forceinline__ void seg_bwd_groups(double (&acc)[4], int G) {
    for (int off = G; off < 64; off <<= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += __shfl_xor(acc[k], off);
    }
}
__device__ __forceinline__ void seg_bwd_store(const double (&acc)[4], float* __restrict__ dX, int64_t r, int32_t D, int32_t d0) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (d0 + k < D) dX[r * D + d0 + k] = (float)acc[k];
}

template <bool VEC>
__global__ __launch_bounds__(256) void segment_max_bwd_kernel(const int32_t* __restrict__ rowptr_t, const int32_t* __restrict__ col_t,
                                                              const int32_t* __restrict__ perm, int32_t N, int64_t E, const uint32_t* __restrict__ arg,
                                                              const float* __restrict__ dY, int32_t D, int lgG, int xcd_map, float* __restrict__ dX) {
    __shared__ int64_t sp[kSegRowsPerWg + 1];
    __shared__ double sacc[4][64][4];
    const int64_t row0 = seg_chunk(xcd_map) * kSegRowsPerWg;
    if (row0 >= N) return;
    seg_load_rows(rowptr_t, row0, N, E, sp);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int G = 1 << lgG, eps = 64 >> lgG, grp = lane >> lgG, sub = lane & (G - 1);
    const int32_t d0 = (int32_t)blockIdx.y * kSegColBlock + 4 * sub;
    const bool active = d0 < D;
    for (int q = wave; q < kSegRowsPerWg && row0 + q < N; q += 4) {
        const int64_t lo = sp[q], hi = sp[q + 1] > lo ? sp[q + 1] : lo;
        if (hi - lo > kSegWaveRow) continue;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        seg_bwd_walk<VEC>(col_t, perm, N, E, arg, dY, D, lo, active ? hi : lo, grp, eps, d0, acc);
        seg_bwd_groups(acc, G);
        if (grp == 0 && active) seg_bwd_store(acc, dX, row0 + q, D, d0);
    }
    for (int q = 0; q < kSegRowsPerWg && row0 + q < N; ++q) {
        const int64_t lo = sp[q], hi = sp[q + 1];
        if (hi - lo <= kSegWaveRow) continue;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        seg_bwd_walk<VEC>(col_t, perm, N, E, arg, dY, D, lo, active ? hi : lo, wave * eps + grp, 4 * eps, d0, acc);
        seg_bwd_groups(acc, G);
        if (grp == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) sacc[wave][sub][k] = acc[k];
        }
        __syncthreads();
        if (wave == 0 && grp == 0 && active) {
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = (sacc[0][sub][k] + sacc[1][sub][k]) + (sacc[2][sub][k] + sacc[3][sub][k]);
            seg_bwd_store(acc, dX, row0 + q, D, d0);
        }
        __syncthreads();
    }
}

// lanes of a group as a power of two: the smallest 2^lg >= ceil(min(D, 256) / 4)
inline int seg_lg_group(int32_t D) {
    const int need = ((D < kSegColBlock ? D : kSegColBlock) + 3) / 4;
    int lg = 0;
    while ((1 << lg) < need) ++lg;
    return lg;
}
inline dim3 seg_grid(int32_t N, int32_t D, int xcd_map) {
    int64_t chunks = ((int64_t)N + kSegRowsPerWg - 1) / kSegRowsPerWg;
    if (xcd_map) chunks = (chunks + 7) / 8 * 8;
    return dim3((unsigned)chunks, (unsigned)((D + kSegColBlock - 1) / kSegColBlock));
}
inline bool seg_rows_aligned(const void* base, int32_t D) { return D % 4 == 0 && (reinterpret_cast<uintptr_t>(base) & 15) == 0; }

} // namespace

extern "C" int tcgnn_segment_max(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges, const float* d_X,
                                 int32_t D, float* d_Y, int32_t* d_arg, void* stream_v) {
    if (num_nodes < 0 || num_edges < 0 || num_edges > 0x7fffffffLL || D < 0)
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_segment_max: bad size (int32 CSR positions only)");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_nodes == 0 || D == 0) return TCGNN_OK;
    const size_t elems = (size_t)num_nodes * (size_t)D;
    if (num_edges == 0) {   // every row is empty
        if (d_Y) HIP_TRY(hipMemsetAsync(d_Y, 0, sizeof(float) * elems, stream));
        if (d_arg) HIP_TRY(hipMemsetAsync(d_arg, 0xff, sizeof(int32_t) * elems, stream));
        return TCGNN_OK;
    }
    if (!d_nodePointer || !d_edgeList || !d_X || !d_Y) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_segment_max: null array");
    const int lg = seg_lg_group(D), xcd = g_segmax_xcd_map ? 1 : 0;
    const dim3 grid = seg_grid(num_nodes, D, xcd), block(256);
    const uint32_t* X = reinterpret_cast<const uint32_t*>(d_X);
    uint32_t* Y = reinterpret_cast<uint32_t*>(d_Y);
    if (seg_rows_aligned(d_X, D))
        hipLaunchKernelGGL(segment_max_fwd_kernel<true>, grid, block, 0, stream, d_nodePointer, d_edgeList, num_nodes, num_edges, X, D, lg, xcd, Y, d_arg);
    else
        hipLaunchKernelGGL(segment_max_fwd_kernel<false>, grid, block, 0, stream, d_nodePointer, d_edgeList, num_nodes, num_edges, X, D, lg, xcd, Y, d_arg);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}

extern "C" int tcgnn_segment_max_backward(const int32_t* d_nodePointer_t, const int32_t* d_edgeList_t, const int32_t* d_perm, int32_t num_nodes,
                                          int64_t num_edges, const int32_t* d_arg, const float* d_dY, int32_t D, float* d_dX, void* stream_v) {
    if (num_nodes < 0 || num_edges < 0 || num_edges > 0x7fffffffLL || D < 0)
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_segment_max_backward: bad size (int32 CSR positions only)");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_nodes == 0 || D == 0) return TCGNN_OK;
    if (num_edges == 0) {   // nobody chose anybody
        if (d_dX) HIP_TRY(hipMemsetAsync(d_dX, 0, sizeof(float) * (size_t)num_nodes * (size_t)D, stream));
        return TCGNN_OK;
    }
    if (!d_nodePointer_t || !d_edgeList_t || !d_perm || !d_arg || !d_dY || !d_dX) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_segment_max_backward: null array");
    const int lg = seg_lg_group(D), xcd = g_segmax_xcd_map ? 1 : 0;
    const dim3 grid = seg_grid(num_nodes, D, xcd), block(256);
    const uint32_t* arg = reinterpret_cast<const uint32_t*>(d_arg);
    if (seg_rows_aligned(d_arg, D))
        hipLaunchKernelGGL(segment_max_bwd_kernel<true>, grid, block, 0, stream, d_nodePointer_t, d_edgeList_t, d_perm, num_nodes, num_edges, arg, d_dY, D, lg,
                           xcd, d_dX);
    else
        hipLaunchKernelGGL(segment_max_bwd_kernel<false>, grid, block, 0, stream, d_nodePointer_t, d_edgeList_t, d_perm, num_nodes, num_edges, arg, d_dY, D, lg,
                           xcd, d_dX);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}
