// tcgnn_gatv2.inc - GATv2 attention (Brody et al.; DGL's / PyG's GATv2Conv): the scores and their softmax over a node's incoming edges in
// ONE launch, the row-side backward (g, d_xr, d_attn) in one launch plus a small reduction, the source-side backward (d_xl) over A^T,
// and their C ABI.  Included by tcgnn_device.hip behind tcgnn_segment_max.inc, so that `make audit` lists the kernels; it uses
// tcgnn_edge_softmax.inc's row schedule and reductions (es_*) and tcgnn_gat.inc's roundings and clamps (gat_score, gat_mul_rn, gat_node,
// gat_edge) as they are.
//
//   forward   z = fl32(xl[col e, hF+f] + xr[row e, hF+f]),  l = z > 0 ? z : fl32(z slope);   s[h,e] = fl32(sum_f (double)attn[h,f] (double)l)
//             p[h,.] = softmax of s[h,.] over each row - tcgnn_edge_softmax's arithmetic with beta = 1 (es_fwd_rows, the same code)
//   row side  g = p (dp - sum_row p dp) (es_bwd_rows, beta = 1);  c = z > 0 ? attn[h,f] : fl32(attn[h,f] slope)
//             d_xr[i, hF+f] = fl32(sum_{e in row i} (double)fl32(g[h,e] c));   d_attn[h,f] = fl32(sum_e (double)g[h,e] (double)l)
//   source    d_xl[j, hF+f] = fl32(sum_{eT in row j of A^T} (double)fl32(g[h, perm eT] c)),  z = fl32(xl[j] + xr[col_t eT])
//
// The non-linearity sits in front of the attention vector, so unlike GAT's the score does not split into two per-node scalars: every edge
// needs the whole H F-wide source row.  The gather is tcgnn_segment_max.inc's: a GROUP of lanes owns one neighbour row, four columns
// (one 16-byte load) per lane, kGv2Unroll edges per lane group in flight.  Within a group the lanes are dealt out per HEAD (gv2_geom, the
// one place that says how): L = the smallest power of two >= ceil(F / 4) lanes, at most 64, hold one head's F columns - F > 256 in
// chunks of 4 L - and a group is as many heads as fit in a wavefront (a power of two >= H, at most 64 / L); heads beyond a group take
// another pass.  The lanes of one head reduce among themselves (an fp64 butterfly over L lanes), so any H >= 1 and F >= 1 goes, at the
// price of idle lanes where H or ceil(F / 4) is no power of two (H = 3: a quarter; (5, 24): half).
// Schedule: a workgroup of four wavefronts owns the 32 consecutive rows of tcgnn_edge_softmax.inc's workgroup.  Score pass: rows of up to
// kGv2WaveRow edges take a wavefront each in turn, longer ones the whole workgroup; every neighbour row is gathered once and every score
// formed once, rounded, and PARKED in its slot of p (and written to d_score where given).  Behind a barrier the softmax runs in place
// over those slots, head by head, in es_fwd_rows' bins - 4 bytes written and read again per head-edge beside the 4 F gathered.
// Backward walks a row once per column pass: the lane's four fp64 sums for d_xr / d_xl and four for d_attn (16 VGPRs) live across the
// row, long rows meet in LDS in wavefront order, and d_attn leaves each workgroup as fp64 partials [H F][workgroups] in the caller's
// scratch, which gatv2_dattn_kernel adds in workgroup order.
// VEC = false is the dword form, taken when F % 4 != 0 or a base address is off 16 bytes: the same lanes, four 4-byte loads each - the
// same bits.  No atomics anywhere, every order fixed: results are bit-identical on repetition.
// Row pointers are clamped to [0, E] (es_load_rows) and a descending pair is an empty row; a column id is clamped to [0, N) and a perm
// entry outside [0, E) reads position 0; nothing outside [0, E) of a head's row of p / score / g and nothing outside [0, N H F) of
// d_xr / d_xl is written, and every element of those two is.  g may alias dp (es_bwd_rows reads position e before it writes it).

namespace {

constexpr int kGv2WaveRow = kEsMedium, kGv2Unroll = 4;

// the lane layout of one (H, F): lgL = log2 of the lanes per head, lgHp = log2 of the heads per lane group
struct Gv2Geom {
    int lgL, lgHp;
};
inline Gv2Geom gv2_geom(int32_t H, int32_t F) {
    Gv2Geom g{0, 0};
    const int need = (F + 3) / 4;
    while ((1 << g.lgL) < need && g.lgL < 6) ++g.lgL;
    while ((1 << g.lgHp) < H && g.lgL + g.lgHp < 6) ++g.lgHp;
    return g;
}

// what a lane is within the layout, and the column passes of a walk: pass cp covers heads (cp / fchunks) hpg .. + hpg, of each the
// columns (cp % fchunks) 4 L .. + 4 L
struct Gv2Lane {
    int L, G, eps, sub, hg, grp, hpg, fchunks, passes;
    __device__ __forceinline__ Gv2Lane(int lgL, int lgHp, int32_t H, int32_t F) {
        const int lane = threadIdx.x & 63;
        L = 1 << lgL; hpg = 1 << lgHp; G = L << lgHp; eps = 64 >> (lgL + lgHp);
        sub = lane & (L - 1); hg = (lane >> lgL) & (hpg - 1); grp = lane >> (lgL + lgHp);
        fchunks = (F + 4 * L - 1) >> (lgL + 2);
        passes = ((H + hpg - 1) / hpg) * fchunks;
    }
    __device__ __forceinline__ int32_t head(int cp) const { return (cp / fchunks) * hpg + hg; }
    __device__ __forceinline__ int32_t col0(int cp) const { return (cp % fchunks) * 4 * L + 4 * sub; }
};

// four consecutive floats of a head's columns from f0 on; VEC: one 16-byte load (the caller saw to the alignment, F % 4 == 0 and f0 < F)
template <bool VEC>
__device__ __forceinline__ void gv2_load4(const float* __restrict__ head_row, int32_t f0, int32_t F, float (&x)[4]) {
    if constexpr (VEC) {
        const float4 t = *reinterpret_cast<const float4*>(head_row + f0);
        x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = f0 + k < F ? head_row[f0 + k] : 0.f;
    }
}
// sum over the lanes of one head (they are L consecutive lanes; every lane of the wavefront comes here together)
__device__ __forceinline__ double gv2_head_sum(double t, int L) {
    for (int off = 1; off < L; off <<= 1) t += __shfl_xor(t, off);
    return t;
}
// this lane's four exact products attn l, added pairwise
__device__ __forceinline__ double gv2_dot4(const float (&x)[4], const float (&r)[4], const float (&a)[4], float slope) {
    double t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = (double)a[k] * (double)gat_score(x[k], r[k], slope);
    return (t[0] + t[1]) + (t[2] + t[3]);
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
// the scores of head h (this lane's) of the edges lo + slot, lo + slot + stride, ... of one row; xr_h / attn_h: the row's and the
// attention vector's columns of that head.  Every lane of the wavefront makes every trip (the head sums shuffle).
template <bool VEC>
__device__ __forceinline__ void gv2_score_walk(const Gv2Lane& ln, const int32_t* __restrict__ col, const float* __restrict__ xl, const float* __restrict__ xr_h,
                                               const float* __restrict__ attn_h, int32_t N, int64_t HF, int32_t F, int32_t h, bool head_ok, float slope,
                                               int64_t lo, int64_t hi, int slot, int stride, float* p_h, float* s_h) {
    const int32_t f0 = 4 * ln.sub, fstep = 4 * ln.L;
    const bool active = head_ok && f0 < F;
    float r[4] = {0.f, 0.f, 0.f, 0.f}, a[4] = {0.f, 0.f, 0.f, 0.f};
    if (active) {
        gv2_load4<VEC>(xr_h, f0, F, r);
        gv2_load4<VEC>(attn_h, f0, F, a);
    }
    for (int64_t base = lo; base < hi; base += (int64_t)kGv2Unroll * stride) {
        float x[kGv2Unroll][4];
        const float* src[kGv2Unroll];
#pragma unroll
        for (int u = 0; u < kGv2Unroll; ++u) {
            const int64_t e = base + slot + (int64_t)u * stride;
            src[u] = xl + (int64_t)gat_node(e < hi ? col[e] : 0, N) * HF + (int64_t)h * F;
        }
#pragma unroll
        for (int u = 0; u < kGv2Unroll; ++u) {
            const int64_t e = base + slot + (int64_t)u * stride;
            if (active && e < hi) gv2_load4<VEC>(src[u], f0, F, x[u]);
            else x[u][0] = x[u][1] = x[u][2] = x[u][3] = 0.f;
        }
#pragma unroll
        for (int u = 0; u < kGv2Unroll; ++u) {
            const int64_t e = base + slot + (int64_t)u * stride;
            double t = gv2_dot4(x[u], r, a, slope);
            for (int32_t f = f0 + fstep; f < F; f += fstep) {   // F > 256 only: the head's further chunks (f < F is uniform over its lanes up to the last chunk, whose idle lanes add 0)
                float xc[4] = {0.f, 0.f, 0.f, 0.f}, rc[4] = {0.f, 0.f, 0.f, 0.f}, ac[4] = {0.f, 0.f, 0.f, 0.f};
                if (head_ok && e < hi) {
                    gv2_load4<VEC>(src[u], f, F, xc);
                    gv2_load4<VEC>(xr_h, f, F, rc);
                    gv2_load4<VEC>(attn_h, f, F, ac);
                }
                t += gv2_dot4(xc, rc, ac, slope);
            }
            t = gv2_head_sum(t, ln.L);
            if (ln.sub == 0 && head_ok && e < hi) {
                const float s = (float)t;
                p_h[e] = s;
                if (s_h) s_h[e] = s;
            }
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void gatv2_softmax_fwd_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int32_t N, int64_t E,
                                                                int32_t H, int32_t F, int lgL, int lgHp, const float* __restrict__ xl,
                                                                const float* __restrict__ xr, const float* __restrict__ attn, float slope, float* score,
                                                                float* p) {
    __shared__ int64_t sp[kEsRowsPerWg + 1];
    __shared__ float redf[4];
    __shared__ double redd[4];
    es_load_rows(rowptr, N, E, sp);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t row0 = (int64_t)blockIdx.x * kEsRowsPerWg, HF = (int64_t)H * F;
    const Gv2Lane ln(lgL, lgHp, H, F);
    for (int32_t hb = 0; hb < H; hb += ln.hpg) {   // the heads of one lane group at a time
        const int32_t h = hb + ln.hg;
        const bool head_ok = h < H;
        const int32_t hc = head_ok ? h : 0;
        float* const p_h = p + (int64_t)hc * E;
        float* const s_h = score ? score + (int64_t)hc * E : nullptr;
        const float* const attn_h = attn + (int64_t)hc * F;
        for (int q = 0; q < kEsRowsPerWg && row0 + q < N; ++q) {
            const int64_t lo = sp[q], hi = sp[q + 1];
            const bool whole = hi - lo > kGv2WaveRow;   // (workgroup-uniform)
            if (hi <= lo || (!whole && (q & 3) != wave)) continue;
            const float* const xr_h = xr + (row0 + q) * HF + (int64_t)hc * F;
            if (whole) gv2_score_walk<VEC>(ln, col, xl, xr_h, attn_h, N, HF, F, hc, head_ok, slope, lo, hi, wave * ln.eps + ln.grp, 4 * ln.eps, p_h, s_h);
            else gv2_score_walk<VEC>(ln, col, xl, xr_h, attn_h, N, HF, F, hc, head_ok, slope, lo, hi, ln.grp, ln.eps, p_h, s_h);
        }
    }
    __syncthreads();   // the scores of the workgroup's rows are in their slots of p: the softmax bins the rows over other lanes
    for (int32_t h = 0; h < H; ++h) es_fwd_rows(sp, p + (int64_t)h * E, p + (int64_t)h * E, 1.0f, redf, redd);
}

// ---- backward: one walk for both sides ------------------------------------------------------------------------------------------
// SRC = false (row side, rows of A): fixed = xr[i], gathered = xl[col e], g at e; d_attn's sums ride along.
// SRC = true (source side, rows of A^T): fixed = xl[j], gathered = xr[col_t eT], g at perm[eT].
template <bool VEC, bool SRC>
__device__ __forceinline__ void gv2_grad_walk(const int32_t* __restrict__ col, const int32_t* __restrict__ perm, const float* __restrict__ gathered,
                                              const float* g_h, int32_t N, int64_t E, int64_t HF, int32_t F, int32_t h, bool active, int32_t f0,
                                              const float (&r)[4], const float (&a)[4], const float (&as)[4], float slope, int64_t lo, int64_t hi,
                                              int slot, int stride, double (&acc)[4], double (&da)[4]) {
    for (int64_t base = lo + slot; base < hi; base += (int64_t)kGv2Unroll * stride) {
        float x[kGv2Unroll][4], gv[kGv2Unroll];
#pragma unroll
        for (int u = 0; u < kGv2Unroll; ++u) {
            const int64_t e = base + (int64_t)u * stride;
            const bool in = active && e < hi;
            if (in) {
                gv2_load4<VEC>(gathered + (int64_t)gat_node(col[e], N) * HF + (int64_t)h * F, f0, F, x[u]);
                gv[u] = g_h[SRC ? gat_edge(perm[e], E) : e];
            } else {
                x[u][0] = x[u][1] = x[u][2] = x[u][3] = 0.f;
                gv[u] = 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < kGv2Unroll; ++u) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float z = x[u][k] + r[k];
                acc[k] += (double)gat_mul_rn(gv[u], z > 0.f ? a[k] : as[k]);
                if constexpr (!SRC) da[k] += (double)gv[u] * (double)(z > 0.f ? z : gat_mul_rn(z, slope));
            }
        }
    }
}
// the lane groups of a wavefront hold the same columns off, 2 off, ... lanes apart: every lane ends with the wavefront's sum
__device__ __forceinline__ void gv2_group_sum(double (&acc)[4], int G) {
    for (int off = G; off < 64; off <<= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += __shfl_xor(acc[k], off);
    }
}

// the node-side gradient of the workgroup's rows for one column pass: every row in front of N is written, an empty one with 0
template <bool VEC, bool SRC>
__device__ __forceinline__ void gv2_grad_rows(const Gv2Lane& ln, const int64_t* sp, const int32_t* __restrict__ col, const int32_t* __restrict__ perm,
                                              const float* __restrict__ fixed, const float* __restrict__ gathered, const float* __restrict__ attn,
                                              const float* g, int32_t N, int64_t E, int32_t H, int32_t F, float slope, int cp, float* __restrict__ d_node,
                                              double (*sacc)[64][4], double (&da)[4]) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t row0 = (int64_t)blockIdx.x * kEsRowsPerWg, HF = (int64_t)H * F;
    const int32_t h = ln.head(cp), f0 = ln.col0(cp);
    const bool active = h < H && f0 < F;
    const int32_t hc = active ? h : 0;
    const float* const g_h = g + (int64_t)hc * E;
    float a[4] = {0.f, 0.f, 0.f, 0.f}, as[4];
    if (active) gv2_load4<VEC>(attn + (int64_t)hc * F, f0, F, a);
#pragma unroll
    for (int k = 0; k < 4; ++k) as[k] = gat_mul_rn(a[k], slope);
    for (int q = 0; q < kEsRowsPerWg && row0 + q < N; ++q) {
        const int64_t lo = sp[q], hi = sp[q + 1] > lo ? sp[q + 1] : lo;
        const bool whole = hi - lo > kGv2WaveRow;   // (workgroup-uniform)
        if (!whole && (q & 3) != wave) continue;
        float r[4] = {0.f, 0.f, 0.f, 0.f};
        if (active) gv2_load4<VEC>(fixed + (row0 + q) * HF + (int64_t)hc * F, f0, F, r);
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        float* const dst = d_node + (row0 + q) * HF + (int64_t)hc * F + f0;
        if (!whole) {
            gv2_grad_walk<VEC, SRC>(col, perm, gathered, g_h, N, E, HF, F, hc, active, f0, r, a, as, slope, lo, hi, ln.grp, ln.eps, acc, da);
            gv2_group_sum(acc, ln.G);
            if (ln.grp == 0 && active) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (f0 + k < F) dst[k] = (float)acc[k];
            }
        } else {   // the four wavefronts' sums meet in LDS, in wavefront order
            gv2_grad_walk<VEC, SRC>(col, perm, gathered, g_h, N, E, HF, F, hc, active, f0, r, a, as, slope, lo, hi, wave * ln.eps + ln.grp, 4 * ln.eps, acc, da);
            gv2_group_sum(acc, ln.G);
            if (ln.grp == 0) {
#pragma unroll
                for (int k = 0; k < 4; ++k) sacc[wave][lane][k] = acc[k];
            }
            __syncthreads();
            if (wave == 0 && ln.grp == 0 && active) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (f0 + k < F) dst[k] = (float)((sacc[0][lane][k] + sacc[1][lane][k]) + (sacc[2][lane][k] + sacc[3][lane][k]));
            }
            __syncthreads();
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void gatv2_softmax_bwd_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int32_t N, int64_t E,
                                                                int32_t H, int32_t F, int lgL, int lgHp, const float* __restrict__ xl,
                                                                const float* __restrict__ xr, const float* __restrict__ attn, float slope,
                                                                const float* __restrict__ p, const float* dp, float* g, float* __restrict__ d_xr,
                                                                double* __restrict__ partial) {
    __shared__ int64_t sp[kEsRowsPerWg + 1];
    __shared__ double redd[4];
    __shared__ double sacc[4][64][4];
    es_load_rows(rowptr, N, E, sp);
    double unused = 0.0;
    for (int32_t h = 0; h < H; ++h)
        es_bwd_rows<false>(sp, p + (int64_t)h * E, dp + (int64_t)h * E, nullptr, g + (int64_t)h * E, 1.0f, redd, unused);
    __syncthreads();   // g of the workgroup's rows is written: the gather walk deals the edges to other lanes
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const Gv2Lane ln(lgL, lgHp, H, F);
    for (int cp = 0; cp < ln.passes; ++cp) {
        double da[4] = {0.0, 0.0, 0.0, 0.0};
        gv2_grad_rows<VEC, false>(ln, sp, col, nullptr, xr, xl, attn, g, N, E, H, F, slope, cp, d_xr, sacc, da);
        // d_attn: this workgroup's fp64 partial of every column of the pass, partial[column][workgroup]
        gv2_group_sum(da, ln.G);
        if (ln.grp == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) sacc[wave][lane][k] = da[k];
        }
        __syncthreads();
        const int32_t h = ln.head(cp), f0 = ln.col0(cp);
        if (wave == 0 && ln.grp == 0 && h < H) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (f0 + k < F)
                    partial[((int64_t)h * F + f0 + k) * gridDim.x + blockIdx.x] = (sacc[0][lane][k] + sacc[1][lane][k]) + (sacc[2][lane][k] + sacc[3][lane][k]);
        }
        __syncthreads();
    }
}

// d_attn[c] = the workgroups' partials of column c, added in workgroup order per thread and then in the fixed tree: a workgroup per column
__global__ __launch_bounds__(256) void gatv2_dattn_kernel(const double* __restrict__ partial, int32_t n, float* __restrict__ d_attn) {
    __shared__ double redd[4];
    const double* const mine = partial + (int64_t)blockIdx.x * n;
    double acc = 0.0;
    for (int32_t k = threadIdx.x; k < n; k += 256) acc += mine[k];
    const double total = es_block_sum(acc, redd);
    if (threadIdx.x == 0) d_attn[blockIdx.x] = (float)total;
}

template <bool VEC>
__global__ __launch_bounds__(256) void gatv2_source_grad_kernel(const int32_t* __restrict__ rowptr_t, const int32_t* __restrict__ col_t,
                                                                const int32_t* __restrict__ perm, int32_t N, int64_t E, int32_t H, int32_t F, int lgL,
                                                                int lgHp, const float* __restrict__ xl, const float* __restrict__ xr,
                                                                const float* __restrict__ attn, float slope, const float* __restrict__ g,
                                                                float* __restrict__ d_xl) {
    __shared__ int64_t sp[kEsRowsPerWg + 1];
    __shared__ double sacc[4][64][4];
    es_load_rows(rowptr_t, N, E, sp);
    const Gv2Lane ln(lgL, lgHp, H, F);
    double unused[4] = {0.0, 0.0, 0.0, 0.0};
    for (int cp = 0; cp < ln.passes; ++cp) gv2_grad_rows<VEC, true>(ln, sp, col_t, perm, xl, xr, attn, g, N, E, H, F, slope, cp, d_xl, sacc, unused);
}

// launch geometry of the family: 256 threads, a workgroup per 32 rows (es_grid); the d_attn reduction one workgroup per column
inline bool gv2_sizes_ok(int32_t N, int64_t E, int32_t H, int32_t F) {
    return N >= 0 && E >= 0 && E <= 0x7fffffffLL && H >= 1 && F >= 1 && (int64_t)H * F <= 0x7fffffffLL;
}
inline size_t gv2_partial_bytes(int32_t N, int32_t H, int32_t F) {
    return ((size_t)es_grid(N) * (size_t)H * (size_t)F * sizeof(double) + 255) / 256 * 256;
}
inline bool gv2_vec(int32_t F, const void* a, const void* b, const void* c) {
    return F % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}

} // namespace

extern "C" size_t tcgnn_gatv2_workspace_bytes(int32_t num_nodes, int64_t num_edges, int32_t H, int32_t F) {
    return gv2_sizes_ok(num_nodes, num_edges, H, F) && num_nodes > 0 ? gv2_partial_bytes(num_nodes, H, F) : 0;
}

extern "C" int tcgnn_gatv2_softmax(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges, int32_t H, int32_t F,
                                   const float* d_xl, const float* d_xr, const float* d_attn, float negative_slope, float* d_score, float* d_p,
                                   void* stream) {
    if (!gv2_sizes_ok(num_nodes, num_edges, H, F)) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_gatv2_softmax: bad size (H >= 1, F >= 1, int32 CSR positions only)");
    if (num_nodes == 0 || num_edges == 0) return TCGNN_OK;
    if (!d_nodePointer || !d_edgeList || !d_xl || !d_xr || !d_attn || !d_p) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_gatv2_softmax: null array");
    const Gv2Geom geo = gv2_geom(H, F);
    const dim3 grid(es_grid(num_nodes)), block(256);
    if (gv2_vec(F, d_xl, d_xr, d_attn))
        hipLaunchKernelGGL(gatv2_softmax_fwd_kernel<true>, grid, block, 0, static_cast<hipStream_t>(stream), d_nodePointer, d_edgeList, num_nodes, num_edges, H, F,
                           geo.lgL, geo.lgHp, d_xl, d_xr, d_attn, negative_slope, d_score, d_p);
    else
        hipLaunchKernelGGL(gatv2_softmax_fwd_kernel<false>, grid, block, 0, static_cast<hipStream_t>(stream), d_nodePointer, d_edgeList, num_nodes, num_edges, H, F,
                           geo.lgL, geo.lgHp, d_xl, d_xr, d_attn, negative_slope, d_score, d_p);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}

extern "C" int tcgnn_gatv2_softmax_backward(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges, int32_t H,
                                            int32_t F, const float* d_xl, const float* d_xr, const float* d_attn, float negative_slope, const float* d_p,
                                            const float* d_dp, float* d_g, float* d_dxr, float* d_dattn, void* d_scratch, size_t scratch_bytes,
                                            void* stream_v) {
    if (!gv2_sizes_ok(num_nodes, num_edges, H, F))
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_gatv2_softmax_backward: bad size (H >= 1, F >= 1, int32 CSR positions only)");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const size_t HF = (size_t)H * (size_t)F;
    if (num_nodes == 0 || num_edges == 0) {
        if (num_nodes > 0 && d_dxr) HIP_TRY(hipMemsetAsync(d_dxr, 0, sizeof(float) * (size_t)num_nodes * HF, stream));
        if (d_dattn) HIP_TRY(hipMemsetAsync(d_dattn, 0, sizeof(float) * HF, stream));
        return TCGNN_OK;
    }
    if (!d_nodePointer || !d_edgeList || !d_xl || !d_xr || !d_attn || !d_p || !d_dp || !d_g || !d_dxr || !d_dattn)
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_gatv2_softmax_backward: null array");
    const size_t need = gv2_partial_bytes(num_nodes, H, F);
    if (!d_scratch || scratch_bytes < need || (reinterpret_cast<uintptr_t>(d_scratch) & 7))
        return fail(TCGNN_ERR_WORKSPACE, "tcgnn_gatv2_softmax_backward: scratch needs %zu bytes 8-aligned (tcgnn_gatv2_workspace_bytes), got %zu at %p", need,
                    scratch_bytes, d_scratch);
    double* const partial = static_cast<double*>(d_scratch);
    const Gv2Geom geo = gv2_geom(H, F);
    const dim3 grid(es_grid(num_nodes)), block(256);
    if (gv2_vec(F, d_xl, d_xr, d_attn))
        hipLaunchKernelGGL(gatv2_softmax_bwd_kernel<true>, grid, block, 0, stream, d_nodePointer, d_edgeList, num_nodes, num_edges, H, F, geo.lgL, geo.lgHp, d_xl,
                           d_xr, d_attn, negative_slope, d_p, d_dp, d_g, d_dxr, partial);
    else
        hipLaunchKernelGGL(gatv2_softmax_bwd_kernel<false>, grid, block, 0, stream, d_nodePointer, d_edgeList, num_nodes, num_edges, H, F, geo.lgL, geo.lgHp, d_xl,
                           d_xr, d_attn, negative_slope, d_p, d_dp, d_g, d_dxr, partial);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(gatv2_dattn_kernel, dim3((unsigned)HF), block, 0, stream, (const double*)partial, (int32_t)grid.x, d_dattn);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}

extern "C" int tcgnn_gatv2_source_grad(const int32_t* d_nodePointer_t, const int32_t* d_edgeList_t, const int32_t* d_perm, int32_t num_nodes,
                                       int64_t num_edges, int32_t H, int32_t F, const float* d_xl, const float* d_xr, const float* d_attn,
                                       float negative_slope, const float* d_g, float* d_dxl, void* stream_v) {
    if (!gv2_sizes_ok(num_nodes, num_edges, H, F)) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_gatv2_source_grad: bad size (H >= 1, F >= 1, int32 CSR positions only)");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_nodes == 0 || num_edges == 0) {
        if (num_nodes > 0 && d_dxl) HIP_TRY(hipMemsetAsync(d_dxl, 0, sizeof(float) * (size_t)num_nodes * (size_t)H * (size_t)F, stream));
        return TCGNN_OK;
    }
    if (!d_nodePointer_t || !d_edgeList_t || !d_perm || !d_xl || !d_xr || !d_attn || !d_g || !d_dxl)
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_gatv2_source_grad: null array");
    const Gv2Geom geo = gv2_geom(H, F);
    const dim3 grid(es_grid(num_nodes)), block(256);
    if (gv2_vec(F, d_xl, d_xr, d_attn))
        hipLaunchKernelGGL(gatv2_source_grad_kernel<true>, grid, block, 0, stream, d_nodePointer_t, d_edgeList_t, d_perm, num_nodes, num_edges, H, F, geo.lgL,
                           geo.lgHp, d_xl, d_xr, d_attn, negative_slope, d_g, d_dxl);
    else
        hipLaunchKernelGGL(gatv2_source_grad_kernel<false>, grid, block, 0, stream, d_nodePointer_t, d_edgeList_t, d_perm, num_nodes, num_edges, H, F, geo.lgL,
                           geo.lgHp, d_xl, d_xr, d_attn, negative_slope, d_g, d_dxl);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}
