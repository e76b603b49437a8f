// tcgnn_segment_stats.inc - mean, standard deviation, maximum and minimum over a node's incoming edges in ONE walk (PNA's four
// aggregators), the backward of all four in one walk over A^T, and their C ABI.  Included by tcgnn_device.hip behind
// tcgnn_segment_max.inc, whose scheduling and helpers it uses (SegBest, seg_take / seg_wins, seg_load4, seg_chunk, seg_load_rows,
// seg_fwd_groups, seg_bwd_groups / seg_bwd_store, seg_lg_group, seg_grid, seg_rows_aligned; gat_node / gat_edge for the clamps).
//
//   forward   for a row i with k > 0 edges and x_e = X[col e, d]:
//               mean = sum x_e / k;   std = sqrt(max(var, 0) + eps), var = the population variance;
//               max / argmax as tcgnn_segment_max;   min / argmin its mirror image (numpy.argmin; a NaN beats every number)
//             a row without edges: +0 in all four value outputs (std included), -1 in both args.  Any output may be null.
//   backward  dZ[j,d] = sum over eT in row j of A^T of  a[i,d] + b[i,d] Z[j,d] + [argmax[i,d] == e] dmax[i,d] + [argmin[i,d] == e] dmin[i,d]
//             with i = col_t[eT], e = perm[eT]; the caller folds the mean / std gradients into a and b per destination.
//
// Moments (DESIGN.md 4.14).  Every lane of a row loads the row's FIRST neighbour s = X[col[rowptr[i]], d] before the walk and sums
// t = x - s and t^2 in fp64: mean = s + S1 / k, var = S2 / k - (S1 / k)^2, rounded to fp32 once.  Without the shift the
// subtraction of two squares of the row's magnitude loses what an fp32 result needs on inputs such as 1000 +- 1e-3.
// Every lane, lane group and wavefront of a row uses the same s, so their partial sums add.
// Orders are fixed - a lane's edges ascending, the butterfly over the lane groups, the wavefronts of a long row from LDS in their
// order - and there are no atomics: two calls give the same bits.  The forward has three forms per VEC (moments / extrema / both);
// an absent output inside a form is a null check at the store.  Nothing outside [0, N D) of an output is written and every element
// of a given output is.

namespace {

enum : int { kStatsMoments = 1, kStatsExtrema = 2 };
constexpr int kStatsUnroll = kSegUnroll;   // steps in flight: segment_max's (DESIGN.md 4.14 has what two cost)
constexpr int kStatsUnrollFour = 2;        // ... of the backward that gathers four rows an edge: 64 registers of loads in flight otherwise

struct SegMoments {
    double s1[4], s2[4];   // sums of x - shift and of its square
};

// the mirror image of seg_wins / seg_take: the smaller value, then the smaller position; a NaN still beats every number
__device__ __forceinline__ bool seg_wins_min(uint32_t b1, int32_t p1, uint32_t b2, int32_t p2) {
    const float v1 = __uint_as_float(b1), v2 = __uint_as_float(b2);
    const bool num = v1 < v2 || (v1 == v2 && p1 < p2);
    const bool nan = seg_nan(b1) && (!seg_nan(b2) || p1 < p2);
    return p2 < 0 || (p1 >= 0 && (num || nan));
}
__device__ __forceinline__ void seg_take_min(uint32_t& bv, int32_t& bp, uint32_t x, int32_t e) {
    const bool better = bp < 0 || __uint_as_float(x) < __uint_as_float(bv) || (seg_nan(x) && !seg_nan(bv));
    bv = better ? x : bv;
    bp = better ? e : bp;
}
__device__ __forceinline__ void seg_min_groups(SegBest& b, int G) {
    for (int off = G; off < 64; off <<= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t ov = __shfl_xor(b.v[k], off);
            const int32_t op = __shfl_xor(b.p[k], off);
            const bool keep = seg_wins_min(b.v[k], b.p[k], ov, op);
            b.v[k] = keep ? b.v[k] : ov;
            b.p[k] = keep ? b.p[k] : op;
        }
    }
}
__device__ __forceinline__ void seg_moment_groups(SegMoments& m, int G) {
    for (int off = G; off < 64; off <<= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            m.s1[k] += __shfl_xor(m.s1[k], off);
            m.s2[k] += __shfl_xor(m.s2[k], off);
        }
    }
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
// segment_max's walk (this lane's edges lo + slot, lo + slot + stride, ...; kStatsUnroll steps in flight, the next column ids read
// early) with every aggregator fed from the one loaded row
template <bool VEC, int WHAT>
__device__ __forceinline__ void seg_stats_walk(const uint32_t* __restrict__ X, const int32_t* __restrict__ col, int32_t N, int32_t D, int64_t lo,
                                               int64_t hi, int slot, int stride, int32_t d0, const float (&shift)[4], SegMoments& m, SegBest& mx,
                                               SegBest& mn) {
    int64_t e = lo + slot;
    int32_t c[kStatsUnroll];
#pragma unroll
    for (int u = 0; u < kStatsUnroll; ++u) {
        const int64_t eu = e + (int64_t)u * stride;
        c[u] = eu < hi ? col[eu] : 0;
    }
    while (e < hi) {
        uint32_t x[kStatsUnroll][4];
#pragma unroll
        for (int u = 0; u < kStatsUnroll; ++u) {
            const int64_t eu = e + (int64_t)u * stride;
            if (eu < hi) seg_load4<VEC>(X + (int64_t)gat_node(c[u], N) * D, d0, D, x[u]);
            else x[u][0] = x[u][1] = x[u][2] = x[u][3] = 0u;
        }
        const int64_t en = e + (int64_t)kStatsUnroll * stride;
#pragma unroll
        for (int u = 0; u < kStatsUnroll; ++u) {
            const int64_t eu = en + (int64_t)u * stride;
            c[u] = eu < hi ? col[eu] : 0;
        }
#pragma unroll
        for (int u = 0; u < kStatsUnroll; ++u) {
            const int64_t eu = e + (int64_t)u * stride;
            if (eu < hi) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if constexpr ((WHAT & kStatsMoments) != 0) {
                        const double t = (double)__uint_as_float(x[u][k]) - (double)shift[k];
                        m.s1[k] += t;
                        m.s2[k] = fma(t, t, m.s2[k]);
                    }
                    if constexpr ((WHAT & kStatsExtrema) != 0) {
                        seg_take(mx.v[k], mx.p[k], x[u][k], (int32_t)eu);
                        seg_take_min(mn.v[k], mn.p[k], x[u][k], (int32_t)eu);
                    }
                }
            }
        }
        e = en;
    }
}

struct SegStatsOut {
    float *mean, *stdv;
    uint32_t *vmax, *vmin;
    int32_t *amax, *amin;
};

__device__ __forceinline__ void seg_stats_store_moments(const SegMoments& m, const float (&shift)[4], int64_t k, float eps, const SegStatsOut& o, int64_t r,
                                                        int32_t D, int32_t d0) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (d0 + q < D) {
            float mean = 0.f, sd = 0.f;   // a row without edges
            if (k > 0) {
                const double m1 = m.s1[q] / (double)k, var = m.s2[q] / (double)k - m1 * m1;
                mean = (float)((double)shift[q] + m1);
                sd = (float)sqrt((var < 0.0 ? 0.0 : var) + (double)eps);
            }
            if (o.mean) o.mean[r * D + d0 + q] = mean;
            if (o.stdv) o.stdv[r * D + d0 + q] = sd;
        }
}
__device__ __forceinline__ void seg_stats_store_best(const SegBest& b, uint32_t* __restrict__ Y, int32_t* __restrict__ arg, int64_t r, int32_t D, int32_t d0) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (d0 + k < D) {
            if (Y) Y[r * D + d0 + k] = b.v[k];
            if (arg) arg[r * D + d0 + k] = b.p[k];
        }
}

template <bool VEC, int WHAT>
__global__ __launch_bounds__(256) void segment_stats_fwd_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int32_t N, int64_t E,
                                                                const uint32_t* __restrict__ X, int32_t D, int lgG, int xcd_map, float eps, SegStatsOut o) {
    constexpr bool MOM = (WHAT & kStatsMoments) != 0, EXT = (WHAT & kStatsExtrema) != 0;
    __shared__ int64_t sp[kSegRowsPerWg + 1];
    __shared__ uint32_t sred[4][3][64][4];   // wavefronts 1 .. 3 of a long row: first the moments (s1, s2 as two words each), then the extrema (v, p of both)
    const int64_t row0 = seg_chunk(xcd_map) * kSegRowsPerWg;
    if (row0 >= N) return;
    seg_load_rows(rowptr, row0, N, E, sp);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int G = 1 << lgG, eps_step = 64 >> lgG, grp = lane >> lgG, sub = lane & (G - 1);
    const int32_t d0 = (int32_t)blockIdx.y * kSegColBlock + 4 * sub;
    const bool active = d0 < D;
    for (int q = wave; q < kSegRowsPerWg && row0 + q < N; q += 4) {   // rows of up to kSegWaveRow edges: a wavefront each, in turn
        const int64_t lo = sp[q], hi = sp[q + 1] > lo ? sp[q + 1] : lo;
        if (hi - lo > kSegWaveRow) continue;
        SegMoments m = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
        SegBest mx = {{0u, 0u, 0u, 0u}, {-1, -1, -1, -1}}, mn = mx;
        float shift[4] = {0.f, 0.f, 0.f, 0.f};
        if (MOM && active && hi > lo) {
            uint32_t s[4];
            seg_load4<VEC>(X + (int64_t)gat_node(col[lo], N) * D, d0, D, s);
#pragma unroll
            for (int k = 0; k < 4; ++k) shift[k] = __uint_as_float(s[k]);
        }
        seg_stats_walk<VEC, WHAT>(X, col, N, D, lo, active ? hi : lo, grp, eps_step, d0, shift, m, mx, mn);
        if constexpr (MOM) seg_moment_groups(m, G);
        if constexpr (EXT) {
            seg_fwd_groups(mx, G);
            seg_min_groups(mn, G);
        }
        if (grp == 0 && active) {
            if constexpr (MOM) seg_stats_store_moments(m, shift, hi - lo, eps, o, row0 + q, D, d0);
            if constexpr (EXT) {
                seg_stats_store_best(mx, o.vmax, o.amax, row0 + q, D, d0);
                seg_stats_store_best(mn, o.vmin, o.amin, row0 + q, D, d0);
            }
        }
    }
    for (int q = 0; q < kSegRowsPerWg && row0 + q < N; ++q) {         // longer rows: the whole workgroup (the trip test is workgroup-uniform)
        const int64_t lo = sp[q], hi = sp[q + 1];
        if (hi - lo <= kSegWaveRow) continue;
        SegMoments m = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
        SegBest mx = {{0u, 0u, 0u, 0u}, {-1, -1, -1, -1}}, mn = mx;
        float shift[4] = {0.f, 0.f, 0.f, 0.f};
        if (MOM && active) {
            uint32_t s[4];
            seg_load4<VEC>(X + (int64_t)gat_node(col[lo], N) * D, d0, D, s);
#pragma unroll
            for (int k = 0; k < 4; ++k) shift[k] = __uint_as_float(s[k]);
        }
        seg_stats_walk<VEC, WHAT>(X, col, N, D, lo, active ? hi : lo, wave * eps_step + grp, 4 * eps_step, d0, shift, m, mx, mn);
        if constexpr (MOM) {
            seg_moment_groups(m, G);
            if (grp == 0 && wave > 0) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    sred[0][wave - 1][sub][k] = (uint32_t)__double2loint(m.s1[k]);
                    sred[1][wave - 1][sub][k] = (uint32_t)__double2hiint(m.s1[k]);
                    sred[2][wave - 1][sub][k] = (uint32_t)__double2loint(m.s2[k]);
                    sred[3][wave - 1][sub][k] = (uint32_t)__double2hiint(m.s2[k]);
                }
            }
            __syncthreads();
            if (wave == 0 && grp == 0 && active) {
#pragma unroll
                for (int w = 0; w < 3; ++w)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        m.s1[k] += __hiloint2double((int)sred[1][w][sub][k], (int)sred[0][w][sub][k]);
                        m.s2[k] += __hiloint2double((int)sred[3][w][sub][k], (int)sred[2][w][sub][k]);
                    }
                seg_stats_store_moments(m, shift, hi - lo, eps, o, row0 + q, D, d0);
            }
            __syncthreads();
        }
        if constexpr (EXT) {
            seg_fwd_groups(mx, G);
            seg_min_groups(mn, G);
            if (grp == 0 && wave > 0) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    sred[0][wave - 1][sub][k] = mx.v[k];
                    sred[1][wave - 1][sub][k] = (uint32_t)mx.p[k];
                    sred[2][wave - 1][sub][k] = mn.v[k];
                    sred[3][wave - 1][sub][k] = (uint32_t)mn.p[k];
                }
            }
            __syncthreads();
            if (wave == 0 && grp == 0 && active) {
#pragma unroll
                for (int w = 0; w < 3; ++w)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const uint32_t xv = sred[0][w][sub][k], nv = sred[2][w][sub][k];
                        const int32_t xp = (int32_t)sred[1][w][sub][k], np = (int32_t)sred[3][w][sub][k];
                        const bool keepx = seg_wins(mx.v[k], mx.p[k], xv, xp), keepn = seg_wins_min(mn.v[k], mn.p[k], nv, np);
                        mx.v[k] = keepx ? mx.v[k] : xv;
                        mx.p[k] = keepx ? mx.p[k] : xp;
                        mn.v[k] = keepn ? mn.v[k] : nv;
                        mn.p[k] = keepn ? mn.p[k] : np;
                    }
                seg_stats_store_best(mx, o.vmax, o.amax, row0 + q, D, d0);
                seg_stats_store_best(mn, o.vmin, o.amin, row0 + q, D, d0);
            }
            __syncthreads();
        }
    }
}

// ---- backward: the same walk over A^T, four gathered rows per edge (a, b, argmax, argmin) ------------------------------------
// VEC: the rows of every given array among them are 16-byte aligned.  dmax / dmin are read only where the arg names this edge.
struct SegStatsGrad {
    const uint32_t *a, *b, *amax, *amin;   // (a, b: fp32 travelling as words)
    const float *dmax, *dmin, *Z;
};

template <bool VEC, int WHAT>
__device__ __forceinline__ void seg_stats_bwd_walk(const int32_t* __restrict__ col_t, const int32_t* __restrict__ perm, int32_t N, int64_t E,
                                                   const SegStatsGrad& g, int32_t D, int64_t lo, int64_t hi, int slot, int stride, int32_t d0,
                                                   const double (&z)[4], double (&acc)[4]) {
    constexpr bool MOM = (WHAT & kStatsMoments) != 0, EXT = (WHAT & kStatsExtrema) != 0;
    constexpr int U = MOM && EXT ? kStatsUnrollFour : kStatsUnroll;
    int64_t e = lo + slot;
    int32_t c[U], p[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t eu = e + (int64_t)u * stride;
        c[u] = eu < hi ? col_t[eu] : 0;
        p[u] = eu < hi ? perm[eu] : 0;
    }
    while (e < hi) {
        uint32_t va[U][4], vb[U][4], ax[U][4], an[U][4];
        int64_t at[U];
        uint32_t want[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t eu = e + (int64_t)u * stride;
            at[u] = (int64_t)gat_node(c[u], N) * D;
            want[u] = (uint32_t)gat_edge(p[u], E);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                va[u][k] = vb[u][k] = 0u;
                ax[u][k] = an[u][k] = 0xffffffffu;   // (-1: no position)
            }
            if (eu < hi) {
                if constexpr (MOM) {
                    if (g.a) seg_load4<VEC>(g.a + at[u], d0, D, va[u]);
                    if (g.b) seg_load4<VEC>(g.b + at[u], d0, D, vb[u]);
                }
                if constexpr (EXT) {
                    if (g.amax) seg_load4<VEC>(g.amax + at[u], d0, D, ax[u]);
                    if (g.amin) seg_load4<VEC>(g.amin + at[u], d0, D, an[u]);
                }
            }
        }
        const int64_t en = e + (int64_t)U * stride;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t eu = en + (int64_t)u * stride;
            c[u] = eu < hi ? col_t[eu] : 0;
            p[u] = eu < hi ? perm[eu] : 0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t eu = e + (int64_t)u * stride;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (eu < hi && d0 + k < D) {   // the terms of one edge in the contract's order: a, b Z, dmax, dmin
                    if constexpr (MOM) {
                        if (g.a) acc[k] += (double)__uint_as_float(va[u][k]);
                        if (g.b) acc[k] = fma((double)__uint_as_float(vb[u][k]), z[k], acc[k]);   // (the product is exact in fp64)
                    }
                    if constexpr (EXT) {
                        if (g.amax && ax[u][k] == want[u]) acc[k] += (double)g.dmax[at[u] + d0 + k];
                        if (g.amin && an[u][k] == want[u]) acc[k] += (double)g.dmin[at[u] + d0 + k];
                    }
                }
        }
        e = en;
    }
}

template <bool VEC, int WHAT>
__global__ __launch_bounds__(256) void segment_stats_bwd_kernel(const int32_t* __restrict__ rowptr_t, const int32_t* __restrict__ col_t,
                                                                const int32_t* __restrict__ perm, int32_t N, int64_t E, SegStatsGrad g, int32_t D, int lgG,
                                                                int xcd_map, float* __restrict__ dZ) {
    __shared__ int64_t sp[kSegRowsPerWg + 1];
    __shared__ double sacc[4][64][4];
    const int64_t row0 = seg_chunk(xcd_map) * kSegRowsPerWg;
    if (row0 >= N) return;
    seg_load_rows(rowptr_t, row0, N, E, sp);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int G = 1 << lgG, eps_step = 64 >> lgG, grp = lane >> lgG, sub = lane & (G - 1);
    const int32_t d0 = (int32_t)blockIdx.y * kSegColBlock + 4 * sub;
    const bool active = d0 < D;
    for (int q = wave; q < kSegRowsPerWg && row0 + q < N; q += 4) {
        const int64_t lo = sp[q], hi = sp[q + 1] > lo ? sp[q + 1] : lo;
        if (hi - lo > kSegWaveRow) continue;
        double acc[4] = {0.0, 0.0, 0.0, 0.0}, z[4] = {0.0, 0.0, 0.0, 0.0};
        if ((WHAT & kStatsMoments) != 0 && g.b && active && hi > lo) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (d0 + k < D) z[k] = (double)g.Z[(row0 + q) * D + d0 + k];
        }
        seg_stats_bwd_walk<VEC, WHAT>(col_t, perm, N, E, g, D, lo, active ? hi : lo, grp, eps_step, d0, z, acc);
        seg_bwd_groups(acc, G);
        if (grp == 0 && active) seg_bwd_store(acc, dZ, row0 + q, D, d0);
    }
    for (int q = 0; q < kSegRowsPerWg && row0 + q < N; ++q) {
        const int64_t lo = sp[q], hi = sp[q + 1];
        if (hi - lo <= kSegWaveRow) continue;
        double acc[4] = {0.0, 0.0, 0.0, 0.0}, z[4] = {0.0, 0.0, 0.0, 0.0};
        if ((WHAT & kStatsMoments) != 0 && g.b && active) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (d0 + k < D) z[k] = (double)g.Z[(row0 + q) * D + d0 + k];
        }
        seg_stats_bwd_walk<VEC, WHAT>(col_t, perm, N, E, g, D, lo, active ? hi : lo, wave * eps_step + grp, 4 * eps_step, d0, z, acc);
        seg_bwd_groups(acc, G);
        if (grp == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) sacc[wave][sub][k] = acc[k];
        }
        __syncthreads();
        if (wave == 0 && grp == 0 && active) {
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = (sacc[0][sub][k] + sacc[1][sub][k]) + (sacc[2][sub][k] + sacc[3][sub][k]);
            seg_bwd_store(acc, dZ, row0 + q, D, d0);
        }
        __syncthreads();
    }
}

template <bool VEC>
void launch_stats_fwd(int what, dim3 grid, hipStream_t stream, const int32_t* rowptr, const int32_t* col, int32_t N, int64_t E, const uint32_t* X, int32_t D,
                      int lg, int xcd, float eps, const SegStatsOut& o) {
    const dim3 block(256);
    if (what == kStatsMoments)
        hipLaunchKernelGGL((segment_stats_fwd_kernel<VEC, kStatsMoments>), grid, block, 0, stream, rowptr, col, N, E, X, D, lg, xcd, eps, o);
    else if (what == kStatsExtrema)
        hipLaunchKernelGGL((segment_stats_fwd_kernel<VEC, kStatsExtrema>), grid, block, 0, stream, rowptr, col, N, E, X, D, lg, xcd, eps, o);
    else
        hipLaunchKernelGGL((segment_stats_fwd_kernel<VEC, kStatsMoments | kStatsExtrema>), grid, block, 0, stream, rowptr, col, N, E, X, D, lg, xcd, eps, o);
}
template <bool VEC>
void launch_stats_bwd(int what, dim3 grid, hipStream_t stream, const int32_t* rowptr_t, const int32_t* col_t, const int32_t* perm, int32_t N, int64_t E,
                      const SegStatsGrad& g, int32_t D, int lg, int xcd, float* dZ) {
    const dim3 block(256);
    if (what == kStatsMoments)
        hipLaunchKernelGGL((segment_stats_bwd_kernel<VEC, kStatsMoments>), grid, block, 0, stream, rowptr_t, col_t, perm, N, E, g, D, lg, xcd, dZ);
    else if (what == kStatsExtrema)
        hipLaunchKernelGGL((segment_stats_bwd_kernel<VEC, kStatsExtrema>), grid, block, 0, stream, rowptr_t, col_t, perm, N, E, g, D, lg, xcd, dZ);
    else
        hipLaunchKernelGGL((segment_stats_bwd_kernel<VEC, kStatsMoments | kStatsExtrema>), grid, block, 0, stream, rowptr_t, col_t, perm, N, E, g, D, lg, xcd, dZ);
}

} // namespace

extern "C" int tcgnn_segment_stats(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges, const float* d_X, int32_t D,
                                   float eps, float* d_mean, float* d_std, float* d_max, int32_t* d_argmax, float* d_min, int32_t* d_argmin, void* stream_v) {
    if (num_nodes < 0 || num_edges < 0 || num_edges > 0x7fffffffLL || D < 0)
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_segment_stats: bad size (int32 CSR positions only)");
    if ((d_argmax && !d_max) || (d_argmin && !d_min)) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_segment_stats: an arg output without its value output");
    if (!d_mean && !d_std && !d_max && !d_min) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_segment_stats: no output");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_nodes == 0 || D == 0) return TCGNN_OK;
    const size_t elems = (size_t)num_nodes * (size_t)D;
    if (num_edges == 0) {   // every row is empty
        for (float* v : {d_mean, d_std, d_max, d_min})
            if (v) HIP_TRY(hipMemsetAsync(v, 0, sizeof(float) * elems, stream));
        for (int32_t* a : {d_argmax, d_argmin})
            if (a) HIP_TRY(hipMemsetAsync(a, 0xff, sizeof(int32_t) * elems, stream));
        return TCGNN_OK;
    }
    if (!d_nodePointer || !d_edgeList || !d_X) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_segment_stats: null array");
    const int lg = seg_lg_group(D), xcd = g_segmax_xcd_map ? 1 : 0;
    const dim3 grid = seg_grid(num_nodes, D, xcd);
    const int what = ((d_mean || d_std) ? kStatsMoments : 0) | ((d_max || d_min) ? kStatsExtrema : 0);
    const SegStatsOut o = {d_mean, d_std, reinterpret_cast<uint32_t*>(d_max), reinterpret_cast<uint32_t*>(d_min), d_argmax, d_argmin};
    const uint32_t* X = reinterpret_cast<const uint32_t*>(d_X);
    if (seg_rows_aligned(d_X, D))
        launch_stats_fwd<true>(what, grid, stream, d_nodePointer, d_edgeList, num_nodes, num_edges, X, D, lg, xcd, eps, o);
    else
        launch_stats_fwd<false>(what, grid, stream, d_nodePointer, d_edgeList, num_nodes, num_edges, X, D, lg, xcd, eps, o);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}

extern "C" int tcgnn_segment_stats_backward(const int32_t* d_nodePointer_t, const int32_t* d_edgeList_t, const int32_t* d_perm, int32_t num_nodes,
                                            int64_t num_edges, const float* d_Z, const float* d_a, const float* d_b, const int32_t* d_argmax,
                                            const float* d_dmax, const int32_t* d_argmin, const float* d_dmin, int32_t D, float* d_dZ, void* stream_v) {
    if (num_nodes < 0 || num_edges < 0 || num_edges > 0x7fffffffLL || D < 0)
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_segment_stats_backward: bad size (int32 CSR positions only)");
    if (!d_b != !d_Z || !d_argmax != !d_dmax || !d_argmin != !d_dmin)
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_segment_stats_backward: half of a group (b with Z, argmax with dmax, argmin with dmin)");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_nodes == 0 || D == 0) return TCGNN_OK;
    const size_t elems = (size_t)num_nodes * (size_t)D;
    const int what = ((d_a || d_b) ? kStatsMoments : 0) | ((d_argmax || d_argmin) ? kStatsExtrema : 0);
    if (num_edges == 0 || (what == 0 && d_dZ)) {   // no edge, or no term
        if (d_dZ) HIP_TRY(hipMemsetAsync(d_dZ, 0, sizeof(float) * elems, stream));
        return TCGNN_OK;
    }
    if (!d_nodePointer_t || !d_edgeList_t || !d_perm || !d_dZ) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_segment_stats_backward: null array");
    const int lg = seg_lg_group(D), xcd = g_segmax_xcd_map ? 1 : 0;
    const dim3 grid = seg_grid(num_nodes, D, xcd);
    const SegStatsGrad g = {reinterpret_cast<const uint32_t*>(d_a), reinterpret_cast<const uint32_t*>(d_b), reinterpret_cast<const uint32_t*>(d_argmax),
                            reinterpret_cast<const uint32_t*>(d_argmin), d_dmax, d_dmin, d_Z};
    const bool vec = seg_rows_aligned(d_a, D) && seg_rows_aligned(d_b, D) && seg_rows_aligned(d_argmax, D) && seg_rows_aligned(d_argmin, D);   // (a null one is aligned)
    if (vec)
        launch_stats_bwd<true>(what, grid, stream, d_nodePointer_t, d_edgeList_t, d_perm, num_nodes, num_edges, g, D, lg, xcd, d_dZ);
    else
        launch_stats_bwd<false>(what, grid, stream, d_nodePointer_t, d_edgeList_t, d_perm, num_nodes, num_edges, g, D, lg, xcd, d_dZ);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}
