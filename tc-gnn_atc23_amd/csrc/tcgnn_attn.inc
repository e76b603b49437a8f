// tcgnn_attn.inc - fused sparse attention (multi-head dot-product attention over a node's incoming edges: PyG's TransformerConv, DGL's
// DotGatConv): scores, their softmax and the weighted sum of the values in ONE walk with the softmax done online, the row-side backward
// (dq, delta) in one walk, the source-side backward (dk, dv) in one walk over A^T, and their C ABI.  Nothing of size E is written or read.
// Included by tcgnn_device.hip behind tcgnn_gatedgcn.inc; it uses tcgnn_segment_max.inc's scheduling (seg_chunk, seg_load_rows,
// kSegRowsPerWg, kSegWaveRow, kSegUnroll, the XCD row mapping), tcgnn_gatv2.inc's head-wise lane layout and helpers (gv2_geom, Gv2Lane,
// gv2_load4, gv2_head_sum), tcgnn_edge_softmax.inc's es_exp, tcgnn_gat.inc's gat_node clamp and tcgnn_gated.inc's gt_zero.
//
//   score     s[h,e] = fl32(fl32(sum_f (double)q[row e, hF+f] (double)k[col e, hF+f]) scale): exact products, an fp64 sum over the head's
//             lanes (four a lane pairwise, then a butterfly), rounded once, ONE fp32 product with scale
//   forward   L[i,h] = fl32(m + log(l)),  m = max_e s,  l = sum_e (double)es_exp(s - m);   Y[i, hF+f] = fl32((sum_e (double)p' v[col e]) / l)
//             with p' = es_exp(s - m) under the running maximum (below); a row without edges: Y = 0, L = 0
//   row side  delta[i,h] = fl32(sum_f (double)dY[i] (double)Y[i]);  p = es_exp(s - L[i,h]);  a = sum_f (double)dY[i] (double)v[col e] in fp64;
//             g = (double)p (a - (double)delta);  dq[i] = fl32((double)scale sum_e g k[col e])
//   source    over the rows of A^T, i = col_t[eT]: the same s (the products commute, the lanes and the butterfly are the forward's), p, a
//             and g from L[i,h] and delta[i,h];  dk[j] = fl32((double)scale sum g q[i]),  dv[j] = fl32(sum (double)p (double)dY[i])
//
// The walk is segment_max's as gated_kernel uses it: a lane GROUP owns one edge, kSegUnroll steps in flight (two gathered rows each), the
// column ids of the next steps read before the rows of these are used, kSegRowsPerWg rows a workgroup of four wavefronts, a row of up to
// kSegWaveRow edges on one wavefront and a longer one on all four.  Within a group the lanes are dealt out per HEAD as Gv2Lane does it
// (L lanes hold a head's F columns four at a time, a group is as many heads as fit); heads beyond a group and F > 256 are column
// passes, one per blockIdx.y.  A pass of an F > 256 head forms the whole dot from memory, chunk by chunk in one order, so that every
// pass and every direction sees the same score.  Every lane of a wavefront makes every trip of a row (the head sums shuffle); a lane
// without columns adds zeros.
// Online softmax (forward): a lane keeps the head's running maximum m, l in fp64 and its four fp64 sums.  The kSegUnroll scores of a
// trip are formed first; when their maximum exceeds m, l and the sums are multiplied by es_exp(m_old - m_new), once per trip at most -
// nowhere else inside the walk.  At the end of the row the groups' states merge by butterfly over lanes G, 2 G, ... apart (at_merge:
// each side rescaled to the common maximum, contraction off, so both lanes of a pair hold the same bits); the four wavefronts of a long
// row meet in LDS and are folded in wavefront order.  The backward walks have no state but fp64 sums, which meet the same way.
// Matrix instructions do not fit: a per-edge dot of length F <= 64 between one fixed and one gathered row is a matrix-vector product
// per edge with no operand shared between edges.
// VEC = false is the dword form (F % 4 != 0 or an operand off 16 bytes): the same lanes, the same order, the same bits.  No atomics, every
// order fixed.  Row pointers are clamped to [0, E] and a descending pair is an empty row; a column id is clamped to [0, N); perm is not
// read.  Every element of the outputs is written and nothing else.  A hub row stays on one workgroup.

namespace {

constexpr int kAtUnroll = kSegUnroll;

// a lane's place in the pass blockIdx.y: its head, its first column within the head, and whether it holds a head / columns at all
struct AtLane {
    Gv2Lane ln;
    int32_t h, f0;
    int64_t hoff;    // h F, the head's offset within a node row (head 0's for a lane without a head)
    bool head_ok, active;
    __device__ __forceinline__ AtLane(int lgL, int lgHp, int32_t H, int32_t F) : ln(lgL, lgHp, H, F) {
        const int cp = (int)blockIdx.y;
        h = ln.head(cp);
        f0 = ln.col0(cp);
        head_ok = h < H;
        active = head_ok && f0 < F;
        if (!head_ok) h = 0;
        hoff = (int64_t)h * F;
    }
    __device__ __forceinline__ bool first_chunk() const { return f0 < 4 * ln.L; }
};

struct AtState {
    float m;
    double l, acc[4];
};

__device__ __forceinline__ void at_zero4(float (&x)[4]) { x[0] = x[1] = x[2] = x[3] = 0.f; }

// four exact products, added pairwise (an FMA changes nothing: the products are exact)
__device__ __forceinline__ double at_dot4(const float (&a)[4], const float (&b)[4]) {
    double t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = (double)a[k] * (double)b[k];
    return (t[0] + t[1]) + (t[2] + t[3]);
}

// the dot of two head rows over the head's lanes; every lane of the wavefront comes here together.  One chunk (F <= 256): from the
// registers ra / rb (zeros where the lane holds nothing).  More: from memory a_h / b_h, chunk by chunk, whatever chunk the pass owns.
template <bool VEC>
__device__ __forceinline__ double at_head_dot(const AtLane& at, const float* a_h, const float* b_h, const float (&ra)[4], const float (&rb)[4], int32_t F,
                                              bool live) {
    double t;
    if (at.ln.fchunks == 1) {
        t = at_dot4(ra, rb);
    } else {
        t = 0.0;
        if (live) {
            for (int32_t f = 4 * at.ln.sub; f < F; f += 4 * at.ln.L) {
                float xa[4], xb[4];
                gv2_load4<VEC>(a_h, f, F, xa);
                gv2_load4<VEC>(b_h, f, F, xb);
                t += at_dot4(xa, xb);
            }
        }
    }
    return gv2_head_sum(t, at.ln.L);
}

__device__ __forceinline__ float at_score(double t, float scale) {
#pragma clang fp contract(off)
    return (float)t * scale;
}

// b's state into a's, each rescaled to the common maximum; a side that already stands at it is not touched (an empty side has m = -inf, l = 0)
__device__ __forceinline__ void at_merge(AtState& a, float om, double ol, const double (&oa)[4]) {
#pragma clang fp contract(off)
    const float mn = fmaxf(a.m, om);
    const double ra = a.m == mn ? 1.0 : (double)es_exp(a.m - mn), rb = om == mn ? 1.0 : (double)es_exp(om - mn);
    a.l = a.l * ra + ol * rb;
#pragma unroll
    for (int k = 0; k < 4; ++k) a.acc[k] = a.acc[k] * ra + oa[k] * rb;
    a.m = mn;
}
__device__ __forceinline__ void at_merge_groups(AtState& st, int G) {
    for (int off = G; off < 64; off <<= 1) {
        const float om = __shfl_xor(st.m, off);
        const double ol = __shfl_xor(st.l, off);
        double oa[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) oa[k] = __shfl_xor(st.acc[k], off);
        at_merge(st, om, ol, oa);
    }
}
__device__ __forceinline__ void at_sum_groups(double (&acc)[4], int G) {
    for (int off = G; off < 64; off <<= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += __shfl_xor(acc[k], off);
    }
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
// the edges lo + slot, lo + slot + stride, ... of one row: qr = this lane's columns of q[i], q_h = q[i]'s head row
template <bool VEC>
__device__ __forceinline__ void at_fwd_walk(const AtLane& at, const int32_t* __restrict__ col, const float* q_h, const float* k, const float* v, int32_t N,
                                            int64_t HF, int32_t F, float scale, int64_t lo, int64_t hi, int slot, int stride, const float (&qr)[4],
                                            AtState& st) {
#pragma clang fp contract(off)
    const bool one = at.ln.fchunks == 1;
    int32_t c[kAtUnroll];
#pragma unroll
    for (int u = 0; u < kAtUnroll; ++u) {
        const int64_t e = lo + slot + (int64_t)u * stride;
        c[u] = e < hi ? col[e] : 0;
    }
    for (int64_t base = lo; base < hi; base += (int64_t)kAtUnroll * stride) {   // (wavefront-uniform: every lane makes every trip)
        float x[kAtUnroll][4], w[kAtUnroll][4];
        int64_t src[kAtUnroll];
#pragma unroll
        for (int u = 0; u < kAtUnroll; ++u) {
            const int64_t e = base + slot + (int64_t)u * stride;
            src[u] = (int64_t)gat_node(c[u], N) * HF + at.hoff;
            at_zero4(x[u]);
            at_zero4(w[u]);
            if (at.active && e < hi) {
                if (one) gv2_load4<VEC>(k + src[u], at.f0, F, x[u]);
                gv2_load4<VEC>(v + src[u], at.f0, F, w[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < kAtUnroll; ++u) {   // the next steps' column ids, before these steps' rows are waited for
            const int64_t e = base + slot + (int64_t)(kAtUnroll + u) * stride;
            c[u] = e < hi ? col[e] : 0;
        }
        float s[kAtUnroll], mn = st.m;
#pragma unroll
        for (int u = 0; u < kAtUnroll; ++u) {
            const bool in = base + slot + (int64_t)u * stride < hi;
            const double t = at_head_dot<VEC>(at, q_h, k + src[u], qr, x[u], F, in && at.head_ok);
            s[u] = in ? at_score(t, scale) : -INFINITY;
            mn = fmaxf(mn, s[u]);
        }
        if (mn > st.m) {   // the maximum rose: the one place the running state is rescaled
            const double r = (double)es_exp(st.m - mn);
            st.l *= r;
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4) st.acc[k4] *= r;
            st.m = mn;
        }
#pragma unroll
        for (int u = 0; u < kAtUnroll; ++u) {
            if (base + slot + (int64_t)u * stride < hi) {
                const double p = (double)es_exp(s[u] - st.m);
                st.l += p;
#pragma unroll
                for (int k4 = 0; k4 < 4; ++k4) st.acc[k4] = __builtin_fma(p, (double)w[u][k4], st.acc[k4]);
            }
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int32_t N, int64_t E, int32_t H,
                                                       int32_t F, int lgL, int lgHp, int xcd_map, float scale, const float* q, const float* k, const float* v,
                                                       float* __restrict__ Y, float* __restrict__ Lse) {
    __shared__ int64_t sp[kSegRowsPerWg + 1];
    __shared__ float sm[4][64];
    __shared__ double sl[4][64];
    __shared__ double sacc[4][64][4];
    const int64_t row0 = seg_chunk(xcd_map) * kSegRowsPerWg;
    if (row0 >= N) return;   // (the grid is rounded up to a multiple of eight under the XCD mapping)
    seg_load_rows(rowptr, row0, N, E, sp);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const AtLane at(lgL, lgHp, H, F);
    const int64_t HF = (int64_t)H * F;
    // the row's results from its merged state; only the lanes of group 0 that hold columns come here
    auto store = [&](int64_t r, const AtState& st) {
        const bool any = st.l > 0.0;
        const double inv = any ? 1.0 / st.l : 0.0;
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4)
            if (at.f0 + k4 < F) Y[r * HF + at.hoff + at.f0 + k4] = (float)(st.acc[k4] * inv);
        if (Lse && at.ln.sub == 0 && at.first_chunk()) Lse[r * H + at.h] = any ? (float)((double)st.m + log(st.l)) : 0.f;
    };
    for (int pass = 0; pass < 2; ++pass) {   // 0: rows of up to kSegWaveRow edges, a wavefront each in turn; 1: longer rows, the whole workgroup
        for (int rq = pass ? 0 : wave; rq < kSegRowsPerWg && row0 + rq < N; rq += pass ? 1 : 4) {
            const int64_t lo = sp[rq], hi = sp[rq + 1] > lo ? sp[rq + 1] : lo;
            if ((hi - lo > kSegWaveRow) != (pass == 1)) continue;   // (workgroup-uniform in pass 1)
            const float* const q_h = q + (row0 + rq) * HF + at.hoff;
            float qr[4] = {0.f, 0.f, 0.f, 0.f};
            if (at.active) gv2_load4<VEC>(q_h, at.f0, F, qr);
            AtState st = {-INFINITY, 0.0, {0.0, 0.0, 0.0, 0.0}};
            if (!pass) {
                at_fwd_walk<VEC>(at, col, q_h, k, v, N, HF, F, scale, lo, hi, at.ln.grp, at.ln.eps, qr, st);
                at_merge_groups(st, at.ln.G);
                if (at.ln.grp == 0 && at.active) store(row0 + rq, st);
            } else {
                at_fwd_walk<VEC>(at, col, q_h, k, v, N, HF, F, scale, lo, hi, wave * at.ln.eps + at.ln.grp, 4 * at.ln.eps, qr, st);
                at_merge_groups(st, at.ln.G);
                if (at.ln.grp == 0) {
                    sm[wave][lane] = st.m;
                    sl[wave][lane] = st.l;
#pragma unroll
                    for (int k4 = 0; k4 < 4; ++k4) sacc[wave][lane][k4] = st.acc[k4];
                }
                __syncthreads();
                if (wave == 0 && at.ln.grp == 0 && at.active) {   // the four wavefronts' states, folded in wavefront order
#pragma unroll
                    for (int w = 1; w < 4; ++w) at_merge(st, sm[w][lane], sl[w][lane], sacc[w][lane]);
                    store(row0 + rq, st);
                }
                __syncthreads();
            }
        }
    }
}

// ---- backward: one walk for both sides ------------------------------------------------------------------------------------------
// SRC = false (row side, rows of A): fixed rows q[i] (fa) and dY[i] (fb), gathered k[j] (ga) and v[j] (gb); L and delta are the row's.
// SRC = true (source side, rows of A^T): fixed k[j] (fa) and v[j] (fb), gathered q[i] (ga) and dY[i] (gb) with L[i, h] and delta[i, h].
// acc0 += g ga (dq / dk before the scale); SRC: acc1 += p gb (dv).
template <bool VEC, bool SRC>
__device__ __forceinline__ void at_bwd_walk(const AtLane& at, const int32_t* __restrict__ col, const float* fa_h, const float* fb_h, const float* ga,
                                            const float* gb, const float* Lse, const float* delta, float L_row, float delta_row, int32_t N, int32_t H,
                                            int64_t HF, int32_t F, float scale, int64_t lo, int64_t hi, int slot, int stride, const float (&fa)[4],
                                            const float (&fb)[4], double (&acc0)[4], double (&acc1)[4]) {
#pragma clang fp contract(off)
    int32_t c[kAtUnroll];
#pragma unroll
    for (int u = 0; u < kAtUnroll; ++u) {
        const int64_t e = lo + slot + (int64_t)u * stride;
        c[u] = e < hi ? col[e] : 0;
    }
    for (int64_t base = lo; base < hi; base += (int64_t)kAtUnroll * stride) {   // (wavefront-uniform)
        float x[kAtUnroll][4], w[kAtUnroll][4], Le[kAtUnroll], de[kAtUnroll];
        int64_t src[kAtUnroll];
#pragma unroll
        for (int u = 0; u < kAtUnroll; ++u) {
            const int64_t e = base + slot + (int64_t)u * stride;
            const int64_t node = gat_node(c[u], N);
            src[u] = node * HF + at.hoff;
            at_zero4(x[u]);
            at_zero4(w[u]);
            Le[u] = L_row;
            de[u] = delta_row;
            if (at.active && e < hi) {
                gv2_load4<VEC>(ga + src[u], at.f0, F, x[u]);
                gv2_load4<VEC>(gb + src[u], at.f0, F, w[u]);
                if constexpr (SRC) {
                    Le[u] = Lse[node * H + at.h];
                    de[u] = delta[node * H + at.h];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kAtUnroll; ++u) {
            const int64_t e = base + slot + (int64_t)(kAtUnroll + u) * stride;
            c[u] = e < hi ? col[e] : 0;
        }
#pragma unroll
        for (int u = 0; u < kAtUnroll; ++u) {
            const bool in = base + slot + (int64_t)u * stride < hi, live = in && at.head_ok;
            // (q is the first factor of the score and dY of a on both sides: the products commute, the sums are the forward's)
            const double t = SRC ? at_head_dot<VEC>(at, ga + src[u], fa_h, x[u], fa, F, live) : at_head_dot<VEC>(at, fa_h, ga + src[u], fa, x[u], F, live);
            const double a = SRC ? at_head_dot<VEC>(at, gb + src[u], fb_h, w[u], fb, F, live) : at_head_dot<VEC>(at, fb_h, gb + src[u], fb, w[u], F, live);
            if (in && at.active) {
                const double p = (double)es_exp(at_score(t, scale) - Le[u]);
                const double g = p * (a - (double)de[u]);
#pragma unroll
                for (int k4 = 0; k4 < 4; ++k4) {
                    acc0[k4] = __builtin_fma(g, (double)x[u][k4], acc0[k4]);
                    if constexpr (SRC) acc1[k4] = __builtin_fma(p, (double)w[u][k4], acc1[k4]);
                }
            }
        }
    }
}

// SRC = false: rowptr / col of A, fa = q, fb = dY, ga = k, gb = v; delta is WRITTEN (from Y and dY) and o0 = dq - WALK = false writes
// delta alone.  SRC = true: rowptr / col of A^T, fa = k, fb = v, ga = q, gb = dY; L and delta are read per edge, o0 = dk, o1 = dv.
template <bool VEC, bool SRC, bool WALK>
__global__ __launch_bounds__(256) void attn_bwd_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int32_t N, int64_t E, int32_t H,
                                                       int32_t F, int lgL, int lgHp, int xcd_map, float scale, const float* fa, const float* fb,
                                                       const float* ga, const float* gb, const float* Y, const float* Lse, float* delta,
                                                       float* __restrict__ o0, float* __restrict__ o1) {
    __shared__ int64_t sp[kSegRowsPerWg + 1];
    __shared__ double sacc[2][4][64][4];
    const int64_t row0 = seg_chunk(xcd_map) * kSegRowsPerWg;
    if (row0 >= N) return;
    seg_load_rows(rowptr, row0, N, E, sp);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const AtLane at(lgL, lgHp, H, F);
    const int64_t HF = (int64_t)H * F;
    auto store = [&](int64_t r, const double (&a0)[4], const double (&a1)[4]) {
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4)
            if (at.f0 + k4 < F) {
                o0[r * HF + at.hoff + at.f0 + k4] = (float)((double)scale * a0[k4]);
                if constexpr (SRC) o1[r * HF + at.hoff + at.f0 + k4] = (float)a1[k4];
            }
    };
    for (int pass = 0; pass < 2; ++pass) {
        for (int rq = pass ? 0 : wave; rq < kSegRowsPerWg && row0 + rq < N; rq += pass ? 1 : 4) {
            const int64_t lo = sp[rq], hi = sp[rq + 1] > lo ? sp[rq + 1] : lo;
            if ((hi - lo > kSegWaveRow) != (pass == 1)) continue;   // (workgroup-uniform in pass 1)
            const int64_t r = row0 + rq;
            const float* const fa_h = fa + r * HF + at.hoff;
            const float* const fb_h = fb + r * HF + at.hoff;
            float ra[4] = {0.f, 0.f, 0.f, 0.f}, rb[4] = {0.f, 0.f, 0.f, 0.f};
            if (at.active) {
                if constexpr (WALK) gv2_load4<VEC>(fa_h, at.f0, F, ra);   // (without the walk q, k, v and L may be null)
                gv2_load4<VEC>(fb_h, at.f0, F, rb);
            }
            float L_row = 0.f, delta_row = 0.f;
            if constexpr (!SRC) {   // delta[i, h] from dY[i] (fb) and Y[i], at the top of the row
                float yr[4] = {0.f, 0.f, 0.f, 0.f};
                if (at.active) gv2_load4<VEC>(Y + r * HF + at.hoff, at.f0, F, yr);
                delta_row = (float)at_head_dot<VEC>(at, fb_h, Y + r * HF + at.hoff, rb, yr, F, at.head_ok);
                if constexpr (WALK) {
                    if (at.head_ok) L_row = Lse[r * H + at.h];
                }
                if (at.ln.grp == 0 && at.ln.sub == 0 && at.head_ok && at.first_chunk() && (!pass || wave == 0)) delta[r * H + at.h] = delta_row;
            }
            if constexpr (WALK) {
                double a0[4] = {0.0, 0.0, 0.0, 0.0}, a1[4] = {0.0, 0.0, 0.0, 0.0};
                if (!pass) {
                    at_bwd_walk<VEC, SRC>(at, col, fa_h, fb_h, ga, gb, Lse, delta, L_row, delta_row, N, H, HF, F, scale, lo, hi, at.ln.grp, at.ln.eps, ra, rb,
                                          a0, a1);
                    at_sum_groups(a0, at.ln.G);
                    if constexpr (SRC) at_sum_groups(a1, at.ln.G);
                    if (at.ln.grp == 0 && at.active) store(r, a0, a1);
                } else {
                    at_bwd_walk<VEC, SRC>(at, col, fa_h, fb_h, ga, gb, Lse, delta, L_row, delta_row, N, H, HF, F, scale, lo, hi,
                                          wave * at.ln.eps + at.ln.grp, 4 * at.ln.eps, ra, rb, a0, a1);
                    at_sum_groups(a0, at.ln.G);
                    if constexpr (SRC) at_sum_groups(a1, at.ln.G);
                    if (at.ln.grp == 0) {
#pragma unroll
                        for (int k4 = 0; k4 < 4; ++k4) {
                            sacc[0][wave][lane][k4] = a0[k4];
                            if constexpr (SRC) sacc[1][wave][lane][k4] = a1[k4];
                        }
                    }
                    __syncthreads();
                    if (wave == 0 && at.ln.grp == 0 && at.active) {   // the four wavefronts' sums, in wavefront order
#pragma unroll
                        for (int k4 = 0; k4 < 4; ++k4) {
                            a0[k4] = (sacc[0][0][lane][k4] + sacc[0][1][lane][k4]) + (sacc[0][2][lane][k4] + sacc[0][3][lane][k4]);
                            if constexpr (SRC) a1[k4] = (sacc[1][0][lane][k4] + sacc[1][1][lane][k4]) + (sacc[1][2][lane][k4] + sacc[1][3][lane][k4]);
                        }
                        store(r, a0, a1);
                    }
                    __syncthreads();
                }
            }
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
struct AtLaunch {
    Gv2Geom geo;
    dim3 grid;
    int xcd;
};
// the family's launch geometry: seg_grid's row chunks by the column passes of Gv2Lane (heads beyond a lane group, chunks of F > 256)
inline bool at_geometry(int32_t N, int32_t H, int32_t F, AtLaunch& g) {
    g.geo = gv2_geom(H, F);
    g.xcd = g_segmax_xcd_map ? 1 : 0;
    const int64_t L = 1 << g.geo.lgL, hpg = 1 << g.geo.lgHp;
    const int64_t passes = ((H + hpg - 1) / hpg) * ((F + 4 * L - 1) / (4 * L));
    if (passes > 65535) return false;
    g.grid = dim3(seg_grid(N, 1, g.xcd).x, (unsigned)passes);
    return true;
}
inline int at_sizes_ok(const char* call, int32_t N, int64_t E, int32_t H, int32_t F) {
    if (N < 0 || E < 0 || E > 0x7fffffffLL || H < 0 || F < 0 || (int64_t)H * F > 0x7fffffffLL)
        return fail(TCGNN_ERR_INVALID_ARG, "%s: bad size (int32 CSR positions only)", call);
    return TCGNN_OK;
}
inline bool at_vec(int32_t F, std::initializer_list<const void*> rows) {
    uintptr_t bits = 0;
    for (const void* p : rows) bits |= reinterpret_cast<uintptr_t>(p);
    return F % 4 == 0 && (bits & 15) == 0;
}
// an output without a meaning in this call (no edges, or F = 0): zero where it exists
inline int at_zero(float* a, int64_t n, hipStream_t stream) {
    if (!a || n <= 0) return TCGNN_OK;
    const unsigned blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(gated_zero_kernel, dim3(blocks), dim3(256), 0, stream, a, (float*)nullptr, n);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}

} // namespace

extern "C" int tcgnn_attn_forward(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges, const float* d_q,
                                  const float* d_k, const float* d_v, int32_t H, int32_t F, float scale, float* d_Y, float* d_L, void* stream_v) {
    if (const int rc = at_sizes_ok("tcgnn_attn_forward", num_nodes, num_edges, H, F)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_nodes == 0 || H == 0) return TCGNN_OK;
    if (F == 0) return at_zero(d_L, (int64_t)num_nodes * H, stream);
    if (!d_Y) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_attn_forward: null array");
    if (num_edges == 0) {   // every row is empty
        if (const int rc = at_zero(d_Y, (int64_t)num_nodes * H * F, stream)) return rc;
        return at_zero(d_L, (int64_t)num_nodes * H, stream);
    }
    if (!d_nodePointer || !d_edgeList || !d_q || !d_k || !d_v) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_attn_forward: null array");
    AtLaunch g;
    if (!at_geometry(num_nodes, H, F, g)) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_attn_forward: too many heads");
    const dim3 block(256);
    if (at_vec(F, {d_q, d_k, d_v}))
        hipLaunchKernelGGL(attn_fwd_kernel<true>, g.grid, block, 0, stream, d_nodePointer, d_edgeList, num_nodes, num_edges, H, F, g.geo.lgL, g.geo.lgHp, g.xcd,
                           scale, d_q, d_k, d_v, d_Y, d_L);
    else
        hipLaunchKernelGGL(attn_fwd_kernel<false>, g.grid, block, 0, stream, d_nodePointer, d_edgeList, num_nodes, num_edges, H, F, g.geo.lgL, g.geo.lgHp, g.xcd,
                           scale, d_q, d_k, d_v, d_Y, d_L);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}

extern "C" int tcgnn_attn_backward(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges, const float* d_q,
                                   const float* d_k, const float* d_v, const float* d_Y, const float* d_dY, const float* d_L, int32_t H, int32_t F,
                                   float scale, float* d_dq, float* d_delta, void* stream_v) {
    if (const int rc = at_sizes_ok("tcgnn_attn_backward", num_nodes, num_edges, H, F)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_nodes == 0 || H == 0) return TCGNN_OK;
    if (F == 0) return at_zero(d_delta, (int64_t)num_nodes * H, stream);
    if (!d_delta) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_attn_backward: null array");
    if (num_edges == 0) {   // Y is 0 everywhere: so are delta and dq
        if (const int rc = at_zero(d_dq, (int64_t)num_nodes * H * F, stream)) return rc;
        return at_zero(d_delta, (int64_t)num_nodes * H, stream);
    }
    if (!d_nodePointer || !d_edgeList || !d_Y || !d_dY || (d_dq && (!d_q || !d_k || !d_v || !d_L)))
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_attn_backward: null array");
    AtLaunch g;
    if (!at_geometry(num_nodes, H, F, g)) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_attn_backward: too many heads");
    const dim3 block(256);
    const bool vec = d_dq ? at_vec(F, {d_q, d_k, d_v, d_Y, d_dY}) : at_vec(F, {d_Y, d_dY});
#define TCGNN_AT_ROW(V, W)                                                                                                                              \
    hipLaunchKernelGGL((attn_bwd_kernel<V, false, W>), g.grid, block, 0, stream, d_nodePointer, d_edgeList, num_nodes, num_edges, H, F, g.geo.lgL,     \
                       g.geo.lgHp, g.xcd, scale, d_q, d_dY, d_k, d_v, d_Y, d_L, d_delta, d_dq, (float*)nullptr)
    if (d_dq) {
        if (vec) TCGNN_AT_ROW(true, true);
        else TCGNN_AT_ROW(false, true);
    } else {   // delta alone: the rows' tops without the walk
        if (vec) TCGNN_AT_ROW(true, false);
        else TCGNN_AT_ROW(false, false);
    }
#undef TCGNN_AT_ROW
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}

extern "C" int tcgnn_attn_source_grad(const int32_t* d_nodePointer_t, const int32_t* d_edgeList_t, const int32_t* d_perm, int32_t num_nodes,
                                      int64_t num_edges, const float* d_q, const float* d_k, const float* d_v, const float* d_dY, const float* d_L,
                                      const float* d_delta, int32_t H, int32_t F, float scale, float* d_dk, float* d_dv, void* stream_v) {
    (void)d_perm;   // (the values do not depend on A's positions)
    if (const int rc = at_sizes_ok("tcgnn_attn_source_grad", num_nodes, num_edges, H, F)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_nodes == 0 || H == 0 || F == 0) return TCGNN_OK;
    if (!d_dk || !d_dv) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_attn_source_grad: null array");
    if (num_edges == 0) {   // nobody reads anybody
        if (const int rc = at_zero(d_dk, (int64_t)num_nodes * H * F, stream)) return rc;
        return at_zero(d_dv, (int64_t)num_nodes * H * F, stream);
    }
    if (!d_nodePointer_t || !d_edgeList_t || !d_q || !d_k || !d_v || !d_dY || !d_L || !d_delta)
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_attn_source_grad: null array");
    AtLaunch g;
    if (!at_geometry(num_nodes, H, F, g)) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_attn_source_grad: too many heads");
    const dim3 block(256);
    if (at_vec(F, {d_q, d_k, d_v, d_dY}))
        hipLaunchKernelGGL((attn_bwd_kernel<true, true, true>), g.grid, block, 0, stream, d_nodePointer_t, d_edgeList_t, num_nodes, num_edges, H, F, g.geo.lgL,
                           g.geo.lgHp, g.xcd, scale, d_k, d_v, d_q, d_dY, (const float*)nullptr, d_L, const_cast<float*>(d_delta), d_dk, d_dv);
    else
        hipLaunchKernelGGL((attn_bwd_kernel<false, true, true>), g.grid, block, 0, stream, d_nodePointer_t, d_edgeList_t, num_nodes, num_edges, H, F, g.geo.lgL,
                           g.geo.lgHp, g.xcd, scale, d_k, d_v, d_q, d_dY, (const float*)nullptr, d_L, const_cast<float*>(d_delta), d_dk, d_dv);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}
