// tcgnn_attn_edge.inc - fused sparse attention WITH EDGE FEATURES (PyG's TransformerConv(edge_dim=...): the projected edge vector joins the
// key in the score and the value in the message): forward, row-side backward (dq, delta, dee, pg) and source-side backward (dk, dv), and
// their C ABI.  Included by tcgnn_device.hip behind tcgnn_attn.inc, whose schedule, lane layout and helpers it uses unchanged (AtLane,
// AtState, at_head_dot, at_score, at_merge, at_merge_groups, at_sum_groups, at_geometry, at_sizes_ok, at_vec, at_zero; es_exp; gat_node,
// gat_edge).  ee is fp32 [E, H F] in the CSR order of A: ee[e] is the vector of the edge at CSR position e.
//
//   score     s[h,e] = fl32(fl32(t) scale),  t = dot(q[i], k[j]) + dot(q[i], ee[e]): two at_head_dot sums (exact products, the fp64 sum over
//             the head's lanes), the second added to the first in fp64.  ee = 0 adds +0.0: the bits of tcgnn_attn_forward's score
//   forward   tcgnn_attn_forward's online softmax (state, rescale and merge order) with the message (double)v[j] + (double)ee[e], added
//             per component before the FMA with p;   Y[i] = fl32((sum_e p' (v[j] + ee[e])) / l),  L[i,h] = fl32(m + log l)
//   row side  delta[i,h] = fl32(<dY[i], Y[i]>);  p = es_exp(s - L[i,h]);  a = dot(dY[i], v[j]) + dot(dY[i], ee[e]);  g = p (a - delta);
//             dq[i] = fl32((double)scale sum_e g ((double)k[j] + (double)ee[e]));
//             dee[e] = fl32(((double)scale g) (double)q[i] + p (double)dY[i]) - written by the row that owns e: contiguous along the row;
//             pg[e,h] = (fl32 p, fl32 g), [E, H, 2] - what the source side reads instead of forming scores again
//   source    over the rows of A^T, i = col_t[eT], e = perm[eT], (p, g) = pg[e,h]:  dk[j] = fl32((double)scale sum g q[i]),
//             dv[j] = fl32(sum p dY[i]) - a plain two-row weighted gather-sum with fp64 sums: no dot, no shuffle inside the walk
//
// The forward and the row side stream ee[e] beside their two gathered rows: the load is issued with its step's gathers (kAtUnroll steps in
// flight, three loads a step), and since a lane group owns one edge and its lanes are dealt out head by head, a group reads - and the
// row side writes - H F consecutive floats of ee / dee.  The source side would have to gather ee[perm eT] at random, form two head-wise
// fp64 butterflies per edge and gather L and delta; it reads 2 H words per edge instead (at most 2 / F of the dee traffic).  Its walk
// keeps kAeSrcUnroll = 8 steps in flight: a step costs 10 VGPRs (two 16-byte rows, p, g) and nothing but two dependent loads (perm,
// then pg) stands between the index and the FMAs, so the latency is hidden by depth, not by arithmetic.
// Column passes (heads beyond a lane group, chunks of F > 256) each write their own columns of dee; every pass forms the whole score, and
// pg[e,h] is written once, by the lane with sub == 0 of the head's first chunk.  VEC = false is the dword form (F % 4 != 0 or a row
// operand, ee / dee included, off 16 bytes): the same lanes, the same order, the same bits.  pg is read and written a word at a time
// and needs no alignment beyond a float's.  No atomics, every order fixed; row pointers are clamped to [0, E], a column id to [0, N), a
// perm entry outside [0, E) reads position 0.  Every element of every output is written and nothing else.  A hub row stays on one
// workgroup.

namespace {

constexpr int kAeSrcUnroll = 8;

template <bool VEC>
__device__ __forceinline__ void ae_store4(float* head_row, int32_t f0, int32_t F, const float (&x)[4]) {
    if constexpr (VEC) {
        *reinterpret_cast<float4*>(head_row + f0) = make_float4(x[0], x[1], x[2], x[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (f0 + k < F) head_row[f0 + k] = x[k];
    }
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
// at_fwd_walk with the edge's own vector: z = this lane's columns of ee[e]
template <bool VEC>
__device__ __forceinline__ void ae_fwd_walk(const AtLane& at, const int32_t* __restrict__ col, const float* q_h, const float* k, const float* v,
                                            const float* ee, int32_t N, int64_t HF, int32_t F, float scale, int64_t lo, int64_t hi, int slot, int stride,
                                            const float (&qr)[4], AtState& st) {
#pragma clang fp contract(off)
    const bool one = at.ln.fchunks == 1;
    int32_t c[kAtUnroll];
#pragma unroll
    for (int u = 0; u < kAtUnroll; ++u) {
        const int64_t e = lo + slot + (int64_t)u * stride;
        c[u] = e < hi ? col[e] : 0;
    }
    for (int64_t base = lo; base < hi; base += (int64_t)kAtUnroll * stride) {   // (wavefront-uniform: every lane makes every trip)
        float x[kAtUnroll][4], w[kAtUnroll][4], z[kAtUnroll][4];
        int64_t src[kAtUnroll], eoff[kAtUnroll];
#pragma unroll
        for (int u = 0; u < kAtUnroll; ++u) {
            const int64_t e = base + slot + (int64_t)u * stride;
            src[u] = (int64_t)gat_node(c[u], N) * HF + at.hoff;
            eoff[u] = (e < hi ? e : lo) * HF + at.hoff;
            at_zero4(x[u]);
            at_zero4(w[u]);
            at_zero4(z[u]);
            if (at.active && e < hi) {
                if (one) gv2_load4<VEC>(k + src[u], at.f0, F, x[u]);
                gv2_load4<VEC>(v + src[u], at.f0, F, w[u]);
                gv2_load4<VEC>(ee + eoff[u], at.f0, F, z[u]);
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
            const bool in = base + slot + (int64_t)u * stride < hi, live = in && at.head_ok;
            const double tk = at_head_dot<VEC>(at, q_h, k + src[u], qr, x[u], F, live);
            const double te = at_head_dot<VEC>(at, q_h, ee + eoff[u], qr, z[u], F, live);
            s[u] = in ? at_score(tk + te, scale) : -INFINITY;
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
                for (int k4 = 0; k4 < 4; ++k4) st.acc[k4] = __builtin_fma(p, (double)w[u][k4] + (double)z[u][k4], st.acc[k4]);
            }
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void attn_edge_fwd_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int32_t N, int64_t E,
                                                            int32_t H, int32_t F, int lgL, int lgHp, int xcd_map, float scale, const float* q, const float* k,
                                                            const float* v, const float* ee, float* __restrict__ Y, float* __restrict__ Lse) {
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
    auto store = [&](int64_t r, const AtState& st) {   // (as attn_fwd_kernel's)
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
                ae_fwd_walk<VEC>(at, col, q_h, k, v, ee, N, HF, F, scale, lo, hi, at.ln.grp, at.ln.eps, qr, st);
                at_merge_groups(st, at.ln.G);
                if (at.ln.grp == 0 && at.active) store(row0 + rq, st);
            } else {
                ae_fwd_walk<VEC>(at, col, q_h, k, v, ee, N, HF, F, scale, lo, hi, wave * at.ln.eps + at.ln.grp, 4 * at.ln.eps, qr, st);
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

// ---- row side ---------------------------------------------------------------------------------------------------------------
// fixed rows q[i] (qr) and dY[i] (gr), gathered k[j] (x) and v[j] (w), streamed ee[e] (z); acc += g (k + ee) where dq is wanted
template <bool VEC>
__device__ __forceinline__ void ae_bwd_walk(const AtLane& at, const int32_t* __restrict__ col, const float* q_h, const float* dY_h, const float* k,
                                            const float* v, const float* ee, float L_row, float delta_row, int32_t N, int32_t H, int64_t HF, int32_t F,
                                            float scale, int64_t lo, int64_t hi, int slot, int stride, const float (&qr)[4], const float (&gr)[4],
                                            bool want_dq, float* __restrict__ dee, float* __restrict__ pg, double (&acc)[4]) {
#pragma clang fp contract(off)
    const bool writes_pg = pg && at.head_ok && at.ln.sub == 0 && at.first_chunk();
    int32_t c[kAtUnroll];
#pragma unroll
    for (int u = 0; u < kAtUnroll; ++u) {
        const int64_t e = lo + slot + (int64_t)u * stride;
        c[u] = e < hi ? col[e] : 0;
    }
    for (int64_t base = lo; base < hi; base += (int64_t)kAtUnroll * stride) {   // (wavefront-uniform)
        float x[kAtUnroll][4], w[kAtUnroll][4], z[kAtUnroll][4];
        int64_t src[kAtUnroll], eoff[kAtUnroll];
#pragma unroll
        for (int u = 0; u < kAtUnroll; ++u) {
            const int64_t e = base + slot + (int64_t)u * stride;
            src[u] = (int64_t)gat_node(c[u], N) * HF + at.hoff;
            eoff[u] = (e < hi ? e : lo) * HF + at.hoff;
            at_zero4(x[u]);
            at_zero4(w[u]);
            at_zero4(z[u]);
            if (at.active && e < hi) {
                gv2_load4<VEC>(k + src[u], at.f0, F, x[u]);
                gv2_load4<VEC>(v + src[u], at.f0, F, w[u]);
                gv2_load4<VEC>(ee + eoff[u], at.f0, F, z[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < kAtUnroll; ++u) {
            const int64_t e = base + slot + (int64_t)(kAtUnroll + u) * stride;
            c[u] = e < hi ? col[e] : 0;
        }
#pragma unroll
        for (int u = 0; u < kAtUnroll; ++u) {
            const int64_t e = base + slot + (int64_t)u * stride;
            const bool in = e < hi, live = in && at.head_ok;
            const double tk = at_head_dot<VEC>(at, q_h, k + src[u], qr, x[u], F, live);
            const double te = at_head_dot<VEC>(at, q_h, ee + eoff[u], qr, z[u], F, live);
            const double av = at_head_dot<VEC>(at, dY_h, v + src[u], gr, w[u], F, live);
            const double ae = at_head_dot<VEC>(at, dY_h, ee + eoff[u], gr, z[u], F, live);
            if (live) {
                const double p = (double)es_exp(at_score(tk + te, scale) - L_row);
                const double g = p * ((av + ae) - (double)delta_row);
                if (writes_pg) {
                    pg[(e * H + at.h) * 2] = (float)p;
                    pg[(e * H + at.h) * 2 + 1] = (float)g;
                }
                if (at.active) {
                    if (want_dq) {
#pragma unroll
                        for (int k4 = 0; k4 < 4; ++k4) acc[k4] = __builtin_fma(g, (double)x[u][k4] + (double)z[u][k4], acc[k4]);
                    }
                    if (dee) {
                        const double sg = (double)scale * g;
                        float d[4];
#pragma unroll
                        for (int k4 = 0; k4 < 4; ++k4) d[k4] = (float)(sg * (double)qr[k4] + p * (double)gr[k4]);
                        ae_store4<VEC>(dee + eoff[u], at.f0, F, d);
                    }
                }
            }
        }
    }
}

// delta is always written; WALK = false (no dq, no dee, no pg wanted) writes delta alone and reads only Y and dY
template <bool VEC, bool WALK>
__global__ __launch_bounds__(256) void attn_edge_bwd_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int32_t N, int64_t E,
                                                            int32_t H, int32_t F, int lgL, int lgHp, int xcd_map, float scale, const float* q, const float* k,
                                                            const float* v, const float* ee, const float* Y, const float* dY, const float* Lse, float* dq,
                                                            float* delta, float* dee, float* pg) {
    __shared__ int64_t sp[kSegRowsPerWg + 1];
    __shared__ double sacc[4][64][4];
    const int64_t row0 = seg_chunk(xcd_map) * kSegRowsPerWg;
    if (row0 >= N) return;
    seg_load_rows(rowptr, row0, N, E, sp);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const AtLane at(lgL, lgHp, H, F);
    const int64_t HF = (int64_t)H * F;
    auto store = [&](int64_t r, const double (&a)[4]) {
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4)
            if (at.f0 + k4 < F) dq[r * HF + at.hoff + at.f0 + k4] = (float)((double)scale * a[k4]);
    };
    for (int pass = 0; pass < 2; ++pass) {
        for (int rq = pass ? 0 : wave; rq < kSegRowsPerWg && row0 + rq < N; rq += pass ? 1 : 4) {
            const int64_t lo = sp[rq], hi = sp[rq + 1] > lo ? sp[rq + 1] : lo;
            if ((hi - lo > kSegWaveRow) != (pass == 1)) continue;   // (workgroup-uniform in pass 1)
            const int64_t r = row0 + rq;
            const float* const q_h = q + r * HF + at.hoff;
            const float* const dY_h = dY + r * HF + at.hoff;
            float qr[4] = {0.f, 0.f, 0.f, 0.f}, gr[4] = {0.f, 0.f, 0.f, 0.f}, yr[4] = {0.f, 0.f, 0.f, 0.f};
            if (at.active) {
                if constexpr (WALK) gv2_load4<VEC>(q_h, at.f0, F, qr);   // (without the walk q, k, v, ee and L may be null)
                gv2_load4<VEC>(dY_h, at.f0, F, gr);
                gv2_load4<VEC>(Y + r * HF + at.hoff, at.f0, F, yr);
            }
            const float delta_row = (float)at_head_dot<VEC>(at, dY_h, Y + r * HF + at.hoff, gr, yr, F, at.head_ok);
            if (at.ln.grp == 0 && at.ln.sub == 0 && at.head_ok && at.first_chunk() && (!pass || wave == 0)) delta[r * H + at.h] = delta_row;
            if constexpr (WALK) {
                const float L_row = at.head_ok ? Lse[r * H + at.h] : 0.f;
                double a0[4] = {0.0, 0.0, 0.0, 0.0};
                const int slot = pass ? wave * at.ln.eps + at.ln.grp : at.ln.grp, stride = pass ? 4 * at.ln.eps : at.ln.eps;
                ae_bwd_walk<VEC>(at, col, q_h, dY_h, k, v, ee, L_row, delta_row, N, H, HF, F, scale, lo, hi, slot, stride, qr, gr, dq != nullptr, dee, pg, a0);
                if (!dq) continue;   // (kernel-uniform: the barriers below are met by every wavefront or by none)
                at_sum_groups(a0, at.ln.G);
                if (!pass) {
                    if (at.ln.grp == 0 && at.active) store(r, a0);
                } else {
                    if (at.ln.grp == 0) {
#pragma unroll
                        for (int k4 = 0; k4 < 4; ++k4) sacc[wave][lane][k4] = a0[k4];
                    }
                    __syncthreads();
                    if (wave == 0 && at.ln.grp == 0 && at.active) {   // the four wavefronts' sums, in wavefront order
#pragma unroll
                        for (int k4 = 0; k4 < 4; ++k4) a0[k4] = (sacc[0][lane][k4] + sacc[1][lane][k4]) + (sacc[2][lane][k4] + sacc[3][lane][k4]);
                        store(r, a0);
                    }
                    __syncthreads();
                }
            }
        }
    }
}

// ---- source side --------------------------------------------------------------------------------------------------------------
// the edges lo + slot, lo + slot + stride, ... of one row of A^T: a0 += g q[i], a1 += p dY[i] with (p, g) = pg[perm eT, h]
template <bool VEC>
__device__ __forceinline__ void ae_src_walk(const AtLane& at, const int32_t* __restrict__ col_t, const int32_t* __restrict__ perm, const float* q,
                                            const float* dY, const float* __restrict__ pg, int32_t N, int64_t E, int32_t H, int64_t HF, int32_t F, int64_t lo,
                                            int64_t hi, int slot, int stride, double (&a0)[4], double (&a1)[4]) {
    int32_t c[kAeSrcUnroll], pe[kAeSrcUnroll];
#pragma unroll
    for (int u = 0; u < kAeSrcUnroll; ++u) {
        const int64_t e = lo + slot + (int64_t)u * stride;
        c[u] = e < hi ? col_t[e] : 0;
        pe[u] = e < hi ? perm[e] : 0;
    }
    for (int64_t base = lo + slot; base < hi; base += (int64_t)kAeSrcUnroll * stride) {   // (no shuffle inside: a lane leaves when its edges end)
        float x[kAeSrcUnroll][4], w[kAeSrcUnroll][4], p[kAeSrcUnroll], g[kAeSrcUnroll];
#pragma unroll
        for (int u = 0; u < kAeSrcUnroll; ++u) {
            at_zero4(x[u]);
            at_zero4(w[u]);
            p[u] = g[u] = 0.f;
            if (base + (int64_t)u * stride < hi) {
                const int64_t src = (int64_t)gat_node(c[u], N) * HF + at.hoff, at_pg = (gat_edge(pe[u], E) * H + at.h) * 2;
                gv2_load4<VEC>(q + src, at.f0, F, x[u]);
                gv2_load4<VEC>(dY + src, at.f0, F, w[u]);
                p[u] = pg[at_pg];
                g[u] = pg[at_pg + 1];
            }
        }
#pragma unroll
        for (int u = 0; u < kAeSrcUnroll; ++u) {   // the next steps' indices, before these steps' rows are waited for
            const int64_t e = base + (int64_t)(kAeSrcUnroll + u) * stride;
            c[u] = e < hi ? col_t[e] : 0;
            pe[u] = e < hi ? perm[e] : 0;
        }
#pragma unroll
        for (int u = 0; u < kAeSrcUnroll; ++u) {
            if (base + (int64_t)u * stride < hi) {
#pragma unroll
                for (int k4 = 0; k4 < 4; ++k4) {
                    a0[k4] = __builtin_fma((double)g[u], (double)x[u][k4], a0[k4]);
                    a1[k4] = __builtin_fma((double)p[u], (double)w[u][k4], a1[k4]);
                }
            }
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void attn_edge_src_kernel(const int32_t* __restrict__ rowptr_t, const int32_t* __restrict__ col_t,
                                                            const int32_t* __restrict__ perm, int32_t N, int64_t E, int32_t H, int32_t F, int lgL, int lgHp,
                                                            int xcd_map, float scale, const float* q, const float* dY, const float* __restrict__ pg,
                                                            float* __restrict__ dk, float* __restrict__ dv) {
    __shared__ int64_t sp[kSegRowsPerWg + 1];
    __shared__ double sacc[2][4][64][4];
    const int64_t row0 = seg_chunk(xcd_map) * kSegRowsPerWg;
    if (row0 >= N) return;
    seg_load_rows(rowptr_t, row0, N, E, sp);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const AtLane at(lgL, lgHp, H, F);
    const int64_t HF = (int64_t)H * F;
    auto store = [&](int64_t r, const double (&a0)[4], const double (&a1)[4]) {
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4)
            if (at.f0 + k4 < F) {
                dk[r * HF + at.hoff + at.f0 + k4] = (float)((double)scale * a0[k4]);
                dv[r * HF + at.hoff + at.f0 + k4] = (float)a1[k4];
            }
    };
    for (int pass = 0; pass < 2; ++pass) {
        for (int rq = pass ? 0 : wave; rq < kSegRowsPerWg && row0 + rq < N; rq += pass ? 1 : 4) {
            const int64_t lo = sp[rq], hi = sp[rq + 1] > lo ? sp[rq + 1] : lo;
            if ((hi - lo > kSegWaveRow) != (pass == 1)) continue;   // (workgroup-uniform in pass 1)
            double a0[4] = {0.0, 0.0, 0.0, 0.0}, a1[4] = {0.0, 0.0, 0.0, 0.0};
            const int slot = pass ? wave * at.ln.eps + at.ln.grp : at.ln.grp, stride = pass ? 4 * at.ln.eps : at.ln.eps;
            if (at.active) ae_src_walk<VEC>(at, col_t, perm, q, dY, pg, N, E, H, HF, F, lo, hi, slot, stride, a0, a1);
            at_sum_groups(a0, at.ln.G);
            at_sum_groups(a1, at.ln.G);
            if (!pass) {
                if (at.ln.grp == 0 && at.active) store(row0 + rq, a0, a1);
            } else {
                if (at.ln.grp == 0) {
#pragma unroll
                    for (int k4 = 0; k4 < 4; ++k4) {
                        sacc[0][wave][lane][k4] = a0[k4];
                        sacc[1][wave][lane][k4] = a1[k4];
                    }
                }
                __syncthreads();
                if (wave == 0 && at.ln.grp == 0 && at.active) {   // the four wavefronts' sums, in wavefront order
#pragma unroll
                    for (int k4 = 0; k4 < 4; ++k4) {
                        a0[k4] = (sacc[0][0][lane][k4] + sacc[0][1][lane][k4]) + (sacc[0][2][lane][k4] + sacc[0][3][lane][k4]);
                        a1[k4] = (sacc[1][0][lane][k4] + sacc[1][1][lane][k4]) + (sacc[1][2][lane][k4] + sacc[1][3][lane][k4]);
                    }
                    store(row0 + rq, a0, a1);
                }
                __syncthreads();
            }
        }
    }
}

} // namespace

extern "C" int tcgnn_attn_edge_forward(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges, const float* d_q,
                                       const float* d_k, const float* d_v, const float* d_ee, int32_t H, int32_t F, float scale, float* d_Y, float* d_L,
                                       void* stream_v) {
    if (const int rc = at_sizes_ok("tcgnn_attn_edge_forward", num_nodes, num_edges, H, F)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_nodes == 0 || H == 0) return TCGNN_OK;
    if (F == 0) return at_zero(d_L, (int64_t)num_nodes * H, stream);
    if (!d_Y) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_attn_edge_forward: null array");
    if (num_edges == 0) {   // every row is empty
        if (const int rc = at_zero(d_Y, (int64_t)num_nodes * H * F, stream)) return rc;
        return at_zero(d_L, (int64_t)num_nodes * H, stream);
    }
    if (!d_nodePointer || !d_edgeList || !d_q || !d_k || !d_v || !d_ee) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_attn_edge_forward: null array");
    AtLaunch g;
    if (!at_geometry(num_nodes, H, F, g)) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_attn_edge_forward: too many heads");
    const dim3 block(256);
    if (at_vec(F, {d_q, d_k, d_v, d_ee}))
        hipLaunchKernelGGL(attn_edge_fwd_kernel<true>, g.grid, block, 0, stream, d_nodePointer, d_edgeList, num_nodes, num_edges, H, F, g.geo.lgL, g.geo.lgHp,
                           g.xcd, scale, d_q, d_k, d_v, d_ee, d_Y, d_L);
    else
        hipLaunchKernelGGL(attn_edge_fwd_kernel<false>, g.grid, block, 0, stream, d_nodePointer, d_edgeList, num_nodes, num_edges, H, F, g.geo.lgL, g.geo.lgHp,
                           g.xcd, scale, d_q, d_k, d_v, d_ee, d_Y, d_L);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}

extern "C" int tcgnn_attn_edge_backward(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges, const float* d_q,
                                        const float* d_k, const float* d_v, const float* d_ee, const float* d_Y, const float* d_dY, const float* d_L, int32_t H,
                                        int32_t F, float scale, float* d_dq, float* d_delta, float* d_dee, float* d_pg, void* stream_v) {
    if (const int rc = at_sizes_ok("tcgnn_attn_edge_backward", num_nodes, num_edges, H, F)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_nodes == 0 || H == 0) return TCGNN_OK;
    if (F == 0) return at_zero(d_delta, (int64_t)num_nodes * H, stream);
    if (!d_delta) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_attn_edge_backward: null array");
    if (num_edges == 0) {   // Y is 0 everywhere: so are delta and dq; dee and pg have no elements
        if (const int rc = at_zero(d_dq, (int64_t)num_nodes * H * F, stream)) return rc;
        return at_zero(d_delta, (int64_t)num_nodes * H, stream);
    }
    const bool walk = d_dq || d_dee || d_pg;
    if (!d_nodePointer || !d_edgeList || !d_Y || !d_dY || (walk && (!d_q || !d_k || !d_v || !d_ee || !d_L)))
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_attn_edge_backward: null array");
    AtLaunch g;
    if (!at_geometry(num_nodes, H, F, g)) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_attn_edge_backward: too many heads");
    const dim3 block(256);
    // (a null d_dee adds no bits to the alignment test)
    const bool vec = walk ? at_vec(F, {d_q, d_k, d_v, d_ee, d_Y, d_dY, d_dee}) : at_vec(F, {d_Y, d_dY});
#define TCGNN_AE_ROW(V, W)                                                                                                                              \
    hipLaunchKernelGGL((attn_edge_bwd_kernel<V, W>), g.grid, block, 0, stream, d_nodePointer, d_edgeList, num_nodes, num_edges, H, F, g.geo.lgL,       \
                       g.geo.lgHp, g.xcd, scale, d_q, d_k, d_v, d_ee, d_Y, d_dY, d_L, d_dq, d_delta, d_dee, d_pg)
    if (walk) {
        if (vec) TCGNN_AE_ROW(true, true);
        else TCGNN_AE_ROW(false, true);
    } else {   // delta alone: the rows' tops without the walk
        if (vec) TCGNN_AE_ROW(true, false);
        else TCGNN_AE_ROW(false, false);
    }
#undef TCGNN_AE_ROW
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}

extern "C" int tcgnn_attn_edge_source_grad(const int32_t* d_nodePointer_t, const int32_t* d_edgeList_t, const int32_t* d_perm, int32_t num_nodes,
                                           int64_t num_edges, const float* d_q, const float* d_dY, const float* d_pg, int32_t H, int32_t F, float scale,
                                           float* d_dk, float* d_dv, void* stream_v) {
    if (const int rc = at_sizes_ok("tcgnn_attn_edge_source_grad", num_nodes, num_edges, H, F)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_nodes == 0 || H == 0 || F == 0) return TCGNN_OK;
    if (!d_dk || !d_dv) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_attn_edge_source_grad: null array");
    if (num_edges == 0) {   // nobody reads anybody
        if (const int rc = at_zero(d_dk, (int64_t)num_nodes * H * F, stream)) return rc;
        return at_zero(d_dv, (int64_t)num_nodes * H * F, stream);
    }
    if (!d_nodePointer_t || !d_edgeList_t || !d_perm || !d_q || !d_dY || !d_pg)
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_attn_edge_source_grad: null array");
    AtLaunch g;
    if (!at_geometry(num_nodes, H, F, g)) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_attn_edge_source_grad: too many heads");
    const dim3 block(256);
    if (at_vec(F, {d_q, d_dY}))
        hipLaunchKernelGGL(attn_edge_src_kernel<true>, g.grid, block, 0, stream, d_nodePointer_t, d_edgeList_t, d_perm, num_nodes, num_edges, H, F, g.geo.lgL,
                           g.geo.lgHp, g.xcd, scale, d_q, d_dY, d_pg, d_dk, d_dv);
    else
        hipLaunchKernelGGL(attn_edge_src_kernel<false>, g.grid, block, 0, stream, d_nodePointer_t, d_edgeList_t, d_perm, num_nodes, num_edges, H, F, g.geo.lgL,
                           g.geo.lgHp, g.xcd, scale, d_q, d_dY, d_pg, d_dk, d_dv);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}
