// tcgnn_edge_project.inc - GINE's message with the edge projection fused into the walk: u (+) (A We + be) -> act -> sum, and its four
// gradients, on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32), and their C ABI.  Included by tcgnn_device.hip behind
// tcgnn_edge_message.inc; it uses tcgnn_segment_max.inc's scheduling (seg_chunk, seg_load_rows, seg_grid, seg_rows_aligned, the XCD row
// mapping, the long-row rule kSegWaveRow), ue_pass, and gat_node / gat_edge for the clamps.
//
//   p[e, d]  = be[d] + sum_k A[e, k] We[k, d]       fp32, the MFMA's order, the bias as row K of We' against a column of ones in A'
//   z[e, d]  = fl32(X[col e, d] + p[e, d]);  m = act(z);  pass = act is the identity or !(z <= 0)
//   forward      Y[i, d]   = fl32(sum over e in row i of (double)m[e, d])                                            (empty row: 0)
//   row side     dA[e, k]  = sum_d g[e, d] We[k, d],  g[e, d] = pass ? dY[row e, d] : 0                               fp32
//                dWe[k, d] = fl32(sum in fp64 over the workgroups' fp32 partials of sum_e A[e, k] g[e, d]);  dbe[d]: the same with A[e, K] = 1
//   source side  dX[j, d]  = fl32(sum over t in row j of A^T of (double)g[perm t, d]),  z = X[j, d] + p[perm t, d], dY's row = col_t[t]
//
// No [E, D] array exists: p and pass are recomputed from A [E, K] wherever they are needed.  No atomics, every order fixed.
//
// Tile (DESIGN.md 4.20).  The unit of work is 16 consecutive positions of one row on one wavefront: lane = (e = lane & 15, g = lane >> 4).
// Product 1, the TRANSPOSED projection P^T[d, e] = We'^T A'^T per 16-column tile: the matrix operand is We' (registers, loaded once per
// column pass), the other operand the tile's A rows.  Reduction index k = 16 j + 4 g + t sits in step 4 j + t of lane group g, so that a
// lane's operand words of four steps are ONE 16-byte load of A[e, 16 j + 4 g ..]: a wavefront load is the tile's contiguous 64 K bytes.
// In the result a lane holds four CONSECUTIVE columns d = 16 c + 4 g + r of ONE edge e: the X[col e] gather stays a 16-byte load a lane.
// Product 2 (row side), dA^T[k, e] = We g^T: the result layout of product 1 IS the second operand when step (c, r) reduces over
// d = 16 c + 4 g + r, g = 0..3; We sits in registers in that order.  A lane gets four consecutive k of one edge: a 16-byte store.
// Product 3 (row side), dWe'[k, d] = A'^T g needs e on the reduction axis - the other orientation of the 16 x 16 pass mask.  Four wave-wide
// ballots per column tile (one per r) hold the mask; lane (n, g) of step s picks bit 16 (n >> 2) + 4 s + g of ballot n & 3: edge 4 s + g,
// column 16 c + n.  The value is dY[i, 16 c + n] (one dword load a row) or zero, A' comes by dword loads of the tile (a second read, from
// cache).  The accumulators live in the MFMA result registers for the whole column pass: an fp32 sum over the wavefront's edges.
// Rows: a row of up to kSegWaveRow positions takes one wavefront, a longer one the workgroup's four (tiles w, w + 4, ..), whose fp64
// sums meet in LDS in wavefront order.  D goes in column passes of 64 (32 where K + 1 > 32) inside the family's 256-column blocks.
// The [., D] operands take 16-byte accesses when D % 4 == 0 and their bases are aligned, A / dA when K % 4 == 0 and theirs are, the
// dword form otherwise (run-time switches around loads and stores only): the same lanes, the same order, the same bits either way.

#include <type_traits>

namespace {

typedef float floatx4p __attribute__((ext_vector_type(4)));

constexpr int kUepMaxK = 63;     // K + 1 <= 64: at most 16 steps of four
constexpr int kUepMaxWg = 512;   // workgroups of the row-side backward = partials of dWe' (32 MB of scratch at K = 63, D = 256)
constexpr int kUepTiles = 2;     // tiles a wavefront has in flight
enum : int { kUepFwd = 0, kUepSrc = 1 };

// steps of a tile's projection: k = 16 j + 4 g + t is step 4 j + t, so K + 1 rows of We' take 4 (n / 16) + min(n % 16, 4) steps
inline int uep_steps(int32_t K) { const int n = K + 1; return 4 * (n / 16) + (n % 16 < 4 ? n % 16 : 4); }
// ... rounded up to a compiled count (5: K = 16, the common edge_dim)
inline int uep_ns(int32_t K) { const int s = uep_steps(K); return s <= 4 ? 4 : (s == 5 ? 5 : (s <= 8 ? 8 : (s <= 12 ? 12 : 16))); }
// 16-column tiles of a column pass: what D needs, at most 4, and 2 where K + 1 > 32 (registers: NS * CT for We', and on the row side
// as many again for each of We and dWe')
inline int uep_ct(int ns, int32_t D) {
    const int want = D <= 16 ? 1 : (D <= 32 ? 2 : 4), most = ns > 8 ? 2 : 4;
    return want < most ? want : most;
}

// four consecutive floats of a row from column d0 on, zero past D and for a lane without an edge
__device__ __forceinline__ void uep_load4(bool vec, const float* __restrict__ row, int32_t d0, int32_t D, bool live, float (&x)[4]) {
    x[0] = x[1] = x[2] = x[3] = 0.0f;
    if (!live || d0 >= D) return;
    if (vec) {
        const floatx4p t = *reinterpret_cast<const floatx4p*>(row + d0);
        x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (d0 + r < D) x[r] = row[d0 + r];
    }
}
__device__ __forceinline__ void uep_store4(bool vec, float* __restrict__ row, int32_t d0, int32_t D, const double (&a)[4]) {
    if (d0 >= D) return;
    if (vec) {
        floatx4p t;
        t.x = (float)a[0]; t.y = (float)a[1]; t.z = (float)a[2]; t.w = (float)a[3];
        *reinterpret_cast<floatx4p*>(row + d0) = t;
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (d0 + r < D) row[d0 + r] = (float)a[r];
    }
}

// the tile's A' operand of product 1: b[4 j + t] = A'[pos, 16 j + 4 g + t] - A's row, a one in column K, zero behind it; the row is
// read once per call, past the caches' retention.  avec: K % 4 == 0 and A 16-byte aligned (a quad is then wholly inside or outside)
template <int NS>
__device__ __forceinline__ void uep_load_a(const float* __restrict__ A, int64_t pos, bool live, int32_t K, bool avec, int g, float (&b)[NS]) {
    const float* const row = A + pos * K;
#pragma unroll
    for (int j = 0; j < (NS + 3) / 4; ++j) {
        const int k0 = 16 * j + 4 * g;
        float q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (live) {
            if (avec && k0 < K) {
                const floatx4p t = __builtin_nontemporal_load(reinterpret_cast<const floatx4p*>(row + k0));
                q[0] = t.x; q[1] = t.y; q[2] = t.z; q[3] = t.w;
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (k0 + t < K) q[t] = __builtin_nontemporal_load(row + k0 + t);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (k0 + t == K) q[t] = 1.0f;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (4 * j + t < NS) b[4 * j + t] = q[t];
    }
}

// We' as the matrix operand of product 1: w[s][c] = We'[16 (s / 4) + 4 g + s % 4, cb + 16 c + i], i = lane & 15; row K is be, rows
// behind it and columns from D on are zero (the padding exists in registers only)
template <int NS, int CT>
__device__ __forceinline__ void uep_load_w(const float* __restrict__ We, const float* __restrict__ be, int32_t K, int32_t D, int32_t cb, int lane,
                                           float (&w)[NS][CT]) {
    const int i = lane & 15, g = lane >> 4;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int k = 16 * (s >> 2) + 4 * g + (s & 3);
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int32_t d = cb + 16 * c + i;
            w[s][c] = d < D ? (k < K ? We[(int64_t)k * D + d] : (k == K ? be[d] : 0.0f)) : 0.0f;
        }
    }
}

// product 1 on every column tile of the pass.  The rule of this file, for all three products: NO TWO WAYS OF CONTROL FLOW MAY JOIN
// BETWEEN THE LAST MFMA THAT WRITES A RESULT REGISTER AND THE FIRST INSTRUCTION THAT READS IT - no `if` (a wavefront-uniform one
// included) around a chain, or around some of its steps or column tiles, whose result is read behind the `if`.  With such a join the
// compiler's wait states covered one way into it only, and the other way read a result register too early (seen on the source side at
// K = 63 with one live tile of two: word 3 of the tile).  A branch that skips a chain TOGETHER WITH every read of its result is fine:
// uep_walk's `break` on a dead tile leaves out the tile's projection and its accumulation alike, and what follows starts a new chain.
// So a dead COLUMN tile of the last pass multiplies zeros, and a lane without an edge is a select.  tests/test_gpu_edge_project.py
// holds the case that showed it (K = 63, rows whose last trip has one live tile of two, both sides) to exact equality.
template <int NS, int CT>
__device__ __forceinline__ void uep_project(const float (&w)[NS][CT], const float (&b)[NS], floatx4p (&p)[CT]) {
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        p[c] = floatx4p{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < NS; ++s) p[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[s][c], b[s], p[c], 0, 0, 0);
    }
}

// ---- forward and source side: one template -------------------------------------------------------------------------------------------
// tiles first, first + stride, .. of the positions [lo, hi) of one row, the column pass from cb on.
//   kUepFwd: gat = X, ids = col;            message act(X[col e] + p[e])
//   kUepSrc: gat = dY, ids = col_t, perm;   message pass(fix + p[perm t]) ? dY[col_t t] : 0, fix = this lane's words of X[j]
// (Under the identity the projection is formed all the same and its mask ignored: one code path.)
template <int NS, int CT, int MODE>
__device__ __forceinline__ void uep_walk(const int32_t* __restrict__ ids, const int32_t* __restrict__ perm, const float* __restrict__ gat,
                                         const float* __restrict__ A, int32_t N, int64_t E, int32_t K, int32_t D, bool relu, bool vec, bool avec,
                                         const float (&w)[NS][CT], const float (&fix)[CT][4], int32_t cb, int nct, int64_t lo, int64_t hi,
                                         int first, int stride, int lane, double (&acc)[CT][4]) {
    constexpr int U = kUepTiles;
    const int e = lane & 15, g = lane >> 4;
    const int64_t step = 16 * (int64_t)stride;
    int64_t t0 = lo + 16 * (int64_t)first;
    int32_t id[U], pm[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t pos = t0 + u * step + e;
        id[u] = pos < hi ? ids[pos] : 0;
        pm[u] = MODE == kUepSrc && pos < hi ? perm[pos] : 0;
    }
    while (t0 < hi) {
        float b[U][NS], x[U][CT][4];
#pragma unroll
        for (int u = 0; u < U; ++u) {   // the stream first: going forward its addresses need no id
            const int64_t pos = t0 + u * step + e;
            const bool live = pos < hi;
            uep_load_a<NS>(A, MODE == kUepSrc ? gat_edge(pm[u], E) : (live ? pos : 0), live, K, avec, g, b[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t pos = t0 + u * step + e;
            const float* const row = gat + (int64_t)gat_node(id[u], N) * D;
#pragma unroll
            for (int c = 0; c < CT; ++c) uep_load4(vec, row, cb + 16 * c + 4 * g, D, pos < hi && c < nct, x[u][c]);
        }
        const int64_t tn = t0 + U * step;
#pragma unroll
        for (int u = 0; u < U; ++u) {   // the next tiles' ids, before these tiles' rows are waited for
            const int64_t pos = tn + u * step + e;
            id[u] = pos < hi ? ids[pos] : 0;
            pm[u] = MODE == kUepSrc && pos < hi ? perm[pos] : 0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (t0 + u * step >= hi) break;   // (wavefront-uniform)
            const bool live = t0 + u * step + e < hi;
            floatx4p p[CT];
            uep_project<NS, CT>(w, b[u], p);
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float m;
                    if constexpr (MODE == kUepFwd) {
                        const float z = x[u][c][r] + p[c][r];
                        m = !relu || ue_pass(z) ? z : 0.0f;
                    } else {
                        m = !relu || ue_pass(fix[c][r] + p[c][r]) ? x[u][c][r] : 0.0f;
                    }
                    acc[c][r] += live ? (double)m : 0.0;   // (a select, not a branch: the result registers are read in line; a dead tile adds +0)
                }
        }
        t0 = tn;
    }
}

// the 16 edge lanes of a group, in a fixed order: every lane ends with the group's sums
template <int CT>
__device__ __forceinline__ void uep_fold(double (&acc)[CT][4]) {
#pragma unroll
    for (int off = 1; off < 16; off <<= 1)
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[c][r] += __shfl_xor(acc[c][r], off);
}

template <int NS, int CT, int MODE>
__global__ __launch_bounds__(256) void edge_project_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ ids,
                                                           const int32_t* __restrict__ perm, int32_t N, int64_t E, const float* __restrict__ X,
                                                           const float* __restrict__ dY, const float* __restrict__ A, const float* __restrict__ We,
                                                           const float* __restrict__ be, int32_t K, int32_t D, int relu_i, int vec_i, int avec_i,
                                                           int xcd_map, float* __restrict__ Y) {
    __shared__ int64_t sp[kSegRowsPerWg + 1];
    __shared__ double sacc[4][4][CT][4];
    const int64_t row0 = seg_chunk(xcd_map) * kSegRowsPerWg;
    if (row0 >= N) return;   // (the grid is rounded up to a multiple of eight under the XCD mapping)
    seg_load_rows(rowptr, row0, N, E, sp);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int e = lane & 15, g = lane >> 4;
    const bool relu = relu_i != 0, vec = vec_i != 0, avec = avec_i != 0;
    const float* const gat = MODE == kUepFwd ? X : dY;
    const int32_t blk0 = (int32_t)blockIdx.y * kSegColBlock, blk1 = D - blk0 < kSegColBlock ? D : blk0 + kSegColBlock;
    for (int32_t cb = blk0; cb < blk1; cb += 16 * CT) {
        const int left = (blk1 - cb + 15) / 16, nct = left < CT ? left : CT;
        float w[NS][CT];
        uep_load_w<NS, CT>(We, be, K, D, cb, lane, w);
        for (int q = wave; q < kSegRowsPerWg && row0 + q < N; q += 4) {   // rows of up to kSegWaveRow positions: a wavefront each, in turn
            const int64_t lo = sp[q], hi = sp[q + 1] > lo ? sp[q + 1] : lo;
            if (hi - lo > kSegWaveRow) continue;
            float fix[CT][4];
            double acc[CT][4];
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                uep_load4(vec, X + (row0 + q) * D, cb + 16 * c + 4 * g, D, MODE == kUepSrc && c < nct, fix[c]);
                acc[c][0] = acc[c][1] = acc[c][2] = acc[c][3] = 0.0;
            }
            uep_walk<NS, CT, MODE>(ids, perm, gat, A, N, E, K, D, relu, vec, avec, w, fix, cb, nct, lo, hi, 0, 1, lane, acc);
            uep_fold<CT>(acc);
            if (e == 0) {
#pragma unroll
                for (int c = 0; c < CT; ++c)
                    if (c < nct) uep_store4(vec, Y + (row0 + q) * D, cb + 16 * c + 4 * g, D, acc[c]);
            }
        }
        for (int q = 0; q < kSegRowsPerWg && row0 + q < N; ++q) {         // longer rows: the whole workgroup (the trip test is workgroup-uniform)
            const int64_t lo = sp[q], hi = sp[q + 1];
            if (hi - lo <= kSegWaveRow) continue;
            float fix[CT][4];
            double acc[CT][4];
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                uep_load4(vec, X + (row0 + q) * D, cb + 16 * c + 4 * g, D, MODE == kUepSrc && c < nct, fix[c]);
                acc[c][0] = acc[c][1] = acc[c][2] = acc[c][3] = 0.0;
            }
            uep_walk<NS, CT, MODE>(ids, perm, gat, A, N, E, K, D, relu, vec, avec, w, fix, cb, nct, lo, hi, wave, 4, lane, acc);
            uep_fold<CT>(acc);
            if (e == 0) {
#pragma unroll
                for (int c = 0; c < CT; ++c)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sacc[wave][g][c][r] = acc[c][r];
            }
            __syncthreads();
            if (wave == 0 && e == 0) {
#pragma unroll
                for (int c = 0; c < CT; ++c) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[c][r] = (sacc[0][g][c][r] + sacc[1][g][c][r]) + (sacc[2][g][c][r] + sacc[3][g][c][r]);
                    if (c < nct) uep_store4(vec, Y + (row0 + q) * D, cb + 16 * c + 4 * g, D, acc[c]);
                }
            }
            __syncthreads();
        }
    }
}

// ---- row side: dA, and the workgroup's partial of dWe' -------------------------------------------------------------------------------
// dWe' partials: [gridDim.x][K + 1][D] fp32, row K = dbe's
template <int NS, int CT>
struct UepBwdRegs {
    static constexpr int KT = (NS + 3) / 4;       // 16-row tiles of We' (K + 1 rows)
    static constexpr int KA = NS == 5 ? 1 : KT;   // ... of We (K rows: dA has no ones column; NS = 5 is K = 16)
    float w[NS][CT];          // product 1: We'
    float wb[KA][CT][4];      // product 2: We[16 kt + i, cb + 16 c + 4 g + r]
    floatx4p dw[KT][CT];      // product 3's accumulators: dWe'[16 kt + 4 g + r, cb + 16 c + n]
};

template <int NS, int CT>
__device__ __forceinline__ void uep_bwd_walk(const int32_t* __restrict__ col, const float* __restrict__ X, const float* __restrict__ A,
                                             const float* __restrict__ dyrow, int32_t N, int32_t K, int32_t D, bool relu, bool vec, bool avec, bool first_pass,
                                             UepBwdRegs<NS, CT>& R, int32_t cb, int nct, int64_t lo, int64_t hi, int first, int stride, int lane,
                                             float* __restrict__ dA) {
    constexpr int KT = UepBwdRegs<NS, CT>::KT, KA = UepBwdRegs<NS, CT>::KA;
    const int e = lane & 15, g = lane >> 4;
    float dyl[CT][4], dyt[CT];       // dY[i] in the result layout of product 1, and a dword per column tile for product 3
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        uep_load4(vec, dyrow, cb + 16 * c + 4 * g, D, c < nct, dyl[c]);
        dyt[c] = c < nct && cb + 16 * c + e < D ? dyrow[cb + 16 * c + e] : 0.0f;
    }
    for (int64_t t0 = lo + 16 * (int64_t)first; t0 < hi; t0 += 16 * (int64_t)stride) {
        const int64_t pos = t0 + e;
        const bool live = pos < hi;
        bool pass[CT][4];
        {
            float b[NS], x[CT][4];
            uep_load_a<NS>(A, live ? pos : 0, live, K, avec, g, b);
            const float* const row = X + (int64_t)gat_node(live ? col[pos] : 0, N) * D;
#pragma unroll
            for (int c = 0; c < CT; ++c) uep_load4(vec, row, cb + 16 * c + 4 * g, D, live && c < nct, x[c]);
            floatx4p p[CT];
            uep_project<NS, CT>(R.w, b, p);
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) pass[c][r] = live && (!relu || ue_pass(x[c][r] + p[c][r]));
        }
        // product 2: dA[pos, 16 kt + 4 g ..] - a later column pass adds to what the first stored (the same lane, in program order)
#pragma unroll
        for (int kt = 0; kt < KA; ++kt) {
            floatx4p a = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) a = __builtin_amdgcn_mfma_f32_16x16x4f32(R.wb[kt][c][r], pass[c][r] ? dyl[c][r] : 0.0f, a, 0, 0, 0);
            const int k0 = 16 * kt + 4 * g;
            float* const out = dA + pos * K + k0;
            if (live && k0 < K) {
                if (avec) {
                    floatx4p* const o4 = reinterpret_cast<floatx4p*>(out);
                    if (!first_pass) a += *o4;
                    __builtin_nontemporal_store(a, o4);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (k0 + r < K) {
                            const float v = first_pass ? a[r] : a[r] + out[r];
                            __builtin_nontemporal_store(v, out + r);
                        }
                }
            }
        }
        // product 3: A'^T (second read of the tile, k on the lanes) times the mask's other orientation
        float at[KT][4];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int64_t ps = t0 + 4 * s + g;
                const int k = 16 * kt + e;
                at[kt][s] = ps < hi ? (k < K ? A[ps * K + k] : (k == K ? 1.0f : 0.0f)) : 0.0f;
            }
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const uint64_t m0 = __ballot(pass[c][0]), m1 = __ballot(pass[c][1]), m2 = __ballot(pass[c][2]), m3 = __ballot(pass[c][3]);
            const uint64_t mine = (e & 2) ? ((e & 1) ? m3 : m2) : ((e & 1) ? m1 : m0);
            const uint32_t bits = (uint32_t)(mine >> (16 * (e >> 2) + g));   // bit 4 s: edge 4 s + g, column 16 c + e
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float bt = (bits >> (4 * s)) & 1u ? dyt[c] : 0.0f;
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) R.dw[kt][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(at[kt][s], bt, R.dw[kt][c], 0, 0, 0);
            }
        }
    }
}

template <int NS, int CT>
__global__ __launch_bounds__(256) void edge_project_bwd_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int32_t N, int64_t E,
                                                               const float* __restrict__ X, const float* __restrict__ dY, const float* __restrict__ A,
                                                               const float* __restrict__ We, const float* __restrict__ be, int32_t K, int32_t D,
                                                               int relu_i, int vec_i, int avec_i, int32_t chunks, float* __restrict__ dA,
                                                               float* __restrict__ partial) {
    constexpr int KT = UepBwdRegs<NS, CT>::KT, KA = UepBwdRegs<NS, CT>::KA;
    __shared__ int64_t sp[kSegRowsPerWg + 1];
    __shared__ float ssum[KT * CT * 4 * 64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int e = lane & 15, g = lane >> 4;
    const bool relu = relu_i != 0, vec = vec_i != 0, avec = avec_i != 0;
    UepBwdRegs<NS, CT> R;
    for (int32_t cb = 0; cb < D; cb += 16 * CT) {
        const int left = (D - cb + 15) / 16, nct = left < CT ? left : CT;
        uep_load_w<NS, CT>(We, be, K, D, cb, lane, R.w);
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                R.dw[kt][c] = floatx4p{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k = 16 * kt + e;
                    const int32_t d = cb + 16 * c + 4 * g + r;
                    if (kt < KA) R.wb[kt][c][r] = k < K && d < D ? We[(int64_t)k * D + d] : 0.0f;
                }
            }
        for (int32_t chunk = (int32_t)blockIdx.x; chunk < chunks; chunk += (int32_t)gridDim.x) {   // chunks w, w + W, .. in order
            const int64_t row0 = (int64_t)chunk * kSegRowsPerWg;
            __syncthreads();   // (the last chunk's row pointers are done with)
            seg_load_rows(rowptr, row0, N, E, sp);
            for (int q = wave; q < kSegRowsPerWg && row0 + q < N; q += 4) {
                const int64_t lo = sp[q], hi = sp[q + 1] > lo ? sp[q + 1] : lo;
                if (hi - lo > kSegWaveRow || hi == lo) continue;
                uep_bwd_walk<NS, CT>(col, X, A, dY + (row0 + q) * D, N, K, D, relu, vec, avec, cb == 0, R, cb, nct, lo, hi, 0, 1, lane, dA);
            }
            for (int q = 0; q < kSegRowsPerWg && row0 + q < N; ++q) {
                const int64_t lo = sp[q], hi = sp[q + 1];
                if (hi - lo <= kSegWaveRow) continue;
                uep_bwd_walk<NS, CT>(col, X, A, dY + (row0 + q) * D, N, K, D, relu, vec, avec, cb == 0, R, cb, nct, lo, hi, wave, 4, lane, dA);
            }
            if (cb == 0) {   // positions in front of the first row and behind the last (none in a canonical CSR): zero
                if (chunk == 0)
                    for (int64_t x = threadIdx.x; x < sp[0] * K; x += 256) dA[x] = 0.0f;
                if (chunk == chunks - 1)
                    for (int64_t x = sp[kSegRowsPerWg] * K + threadIdx.x; x < E * K; x += 256) dA[x] = 0.0f;
            }
        }
        // the four wavefronts' accumulators, added in wavefront order; the last one writes the workgroup's partial
        for (int wv = 0; wv < 4; ++wv) {
            __syncthreads();
            if (wave != wv) continue;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int c = 0; c < CT; ++c)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int at = ((kt * CT + c) * 4 + r) * 64 + lane;
                        float v = R.dw[kt][c][r];
                        if (wv > 0) v = ssum[at] + v;
                        if (wv < 3) {
                            ssum[at] = v;
                        } else {
                            const int k = 16 * kt + 4 * g + r;
                            const int32_t d = cb + 16 * c + e;
                            if (k <= K && d < D && c < nct) partial[((int64_t)blockIdx.x * (K + 1) + k) * D + d] = v;
                        }
                    }
        }
    }
}

// dWe' = the workgroups' partials of an element, added in fp64 in workgroup order and rounded once; row K goes to dbe
__global__ __launch_bounds__(256) void edge_project_reduce_kernel(const float* __restrict__ partial, int32_t W, int32_t K, int32_t D,
                                                                  float* __restrict__ dWe, float* __restrict__ dbe) {
    const int64_t n = (int64_t)(K + 1) * D, at = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= n) return;
    double s = 0.0;
    for (int32_t w = 0; w < W; ++w) s += (double)partial[w * n + at];
    if (at < (int64_t)K * D) dWe[at] = (float)s;
    else dbe[at - (int64_t)K * D] = (float)s;
}

// zeroes an output of a call that has nothing to walk (a kernel, so that the call stays capturable)
__global__ __launch_bounds__(256) void edge_project_zero_kernel(float* __restrict__ out, int64_t n) {
    for (int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x; at < n; at += (int64_t)gridDim.x * 256) out[at] = 0.0f;
}

// The family's launch geometry: 256 threads.  Forward and source side: a workgroup per kSegRowsPerWg rows and 256-column block
// (seg_grid) under the XCD row mapping; row side: wg = min(chunks, kUepMaxWg) workgroups, each over every column.  ns: the compiled
// step count, ct: the compiled column tiles of a pass.
struct UepGeom {
    dim3 grid, block;
    int ns, ct, xcd;
    int32_t chunks, wg;
};
inline UepGeom uep_geom(int32_t N, int32_t K, int32_t D) {
    const int xcd = g_segmax_xcd_map ? 1 : 0, ns = uep_ns(K);
    const int32_t chunks = (int32_t)(((int64_t)N + kSegRowsPerWg - 1) / kSegRowsPerWg);
    return UepGeom{seg_grid(N, D, xcd), dim3(256), ns, uep_ct(ns, D), xcd, chunks, chunks < kUepMaxWg ? chunks : kUepMaxWg};
}
inline size_t uep_partial_bytes(int32_t N, int32_t K, int32_t D) {
    return ((size_t)uep_geom(N, K, D).wg * (size_t)(K + 1) * (size_t)D * sizeof(float) + 255) / 256 * 256;
}
inline bool uep_a_vec(int32_t K, const void* a, const void* b) {
    return K % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
}
inline int uep_args_ok(const char* call, int32_t N, int64_t E, int32_t K, int32_t D, int32_t act) {
    if (N < 0 || E < 0 || E > 0x7fffffffLL || D < 0) return fail(TCGNN_ERR_INVALID_ARG, "%s: bad size (int32 CSR positions only)", call);
    if (K < 1 || K > kUepMaxK) return fail(TCGNN_ERR_INVALID_ARG, "%s: K = %d, 1 <= K <= %d", call, K, kUepMaxK);
    if (act != TCGNN_ACT_IDENTITY && act != TCGNN_ACT_RELU) return fail(TCGNN_ERR_INVALID_ARG, "%s: unknown act %d", call, act);
    return TCGNN_OK;
}
inline int uep_zero(float* out, size_t n, hipStream_t stream) {
    if (!n) return TCGNN_OK;
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(edge_project_zero_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, out, (int64_t)n);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}

// f(NS, CT) with the two as compile-time constants
template <class F>
inline void uep_dispatch(int ns, int ct, F&& f) {
    auto wide = [&](auto n) {   // K + 1 <= 32: 1, 2 or 4 column tiles
        if (ct == 1) f(n, std::integral_constant<int, 1>{});
        else if (ct == 2) f(n, std::integral_constant<int, 2>{});
        else f(n, std::integral_constant<int, 4>{});
    };
    auto narrow = [&](auto n) {
        if (ct == 1) f(n, std::integral_constant<int, 1>{});
        else f(n, std::integral_constant<int, 2>{});
    };
    switch (ns) {
        case 4: wide(std::integral_constant<int, 4>{}); break;
        case 5: wide(std::integral_constant<int, 5>{}); break;
        case 8: wide(std::integral_constant<int, 8>{}); break;
        case 12: narrow(std::integral_constant<int, 12>{}); break;
        default: narrow(std::integral_constant<int, 16>{}); break;
    }
}

// forward (MODE kUepFwd: ids = col, dY unused, out = Y) and source side (kUepSrc: the transposed CSR, out = dX)
template <int MODE>
inline int uep_launch_walk(const int32_t* rowptr, const int32_t* ids, const int32_t* perm, int32_t N, int64_t E, const float* X, const float* dY,
                           const float* A, const float* We, const float* be, int32_t K, int32_t D, int32_t act, float* out, hipStream_t stream) {
    const UepGeom geo = uep_geom(N, K, D);
    const int vec = seg_rows_aligned(X, D) && seg_rows_aligned(out, D) && (MODE == kUepFwd || seg_rows_aligned(dY, D));
    const int relu = act == TCGNN_ACT_RELU, avec = uep_a_vec(K, A, A);
    uep_dispatch(geo.ns, geo.ct, [&](auto n, auto c) {
        hipLaunchKernelGGL((edge_project_kernel<decltype(n)::value, decltype(c)::value, MODE>), geo.grid, geo.block, 0, stream, rowptr, ids, perm, N, E, X, dY,
                           A, We, be, K, D, relu, vec, avec, geo.xcd, out);
    });
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}

} // namespace

extern "C" size_t tcgnn_edge_project_workspace_bytes(int32_t num_nodes, int32_t K, int32_t D) {
    return num_nodes > 0 && K >= 1 && K <= kUepMaxK && D > 0 ? uep_partial_bytes(num_nodes, K, D) : 0;
}

extern "C" int tcgnn_edge_project_message(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges, const float* d_X,
                                          const float* d_A, const float* d_We, const float* d_be, int32_t K, int32_t D, int32_t act, float* d_Y,
                                          void* stream_v) {
    if (const int rc = uep_args_ok("tcgnn_edge_project_message", num_nodes, num_edges, K, D, act)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_nodes == 0 || D == 0) return TCGNN_OK;
    if (!d_Y) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_edge_project_message: null array");
    if (num_edges == 0) return uep_zero(d_Y, (size_t)num_nodes * (size_t)D, stream);   // every row is empty
    if (!d_nodePointer || !d_edgeList || !d_X || !d_A || !d_We || !d_be) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_edge_project_message: null array");
    return uep_launch_walk<kUepFwd>(d_nodePointer, d_edgeList, nullptr, num_nodes, num_edges, d_X, nullptr, d_A, d_We, d_be, K, D, act, d_Y, stream);
}

extern "C" int tcgnn_edge_project_source_grad(const int32_t* d_nodePointer_t, const int32_t* d_edgeList_t, const int32_t* d_perm, int32_t num_nodes,
                                              int64_t num_edges, const float* d_X, const float* d_A, const float* d_We, const float* d_be,
                                              const float* d_dY, int32_t K, int32_t D, int32_t act, float* d_dX, void* stream_v) {
    if (const int rc = uep_args_ok("tcgnn_edge_project_source_grad", num_nodes, num_edges, K, D, act)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_nodes == 0 || D == 0) return TCGNN_OK;
    if (!d_dX) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_edge_project_source_grad: null array");
    if (num_edges == 0) return uep_zero(d_dX, (size_t)num_nodes * (size_t)D, stream);   // nobody reads anybody
    if (!d_nodePointer_t || !d_edgeList_t || !d_perm || !d_X || !d_A || !d_We || !d_be || !d_dY)
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_edge_project_source_grad: null array");
    return uep_launch_walk<kUepSrc>(d_nodePointer_t, d_edgeList_t, d_perm, num_nodes, num_edges, d_X, d_dY, d_A, d_We, d_be, K, D, act, d_dX, stream);
}

extern "C" int tcgnn_edge_project_backward(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges, const float* d_X,
                                           const float* d_A, const float* d_We, const float* d_be, const float* d_dY, int32_t K, int32_t D, int32_t act,
                                           float* d_dA, float* d_dWe, float* d_dbe, void* d_scratch, size_t scratch_bytes, void* stream_v) {
    if (const int rc = uep_args_ok("tcgnn_edge_project_backward", num_nodes, num_edges, K, D, act)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const size_t ek = (size_t)num_edges * (size_t)K, kd = (size_t)K * (size_t)D;
    if ((ek && !d_dA) || (D && (!d_dWe || !d_dbe))) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_edge_project_backward: null array");
    if (num_nodes == 0 || num_edges == 0 || D == 0) {   // no message: every gradient that has elements is zero
        if (const int rc = uep_zero(d_dA, ek, stream)) return rc;
        if (const int rc = uep_zero(d_dWe, kd, stream)) return rc;
        return uep_zero(d_dbe, (size_t)D, stream);
    }
    if (!d_nodePointer || !d_edgeList || !d_X || !d_A || !d_We || !d_be || !d_dY) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_edge_project_backward: null array");
    const size_t need = uep_partial_bytes(num_nodes, K, D);
    if (!d_scratch || scratch_bytes < need || (reinterpret_cast<uintptr_t>(d_scratch) & 3))
        return fail(TCGNN_ERR_WORKSPACE, "tcgnn_edge_project_backward: scratch needs %zu bytes 4-aligned (tcgnn_edge_project_workspace_bytes), got %zu at %p",
                    need, scratch_bytes, d_scratch);
    const UepGeom geo = uep_geom(num_nodes, K, D);
    float* const partial = static_cast<float*>(d_scratch);
    const int vec = seg_rows_aligned(d_X, D) && seg_rows_aligned(d_dY, D);
    const int relu = act == TCGNN_ACT_RELU, avec = uep_a_vec(K, d_A, d_dA);
    uep_dispatch(geo.ns, geo.ct, [&](auto n, auto c) {
        hipLaunchKernelGGL((edge_project_bwd_kernel<decltype(n)::value, decltype(c)::value>), dim3((unsigned)geo.wg), geo.block, 0, stream, d_nodePointer,
                           d_edgeList, num_nodes, num_edges, d_X, d_dY, d_A, d_We, d_be, K, D, relu, vec, avec, geo.chunks, d_dA, partial);
    });
    HIP_TRY(hipGetLastError());
    const size_t n = (size_t)(K + 1) * (size_t)D;
    hipLaunchKernelGGL(edge_project_reduce_kernel, dim3((unsigned)((n + 255) / 256)), geo.block, 0, stream, (const float*)partial, geo.wg, K, D, d_dWe, d_dbe);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}
