// tcgnn_stage.inc - the staging pass every hot-path operator starts with, device and host: an abs-max pass writes the range words of
// the workspace's header, a conversion pass writes the scaled fp16 image behind it.  Included by tcgnn_device.hip, ahead of every kernel.
// In this order: the header's words; the scale and the rounding; the range guard's rule; the abs-max kernels and the converters
// (row-major, planar, the planar image in one pass over X, slice); image and workspace sizes; Guard; check_workspace; fill_header; one
// converter launcher per layout; launch_stage_onepass; stage_features; the C ABI of the caller-staged images, tcgnn_range_mode and
// tcgnn_plan_stage_stats.

// ---- the header: kHdrBytes at the start of a workspace (and of a caller-staged image, which carries word kHdrMaxX alone), 32-bit words.
// Every file names a word through this enum.  The X and the edge-value word of a pair are neighbours: range_spread and absmax_body
// step from one to the other.
enum HdrWord : int {
    kHdrMaxX = 0, kHdrMaxVal = 1,     // bits of max |X| / max |edge value|: the image's power-of-two scale (scale_exp_from_bits)
    kHdrLoX = 2, kHdrLoVal = 3,       // 0x7f800000 - bits of their smallest nonzero finite magnitude (0: none seen)
    kHdrCapX = 4, kHdrCapVal = 5,     // their caps: lost-precision terms one result can collect (0: guard off / caller-staged: never wide)
    kHdrTiny = 6,                     // n_tiny: elements of X that lose bits in the image (counted by the conversion pass)
    kHdrPow = 7,                      // the power of max |X| in the bound: 1 (SpMM) or 2 (SDDMM, fused AGNN)
    kHdrDirtyRows = 8,                // rows of X marked in the dirty-row bitmap (SDDMM / fused AGNN at guard level 2)
    kHdrStrict = 9,                   // nonzero: guard level 3 - a wide SDDMM / fused-AGNN call runs in plain fp32
    kHdrDwExtra = 10,                 // words 10 - 11, ONE double: wide_patch_kernel's correction of the fused backward's d_w (agnn_reduce_kernel adds it)
    kHdrWords = 12
};
static constexpr size_t kHdrBytes = 256;
static constexpr size_t kHdrRangeBytes = kHdrDirtyRows * sizeof(uint32_t);                       // what a second image of one matrix copies: words 0 .. 7
static constexpr size_t kHdrClearBytes = (kHdrWords * sizeof(uint32_t) + 63) / 64 * 64;          // what a fresh header clears: every word in use, in whole 64 bytes
static_assert(kHdrDwExtra % 2 == 0 && kHdrDwExtra + 2 == kHdrWords, "the header ends with an 8-byte aligned double");
static_assert(kHdrWords * sizeof(uint32_t) <= kHdrClearBytes && kHdrClearBytes <= kHdrBytes, "every word in use lies inside what is cleared, and that inside the header");
static_assert(kHdrMaxVal == kHdrMaxX + 1 && kHdrLoVal == kHdrLoX + 1 && kHdrCapVal == kHdrCapX + 1, "the edge values' word of a pair follows X's");

// Power-of-two exponent k such that absmax * 2^k lies in [2^14, 2^15): fp16-safe (max 65504) with
// 29 binades of normal range below the largest element.  0 for all-zero / non-finite data.
__device__ __forceinline__ int scale_exp_from_bits(uint32_t b) {
    if (b == 0u || b >= 0x7f800000u) return 0;
    int e = (int)(b >> 23) - 127;
    int k = 14 - e;
    return k > 126 ? 126 : (k < -126 ? -126 : k);
}
__device__ __forceinline__ float pow2f(int k) { return __uint_as_float((uint32_t)(127 + k) << 23); }

// Round to a 10-bit mantissa, nearest with ties AWAY from zero: bit-for-bit what the reference's
// wmma::__float_to_tf32 (cvt.rna.tf32.f32, TCGNN_kernel.cu:441-444) does.  The result has at most
// 11 significant bits, so the following fp32 -> fp16 conversion is exact for every element within
// 2^-28 of the (scaled) maximum; fp16's default nearest-EVEN would differ on ties (about one
// element in 2^13), which shows up as 2^-10-sized output differences.
__device__ __forceinline__ float round_rna10(float x) {   // the same rounding kept in fp32 (fallback kernels)
    uint32_t u = __float_as_uint(x);
    if ((u & 0x7f800000u) != 0x7f800000u) u = (u + 0x1000u) & 0xffffe000u;
    return __uint_as_float(u);
}
__device__ __forceinline__ _Float16 to_half_rna(float x) {
    uint32_t u = __float_as_uint(x);
    if ((u & 0x7f800000u) != 0x7f800000u) u = (u + 0x1000u) & 0xffffe000u;
    return (_Float16)__uint_as_float(u);
}

// ---- the within-matrix range guard (SURVEY.md 7.3, VERDICT r02 item 6) -------------------------------------------------------
// The fp16 operand image carries ONE power-of-two scale per matrix: an element more than 2^28 below the largest loses mantissa
// bits (fp16 subnormal) and one more than 2^39 below it is flushed to zero, where the reference's TF32 keeps fp32's exponent
// (TCGNN_kernel.cu:438-444).  The absolute error that leaves per element is <= max|X| * 2^-39, which stays far inside the
// contract's |d| <= 1e-3 max(1, |ref|) whenever max|X| < 2^8 - whatever the small elements are.  A matrix that holds BOTH an
// element >= 2^8 and a nonzero one more than 2^28 below the maximum is "wide": for it every fp16-path kernel returns at once and
// a fallback kernel launched behind it (plain fp32, operands rounded exactly like the reference's, CSR order) does the work; for
// every other matrix the fallback returns at once.  The decision is made on the device from the staging pass's header words (HdrWord),
// so no call synchronises or reads anything back.
// How large is "large": what an element below max 2^-28 loses is at most max 2^-39 in absolute terms, and a result may collect at
// most k such errors - k = min(cap, n_tiny), cap = the longest row of the graph (SpMM) or 2 D (SDDMM, fused AGNN: the terms of one
// dot product), n_tiny = how many elements of the matrix lose bits at all (counted by the conversion pass: ONE stray 1e-5 in a
// matrix of 1e4's - what a training epoch's activations look like, tools/probe_training_ranges.py - costs one error, not cap).
// The sum must stay inside the contract's 1e-3 max(1, |ref|) whatever the result is, i.e. below 2^-10:
//   binary SpMM        k max 2^-39 <= 2^-10                 -> wide iff     log2 max  >= 29 - log2 k
//   SDDMM / fused AGNN k max^2 2^-39 <= 2^-10               -> wide iff 2 * log2 max  >= 29 - log2 k
//   edge-valued SpMM   2 k max|A| max|X| 2^-39 <= 2^-10     -> wide iff log2 max|A| + log2 max|X| >= 28 - log2 k
// (k = 0: X, 1: the edge values.  Host and device: tcgnn_range_mode reports the decision with the same four functions on a copy of the header words)
__host__ __device__ __forceinline__ bool range_spread(const uint32_t* hdr, int k, int& emax) {
    const uint32_t mx = hdr[kHdrMaxX + k], mi = hdr[kHdrLoX + k];
    emax = (int)(mx >> 23);
    if (mi == 0u || mx == 0u || mx >= 0x7f800000u) return false;
    return emax - (int)((0x7f800000u - mi) >> 23) > 28;
}
__host__ __device__ __forceinline__ int ceil_log2_u32(uint32_t k) {
#ifdef __HIP_DEVICE_COMPILE__
    return k <= 1u ? 0 : 32 - __clz((int)(k - 1u));
#else
    return k <= 1u ? 0 : 32 - __builtin_clz(k - 1u);
#endif
}
__host__ __device__ __forceinline__ bool range_is_wide(const uint32_t* hdr, int) {   // the feature matrix alone (binary SpMM, SDDMM, fused AGNN)
    int emax;
    const uint32_t cap = hdr[kHdrCapX], n = hdr[kHdrTiny];
    if (!range_spread(hdr, 0, emax) || cap == 0u || n == 0u) return false;
    return (int)hdr[kHdrPow] * (emax - 127) >= 29 - ceil_log2_u32(n < cap ? n : cap);
}
__host__ __device__ __forceinline__ bool range_is_wide_val(const uint32_t* hdr) {
    int ex, ea;
    const bool sx = range_spread(hdr, 0, ex), sa = range_spread(hdr, 1, ea);
    const uint32_t cap = hdr[kHdrCapVal];
    if (!(sx || sa) || cap == 0u || hdr[kHdrMaxX] == 0u || hdr[kHdrMaxVal] == 0u) return false;
    const uint32_t n = hdr[kHdrTiny], k = (sa || n >= cap) ? cap : (n ? n : 1u);   // (edge values that lose bits are not counted: the longest row bounds them)
    return (ex - 127) + (ea - 127) >= 28 - ceil_log2_u32(k);
}
// ---- SDDMM and the fused AGNN pair at guard level 2: the way through a "wide" matrix (r04: a few dirty rows; r05: any number).
// What makes a matrix wide is elements that lose bits in the image, i.e. DIRTY ROWS of X - one stray 1e-5 among 1e4's in a training
// epoch (tools/probe_training_ranges.py), hub rows by the hundred on a power-law graph under the reference's unscaled weights.  The
// conversion pass marks them in a bitmap behind the image (one bit per row of X; kHdrDirtyRows counts them).  The MFMA kernels run
// as usual and wide_patch_kernel - one launch behind them, returning at once when nothing is wide - scans the edges and recomputes,
// in fp32 with the reference's operand rounding, every edge that touches a dirty row (its score, and what it contributes to the
// aggregate and to d_w), a wavefront per such edge: cost proportional to the dirty edges, 0.2 ms of scan when anything is wide at
// all.  r04 kept a list of at most 48 rows and left a matrix with more to the documented bound (VERDICT r04 "the default guard level
// leaves a hole"): the hole is closed.  Level 3 (kHdrStrict): the MFMA kernels return and the same launch does all the
// work in plain fp32 (wide_dense_body).  The aggregation operators, whose bound is linear and never reached in training, keep
// their own fallback kernels (spmm_wide_fallback_kernel, the fp32-MFMA walk).
__device__ __forceinline__ bool wide2_dense(const uint32_t* hdr) { return range_is_wide(hdr, 0) && hdr[kHdrStrict] != 0u; }   // (strict level: plain fp32)
// conversion pass: a thread that met an element losing bits marks the row; the first to mark a row counts it
__device__ __forceinline__ void note_dirty_row(uint32_t* hdr, uint32_t* bitmap, uint32_t nt, int64_t row) {
    if (!bitmap || !nt) return;
    const uint32_t bit = 1u << (row & 31);
    if (!(atomicOr(bitmap + (row >> 5), bit) & bit)) atomicAdd(hdr + kHdrDirtyRows, 1u);
}
// conversion pass: this thread's count of elements that lose bits (nonzero, below fp16's normal range once scaled) -> kHdrTiny
__device__ __forceinline__ void count_tiny(uint32_t* cnt, uint32_t mine) {   // mine <= 15; lanes that left the kernel early count as 0
    if (!cnt) return;
    uint32_t total = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) total += (uint32_t)__popcll(__ballot((mine >> b) & 1u)) << b;
    if (total && (int)(threadIdx.x & 63) == __ffsll((long long)__ballot(1)) - 1) atomicAdd(cnt, total);
}
// (decided on the SOURCE element and its scaled fp32 value, not on the converted half: an element more than 2^39 below the maximum
//  converts to exactly 0 and must still count - ADVICE r03: one 1e12 among O(1) data had n_tiny = 0 and stayed on the MFMA path)
__device__ __forceinline__ uint32_t is_tiny(float x, float s) { return (x != 0.0f && fabsf(x * s) < 6.103515625e-5f) ? 1u : 0u; }

// ------------------------------------------------------------------------------------------
// staging: absmax + fp32 -> scaled fp16 copy with a zero sentinel row
// ------------------------------------------------------------------------------------------
// (out_lo: where the smallest nonzero magnitude is recorded for the range guard, nullptr: not wanted - images a caller stages
//  itself, tcgnn_stage_absmax, carry no such word and are never "wide")
// Both absmax kernels: kAbsmaxThreads threads per workgroup, four independent 16-byte loads in flight per thread (r03: one load per
// trip of a grid-stride loop left 8 KB in flight per CU - 25 us for the 60 MB of a Reddit-shaped X, 2.4 TB/s), one atomic per
// workgroup and word.
constexpr int kAbsmaxThreads = 1024;
// one workgroup per CU at most, and none without sixteen 16-byte loads per thread to do
static inline int absmax_grid(int64_t n) { return (int)std::min<int64_t>(256, n / ((int64_t)kAbsmaxThreads * 64) + 1); }
// SCALED (tcgnn_spmm_scaled): the operand is cs[row] * X'[row, :] (X' = X where the gate lets it through), rows of D elements - the
// matrix the kernels actually round, so that the guard decides as it would for the composition tcgnn_spmm(cs * X').
template <bool GATED, bool SCALED = false>
__device__ __forceinline__ void absmax_body(const float* __restrict__ p, const float* __restrict__ gate, int64_t n, uint32_t* out, uint32_t* out_lo,
                                            uint32_t guard_cap, uint32_t guard_pow, const float* __restrict__ cs = nullptr, int64_t D = 1) {
    uint32_t m = 0, lo = 0;   // lo: 0x7f800000 - bits of the smallest nonzero finite magnitude (larger = smaller; 0 = none): range_is_wide
    auto see = [&](float f, float gt) {
        const uint32_t b = (!GATED || gt > 0.0f) ? __float_as_uint(f) & 0x7fffffffu : 0u;
        m = max(m, b);
        lo = max(lo, (b - 1u < 0x7f7fffffu) ? 0x7f800000u - b : 0u);   // (b - 1 wraps for 0: zero, Inf and NaN do not count)
    };
    auto see4 = [&](const float4& v, const float4& gt) { see(v.x, gt.x); see(v.y, gt.y); see(v.z, gt.z); see(v.w, gt.w); };
    // (SCALED: the row of element e; a 32-bit division wherever the matrix has fewer than 2^32 elements - the 64-bit one is ~4x the
    //  instructions in a pass that is otherwise a stream of loads)
    const bool n32 = n <= (int64_t)0xffffffffu;
    auto row_of = [&](int64_t e) -> int64_t { return n32 ? (int64_t)((uint32_t)e / (uint32_t)D) : e / D; };
    auto sc4 = [&](float4 v, int64_t k4) {   // (SCALED: a float4 lies inside one row - the vector path needs D % 4 == 0)
        if constexpr (SCALED) {
            const float c = cs[row_of(k4 << 2)];
            v.x = c * v.x; v.y = c * v.y; v.z = c * v.z; v.w = c * v.w;
        }
        return v;
    };
    auto sc1 = [&](float v, int64_t k) {
        if constexpr (SCALED) {
            v = cs[row_of(k)] * v;
        }
        return v;
    };
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    const uintptr_t both = reinterpret_cast<uintptr_t>(p) | (GATED ? reinterpret_cast<uintptr_t>(gate) : 0);
    if ((both & 15) == 0 && (!SCALED || D % 4 == 0)) {   // (scalar loads: 85 us for 2 x 60 MB)
        const int64_t n4 = n >> 2;
        const float4* p4 = reinterpret_cast<const float4*>(p);
        const float4* g4 = reinterpret_cast<const float4*>(gate);
        const float4 one = {1.f, 1.f, 1.f, 1.f};
        int64_t k = gid;
        for (; k + 3 * gsz < n4; k += 4 * gsz) {
            const float4 v0 = sc4(p4[k], k), v1 = sc4(p4[k + gsz], k + gsz), v2 = sc4(p4[k + 2 * gsz], k + 2 * gsz), v3 = sc4(p4[k + 3 * gsz], k + 3 * gsz);
            if constexpr (GATED) {
                const float4 t0 = g4[k], t1 = g4[k + gsz], t2 = g4[k + 2 * gsz], t3 = g4[k + 3 * gsz];
                see4(v0, t0); see4(v1, t1); see4(v2, t2); see4(v3, t3);
            } else { see4(v0, one); see4(v1, one); see4(v2, one); see4(v3, one); }
        }
        if (k < n4) {   // the last, partial round: its loads in flight together as well (one by one they were a 4 us tail of a 15 us kernel)
            const float4 zero = {0.f, 0.f, 0.f, 0.f};
            const bool b1 = k + gsz < n4, b2 = k + 2 * gsz < n4;
            const float4 v0 = sc4(p4[k], k), v1 = b1 ? sc4(p4[k + gsz], k + gsz) : zero, v2 = b2 ? sc4(p4[k + 2 * gsz], k + 2 * gsz) : zero;
            if constexpr (GATED) {
                const float4 t0 = g4[k], t1 = b1 ? g4[k + gsz] : zero, t2 = b2 ? g4[k + 2 * gsz] : zero;
                see4(v0, t0); see4(v1, t1); see4(v2, t2);
            } else { see4(v0, one); see4(v1, one); see4(v2, one); }
        }
        for (int64_t t = (n4 << 2) + gid; t < n; t += gsz) see(sc1(p[t], t), GATED ? gate[t] : 1.f);
    } else {
        for (int64_t k = gid; k < n; k += gsz) see(sc1(p[k], k), GATED ? gate[k] : 1.f);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { m = max(m, (uint32_t)__shfl_xor((int)m, off)); lo = max(lo, (uint32_t)__shfl_xor((int)lo, off)); }
    // one atomic per workgroup: a single word saturates near 88 atomics/us (MI355X_MICROARCH.md
    // "dequeue"), so per-wave atomics from a 2048-block grid alone cost ~90 us
    __shared__ uint32_t wmax[kAbsmaxThreads / 64], wlo[kAbsmaxThreads / 64];
    if ((threadIdx.x & 63) == 0) { wmax[threadIdx.x >> 6] = m; wlo[threadIdx.x >> 6] = lo; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nwv = (int)(blockDim.x >> 6);
        m = 0; lo = 0;
        for (int w = 0; w < nwv; ++w) { m = max(m, wmax[w]); lo = max(lo, wlo[w]); }
        if (m) atomicMax(out, m);
        if (lo && out_lo) atomicMax(out_lo, lo);
        // (out_lo is X's or the edge values' kHdrLo word: its cap and, for X, the power: range_is_wide; bit 8 of guard_pow -> the STRICT
        //  level, a matrix with many dirty rows takes the fp32 way)
        if (out_lo && blockIdx.x == 0) {
            out_lo[kHdrCapX - kHdrLoX] = guard_cap;
            if (guard_pow) { out_lo[kHdrPow - kHdrLoX] = guard_pow & 0xffu; out_lo[kHdrStrict - kHdrLoX] = guard_pow >> 8; }
        }
    }
}
__global__ __launch_bounds__(kAbsmaxThreads) void absmax_kernel(const float* __restrict__ p, int64_t n,
                                                                uint32_t* out, uint32_t* out_lo, uint32_t guard_cap, uint32_t guard_pow) {
    absmax_body<false>(p, nullptr, n, out, out_lo, guard_cap, guard_pow);
}
// absmax over the elements a gate lets through (gate > 0): the ReLU backward mask applied while staging dY
__global__ __launch_bounds__(kAbsmaxThreads) void absmax_gated_kernel(const float* __restrict__ p, const float* __restrict__ gate, int64_t n, uint32_t* out, uint32_t* out_lo, uint32_t guard_cap, uint32_t guard_pow) {
    absmax_body<true>(p, gate, n, out, out_lo, guard_cap, guard_pow);
}
// absmax of cs[row] * X'[row, :] (tcgnn_spmm_scaled's column scale, gate optional): rows of D elements
template <bool GATED>
__global__ __launch_bounds__(kAbsmaxThreads) void absmax_scaled_kernel(const float* __restrict__ p, const float* __restrict__ gate, const float* __restrict__ cs, int64_t n,
                                                                       int64_t D, uint32_t* out, uint32_t* out_lo, uint32_t guard_cap, uint32_t guard_pow) {
    absmax_body<GATED, true>(p, gate, n, out, out_lo, guard_cap, guard_pow, cs, D);
}

// One thread per 16-byte output chunk (8 halves).  Rows: N real + 1 all-zero sentinel row that
// padding columns of the tile stream point at (the reference zero-fills those, :423-424).
// (the scaled twin below differs in `c *` alone and is kept apart deliberately: profiles/r14/staging_refactor_ab.txt)
template <bool VEC>
__global__ __launch_bounds__(256) void convert_kernel(const float* __restrict__ X, int32_t N,
                                                      int32_t D, int32_t Dpad, int32_t pitch,
                                                      _Float16* __restrict__ X16,
                                                      const uint32_t* __restrict__ hdr, const float* __restrict__ G, int64_t ldx,
                                                      uint32_t* __restrict__ tiny, uint32_t* __restrict__ dirty_bitmap) {
    if (ldx == 0) ldx = D;   // row stride of X (and G) in floats: > D when X is a column block of a wider matrix
    const int cpr = Dpad >> 3;
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = ((int64_t)N + 1) * cpr;
    if (q >= total) return;
    const int64_t row = q / cpr;
    const int d0 = (int)(q - row * cpr) * 8;
    const float s = pow2f(scale_exp_from_bits(hdr[kHdrMaxX]));
    half8 o;
    uint32_t nt = 0;   // elements that lose bits in the image (range guard): nonzero, below fp16's normal range once scaled
    if (row < N && VEC && d0 + 8 <= D) {
        const float4* src = reinterpret_cast<const float4*>(X + row * ldx + d0);
        const float4 a = src[0], b = src[1];
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool on = !G || G[row * ldx + d0 + j] > 0.0f;
            o[j] = on ? to_half_rna(v[j] * s) : (_Float16)0.0f;
            nt += on ? is_tiny(v[j], s) : 0u;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int d = d0 + j;
            const bool on = row < N && d < D && (!G || G[row * ldx + d] > 0.0f);
            const float v = on ? X[row * ldx + d] : 0.0f;
            o[j] = to_half_rna(v * s);
            nt += is_tiny(v, s);
        }
    }
    *reinterpret_cast<half8*>(X16 + row * pitch + d0) = o;
    note_dirty_row(const_cast<uint32_t*>(hdr), dirty_bitmap, nt, row);
    count_tiny(tiny, nt);
}
// tcgnn_spmm_scaled: convert_kernel on cs[row] * X'[row, :], multiplied in fp32 before the power-of-two scale and the rounding
template <bool VEC>
__global__ __launch_bounds__(256) void convert_scaled_kernel(const float* __restrict__ X, const float* __restrict__ cs, int32_t N,
                                                             int32_t D, int32_t Dpad, int32_t pitch,
                                                             _Float16* __restrict__ X16,
                                                             const uint32_t* __restrict__ hdr, const float* __restrict__ G, int64_t ldx,
                                                             uint32_t* __restrict__ tiny, uint32_t* __restrict__ dirty_bitmap) {
    if (ldx == 0) ldx = D;
    const int cpr = Dpad >> 3;
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = ((int64_t)N + 1) * cpr;
    if (q >= total) return;
    const int64_t row = q / cpr;
    const int d0 = (int)(q - row * cpr) * 8;
    const float s = pow2f(scale_exp_from_bits(hdr[kHdrMaxX]));
    half8 o;
    uint32_t nt = 0;
    if (row < N && VEC && d0 + 8 <= D) {
        const float4* src = reinterpret_cast<const float4*>(X + row * ldx + d0);
        const float4 a = src[0], b = src[1];
        const float c = cs[row];
        const float v[8] = {c * a.x, c * a.y, c * a.z, c * a.w, c * b.x, c * b.y, c * b.z, c * b.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool on = !G || G[row * ldx + d0 + j] > 0.0f;
            o[j] = on ? to_half_rna(v[j] * s) : (_Float16)0.0f;
            nt += on ? is_tiny(v[j], s) : 0u;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int d = d0 + j;
            const bool on = row < N && d < D && (!G || G[row * ldx + d] > 0.0f);
            const float v = on ? cs[row] * X[row * ldx + d] : 0.0f;
            o[j] = to_half_rna(v * s);
            nt += is_tiny(v, s);
        }
    }
    *reinterpret_cast<half8*>(X16 + row * pitch + d0) = o;
    note_dirty_row(const_cast<uint32_t*>(hdr), dirty_bitmap, nt, row);
    count_tiny(tiny, nt);
}

// fp32 X -> PLANAR fp16 image for the LDS kernel: plane p = columns 16p .. 16p+15 of every row, [planes][N + 1][16]
// halves (32-byte records; row N all zero).  A column range of one plane is then one contiguous run of memory (each
// LDS-DMA instruction moves 1 KB of consecutive bytes), and inside LDS a row's 16-column slices sit a whole plane apart:
// the transposed read of slice s is the SAME address register with the immediate offset s * plane.
// One thread per 16-byte chunk; writes are consecutive.  Rounding as convert_kernel.
// (CS: tcgnn_spmm_scaled's column scale, as in convert_scaled_kernel)
template <bool VEC, bool CS>
__device__ __forceinline__ void convert_planar_body(const float* __restrict__ X, int32_t N, int32_t D, int32_t nplanes,
                                                    _Float16* __restrict__ X16, const uint32_t* __restrict__ hdr,
                                                    const float* __restrict__ G, uint32_t* __restrict__ tiny, const float* __restrict__ cs) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t per_plane = ((int64_t)N + 1) * 2;
    if (q >= per_plane * nplanes) return;
    const int p = (int)(q / per_plane);
    const int64_t rem = q - (int64_t)p * per_plane;
    const int64_t row = rem >> 1;
    const int d0 = p * 16 + (int)(rem & 1) * 8;
    const float s = pow2f(scale_exp_from_bits(hdr[kHdrMaxX]));
    half8 o;
    uint32_t nt = 0;   // (range guard: elements that lose bits in the image - counted on the source values, is_tiny)
    if (row < N && VEC && d0 + 8 <= D) {
        const float4* src = reinterpret_cast<const float4*>(X + row * D + d0);
        const float4 a = src[0], b = src[1];
        float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        if constexpr (CS) {
            const float c = cs[row];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = c * v[j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool on = !G || G[row * D + d0 + j] > 0.0f;
            o[j] = on ? to_half_rna(v[j] * s) : (_Float16)0.0f;
            nt += on ? is_tiny(v[j], s) : 0u;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int d = d0 + j;
            const bool on = row < N && d < D && (!G || G[row * D + d] > 0.0f);
            const float v = on ? (CS ? cs[row] * X[row * D + d] : X[row * D + d]) : 0.0f;
            o[j] = to_half_rna(v * s);
            nt += is_tiny(v, s);
        }
    }
    *reinterpret_cast<half8*>(X16 + q * 8) = o;
    count_tiny(tiny, nt);
}

template <bool VEC>
__global__ __launch_bounds__(256) void convert_planar_kernel(const float* __restrict__ X, int32_t N, int32_t D, int32_t nplanes,
                                                             _Float16* __restrict__ X16, const uint32_t* __restrict__ hdr,
                                                             const float* __restrict__ G, uint32_t* __restrict__ tiny) {
    convert_planar_body<VEC, false>(X, N, D, nplanes, X16, hdr, G, tiny, nullptr);
}
template <bool VEC>
__global__ __launch_bounds__(256) void convert_planar_scaled_kernel(const float* __restrict__ X, const float* __restrict__ cs, int32_t N, int32_t D, int32_t nplanes,
                                                                    _Float16* __restrict__ X16, const uint32_t* __restrict__ hdr,
                                                                    const float* __restrict__ G, uint32_t* __restrict__ tiny) {
    convert_planar_body<VEC, true>(X, N, D, nplanes, X16, hdr, G, tiny, cs);
}

// The same image for D % 16 == 0 (no padding columns), read the way X lies in memory: one thread per float4, so a wavefront
// reads 1 KB of consecutive bytes and writes, per plane, the 32-byte records of consecutive rows - whole lines.  (The
// chunk-per-thread version above reads 64-byte pieces a row apart and touches every line of X twice, from two planes: 30 us
// for Reddit at D = 64 against 17 us this way.)  The all-zero sentinel row is written by the threads past the last float4.
template <bool CS>
__device__ __forceinline__ void convert_planar_rows_body(const float* __restrict__ X, int32_t N, int32_t D, _Float16* __restrict__ X16,
                                                         const uint32_t* __restrict__ hdr, const float* __restrict__ G, uint32_t* __restrict__ tiny,
                                                         const float* __restrict__ cs) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int q = D >> 2;                              // float4 per row
    const int64_t total = (int64_t)N * q;
    if (f >= total + q) return;
    const int64_t row = f / q;                         // (row == N: the sentinel row)
    const int c4 = (int)(f - row * q);
    half4 o = {(_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f};
    uint32_t nt = 0;   // (range guard)
    if (f < total) {
        const float s = pow2f(scale_exp_from_bits(hdr[kHdrMaxX]));
        float4 v = reinterpret_cast<const float4*>(X)[f];
        if (G) {
            const float4 gt = reinterpret_cast<const float4*>(G)[f];
            if (!(gt.x > 0.0f)) v.x = 0.0f;
            if (!(gt.y > 0.0f)) v.y = 0.0f;
            if (!(gt.z > 0.0f)) v.z = 0.0f;
            if (!(gt.w > 0.0f)) v.w = 0.0f;
        }
        if constexpr (CS) {
            const float c = cs[row];
            v.x = c * v.x; v.y = c * v.y; v.z = c * v.z; v.w = c * v.w;
        }
        o[0] = to_half_rna(v.x * s); o[1] = to_half_rna(v.y * s); o[2] = to_half_rna(v.z * s); o[3] = to_half_rna(v.w * s);
        nt = is_tiny(v.x, s) + is_tiny(v.y, s) + is_tiny(v.z, s) + is_tiny(v.w, s);
    }
    const int plane = c4 >> 2;
    *reinterpret_cast<half4*>(X16 + (((int64_t)plane * ((int64_t)N + 1) + row) * 16 + (c4 & 3) * 4)) = o;
    count_tiny(tiny, nt);
}

__global__ __launch_bounds__(256) void convert_planar_rows_kernel(const float* __restrict__ X, int32_t N, int32_t D, _Float16* __restrict__ X16,
                                                                  const uint32_t* __restrict__ hdr, const float* __restrict__ G, uint32_t* __restrict__ tiny) {
    convert_planar_rows_body<false>(X, N, D, X16, hdr, G, tiny, nullptr);
}
__global__ __launch_bounds__(256) void convert_planar_rows_scaled_kernel(const float* __restrict__ X, const float* __restrict__ cs, int32_t N, int32_t D, _Float16* __restrict__ X16,
                                                                         const uint32_t* __restrict__ hdr, const float* __restrict__ G, uint32_t* __restrict__ tiny) {
    convert_planar_rows_body<true>(X, N, D, X16, hdr, G, tiny, cs);
}

// ---- the planar image of whole aligned float4 rows in ONE pass over X (stage_features: where launch_convert_planar would take the
// rows kernel).  The second read of X above exists only because the power-of-two scale is not known during the first, and from call to
// call it rarely changes: it moves when max |X| crosses a power of two.  So the plan remembers, per kind of call, the scale exponent
// of the last matrix staged (tcgnn_plan::d_stage, a guess and nothing more), and
//   stage_fused_kernel   (pass 1) reads X once, abs-max as absmax_body and - with a usable guess - conversion as
//                        convert_planar_rows_body with s = 2^guess; every workgroup leaves {max bits, lo word, tiny count, the guess
//                        word it converted with} in its own 16-byte slot behind the dirty-row bitmap; workgroup 0 clears the header;
//   stage_settle_kernel  (pass 2, the same grid) reduces the slots (4 KB at most), writes the header words, and returns when every
//                        workgroup converted with the true exponent (a HIT); on a MISS it stores the true exponent as the next guess
//                        and converts X with it, as the two-pass path would have.
// Plain stores in pass 1, the stream's order between the passes: no workgroup waits for another.  A hit is an EQUAL exponent - a
// neighbouring scale would change which elements are tiny - so image, header and everything behind them are bit for bit what
// memset + absmax + convert_planar_rows produce.  The guess word is read by every workgroup of pass 1 on its own: a second stream
// storing into it meanwhile makes the slots disagree, which is a miss.
constexpr int kStageSlots = 256;          // absmax_grid's ceiling, and this path's: one slot per workgroup of pass 1
constexpr int kStageHintEntries = 16;     // direct-mapped by stage_hint_index
enum StageWord : int { kStageHits = kStageHintEntries, kStageMisses = kStageHintEntries + 1, kStageWords = kStageHintEntries + 2 };   // tcgnn_plan::d_stage
// a guess word: 0 = none, else the exponent + 127 (scale_exp_from_bits returns -126 .. 126: words 1 .. 253)
__device__ __forceinline__ bool stage_hint_usable(uint32_t w) { return w - 1u < 253u; }
__device__ __forceinline__ uint32_t stage_hint_word(int k) { return (uint32_t)(k + 127); }
static inline int stage_hint_index(int32_t D, bool gated, bool scaled, uint32_t pow) {
    const uint32_t key = (uint32_t)(D >> 4) | (gated ? 0x100u : 0u) | (scaled ? 0x200u : 0u) | ((pow & 0xffu) << 10);
    return (int)((key * 0x9e3779b1u) >> 28);
}
// float4 f of X -> (row, float4 of the row), stepped by the grid's stride without a division per step
struct RowWalk {
    int32_t row, c4, q, drow, dc;
    __device__ __forceinline__ RowWalk(uint32_t f, uint32_t stride, int32_t q_) : q(q_) {
        row = (int32_t)(f / (uint32_t)q_); c4 = (int32_t)(f - (uint32_t)row * (uint32_t)q_);
        drow = (int32_t)(stride / (uint32_t)q_); dc = (int32_t)(stride - (uint32_t)drow * (uint32_t)q_);
    }
    __device__ __forceinline__ void step() { row += drow; c4 += dc; if (c4 >= q) { c4 -= q; ++row; } }
};
__device__ __forceinline__ _Float16* planar_rows_record(_Float16* X16, int32_t N, int64_t row, int c4) {   // (convert_planar_rows_body's store address)
    return X16 + (((int64_t)(c4 >> 2) * ((int64_t)N + 1) + row) * 16 + (c4 & 3) * 4);
}
// workgroup-wide maxima of four words and sum of a fifth, in every thread
__device__ __forceinline__ void stage_reduce(uint32_t (&mx)[4], uint32_t& sum) {
    __shared__ uint32_t part[kAbsmaxThreads / 64][5];
    __syncthreads();   // (a second reduction of one kernel: nobody still reads the first one's words)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) mx[j] = max(mx[j], (uint32_t)__shfl_xor((int)mx[j], off));
        sum += (uint32_t)__shfl_xor((int)sum, off);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) part[threadIdx.x >> 6][j] = mx[j];
        part[threadIdx.x >> 6][4] = sum;
    }
    __syncthreads();
    const int nwv = (int)(blockDim.x >> 6);
    sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) mx[j] = 0;
    for (int w = 0; w < nwv; ++w) {
#pragma unroll
        for (int j = 0; j < 4; ++j) mx[j] = max(mx[j], part[w][j]);
        sum += part[w][4];
    }
}
// The grid-stride walk both passes share, four 16-byte loads in flight per thread as in absmax_body.  ABS: the abs-max side - m and
// lo exactly as absmax_body's see() (tlo = the smallest b - 1 seen: zero wraps to the top, Inf and NaN lie at 0x7f7fffff or above, so a
// value below that is the smallest nonzero finite magnitude, less one).  CONV: the conversion side - convert_planar_rows_body element
// by element with scale s, the sentinel row included; nt counts the tiny elements.
template <bool GATED, bool CS, bool ABS, bool CONV>
__device__ __forceinline__ void stage_walk(const float* __restrict__ X, const float* __restrict__ G, const float* __restrict__ cs, int32_t N, int32_t D,
                                           _Float16* __restrict__ X16, float s, uint32_t& m, uint32_t& tlo, uint32_t& nt) {
    const int q = D >> 2;                                // float4 per row
    const int64_t n4 = (int64_t)N * q;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;   // (at most 2^18: kStageSlots workgroups of kAbsmaxThreads)
    const float4* p4 = reinterpret_cast<const float4*>(X);
    const float4* g4 = reinterpret_cast<const float4*>(G);
    const float4 one = {1.f, 1.f, 1.f, 1.f};
    auto see = [&](float f, float gt) {
        const uint32_t b = (!GATED || gt > 0.0f) ? __float_as_uint(f) & 0x7fffffffu : 0u;
        m = max(m, b);
        tlo = min(tlo, b - 1u);
    };
    auto take = [&](float4 v, const float4& gt, float c, int32_t row, int32_t c4) {
        if constexpr (ABS) {
            if constexpr (CS) { see(c * v.x, gt.x); see(c * v.y, gt.y); see(c * v.z, gt.z); see(c * v.w, gt.w); }
            else { see(v.x, gt.x); see(v.y, gt.y); see(v.z, gt.z); see(v.w, gt.w); }
        }
        if constexpr (CONV) {
            if constexpr (GATED) {
                if (!(gt.x > 0.0f)) v.x = 0.0f;
                if (!(gt.y > 0.0f)) v.y = 0.0f;
                if (!(gt.z > 0.0f)) v.z = 0.0f;
                if (!(gt.w > 0.0f)) v.w = 0.0f;
            }
            if constexpr (CS) { v.x = c * v.x; v.y = c * v.y; v.z = c * v.z; v.w = c * v.w; }
            half4 o;
            o[0] = to_half_rna(v.x * s); o[1] = to_half_rna(v.y * s); o[2] = to_half_rna(v.z * s); o[3] = to_half_rna(v.w * s);
            nt += is_tiny(v.x, s) + is_tiny(v.y, s) + is_tiny(v.z, s) + is_tiny(v.w, s);
            *reinterpret_cast<half4*>(planar_rows_record(X16, N, row, c4)) = o;
        }
    };
    RowWalk w((uint32_t)gid, (uint32_t)gsz, q);
    int64_t k = gid;
    for (; k + 3 * gsz < n4; k += 4 * gsz) {
        const int32_t r0 = w.row, c0 = w.c4; w.step();
        const int32_t r1 = w.row, c1 = w.c4; w.step();
        const int32_t r2 = w.row, c2 = w.c4; w.step();
        const int32_t r3 = w.row, c3 = w.c4; w.step();
        const float4 v0 = p4[k], v1 = p4[k + gsz], v2 = p4[k + 2 * gsz], v3 = p4[k + 3 * gsz];
        float4 t0 = one, t1 = one, t2 = one, t3 = one;
        if constexpr (GATED) { t0 = g4[k]; t1 = g4[k + gsz]; t2 = g4[k + 2 * gsz]; t3 = g4[k + 3 * gsz]; }
        float s0 = 1.f, s1 = 1.f, s2 = 1.f, s3 = 1.f;
        if constexpr (CS) { s0 = cs[r0]; s1 = cs[r1]; s2 = cs[r2]; s3 = cs[r3]; }
        take(v0, t0, s0, r0, c0); take(v1, t1, s1, r1, c1); take(v2, t2, s2, r2, c2); take(v3, t3, s3, r3, c3);
    }
    if (k < n4) {   // the last, partial round: its loads in flight together as well
        const bool b1 = k + gsz < n4, b2 = k + 2 * gsz < n4;
        const int32_t r0 = w.row, c0 = w.c4; w.step();
        const int32_t r1 = w.row, c1 = w.c4; w.step();
        const int32_t r2 = w.row, c2 = w.c4;
        const float4 v0 = p4[k], v1 = b1 ? p4[k + gsz] : one, v2 = b2 ? p4[k + 2 * gsz] : one;
        float4 t0 = one, t1 = one, t2 = one;
        if constexpr (GATED) { t0 = g4[k]; if (b1) t1 = g4[k + gsz]; if (b2) t2 = g4[k + 2 * gsz]; }
        float s0 = 1.f, s1 = 1.f, s2 = 1.f;
        if constexpr (CS) { s0 = cs[r0]; if (b1) s1 = cs[r1]; if (b2) s2 = cs[r2]; }
        take(v0, t0, s0, r0, c0);
        if (b1) take(v1, t1, s1, r1, c1);
        if (b2) take(v2, t2, s2, r2, c2);
    }
    if constexpr (CONV) {   // the all-zero sentinel row N of every plane
        const half4 zero = {(_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f};
        for (int64_t t = gid; t < q; t += gsz) *reinterpret_cast<half4*>(planar_rows_record(X16, N, N, (int)t)) = zero;
    }
}
template <bool GATED, bool CS>
__global__ __launch_bounds__(kAbsmaxThreads) void stage_fused_kernel(const float* __restrict__ X, const float* __restrict__ G, const float* __restrict__ cs, int32_t N, int32_t D,
                                                                     _Float16* __restrict__ X16, uint32_t* __restrict__ hdr, uint4* __restrict__ slots,
                                                                     const uint32_t* __restrict__ hint) {
    const uint32_t hw = *hint;
    const bool conv = stage_hint_usable(hw);
    uint32_t m = 0, tlo = 0xffffffffu, nt = 0;
    if (conv) stage_walk<GATED, CS, true, true>(X, G, cs, N, D, X16, pow2f((int)hw - 127), m, tlo, nt);
    else      stage_walk<GATED, CS, true, false>(X, G, cs, N, D, X16, 1.0f, m, tlo, nt);
    uint32_t mx[4] = {m, ~tlo, 0u, 0u};
    stage_reduce(mx, nt);
    if (threadIdx.x == 0) {
        const uint32_t t = ~mx[1];
        slots[blockIdx.x] = make_uint4(mx[0], t < 0x7f7fffffu ? 0x7f800000u - (t + 1u) : 0u, nt, conv ? hw : 0u);
    }
    if (blockIdx.x == 0 && threadIdx.x < (unsigned)kHdrWords) hdr[threadIdx.x] = 0u;   // (the only stores of this kernel into the header)
}
template <bool GATED, bool CS>
__global__ __launch_bounds__(kAbsmaxThreads) void stage_settle_kernel(const float* __restrict__ X, const float* __restrict__ G, const float* __restrict__ cs, int32_t N, int32_t D,
                                                                      _Float16* __restrict__ X16, uint32_t* __restrict__ hdr, const uint4* __restrict__ slots, int32_t nslots,
                                                                      uint32_t* __restrict__ stage, int32_t hint_index, uint32_t guard_cap, uint32_t guard_pow) {
    uint32_t mx[4] = {0u, 0u, 0u, 0u}, tiny = 0;   // max bits, lo word, the largest guess word and the complement of the smallest
    if ((int)threadIdx.x < nslots) {
        const uint4 p = slots[threadIdx.x];
        mx[0] = p.x; mx[1] = p.y; mx[2] = p.w; mx[3] = ~p.w; tiny = p.z;
    }
    stage_reduce(mx, tiny);
    const int k = scale_exp_from_bits(mx[0]);
    const bool hit = mx[2] == stage_hint_word(k) && ~mx[3] == mx[2];   // every workgroup of pass 1 converted, and with the true exponent
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        hdr[kHdrMaxX] = mx[0]; hdr[kHdrLoX] = mx[1]; hdr[kHdrCapX] = guard_cap;
        hdr[kHdrPow] = guard_pow & 0xffu; hdr[kHdrStrict] = guard_pow >> 8;
        if (hit) hdr[kHdrTiny] = tiny;
        else stage[hint_index] = stage_hint_word(k);
        atomicAdd(stage + (hit ? kStageHits : kStageMisses), 1u);
    }
    if (hit) return;
    uint32_t m = 0, tlo = 0, nt = 0;
    stage_walk<GATED, CS, false, true>(X, G, cs, N, D, X16, pow2f(k), m, tlo, nt);
    uint32_t none[4] = {0u, 0u, 0u, 0u};
    stage_reduce(none, nt);
    if (threadIdx.x == 0 && nt) atomicAdd(hdr + kHdrTiny, nt);   // (cleared by pass 1; workgroup 0 leaves it alone on a miss)
}

// A SLICE of rows into the planes of a caller's image (tcgnn_stage_rows_planar: a rank of a row-sharded run converts only ITS rows;
// plane p of the image starts plane_rows records behind plane p - 1).  One thread per 16-byte chunk, rounding as convert_kernel; no
// sentinel row, no range words: the caller's image holds zeros wherever nobody writes.
__global__ __launch_bounds__(256) void convert_planar_slice_kernel(const float* __restrict__ X, int32_t rows, int32_t D, int32_t nplanes, _Float16* __restrict__ dst,
                                                                   int64_t plane_rows, const uint32_t* __restrict__ word) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t per_plane = (int64_t)rows * 2;
    if (q >= per_plane * nplanes) return;
    const int p = (int)(q / per_plane);
    const int64_t rem = q - (int64_t)p * per_plane;
    const int64_t row = rem >> 1;
    const int d0 = p * 16 + (int)(rem & 1) * 8;
    const float s = pow2f(scale_exp_from_bits(word[kHdrMaxX]));
    half8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int d = d0 + j;
        o[j] = to_half_rna((d < D ? X[row * D + d] : 0.0f) * s);
    }
    *reinterpret_cast<half8*>(dst + (((int64_t)p * plane_rows + row) * 2 + (rem & 1)) * 8) = o;
}

// The same conversion for row lengths that rule out 16-byte loads (D % 4 != 0, e.g. Reddit's 41 classes): a workgroup stages
// 64 rows x D floats through LDS with coalesced scalar loads (the per-thread version above reads 32-byte pieces 4*D bytes
// apart: 58 us against 23 us for the vector path at the same size), then every thread emits 16-byte planar chunks.
__global__ __launch_bounds__(256) void convert_planar_tiled_kernel(const float* __restrict__ X, int32_t N, int32_t D, int32_t nplanes,
                                                                   _Float16* __restrict__ X16, const uint32_t* __restrict__ hdr,
                                                                   const float* __restrict__ G, uint32_t* __restrict__ tiny) {
    extern __shared__ float stage[];                 // [64][D]
    constexpr int ROWS = 64;
    const int64_t row0 = (int64_t)blockIdx.x * ROWS;
    const int64_t nrows = (int64_t)N + 1 - row0 < ROWS ? (int64_t)N + 1 - row0 : ROWS;   // includes the sentinel row N
    const float s = pow2f(scale_exp_from_bits(hdr[kHdrMaxX]));
    const int64_t total = nrows * D;
    uint32_t nt = 0;                                 // (range guard: counted where every source element is seen once)
    for (int64_t k = threadIdx.x; k < total; k += blockDim.x) {
        const int64_t e = row0 * D + k;
        float v = 0.0f;
        if (e < (int64_t)N * D && (!G || G[e] > 0.0f)) { const float x = X[e]; v = x * s; nt += is_tiny(x, s); }
        stage[k] = v;
    }
    __syncthreads();
    const int chunks = nplanes * 2;                  // 16-byte chunks per row
    for (int64_t c = threadIdx.x; c < nrows * chunks; c += blockDim.x) {
        const int r = (int)(c / chunks), ch = (int)(c % chunks);
        const int p = ch >> 1, d0 = p * 16 + (ch & 1) * 8;
        half8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = d0 + j < D ? to_half_rna(stage[(int64_t)r * D + d0 + j]) : (_Float16)0.0f;
        *reinterpret_cast<half8*>(X16 + (((int64_t)p * ((int64_t)N + 1) + row0 + r) * 2 + (ch & 1)) * 8) = o;
    }
    if (tiny && nt) atomicAdd(tiny, nt);   // (range guard; a loop of uneven trip counts: one atomic per thread that saw any - rare)
}

// Row pitch of the fp16 image in halves: a gathered row should touch as few 128-byte lines as
// possible (a 96-byte row at pitch 96 straddles two lines three times out of four: D = 41..48 ran
// slower than D = 64), so rows up to 128 B are padded to a power of two and longer ones to whole lines.
static int x16_pitch(int dpad) {
    const int bytes = dpad * 2;
    if (bytes > 128) return ((bytes + 127) / 128 * 128) / 2;   // whole lines (D = 602: 1280 B, not the 2048 B of the next power of two)
    int p = 32;
    while (p < bytes) p <<= 1;   // power of two: 32 B .. 128 B inside one line
    return p / 2;
}
// The gather walks address X16 through a structured buffer descriptor whose record stride (the row pitch in bytes) is a
// 14-bit field: a wider row would wrap it (stride 0 + the swizzle bit set) and every gather would silently read the wrong row.
static constexpr int kMaxStructStride = 16383;
// ... and whose index * stride + offset is formed in 32 bits: an image of 4 GB or more (a papers100M-sized shard: 111 M rows of
// 128 B) wraps.  The kernels then form 64-bit lane addresses instead (one v_mad_u64_u32 per gathered piece).
static int32_t image_is_big(int32_t rows, int pitch_halves) { return ((uint64_t)rows + 1) * (uint64_t)pitch_halves * 2u >= (1ull << 32) ? 1 : 0; }
static size_t image_bytes(const tcgnn_plan* plan, int pitch_halves) { return ((size_t)plan->Nc + 1) * pitch_halves * sizeof(_Float16); }   // (the rows a walk gathers from, + the zero row)
static bool pitch_fits_descriptor(int D) { return x16_pitch(round_up(D, 16)) * 2 <= kMaxStructStride; }

// (behind the image: the dirty-row bitmap of the range guard, one bit per row of X - wide_patch_kernel)
static size_t image_body_bytes(int32_t N, int32_t D) { return ((((size_t)N + 1) * (size_t)x16_pitch(round_up(D, 16)) * sizeof(_Float16)) + 255) / 256 * 256; }
static size_t dirty_bitmap_bytes(int32_t N) { return ((((size_t)N + 1 + 31) / 32) * 4 + 255) / 256 * 256; }
// (behind the bitmap: the one-pass staging's slot array, 16 bytes per workgroup of stage_fused_kernel - rewritten by every call that
//  takes that path before it is read, so the workspace carries nothing from call to call)
static constexpr size_t kStageSlotBytes = (size_t)kStageSlots * sizeof(uint4);
static size_t workspace_bytes_for(int32_t N, int32_t D) { return kHdrBytes + image_body_bytes(N, D) + dirty_bitmap_bytes(N) + kStageSlotBytes; }
static uint32_t* dirty_bitmap_of(void* ws, int32_t N, int32_t D) { return reinterpret_cast<uint32_t*>(static_cast<char*>(ws) + kHdrBytes + image_body_bytes(N, D)); }
static uint4* stage_slots_of(void* ws, int32_t N, int32_t D) { return reinterpret_cast<uint4*>(static_cast<char*>(ws) + kHdrBytes + image_body_bytes(N, D) + dirty_bitmap_bytes(N)); }

// ---- range guard parameters (range_is_wide): cap = how many lost-precision terms one result can collect at most - the longest row
// of the graph (SpMM) or 2 D (SDDMM / fused AGNN) - and the power of max|X| in the error bound.  cap 0 = guard off
// (tcgnn_set_range_guard(0), TCGNN_RANGE_GUARD=0).
static int g_range_guard = [] { const char* e = getenv("TCGNN_RANGE_GUARD"); return e ? atoi(e) : 2; }();   // (r04: 2 - the usual wide input of SDDMM / fused AGNN costs one patch launch; 3 = strict)
static inline int range_guard_of(const tcgnn_plan* p) { const int g = p ? (int)p->range_guard.load(std::memory_order_relaxed) : -1; return g >= 0 ? g : g_range_guard; }
struct Guard { uint32_t cap, pow; };
static Guard guard_spmm(const tcgnn_plan* p) { return {range_guard_of(p) ? (uint32_t)std::max(p->max_degree, 1) : 0u, 1u}; }
// (level 1, the default: the aggregation operators - binary and edge-valued SpMM, the fused dense update - whose bound is linear in
//  max|X| and which a training epoch never reaches; level 2 adds SDDMM and the fused AGNN pair, whose bound is QUADRATIC in max|X|:
//  an AGNN epoch of the reference's unscaled recipe crosses 2^14.5 with a single lost element now and then, and each such call
//  costs ~25 ms in the CSR fallbacks against 2 ms - so those two answer to the documented bound unless asked to be strict)
static Guard guard_sddmm(const tcgnn_plan* p, int D) { const int lv = range_guard_of(p); return {lv >= 2 ? (uint32_t)(2 * std::max(D, 1)) : 0u, 2u | (lv >= 3 ? 0x100u : 0u)}; }   // (bit 8: strict, kHdrStrict)

// the workspace the header prescribes for the call (tcgnn_workspace_bytes / tcgnn_sddmm2_workspace_bytes), whichever walk will run:
// a walk that needs less than that does not make a smaller buffer legal
static int check_workspace(const char* call, const void* ws, size_t ws_bytes, size_t need) {
    if (!ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 255))
        return fail(TCGNN_ERR_WORKSPACE, "%s: workspace needs %zu bytes 256-aligned, got %zu at %p", call, need, ws_bytes, ws);
    return TCGNN_OK;
}

// ---- one way to fill a header.  The edge values' words: n values under the SpMM's own cap (n = E; H E for a multi-head call - ONE
// scale and one range-guard decision for all heads)
static void launch_absmax_val(const tcgnn_plan* plan, const float* d_val, int64_t n, uint32_t* hdr, hipStream_t stream) {
    if (!d_val || n <= 0) return;   // (no caller gets here with a multi-head call without edges: tcgnn_spmm_heads returns before it stages)
    hipLaunchKernelGGL(absmax_kernel, dim3(absmax_grid(n)), dim3(kAbsmaxThreads), 0, stream, d_val, n, hdr + kHdrMaxVal, hdr + kHdrLoVal, guard_spmm(plan).cap, 0u);
}
// A fresh header: every word in use cleared, then abs-max of X under gx - gated / column-scaled like the image will be - and of the
// nval edge values, if any.  Whoever stages the blocks of a wider matrix fills the header once, over the whole matrix, with this.
static int fill_header(const tcgnn_plan* plan, uint32_t* hdr, const float* d_X, const float* d_gate, const float* d_cs, int32_t D, const Guard& gx, const float* d_val, int64_t nval,
                       hipStream_t stream) {
    HIP_TRY(hipMemsetAsync(hdr, 0, kHdrClearBytes, stream));
    const int64_t nx = (int64_t)plan->Nc * D;
    if (nx > 0) {
        const dim3 grid(absmax_grid(nx)), block(kAbsmaxThreads);
        uint32_t* const mx = hdr + kHdrMaxX; uint32_t* const lo = hdr + kHdrLoX;
        if (d_cs && d_gate) hipLaunchKernelGGL(absmax_scaled_kernel<true>, grid, block, 0, stream, d_X, d_gate, d_cs, nx, (int64_t)D, mx, lo, gx.cap, gx.pow);
        else if (d_cs) hipLaunchKernelGGL(absmax_scaled_kernel<false>, grid, block, 0, stream, d_X, d_gate, d_cs, nx, (int64_t)D, mx, lo, gx.cap, gx.pow);
        else if (d_gate) hipLaunchKernelGGL(absmax_gated_kernel, grid, block, 0, stream, d_X, d_gate, nx, mx, lo, gx.cap, gx.pow);
        else hipLaunchKernelGGL(absmax_kernel, grid, block, 0, stream, d_X, nx, mx, lo, gx.cap, gx.pow);
    }
    launch_absmax_val(plan, d_val, nval, hdr, stream);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}

// ---- one converter launcher per layout: which kernel writes an image is decided here and nowhere else, and never shows in the image.
// 16-byte loads of X: whole float4 in every row from a 16-byte aligned start (ldx: the row stride of a column block; 0: D)
static bool rows_are_float4(const float* d_X, int32_t D, int64_t ldx) { return (D % 4 == 0) && (ldx % 4 == 0) && ((reinterpret_cast<uintptr_t>(d_X) & 15) == 0); }
// row-major, [rows + 1][x16_pitch] halves: a 16-byte chunk per thread
static void launch_convert_rows(const float* d_X, const float* d_cs, const float* d_gate, int32_t rows, int32_t D, int64_t ldx, _Float16* x16, const uint32_t* hdr, uint32_t* tiny,
                                uint32_t* dirty, hipStream_t stream) {
    const int dpad = round_up(D, 16), pitch = x16_pitch(dpad);
    const int64_t chunks = ((int64_t)rows + 1) * (dpad / 8);
    const dim3 grid((unsigned)((chunks + 255) / 256)), block(256);
    const bool vec = rows_are_float4(d_X, D, ldx);
    if (d_cs && vec) hipLaunchKernelGGL((convert_scaled_kernel<true>), grid, block, 0, stream, d_X, d_cs, rows, D, dpad, pitch, x16, hdr, d_gate, ldx, tiny, dirty);
    else if (d_cs)   hipLaunchKernelGGL((convert_scaled_kernel<false>), grid, block, 0, stream, d_X, d_cs, rows, D, dpad, pitch, x16, hdr, d_gate, ldx, tiny, dirty);
    else if (vec)    hipLaunchKernelGGL((convert_kernel<true>), grid, block, 0, stream, d_X, rows, D, dpad, pitch, x16, hdr, d_gate, ldx, tiny, dirty);
    else             hipLaunchKernelGGL((convert_kernel<false>), grid, block, 0, stream, d_X, rows, D, dpad, pitch, x16, hdr, d_gate, ldx, tiny, dirty);
}
// planar, [dpad / 16 planes][N + 1][16 halves] for the LDS-resident kernels (whole rows of X only).  The rows kernel where X and the
// gate are whole aligned float4 rows without padding columns; else a chunk per thread with 16-byte loads; without those the tiled
// kernel (unscaled, 64 rows of X within 48 KB of LDS), else a chunk per thread with scalar loads.
static void launch_convert_planar(const float* d_X, const float* d_cs, const float* d_gate, int32_t N, int32_t D, _Float16* x16, const uint32_t* hdr, uint32_t* tiny,
                                  hipStream_t stream) {
    const int nplanes = round_up(D, 16) / 16;
    const int64_t chunks = ((int64_t)N + 1) * 2 * nplanes;   // (as many as the row-major image has: no pitch padding)
    const dim3 cgrid((unsigned)((chunks + 255) / 256)), block(256);
    const bool vec = rows_are_float4(d_X, D, 0);
    if (vec && D % 16 == 0 && (!d_gate || (reinterpret_cast<uintptr_t>(d_gate) & 15) == 0)) {
        const int64_t threads = ((int64_t)N + 1) * (D / 4);
        const dim3 grid((unsigned)((threads + 255) / 256));
        if (d_cs) hipLaunchKernelGGL(convert_planar_rows_scaled_kernel, grid, block, 0, stream, d_X, d_cs, N, D, x16, hdr, d_gate, tiny);
        else      hipLaunchKernelGGL(convert_planar_rows_kernel, grid, block, 0, stream, d_X, N, D, x16, hdr, d_gate, tiny);
    } else if (d_cs) {
        if (vec) hipLaunchKernelGGL((convert_planar_scaled_kernel<true>), cgrid, block, 0, stream, d_X, d_cs, N, D, nplanes, x16, hdr, d_gate, tiny);
        else     hipLaunchKernelGGL((convert_planar_scaled_kernel<false>), cgrid, block, 0, stream, d_X, d_cs, N, D, nplanes, x16, hdr, d_gate, tiny);
    } else if (vec) hipLaunchKernelGGL((convert_planar_kernel<true>), cgrid, block, 0, stream, d_X, N, D, nplanes, x16, hdr, d_gate, tiny);
    else if ((size_t)D * 64 * sizeof(float) <= 48 * 1024)
        hipLaunchKernelGGL(convert_planar_tiled_kernel, dim3((unsigned)(((int64_t)N + 1 + 63) / 64)), block, (size_t)D * 64 * sizeof(float), stream, d_X, N, D, nplanes, x16, hdr, d_gate, tiny);
    else hipLaunchKernelGGL((convert_planar_kernel<false>), cgrid, block, 0, stream, d_X, N, D, nplanes, x16, hdr, d_gate, tiny);
}

// ---- the planar image in one pass over X (stage_fused_kernel + stage_settle_kernel).  tcgnn_set_stage_onepass(0) /
// TCGNN_STAGE_ONEPASS=0: every call stages with memset + abs-max + convert.
static int g_stage_onepass = [] { const char* e = getenv("TCGNN_STAGE_ONEPASS"); return e ? atoi(e) : 1; }();
// header cleared, range words of X written, image converted: what fill_header (without the edge values) + launch_convert_planar's rows
// kernel leave.  The caller checked onepass_takes.
static void launch_stage_onepass(const tcgnn_plan* plan, const float* d_X, const float* d_cs, const float* d_gate, int32_t D, const Guard& gx, void* ws, hipStream_t stream) {
    const int32_t N = plan->Nc;
    uint32_t* const hdr = static_cast<uint32_t*>(ws);
    _Float16* const x16 = reinterpret_cast<_Float16*>(static_cast<char*>(ws) + kHdrBytes);
    uint4* const slots = stage_slots_of(ws, N, D);
    // (a finer grid than absmax_grid's: a workgroup from one full round of float4 per thread, not four - at 16 columns the Reddit shape
    //  gave absmax_grid 57 workgroups, too few for a pass that also converts: 7 us slower than the two-pass staging, measured)
    const int nslots = (int)std::min<int64_t>(kStageSlots, (int64_t)N * (D / 4) / ((int64_t)kAbsmaxThreads * 4) + 1);
    const int idx = stage_hint_index(D, d_gate != nullptr, d_cs != nullptr, gx.pow);
    const dim3 grid(nslots), block(kAbsmaxThreads);
    uint32_t* const stage = plan->d_stage;
#define TCGNN_STAGE_ONEPASS_LAUNCH(GATED, CS)                                                                                                           \
    do {                                                                                                                                                \
        hipLaunchKernelGGL((stage_fused_kernel<GATED, CS>), grid, block, 0, stream, d_X, d_gate, d_cs, N, D, x16, hdr, slots, (const uint32_t*)(stage + idx)); \
        hipLaunchKernelGGL((stage_settle_kernel<GATED, CS>), grid, block, 0, stream, d_X, d_gate, d_cs, N, D, x16, hdr, (const uint4*)slots, (int32_t)nslots, \
                           stage, (int32_t)idx, gx.cap, gx.pow);                                                                                        \
    } while (0)
    if (d_gate && d_cs) TCGNN_STAGE_ONEPASS_LAUNCH(true, true);
    else if (d_gate)    TCGNN_STAGE_ONEPASS_LAUNCH(true, false);
    else if (d_cs)      TCGNN_STAGE_ONEPASS_LAUNCH(false, true);
    else                TCGNN_STAGE_ONEPASS_LAUNCH(false, false);
#undef TCGNN_STAGE_ONEPASS_LAUNCH
}

struct StagedImage { const uint32_t* hdr = nullptr; const _Float16* x16 = nullptr; int dpad = 0, pitch = 0; };
struct StageOpts {
    bool planar = false;                 // [dpad / 16 planes][Nc + 1][16 halves] for the LDS-resident kernels instead of row-major
    const float* d_gate = nullptr;
    // ldx > 0: X (and the gate) is a column block of a wider row-major matrix with that row stride; the scale words in the
    // header were then computed over the WHOLE matrix by the caller (block_of_wider = true: fill_header was the caller's), so
    // every block is rounded exactly as the undivided call would round it.
    int64_t ldx = 0; bool block_of_wider = false;
    // hdr_from: the scale words of an image of the same matrix staged a moment ago (the planar one of a plan with a cold remainder):
    // copied instead of recomputed, so both images are rounded with the same scale without a second pass over X
    const uint32_t* hdr_from = nullptr;
    const Guard* guard = nullptr;        // (null: the binary SpMM's bound; else the caller's operator has its own)
    const float* d_cs = nullptr;         // (tcgnn_spmm_scaled): the operand is d_cs[row] * X'[row, :] - absmax, tiny count and image all of that product
};
// the one-pass path takes a call where launch_convert_planar takes the rows kernel and the header is this call's own to fill
static bool onepass_takes(const tcgnn_plan* plan, const float* d_X, int32_t D, const StageOpts& o) {
    return g_stage_onepass && plan->d_stage && o.planar && !o.hdr_from && !o.block_of_wider && (int64_t)plan->Nc * D > 0 && rows_are_float4(d_X, D, 0) && D % 16 == 0 &&
           (!o.d_gate || (reinterpret_cast<uintptr_t>(o.d_gate) & 15) == 0);
}
// enqueue absmax(X) [+ absmax(val)] + convert; *out: the fp16 image
static int stage_features(const tcgnn_plan* plan, const float* d_X, const float* d_val, int32_t D, void* ws, size_t ws_bytes, hipStream_t stream, const StageOpts& o, StagedImage* out) {
    const Guard gx = o.guard ? *o.guard : guard_spmm(plan);
    if (const int rc = check_workspace("staging", ws, ws_bytes, workspace_bytes_for(plan->Nc, D))) return rc;
    uint32_t* hdr = static_cast<uint32_t*>(ws);
    _Float16* x16 = reinterpret_cast<_Float16*>(static_cast<char*>(ws) + kHdrBytes);
    if (onepass_takes(plan, d_X, D, o)) {
        launch_stage_onepass(plan, d_X, o.d_cs, o.d_gate, D, gx, ws, stream);
        launch_absmax_val(plan, d_val, plan->E, hdr, stream);   // (its words were cleared by pass 1)
        HIP_TRY(hipGetLastError());
        out->hdr = hdr; out->x16 = x16; out->dpad = round_up(D, 16); out->pitch = x16_pitch(out->dpad);
        return TCGNN_OK;
    }
    if (o.hdr_from) HIP_TRY(hipMemcpyAsync(hdr, o.hdr_from, kHdrRangeBytes, hipMemcpyDeviceToDevice, stream));
    else if (!o.block_of_wider) { if (const int rc = fill_header(plan, hdr, d_X, o.d_gate, o.d_cs, D, gx, d_val, plan->E, stream)) return rc; }
    uint32_t* const tiny = o.hdr_from ? nullptr : hdr + kHdrTiny;   // (a second image of the same matrix: its elements are counted already)
    if (o.planar) launch_convert_planar(d_X, o.d_cs, o.d_gate, plan->Nc, D, x16, hdr, tiny, stream);
    else {
        uint32_t* const dirty = (tiny && (gx.pow & 0xffu) == 2u && gx.cap) ? dirty_bitmap_of(ws, plan->Nc, D) : nullptr;   // (SDDMM / fused AGNN at guard level 2: dirty rows for wide_patch_kernel)
        if (dirty) HIP_TRY(hipMemsetAsync(dirty, 0, dirty_bitmap_bytes(plan->Nc), stream));
        launch_convert_rows(d_X, o.d_cs, o.d_gate, plan->Nc, D, o.ldx, x16, hdr, tiny, dirty, stream);
    }
    HIP_TRY(hipGetLastError());
    out->hdr = hdr; out->x16 = x16; out->dpad = round_up(D, 16); out->pitch = x16_pitch(out->dpad);
    return TCGNN_OK;
}

// ---- C ABI: images a caller stages itself (one abs-max word, no range words: never "wide") and the guard's decision read back
extern "C" {

int tcgnn_x16_pitch(int32_t D) { return D < 1 ? 0 : x16_pitch(round_up(D, 16)); }

int tcgnn_stage_absmax(const float* d_X, int64_t n, uint32_t* d_word, void* stream_v) {
    if (n < 0 || (n > 0 && !d_X) || !d_word) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_stage_absmax: null argument");
    if (n == 0) return TCGNN_OK;
    const int grid = absmax_grid(n);
    hipLaunchKernelGGL(absmax_kernel, dim3(grid), dim3(kAbsmaxThreads), 0, static_cast<hipStream_t>(stream_v), d_X, n, d_word, (uint32_t*)nullptr, 0u, 0u);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}

int tcgnn_stage_rows(const float* d_X, int32_t rows, int32_t D, const uint32_t* d_absmax_word, void* d_dst, void* stream_v) {
    if (rows < 0 || D < 1 || (rows > 0 && !d_X) || !d_absmax_word || !d_dst) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_stage_rows: bad argument");
    if ((reinterpret_cast<uintptr_t>(d_dst) & 15) != 0) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_stage_rows: destination must be 16-byte aligned");
    launch_convert_rows(d_X, nullptr, nullptr, rows, D, 0, static_cast<_Float16*>(d_dst), d_absmax_word, nullptr, nullptr, static_cast<hipStream_t>(stream_v));
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}

int tcgnn_stage_rows_planar(const float* d_X, int32_t rows, int32_t D, const uint32_t* d_absmax_word, void* d_dst, int64_t plane_rows, void* stream_v) {
    if (rows < 0 || D < 1 || (rows > 0 && !d_X) || !d_absmax_word || !d_dst || plane_rows < rows) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_stage_rows_planar: bad argument");
    if ((reinterpret_cast<uintptr_t>(d_dst) & 31) != 0) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_stage_rows_planar: destination must be 32-byte aligned");
    const int nplanes = round_up(D, 16) / 16;
    const int64_t chunks = (int64_t)rows * 2 * nplanes;
    if (chunks > 0) {
        hipLaunchKernelGGL(convert_planar_slice_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream_v), d_X, rows, D, nplanes,
                           static_cast<_Float16*>(d_dst), plane_rows, d_absmax_word);
        HIP_TRY(hipGetLastError());
    }
    return TCGNN_OK;
}

// which way the last staged call on this workspace went: the range guard's own rule (range_is_wide / range_is_wide_val) on the header words
int tcgnn_range_mode(const void* d_workspace, void* stream_v, int32_t* wide_x, int32_t* wide_val) {
    if (!d_workspace || !wide_x) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_range_mode: null argument");
    uint32_t h[kHdrDwExtra];   // (the range words and flags: everything in front of the d_w correction)
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    HIP_TRY(hipMemcpyAsync(h, d_workspace, sizeof(h), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *wide_x = range_is_wide(h, 0) ? 1 : 0;
    if (*wide_x && h[kHdrPow] == 2u) *wide_x = h[kHdrStrict] ? 1 : 2;   // (SDDMM / fused AGNN: a few dirty rows - MFMA kernel + wide_patch_kernel; many - fp32 only at the strict level)
    if (wide_val) *wide_val = range_is_wide_val(h) ? 1 : 0;
    return TCGNN_OK;
}

// how the one-pass staging of this plan's calls went so far: calls whose guess of the scale held / calls that converted again
int tcgnn_plan_stage_stats(const tcgnn_plan* plan, void* stream_v, int64_t* hits, int64_t* misses) {
    if (!plan || !hits || !misses) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_plan_stage_stats: null argument");
    uint32_t h[2] = {0u, 0u};
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (plan->d_stage) {
        HIP_TRY(hipMemcpyAsync(h, plan->d_stage + kStageHits, sizeof(h), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    *hits = h[0]; *misses = h[1];
    return TCGNN_OK;
}

} // extern "C"
