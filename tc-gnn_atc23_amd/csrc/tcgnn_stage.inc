// tcgnn_stage.inc - the staging pass every hot-path operator starts with, device and host: an abs-max pass writes the range words of
// the workspace's header, a conversion pass writes the scaled fp16 image behind it.  Included by tcgnn_device.hip, ahead of every kernel.
// In this order: the header's words; the scale and the rounding; the range guard's rule; the abs-max kernels and the converters
// (row-major, planar, slice); image and workspace sizes; Guard; check_workspace; fill_header; one converter launcher per layout;
// stage_features; the C ABI of the caller-staged images and tcgnn_range_mode.

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
static size_t workspace_bytes_for(int32_t N, int32_t D) { return kHdrBytes + image_body_bytes(N, D) + dirty_bitmap_bytes(N); }
static uint32_t* dirty_bitmap_of(void* ws, int32_t N, int32_t D) { return reinterpret_cast<uint32_t*>(static_cast<char*>(ws) + kHdrBytes + image_body_bytes(N, D)); }

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
// enqueue absmax(X) [+ absmax(val)] + convert; *out: the fp16 image
static int stage_features(const tcgnn_plan* plan, const float* d_X, const float* d_val, int32_t D, void* ws, size_t ws_bytes, hipStream_t stream, const StageOpts& o, StagedImage* out) {
    const Guard gx = o.guard ? *o.guard : guard_spmm(plan);
    if (const int rc = check_workspace("staging", ws, ws_bytes, workspace_bytes_for(plan->Nc, D))) return rc;
    uint32_t* hdr = static_cast<uint32_t*>(ws);
    _Float16* x16 = reinterpret_cast<_Float16*>(static_cast<char*>(ws) + kHdrBytes);
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

} // extern "C"
