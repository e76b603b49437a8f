// tcgnn_launch.inc - what every launch table shares: a kernel family's launch geometry, the width dispatcher, the launch itself.
// Included by tcgnn_device.hip in front of the kernels.  Each family states its geometry ONCE, beside its kernel (spmm_geom,
// blocked_geom, sync_geom, heads_geom, sddmm_geom, sddmm_heads_geom, agnn_geom, lds_geom, flat_geom, val_geom): the kernel's
// __launch_bounds__, its launcher and every persistent-grid size in the dispatch files read it.
struct LaunchGeom {
    int threads;          // per workgroup
    int lds_bytes;        // dynamic LDS per workgroup
    int waves_per_simd;   // the kernel's second launch bound: its register budget
    int maxw;             // windows a persistent wavefront owns (0: the walk is not persistent)
    // workgroups of a persistent grid resident on one CU: what its 160 KB of LDS hold, at most what the kernel's registers allow
    // (four SIMDs of waves_per_simd wavefronts), at least one
    constexpr int wgs_per_cu() const { return std::max(1, std::min(waves_per_simd * 256 / threads, (160 * 1024) / lds_bytes)); }
};

// for the pin tables beside each geometry: f(1) .. f(N) against the literal values the formulas this geometry replaced gave
template <class F, int N>
static constexpr bool widths_give(F f, const int (&want)[N]) {
    for (int n = 1; n <= N; ++n) if (f(n) != want[n - 1]) return false;
    return true;
}

// a run-time width n in 1 .. MAX as a compile-time constant: f(std::integral_constant<int, n>{}); any other n is an invalid value
template <int MAX, class F>
static hipError_t with_width(int n, F&& f) {
    if constexpr (MAX >= 1) {
        if (n == MAX) return f(std::integral_constant<int, MAX>{});
        return with_width<MAX - 1>(n, f);
    } else {
        return hipErrorInvalidValue;
    }
}

// more dynamic LDS than the 64 KB a kernel gets by default: asked for once per kernel and process (two streams may call into one plan)
template <auto Kernel>
static hipError_t raise_dynamic_lds(int bytes) {
    static std::atomic<bool> raised{false};
    if (raised.load(std::memory_order_acquire)) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) raised.store(true, std::memory_order_release);
    return e;
}
// one launch with the family's geometry.  RAISE_TO > 0: the kernel's LDS ceiling is raised to that many bytes first
template <auto Kernel, int RAISE_TO = 0, class... Args>
static hipError_t launch_kernel(dim3 grid, const LaunchGeom& g, hipStream_t stream, const Args&... args) {
    if constexpr (RAISE_TO > 0) {
        if (const hipError_t e = raise_dynamic_lds<Kernel>(RAISE_TO)) return e;
    }
    hipLaunchKernelGGL(Kernel, grid, dim3((unsigned)g.threads), (size_t)g.lds_bytes, stream, args...);
    return hipGetLastError();
}
// tcgnn_spmm_scaled's row scale / bias: the twin kernel with the epilogue in its store (its argument is {args, epi}), else the plain one
template <class T> T kernel_arg_of(void (*)(T));
template <auto Plain, auto Twin, int RAISE_TO = 0, class Args>
static hipError_t launch_plain_or_twin(dim3 grid, const LaunchGeom& g, hipStream_t stream, const Args& args, const Epi& epi) {
    if (epi.rs || epi.bias) return launch_kernel<Twin, RAISE_TO>(grid, g, stream, decltype(kernel_arg_of(Twin)){args, epi});
    return launch_kernel<Plain, RAISE_TO>(grid, g, stream, args);
}
