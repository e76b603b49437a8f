// tcgnn_device.hip - gfx950 (MI355X / CDNA4) kernels and C-ABI launchers of libtcgnn_hip.so.
//
// What replaces what (reference paths relative to /root/reference):
//   pack_kernel        legacy metadata -> packed tile stream.  The reference has no such step: its
//                      kernels rebuild every 16x8 tile by rescanning ALL edges of the window once
//                      per tile (TCGNN_kernel.cu:400-408, :656-663).  Packing once per graph
//                      removes that O(tiles x edges) work from every call.
//   absmax / convert   fp32 X -> fp16 staging copy, scaled by a per-call power of two so the
//                      10-bit-mantissa rounding equals the reference's TF32 rounding
//                      (wmma::__float_to_tf32, TCGNN_kernel.cu:438-444) without fp16's range limit.
//   spmm_kernel        TCGNN_kernel.cu:336-454 (binary A) and :459-578 (edge-valued A).
//   sddmm_kernel       TCGNN_kernel.cu:584-727.
//   spmm_blocked_kernel / spmm_lds_kernel (tcgnn_lds_spmm.inc) / spmm_small_kernel
//                      the same SpMM for big feature matrices (column-range-blocked gather), dense graphs (column ranges
//                      resident in LDS) and launch-latency-sized graphs (one launch, fp32 MFMA on fp32 X).
//   agnn_kernel        the SDDMM + edge-weighted SpMM pair of gnn_conv.py:115-158 in one gather, forward and backward.
//   *_csr_kernel       slow-but-correct HIP paths for CSRs whose rows are not strictly increasing
//                      (the packed edge-offset table assumes canonical rows).
//
// Data flow of one SpMM workgroup (one 16-row window, 1 or 4 wavefronts):
//   each wavefront walks its share of the window's 16x32 tiles; per tile it
//     (1) reads 32 source-row ids and a 16x32 adjacency bitmask (coalesced, 192 B),
//     (2) gathers the 32 fp16 feature rows straight into LDS with per-lane-addressed
//         global_load_lds_dwordx4 (no VGPR round trip, no ds_write), in an XOR-swizzled image,
//     (3) synthesises the MFMA A fragment from the bitmask in registers,
//     (4) reads B fragments with ds_read_b64_tr_b16 (hardware transpose: K runs over gathered
//         rows, which are the LDS rows) and issues one v_mfma_f32_16x16x32_f16 per 16 columns;
//   partial accumulators of the wavefronts are summed through LDS in a fixed order.
//
// File map (r04: one translation unit - the kernels are templates their launchers instantiate - cut by operator; in include order):
//   tcgnn_device.hip          HIP_TRY, DevBuf (owner of one device allocation), struct tcgnn_plan, KernelTimer, device helpers, switches
//                             and walk predicates, sync_chosen; behind the includes the C ABI of the operators.  It launches nothing
//   tcgnn_launch.inc          what the launch tables beside the kernels (*_geom, launch_*) share: LaunchGeom, with_width, launch_kernel, launch_plain_or_twin
//   tcgnn_stage.inc           the staging pass, device and host: the header's words by name, the range guard's rule, abs-max kernels and every
//                             fp16 converter (row-major, planar, slice), image and workspace sizes, Guard, fill_header, one converter launcher
//                             per layout, the one-pass staging of the planar image (stage_fused_kernel + stage_settle_kernel), stage_features;
//                             the C ABI of the caller-staged images, tcgnn_range_mode and tcgnn_plan_stage_stats
//   tcgnn_pack.inc            plan-time kernels (fill, longest row, locality, pack)
//   tcgnn_gather_spmm.inc     TileWalker, spmm_kernel; spmm_blocked_kernel's two forms from tcgnn_blocked_kernel.inc (+ generated tcgnn_lds_blocks.inc);
//                             launch_spmm_*, launch_blocked_*
//   tcgnn_heads.inc           multi-head edge-valued SpMM: HeadsWalker (TileWalker with one A fragment per head), spmm_heads_kernel, spmm_heads_csr_kernel;
//                             launch_heads_* (included behind tcgnn_small_fallback.inc)
//   tcgnn_sync_walk.inc       slice-synchronised range walk: SyncArgs, spmm_sync_kernel's two forms from tcgnn_sync_kernel.inc, launch_sync_*, table kernels
//   tcgnn_small_spmm.inc      spmm_small_kernel (single launch, fp32 MFMA on fp32 X; also the binary SpMM's range-guard fallback)
//   tcgnn_lds_spmm.inc        LDS-resident SpMM, ordinary cell stream; cell-stream build kernels
//   tcgnn_lds_flat.inc        LDS-resident SpMM, flat cell stream (the headline kernel; its forms from tcgnn_lds_flat_kernel.inc)
//   tcgnn_lds_val.inc         LDS-resident edge-valued SpMM (single-edge stream, per-call slot values)
//   tcgnn_sddmm.inc           sddmm_kernel, sddmm_wide_kernel (one and two operands), sddmm2_csr_kernel; launch_sddmm_*
//   tcgnn_agnn.inc            agnn_kernel (fused pair, forward / backward), slice sum, d_w reduction; launch_agnn*
//   tcgnn_small_fallback.inc  CSR kernels of non-canonical plans, the range guard's fallbacks, symmetry_kernel, wide_patch_kernel
//   tcgnn_transpose.inc       hand-written kernels of the CSR transpose (host side: tcgnn_transpose.hip)
//   tcgnn_sample.inc          seeded neighbour sampling: row counts + validation, the per-row select, both also from a list of rows (host side: tcgnn_sample.hip)
//   tcgnn_edge_softmax.inc    softmax over a row's edges, forward / backward, and its C ABI
//   tcgnn_gat.inc             multi-head GAT attention: fused score + softmax, its backward with d_er, per-source-node edge sums
//   tcgnn_segment_max.inc     element-wise maximum over a row's edges and its backward over A^T (the wide-row gather: a lane group per neighbour row)
//   tcgnn_segment_stats.inc   mean / std / max / min over a row's edges in one walk and the backward of all four over A^T (PNA; segment_max's scheduling)
//   tcgnn_gatv2.inc           GATv2 attention: fused score + softmax, the row-side backward (g, d_xr, d_attn), the source-side backward (d_xl)
//   tcgnn_edge_message.inc    a feature vector per edge: sum of act(X[col] + Ef) over a row's edges, its backward (the per-edge gradient dM),
//                             the sum of per-edge rows into nodes, optionally through perm over A^T (segment_max's scheduling)
//   tcgnn_lds_plan.inc        host side of the LDS-resident walks: time models, placement, build_lds_cells (a cell stream in named steps over a
//                             CellBuild; flat_entries, the entry records, is a pure host function; cells_publish cannot fail), build_val_stream
//   tcgnn_edge_dispatch.inc   host side of an SDDMM / fused-AGNN call: SddmmCall, route_sddmm, AgnnCall, route_agnn, launchers, run_sddmm, run_agnn
//   tcgnn_spmm_dispatch.inc   host side of an SpMM call: SpmmCall, route_spmm (which walk runs), one launcher per walk, run_spmm; of a
//                             multi-head call: route_heads, run_spmm_heads
//   tcgnn_plan.inc            plan lifetime: creation in named steps (order_windows, build_sync_tables, ...), destroy, info, prepare, timing, setters
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <numeric>
#include <type_traits>
#include <vector>

#include "tcgnn.h"
#include "tcgnn_internal.h"

using namespace tcgnn;

#define LDS_AS __attribute__((address_space(3)))
#define GLB_AS __attribute__((address_space(1)))

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef __attribute__((__vector_size__(4 * sizeof(__fp16)))) __fp16 fp16x4_raw;

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) return fail(TCGNN_ERR_HIP, "%s -> %s", #expr, hipGetErrorString(e_)); \
    } while (0)
static inline int hip_rc(hipError_t e) { return e == hipErrorOutOfMemory ? TCGNN_ERR_OOM : TCGNN_ERR_HIP; }
// Owner of one device allocation: frees it on every way out of a scope; release() hands the pointer over (to the plan, which keeps
// raw pointers) and returns the bytes handed over, so what the plan owns is summed from what it was given.
template <class T> struct DevBuf {
    T* ptr = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : ptr(o.ptr), bytes(o.bytes) { o.ptr = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(ptr, o.ptr); std::swap(bytes, o.bytes); return *this; }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { reset(); }
    hipError_t alloc(size_t count) {
        reset();
        const hipError_t e = hipMalloc(&ptr, count * sizeof(T));
        if (e == hipSuccess) bytes = count * sizeof(T); else ptr = nullptr;
        return e;
    }
    void reset() { if (ptr) (void)hipFree(ptr); ptr = nullptr; bytes = 0; }
    size_t release(T*& to) { const size_t b = bytes; to = ptr; ptr = nullptr; bytes = 0; return b; }
    operator T*() const { return ptr; }
};

struct tcgnn_plan {
    int32_t N = 0, nw = 0, nw_eff = 0;   // N: rows of A (= rows of Y)
    double near_frac = 0;                // share of the condensed columns within num_cols / 16 rows of their window (locality_kernel)
    int32_t Nc = 0;                      // columns of A = rows of X (== N unless row-sharded)
    int32_t row_off = 0;                 // X row holding A's row 0 (row-sharded SDDMM)
    int32_t* d_sym = nullptr;            // device word: 1 = structurally symmetric (symmetry_kernel at plan creation; canonical square plans only)
    int64_t E = 0, tc_blocks = 0, total_wb = 0, max_wb = 0;   // max_wb: wide blocks of the longest window
    int canonical = 0, waves = 1;
    int32_t max_degree = 0;              // longest row of A (max_degree_kernel at creation): the range guard's thresholds follow it
    const int32_t *rowptr = nullptr, *col = nullptr, *bp = nullptr, *e2c = nullptr, *e2r = nullptr; // borrowed
    int64_t* d_wb_ptr = nullptr;  // [nw_eff + 1] first wide block of each window
    int32_t* d_order = nullptr;   // [nw_eff] window ids, heaviest first
    int32_t* d_cols = nullptr;    // [total_wb][32] source row of each condensed column (N = none)
    uint32_t* d_mask = nullptr;   // [total_wb][16] bit c of word r: A[r][c] != 0
    int32_t* d_ebase = nullptr;   // [total_wb][16] CSR position of the first edge of row r in the tile
    // column buckets for the range-blocked SpMM (0 = graph too sparse per window / too small)
    int32_t nbuckets = 0, bucket_rows = 0;
    uint32_t* d_bptr = nullptr;   // [nw_eff][nbuckets + 1] tile offset of the first tile whose first column is in bucket >= k
    int32_t num_cus = 256;
    size_t bytes = 0;
    // one-pass staging (tcgnn_stage.inc): kStageHintEntries guess words - the scale exponent of the last matrix staged per kind of call,
    // 0 = none - then the hit and the miss counter.  Device words, zeroed at creation; a guess and two statistics, never state a result depends on
    uint32_t* d_stage = nullptr;
    // tables of the slice-synchronised range walk (tcgnn_sync_walk.inc; r06): graphs whose communities exceed an XCD's L2
    struct SyncTables {
        int32_t S = 0, R = 0, nwx = 0, kmax = 0, fb_shift = 0;
        uint32_t* d_T = nullptr;     // [nw_eff][kmax + 1]
        int32_t* d_nk = nullptr;     // [8 * R]
        double hot_frac = 0, avg_k = 0;   // share of the tiles inside their slice's hot buckets; hot buckets per slice, weighted by tiles
        int32_t max_k = 0;
        bool ok = false;
    } sync;
    // cell streams of the LDS-resident column-range SpMM (tcgnn_lds_spmm.inc), one per range length in use (lds_stream_of: 4 windows per
    // wavefront x 4 / 2 / 1 / 3 planes, 8 windows x 2 / 1 planes); nranges == 0: not built
    struct CellStream {   // published by build_lds_cells under its mutex; nranges is written last (release) and read first (acquire)
        std::atomic<int32_t> nranges{0};
        int32_t nwg = 0;
        int64_t tiles = 0;
        int32_t* d_order = nullptr;        // [nwg * 16 * maxw] window id of slot (workgroup, wavefront, window slot), -1 = none (lds_place_windows)
        // hot (workgroup, range) pairs: the ranges a workgroup streams into LDS.  Pair k of the compact cell table belongs to
        // workgroup wg for rbase[wg] <= k < rbase[wg + 1] and covers column range rlist[k].
        int32_t npairs = 0;
        int32_t* d_rbase = nullptr;        // [nwg + 1]
        int32_t* d_rlist = nullptr;        // [npairs + 4]
        // flat streams: the workgroup's walk as a list of ENTRIES (tcgnn_lds_flat.inc) - npairs and rbase then count entries, and
        // d_rl2 holds [entries][4] entry records (range | flags, -, range to fetch, -) and behind them [entries][16 wavefronts] descriptor words
        uint32_t* d_rl2 = nullptr;
        int32_t dense_entries = 0;
        // cold remainder: columns of the (workgroup, range) pairs too thin for a range fill, re-condensed per window in the gather
        // walks' packed format; run by spmm_kernel, ADDING into what the LDS-resident kernel stored
        int64_t cold_tiles = 0, hot_cols = 0, cold_cols = 0, cold_max = 0;   // cold_max: cold tiles of the longest window
        uint32_t* d_parts = nullptr;       // [slots] split windows: part | parts << 8 | LDS scratch index << 16 (nullptr: no window is split)
        int32_t nsplit = 0;                // windows shared by several wavefronts of their workgroup
        int64_t* d_cold_ptr = nullptr;     // [nw_eff + 1]
        int32_t* d_cold_cols = nullptr;    // [cold_tiles][32]
        uint32_t* d_cold_mask = nullptr;   // [cold_tiles][16]
        uint32_t* d_cell_ptr = nullptr;    // [nwg * nranges * 16 * maxw + 1] tile offset of cell (workgroup, range, wavefront, window slot)
        uint32_t* d_cell_tiles = nullptr;  // [tiles][32] 32 u16 row ids local to the range + 16 mask words
        // FLAT stream (tcgnn_lds_flat.inc): every cell of a hot pair has exactly flat_tpc tiles at a computed position - no cell
        // table, no ordinary tiles; what a cell holds beyond 32 flat_tpc columns sits in the cold remainder, which
        // spmm_cold_planar_kernel adds from the planar image.  0: an ordinary stream.
        int32_t flat_tpc = 0;
        uint32_t* d_flat = nullptr;        // [npairs][16 wavefronts][32 * maxw * flat_tpc words] metadata blocks
        int32_t* d_wcold_ptr = nullptr;    // [nwg * 16 + 1] the cold remainder as per-wavefront record lists, multiplied inside the flat kernel
        uint32_t* d_wcold = nullptr;       // [cold tiles][64 words] 32 column ids, 16 mask words, window slot (layouts with LDS to spare)
        // single-edge streams only (slot 6): CSR position of the edge in every K slot of the flat stream / of the cold tiles, -1: none
        int32_t* d_eidx = nullptr;         // [tiles][32], tile (pair k, wavefront v, entry x) = (k * 16 + v) * maxw * flat_tpc + x  (build time only)
        int32_t* d_cold_eidx = nullptr;    // [cold_tiles][32]                                                                          (build time only)
        uint16_t* d_eidx16 = nullptr;      // the same as offsets from the window's first CSR edge, 0xffff: none (what val_permute_kernel reads)
        uint16_t* d_cold_eidx16 = nullptr;
    };
    CellStream lds[8];   // (kLdsStreams; slot 6: the single-edge stream of the edge-valued LDS-resident SpMM, tcgnn_lds_val.inc; slot 7: slot 4's layout on 952-row ranges)
    // whole 64-column chunks run on slot 4 (760-row ranges) or slot 7 (952-row ranges): decided by build_lds_cells the first time either is
    // asked for (-1: not yet), then only that one is ever built
    mutable std::atomic<int8_t> lds_long{-1};
    // single-edge tile stream (built with slot 6, on the first edge-valued call that would use it): every condensed column repeated
    // once per edge, so a K slot of a tile carries exactly ONE edge and a per-call value array can sit beside the slots
    int64_t* d_xwb_ptr = nullptr;   // [nw_eff + 1]
    int32_t* d_xcols = nullptr;     // [total_xwb][32]
    uint32_t* d_xmask = nullptr;    // [total_xwb][16] one bit per column
    int32_t* d_xeidx = nullptr;     // [total_xwb][32] CSR position of the slot's edge, -1: none
    int64_t total_xwb = 0;
    std::atomic<int8_t> val_choice{-1};   // -1 not tried, 0 the single-edge stream is of no use here (gather walks), 1 built
    mutable std::atomic<int8_t> lds_choice[65];   // automatic mode, per padded width / 16: -1 not decided yet, 0 gather walks, 1 LDS-resident kernel
    tcgnn_plan() { for (auto& c : lds_choice) c.store(-1, std::memory_order_relaxed); }
    // optional kernel timing (tcgnn_plan_set_timing): event pairs around the main kernel launches; slots are claimed atomically
    // (two streams may call into one plan)
    mutable std::vector<hipEvent_t> ev;
    mutable std::atomic<int> ev_used{0};
    mutable std::atomic<const char*> last_kernel{""};   // name of the main kernel the last call launched (tcgnn_plan_last_kernel)
    // per-plan overrides of the process-wide switches (tcgnn_plan_set_spmm_mode / tcgnn_plan_set_range_guard; -1: follow the process-wide
    // value of tcgnn_set_spmm_mode / tcgnn_set_range_guard) - two plans of one process may differ
    std::atomic<int8_t> spmm_mode{-1}, range_guard{-1};
    std::vector<int32_t> h_bp;       // blockPartition on the host: window weights for the placement of the LDS-resident walks
    mutable std::atomic<int> lds_extra[2] = {{-1}, {-1}};   // window slots the split hub windows add (4 / 8 windows per wavefront); -1: not computed
};

// Brackets the dominant kernel (spmm / sddmm proper, not the staging pass) with HIP events on the
// stream it is launched on, when timing is enabled and a pair is free.
struct KernelTimer {
    const tcgnn_plan* p; hipStream_t s; int slot = -1;
    KernelTimer(const tcgnn_plan* plan, hipStream_t stream, const char* kernel_name = nullptr) : p(plan), s(stream) {
        if (p && kernel_name) p->last_kernel.store(kernel_name, std::memory_order_relaxed);
        if (p && !p->ev.empty()) {
            const int k = p->ev_used.fetch_add(1, std::memory_order_relaxed);
            if (2 * k + 1 < (int)p->ev.size()) { slot = k; (void)hipEventRecord(p->ev[2 * slot], s); }
            else p->ev_used.store((int)p->ev.size() / 2, std::memory_order_relaxed);   // full: stay saturated, never wrap
        }
    }
    void stop() { if (slot >= 0) { (void)hipEventRecord(p->ev[2 * slot + 1], s); slot = -1; } }   // (before the range guard's fallback launch: not part of the kernel)
    ~KernelTimer() { stop(); }
};

// ------------------------------------------------------------------------------------------
// small device helpers
// ------------------------------------------------------------------------------------------
static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
static constexpr int kXcds = 8;   // workgroups are dealt to the XCDs round-robin in launch order: workgroup b runs on XCD b % 8 (observed, used for speed only)

__device__ __forceinline__ float relu_if(int on, float v) { return on ? fmaxf(v, 0.0f) : v; }
// tcgnn_spmm_scaled's epilogue in the final store: Y[r, c] = relu(fl32(fl32(s * rs[r]) + bias[c])).  Each pointer may be null (that
// step is left out).  No contraction into an FMA: the result must equal torch's separate multiply and add bit for bit.
struct Epi { const float* rs; const float* bias; };
__device__ __forceinline__ float epi_apply(int relu, const Epi& e, int64_t row, int col, float v) {
#pragma clang fp contract(off)
    if (e.rs) v = v * e.rs[row];
    if (e.bias) v = v + e.bias[col];
    return relu_if(relu, v);
}

// LDS image of one tile: 32 gathered rows x (NT*16) halves, addressed in 16-byte slots.
// global_load_lds lands lane l of an instruction at slot (instr*64 + l), so the image is any
// bijection (row, slot-in-row) <-> slot we like, applied on the SOURCE address.  The bijection is
// chosen so that every 32-lane pass of ds_read_b64_tr_b16 (8 rows x 32 B) touches all 64 banks once.
template <int NT>
struct TileImage {
    static constexpr int C = 2 * NT; // 16-byte slots per row
    __device__ static __forceinline__ int slot(int row, int c) {
        if constexpr (NT == 1) {
            int rp = (row & ~0xC) | ((row & 4) << 1) | ((row & 8) >> 1); // swap row bits 2 and 3
            return rp * 2 + c;
        } else if constexpr (NT == 2) {
            return row * 4 + (c ^ (((row >> 3) & 1) << 1));
        } else if constexpr (NT == 4) {
            return row * 8 + (c ^ ((((row >> 1) & 1) << 1) | (((row >> 3) & 1) << 2)));
        } else if constexpr (NT == 8) {
            return row * 16 + (c ^ (((row & 3) | (((row >> 3) & 1) << 2)) << 1));
        } else {
            return row * C + c;
        }
    }
    __device__ static __forceinline__ void unslot(int q, int& row, int& c) {
        if constexpr (NT == 1) {
            int rp = q >> 1;
            row = (rp & ~0xC) | ((rp & 4) << 1) | ((rp & 8) >> 1);
            c = q & 1;
        } else if constexpr (NT == 2) {
            row = q >> 2;
            c = (q & 3) ^ (((row >> 3) & 1) << 1);
        } else if constexpr (NT == 4) {
            row = q >> 3;
            c = (q & 7) ^ ((((row >> 1) & 1) << 1) | (((row >> 3) & 1) << 2));
        } else if constexpr (NT == 8) {
            row = q >> 4;
            c = (q & 15) ^ (((row & 3) | (((row >> 3) & 1) << 2)) << 1);
        } else {
            row = q / C;
            c = q - row * C;
        }
    }
};

__device__ __forceinline__ half4 lds_read_tr16(const char* p) {
    fp16x4_raw v = __builtin_amdgcn_ds_read_tr16_b64_v4f16((LDS_AS fp16x4_raw*)(p));
    return __builtin_bit_cast(half4, v);
}

#include "tcgnn_launch.inc"
#include "tcgnn_stage.inc"
#include "tcgnn_pack.inc"

#include "tcgnn_gather_spmm.inc"
#include "tcgnn_sync_walk.inc"


#include "tcgnn_small_spmm.inc"
#include "tcgnn_lds_spmm.inc"
#include "tcgnn_lds_flat.inc"
#include "tcgnn_lds_val.inc"

#include "tcgnn_sddmm.inc"

#include "tcgnn_agnn.inc"

#include "tcgnn_small_fallback.inc"
#include "tcgnn_heads.inc"   // (behind the fallbacks: its range-guard kernel is spmm_wide_fallback_body per head)

#include "tcgnn_transpose.inc"
#include "tcgnn_sample.inc"

#include "tcgnn_edge_softmax.inc"
#include "tcgnn_gat.inc"
#include "tcgnn_segment_max.inc"
#include "tcgnn_segment_stats.inc"
#include "tcgnn_gatv2.inc"
#include "tcgnn_edge_message.inc"

// ---- run-time switches.  Product: TCGNN_SPMM_MODE / TCGNN_RANGE_GUARD (initial values of tcgnn_set_spmm_mode / tcgnn_set_range_guard,
// include/tcgnn.h) and TCGNN_VERBOSE (plan statistics on stderr).  TEST AIDS, read through test_knob() only - tests/ forces every walk
// and layout through them against the oracle; no caller needs them: TCGNN_LDS_AUTO=0 (automatic mode never takes the LDS-resident
// kernel), TCGNN_LDS_MAXW=4|8 (one layout for every pass), TCGNN_LDS_FLAT=0|1|2 (ordinary stream / tiles per cell),
// TCGNN_LDS_HOT_COLS (hot / cold threshold), TCGNN_LDS_PLACE=local|localsplit|global, TCGNN_AGNN_SLICED=0|1|2|16,
// TCGNN_SDDMM_XCD=0|1|2, TCGNN_RANGE_KB (column-range size of the range-major walks).  The A/B switches of closed experiments (r01-r03: DESIGN.md lists what each measured) are gone; the
// phase timers of the LDS-resident kernels (TCGNN_LDS_DBG) exist only in a -DTCGNN_DEBUG_TIMERS build (make DEBUG_TIMERS=1).
static const char* test_knob(const char* name) { return getenv(name); }
static int verbose_level() { const char* e = getenv("TCGNN_VERBOSE"); return e ? atoi(e) : 0; }   // (read per build, not once: builds are rare, and tests switch it on)
static constexpr int g_bucket_min_tiles = 2;   // tiles per (window, bucket) a bucket table needs
static int g_lds_auto = [] { const char* e = test_knob("TCGNN_LDS_AUTO"); return e ? atoi(e) : 1; }();
#ifdef TCGNN_DEBUG_TIMERS
static int g_lds_dbg = [] { const char* e = getenv("TCGNN_LDS_DBG"); return e ? atoi(e) : 0; }();
#else
static constexpr int g_lds_dbg = 0;
#endif
static constexpr int g_lds_fill_quota = 1;     // (r03: the wavefronts with an empty last slot take the range fills, -0.5 %)
static int g_spmm_mode = [] { const char* e = getenv("TCGNN_SPMM_MODE"); return e ? atoi(e) : 0; }();
static inline int spmm_mode_of(const tcgnn_plan* p) { const int m = p ? (int)p->spmm_mode.load(std::memory_order_relaxed) : -1; return m >= 0 ? m : g_spmm_mode; }
static constexpr size_t kBlockedMinBytes = 6u << 20;   // below this X16 is (nearly) L2-resident anyway
static constexpr size_t kRangeTargetBytes = 1u << 20;  // X16 bytes per column range: wavefronts drift by a range or two
                                                        // and the 4 MB L2 also streams metadata (sweep: 0.5-1.5 MB best at D=64)

// the fused AGNN backward keeps one double per workgroup (per window; the XCD-sliced walk: per slice and four windows) behind the fp16 image
static constexpr int kAgnnMaxSlices = 16;   // two rounds of eight (= XCDs)
static size_t agnn_partial_bytes(const tcgnn_plan* plan) {
    const size_t slots = std::max<size_t>((size_t)std::max(plan->nw_eff, 1), (size_t)kAgnnMaxSlices * (((size_t)std::max(plan->nw_eff, 1) + 3) / 4));
    return (slots * sizeof(double) + 255) / 256 * 256;
}

// The range-blocked walks bind up to 4 windows to one persistent wavefront for the whole launch: a hub window (skewed
// degrees) then holds its wavefront far beyond the others (measured on a Reddit-sized graph with a 93 k-degree hub:
// 2.48 ms against 1.60 ms for the per-window walk, which spreads a window over 4 wavefronts).  Automatic mode only takes
// them when the longest window is within 8x the mean.
static bool has_locality(const tcgnn_plan* plan) { return plan->near_frac > 0.5; }
static bool windows_balanced(const tcgnn_plan* plan) {
    return plan->nw_eff > 0 && plan->max_wb * (int64_t)plan->nw_eff <= 8 * std::max<int64_t>(plan->total_wb, 1);
}
// ... and when the bucket table can cut the image into ranges an XCD's 4 MB L2 holds (ogbn-products at D = 128: 8 buckets
// of 78 MB - the range-major SDDMM then only pays for its bookkeeping: 5.70 ms against 4.93 ms per-window)
// ... and when there are enough windows for two workgroups of persistent wavefronts per CU at 4 windows each: with 3750 /
// 6250 windows the range-blocked walk left the chip a quarter full (0.33 / 1.03 ms against 0.13 / 0.66 ms per-window).
static bool ranges_fit_l2(const tcgnn_plan* plan, size_t x16_bytes) {
    return plan->nbuckets > 0 && x16_bytes / (size_t)plan->nbuckets <= ((size_t)8 << 20) && plan->nw_eff >= 32 * plan->num_cus;
}
// automatic mode, SpMM and SDDMM alike: a range-major walk pays when the fp16 image overflows L2 and all of the above hold
static bool range_walk_pays(const tcgnn_plan* plan, size_t x16_bytes) {
    return x16_bytes > kBlockedMinBytes && windows_balanced(plan) && ranges_fit_l2(plan, x16_bytes) && !has_locality(plan);
}
// column ranges of a range-major walk: the image cut in halves until a range holds range_bytes (TCGNN_RANGE_KB, read per call, overrides
// the operator's size - tests: several ranges on a graph the oracle can handle), at most one range per bucket
static int range_count(const tcgnn_plan* plan, size_t x16_bytes, size_t range_bytes) {
    if (const char* e = test_knob("TCGNN_RANGE_KB")) range_bytes = (size_t)atol(e) << 10;
    int nranges = 1;
    while (nranges < plan->nbuckets && x16_bytes / nranges > range_bytes) nranges <<= 1;
    return nranges;
}
// ---- what every hot-path entry point asks of the caller's buffers BEFORE it enqueues anything (include/tcgnn.h "Alignment"): a
// refused call has touched neither the outputs nor the workspace.
// [N, D] outputs: spmm_cold_planar_kernel and spmm_cold_val_kernel read-modify-write Y as float4 wherever D % 4 == 0, and
// agnn_slice_sum_kernel stores it that way - on the host, so that no kernel carries a pointer test
static int check_output_aligned(const char* call, const char* what, const void* p) {
    if (reinterpret_cast<uintptr_t>(p) & 15) return fail(TCGNN_ERR_INVALID_ARG, "%s: %s must be 16-byte aligned, got %p", call, what, p);
    return TCGNN_OK;
}

#include "tcgnn_lds_plan.inc"

// When the walk is taken (automatic mode; TCGNN_SYNC=0 never, 2 whenever the tables exist; mode 5 forces it).  Measured on the ogbn-products
// shape with 25 / 50 / 100 / 200 communities (25 / 12.5 / 6.3 / 3.1 MB of image each at D = 128, half that at 64; tools/exp_r06d.py, kernel ms,
// per-window -> this walk):
//                      25             50             100            200
//   SpMM       D = 128   3.94 -> 3.13   3.64 -> 2.63   3.14 -> 2.47   3.02 -> 2.46     always
//   edge-valued          4.22 -> 3.70   3.95 -> 3.19   3.79 -> 2.98                    always
//   SDDMM                3.98 -> 3.39   3.39 -> 2.83   2.53 -> 2.54   2.30 -> 2.51     where a slice's hot span (avg_k buckets) exceeds ~10 MB of image
//   fused fwd            4.39 -> 4.41   4.17 -> 3.61   4.05 -> 3.29                    where it stays below ~20 MB (beyond, the two windows a
//   fused bwd            4.29 -> 4.42   4.03 -> 3.83   3.88 -> 3.57                    wavefront owns walk more phases than its L2 share covers)
//   SpMM       D = 64    1.77 -> 1.55   1.49 -> 1.49   1.42 -> 1.43                    beyond ~10 MB of hot span
//   edge-valued          2.15 -> 2.09   2.13 -> 2.02   2.07 -> 1.93                    always
//   SDDMM                1.84 -> 1.88   1.69 -> 1.77   1.65 -> 1.68                    never
//   fused fwd            2.29 -> 2.16   2.29 -> 2.03   2.24 -> 1.94                    always
//   fused bwd            2.24 -> 2.35   2.22 -> 2.24   2.18 -> 2.17                    never
// and at 48 columns (three tiles of width) every operator loses 5 - 10 %: the walk starts at 64.
// All of this holds for SPARSE windows - 25 wide blocks per window on that shape: the per-window walk splits a window over four wavefronts,
// and at ~6 tiles each its run starts and four-way reduction weigh as much as the gathers.  On the Reddit shape with 50 communities (141
// wide blocks per window, communities of 1.2 MB) the per-window walk is the better kernel for every operator (D = 128: SpMM 1.04 against
// 1.13 ms, SDDMM 1.14 / 1.28, fused 1.37 / 1.51 and 1.36 / 1.81; D = 64: edge-valued 0.80 / 0.97): the walk is only taken up to 64 wide
// blocks per window.
enum { kSyncSpmm = 0, kSyncVal = 1, kSyncSddmm = 2, kSyncFusedFwd = 3, kSyncFusedBwd = 4 };
static constexpr size_t kSyncPhaseBytes = (size_t)3 << 20;   // image bytes of one phase (products shape, D = 128: 3.01 / 2.77 / 2.72 ms at 1 / 2 / 3 MB)
static bool sync_chosen(const tcgnn_plan* plan, int pitch_bytes, int mode, int op, int nt) {
    if (!plan->sync.ok || (mode != 0 && mode != 5)) return false;
    const char* const env = test_knob("TCGNN_SYNC");
    const int knob = env ? atoi(env) : 1;
    if (!knob) return false;
    if (knob >= 2 || mode == 5) return true;
    if (!(has_locality(plan) && windows_balanced(plan)) || nt < 4 || plan->total_wb > (int64_t)64 * plan->nw_eff) return false;
    const double span_mb = plan->sync.avg_k * (double)((size_t)pitch_bytes << plan->sync.fb_shift) / 1048576.0;
    const bool wide = nt > 4;
    switch (op) {
        case kSyncSpmm: return wide || span_mb > 10.0;
        case kSyncVal: return true;
        case kSyncSddmm: return wide && span_mb > 10.0;
        case kSyncFusedFwd: return !wide || span_mb < 20.0;
        default: return wide && span_mb < 20.0;   // kSyncFusedBwd
    }
}
static SyncArgs sync_args(const tcgnn_plan* plan, int pitch_bytes) {
    const tcgnn_plan::SyncTables& t = plan->sync;
    size_t phase = kSyncPhaseBytes;
    if (const char* e = test_knob("TCGNN_RANGE_KB")) phase = (size_t)atol(e) << 10;
    const int m = (int)std::max<size_t>(1, phase / ((size_t)pitch_bytes << t.fb_shift));
    return SyncArgs{t.d_T, t.d_nk, t.kmax, std::min(m, t.kmax), t.S, t.R, t.nwx, 0, plan->nw_eff};
}

#include "tcgnn_edge_dispatch.inc"
#include "tcgnn_spmm_dispatch.inc"
#include "tcgnn_plan.inc"

// ------------------------------------------------------------------------------------------
// C ABI: the operators (plan lifetime, timing and the mode / guard setters: tcgnn_plan.inc)
// ------------------------------------------------------------------------------------------
extern "C" {

int tcgnn_agnn_supported(const tcgnn_plan* plan, int32_t D) { return agnn_supported(plan, D) ? 1 : 0; }

static int agnn_words_ok(const tcgnn_plan* plan, int64_t words, const char* name) {
    if (plan && words < 1 + (int64_t)plan->N)
        return fail(TCGNN_ERR_INVALID_ARG, "%s: d_ef_absmax holds %lld words, the call writes / reads 1 + N = %lld (max |ef| + one scale exponent per row)", name, (long long)words, 1 + (long long)plan->N);
    return TCGNN_OK;
}

static AgnnCall agnn_call(const tcgnn_plan* plan, const float* d_X, const float* d_w, float* d_ef, uint32_t* d_absmax, float* d_Y, float* d_dw, int32_t D, void* ws, size_t ws_bytes, void* stream, bool bwd) {
    AgnnCall c;
    c.plan = plan; c.d_X = d_X; c.d_w = d_w; c.d_ef = d_ef; c.d_absmax = d_absmax; c.d_Y = d_Y; c.d_dw = d_dw; c.D = D; c.ws = ws; c.ws_bytes = ws_bytes;
    c.stream = static_cast<hipStream_t>(stream); c.bwd = bwd; c.name = bwd ? "tcgnn_agnn_pair_backward" : "tcgnn_agnn_pair_forward";
    return c;
}

int tcgnn_agnn_pair_forward(const tcgnn_plan* plan, const float* d_X, const float* d_w, float* d_ef, uint32_t* d_ef_absmax, int64_t ef_absmax_words, float* d_Y,
                            int32_t D, void* ws, size_t ws_bytes, void* stream) {
    if (const int rc = agnn_words_ok(plan, ef_absmax_words, "tcgnn_agnn_pair_forward")) return rc;
    return run_agnn(agnn_call(plan, d_X, d_w, d_ef, d_ef_absmax, d_Y, nullptr, D, ws, ws_bytes, stream, false));
}

int tcgnn_agnn_pair_backward(const tcgnn_plan* plan, const float* d_dY, const float* d_w, const float* d_ef, const uint32_t* d_ef_absmax, int64_t ef_absmax_words,
                             float* d_G, float* d_dw, int32_t D, void* ws, size_t ws_bytes, void* stream) {
    if (const int rc = agnn_words_ok(plan, ef_absmax_words, "tcgnn_agnn_pair_backward")) return rc;
    return run_agnn(agnn_call(plan, d_dY, d_w, const_cast<float*>(d_ef), const_cast<uint32_t*>(d_ef_absmax), d_G, d_dw, D, ws, ws_bytes, stream, true));
}

size_t tcgnn_workspace_bytes(const tcgnn_plan* plan, int32_t D) {
    if (!plan || D < 1) return 0;
    // (the fused AGNN calls' reduction slots and the partial score streams of the LDS-resident SDDMM ride along)
    // ... and the second (row-major) image of a plan whose LDS-resident walk leaves a cold remainder to the gather walk
    const size_t image = workspace_bytes_for(plan->Nc, D);
    // (before the width's streams exist the answer is the conservative one; once built, only an ORDINARY stream with a cold
    //  remainder stages the second image - a flat stream's remainder reads the planar one)
    // (of route_spmm's conditions only the plan-and-width part: it does not know the call.  It does not test planar_records_fit either, so
    //  a width the record bound keeps off the LDS-resident kernel still reserves the second image - drift rather than intent, kept: the
    //  size is observable)
    const int dp = round_up(D, 16);
    bool two_images = lds_wanted(plan, spmm_mode_of(plan), dp);
    if (two_images) {
        LdsPass passes[2];
        const LdsStreamFacts f = lds_stream_facts(plan, passes, lds_passes(dp, passes));
        if (f.all_built && !f.rows_cold) two_images = false;
    }
    // (the edge-valued LDS-resident walk keeps its per-call slot values behind the image, once its stream exists: tcgnn_lds_val.inc;
    //  the width alone is asked - a stream only exists where val_lds_width_ok held)
    const size_t vals = val_lds_width(dp) ? val_stream_bytes(plan) : (size_t)0;
    return image + std::max({agnn_partial_bytes(plan) + agnn_slice_bytes(plan, D), two_images ? image : (size_t)0, vals});
}

// what every SpMM entry point has: the rest of the request is set by name
static SpmmCall spmm_call(const tcgnn_plan* plan, const float* d_X, float* d_Y, int32_t D, void* ws, size_t ws_bytes, void* stream) {
    SpmmCall c;
    c.plan = plan; c.d_X = d_X; c.d_Y = d_Y; c.D = D; c.ws = ws; c.ws_bytes = ws_bytes; c.stream = static_cast<hipStream_t>(stream);
    return c;
}

int tcgnn_spmm(const tcgnn_plan* plan, const float* d_X, float* d_Y, int32_t D, void* ws, size_t ws_bytes, void* stream) {
    return run_spmm(spmm_call(plan, d_X, d_Y, D, ws, ws_bytes, stream));
}

int tcgnn_spmm_fused(const tcgnn_plan* plan, const float* d_X, const float* d_gate, float* d_Y, int32_t D, int32_t flags,
                     void* ws, size_t ws_bytes, void* stream) {
    if (flags & ~TCGNN_FUSE_RELU) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_spmm_fused: unknown flag bits 0x%x", flags & ~TCGNN_FUSE_RELU);
    SpmmCall c = spmm_call(plan, d_X, d_Y, D, ws, ws_bytes, stream);
    c.relu = (flags & TCGNN_FUSE_RELU) ? 1 : 0; c.d_gate = d_gate;
    return run_spmm(c);
}

int tcgnn_spmm_scaled(const tcgnn_plan* plan, const float* d_X, const float* d_col_scale, const float* d_gate, const float* d_row_scale,
                      const float* d_bias, float* d_Y, int32_t D, int32_t flags, void* ws, size_t ws_bytes, void* stream) {
    if (flags & ~TCGNN_FUSE_RELU) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_spmm_scaled: unknown flag bits 0x%x", flags & ~TCGNN_FUSE_RELU);
    SpmmCall c = spmm_call(plan, d_X, d_Y, D, ws, ws_bytes, stream);
    c.relu = (flags & TCGNN_FUSE_RELU) ? 1 : 0; c.d_gate = d_gate;
    c.sc.col = d_col_scale; c.sc.row = d_row_scale; c.sc.bias = d_bias;   // (all null: exactly tcgnn_spmm_fused)
    return run_spmm(c);
}

int tcgnn_spmm_gemm(const tcgnn_plan* plan, const float* d_X, const float* d_W, float* d_Y, int32_t D_in, int32_t D_out, int32_t flags,
                    void* ws, size_t ws_bytes, void* stream) {
    if (flags & ~TCGNN_FUSE_RELU) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_spmm_gemm: unknown flag bits 0x%x", flags & ~TCGNN_FUSE_RELU);
    if (!d_W || D_out < 1) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_spmm_gemm: null W or D_out < 1");
    if (D_in > kMaxChunkDims || D_out > kMaxChunkDims)
        return fail(TCGNN_ERR_UNSUPPORTED, "tcgnn_spmm_gemm: the fused dense update covers D_in, D_out <= %d (got %d -> %d)", kMaxChunkDims, D_in, D_out);
    SpmmCall c = spmm_call(plan, d_X, d_Y, D_in, ws, ws_bytes, stream);
    c.relu = (flags & TCGNN_FUSE_RELU) ? 1 : 0; c.d_W = d_W; c.D_out = D_out;
    return run_spmm(c);
}

int tcgnn_spmm_staged(const tcgnn_plan* plan, const void* d_image, float* d_Y, int32_t D, void* stream) {
    if (!d_image || (reinterpret_cast<uintptr_t>(d_image) & 255)) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_spmm_staged: the image must be 256-byte aligned");
    // Every MFMA kernel opens with the range guard's test on the header's range words (kHdrLoX, kHdrCapX, kHdrTiny, kHdrPow); a caller-staged image carries no range words
    // (never "wide": there is no fp32 X to fall back to).  The gather walks are told so (SpmmArgs::unguarded) and never look at
    // bytes 4 .. 255 of the header: the image is READ-ONLY to this call, as the signature says - one staged image may be shared by
    // several streams or ranks (r04 cleared those words with a memset on the caller's image, a write racing with other readers).
    SpmmCall c = spmm_call(plan, nullptr, d_Y, D, nullptr, 0, stream);
    c.d_image = d_image; c.staged = StagedLayout::kRowMajor;
    return run_spmm(c);
}

// ---- r06: the staged image in the LDS-resident kernel's own (planar) layout, so that a row-sharded call keeps the fast kernel
// (VERDICT r05 item 5).  Would tcgnn_spmm run the LDS-resident kernel on this plan at this width?  Builds the width's cell streams if
// they are missing (synchronises once, like tcgnn_plan_prepare) and asks what route_spmm asks for a planar staged call.
static bool lds_takes_staged(const tcgnn_plan* plan, int32_t D, hipStream_t stream) {
    const int mode = spmm_mode_of(plan);
    const int dp = round_up(D, 16);
    if (!lds_wanted(plan, mode, dp) || !planar_records_fit(plan, dp)) return false;
    LdsPass passes[2];
    const int npass = lds_passes(dp, passes);
    bool ok, settle;
    const tcgnn_plan::CellStream* cold;
    (void)ensure_lds_streams(plan, stream, mode, dp, passes, npass, LdsBuild::kQuery, &ok);
    return ok && lds_streams_serve(plan, mode, passes, npass, false, true, &settle, &cold);   // (a query: what would settle the width is left to the call)
}

int tcgnn_spmm_staged_layout(const tcgnn_plan* plan, int32_t D, void* stream) {
    if (!plan || D < 1) return 0;
    return lds_takes_staged(plan, D, static_cast<hipStream_t>(stream)) ? 1 : 0;
}

int tcgnn_spmm_staged_planar(const tcgnn_plan* plan, const void* d_image, float* d_Y, int32_t D, void* stream) {
    if (!d_image || (reinterpret_cast<uintptr_t>(d_image) & 255)) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_spmm_staged_planar: the image must be 256-byte aligned");
    SpmmCall c = spmm_call(plan, nullptr, d_Y, D, nullptr, 0, stream);
    c.d_image = d_image; c.staged = StagedLayout::kPlanar;
    return run_spmm(c);
}

int tcgnn_spmm_val(const tcgnn_plan* plan, const float* d_X, const float* d_edge_val, float* d_Y, int32_t D,
                   void* ws, size_t ws_bytes, void* stream) {
    if (plan && plan->E > 0 && !d_edge_val) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_spmm_val: edge values are null");
    SpmmCall c = spmm_call(plan, d_X, d_Y, D, ws, ws_bytes, stream);
    if (plan && plan->E > 0) c.d_val = d_edge_val;
    return run_spmm(c);
}

size_t tcgnn_spmm_heads_workspace_bytes(const tcgnn_plan* plan, int32_t H, int32_t F) {
    if (!plan || H < 1 || F < 1 || (int64_t)H * F > INT32_MAX) return 0;
    return heads_workspace_bytes(plan, H, F);
}

int tcgnn_spmm_heads(const tcgnn_plan* plan, const float* d_X, const float* d_edge_val, float* d_Y, int32_t H, int32_t F,
                     void* ws, size_t ws_bytes, void* stream) {
    HeadsCall c;
    c.plan = plan; c.d_X = d_X; c.d_val = d_edge_val; c.d_Y = d_Y; c.H = H; c.F = F; c.ws = ws; c.ws_bytes = ws_bytes; c.stream = static_cast<hipStream_t>(stream);
    return run_spmm_heads(c);
}

static SddmmCall sddmm_call(const char* name, const tcgnn_plan* plan, const float* d_Xw, const float* d_X, float* d_ef, int32_t D, void* ws, size_t ws_bytes, void* stream) {
    SddmmCall c;
    c.plan = plan; c.d_Xw = d_Xw; c.d_X = d_X; c.d_ef = d_ef; c.D = D; c.ws = ws; c.ws_bytes = ws_bytes; c.stream = static_cast<hipStream_t>(stream); c.name = name;
    return c;
}

int tcgnn_sddmm(const tcgnn_plan* plan, const float* d_X, float* d_ef, int32_t D, void* ws, size_t ws_bytes, void* stream_v) {
    if (!plan || D < 1 || (plan->N > 0 && !d_X) || (plan->E > 0 && !d_ef)) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_sddmm: null argument or D < 1");
    return run_sddmm(sddmm_call("tcgnn_sddmm", plan, nullptr, d_X, d_ef, D, ws, ws_bytes, stream_v));
}

size_t tcgnn_sddmm2_workspace_bytes(const tcgnn_plan* plan, int32_t D) {
    if (!plan || D < 1) return 0;
    return 2 * workspace_bytes_for(plan->Nc, D);
}

int tcgnn_sddmm2(const tcgnn_plan* plan, const float* d_X, const float* d_Z, float* d_ef, int32_t D, void* ws, size_t ws_bytes, void* stream_v) {
    if (!plan || D < 1 || (plan->N > 0 && !(d_X && d_Z)) || (plan->E > 0 && !d_ef)) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_sddmm2: null argument or D < 1");
    return run_sddmm(sddmm_call("tcgnn_sddmm2", plan, d_X, d_Z, d_ef, D, ws, ws_bytes, stream_v));
}

size_t tcgnn_sddmm_heads_workspace_bytes(const tcgnn_plan* plan, int32_t H, int32_t F) {
    if (!plan || H < 1 || F < 1 || (int64_t)H * F > INT32_MAX) return 0;
    return sddmm_heads_workspace_bytes(plan, H, F);
}

int tcgnn_sddmm_heads(const tcgnn_plan* plan, const float* d_X, const float* d_Z, float* d_ef, int32_t H, int32_t F, void* ws, size_t ws_bytes, void* stream_v) {
    SddmmHeadsCall c;
    c.plan = plan; c.d_X = d_X; c.d_Z = d_Z; c.d_ef = d_ef; c.H = H; c.F = F; c.ws = ws; c.ws_bytes = ws_bytes; c.stream = static_cast<hipStream_t>(stream_v);
    return run_sddmm_heads(c);
}

} // extern "C"
