// tcgnn_sync_walk.inc - the slice-synchronised range walk (r06): gather walks for graphs whose communities are LARGER than an XCD's L2.
// Included by tcgnn_device.hip behind tcgnn_gather_spmm.inc (TileWalker) - the SDDMM and fused-AGNN forms live in their own kernels
// (SddmmArgs::sync / AgnnArgs::sync) and share the tables built here.
// ------------------------------------------------------------------------------------------
// ogbn-products shape, 50 communities of 49 k rows, D = 128: a community's fp16 image is 12.5 MB.  The per-window walk in
// XCD-contiguous order keeps every XCD inside ONE community at a time, but each window sweeps the whole 12.5 MB while the XCD's L2
// holds 4: 27 % hits, 25.7 GB of fabric reads for 3.0 GB of algorithmic bytes (profiles/r05), 3.6 ms - although the same walk over
// communities that FIT the L2 (Reddit shape, 50 communities of 1.2 MB) gathers 256-byte rows at 28 TB/s, 9.1 ps per edge.
// The range-blocked walks of r01-r03 cut the columns into L2-sized ranges and let persistent wavefronts walk them "in step", which
// holds on a graph without locality (every window has the same share of its tiles in every range) and fails on one with it: a
// wavefront is heavy in the ranges of its own windows' community and light elsewhere, the wavefronts of different communities fall
// out of step within one group of windows, and several ranges are live at once.
//
// Here the step is kept by construction:
//   * a SLICE is S consecutive windows of one XCD's contiguous eighth of the graph (workgroup b runs on XCD b % 8 - observed, used
//     for speed only) - what the wavefronts resident on that XCD own AT ONCE.  Neighbours in the numbering: one community, or two;
//   * per slice the plan lists its HOT column buckets (fine buckets of fb_rows rows in which the slice has at least S / 4 tiles) and
//     a table T[window][k] = first tile of the window at or beyond hot bucket k.  A PHASE is m consecutive hot buckets (m from the
//     width: ~2 MB of image); the tiles between two hot buckets ride with the phase in front of them, so the phases cover every tile
//     exactly once, in the stream's own order;
//   * one LAUNCH per slice round: every wavefront of the chip starts its slice's first phase at the same moment, owns MAXW windows
//     of it (accumulators in registers, as spmm_blocked_kernel) and walks the phases; the windows of a slice are alike (same
//     community), so the wavefronts of an XCD stay inside one phase - 2 MB of rows that 1024 windows x ~120 columns each reuse 15 x -
//     until the launch ends.  The kernel boundary is the barrier: nothing inside a launch waits for another workgroup.
// No partial sums leave the registers, no atomics: as deterministic as the other walks (and bit-identical to the per-window walk
// with one wavefront per window: same tile order per window).
// ------------------------------------------------------------------------------------------
static constexpr int kSyncKmax = 64;          // hot buckets a slice may list
// windows of one XCD per launch.  Up to 64 columns its wavefronts hold them at once (32 CUs x 16 wavefronts x 2 windows = 1024: the grid
// is cut to the slice).  Beyond, 32 CUs x 8 wavefronts x 2 windows = 512 are resident and a slice round takes a second trip, a third
// filled (the figure dates from a layout of 12 wavefronts x 2 windows per CU that the kernels no longer have: ADVICE r06)
static constexpr int kSyncSlice = 768;
static constexpr int kSyncFbShift0 = 11;      // finest bucket: 2048 rows

struct SyncArgs {
    const uint32_t* T;      // [nw][kmax + 1] per window: tile offset of the first tile at or beyond hot bucket k of the window's slice (k >= the slice's count: all of them)
    const int32_t* nk;      // [8 * R] hot buckets of slice (x, round)
    int32_t kmax, m;        // m: hot buckets per phase
    int32_t S, R, nwx;      // windows per slice, slices per XCD, windows per XCD share
    int32_t round;          // the slice of every XCD's share this launch covers
    int32_t nw;
};
struct SpmmSyncArgs {
    SpmmArgs base;
    SyncArgs s;
};

__device__ __forceinline__ void sync_slice_of(const SyncArgs& s, int& x, int& w_lo, int& w_hi, int& nph) {
    x = (int)(blockIdx.x % (unsigned)kXcds);
    const int64_t share_hi = (int64_t)(x + 1) * s.nwx < (int64_t)s.nw ? (int64_t)(x + 1) * s.nwx : (int64_t)s.nw;
    const int64_t lo = (int64_t)x * s.nwx + (int64_t)s.round * s.S;
    w_lo = (int)(lo < share_hi ? lo : share_hi);
    w_hi = (int)(lo + s.S < share_hi ? lo + s.S : share_hi);
    const int k = s.nk[x * s.R + s.round];
    nph = k <= s.m ? 1 : (k + s.m - 1) / s.m;
}

// spmm_sync_kernel's launch geometry.  Tile buffers per wavefront: two up to 32 columns; beyond, ONE and a run list - the kernel walks
// its runs as one pipeline (TileWalker::walk_list).  A wavefront owns 2 windows at every width (three spilled 34-44 words at 128
// columns).  Four wavefronts per SIMD up to 64 columns, two beyond: walk_list's three list cursors want the 256 registers.
static constexpr int sync_nbuf(int nt) { return nt <= 2 ? 2 : 1; }
static constexpr LaunchGeom sync_geom(int nt, bool val) { return {256, 4 * tile_wave_lds(nt, val, sync_nbuf(nt)) + 4096, nt <= 4 ? 4 : 2, 2}; }
// (pinned: resident workgroups per CU at 1 .. 8 tiles of width)
static_assert(widths_give([](int nt) { return sync_geom(nt, false).wgs_per_cu(); }, {4, 4, 4, 4, 2, 2, 2, 2}), "spmm_sync_kernel, binary A");
static_assert(widths_give([](int nt) { return sync_geom(nt, true).wgs_per_cu(); }, {4, 4, 4, 4, 2, 2, 2, 2}), "spmm_sync_kernel, edge values");
#define TCGNN_KERNEL_NAME spmm_sync_kernel
#define TCGNN_KERNEL_PARAM const SpmmSyncArgs b
#define TCGNN_KERNEL_PROLOGUE
#define TCGNN_KERNEL_STORE(relu, row, col, v) relu_if(relu, v)
#include "tcgnn_sync_kernel.inc"
#undef TCGNN_KERNEL_NAME
#undef TCGNN_KERNEL_PARAM
#undef TCGNN_KERNEL_PROLOGUE
#undef TCGNN_KERNEL_STORE
// tcgnn_spmm_scaled on this walk (binary A only: VAL = false)
struct SpmmSyncEpiArgs { SpmmSyncArgs b; Epi epi; };
#define TCGNN_KERNEL_NAME spmm_sync_epi_kernel
#define TCGNN_KERNEL_PARAM const SpmmSyncEpiArgs e
#define TCGNN_KERNEL_PROLOGUE const SpmmSyncArgs& b = e.b;
#define TCGNN_KERNEL_STORE(relu, row, col, v) epi_apply(relu, e.epi, row, col, v)
#include "tcgnn_sync_kernel.inc"
#undef TCGNN_KERNEL_NAME
#undef TCGNN_KERNEL_PARAM
#undef TCGNN_KERNEL_PROLOGUE
#undef TCGNN_KERNEL_STORE

template <int NT, bool VAL>
static hipError_t launch_sync_one(const SpmmSyncArgs& args, int nwg, int nchunks, hipStream_t stream, const Epi& epi) {
    constexpr LaunchGeom g = sync_geom(NT, VAL);
    constexpr int NBUF = sync_nbuf(NT);
    const dim3 grid((unsigned)nwg, (unsigned)nchunks);
    if constexpr (VAL) return launch_kernel<spmm_sync_kernel<NT, g.maxw, true, NBUF>>(grid, g, stream, args);
    else return launch_plain_or_twin<spmm_sync_kernel<NT, g.maxw, false, NBUF>, spmm_sync_epi_kernel<NT, g.maxw, false, NBUF>>(grid, g, stream, args, epi);
}
static hipError_t launch_sync_any(bool val, int nt, const SpmmSyncArgs& args, int nwg, int nchunks, hipStream_t stream, const Epi& epi) {
    return with_width<8>(nt, [&](auto NT) {
        return val ? launch_sync_one<NT, true>(args, nwg, nchunks, stream, epi) : launch_sync_one<NT, false>(args, nwg, nchunks, stream, epi);
    });
}

// ---- plan-time tables -----------------------------------------------------------------------
// tiles of every slice per fine bucket (bucket of a tile = that of its first column: the stream is sorted by column inside a window)
__global__ __launch_bounds__(64) void sync_hist_kernel(const int64_t* __restrict__ wb_ptr, const int32_t* __restrict__ cols, int32_t nw, int32_t nwx, int32_t S,
                                                      int32_t R, int32_t fb_shift, int32_t nfb, uint32_t* __restrict__ hist) {
    const int w = (int)blockIdx.x;
    if (w >= nw) return;
    const int x = w / nwx, slice = x * R + (w - x * nwx) / S;
    const int64_t tb = wb_ptr[w], te = wb_ptr[w + 1];
    for (int64_t t = tb + threadIdx.x; t < te; t += 64) {
        int b = cols[t * kWbCols] >> fb_shift;
        if (b >= nfb) b = nfb - 1;
        atomicAdd(hist + (int64_t)slice * nfb + b, 1u);
    }
}
// T[w][k]: 0 for k = 0; the first tile whose first column lies at or beyond the start of hot bucket k of the window's slice; every tile for k >= the slice's count
__global__ void sync_table_kernel(const int64_t* __restrict__ wb_ptr, const int32_t* __restrict__ cols, int32_t nw, int32_t nwx, int32_t S, int32_t R, int32_t kmax,
                                  int32_t fb_shift, const int32_t* __restrict__ hot, const int32_t* __restrict__ nk, uint32_t* __restrict__ T) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)nw * (kmax + 1)) return;
    const int w = (int)(idx / (kmax + 1)), k = (int)(idx % (kmax + 1));
    const int x = w / nwx, slice = x * R + (w - x * nwx) / S;
    const int64_t tb = wb_ptr[w];
    const int64_t n = wb_ptr[w + 1] - tb;
    int64_t lo = 0, hi = n;
    if (k == 0) hi = 0;
    else if (k >= nk[slice]) lo = n;
    else {
        const int64_t first_col = (int64_t)hot[slice * kmax + k] << fb_shift;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)cols[(tb + mid) * kWbCols] >= first_col) hi = mid; else lo = mid + 1;
        }
    }
    T[idx] = (uint32_t)lo;
}
