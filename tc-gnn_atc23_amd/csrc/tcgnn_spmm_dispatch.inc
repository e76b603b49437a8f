// tcgnn_spmm_dispatch.inc - host side of every SpMM call: the request (SpmmCall), the one routing decision (route_spmm: DESIGN.md
// sections 5 and 4.4 are applied here and nowhere else), the lazy stream builds it relies on, one launcher per walk, run_spmm.
// Included by tcgnn_device.hip.  tcgnn_workspace_bytes, tcgnn_plan_prepare[_val] and tcgnn_spmm_staged_layout ask the same
// predicates (lds_wanted, lds_streams_serve, val_lds_wanted, ensure_*), so what they answer is what run_spmm will do.
// columns one gather-walk launch may cover: the widest row whose pitch the structured descriptor can express, in whole
// 128-column chunks.  Wider matrices go through the gather walks as independent column blocks (ld = the full row length).
static constexpr int kMaxGatherBlockDims = 4096;

// tcgnn_spmm_scaled: the column scale enters the staging pass (and the kernels that read fp32 X), the row scale and bias the final store
struct Scales { const float* col = nullptr; const float* row = nullptr; const float* bias = nullptr; };
// an image the caller staged itself (tcgnn_spmm_staged: row-major, the gather walks; tcgnn_spmm_staged_planar, r06: the LDS-resident kernel's)
enum class StagedLayout { kNone, kRowMajor, kPlanar };
// One SpMM call as the C ABI's entry points (and the column-block recursion) describe it; every field is named where it is set.
struct SpmmCall {
    const tcgnn_plan* plan = nullptr;
    const float *d_X = nullptr, *d_val = nullptr, *d_gate = nullptr;   // d_val: edge values (null: binary A)
    float* d_Y = nullptr;
    int32_t D = 0, relu = 0;
    void* ws = nullptr; size_t ws_bytes = 0;
    hipStream_t stream = nullptr;
    const void* d_image = nullptr; StagedLayout staged = StagedLayout::kNone;
    // ld > 0: X (and the gate, and Y) is a column block of a wider row-major matrix with that row stride; the scale words in the
    // header were then computed over the WHOLE matrix by the caller (block_of_wider)
    int64_t ld = 0; bool block_of_wider = false;
    const float* d_W = nullptr; int32_t D_out = 0;   // tcgnn_spmm_gemm's fused dense update
    Scales sc;
    bool scaled() const { return sc.col || sc.row || sc.bias; }
    Epi epi() const { return Epi{sc.row, sc.bias}; }
    int64_t stride() const { return ld ? ld : D; }
    int dpad() const { return round_up(D, 16); }
};
// no staging: kValCsr (edge values on a non-canonical or tiny CSR), kSmall (single-launch fp32 MFMA on fp32 X), kColumnBlocks (run_spmm per
// block of kMaxGatherBlockDims columns); LDS-resident: kLds, kValLds (edge values); gather: kValSliced (edge values on the fused AGNN
// kernel's XCD-sliced walk), kSync (slice-synchronised), kBlocked (range-blocked), kPerWindow
enum class Walk { kValCsr, kSmall, kColumnBlocks, kLds, kValLds, kValSliced, kSync, kBlocked, kPerWindow };
struct SpmmRoute {
    Walk walk = Walk::kPerWindow;
    LdsPass passes[2]; int npass = 0;                  // kLds
    const tcgnn_plan::CellStream* cold = nullptr;      // kLds: the ordinary stream whose remainder spmm_kernel ADDS from a second, row-major image
    bool own_fb = false;                               // kLds: the kernel is its own range-guard fallback (no launch behind it)
    int accumulate = 0;                                // kLds + dense update over more than one column chunk: Y is zeroed, passes add
    int nslices = 0;                                   // kValSliced
    bool planar() const { return walk == Walk::kLds || walk == Walk::kValLds; }
};
// ---- the parts of the decision that read only plan facts, mode and width (tcgnn_workspace_bytes may ask them: nothing is built,
// allocated or synchronised; lds_chosen caching its answer in lds_choice is the one write)
static bool lds_wanted(const tcgnn_plan* plan, int mode, int dpad) { return plan->nw_eff > 0 && (mode == 3 || (mode == 0 && lds_chosen(plan, dpad))); }
// (the planar image is addressed as planes * rows 32-byte records through one buffer descriptor: records * 32 B inside its 32-bit offset)
static bool planar_records_fit(const tcgnn_plan* plan, int dpad) { return (int64_t)(dpad / 16) * ((int64_t)plan->Nc + 1) * 32 < ((int64_t)1 << 32); }
// widths the LDS-resident edge-valued walk covers: whole 64-column chunks of a canonical plan whose planar image one descriptor addresses -
// and, r05, a remainder of THREE planes (Reddit's 41 classes), which goes as one more pair of 32-column chunks with the fourth plane filled
// with zeros, exactly as the binary walk takes it (lds_passes): 0.85 against the gather walk's 1.48 ms on the calibrated SBM graph
static bool val_lds_width(int dp) { return (dp % 64 == 0 || dp % 64 == 48) && dp <= 2 * kMaxChunkDims; }
static bool val_lds_width_ok(const tcgnn_plan* plan, int dp) { return val_lds_width(dp) && plan->canonical && plan->nw_eff > 0 && planar_records_fit(plan, dp); }
// ... on graphs the binary SpMM's time model sends to the LDS-resident kernel
static bool val_lds_wanted(const tcgnn_plan* plan, int mode, int dp) { return (mode == 0 || mode == 3) && val_lds_width_ok(plan, dp) && (mode == 3 || lds_chosen(plan, dp)); }
// automatic mode gives up the LDS-resident kernel for this width: later calls - and tcgnn_workspace_bytes, which reserves a second image
// for LDS-chosen widths - stop coming back (ADVICE r02)
static void settle_on_gather_walks(const tcgnn_plan* plan, int dpad) { if (dpad / 16 <= 64) plan->lds_choice[dpad / 16] = 0; }
// a flat stream whose remainder spmm_cold_planar_kernel adds behind it from the planar image (one multiplied inside the flat kernel,
// d_wcold_ptr, needs nothing from the dispatcher)
static bool flat_cold_behind(const tcgnn_plan::CellStream& cs) { return cs.flat_tpc && cs.cold_tiles > 0 && !cs.d_wcold_ptr; }
// What the BUILT streams of a width's passes say (streams not built yet say nothing and clear all_built).
struct LdsStreamFacts { bool all_built, rows_cold, flat_cold, thin; };
static LdsStreamFacts lds_stream_facts(const tcgnn_plan* plan, const LdsPass* passes, int npass) {
    LdsStreamFacts f{npass > 0, false, false, false};
    for (int i = 0; i < npass; ++i) {
        const tcgnn_plan::CellStream& ci = plan->lds[lds_pass_slot(plan, passes[i])];
        if (ci.nranges == 0) { f.all_built = false; continue; }
        // (a flat stream's remainder is added per pass from the planar image by spmm_cold_planar_kernel: no second image, any
        //  number of passes - but not under the fused dense update, which needs the whole sum before it multiplies)
        if (ci.flat_tpc) f.flat_cold = f.flat_cold || flat_cold_behind(ci);
        else f.rows_cold = f.rows_cold || ci.cold_tiles > 0;
        f.thin = f.thin || ci.hot_cols * 2 < ci.hot_cols + ci.cold_cols;
    }
    return f;
}
// ---- a plan with locality: the (workgroup, range) pairs too thin for a range fill were left out of the cell stream and sit
//      in a re-condensed remainder that the gather walk ADDS afterwards.  One stream must serve every pass of the call (the
//      remainder is per stream), the fused dense update cannot span two kernels, and a stream that kept less than half of the
//      columns is not worth its range fills at all.
// Do the built streams serve this call?  *settle: the answer holds for every later call of the width in automatic mode (the caller
// stores it; a query - tcgnn_spmm_staged_layout - settles nothing).  *cold: the stream whose remainder wants a row-major image.
static bool lds_streams_serve(const tcgnn_plan* plan, int mode, const LdsPass* passes, int npass, bool dense_update, bool planar_staged, bool* settle,
                              const tcgnn_plan::CellStream** cold) {
    const LdsStreamFacts f = lds_stream_facts(plan, passes, npass);
    *settle = false; *cold = nullptr;
    if ((f.rows_cold && (npass > 1 || dense_update)) || (f.flat_cold && dense_update)) {
        *settle = f.rows_cold && npass > 1 && mode != 3;   // (a width whose passes can never share one remainder)
        return false;
    }
    if (f.thin && mode != 3) { *settle = true; return false; }
    if (f.rows_cold && planar_staged) return false;   // (the remainder's gather walk wants a row-major image of the same matrix: not in a planar staged call)
    if (f.rows_cold) *cold = &plan->lds[lds_pass_slot(plan, passes[0])];
    return true;
}
// ---- lazy stream builds (allocate and synchronise the stream once)
static bool stream_is_capturing(hipStream_t stream) {
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(stream, &capturing) == hipSuccess && capturing != hipStreamCaptureStatusNone;
}
// Every (layout, pass width) has its own cell stream, built the first time it is needed (plan creation builds the one a 64-column
// matrix uses).  A failed build: the forced mode reports the error; automatic mode settles the width on the gather walks, which need
// no stream (e.g. no memory left for it).  *ok: every pass has its stream.  Who asks:
enum class LdsBuild {
    kInCall,    // run_spmm: a stream that is being captured into a HIP graph cannot allocate or synchronise - this call takes the gather
                // walks (nothing is remembered: the next call outside a capture builds the cell stream); stops at the first failure
    kPrepare,   // tcgnn_plan_prepare: called outside a capture by contract (no test); after a failure in automatic mode it still builds
                // the other pass's stream (looks like drift from kInCall, kept: the plan's memory afterwards is observable)
    kQuery      // tcgnn_spmm_staged_layout: a failure only answers "no" - nothing reported, nothing settled (no capture test either)
};
static int ensure_lds_streams(const tcgnn_plan* plan, hipStream_t stream, int mode, int dpad, const LdsPass* passes, int npass, LdsBuild who, bool* ok) {
    *ok = true;
    for (int i = 0; i < npass; ++i) {
        if (plan->lds[lds_pass_slot(plan, passes[i])].nranges > 0) continue;
        // (whole 64-column chunks: the build decides between the 760- and the 952-row stream the first time and builds that one - lds_pass_slot follows)
        const int slot = lds_stream_of(passes[i].nt, passes[i].maxw);
        if (who == LdsBuild::kInCall && stream_is_capturing(stream)) {
            *ok = false;
            return mode == 3 ? fail(TCGNN_ERR_INVALID_ARG, "LDS-resident SpMM: the cell stream of this width has to be built before the call is captured into a graph") : TCGNN_OK;
        }
        const int b = build_lds_cells(const_cast<tcgnn_plan*>(plan), stream, slot);
        if (!b) continue;
        *ok = false;
        if (who == LdsBuild::kQuery) return TCGNN_OK;
        if (mode == 3) return b;
        settle_on_gather_walks(plan, dpad);
        if (who == LdsBuild::kInCall) return TCGNN_OK;
    }
    return TCGNN_OK;
}
// The single-edge stream of the edge-valued walk, tried once per plan (val_choice).  in_call: never inside a graph capture.
// (ADVICE r04: the stream is an optional acceleration - in automatic mode a failed build, e.g. no memory for its 0.9 GB of temporaries,
//  settles the plan on the gather walks, as the binary path does; only the forced mode reports it)
static int ensure_val_stream(const tcgnn_plan* plan, hipStream_t stream, int mode, bool in_call) {
    if (plan->val_choice.load(std::memory_order_acquire) >= 0 || (in_call && stream_is_capturing(stream))) return TCGNN_OK;
    const int b = build_val_stream(const_cast<tcgnn_plan*>(plan), stream);
    if (b && mode == 3) return b;
    if (b) const_cast<tcgnn_plan*>(plan)->val_choice.store(0, std::memory_order_release);
    return TCGNN_OK;
}
// ---- the routing decision: which walk runs for this call and what it runs with.  Builds the streams the walk needs first - before
// the staging pass, which lays the image out for the kernel that will run, and before any timer starts.
static int route_spmm(const SpmmCall& c, SpmmRoute* r) {
    const tcgnn_plan* const plan = c.plan;
    const int32_t D = c.D;
    const int dpad = c.dpad();
    const bool staged = c.staged != StagedLayout::kNone, planar_staged = c.staged == StagedLayout::kPlanar;
    if (c.d_val && (!plan->canonical || plan->E < 4)) { r->walk = Walk::kValCsr; return TCGNN_OK; }
    const int mode = spmm_mode_of(plan); // 0 auto, 1 plain, 2 blocked, 3 LDS-resident ranges, 4 single-launch fp32 kernel, 5 slice-synchronised
    // (a staged call never takes the small kernel: it has no fp32 X)
    if (!c.d_val && !staged && !c.d_W && plan->nw_eff > 0 && (mode == 4 || (mode == 0 && plan->total_wb <= kSmallMaxTiles))) { r->walk = Walk::kSmall; return TCGNN_OK; }
    // (a caller-staged image is row-major - the gather walks - unless it was staged PLANAR for this kernel)
    bool lds = !c.d_val && (!staged || planar_staged) && !c.block_of_wider && lds_wanted(plan, mode, dpad) && planar_records_fit(plan, dpad);
    // f3 on the LDS-resident kernel: one pass stores its product, the two 32-column passes of a 64-column matrix ADD theirs into a
    // zeroed Y (two addends: the sum does not depend on their order); wider inputs would need an ordered reduction - gather walk
    if (lds && c.d_W && !(dpad <= 64 && !g_lds_maxw)) lds = false;
    if (lds) {
        r->npass = lds_passes(dpad, r->passes);
        if (const int rc = ensure_lds_streams(plan, c.stream, mode, dpad, r->passes, r->npass, LdsBuild::kInCall, &lds)) return rc;
    }
    if (lds) {
        bool settle;
        lds = lds_streams_serve(plan, mode, r->passes, r->npass, c.d_W != nullptr, planar_staged, &settle, &r->cold);
        if (settle) settle_on_gather_walks(plan, dpad);
    }
    if (planar_staged && !lds)
        return fail(TCGNN_ERR_UNSUPPORTED, "tcgnn_spmm_staged_planar: the LDS-resident kernel does not take this plan at %d columns (tcgnn_spmm_staged_layout tells; stage row-major and call tcgnn_spmm_staged)", D);
    if (lds) {
        int total_chunks = 0;
        for (int i = 0; i < r->npass; ++i) total_chunks += r->passes[i].nchunks;
        r->accumulate = (c.d_W && total_chunks > 1) ? 1 : 0;
        // one launch, binary A, whole rows, nothing added behind it: the kernel is its own range-guard fallback (lds_own_fallback)
        r->own_fb = r->npass == 1 && !r->cold && !c.d_W && !staged && c.stride() == D && !flat_cold_behind(plan->lds[lds_pass_slot(plan, r->passes[0])]) &&
                    !c.scaled();   // (a scaled call's fallback is the scaled fp32 kernel behind the launch)
        r->walk = Walk::kLds;
        return TCGNN_OK;
    }
    if (!pitch_fits_descriptor(D)) {
        // a row too long for the gather walks' buffer descriptor (ADVICE r1): independent column blocks
        if (staged) return fail(TCGNN_ERR_UNSUPPORTED, "tcgnn_spmm_staged: rows of %d columns exceed the %d-byte descriptor stride", D, kMaxStructStride);
        if (c.block_of_wider) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_spmm: nested column blocks");
        r->walk = Walk::kColumnBlocks;
        return TCGNN_OK;
    }
    const bool plain_val = c.d_val && !staged && !c.block_of_wider && !c.d_gate && !c.relu;   // (what the two edge-valued special walks take)
    // ---- edge values on the LDS-resident flat walk (r04, tcgnn_lds_val.inc): whole 64-column chunks, on graphs the binary SpMM's
    //      time model sends to the LDS-resident kernel, canonical CSR (the single-edge stream is cut with the packed edge offsets).
    //      The first such call builds the stream (unless it is being captured into a graph) and still takes a gather walk - its
    //      workspace was sized before the stream existed; later calls find tcgnn_workspace_bytes grown by the slot values.
    if (plain_val && !c.d_W && val_lds_wanted(plan, mode, dpad)) {
        if (const int rc = ensure_val_stream(plan, c.stream, mode, true)) return rc;
        if (plan->val_choice.load(std::memory_order_acquire) == 1 && c.ws_bytes >= workspace_bytes_for(plan->Nc, D) + val_stream_bytes(plan)) { r->walk = Walk::kValLds; return TCGNN_OK; }
    }
    // ---- edge values on the fused AGNN kernel's XCD-sliced walk (r03).  Where the fused pair's backward pass takes that walk (graphs
    //      without locality of their own, windows alike, an fp16 image of 16 - 64 MB: agnn_plan_walk) the edge-valued SpMM is the same
    //      gather with less to do per tile, so it runs as that kernel with the score half switched off (AgnnArgs::valonly: w = 1,
    //      ef = the caller's values, their abs-max from this call's header): 76 % L2 hits and 5.8 GB of fabric reads instead of the
    //      per-window walk's 31 % and 12.2 GB on the Reddit shape at D = 64.  Same operand rounding and scales; the sums run in slice order.
    if (plain_val && plan->nw_eff > 0 && mode == 0 && dpad > 32 && dpad <= kMaxChunkDims && agnn_supported(plan, D)) {
        const size_t need = workspace_bytes_for(plan->Nc, D) + agnn_partial_bytes(plan) + agnn_slice_bytes(plan, D);
        const AgnnRoute bw = agnn_plan_walk(plan, D, true);
        if (bw.walk == AgnnWalk::kSliced && bw.nslices > 0 && c.ws_bytes >= need) { r->nslices = bw.nslices; r->walk = Walk::kValSliced; return TCGNN_OK; }
    }
    const int pitch = x16_pitch(dpad);
    // slice-synchronised range walk (r06, tcgnn_sync_walk.inc): communities larger than an XCD's L2
    if (plan->nw_eff > 0 && !c.d_W && !image_is_big(plan->Nc, pitch) && sync_chosen(plan, pitch * 2, mode, c.d_val ? kSyncVal : kSyncSpmm, dpad / 16)) { r->walk = Walk::kSync; return TCGNN_OK; }
    // range-blocked walk when the fp16 image of X overflows L2 and the windows are long enough to cut
    const size_t x16_bytes = image_bytes(plan, pitch);
    // (a numbering with locality keeps the per-window walk: in XCD-contiguous order its co-resident workgroups share their gathered
    //  rows in L2 - 50-community Reddit shape, edge values: 0.92 ms against 1.18 ms range-blocked; the range-blocked walk is for
    //  graphs without it, where it wins by 1.4x)
    // (edge values: two windows per wavefront instead of four; at Reddit's 30 MB image the per-window walk in contiguous order is
    //  6 % faster - 1.70 against 1.79 ms per call - so only images beyond the Infinity Cache's reach)
    const bool blocked = !c.d_W && plan->nbuckets > 0 && mode != 1 && (mode == 2 || (range_walk_pays(plan, x16_bytes) && (!c.d_val || x16_bytes > ((size_t)64 << 20))));
    r->walk = blocked ? Walk::kBlocked : Walk::kPerWindow;
    return TCGNN_OK;
}
// ---- kernel arguments: every builder names each field it sets; what is not named is zero
static SpmmSmallArgs small_args(const SpmmCall& c, const uint32_t* guard_hdr) {
    const tcgnn_plan* const plan = c.plan;
    SpmmSmallArgs a{};
    a.wb_ptr = plan->d_wb_ptr; a.cols = plan->d_cols; a.mask = plan->d_mask; a.x = c.d_X; a.gate = c.d_gate; a.y = c.d_Y;
    a.N = plan->N; a.Nc = plan->Nc; a.D = c.D; a.relu = c.relu; a.nw = plan->nw_eff; a.guard = guard_hdr;
    return a;
}
// the plan's tile stream over a row-major image: what the gather walks, the cold remainder of an ordinary cell stream and the fused
// multi-head walk start from (whole rows of Y, binary A, no epilogue - each sets the rest)
static SpmmArgs spmm_args(const tcgnn_plan* plan, const StagedImage& im, float* d_Y, int32_t D) {
    SpmmArgs a{};
    a.wb_ptr = plan->d_wb_ptr; a.order = plan->d_order; a.cols = plan->d_cols; a.mask = plan->d_mask; a.ebase = plan->d_ebase;
    a.x16 = im.x16; a.hdr = im.hdr; a.y = d_Y;
    a.N = plan->N; a.D = D; a.stride = im.pitch; a.E = plan->E; a.xrows = plan->Nc + 1; a.ldy = D;
    a.big = image_is_big(plan->Nc, im.pitch);
    return a;
}
// dpad columns as whole 128-column chunks, then one launch for the remainder: launch(tiles of width, first chunk, chunks)
template <class F>
static int for_column_chunks(int dpad, F&& launch) {
    const int nfull = dpad / kMaxChunkDims, rem = (dpad % kMaxChunkDims) / 16;
    if (nfull) HIP_TRY(launch(8, 0, nfull));
    if (rem) HIP_TRY(launch(rem, nfull, 1));
    return TCGNN_OK;
}
// ---- launchers: one per walk, each given the call, its route and the staged image
static void launch_small_pair(const SpmmCall& c, unsigned grid_x, const uint32_t* guard_hdr) {   // (guard_hdr: as the range guard's fallback - returns at once unless wide)
    const SpmmSmallArgs sa = small_args(c, guard_hdr);
    const dim3 grid(grid_x, (unsigned)((c.D + 63) / 64));
    if (c.scaled()) hipLaunchKernelGGL(spmm_small_scaled_kernel, grid, dim3(64), 0, c.stream, SpmmSmallScaledArgs{sa, c.sc.col, c.epi()});
    else hipLaunchKernelGGL(spmm_small_kernel, grid, dim3(64), 0, c.stream, sa);
}
// the range guard's fallback, launched behind the fp16-path kernels of this call (returns at once unless the staged matrix is
// "wide": range_is_wide).  An image the caller staged itself carries no range words: no guard.
static int launch_wide_fallback(const SpmmCall& c, const StagedImage& im) {
    const tcgnn_plan* const plan = c.plan;
    if (c.d_image) return TCGNN_OK;
    const int32_t D = c.D;
    const int64_t ld = c.stride();
    const unsigned grid = (unsigned)std::min<int64_t>(((int64_t)plan->N + 3) / 4, 4096);
    if (c.d_W) hipLaunchKernelGGL(spmm_gemm_wide_fallback_kernel, dim3(grid), dim3(256), 0, c.stream, im.hdr, plan->rowptr, plan->col, c.d_X, c.d_W, c.d_Y, plan->N, D, c.D_out, c.relu);
    else if (!c.d_val && ld == D) launch_small_pair(c, (unsigned)std::min(plan->nw_eff, 2048), im.hdr);   // binary A, whole rows: the fp32-MFMA walk small graphs take anyway (10-bit operands, fp32's exponent)
    else if (c.scaled()) hipLaunchKernelGGL(spmm_wide_fallback_scaled_kernel, dim3(grid), dim3(256), 0, c.stream, im.hdr, plan->rowptr, plan->col, c.d_X, c.d_gate, c.sc.col, c.epi(), c.d_Y,
                                            plan->N, D, ld, ld, c.relu, plan->canonical ? 0 : 1);
    else hipLaunchKernelGGL(spmm_wide_fallback_kernel, dim3(grid), dim3(256), 0, c.stream, im.hdr, c.d_val ? 1 : 0, plan->rowptr, plan->col, c.d_val, (const float*)nullptr, c.d_X, c.d_gate, c.d_Y,
                            plan->N, D, ld, ld, c.relu, (!c.d_val && !plan->canonical) ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}
static int run_spmm(const SpmmCall& c);
// every block rounded with the scale of the whole matrix (absmax over all of X / the edge values here, once)
static int run_column_blocks(const SpmmCall& c) {
    const tcgnn_plan* const plan = c.plan;
    if (const int rc = check_workspace("staging", c.ws, c.ws_bytes, workspace_bytes_for(plan->Nc, c.D))) return rc;
    if (const int rc = fill_header(plan, static_cast<uint32_t*>(c.ws), c.d_X, c.d_gate, c.sc.col, c.D, guard_spmm(plan), c.d_val, plan->E, c.stream)) return rc;
    for (int c0 = 0; c0 < c.D; c0 += kMaxGatherBlockDims) {
        SpmmCall b = c;
        b.d_X = c.d_X + c0; b.d_Y = c.d_Y + c0; b.D = std::min(kMaxGatherBlockDims, c.D - c0);
        if (c.d_gate) b.d_gate = c.d_gate + c0;
        if (c.sc.bias) b.sc.bias = c.sc.bias + c0;
        b.ld = c.D; b.block_of_wider = true;
        if (const int rc = run_spmm(b)) return rc;
    }
    return TCGNN_OK;
}
static int launch_val_lds(const SpmmCall& c, const StagedImage& im) {
    const tcgnn_plan* const plan = c.plan;
    hipStream_t stream = c.stream;
    const tcgnn_plan::CellStream& cs = plan->lds[kLdsValSlot];
    const size_t image = workspace_bytes_for(plan->Nc, c.D);
    _Float16* const vals = reinterpret_cast<_Float16*>(static_cast<char*>(c.ws) + image);
    _Float16* const cvals = vals + (size_t)std::max<int64_t>(cs.tiles, 1) * 32;
    KernelTimer timer(plan, stream, cs.cold_tiles > 0 ? "val_permute_kernel + spmm_lds_val_kernel + spmm_cold_val_kernel (cold remainder)" : "val_permute_kernel + spmm_lds_val_kernel");
    constexpr LaunchGeom permute{kValThreads, kValSpanHalves * 2, 0, 0};
    HIP_TRY((launch_kernel<val_permute_kernel, permute.lds_bytes>(dim3((unsigned)(cs.nwg * kLdsWaves * (kLdsMaxW2 / kValWpb))), permute, stream, c.d_val, plan->rowptr, cs.d_order, cs.d_eidx16, cs.d_rbase, im.hdr,
                                                                 vals, plan->N, cs.cold_tiles > 0 ? cs.d_cold_ptr : nullptr, cs.d_cold_eidx16, cvals, cs.d_rl2, cs.dense_entries > 0 ? 1 : 0, std::max(cs.npairs, 1))));
    SpmmValArgs va{};
    va.blocks = cs.d_flat; va.vals = vals; va.order = cs.d_order; va.x16 = im.x16; va.hdr = im.hdr; va.y = c.d_Y;
    va.N = plan->N; va.D = c.D; va.stride = im.dpad / 16; va.xrows = plan->Nc + 1; va.nw = plan->nw_eff; va.nwg = cs.nwg;
    va.rbase = cs.d_rbase; va.rl2 = cs.d_rl2; va.nent = std::max(cs.npairs, 1);
    HIP_TRY(launch_lds_val(va, (im.dpad + 31) / 32, stream));   // (a three-plane remainder: its last chunk's second plane lies beyond the matrix - zeros)
    if (cs.cold_tiles > 0) {
        ColdValArgs ca{};
        ca.cold_ptr = cs.d_cold_ptr; ca.ccols = cs.d_cold_cols; ca.cmask = cs.d_cold_mask; ca.cvals = cvals; ca.x16 = im.x16; ca.hdr = im.hdr; ca.y = c.d_Y;
        ca.N = plan->N; ca.D = c.D; ca.xrows = plan->Nc + 1; ca.nw = plan->nw_eff; ca.ncols = im.dpad;
        hipLaunchKernelGGL(spmm_cold_val_kernel, dim3((unsigned)((plan->nw_eff + 3) / 4), (unsigned)((im.dpad + 63) / 64)), dim3(256), 0, stream, ca);
        HIP_TRY(hipGetLastError());
    }
    return TCGNN_OK;
}
// the remainder of an ordinary stream: spmm_kernel over the re-condensed cold tiles, adding into what the LDS-resident kernel stored
static int launch_cold_rows(const SpmmCall& c, const tcgnn_plan::CellStream* cold, const StagedImage& im, const _Float16* x16_rows) {
    const tcgnn_plan* const plan = c.plan;
    const int pitch_r = x16_pitch(im.dpad);
    // (the per-tile metadata DMA fetches 16 edge-offset words too; binary SpMM never looks at them: the mask array stands in)
    SpmmArgs a = spmm_args(plan, im, c.d_Y, c.D);
    a.wb_ptr = cold->d_cold_ptr; a.cols = cold->d_cold_cols; a.mask = cold->d_cold_mask; a.ebase = reinterpret_cast<const int32_t*>(cold->d_cold_mask);
    a.x16 = x16_rows; a.stride = pitch_r; a.big = image_is_big(plan->Nc, pitch_r); a.relu = c.relu; a.accumulate = 1;
    constexpr int cold_w4 = 48;   // tiles per window from which 4 wavefronts share it (SBM Reddit shape, 25 cold tiles per window: 169 us with one wavefront, 202 with four)
    // (and a window with hundreds of cold tiles - a hub - is 0.25 us per tile of serial work for one wavefront)
    const int waves = (cold->cold_tiles >= (int64_t)cold_w4 * plan->nw_eff || cold->cold_max >= 512) ? 4 : 1;
    return for_column_chunks(im.dpad, [&](int nt, int chunk0, int nchunks) {
        a.chunk0 = chunk0;
        return launch_spmm_any(false, waves, nt, a, plan->nw_eff, nchunks, c.stream, c.epi());
    });
}
static int launch_lds(const SpmmCall& c, const SpmmRoute& r, const StagedImage& im) {
    const tcgnn_plan* const plan = c.plan;
    hipStream_t stream = c.stream;
    const int32_t D = c.D;
    const Epi epi = c.epi(), no_epi{nullptr, nullptr};
    if (r.accumulate) {
        if (c.relu) return fail(TCGNN_ERR_UNSUPPORTED, "tcgnn_spmm_gemm: ReLU cannot be fused when the product is accumulated over column passes");
        HIP_TRY(hipMemsetAsync(c.d_Y, 0, (size_t)plan->N * c.D_out * sizeof(float), stream));
    }
    const _Float16* x16_rows = nullptr;
    if (r.cold) {   // the remainder's gather walk reads the row-major image: staged behind the planar one, with its scale words
        const size_t image = workspace_bytes_for(plan->Nc, D);
        if (c.ws_bytes < 2 * image) return fail(TCGNN_ERR_WORKSPACE, "tcgnn_spmm: a plan with a cold remainder stages two images: %zu bytes, got %zu", 2 * image, c.ws_bytes);
        StageOpts o; o.d_gate = c.d_gate; o.hdr_from = im.hdr; o.d_cs = c.sc.col;
        StagedImage rows;
        if (const int rc = stage_features(plan, c.d_X, nullptr, D, static_cast<char*>(c.ws) + image, c.ws_bytes - image, stream, o, &rows)) return rc;
        x16_rows = rows.x16;
    }
    const tcgnn_plan::CellStream& cs0 = plan->lds[lds_pass_slot(plan, r.passes[0])];
    const SpmmSmallArgs fb = small_args(c, r.own_fb ? im.hdr : nullptr);
    KernelTimer timer(plan, stream, r.cold ? "spmm_lds_kernel + spmm_kernel (cold remainder)" :
                                    (cs0.flat_tpc ? (flat_cold_behind(cs0) ? "spmm_lds_flat_kernel + spmm_cold_planar_kernel (cold remainder)" : "spmm_lds_flat_kernel") : "spmm_lds_kernel"));   // (the long walk, 952-row ranges, reports the family's name too)
    for (int i = 0; i < r.npass; ++i) {
        const LdsPass& p = r.passes[i];
        const int slot = lds_pass_slot(plan, p);
        const tcgnn_plan::CellStream& cs = plan->lds[slot];
        if (cs.flat_tpc) {
            const bool has_cold = flat_cold_behind(cs);
            // (tcgnn_spmm_scaled: with a remainder behind it this kernel stores raw sums and spmm_cold_planar_kernel, the final writer,
            //  applies row scale, bias and ReLU; otherwise its twin spmm_lds_flat_epi_kernel applies them in its own store)
            SpmmFlatArgs f{};
            f.blocks = cs.d_flat; f.order = cs.d_order; f.x16 = im.x16; f.hdr = im.hdr; f.y = c.d_Y;
            f.N = plan->N; f.D = D; f.stride = im.dpad / 16; f.chunk0 = p.chunk0; f.xrows = plan->Nc + 1; f.nw = plan->nw_eff; f.nwg = cs.nwg;
            f.dbg = g_lds_dbg; f.relu = has_cold ? 0 : c.relu; f.rbase = cs.d_rbase; f.rl2 = cs.d_rl2; f.nent = std::max(cs.npairs, 1);
            f.w = c.d_W; f.dout = c.D_out; f.accumulate = r.accumulate; f.fill_quota = g_lds_fill_quota; f.wcold_ptr = cs.d_wcold_ptr; f.wcold = cs.d_wcold; f.fb = fb;
            HIP_TRY(launch_flat_any(p.maxw, p.nt, cs.flat_tpc, f, p.nchunks, stream, cs.dense_entries > 0, has_cold ? no_epi : epi, slot == kLdsLongSlot));
            if (has_cold && !(g_lds_dbg & 16)) {
                const int cd = lds_chunk_dims(p.maxw);
                const int col0 = p.chunk0 * cd, ncols = std::min(p.nchunks * cd, im.dpad - col0);
                ColdPlanarArgs ca{};
                ca.cold_ptr = cs.d_cold_ptr; ca.ccols = cs.d_cold_cols; ca.cmask = cs.d_cold_mask; ca.x16 = im.x16; ca.hdr = im.hdr; ca.y = c.d_Y;
                ca.N = plan->N; ca.D = D; ca.xrows = plan->Nc + 1; ca.nw = plan->nw_eff; ca.col0 = col0; ca.ncols = ncols; ca.relu = c.relu; ca.epi = epi;
                hipLaunchKernelGGL(spmm_cold_planar_kernel, dim3((unsigned)((plan->nw_eff + 3) / 4), (unsigned)((ncols + 63) / 64)), dim3(256), 0, stream, ca);
                HIP_TRY(hipGetLastError());
            }
            continue;
        }
        SpmmLdsArgs l{};
        l.cell_ptr = cs.d_cell_ptr; l.tiles = cs.d_cell_tiles; l.order = cs.d_order; l.x16 = im.x16; l.hdr = im.hdr; l.y = c.d_Y;
        l.N = plan->N; l.D = D; l.stride = im.dpad / 16; l.chunk0 = p.chunk0; l.xrows = plan->Nc + 1; l.nranges = cs.nranges; l.nw = plan->nw_eff; l.nwg = cs.nwg;
        l.dbg = g_lds_dbg; l.relu = r.cold ? 0 : c.relu; l.rbase = cs.d_rbase; l.rlist = cs.d_rlist;
        l.w = c.d_W; l.dout = c.D_out; l.accumulate = r.accumulate; l.parts = cs.d_parts; l.fb = fb; l.epi = r.cold ? no_epi : epi;
        HIP_TRY(launch_lds_any(p.maxw, p.nt, l, p.nchunks, stream));
    }
    return r.cold ? launch_cold_rows(c, r.cold, im, x16_rows) : TCGNN_OK;
}
// the three gather walks share their kernel arguments and cover dpad columns as for_column_chunks cuts them
static SpmmArgs gather_args(const SpmmCall& c, const StagedImage& im) {
    SpmmArgs a = spmm_args(c.plan, im, c.d_Y, c.D);
    a.edge_val = c.d_val; a.relu = c.relu; a.ldy = c.d_W ? c.D_out : (int32_t)c.stride();
    a.w = c.d_W; a.dout = c.D_out; a.unguarded = c.d_image ? 1 : 0;
    return a;
}
static int launch_sync(const SpmmCall& c, const StagedImage& im) {
    const tcgnn_plan* const plan = c.plan;
    const bool val = c.d_val != nullptr;
    KernelTimer timer(plan, c.stream, "spmm_sync_kernel");
    SpmmSyncArgs sa{gather_args(c, im), sync_args(plan, im.pitch * 2)};
    auto wgs = [&](int nt) {   // workgroups per launch: what holds a slice (S windows per XCD, 4 wavefronts x maxw windows per workgroup), at most what is resident
        const LaunchGeom g = sync_geom(nt, val);
        const int per_xcd = std::min((plan->sync.S + 4 * g.maxw - 1) / (4 * g.maxw), plan->num_cus / kXcds * g.wgs_per_cu());
        return kXcds * std::max(per_xcd, 1);
    };
    for (int r = 0; r < plan->sync.R; ++r) {   // one launch per slice round
        sa.s.round = r;
        const int rc = for_column_chunks(im.dpad, [&](int nt, int chunk0, int nchunks) {
            sa.base.chunk0 = chunk0;
            return launch_sync_any(val, nt, sa, wgs(nt), nchunks, c.stream, c.epi());
        });
        if (rc) return rc;
    }
    return TCGNN_OK;
}
static int launch_blocked(const SpmmCall& c, const StagedImage& im) {
    const tcgnn_plan* const plan = c.plan;
    const bool val = c.d_val != nullptr;
    KernelTimer timer(plan, c.stream, "spmm_blocked_kernel");
    const int nranges = range_count(plan, image_bytes(plan, im.pitch), kRangeTargetBytes);
    SpmmBlockedArgs b{gather_args(c, im), plan->d_bptr, plan->nbuckets, plan->nbuckets / nranges, nranges, plan->nw_eff, 0};
    return for_column_chunks(im.dpad, [&](int nt, int chunk0, int nchunks) {
        // persistent grid = what is resident at once: LDS per workgroup (4 wavefronts: tile buffers, pads, + the 4 KB A table)
        // against 160 KB, and the register budget (4 or 2 workgroups per CU)
        const LaunchGeom g = blocked_geom(nt, val);
        b.base.chunk0 = chunk0;
        b.ngroups = (plan->nw_eff + g.maxw - 1) / g.maxw;
        return launch_blocked_any(val, nt, b, std::min((b.ngroups + 3) / 4, plan->num_cus * g.wgs_per_cu()), nchunks, c.stream, c.epi());
    });
}
static int launch_per_window(const SpmmCall& c, const StagedImage& im) {
    const tcgnn_plan* const plan = c.plan;
    KernelTimer timer(plan, c.stream, "spmm_kernel");
    SpmmArgs a = gather_args(c, im);
    return for_column_chunks(im.dpad, [&](int nt, int chunk0, int nchunks) {
        a.chunk0 = chunk0;
        return launch_spmm_any(c.d_val != nullptr, plan->waves, nt, a, plan->nw_eff, nchunks, c.stream, c.epi());
    });
}
// rows beyond the windows the caller described stay zero, like zeros_like - or hold the epilogue of an empty sum
static int fill_uncovered_rows(const SpmmCall& c) {
    const tcgnn_plan* const plan = c.plan;
    if (c.block_of_wider || (int64_t)plan->nw_eff * kWinRows >= plan->N) return TCGNN_OK;
    HIP_TRY(hipMemsetAsync(c.d_Y, 0, (size_t)plan->N * (c.d_W ? c.D_out : c.D) * sizeof(float), c.stream));
    if (c.sc.row || c.sc.bias) {
        const int64_t n = ((int64_t)plan->N - (int64_t)plan->nw_eff * kWinRows) * c.D;
        hipLaunchKernelGGL(epi_fill_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, c.stream, c.d_Y, (int64_t)plan->nw_eff * kWinRows, plan->N, c.D, c.relu, c.epi());
        HIP_TRY(hipGetLastError());
    }
    return TCGNN_OK;
}
// check, zero fill, route (builds streams), stage, launch (each launcher's timer stops when it returns), the range guard's fallback
static int run_spmm(const SpmmCall& c) {
    const tcgnn_plan* const plan = c.plan;
    if (!plan || c.D < 1 || (plan->N > 0 && ((!c.d_X && !c.d_image) || !c.d_Y))) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_spmm: null argument or D < 1");
    if (plan->N == 0) return TCGNN_OK;
    // (the caller's buffers, before anything is enqueued - a column block of a wider call was checked with the whole call)
    if (!c.block_of_wider) {
        if (const int rc = check_output_aligned("tcgnn_spmm", "Y", c.d_Y)) return rc;
        if (!c.d_image) { if (const int rc = check_workspace("tcgnn_spmm", c.ws, c.ws_bytes, tcgnn_workspace_bytes(plan, c.D))) return rc; }
    }
    if (const int rc = fill_uncovered_rows(c)) return rc;
    SpmmRoute r;
    if (const int rc = route_spmm(c, &r)) return rc;
    if (r.walk == Walk::kValCsr) {
        hipLaunchKernelGGL(spmm_val_csr_kernel, dim3((unsigned)((plan->N + 3) / 4)), dim3(256), 0, c.stream, plan->rowptr, plan->col, c.d_val, c.d_X, c.d_Y, plan->N, c.D);
        HIP_TRY(hipGetLastError());
        return TCGNN_OK;
    }
    if (r.walk == Walk::kSmall) {
        KernelTimer timer(plan, c.stream, "spmm_small_kernel");
        launch_small_pair(c, (unsigned)plan->nw_eff, nullptr);
        HIP_TRY(hipGetLastError());
        return TCGNN_OK;
    }
    if (r.walk == Walk::kColumnBlocks) return run_column_blocks(c);
    StagedImage im;
    if (c.d_image) {   // the caller built the fp16 image itself: tcgnn_spmm_staged / tcgnn_spmm_staged_planar
        im.hdr = static_cast<const uint32_t*>(c.d_image);
        im.x16 = reinterpret_cast<const _Float16*>(static_cast<const char*>(c.d_image) + kHdrBytes);
        im.dpad = c.dpad();
        im.pitch = x16_pitch(im.dpad);   // (planar: [dpad / 16][Nc + 1][16] halves - the LDS-resident launcher does not use the pitch)
    } else {
        StageOpts o; o.planar = r.planar(); o.d_gate = c.d_gate; o.ldx = c.block_of_wider ? c.ld : 0; o.block_of_wider = c.block_of_wider; o.d_cs = c.sc.col;
        if (const int rc = stage_features(plan, c.d_X, c.d_val, c.D, c.ws, c.ws_bytes, c.stream, o, &im)) return rc;
    }
    if (plan->nw_eff == 0) return TCGNN_OK;
    int rc = TCGNN_OK;
    switch (r.walk) {
        case Walk::kValLds:    rc = launch_val_lds(c, im); break;
        case Walk::kValSliced: rc = launch_val_sliced(plan, im, c.d_val, c.d_Y, c.D, c.ws, r.nslices, c.stream); break;
        case Walk::kLds:       rc = launch_lds(c, r, im); break;
        case Walk::kSync:      rc = launch_sync(c, im); break;
        case Walk::kBlocked:   rc = launch_blocked(c, im); break;
        default:               rc = launch_per_window(c, im); break;
    }
    return (rc || r.own_fb) ? rc : launch_wide_fallback(c, im);
}

// ------------------------------------------------------------------------------------------
// tcgnn_spmm_heads: Y[:, hF:(h+1)F] = A_val(edge_val[h, :]) X[:, hF:(h+1)F] for H heads.  One decision (route_heads), from the plan
// and (H, F) alone, before anything is staged; tcgnn_spmm_heads_workspace_bytes asks the same function.
// ------------------------------------------------------------------------------------------
struct HeadsCall {
    const tcgnn_plan* plan = nullptr;
    const float *d_X = nullptr, *d_val = nullptr;   // X [N, H F]; edge values [H, E] head-major
    float* d_Y = nullptr;
    int32_t H = 0, F = 0;
    void* ws = nullptr; size_t ws_bytes = 0;
    hipStream_t stream = nullptr;
};
// kSingle: H == 1 is tcgnn_spmm_val itself (run_spmm, every walk it has); kFused: spmm_heads_kernel - one staged image, one walk of the
// tile stream per pass of whole heads; kCsr: a plan the tile stream cannot serve with edge values (route_spmm's kValCsr), all heads in
// one CSR launch; kPerHead: head by head inside the library - each head a column block of X and Y (run_spmm with ld, block_of_wider,
// as run_column_blocks does it) with its own row of edge values, every block rounded with the scales of the whole call
enum class HeadsWay { kSingle, kFused, kCsr, kPerHead };
// heads one pass of the fused walk takes at F columns each; 0: a width it does not cover.  At most kMaxHeadsPerPass heads and
// kMaxHeadsPassDims columns (what a workgroup's LDS then holds: tcgnn_heads.inc) and at least TWO heads: a pass of one head shares
// no gather with another, it would be the per-window walk once per head - the head-by-head way keeps run_spmm's choice among the
// gather walks for such widths (F > 32).  A pass starts at a multiple of 16 columns (the gather's slices), so where F is not one
// the FULL passes take an even number of heads: F = 8 -> 4, F = 24 -> 2 (F = 16 -> 4, F = 32 -> 2).
static int heads_per_pass(int F) {
    if (F < 8 || F % 8 || F > kMaxHeadsPassDims / 2) return 0;
    const int g = std::min(kMaxHeadsPerPass, kMaxHeadsPassDims / F);
    return F % 16 == 0 ? g : (g & ~1);
}
static HeadsWay route_heads(const tcgnn_plan* plan, int32_t H, int32_t F) {
    if (H == 1) return HeadsWay::kSingle;
    if (!plan->canonical || plan->E < 4) return HeadsWay::kCsr;
    const int D = H * F;
    if (heads_per_pass(F) > 0 && plan->nw_eff > 0 && pitch_fits_descriptor(D) && !image_is_big(plan->Nc, x16_pitch(round_up(D, 16)))) return HeadsWay::kFused;
    return HeadsWay::kPerHead;
}
static size_t heads_workspace_bytes(const tcgnn_plan* plan, int32_t H, int32_t F) {
    switch (route_heads(plan, H, F)) {
        case HeadsWay::kSingle: return tcgnn_workspace_bytes(plan, F);
        case HeadsWay::kFused:  return workspace_bytes_for(plan->Nc, H * F);                          // one image of all of X
        // one head's block at a time.  (kCsr stages nothing, but is handed the same buffer: pointer, alignment and size are checked
        //  alike on every route, so what a caller must provide does not depend on the route)
        default:                return workspace_bytes_for(plan->Nc, std::min(F, kMaxGatherBlockDims));
    }
}
static int launch_heads_fused(const HeadsCall& c) {
    const tcgnn_plan* const plan = c.plan;
    const int32_t D = c.H * c.F;
    StagedImage im;
    if (const int rc = stage_features(plan, c.d_X, nullptr, D, c.ws, c.ws_bytes, c.stream, StageOpts{}, &im)) return rc;
    launch_absmax_val(plan, c.d_val, (int64_t)c.H * plan->E, static_cast<uint32_t*>(c.ws), c.stream);   // (max |edge_val| over all H E values: one scale for the whole call)
    HIP_TRY(hipGetLastError());
    {
        KernelTimer timer(plan, c.stream, "spmm_heads_kernel");
        SpmmArgs a = spmm_args(plan, im, c.d_Y, D);   // (route_heads: never a big image)
        a.edge_val = c.d_val;
        const int g = heads_per_pass(c.F), nfull = c.H / g, rem = c.H % g;
        if (nfull) HIP_TRY(launch_heads_any(g, c.F / 8, SpmmHeadsArgs{a, 0}, plan->waves, plan->nw_eff, nfull, c.stream));
        if (rem) HIP_TRY(launch_heads_any(rem, c.F / 8, SpmmHeadsArgs{a, nfull * g}, plan->waves, plan->nw_eff, 1, c.stream));
    }
    // the range guard's fp32 way behind the kernel, one launch for all heads (returns at once unless the call is "wide": range_is_wide_val)
    const unsigned grid = (unsigned)std::min<int64_t>(((int64_t)plan->N + 3) / 4, 4096);
    hipLaunchKernelGGL(spmm_heads_wide_fallback_kernel, dim3(grid, (unsigned)c.H), dim3(256), 0, c.stream, im.hdr, plan->rowptr, plan->col, c.d_val, c.d_X, c.d_Y, plan->N, c.F,
                       plan->E, (int64_t)D);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}
static int run_heads_one_by_one(const HeadsCall& c) {
    const tcgnn_plan* const plan = c.plan;
    const int32_t D = c.H * c.F;
    // (X's scale over all of X and max |edge_val| over all H E values: every head rounded as the fused walk rounds it)
    if (const int rc = fill_header(plan, static_cast<uint32_t*>(c.ws), c.d_X, nullptr, nullptr, D, guard_spmm(plan), c.d_val, (int64_t)c.H * plan->E, c.stream)) return rc;
    for (int h = 0; h < c.H; ++h)
        for (int c0 = 0; c0 < c.F; c0 += kMaxGatherBlockDims) {   // (a head wider than one gather launch covers: its own column blocks)
            SpmmCall b;
            b.plan = plan; b.d_X = c.d_X + (int64_t)h * c.F + c0; b.d_Y = c.d_Y + (int64_t)h * c.F + c0; b.d_val = c.d_val + (int64_t)h * plan->E;
            b.D = std::min(kMaxGatherBlockDims, c.F - c0); b.ws = c.ws; b.ws_bytes = c.ws_bytes; b.stream = c.stream;
            b.ld = D; b.block_of_wider = true;
            if (const int rc = run_spmm(b)) return rc;
        }
    return TCGNN_OK;
}
// check, zero fill, route, run
static int run_spmm_heads(const HeadsCall& c) {
    const tcgnn_plan* const plan = c.plan;
    if (!plan || c.H < 1 || c.F < 1 || (int64_t)c.H * c.F > INT32_MAX) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_spmm_heads: null plan, H < 1, F < 1 or H * F beyond int32");
    if (plan->N > 0 && (!c.d_X || !c.d_Y || (plan->E > 0 && !c.d_val))) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_spmm_heads: null array");
    if (plan->N == 0) return TCGNN_OK;
    if (c.H == 1) {   // exactly tcgnn_spmm_val
        SpmmCall s;
        s.plan = plan; s.d_X = c.d_X; s.d_Y = c.d_Y; s.D = c.F; s.ws = c.ws; s.ws_bytes = c.ws_bytes; s.stream = c.stream;
        if (plan->E > 0) s.d_val = c.d_val;
        return run_spmm(s);
    }
    if (const int rc = check_output_aligned("tcgnn_spmm_heads", "Y", c.d_Y)) return rc;
    if (const int rc = check_workspace("tcgnn_spmm_heads", c.ws, c.ws_bytes, heads_workspace_bytes(plan, c.H, c.F))) return rc;
    const size_t y_bytes = (size_t)plan->N * c.H * c.F * sizeof(float);
    if (plan->E == 0) { HIP_TRY(hipMemsetAsync(c.d_Y, 0, y_bytes, c.stream)); return TCGNN_OK; }
    const HeadsWay way = route_heads(plan, c.H, c.F);
    if (way == HeadsWay::kCsr) {
        hipLaunchKernelGGL(spmm_heads_csr_kernel, dim3((unsigned)((plan->N + 3) / 4)), dim3(256), 0, c.stream, plan->rowptr, plan->col, c.d_val, c.d_X, c.d_Y, plan->N, c.H, c.F, plan->E);
        HIP_TRY(hipGetLastError());
        return TCGNN_OK;
    }
    // rows beyond the windows the caller described stay zero, like zeros_like (fill_uncovered_rows, for all heads at once)
    if ((int64_t)plan->nw_eff * kWinRows < plan->N) HIP_TRY(hipMemsetAsync(c.d_Y, 0, y_bytes, c.stream));
    return way == HeadsWay::kFused ? launch_heads_fused(c) : run_heads_one_by_one(c);
}
