// tcgnn_edge_dispatch.inc - host side of the two edge operators, in the shape of tcgnn_spmm_dispatch.inc: SDDMM (tcgnn_sddmm, tcgnn_sddmm2,
// and at the end of the file tcgnn_sddmm_heads with its own route on top of run_sddmm) and the fused AGNN pair.  Per operator: the request (SddmmCall / AgnnCall), ONE routing decision made before anything is staged
// (route_sddmm / route_agnn: plan facts, mode, width and the per-call test knobs), one launcher per walk, the range guard's tail, run_*.
// Included by tcgnn_device.hip in front of tcgnn_spmm_dispatch.inc: tcgnn_spmm_val's XCD-sliced walk asks agnn_plan_walk and runs
// launch_val_sliced, and tcgnn_workspace_bytes sizes the slice addends with agnn_slices - one predicate, one AgnnArgs builder for all.
// (Nothing depends on the order of the sections: `make audit`'s listing names template kernels in the order their launch tables are
//  first used, and tools/compare_listings.py compares two listings kernel by kernel, whatever their order.)

// wide_patch_kernel's arguments that both operators take from the plan.  The kernel's row-driven branch is a shortcut of its scan with
// the same scores bit for bit: TCGNN_PATCH_ROWS=0, read per call, hands it no symmetry word, so the same input takes the scan (tests
// compare the two).  rows: what the windows of the plan cover - behind them the outputs keep the zeros run_sddmm / run_agnn wrote.
static const int32_t* patch_sym_of(const tcgnn_plan* plan) {
    const char* const env = test_knob("TCGNN_PATCH_ROWS");
    return env && atoi(env) == 0 ? nullptr : plan->d_sym;
}
static int32_t patch_rows_of(const tcgnn_plan* plan) { return (int32_t)std::min<int64_t>(plan->N, (int64_t)plan->nw_eff * kWinRows); }
// wide_patch_kernel's arguments for an SDDMM call (mode 0); the fused pair adds w, Y, efmax, dw_extra and its mode.  What is not named is zero
static PatchArgs patch_args(const tcgnn_plan* plan, const StagedImage& im, const float* d_X, float* d_ef, int32_t D, void* ws) {
    PatchArgs pa{};
    pa.hdr = im.hdr; pa.bitmap = dirty_bitmap_of(ws, plan->Nc, D); pa.rowptr = plan->rowptr; pa.col = plan->col; pa.e2r = plan->e2r;
    pa.X = d_X; pa.x16 = im.x16; pa.pitch = im.pitch; pa.ef = d_ef;
    pa.N = plan->N; pa.Nc = plan->Nc; pa.D = D; pa.row_off = plan->row_off; pa.E = plan->E; pa.sym = patch_sym_of(plan); pa.rows = patch_rows_of(plan);
    return pa;
}

// ------------------------------------------------------------------------------------------
// the fused AGNN pair
// ------------------------------------------------------------------------------------------
// The fused AGNN kernel's walks beside the per-window one (agnn_kernel), for graphs whose numbering carries no locality of its own and
// whose windows are alike, when the fp16 image does not fit an XCD's 4 MB L2 but an eighth of it does:
//   XCD-sliced  - nslices addends of Y in the workspace and a pass that sums them;
//   range-major - persistent wavefronts owning two windows each (no addends; more registers).
// Measured on the Reddit shape (tools/bench_agnn.py, forward / backward ms; r03 with whole-line gathers at D = 64):
//   D = 16 (7.4 MB)  per-window 1.13 / 1.43   sliced 1.06 / 1.28   range-major 1.19 / 1.59
//   D = 32 (14.9 MB) per-window 1.46 / 1.65   sliced 1.20 / 1.38   range-major 1.26 / 1.65
//   D = 64 (29.8 MB) per-window 1.74 / 1.77   sliced 1.53 / 1.60   range-major 1.45-1.48 / 1.78   (sixteen slices in two rounds 1.81 / 1.85)
//   D = 128 (59.6 MB) per-window 3.48 / 3.53  sliced 2.61-2.67 / 2.71-2.73   range-major 2.68-2.73 / 2.93-2.95   (slices of 7.4 MB: they do
//                     not stay in a 4 MB L2, but an XCD that is asked for an eighth of the image still hits more often than one asked for all of it)
// so: sliced in both directions up to 16 MB; from there to 64 MB range-major forward (within 2 % of sliced, no addends) and sliced backward.
// What these walks are bound by is the memory system's throughput at their hit rate, not by what a wavefront has in flight nor by
// its instruction count (r03, measured on the sliced walk at D = 64): a quarter fewer VALU instructions per tile (103 -> 71 in the
// forward tile block) changed nothing; a second tile buffer with the gather running two tiles ahead (counted vmcnt, no extra
// registers) moved forward 1.53 -> 1.53 and backward 1.60 -> 1.57 and was taken out again; four wavefronts per SIMD instead of
// three (forward kernel squeezed from 130 to 128 registers, 12 bytes of scratch) 1.53 -> 1.43-1.45 sliced but 1.73 -> 1.79-1.87 per-window
// (more wavefronts thrash the L2 harder) - level with range-major's 1.45-1.48, so not kept either.
// TCGNN_AGNN_SLICED (read per call: tests switch it): 0 per-window only, 1 the rule above, 2 sliced whenever possible, 16 two rounds.
static constexpr size_t kAgnnSliceBytes = (size_t)4 << 20;
// (r06) on a graph with locality the sliced walk takes the windows in their own order, rotated per XCD (AgnnArgs::rot: sbm_reddit, forced
// sliced, 1.96 / 2.50 -> 1.59 / 1.63 ms) - which only a forced walk meets: the automatic rule keeps such graphs per-window.  Without locality
// the plan's order stays (uniform graph: 1.61 / 1.63 against 1.62 / 1.67 rotated).  TCGNN_AGNN_ROT=0|1 overrides.
static int agnn_rot(const tcgnn_plan* plan) {
    const char* const env = test_knob("TCGNN_AGNN_ROT");
    return (env ? atoi(env) != 0 : plan->near_frac > 0.2) && windows_balanced(plan) ? 1 : 0;
}
static bool agnn_supported(const tcgnn_plan* plan, int32_t D) {
    return plan && plan->canonical && D >= 1 && D <= kMaxChunkDims && plan->E >= 8;
}
enum class AgnnWalk { kPerWindow, kSliced, kRangeMajor, kSync };
struct AgnnRoute { AgnnWalk walk = AgnnWalk::kPerWindow; int nslices = 0, rot = 0; bool sync_one = false; };   // (nslices, rot: kSliced; sync_one: kSync)
// The plan-and-width rule between the three forms above (kSync is not its to give; nslices set with kSliced).  route_agnn decides a fused
// call on top of it; route_spmm's kValSliced and agnn_slices - the workspace - ask it as it is, so what they answer is what the call does.
static AgnnRoute agnn_plan_walk(const tcgnn_plan* plan, int32_t D, bool bwd) {
    AgnnRoute r;
    const char* const env = test_knob("TCGNN_AGNN_SLICED");
    const int knob = env ? atoi(env) : 1;
    if (!knob || plan->waves != 4 || plan->nbuckets < 8 || plan->nw_eff < 1 || plan->nbuckets % kXcds) return r;
    const int pitch = x16_pitch(round_up(D, 16));
    if (image_is_big(plan->Nc, pitch)) return r;
    const size_t x16_bytes = image_bytes(plan, pitch);
    if (knob >= 2) { r.walk = AgnnWalk::kSliced; r.nslices = (knob == 16 && plan->nbuckets % 16 == 0) ? 16 : kXcds; return r; }   // (forced)
    if (!(x16_bytes > kBlockedMinBytes && x16_bytes <= 2 * (size_t)kXcds * kAgnnSliceBytes && plan->nw_eff >= 8 * plan->num_cus &&
          windows_balanced(plan) && !has_locality(plan))) return r;
    if (!bwd && x16_bytes > (size_t)kXcds * (kAgnnSliceBytes / 2)) { r.walk = AgnnWalk::kRangeMajor; return r; }   // 16 - 64 MB: forward
    // (the sliced walk wants every window's tiles spread evenly over the slices: workgroups are handed to the XCDs round-robin and
    //  in order, so where a window has most of its tiles in one slice - the calibrated SBM graph: 22.5 % of the edges inside the
    //  window's own community, near_frac 0.3 - the XCD of that slice holds the others up: backward 1.81 -> 2.40 ms there)
    if (plan->near_frac > 0.2) return r;
    r.walk = AgnnWalk::kSliced; r.nslices = kXcds;
    return r;
}
// (the workspace is sized for whichever direction slices)
static int agnn_slices(const tcgnn_plan* plan, int32_t D) { return std::max(agnn_plan_walk(plan, D, false).nslices, agnn_plan_walk(plan, D, true).nslices); }
static size_t agnn_slice_bytes(const tcgnn_plan* plan, int32_t D) {
    return ((size_t)agnn_slices(plan, D) * (size_t)plan->N * D * sizeof(float) + 255) / 256 * 256;
}
// Which walk a fused call takes, in this order:
//   1. the slice-synchronised walk (r06, tcgnn_sync_walk.inc: communities larger than an XCD's L2) where sync_chosen takes it - mode 0 or 5,
//      four wavefronts per window, an image below 4 GB;
//   2. the XCD-sliced walk where agnn_plan_walk says so - whatever the mode - unless mode 2 is forced;
//   3. range-major: mode 2 forced, or mode 0 and agnn_plan_walk's answer; needs the bucket table and an image below 4 GB;
//   4. per-window - all a big image (image_is_big) ever gets: agnn_plan_walk answers per-window for it, 1 and 3 exclude it.
// The range-major variant (bit-compatible scores, sums in another order): slower than the per-window walk while the kernel
// asked for every 128-byte line twice (r02: D = 64 1.87 vs 1.80 ms forward); with whole-line gathers (r03) its forward pass
// is the fastest form at D = 64 (1.45-1.48 against 1.74 per-window, 1.53 sliced) - agnn_plan_walk picks it there; mode 2 forces it.
// (the backward kernel beyond 96 columns owns its windows at ONE wavefront per SIMD on the slice-synchronised walk - 256 registers do not hold two
//  windows' accumulators, operands and per-row exponents - and loses more than the walk returns there: products shape, D = 128, 4.10 -> 6.24 ms; it
//  stays per-window unless forced.  sync_one, r06: ONE window per wavefront there - two wavefronts per SIMD, three trips per slice)
static AgnnRoute route_agnn(const tcgnn_plan* plan, int32_t D, bool bwd, int mode) {
    AgnnRoute r = agnn_plan_walk(plan, D, bwd);
    const int pitch = x16_pitch(round_up(D, 16)), nt = round_up(D, 16) / 16;
    const bool big = image_is_big(plan->Nc, pitch);
    const bool range_major = plan->nbuckets > 0 && (mode == 2 || (mode == 0 && r.walk == AgnnWalk::kRangeMajor)) && !big;
    if (plan->waves == 4 && !big && sync_chosen(plan, pitch * 2, mode, bwd ? kSyncFusedBwd : kSyncFusedFwd, nt)) {
        r.walk = AgnnWalk::kSync; r.nslices = 0; r.sync_one = bwd && nt > 6;
    } else if (r.walk == AgnnWalk::kSliced && !range_major) r.rot = agnn_rot(plan);
    else { r.walk = range_major ? AgnnWalk::kRangeMajor : AgnnWalk::kPerWindow; r.nslices = 0; }
    return r;
}
struct AgnnCall {
    const tcgnn_plan* plan = nullptr;
    const float *d_X = nullptr, *d_w = nullptr;   // d_X: X (forward) or dY (backward)
    float* d_ef = nullptr;                        // forward: out; backward: the saved scores (read only)
    uint32_t* d_absmax = nullptr;                 // max |ef| and, behind it, one scale exponent per row
    float *d_Y = nullptr, *d_dw = nullptr;        // d_Y: Y or G; d_dw: backward only
    int32_t D = 0;
    void* ws = nullptr; size_t ws_bytes = 0;
    hipStream_t stream = nullptr;
    bool bwd = false;
    const char* name = "";   // the entry point, for messages
};
// behind the image in the workspace: the d_w reduction slots, then the slice addends of Y (tcgnn_workspace_bytes)
static double* agnn_partial_of(void* ws, const tcgnn_plan* plan, int32_t D) { return reinterpret_cast<double*>(static_cast<char*>(ws) + workspace_bytes_for(plan->Nc, D)); }
static float* agnn_addends_of(void* ws, const tcgnn_plan* plan, int32_t D) { return reinterpret_cast<float*>(static_cast<char*>(ws) + workspace_bytes_for(plan->Nc, D) + agnn_partial_bytes(plan)); }
// the kernel arguments every walk starts from; what is not named here is zero (the walks set their own fields)
static AgnnArgs agnn_args(const tcgnn_plan* plan, const StagedImage& im, int32_t D, const float* w, float* ef, uint32_t* ef_absmax, float* y, double* partial) {
    AgnnArgs a{};
    a.wb_ptr = plan->d_wb_ptr; a.order = plan->d_order; a.cols = plan->d_cols; a.mask = plan->d_mask; a.ebase = plan->d_ebase;
    a.x16 = im.x16; a.hdr = im.hdr; a.w = w; a.ef = ef; a.ef_absmax = ef_absmax; a.y = y; a.partial = partial;
    a.N = plan->N; a.Nc = plan->Nc; a.row_off = plan->row_off; a.Dpad = im.dpad; a.D = D; a.stride = im.pitch; a.E = plan->E;
    a.rowptr = plan->rowptr; a.bptr = plan->d_bptr; a.nbuckets = plan->nbuckets; a.nw = plan->nw_eff;
    a.big = image_is_big(plan->Nc, im.pitch);
    return a;
}
// Y = the sum of the sliced walk's nslices addends (the caller asks hipGetLastError)
static void launch_slice_sum(const tcgnn_plan* plan, const float* ypart, float* d_Y, int32_t D, int nslices, hipStream_t stream) {
    const int64_t nsum = std::min<int64_t>(plan->N, (int64_t)plan->nw_eff * kWinRows) * D;   // (rows beyond the windows were zeroed by the caller)
    const unsigned sg = (unsigned)std::min<int64_t>(2048, (nsum / 4 + 255) / 256 + 1);
    hipLaunchKernelGGL(agnn_slice_sum_kernel, dim3(sg), dim3(256), 0, stream, ypart, d_Y, nsum, (int64_t)plan->N * D, nslices);
}
// tcgnn_spmm_val on the XCD-sliced walk (route_spmm's kValSliced): the backward kernel with the score half off - w = 1, ef = the caller's
// values, their abs-max from this call's header, one scale (no rowka) - and the slice sum
static int launch_val_sliced(const tcgnn_plan* plan, const StagedImage& im, const float* d_val, float* d_Y, int32_t D, void* ws, int ns, hipStream_t stream) {
    AgnnArgs a = agnn_args(plan, im, D, nullptr, const_cast<float*>(d_val), const_cast<uint32_t*>(im.hdr) + kHdrMaxVal, agnn_addends_of(ws, plan, D), agnn_partial_of(ws, plan, D));
    a.gsel = plan->nbuckets / ns; a.nslices = ns; a.valonly = 1; a.rot = agnn_rot(plan);
    KernelTimer timer(plan, stream, "agnn_kernel (XCD-sliced, values only) + agnn_slice_sum_kernel");
    HIP_TRY((launch_agnn<4, true, 0>(im.dpad / 16, a, ns * ((plan->nw_eff + 3) / 4), stream)));
    launch_slice_sum(plan, a.y, d_Y, D, ns, stream);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}
// ---- launchers: one per walk; *nslots: the d_w slots the launch wrote (one per workgroup) - what the patch and agnn_reduce_kernel sum
// slice-synchronised: one launch per slice round, each with its own run of d_w slots
static hipError_t launch_agnn_sync(const AgnnCall& c, const AgnnRoute& r, AgnnArgs a, int* nslots) {
    const tcgnn_plan* const plan = c.plan;
    const int nt = a.Dpad / 16;
    KernelTimer timer(plan, c.stream, "agnn_kernel (slice-synchronised)");
    a.use_sync = 1;
    a.sync = sync_args(plan, a.stride * 2);
    const int mw = r.sync_one ? 1 : kAgnnMaxW;
    const int per_launch = kXcds * std::max(1, std::min((plan->sync.S + 4 * mw - 1) / (4 * mw), plan->num_cus / kXcds * agnn_geom(nt, 4, c.bwd, mw).wgs_per_cu()));
    double* const partial = a.partial;
    hipError_t e = hipSuccess;
    for (int q = 0; q < plan->sync.R && e == hipSuccess; ++q) {
        a.sync.round = q;
        a.partial = partial + (size_t)q * per_launch;
        e = !c.bwd ? launch_agnn<4, false, kAgnnMaxW>(nt, a, per_launch, c.stream) : (r.sync_one ? launch_agnn_wide_one(nt, a, per_launch, c.stream) : launch_agnn<4, true, kAgnnMaxW>(nt, a, per_launch, c.stream));
    }
    *nslots = plan->sync.R * per_launch;   // (R x 768 workgroups at most, fewer than the windows the workspace counts - build_sync_tables wants 2048 of them)
    return e;
}
static hipError_t launch_agnn_sliced(const AgnnCall& c, const AgnnRoute& r, AgnnArgs a, int* nslots) {
    const tcgnn_plan* const plan = c.plan;
    KernelTimer timer(plan, c.stream, "agnn_kernel (XCD-sliced) + agnn_slice_sum_kernel");
    a.nslices = r.nslices;
    a.gsel = plan->nbuckets / r.nslices;
    a.y = agnn_addends_of(c.ws, plan, c.D);
    a.rot = r.rot;
    *nslots = r.nslices * ((plan->nw_eff + 3) / 4);
    hipError_t e = c.bwd ? launch_agnn<4, true, 0>(a.Dpad / 16, a, *nslots, c.stream) : launch_agnn<4, false, 0>(a.Dpad / 16, a, *nslots, c.stream);
    if (e == hipSuccess) {
        launch_slice_sum(plan, a.y, c.d_Y, c.D, r.nslices, c.stream);
        e = hipGetLastError();
    }
    return e;
}
static hipError_t launch_agnn_range_major(const AgnnCall& c, AgnnArgs a, int* nslots) {
    const tcgnn_plan* const plan = c.plan;
    const int nt = a.Dpad / 16;
    KernelTimer timer(plan, c.stream, "agnn_kernel");
    a.nranges = range_count(plan, image_bytes(plan, a.stride), 4 * kRangeTargetBytes);
    a.gsel = plan->nbuckets / a.nranges;
    a.ngroups = (plan->nw_eff + kAgnnMaxW - 1) / kAgnnMaxW;
    *nslots = std::min((a.ngroups + 3) / 4, plan->num_cus * agnn_range_major_wgs_per_cu(nt, c.bwd));
    return c.bwd ? launch_agnn<4, true, kAgnnMaxW>(nt, a, *nslots, c.stream) : launch_agnn<4, false, kAgnnMaxW>(nt, a, *nslots, c.stream);
}
static hipError_t launch_agnn_per_window(const AgnnCall& c, const AgnnArgs& a, int* nslots) {
    const tcgnn_plan* const plan = c.plan;
    const int nt = a.Dpad / 16;
    KernelTimer timer(plan, c.stream, "agnn_kernel");
    *nslots = plan->nw_eff;
    if (plan->waves == 4) return c.bwd ? launch_agnn<4, true, 0>(nt, a, *nslots, c.stream) : launch_agnn<4, false, 0>(nt, a, *nslots, c.stream);
    return c.bwd ? launch_agnn<1, true, 0>(nt, a, *nslots, c.stream) : launch_agnn<1, false, 0>(nt, a, *nslots, c.stream);
}
// check, route, zero fill, stage, launch, the range guard's patch, the d_w reduction
static int run_agnn(const AgnnCall& c) {
    const tcgnn_plan* const plan = c.plan;
    const int32_t D = c.D;
    const bool bwd = c.bwd;
    if (!plan || D < 1 || !c.d_w || !c.d_absmax || (bwd && !c.d_dw) || (plan->N > 0 && (!c.d_X || !c.d_Y)) || (plan->E > 0 && !c.d_ef))
        return fail(TCGNN_ERR_INVALID_ARG, "%s: null argument or D < 1", c.name);
    if (!agnn_supported(plan, D))
        return fail(TCGNN_ERR_UNSUPPORTED, "%s: needs a canonical plan, D <= %d and E >= 8 (canonical=%d, D=%d, E=%lld)", c.name,
                    kMaxChunkDims, plan->canonical, D, (long long)plan->E);
    hipStream_t stream = c.stream;
    const AgnnRoute r = route_agnn(plan, D, bwd, spmm_mode_of(plan));
    if (const int rc = check_output_aligned(c.name, bwd ? "G" : "Y", c.d_Y)) return rc;
    if (const int rc = check_workspace(c.name, c.ws, c.ws_bytes, tcgnn_workspace_bytes(plan, D))) return rc;
    // (tcgnn_workspace_bytes holds the image, the reduction slots and the slice addends of this call: image + max(partial + slices, ..))
    if ((int64_t)plan->nw_eff * kWinRows < plan->N) {   // rows the caller's windows do not cover stay zero
        HIP_TRY(hipMemsetAsync(c.d_Y, 0, (size_t)plan->N * D * sizeof(float), stream));
        if (!bwd) HIP_TRY(hipMemsetAsync(c.d_ef, 0, (size_t)plan->E * sizeof(float), stream));
    }
    if (!bwd) HIP_TRY(hipMemsetAsync(c.d_absmax, 0, sizeof(uint32_t), stream));
    const Guard gsd = guard_sddmm(plan, D);
    StageOpts so; so.guard = &gsd;
    StagedImage im;
    if (const int rc = stage_features(plan, c.d_X, nullptr, D, c.ws, c.ws_bytes, stream, so, &im)) return rc;
    double* const partial = agnn_partial_of(c.ws, plan, D);
    if (plan->nw_eff == 0) {
        if (bwd) HIP_TRY(hipMemsetAsync(c.d_dw, 0, sizeof(float), stream));
        return TCGNN_OK;
    }
    AgnnArgs a = agnn_args(plan, im, D, c.d_w, c.d_ef, c.d_absmax, c.d_Y, partial);
    a.rowka = reinterpret_cast<int32_t*>(c.d_absmax + 1);   // (the per-row exponents of the edge weights sit behind the max |ef| word)
    int nslots = 0;
    hipError_t e;
    switch (r.walk) {
        case AgnnWalk::kSync:       e = launch_agnn_sync(c, r, a, &nslots); break;
        case AgnnWalk::kSliced:     e = launch_agnn_sliced(c, r, a, &nslots); break;
        case AgnnWalk::kRangeMajor: e = launch_agnn_range_major(c, a, &nslots); break;
        default:                    e = launch_agnn_per_window(c, a, &nslots); break;
    }
    HIP_TRY(e);
    // (the d_w correction of the patch: the double at header word kHdrDwExtra, zeroed with the header by fill_header)
    double* const dw_extra = reinterpret_cast<double*>(const_cast<uint32_t*>(im.hdr) + kHdrDwExtra);
    const int guard_level = range_guard_of(plan);
    if (guard_level >= 2) {
        // a few dirty rows (what training produces): the MFMA kernel above ran, the edges that touch them are recomputed here
        PatchArgs pa = patch_args(plan, im, c.d_X, c.d_ef, D, c.ws);
        pa.w = c.d_w; pa.Y = c.d_Y; pa.efmax = c.d_absmax; pa.dw_extra = dw_extra; pa.mode = bwd ? 2 : 1;
        // (many: the same launch does all the work in plain fp32 - wide_dense_body; one launch per call either way, returning at once
        //  unless the staged matrix is "wide")
        HIP_TRY(launch_wide_patch(pa, stream, partial, nslots));
    }
    if (bwd) {
        hipLaunchKernelGGL(agnn_reduce_kernel, dim3(1), dim3(kReduceThreads), 0, stream, partial, nslots, c.d_dw, guard_level >= 2 ? dw_extra : (const double*)nullptr);
        HIP_TRY(hipGetLastError());
    }
    return TCGNN_OK;
}

// ------------------------------------------------------------------------------------------
// SDDMM: tcgnn_sddmm (d_Xw == nullptr: both operands are d_X) and tcgnn_sddmm2 (d_Xw: the window operand, d_X: the gathered one)
// ------------------------------------------------------------------------------------------
struct SddmmCall {
    const tcgnn_plan* plan = nullptr;
    const float *d_Xw = nullptr, *d_X = nullptr;
    float* d_ef = nullptr;
    int32_t D = 0;
    void* ws = nullptr; size_t ws_bytes = 0;
    hipStream_t stream = nullptr;
    const char* name = "";   // the entry point, for messages
    // tcgnn_sddmm_heads on its fused walk: H heads of F columns (D = H F, d_ef [H, E]); 0: one head.  ld > 0: the operands are column
    // blocks of wider row-major matrices of that row stride, whose headers the caller filled over the whole matrices (hdr_filled)
    int32_t H = 0, F = 0;
    int64_t ld = 0; bool hdr_filled = false;
    int dpad() const { return round_up(D, 16); }
    int ks() const { return (dpad() + 31) / 32; }
};
// kCsr: a non-canonical plan (no staging); kSync: slice-synchronised; kRangeMajor: persistent wavefronts over nranges column ranges
enum class SddmmWalk { kCsr, kSync, kRangeMajor, kPerWindow };
struct SddmmRoute { SddmmWalk walk = SddmmWalk::kPerWindow; int nranges = 0, xcd = 0, ident = 0; };   // (nranges, xcd, ident: kRangeMajor)
// persistent grid of the range-major walk: what is resident at once, at most one wavefront per (range, window) item
static int sddmm_range_major_wgs(const tcgnn_plan* plan, int ks, int nranges) {
    const int64_t items = (int64_t)nranges * plan->nw_eff;
    return (int)std::min<int64_t>((items + 3) / 4, (int64_t)plan->num_cus * sddmm_geom(ks, 4).wgs_per_cu());
}
// The passes of the fused multi-head walk: H heads in ceil(H / kSddmmMaxHeadsPerPass) passes of at most 128 columns, as even as they
// come - `nbig` passes of g + 1 heads, then the others of g (5 = 3 + 2, 7 = 4 + 3, 8 = 4 + 4) - so that no pass is a single head.
struct SddmmHeadsPasses { int g = 0, nbig = 0, n = 0; };
static SddmmHeadsPasses sddmm_heads_passes(int H, int F) {
    const int gmax = std::min(kSddmmMaxHeadsPerPass, 128 / F);
    SddmmHeadsPasses p;
    p.n = (H + gmax - 1) / gmax; p.g = H / p.n; p.nbig = H % p.n;
    return p;
}
// resident workgroups per CU of a fused call: those of its widest pass (sddmm_heads_geom); the passes share the CUs - grid.y
static int sddmm_heads_wgs_per_cu(const SddmmCall& c) {
    const SddmmHeadsPasses p = sddmm_heads_passes(c.H, c.F);
    return std::max(1, sddmm_heads_geom(c.F, p.nbig ? p.g + 1 : p.g, 4).wgs_per_cu() / p.n);
}
// launch every pass of a fused call on `nwg` workgroups each: the passes of g + 1 heads in one launch, those of g in another
template <int WAVES, bool BLOCKED>
static hipError_t launch_sddmm_heads_passes(const SddmmCall& c, SddmmArgs a, int nwg) {
    const SddmmHeadsPasses p = sddmm_heads_passes(c.H, c.F);
    a.E = c.plan->E;
    hipError_t e = hipSuccess;
    if (p.nbig) { a.head0 = 0; e = launch_sddmm_heads<WAVES, BLOCKED>(c.F, p.g + 1, a, nwg, p.nbig, c.stream); }
    if (e == hipSuccess && p.n > p.nbig) { a.head0 = p.nbig * (p.g + 1); e = launch_sddmm_heads<WAVES, BLOCKED>(c.F, p.g, a, nwg, p.n - p.nbig, c.stream); }
    return e;
}
static int sddmm_heads_range_major_wgs(const SddmmCall& c, int nranges) {
    const int64_t items = (int64_t)nranges * c.plan->nw_eff;
    return (int)std::min<int64_t>((items + 3) / 4, (int64_t)c.plan->num_cus * sddmm_heads_wgs_per_cu(c));
}
// One walk selection for both calls.  Beyond 128 columns (ks > 4: sddmm_wide_kernel) only the per-window walk exists.
static SddmmRoute route_sddmm(const SddmmCall& c) {
    const tcgnn_plan* const plan = c.plan;
    SddmmRoute r;
    if (!plan->canonical) { r.walk = SddmmWalk::kCsr; return r; }
    const int mode = spmm_mode_of(plan), ks = c.ks(), pitch = x16_pitch(c.dpad());
    if (ks > 4) return r;
    // slice-synchronised range walk (r06, tcgnn_sync_walk.inc): communities larger than an XCD's L2; one launch per slice round, bit-identical scores
    if (!image_is_big(plan->Nc, pitch) && sync_chosen(plan, pitch * 2, mode, kSyncSddmm, c.dpad() / 16)) { r.walk = SddmmWalk::kSync; return r; }
    // Range-major walk (bit-identical results).  With the outputs staged per row the loop is bound by the gather again,
    // and keeping it inside ~4 MB column ranges wins on the Reddit shape: D=16 1.14 -> 1.07 ms, D=32 1.38 -> 1.14,
    // D=64 1.74 -> 1.66, D=128 3.37 -> 3.26.  No accumulators live across ranges, so ranges are 4x the SpMM's.
    const size_t x16_bytes = image_bytes(plan, pitch);
    if (!(plan->nbuckets > 0 && mode != 1 && (mode == 2 || range_walk_pays(plan, x16_bytes)))) return r;
    r.walk = SddmmWalk::kRangeMajor;
    // (r03, whole-line gathers: D = 64 1.26 / 1.24 ms at 4 / 8 MB ranges, 1.36 at 2 MB; D = 128 - an image of 60 MB - 2.33 at 2 MB,
    //  2.58 at 4 MB, 3.5 per-window; with XCD affinity 2.01 at 2 or 4 MB)
    r.nranges = range_count(plan, x16_bytes, x16_bytes > ((size_t)32 << 20) ? 2 * kRangeTargetBytes : 4 * kRangeTargetBytes);
    // XCD affinity (sddmm_kernel; TCGNN_SDDMM_XCD=0 switches it off, read per call: tests compare the two).  Reddit shape:
    // D = 128 2.32 -> 2.01 ms, D = 64 1.36 -> 1.33, D = 16 / 32 -1 .. -2.5 %; before the whole-line gathers it returned nothing.
    const char* const xenv = test_knob("TCGNN_SDDMM_XCD");
    // (like the fused kernel's sliced walk it wants every window's tiles spread evenly over the ranges: on the calibrated SBM graph -
    //  22.5 % of a window's edges inside its own community, near_frac 0.3 - the XCD that owns a window's community holds the others
    //  up, 1.43 -> 2.11 ms at D = 64, where an XCD has ONE range; with four ranges per XCD, spread over the graph, the load evens
    //  out again: D = 128 2.48 -> 2.25 ms there; TCGNN_SDDMM_XCD=2 forces it)
    const int xknob = xenv ? atoi(xenv) : 1;
    // (r06: that was the walk's window order, not the graph - `order` in its XCD-contiguous form hands a persistent wavefront windows of
    //  ONE eighth of the graph only, SddmmArgs::ident; with the windows taken in their own order every wavefront of an XCD is inside the
    //  same community at the same time, heavy or light together.  TCGNN_RM_IDENT=0 restores the old order for A/B runs)
    const char* const ienv = test_knob("TCGNN_RM_IDENT");
    r.ident = (ienv ? atoi(ienv) : 1) && windows_balanced(plan) ? 1 : 0;
    r.xcd = (xknob && (xknob >= 2 || r.ident || plan->near_frac <= 0.2 || r.nranges >= 4 * kXcds) && r.nranges % kXcds == 0 &&
             (c.H ? sddmm_heads_range_major_wgs(c, r.nranges) : sddmm_range_major_wgs(plan, ks, r.nranges)) >= kXcds) ? 1 : 0;
    return r;
}
// the kernel arguments every walk starts from (imw: tcgnn_sddmm2's window operand, empty for one operand)
static SddmmArgs sddmm_args(const SddmmCall& c, const StagedImage& im, const StagedImage& imw) {
    const tcgnn_plan* const plan = c.plan;
    SddmmArgs a{};
    a.wb_ptr = plan->d_wb_ptr; a.order = plan->d_order; a.cols = plan->d_cols; a.mask = plan->d_mask; a.ebase = plan->d_ebase;
    a.x16 = im.x16; a.hdr = im.hdr; a.ef = c.d_ef;
    a.N = plan->N; a.Nc = plan->Nc; a.row_off = plan->row_off; a.Dpad = im.dpad; a.stride = im.pitch;
    a.rowptr = plan->rowptr; a.bptr = plan->d_bptr; a.nbuckets = plan->nbuckets; a.nw = plan->nw_eff;
    a.big = image_is_big(plan->Nc, im.pitch);
    a.xa16 = imw.x16; a.hdr_a = imw.hdr;
    return a;
}
static hipError_t launch_sddmm_sync(const SddmmCall& c, SddmmArgs a) {
    const tcgnn_plan* const plan = c.plan;
    const int ks = c.ks();
    KernelTimer timer(plan, c.stream, c.H ? "sddmm_heads_kernel (slice-synchronised)" : "sddmm_kernel (slice-synchronised)");
    a.use_sync = 1;
    a.sync = sync_args(plan, a.stride * 2);
    const int per_cu = c.H ? sddmm_heads_wgs_per_cu(c) : sddmm_geom(ks, 4).wgs_per_cu();
    const int nwg = kXcds * std::max(1, std::min((plan->sync.S + 3) / 4, plan->num_cus / kXcds * per_cu));
    hipError_t e = hipSuccess;
    for (int r = 0; r < plan->sync.R && e == hipSuccess; ++r) {
        a.sync.round = r;
        e = c.H ? launch_sddmm_heads_passes<4, true>(c, a, nwg) : launch_sddmm_ks<4, true>(ks, a, nwg, c.stream);
    }
    return e;
}
static hipError_t launch_sddmm_range_major(const SddmmCall& c, const SddmmRoute& r, SddmmArgs a) {
    KernelTimer timer(c.plan, c.stream, c.H ? "sddmm_heads_kernel" : "sddmm_kernel");
    a.nranges = r.nranges;
    a.gsel = c.plan->nbuckets / r.nranges;
    a.ident = r.ident;
    a.xcd = r.xcd;
    int nwg = c.H ? sddmm_heads_range_major_wgs(c, r.nranges) : sddmm_range_major_wgs(c.plan, c.ks(), r.nranges);
    if (r.xcd) nwg -= nwg % kXcds;
    if (c.H) return launch_sddmm_heads_passes<4, true>(c, a, nwg);
    return launch_sddmm_ks<4, true>(c.ks(), a, nwg, c.stream);
}
static hipError_t launch_sddmm_per_window(const SddmmCall& c, const SddmmArgs& a) {
    const tcgnn_plan* const plan = c.plan;
    KernelTimer timer(plan, c.stream, c.H ? "sddmm_heads_kernel" : (c.ks() <= 4 ? "sddmm_kernel" : "sddmm_wide_kernel"));
    if (c.H) return plan->waves == 4 ? launch_sddmm_heads_passes<4, false>(c, a, plan->nw_eff) : launch_sddmm_heads_passes<1, false>(c, a, plan->nw_eff);
    return plan->waves == 4 ? launch_sddmm_ks<4, false>(c.ks(), a, plan->nw_eff, c.stream) : launch_sddmm_ks<1, false>(c.ks(), a, plan->nw_eff, c.stream);
}
// sddmm_heads_csr_kernel for all H heads of [.., H F] operands on `rows` rows: a capped grid, the kernel strides over rows and heads
static void launch_sddmm_heads_csr(const tcgnn_plan* plan, const uint32_t* hx, const uint32_t* hz, const float* d_X, const float* d_Z, float* d_ef, int32_t rows, int32_t H,
                                   int32_t F, hipStream_t stream) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(sddmm_heads_csr_kernel, dim3((unsigned)std::min((rows + 3) / 4, 2048), (unsigned)std::min(H, 1024)), dim3(256), 0, stream, hx, hz, plan->rowptr, plan->col,
                       d_X, d_Z, d_ef, rows, H, F, (int64_t)H * F, plan->E, plan->row_off);
}
// the range guard's tail, behind the launchers (returns at once unless X is "wide")
static int launch_sddmm_guard_tail(const SddmmCall& c, const StagedImage& im, const StagedImage& imw) {
    const tcgnn_plan* const plan = c.plan;
    if (c.ld) return TCGNN_OK;   // (a head's column block of tcgnn_sddmm_heads: ONE tail for all heads, behind the last of them - run_sddmm_heads)
    if (range_guard_of(plan) >= 2 && c.H) {   // tcgnn_sddmm_heads, fused: every head in ONE launch
        launch_sddmm_heads_csr(plan, imw.hdr, im.hdr, c.d_Xw, c.d_X, c.d_ef, patch_rows_of(plan), c.H, c.F, c.stream);
    } else if (range_guard_of(plan) >= 2 && c.d_Xw) {   // two operands: the whole call in fp32 when either is wide (sddmm2_wide; returns at once otherwise)
        // (the rows of the windows the plan was given: what lies behind them stays as the memset left it, as on the MFMA path)
        const int32_t rows = (int32_t)std::min<int64_t>(plan->N, (int64_t)plan->nw_eff * kWinRows);
        hipLaunchKernelGGL(sddmm2_csr_kernel, dim3((unsigned)std::min((rows + 3) / 4, 2048)), dim3(256), 0, c.stream, imw.hdr, im.hdr, plan->rowptr, plan->col, c.d_Xw, c.d_X, c.d_ef,
                           rows, c.D, plan->row_off);
    } else if (range_guard_of(plan) >= 2) {   // a few dirty rows: the patch behind the MFMA kernel; many: the CSR fallback (each returns at once otherwise)
        HIP_TRY(launch_wide_patch(patch_args(plan, im, c.d_X, c.d_ef, c.D, c.ws), c.stream));
    }
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}
// check, route, zero fill, stage, launch (each launcher's timer stops when it returns), the range guard's tail
static int run_sddmm(const SddmmCall& c) {
    const tcgnn_plan* const plan = c.plan;
    const int32_t D = c.D;
    if (plan->E == 0 || plan->N == 0) return TCGNN_OK;
    if (const int rc = check_workspace(c.name, c.ws, c.ws_bytes, c.d_Xw ? tcgnn_sddmm2_workspace_bytes(plan, D) : tcgnn_workspace_bytes(plan, D))) return rc;
    const SddmmRoute r = route_sddmm(c);
    if (r.walk == SddmmWalk::kCsr) {
        if (c.d_Xw) hipLaunchKernelGGL(sddmm2_csr_kernel, dim3((unsigned)((plan->N + 3) / 4)), dim3(256), 0, c.stream, (const uint32_t*)nullptr, (const uint32_t*)nullptr, plan->rowptr, plan->col, c.d_Xw, c.d_X, c.d_ef, plan->N, D, plan->row_off);
        else hipLaunchKernelGGL(sddmm_csr_kernel, dim3((unsigned)((plan->N + 3) / 4)), dim3(256), 0, c.stream, plan->rowptr, plan->col, c.d_X, c.d_ef, plan->N, D, plan->row_off);
        HIP_TRY(hipGetLastError());
        return TCGNN_OK;
    }
    if ((int64_t)plan->nw_eff * kWinRows < plan->N) HIP_TRY(hipMemsetAsync(c.d_ef, 0, (size_t)plan->E * std::max(c.H, 1) * sizeof(float), c.stream));
    const Guard gsd = guard_sddmm(plan, D);   // (a fused multi-head call: D = H F where a score has F terms - the conservative cap, one decision for every head)
    StageOpts so; so.guard = &gsd; so.ldx = c.ld; so.block_of_wider = c.hdr_filled;
    StagedImage im, imw;
    if (const int rc = stage_features(plan, c.d_X, nullptr, D, c.ws, c.ws_bytes, c.stream, so, &im)) return rc;
    if (c.d_Xw) {   // the window operand's image behind the gathered operand's: its own header, its own scale
        const size_t first = workspace_bytes_for(plan->Nc, D);
        if (c.ws_bytes < 2 * first) return fail(TCGNN_ERR_WORKSPACE, "tcgnn_sddmm2: workspace needs %zu bytes (tcgnn_sddmm2_workspace_bytes), got %zu", 2 * first, c.ws_bytes);
        if (const int rc = stage_features(plan, c.d_Xw, nullptr, D, static_cast<char*>(c.ws) + first, c.ws_bytes - first, c.stream, so, &imw)) return rc;
    }
    const SddmmArgs a = sddmm_args(c, im, imw);
    const hipError_t e = r.walk == SddmmWalk::kSync ? launch_sddmm_sync(c, a) : (r.walk == SddmmWalk::kRangeMajor ? launch_sddmm_range_major(c, r, a) : launch_sddmm_per_window(c, a));
    HIP_TRY(e);
    return launch_sddmm_guard_tail(c, im, imw);
}

// ------------------------------------------------------------------------------------------
// tcgnn_sddmm_heads: ef[h, e] = <X[row e, hF:(h+1)F], Z[col e, hF:(h+1)F]> for H heads, ef [H, E] head-major.  One decision
// (route_sddmm_heads), from the plan and (H, F) alone, before anything is staged; tcgnn_sddmm_heads_workspace_bytes asks the same function.
// ------------------------------------------------------------------------------------------
struct SddmmHeadsCall {
    const tcgnn_plan* plan = nullptr;
    const float *d_X = nullptr, *d_Z = nullptr;   // X: the window operand, Z: the gathered one; both [Nc, H F]
    float* d_ef = nullptr;                        // [H, E]
    int32_t H = 0, F = 0;
    void* ws = nullptr; size_t ws_bytes = 0;
    hipStream_t stream = nullptr;
};
// kSingle: H == 1 is tcgnn_sddmm2 itself (run_sddmm, every walk it has); kFused: sddmm_kernel's multi-head form ("sddmm_heads_kernel") on
// route_sddmm's walk at width H F - each operand staged once, one walk of the tile stream per pass of up to four heads; kCsr: a plan
// without a tile stream, or fewer than four edges - sddmm_heads_csr_kernel, all heads in one launch; kPerHead: head by head inside the
// library - each head a column block of X and Z (run_sddmm with ld, the headers filled once over the whole matrices) into its row of ef
enum class SddmmHeadsWay { kSingle, kFused, kCsr, kPerHead };
// the fused form's head widths (each with 2 .. 4 heads a pass, F = 64 with 2: launch_sddmm_heads); H F <= 128, and an image one
// buffer descriptor addresses (the big-image lane addresses stay the single-head kernel's)
static bool sddmm_heads_fused_width(int32_t F) { return F == 8 || F == 16 || F == 32 || F == 64; }
static SddmmHeadsWay route_sddmm_heads(const tcgnn_plan* plan, int32_t H, int32_t F) {
    if (H == 1) return SddmmHeadsWay::kSingle;
    if (!plan->canonical || plan->E < 4) return SddmmHeadsWay::kCsr;
    const int64_t D = (int64_t)H * F;
    if (sddmm_heads_fused_width(F) && D <= 128 && plan->nw_eff > 0 && !image_is_big(plan->Nc, x16_pitch(round_up((int)D, 16)))) return SddmmHeadsWay::kFused;
    return SddmmHeadsWay::kPerHead;
}
static size_t sddmm_heads_workspace_bytes(const tcgnn_plan* plan, int32_t H, int32_t F) {
    switch (route_sddmm_heads(plan, H, F)) {
        case SddmmHeadsWay::kSingle: return tcgnn_sddmm2_workspace_bytes(plan, F);
        case SddmmHeadsWay::kFused:  return 2 * workspace_bytes_for(plan->Nc, H * F);   // the two images of all columns
        // two images of one head's block at a time.  (kCsr stages nothing, but is handed the same buffer: what a caller must
        //  provide is checked alike on every route)
        default:                     return 2 * workspace_bytes_for(plan->Nc, F);
    }
}
static int run_sddmm_heads(const SddmmHeadsCall& h) {
    const tcgnn_plan* const plan = h.plan;
    if (!plan || h.H < 1 || h.F < 1 || (int64_t)h.H * h.F > INT32_MAX) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_sddmm_heads: null plan, H < 1, F < 1 or H * F beyond int32");
    if (plan->E > 0 && plan->N > 0 && !(h.d_X && h.d_Z && h.d_ef)) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_sddmm_heads: null array");
    if (plan->E == 0 || plan->N == 0) return TCGNN_OK;
    const int32_t D = h.H * h.F;
    SddmmCall c;
    c.plan = plan; c.d_Xw = h.d_X; c.d_X = h.d_Z; c.d_ef = h.d_ef; c.ws = h.ws; c.ws_bytes = h.ws_bytes; c.stream = h.stream; c.name = "tcgnn_sddmm_heads";
    const SddmmHeadsWay way = route_sddmm_heads(plan, h.H, h.F);
    if (way == SddmmHeadsWay::kSingle) { c.D = h.F; return run_sddmm(c); }   // exactly tcgnn_sddmm2
    if (const int rc = check_workspace("tcgnn_sddmm_heads", h.ws, h.ws_bytes, sddmm_heads_workspace_bytes(plan, h.H, h.F))) return rc;
    if (way == SddmmHeadsWay::kFused) { c.D = D; c.H = h.H; c.F = h.F; return run_sddmm(c); }
    if (way == SddmmHeadsWay::kCsr) {
        // (a canonical plan: the rows of the windows it was handed, what lies behind them zero; a non-canonical one has no windows - every row)
        const int32_t rows = plan->canonical ? patch_rows_of(plan) : plan->N;
        if (rows < plan->N) HIP_TRY(hipMemsetAsync(h.d_ef, 0, (size_t)plan->E * h.H * sizeof(float), h.stream));
        launch_sddmm_heads_csr(plan, nullptr, nullptr, h.d_X, h.d_Z, h.d_ef, rows, h.H, h.F, h.stream);
        HIP_TRY(hipGetLastError());
        return TCGNN_OK;
    }
    // head by head: ONE abs-max per operand for the whole call (every head rounded with the scales the fused walk would use), Z's
    // header where run_sddmm stages the gathered operand and X's where it stages the window operand of an F-column call
    const Guard gsd = guard_sddmm(plan, D);
    const size_t first = workspace_bytes_for(plan->Nc, h.F);
    if (const int rc = fill_header(plan, static_cast<uint32_t*>(h.ws), h.d_Z, nullptr, nullptr, D, gsd, nullptr, 0, h.stream)) return rc;
    if (const int rc = fill_header(plan, reinterpret_cast<uint32_t*>(static_cast<char*>(h.ws) + first), h.d_X, nullptr, nullptr, D, gsd, nullptr, 0, h.stream)) return rc;
    for (int k = 0; k < h.H; ++k) {
        SddmmCall b = c;
        b.d_Xw = h.d_X + (int64_t)k * h.F; b.d_X = h.d_Z + (int64_t)k * h.F; b.d_ef = h.d_ef + (int64_t)k * plan->E;
        b.D = h.F; b.ld = D; b.hdr_filled = true;
        if (const int rc = run_sddmm(b)) return rc;
    }
    // the range guard's tail, ONE launch behind the last head for all of them.  Every head's MFMA kernel asked sddmm2_wide with the
    // lost-element counts of the blocks converted so far; the counts only grow and the rule is monotone in them, so where any head's
    // kernel stood back the tail - which sees the whole call's counts - does the work, and where it runs it rewrites every head
    if (range_guard_of(plan) >= 2)
        launch_sddmm_heads_csr(plan, reinterpret_cast<const uint32_t*>(static_cast<char*>(h.ws) + first), static_cast<const uint32_t*>(h.ws), h.d_X, h.d_Z, h.d_ef,
                               patch_rows_of(plan), h.H, h.F, h.stream);
    HIP_TRY(hipGetLastError());
    return TCGNN_OK;
}
