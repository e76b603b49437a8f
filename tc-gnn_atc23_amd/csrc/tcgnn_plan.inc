// tcgnn_plan.inc - the plan's lifetime: tcgnn_plan_create[_sharded] as a sequence of named steps, tcgnn_plan_destroy, tcgnn_plan_get_info,
// tcgnn_plan_prepare[_val], kernel timing, and the mode / range-guard setters.  Included by tcgnn_device.hip behind the dispatchers,
// whose predicates tcgnn_plan_prepare[_val] ask (lds_wanted, ensure_lds_streams, val_lds_wanted, ensure_val_stream); struct tcgnn_plan
// itself is in tcgnn_device.hip, the plan-time kernels in tcgnn_pack.inc, the cell-stream builds in tcgnn_lds_plan.inc.

// ---- tables of the slice-synchronised range walk (tcgnn_sync_walk.inc), built at plan creation for graphs whose numbering has
// locality (near_frac > 0.5: the walks that rely on it are the ones this one replaces) and whose windows are alike.  Two small kernels, one
// histogram copied to the host (slices x fine buckets words), one table of (kmax + 1) words per window.  Any failure leaves sync.ok false:
// the walk is an optional acceleration, the per-window walk needs nothing from here.
static int build_sync_tables(tcgnn_plan* p, hipStream_t stream) {
    tcgnn_plan::SyncTables& t = p->sync;
    const int nw = p->nw_eff;
    if (nw < kXcds * 256 || !p->d_cols || p->total_wb < 1) return TCGNN_OK;
    const bool verbose = verbose_level() > 0;
    t.nwx = (nw + kXcds - 1) / kXcds;
    t.S = kSyncSlice;
    t.R = (t.nwx + t.S - 1) / t.S;
    t.kmax = kSyncKmax;
    const int nslices = kXcds * t.R;
    const int nfb0 = (int)((((int64_t)p->Nc + 1) >> kSyncFbShift0) + 1);
    DevBuf<uint32_t> d_hist;
    std::vector<uint32_t> hist((size_t)nslices * nfb0);
    hipError_t e = d_hist.alloc(hist.size());
    if (e == hipSuccess) e = hipMemsetAsync(d_hist, 0, hist.size() * sizeof(uint32_t), stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(sync_hist_kernel, dim3((unsigned)nw), dim3(64), 0, stream, p->d_wb_ptr, p->d_cols, nw, t.nwx, t.S, t.R, kSyncFbShift0, nfb0, d_hist.ptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(hist.data(), d_hist, hist.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    d_hist.reset();
    if (e != hipSuccess) { (void)hipGetLastError(); return TCGNN_OK; }
    // hot buckets per slice: at least a quarter of a tile per window of the slice; coarser buckets until every slice's list fits
    std::vector<int32_t> hot((size_t)nslices * t.kmax, 0x7fffffff >> 12), nk((size_t)nslices, 0);
    int shift = -1;
    double tiles_all = 0, tiles_hot = 0, k_weighted = 0;
    for (int sh = 0; sh <= 5 && shift < 0; ++sh) {
        const int nfb = (nfb0 + (1 << sh) - 1) >> sh;
        bool fits = true;
        tiles_all = tiles_hot = k_weighted = 0;
        t.max_k = 0;
        for (int s = 0; s < nslices && fits; ++s) {
            const int x = s / t.R, r = s % t.R;
            const int64_t lo = (int64_t)x * t.nwx + (int64_t)r * t.S, hi = std::min<int64_t>(std::min<int64_t>(lo + t.S, (int64_t)(x + 1) * t.nwx), nw);
            const int64_t wins = std::max<int64_t>(hi - lo, 0);
            const uint32_t thr = (uint32_t)std::max<int64_t>(wins / 4, 16);
            int k = 0;
            double all = 0, hsum = 0;
            for (int b = 0; b < nfb; ++b) {
                uint64_t c = 0;
                for (int q = b << sh; q < std::min(nfb0, (b + 1) << sh); ++q) c += hist[(size_t)s * nfb0 + q];
                all += (double)c;
                if (c >= thr) {
                    if (k == t.kmax) { fits = false; break; }
                    hot[(size_t)s * t.kmax + k++] = b;
                    hsum += (double)c;
                }
            }
            nk[(size_t)s] = k;
            t.max_k = std::max(t.max_k, k);
            tiles_all += all; tiles_hot += hsum; k_weighted += all * k;
        }
        if (fits) shift = sh;
    }
    if (shift < 0 || tiles_all <= 0) {
        if (verbose) fprintf(stderr, "[tcgnn] sync walk: hot buckets do not fit %d entries per slice at any bucket size: not built\n", t.kmax);
        return TCGNN_OK;
    }
    t.fb_shift = kSyncFbShift0 + shift;
    t.hot_frac = tiles_hot / tiles_all;
    t.avg_k = k_weighted / tiles_all;
    if (verbose)
        fprintf(stderr, "[tcgnn] sync walk: %d slices of %d windows, buckets of %d rows, %.1f hot buckets per slice (max %d), %.0f %% of the tiles inside them\n", nslices, t.S,
                1 << t.fb_shift, t.avg_k, t.max_k, 100.0 * t.hot_frac);
    if (t.hot_frac < 0.5) return TCGNN_OK;
    DevBuf<int32_t> d_hot, d_nk;
    DevBuf<uint32_t> d_T;
    e = d_hot.alloc(hot.size());
    if (e == hipSuccess) e = d_nk.alloc(nk.size());
    if (e == hipSuccess) e = d_T.alloc((size_t)nw * (t.kmax + 1));
    if (e == hipSuccess) e = hipMemcpyAsync(d_hot, hot.data(), hot.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_nk, nk.data(), nk.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
        const int64_t total = (int64_t)nw * (t.kmax + 1);
        hipLaunchKernelGGL(sync_table_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, p->d_wb_ptr, p->d_cols, nw, t.nwx, t.S, t.R, t.kmax, t.fb_shift, d_hot.ptr, d_nk.ptr, d_T.ptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);   // (host vectors above must outlive the copies)
    if (e != hipSuccess) { (void)hipGetLastError(); return TCGNN_OK; }
    p->bytes += d_T.release(t.d_T) + d_nk.release(t.d_nk);
    t.ok = true;
    return TCGNN_OK;
}

// ---- plan creation in nine steps.  Each step returns an error code; the plan under construction is destroyed by the caller on any.
// step 1: blockPartition (the window weights) and the longest row - what the range guard's bound follows (guard_spmm) - to the host
static int plan_read_weights(tcgnn_plan* p, hipStream_t stream, std::vector<int32_t>* bp) {
    const int nw = p->nw_eff;
    bp->assign((size_t)nw, 0);
    if (nw <= 0) return TCGNN_OK;
    DevBuf<uint32_t> d_maxdeg;
    uint32_t h_maxdeg = 0;
    hipError_t e = d_maxdeg.alloc(1);
    if (e == hipSuccess) e = hipMemsetAsync(d_maxdeg, 0, sizeof(uint32_t), stream);
    if (e == hipSuccess && p->N > 0) {
        hipLaunchKernelGGL(max_degree_kernel, dim3((unsigned)std::min<int64_t>(1024, ((int64_t)p->N + 255) / 256)), dim3(256), 0, stream, p->rowptr, p->N, d_maxdeg.ptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&h_maxdeg, d_maxdeg, sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(bp->data(), p->bp, (size_t)nw * sizeof(int32_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(TCGNN_ERR_HIP, "read blockPartition: %s", hipGetErrorString(e));
    p->max_degree = (int32_t)std::min<uint32_t>(h_maxdeg, 0x7fffffffu);
    return TCGNN_OK;
}
// step 2 (host): the wide blocks (four 16x8 blocks each) of every window; one or four wavefronts per window
static int plan_count_blocks(tcgnn_plan* p, const std::vector<int32_t>& bp, std::vector<int64_t>* wb_ptr) {
    const int nw = p->nw_eff;
    wb_ptr->assign((size_t)nw + 1, 0);
    for (int w = 0; w < nw; ++w) {
        if (bp[(size_t)w] < 0) return fail(TCGNN_ERR_BAD_GRAPH, "blockPartition[%d] = %d is negative", w, bp[(size_t)w]);
        p->tc_blocks += bp[(size_t)w];
        (*wb_ptr)[(size_t)w + 1] = (*wb_ptr)[(size_t)w] + (bp[(size_t)w] + 3) / 4;
        p->max_wb = std::max<int64_t>(p->max_wb, (bp[(size_t)w] + 3) / 4);
    }
    p->total_wb = (*wb_ptr)[(size_t)nw];
    p->waves = (nw > 0 && p->total_wb >= (int64_t)6 * nw) ? 4 : 1;
    return TCGNN_OK;
}
// step 3 (host, no HIP call: a pure function of the window weights): the block -> window map of the per-window gather walks.
// Heaviest first keeps a hub window from starting last; but when no window is far above the mean the order is free, and then locality
// decides: workgroup b runs on XCD b % 8 (observed dispatch, used for speed only), so XCD x takes the x-th contiguous eighth of the
// windows in their own order - the workgroups resident on one XCD at one time are neighbours in the graph's numbering and share their
// gathered rows in that XCD's L2 (communities).
static std::vector<int32_t> order_windows(const std::vector<int32_t>& bp, int64_t tc_blocks) {
    const int nw = (int)bp.size();
    std::vector<int32_t> order((size_t)nw);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return bp[(size_t)x] > bp[(size_t)y]; });
    int64_t mx = 0;
    for (int w = 0; w < nw; ++w) mx = std::max<int64_t>(mx, bp[(size_t)w]);
    const bool balanced = nw > 0 && mx * nw <= 4 * std::max<int64_t>(tc_blocks, 1);
    // A few hubs over an otherwise even graph (communities + hubs): the K windows more than 4x the mean start first, heaviest first
    // (the round-robin dispatch spreads them over the XCDs), the rest follows in XCD-contiguous order.  A continuous skew
    // (R-MAT: the weight falls with the id, the rest is not even either) keeps heaviest-first throughout.
    int K = 0;
    if (!balanced && nw >= 64) {
        const int64_t mean_x4 = 4 * std::max<int64_t>(tc_blocks, 1) / nw + 1;
        while (K < nw && bp[(size_t)order[(size_t)K]] > mean_x4) ++K;
        int64_t rest = 0, rest_max = 0;
        for (int q = K; q < nw; ++q) { rest += bp[(size_t)order[(size_t)q]]; rest_max = std::max<int64_t>(rest_max, bp[(size_t)order[(size_t)q]]); }
        if (K > nw / 16 || rest_max * (int64_t)(nw - K) > 3 * std::max<int64_t>(rest, 1)) K = -1;   // not "a few hubs": keep heaviest-first
    }
    if (nw < 64 || !(balanced || K > 0)) return order;
    std::vector<int32_t> rest;                                   // the windows behind the hubs, in their own order
    {
        std::vector<char> is_hub((size_t)nw, 0);
        for (int q = 0; q < K; ++q) is_hub[(size_t)order[(size_t)q]] = 1;
        for (int w = 0; w < nw; ++w) if (!is_hub[(size_t)w]) rest.push_back(w);
    }
    // every XCD takes one contiguous eighth: the eighths must weigh about the same (a degree that falls with the id -
    // R-MAT - would hand XCD 0 the heavy end: ogbn-products shape 3.96 -> 4.54 ms), else heaviest-first stays
    int64_t part[kXcds] = {0}, all = 0;
    for (size_t q = 0; q < rest.size(); ++q) { part[q * kXcds / rest.size()] += bp[(size_t)rest[q]]; all += bp[(size_t)rest[q]]; }
    for (int x = 0; x < kXcds; ++x) if (part[x] * kXcds > all + all / 8) return order;
    int cnt[kXcds] = {0}, start[kXcds + 1] = {0}, seen[kXcds] = {0};
    for (int b = K; b < nw; ++b) ++cnt[b % kXcds];                   // positions XCD x gets behind the hubs
    for (int x = 0; x < kXcds; ++x) start[x + 1] = start[x] + cnt[x];
    for (int b = K; b < nw; ++b) { const int x = b % kXcds; order[(size_t)b] = rest[(size_t)(start[x] + seen[x]++)]; }
    return order;
}
// step 4: the packed tile stream (pack_kernel); flags: ids out of range, rows that are not strictly increasing (not canonical)
static int plan_allocate_and_pack(tcgnn_plan* p, hipStream_t stream, const std::vector<int64_t>& wb_ptr, const std::vector<int32_t>& order) {
    const int nw = p->nw_eff;
    const size_t n_wb = (size_t)std::max<int64_t>(p->total_wb, 1);
    const size_t b_ptr = ((size_t)nw + 1) * sizeof(int64_t), b_ord = (size_t)std::max(nw, 1) * sizeof(int32_t);
    const size_t b_cols = n_wb * kWbCols * sizeof(int32_t), b_mask = n_wb * kWinRows * sizeof(uint32_t), b_eb = n_wb * kWinRows * sizeof(int32_t);
    DevBuf<int32_t> d_flags;
    hipError_t e = hipMalloc(&p->d_wb_ptr, b_ptr);
    if (e == hipSuccess) e = hipMalloc(&p->d_order, b_ord);
    if (e == hipSuccess) e = hipMalloc(&p->d_cols, b_cols);
    if (e == hipSuccess) e = hipMalloc(&p->d_mask, b_mask);
    if (e == hipSuccess) e = hipMalloc(&p->d_ebase, b_eb);
    if (e == hipSuccess) e = d_flags.alloc(2);
    if (e != hipSuccess) { return fail(hip_rc(e), "plan allocation (%zu bytes): %s", b_ptr + b_ord + b_cols + b_mask + b_eb, hipGetErrorString(e)); }
    p->bytes = b_ptr + b_ord + b_cols + b_mask + b_eb;
    int32_t flags[2] = {0, 0};
    e = hipMemcpyAsync(p->d_wb_ptr, wb_ptr.data(), b_ptr, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && nw > 0) e = hipMemcpyAsync(p->d_order, order.data(), (size_t)nw * sizeof(int32_t), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_flags, 0, 2 * sizeof(int32_t), stream);
    if (e == hipSuccess && nw > 0) {
        hipLaunchKernelGGL(pack_kernel, dim3((unsigned)nw), dim3(256), 0, stream, p->rowptr, p->col, p->e2c, p->e2r, p->d_wb_ptr, p->N, p->Nc, p->d_cols, p->d_mask, p->d_ebase, d_flags.ptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(flags, d_flags, sizeof flags, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream); // the host vectors must outlive the copies
    if (e != hipSuccess) return fail(TCGNN_ERR_HIP, "plan build: %s", hipGetErrorString(e));
    if (flags[0]) return fail(TCGNN_ERR_BAD_GRAPH, "edgeToColumn / edgeToRow / edgeList hold ids outside the window, blockPartition or node range");
    p->canonical = flags[1] ? 0 : 1;
    return TCGNN_OK;
}
// step 5: is the graph structurally symmetric?  (The range guard's patch walks a few dirty rows' edges AND their mirrors instead of scanning
// every column id, where it is: wide_patch_kernel.)  One thread per edge, a binary search each; the answer stays on the device.
static int plan_symmetry(tcgnn_plan* p, hipStream_t stream) {
    if (!(p->canonical && p->N == p->Nc && p->row_off == 0 && p->E > 0)) return TCGNN_OK;
    hipError_t e = hipMalloc(&p->d_sym, 2 * sizeof(int32_t));   // [answer, (edges above the diagonal) - (edges below)]
    static const int32_t sym_init[2] = {1, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(p->d_sym, sym_init, sizeof sym_init, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(symmetry_kernel, dim3((unsigned)((p->E + 255) / 256)), dim3(256), 0, stream, p->rowptr, p->col, p->e2r, p->E, p->N, p->d_sym);
        hipLaunchKernelGGL(symmetry_finish_kernel, dim3(1), dim3(1), 0, stream, p->d_sym);
        e = hipGetLastError();   // (no synchronisation: nothing on the host waits for the answer - the patch kernels read it on the device)
    }
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? TCGNN_ERR_OOM : TCGNN_ERR_HIP, "plan build (symmetry): %s", hipGetErrorString(e));
    return TCGNN_OK;
}
// step 6: near_frac, the share of the condensed columns within num_cols / 16 rows of their window (has_locality)
static int plan_locality(tcgnn_plan* p, hipStream_t stream) {
    const int nw = p->nw_eff;
    if (nw <= 0) return TCGNN_OK;
    DevBuf<unsigned long long> d_loc;
    unsigned long long h_loc[2] = {0, 0};
    hipError_t e = d_loc.alloc(2);
    if (e == hipSuccess) e = hipMemsetAsync(d_loc, 0, sizeof h_loc, stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(locality_kernel, dim3((unsigned)nw), dim3(256), 0, stream, p->d_wb_ptr, p->d_cols, nw, p->Nc, p->row_off, std::max(p->Nc / 16, kWinRows), d_loc.ptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_loc, d_loc, sizeof h_loc, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(TCGNN_ERR_HIP, "plan build (locality): %s", hipGetErrorString(e));
    p->near_frac = h_loc[1] ? (double)h_loc[0] / (double)h_loc[1] : 0.0;
    if (verbose_level() > 0) fprintf(stderr, "[tcgnn] plan: %.0f %% of the condensed columns lie within num_cols / 16 rows of their window\n", 100.0 * p->near_frac);
    return TCGNN_OK;
}
// step 7: column buckets for the range-blocked SpMM: only when windows are long (>= 2 tiles per bucket on average) and numerous
// enough to fill the chip with one wavefront per 4 windows
static int plan_bucket_table(tcgnn_plan* p, hipStream_t stream) {
    const int nw = p->nw_eff;
    hipDeviceProp_t prop;
    int devid = 0;
    if (hipGetDevice(&devid) == hipSuccess && hipGetDeviceProperties(&prop, devid) == hipSuccess) p->num_cus = prop.multiProcessorCount;
    int nb = 8;
    while (nb < 128 && (int64_t)p->Nc / nb > 4096) nb <<= 1;
    // wide column spaces with short windows (a row shard of a multi-GPU graph: Reddit's 243 tiles per window spread over
    // N x 232 965 columns): fewer, longer buckets rather than no table - without it the shard falls back to the per-window
    // walk (measured 1.77 ms against 0.87 ms for the unsharded graph)
    while (nb > 8 && p->total_wb < (int64_t)g_bucket_min_tiles * nb * nw) nb >>= 1;
    if (!(nw >= 4 * p->num_cus && p->total_wb >= (int64_t)g_bucket_min_tiles * nb * nw)) return TCGNN_OK;
    p->nbuckets = nb;
    p->bucket_rows = (int32_t)(((int64_t)p->Nc + nb - 1) / nb);
    if (p->bucket_rows < 1) p->bucket_rows = 1;
    const size_t b_bp = (size_t)nw * (nb + 1) * sizeof(uint32_t);
    hipError_t e = hipMalloc(&p->d_bptr, b_bp);
    if (e == hipSuccess) {
        const int64_t total = (int64_t)nw * (nb + 1);
        hipLaunchKernelGGL(bucket_ptr_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, p->d_wb_ptr, p->d_cols, nw, nb,
                           p->bucket_rows, p->d_bptr);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
    }
    if (e != hipSuccess) return fail(TCGNN_ERR_HIP, "bucket table: %s", hipGetErrorString(e));
    p->bytes += b_bp;
    return TCGNN_OK;
}
// step 9 (step 8 is build_sync_tables, above): the cell stream of the LDS-resident column-range SpMM (tcgnn_lds_spmm.inc) when the time models
// pick that kernel for a 64-column matrix: built now rather than inside the first call.  Other widths decide, and build, at their
// first call.  TCGNN_LDS_AUTO=0 disables the automatic choice.
static int plan_first_cell_streams(tcgnn_plan* p, hipStream_t stream) {
    if (!lds_chosen(p, 64)) return TCGNN_OK;
    LdsPass passes[2];
    const int np = lds_passes(64, passes);
    for (int i = 0; i < np; ++i) {
        const int rc = build_lds_cells(p, stream, lds_stream_of(passes[i].nt, passes[i].maxw));   // (slot 4: or the 952-row slot 7, if the build prices that lower)
        if (rc == TCGNN_ERR_OOM) { p->lds_choice[4] = 0; break; }   // (the gather walks need no stream)
        if (rc) return rc;
    }
    return TCGNN_OK;
}

// the one-pass staging's guess words and counters (tcgnn_stage.inc): "no guess" everywhere, no call counted
static int plan_stage_words(tcgnn_plan* p, hipStream_t stream) {
    hipError_t e = hipMalloc(&p->d_stage, kStageWords * sizeof(uint32_t));
    if (e != hipSuccess) { p->d_stage = nullptr; return fail(hip_rc(e), "plan build (staging words): %s", hipGetErrorString(e)); }
    e = hipMemsetAsync(p->d_stage, 0, kStageWords * sizeof(uint32_t), stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(TCGNN_ERR_HIP, "plan build (staging words): %s", hipGetErrorString(e));
    p->bytes += kStageWords * sizeof(uint32_t);
    return TCGNN_OK;
}

extern "C" {

int tcgnn_plan_destroy(tcgnn_plan* plan) {
    if (!plan) return TCGNN_OK;
    (void)hipFree(plan->d_wb_ptr); (void)hipFree(plan->d_order); (void)hipFree(plan->d_cols);
    (void)hipFree(plan->d_mask); (void)hipFree(plan->d_ebase); (void)hipFree(plan->d_bptr);
    (void)hipFree(plan->sync.d_T); (void)hipFree(plan->sync.d_nk);
    for (auto& cs : plan->lds) release_cell_stream(cs);
    (void)hipFree(plan->d_xwb_ptr); (void)hipFree(plan->d_xcols); (void)hipFree(plan->d_xmask); (void)hipFree(plan->d_xeidx); (void)hipFree(plan->d_sym);
    (void)hipFree(plan->d_stage);
    for (hipEvent_t e : plan->ev) (void)hipEventDestroy(e);
    delete plan;
    return TCGNN_OK;
}

int tcgnn_plan_create_sharded(const int32_t* d_nodePointer, const int32_t* d_edgeList,
                              const int32_t* d_blockPartition, const int32_t* d_edgeToColumn,
                              const int32_t* d_edgeToRow, int32_t num_rows, int32_t num_cols,
                              int32_t row_offset, int64_t num_edges, int32_t num_windows,
                              void* stream_v, tcgnn_plan** plan_out) {
    if (!plan_out) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_plan_create: plan_out is null");
    *plan_out = nullptr;
    const int32_t num_nodes = num_rows;
    if (num_cols < 0 || row_offset < 0 || (int64_t)row_offset + num_rows > (int64_t)num_cols)
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_plan_create: rows [%d, %d) do not fit in %d feature rows", row_offset, row_offset + num_rows, num_cols);
    if (num_nodes < 0 || num_edges < 0 || num_windows < 0 || !d_nodePointer ||
        (num_windows > 0 && !d_blockPartition) || (num_edges > 0 && (!d_edgeList || !d_edgeToColumn || !d_edgeToRow)))
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_plan_create: null array or negative size");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    tcgnn_plan* p = new (std::nothrow) tcgnn_plan();
    if (!p) return fail(TCGNN_ERR_OOM, "tcgnn_plan_create: host allocation failed");
    p->N = num_nodes; p->Nc = num_cols; p->row_off = row_offset; p->E = num_edges; p->nw = num_windows;
    p->nw_eff = (int32_t)std::min<int64_t>(num_windows, ((int64_t)num_nodes + kWinRows - 1) / kWinRows);
    p->rowptr = d_nodePointer; p->col = d_edgeList; p->bp = d_blockPartition; p->e2c = d_edgeToColumn; p->e2r = d_edgeToRow;
    auto bail = [&](int rc) { tcgnn_plan_destroy(p); return rc; };
    // TCGNN_VERBOSE=2: where plan creation spends its time (each mark synchronises the stream: a measurement aid, not the product's behaviour)
    const bool vtime = verbose_level() >= 2;
    auto t_last = std::chrono::steady_clock::now();
    auto mark = [&](const char* what) {
        if (!vtime) return;
        (void)hipStreamSynchronize(stream);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[tcgnn] plan_create: %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    };
    if (const int rc = plan_stage_words(p, stream)) return bail(rc);
    std::vector<int64_t> wb_ptr;
    if (const int rc = plan_read_weights(p, stream, &p->h_bp)) return bail(rc);   // (h_bp stays: the placement of the LDS-resident walks weighs windows by it)
    mark("blockPartition to the host");
    if (const int rc = plan_count_blocks(p, p->h_bp, &wb_ptr)) return bail(rc);
    const std::vector<int32_t> order = order_windows(p->h_bp, p->tc_blocks);
    mark("window order (host)");
    if (const int rc = plan_allocate_and_pack(p, stream, wb_ptr, order)) return bail(rc);
    mark("allocate + pack_kernel");
    if (const int rc = plan_symmetry(p, stream)) return bail(rc);
    mark("symmetry_kernel");
    if (const int rc = plan_locality(p, stream)) return bail(rc);
    mark("locality_kernel");
    if (const int rc = plan_bucket_table(p, stream)) return bail(rc);
    mark("bucket table");
    if (has_locality(p) && windows_balanced(p)) (void)build_sync_tables(p, stream);
    mark("sync-walk tables");
    if (const int rc = plan_first_cell_streams(p, stream)) return bail(rc);
    mark("LDS cell streams (64 columns)");
    *plan_out = p;
    return TCGNN_OK;
}

int tcgnn_plan_create(const int32_t* d_nodePointer, const int32_t* d_edgeList,
                      const int32_t* d_blockPartition, const int32_t* d_edgeToColumn,
                      const int32_t* d_edgeToRow, int32_t num_nodes, int64_t num_edges,
                      int32_t num_windows, void* stream, tcgnn_plan** plan_out) {
    return tcgnn_plan_create_sharded(d_nodePointer, d_edgeList, d_blockPartition, d_edgeToColumn, d_edgeToRow, num_nodes,
                                     num_nodes, 0, num_edges, num_windows, stream, plan_out);
}

int tcgnn_plan_get_info(const tcgnn_plan* plan, tcgnn_plan_info* info) {
    if (!plan || !info) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_plan_get_info: null argument");
    info->num_nodes = plan->N; info->num_windows = plan->nw; info->num_edges = plan->E;
    info->tc_blocks = plan->tc_blocks; info->wide_blocks = plan->total_wb; info->plan_bytes = (int64_t)plan->bytes;
    info->canonical = plan->canonical; info->waves_per_window = plan->waves;
    info->column_buckets = plan->nbuckets; info->lds_ranges = 0;
    for (int i = 0; i < kLdsStreams; ++i) if (plan->lds[i].nranges > info->lds_ranges) info->lds_ranges = plan->lds[i].nranges;   // finest stream built so far
    return TCGNN_OK;
}

int tcgnn_plan_prepare(tcgnn_plan* plan, int32_t D, void* stream_v) {
    if (!plan || D < 1) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_plan_prepare: null plan or D < 1");
    if (plan->nw_eff <= 0 || plan->N == 0) return TCGNN_OK;
    const int dpad = round_up(D, 16);
    const int mode = spmm_mode_of(plan);
    // (the gather walks need nothing built, nor does the single-launch kernel: route_spmm's bound for it, applied here on the assumption
    //  of a plain call - the calls that kernel does not take, staged or with the dense update, build their streams when they come)
    if (mode == 0 && plan->total_wb <= kSmallMaxTiles) return TCGNN_OK;
    if (!lds_wanted(plan, mode, dpad) || !planar_records_fit(plan, dpad)) return TCGNN_OK;
    LdsPass passes[2];
    bool ok;
    return ensure_lds_streams(plan, static_cast<hipStream_t>(stream_v), mode, dpad, passes, lds_passes(dpad, passes), LdsBuild::kPrepare, &ok);
}

// Builds, now, what the first tcgnn_spmm_val call of width D would build inside the hot path: the single-edge cell stream of the
// LDS-resident edge-valued walk (tcgnn_lds_val.inc) where the plan's time model takes that walk for D.  After it tcgnn_workspace_bytes
// already includes the slot values, so the FIRST forward_AGNN (gnn_conv.py:132) runs the LDS-resident kernels and neither allocates nor
// synchronises (VERDICT r04 item 6 ii).
int tcgnn_plan_prepare_val(tcgnn_plan* plan, int32_t D, void* stream_v) {
    if (!plan || D < 1) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_plan_prepare_val: null plan or D < 1");
    if (plan->nw_eff <= 0 || plan->N == 0 || plan->E < 4 || !plan->canonical) return TCGNN_OK;
    const int dp = round_up(D, 16), mode = spmm_mode_of(plan);
    if (!val_lds_wanted(plan, mode, dp)) return TCGNN_OK;
    return ensure_val_stream(plan, static_cast<hipStream_t>(stream_v), mode, false);
}

int tcgnn_plan_set_spmm_mode(tcgnn_plan* plan, int32_t mode) {
    if (!plan || mode < -1 || mode > 5) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_plan_set_spmm_mode: null plan, or mode outside -1 (process-wide value) .. 5");
    plan->spmm_mode.store((int8_t)mode, std::memory_order_relaxed);
    return TCGNN_OK;
}

int tcgnn_plan_set_range_guard(tcgnn_plan* plan, int32_t level) {
    if (!plan || level < -1 || level > 3) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_plan_set_range_guard: null plan, or level outside -1 (process-wide value) .. 3");
    plan->range_guard.store((int8_t)level, std::memory_order_relaxed);
    return TCGNN_OK;
}

int tcgnn_set_range_guard(int32_t level) {
    if (level < 0 || level > 3) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_set_range_guard: 0 (off), 1 (SpMM operators), 2 (+ SDDMM / fused AGNN with a few lost elements, default) or 3 (strict)");
    g_range_guard = level;
    return TCGNN_OK;
}

int tcgnn_set_stage_onepass(int32_t on) {
    if (on < 0 || on > 1) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_set_stage_onepass: 0 (memset + abs-max + convert for every call) or 1 (one pass where it applies, default)");
    g_stage_onepass = on;
    return TCGNN_OK;
}

int tcgnn_set_spmm_mode(int32_t mode) {
    if (mode < 0 || mode > 5) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_set_spmm_mode: 0 (auto), 1 (plain), 2 (range-blocked), 3 (LDS-resident ranges), 4 (single-launch fp32 kernel) or 5 (slice-synchronised range walk)");
    g_spmm_mode = mode;
    return TCGNN_OK;
}

const char* tcgnn_plan_last_kernel(const tcgnn_plan* plan) { return plan ? plan->last_kernel.load(std::memory_order_relaxed) : ""; }

int tcgnn_plan_set_timing(tcgnn_plan* plan, int32_t max_calls) {
    if (!plan || max_calls < 0) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_plan_set_timing: bad argument");
    for (hipEvent_t e : plan->ev) (void)hipEventDestroy(e);
    plan->ev.clear();
    plan->ev_used = 0;
    for (int i = 0; i < 2 * max_calls; ++i) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        plan->ev.push_back(e);
    }
    return TCGNN_OK;
}

int tcgnn_plan_read_timing(tcgnn_plan* plan, float* ms_out, int32_t capacity, int32_t* count) {
    if (!plan || !count || (capacity > 0 && !ms_out)) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_plan_read_timing: null argument");
    int n = 0;
    const int used = std::min(plan->ev_used.load(), (int)plan->ev.size() / 2);
    for (int i = 0; i < used && n < capacity; ++i) {
        HIP_TRY(hipEventSynchronize(plan->ev[2 * i + 1]));
        HIP_TRY(hipEventElapsedTime(&ms_out[n], plan->ev[2 * i], plan->ev[2 * i + 1]));
        ++n;
    }
    *count = n;
    plan->ev_used = 0;
    return TCGNN_OK;
}

} // extern "C"
