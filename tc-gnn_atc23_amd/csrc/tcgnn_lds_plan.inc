// tcgnn_lds_plan.inc - host side of the LDS-resident walks: passes per width, time models, window placement (lds_place_windows),
// build_lds_cells (a cell stream in named steps - cells_* - over one CellBuild, whose DevBufs own every allocation until cells_publish
// hands the stream to the plan), release_cell_stream, build_val_stream (the single-edge stream of the edge-valued walk: val_source_stream,
// build_lds_cells, val_index16).  Included by tcgnn_device.hip.
// Cell stream of the LDS-resident column-range SpMM: per (workgroup, range, wavefront, window slot) the window's
// condensed columns inside the range, re-tiled 32 to a tile.  Built from the packed tile stream (cols / mask).
static int g_lds_maxw = [] { const char* e = test_knob("TCGNN_LDS_MAXW"); const int v = e ? atoi(e) : 0; return (v == 4 || v == 8) ? v : 0; }();   // 0: by width
// Passes of the LDS-resident kernel over a matrix of dpad columns.  Whole 64-column chunks go as two 32-column passes of the
// 8-windows-per-wavefront layout (half the workgroups stream each plane pair, 760-row ranges: Reddit D = 64 0.56 vs 0.79 ms),
// what is left over (1-3 planes) as one pass of the 4-window layout.  TCGNN_LDS_MAXW = 4 / 8 forces one layout for every
// pass (tests, timing).
struct LdsPass { int maxw, nt, chunk0, nchunks; };
// Whole 64-column chunks (8 windows x 2 planes) have two range lengths: 760 rows (slot 4) and 952 (slot kLdsLongSlot).  build_lds_cells
// prices both the first time either is asked for and builds the cheaper one; plan->lds_long remembers which.  TCGNN_LDS_LONG=0 / 1
// (tests, timing): never / wherever the long stream can be built (a flat stream with one tile per cell).
static int lds_long_knob() { const char* e = test_knob("TCGNN_LDS_LONG"); return e ? (atoi(e) != 0 ? 1 : 0) : -1; }   // -1: by price (read when the stream is built)
static int lds_pass_slot(const tcgnn_plan* p, const LdsPass& pass) {
    return lds_stream_of(pass.nt, pass.maxw, pass.maxw == kLdsMaxW2 && pass.nt == 2 && p->lds_long.load(std::memory_order_acquire) == 1);
}
static int lds_passes(int dpad, LdsPass (&passes)[2]) {
    int n = 0;
    if (g_lds_maxw) {
        const int cd = lds_chunk_dims(g_lds_maxw);
        if (dpad / cd) passes[n++] = {g_lds_maxw, cd / 16, 0, dpad / cd};
        if (dpad % cd) passes[n++] = {g_lds_maxw, (dpad % cd) / 16, dpad / cd, 1};
    } else {
        // (r03: a remainder of THREE planes - Reddit's 41 classes - goes as one more pair of 32-column chunks of the 8-window layout,
        //  the fourth plane lying beyond the matrix and filled with zeros: 0.45 ms against 0.51 for the 3-plane pass of the 4-window
        //  layout, which streams 22 MB per CU and has no room for the in-kernel cold remainder)
        const int full = dpad / 64, rem = (dpad % 64) / 16;
        if (full || rem == 3) passes[n++] = {kLdsMaxW2, 2, 0, 2 * (full + (rem == 3 ? 1 : 0))};
        if (rem && rem != 3) passes[n++] = {kLdsMaxW, rem, full, 1};
    }
    return n;
}
// workgroups of one pass: enough to hold every window, spread over every CU a pass can have (with 8 windows per wavefront a
// 64-column chunk takes two passes, hence half the CUs each)
static bool lds_has_hubs(const tcgnn_plan* p) {
    int64_t mx = 0;
    for (int w = 0; w < p->nw_eff; ++w) mx = std::max<int64_t>(mx, p->h_bp[(size_t)w]);
    return mx * p->nw_eff > 4 * std::max<int64_t>(p->tc_blocks, 1);
}
// Placements of a cell stream (lds_place_windows): contiguous weight-balanced blocks per workgroup (locality: the hot / cold split,
// wavefronts of a workgroup busy in the same ranges), the same with hub windows split, or longest-first over the whole graph with
// hub windows split.  Graphs without hubs take the first; graphs with hubs build the count tables of the other two and keep the
// one whose estimated time is lower (build_lds_cells).  TCGNN_LDS_PLACE=local|localsplit|global forces one.
enum { kPlaceLocal = 0, kPlaceLocalSplit = 1, kPlaceGlobal = 2 };
static int lds_place_forced() {
    const char* env = test_knob("TCGNN_LDS_PLACE");
    if (!env) return -1;
    return !strcmp(env, "global") ? kPlaceGlobal : (!strcmp(env, "localsplit") ? kPlaceLocalSplit : kPlaceLocal);
}
static int lds_buf_rows_for_maxw(int maxw) { return maxw == kLdsMaxW2 ? 768 : 512; }   // (the shortest ranges of the layout: the finest spread)
// weight of a window = the tiles it is likely to cost the LDS-resident walk: its condensed columns spread over the column
// ranges (a cell with a handful of columns still costs a whole tile step), not the column count alone
static double lds_window_weight(const tcgnn_plan* p, int w, double nranges_d) {
    const double cols = 8.0 * std::max(p->h_bp[(size_t)w], 1);
    return std::ceil(cols / 32.0 + nranges_d * (1.0 - std::exp(-cols / nranges_d)));
}
static int lds_workgroups_unsplit(const tcgnn_plan* p, int maxw, int extra_slots) {
    const int per_wg = kLdsWaves * maxw;
    const int64_t slots = (int64_t)p->nw_eff + extra_slots;
    int nwg = (int)((slots + per_wg - 1) / per_wg);
    const int cu_target = maxw == kLdsMaxW2 ? std::max(1, p->num_cus / 2) : p->num_cus;
    if (nwg < cu_target) nwg = std::max(nwg, std::min(cu_target, (p->nw_eff + kLdsWaves - 1) / kLdsWaves));
    return nwg;
}
// Hub windows: a wavefront owns whole windows, so a window whose tiles exceed a wavefront's fair share of the workgroup's work
// is the critical path of every range (R-MAT, Reddit shape: the window of the sixteen top hubs holds 3.6 wavefront shares).
// Such a window is SPLIT: k wavefronts of one workgroup each take every k-th run of its tiles in every range and their partial
// sums are added through LDS, in a fixed order, at the end of the kernel.  parts[w] = k (1: whole).  Only on graphs with hubs
// (lds_has_hubs); TCGNN_LDS_PLACE=local keeps every window whole.
static constexpr int kLdsMaxParts = 8, kLdsMaxFollowers = 32;   // (followers of a workgroup: 32 x NT KB of LDS scratch)
static int lds_split_parts(const tcgnn_plan* p, int maxw, std::vector<uint8_t>* parts, const std::vector<double>* exact = nullptr) {
    const int nw = p->nw_eff;
    if (parts) parts->assign((size_t)nw, 1);
    if (nw <= 0 || !lds_has_hubs(p)) return 0;
    const double nranges_d = std::max(1.0, std::ceil((double)p->Nc / (lds_buf_rows_for_maxw(maxw) - 8)));
    auto weight = [&](int w) { return exact ? (*exact)[(size_t)w] : lds_window_weight(p, w, nranges_d); };
    double total = 0;
    for (int w = 0; w < nw; ++w) total += weight(w);
    const double share = total / ((double)lds_workgroups_unsplit(p, maxw, 0) * kLdsWaves);
    int extra = 0;
    for (int w = 0; w < nw; ++w) {
        const double wt = weight(w);
        if (wt <= 1.5 * share) continue;
        const int k = (int)std::min<double>(kLdsMaxParts, std::ceil(wt / share));
        if (k < 2) continue;
        if (parts) (*parts)[(size_t)w] = (uint8_t)k;
        extra += k - 1;
    }
    return extra;
}
static int lds_workgroups(const tcgnn_plan* p, int maxw) {
    const int which = maxw == kLdsMaxW2 ? 1 : 0;
    int extra = p->lds_extra[which].load(std::memory_order_relaxed);
    if (extra < 0) { extra = lds_split_parts(p, maxw, nullptr); p->lds_extra[which].store(extra, std::memory_order_relaxed); }
    return lds_workgroups_unsplit(p, maxw, extra);
}

// Kernel-time models behind the automatic choice between the LDS-resident kernel and the gather walks, microseconds on
// MI355X (tools/check_lds_threshold.py: nine graphs x two widths; the estimates land within ~15 % of the measured times).
// The LDS kernel's time follows the column ranges it walks, almost whatever the edge count: per range a fixed part (barrier,
// DMA issue, metadata; grows with the bytes a range streams) plus ~0.135 us per tile a wavefront multiplies; workgroups
// beyond one per CU run in further rounds.  The gather walks' time follows the edge count.
static double lds_estimate_us(const tcgnn_plan* p, int dpad) {
    LdsPass passes[2];
    const int np = lds_passes(dpad, passes);
    const double cols_per_window = 32.0 * (double)p->total_wb / std::max(p->nw_eff, 1);
    double t = 25.0;
    for (int i = 0; i < np; ++i) {
        const int maxw = passes[i].maxw, nt = passes[i].nt;
        const int rows = lds_stream_buf_rows(lds_stream_of(nt, maxw)) - 8;
        const double nranges = std::ceil((double)p->Nc / rows);
        const int nwg = lds_workgroups(p, maxw);
        const double rounds = std::ceil((double)nwg * passes[i].nchunks / std::max(p->num_cus, 1));
        const double c = cols_per_window / nranges;                                   // distinct columns of a cell
        const double tiles_per_cell = c <= 24.0 ? 1.0 - std::exp(-c) : c / 32.0 + 0.5;
        const double windows_per_wave = (double)p->nw_eff / ((double)nwg * kLdsWaves);
        static const double fixed4[4] = {0.47, 0.60, 0.89, 1.16};
        const double a = maxw == kLdsMaxW2 ? 0.80 : fixed4[std::min(nt, 4) - 1];
        t += rounds * nranges * (a + 0.135 * windows_per_wave * tiles_per_cell);
    }
    return t;
}
static double gather_estimate_us(const tcgnn_plan* p, int dpad) {
    const double image = ((double)p->Nc + 1) * x16_pitch(dpad) * 2.0;
    double ps;   // picoseconds per edge
    if (image <= (double)kBlockedMinBytes) ps = 4.6 + std::max(0, dpad - 16) * (1.8 / 48.0);        // L2-resident image, per-window walk
    else if (dpad <= 32) ps = 8.5;
    else if (dpad <= 64) ps = 8.5 + (dpad - 32) * (1.1 / 32.0);
    else ps = 9.6 + (dpad - 64) * (6.9 / 64.0);
    // the gathered image leaves first the L2s, then the Infinity Cache (row shards of the multi-GPU workload: 60 / 119 / 239 MB
    // -> 10.0 / 12.4 / 14.7 ps per edge at 64 columns)
    if (image > 45.0e6) ps *= std::pow(image / 45.0e6, 0.3);
    return 20.0 + (double)p->E * ps * 1e-6;
}
// automatic mode: the LDS-resident kernel when its estimate is clearly the lower one (decided once per plan and width)
static bool lds_chosen(const tcgnn_plan* p, int dpad) {
    if (!g_lds_auto || p->nw_eff <= 0 || p->total_wb <= 0) return false;
    const int k = dpad / 16;
    if (k <= 64 && p->lds_choice[k] >= 0) return p->lds_choice[k] != 0;
    LdsPass passes[2];
    const int np = lds_passes(dpad, passes);
    double cells = 0;   // cell-table entries of the streams this width needs (host scan + device memory)
    for (int i = 0; i < np; ++i) {
        const int rows = lds_stream_buf_rows(lds_stream_of(passes[i].nt, passes[i].maxw)) - 8;
        cells += (double)lds_workgroups(p, passes[i].maxw) * kLdsWaves * passes[i].maxw * std::ceil((double)p->Nc / rows);
    }
    const bool yes = cells < 2.0e8 && lds_estimate_us(p, dpad) <= 0.95 * gather_estimate_us(p, dpad);
    if (k <= 64) p->lds_choice[k] = yes ? 1 : 0;
    return yes;
}

// Window slots of a cell stream (order[cell_position(wg, wave, j)] = window id or -1): the windows, in their own order, are cut into
// nwg contiguous blocks of about equal weight (blockPartition = condensed columns) and at most 16 x maxw windows; inside a block
// they go heaviest-first to the least loaded wavefront that still has a free slot.
// One workgroup's windows (heaviest first; a split window's parts weigh wt / k each and are placed when it comes up) go to the
// least loaded wavefront with a free slot, the parts of one window to different wavefronts.  parts_out (if sized) receives
// part | parts << 8 | scratch index << 16 for the slots of split windows: scratch index of a follower = its own, of part 0 = its first follower's.
static bool lds_deal_workgroup(int g, int maxw, const std::vector<int32_t>& items, const std::vector<uint8_t>& k, const std::vector<double>& wt,
                               std::vector<int32_t>& order, std::vector<uint32_t>& parts_out, int& nsplit) {
    double load[kLdsWaves] = {0};
    int used[kLdsWaves] = {0};
    uint32_t next_fol = 0;
    for (const int32_t w : items) {
        const int kk = k.empty() ? 1 : k[(size_t)w];
        uint32_t taken = 0u;                         // wavefronts that hold a part of this window
        const uint32_t fol0 = next_fol;
        for (int part = 0; part < kk; ++part) {
            int best = -1;
            for (int v = 0; v < kLdsWaves; ++v)
                if (used[v] < maxw && !((taken >> v) & 1u) && (best < 0 || load[v] < load[best])) best = v;
            if (best < 0)   // (every free slot sits on a wavefront that already holds a part of this window)
                for (int v = 0; v < kLdsWaves; ++v) if (used[v] < maxw && (best < 0 || load[v] < load[best])) best = v;
            if (best < 0) return false;   // more items than slots: the caller's accounting is off - it falls back to a placement without parts
            const size_t pos = (size_t)cell_position(g, best, used[best], maxw);
            order[pos] = w;
            if (kk > 1) parts_out[pos] = (uint32_t)part | ((uint32_t)kk << 8) | ((part == 0 ? fol0 : fol0 + (uint32_t)part - 1u) << 16);
            taken |= 1u << best;
            load[best] += wt[(size_t)w] / kk;
            ++used[best];
        }
        if (kk > 1) { next_fol += (uint32_t)kk - 1u; ++nsplit; }
    }
    return true;
}
static bool lds_place_windows(const tcgnn_plan* p, int nwg, int maxw, std::vector<int32_t>& order, std::vector<uint32_t>& parts_out, int& nsplit,
                              const std::vector<double>& exact, int mode) {
    const int nw = p->nw_eff, cap = kLdsWaves * maxw;
    order.assign((size_t)nwg * cap, -1);
    parts_out.clear();
    nsplit = 0;
    // Hub windows (power-law graphs numbered by degree) sit next to each other: a contiguous block of them fills a few wavefronts of
    // its workgroup and leaves the rest idle, so the workgroup runs several times longer than the mean (R-MAT, Reddit shape: 1.20 ms
    // against 0.85 ms).  When the heaviest window is far above the mean the windows are instead dealt heaviest first, boustrophedon-wise
    // over workgroups and wavefronts - every workgroup gets one hub and a share of the light windows.  TCGNN_LDS_PLACE=global|local forces it.
    if (mode == kPlaceGlobal) {
        std::vector<uint8_t> k;
        const int extra = lds_split_parts(p, maxw, &k, &exact);
        // (r01's boustrophedon deal of unsplit windows measured the same - 0.53 ms uniform, 0.61 with the hub - and is gone)
        // With split windows: longest-processing-time placement.  Windows (a split one with all its parts) go heaviest first to the
        // least loaded workgroup that has the slots; inside a workgroup the items (whole windows and parts) go heaviest first to
        // the least loaded wavefront with a free slot, the parts of one window to different wavefronts.
        const std::vector<double>& wt = exact;
        std::vector<int32_t> idx((size_t)nw);
        std::iota(idx.begin(), idx.end(), 0);
        std::stable_sort(idx.begin(), idx.end(), [&](int32_t x, int32_t y) { return wt[(size_t)x] > wt[(size_t)y]; });
        std::vector<double> wg_load((size_t)nwg, 0.0);
        std::vector<int> wg_free((size_t)nwg, cap), wg_fol((size_t)nwg, 0);
        std::vector<std::vector<int32_t>> wg_items((size_t)nwg);
        for (int q = 0; q < nw; ++q) {
            const int w = idx[(size_t)q];
            int kk = k[(size_t)w];
            int best = -1;
            for (int pass = 0; pass < 2 && best < 0; ++pass) {   // (second pass: the window whole, wherever one slot is free)
                if (pass == 1) { kk = 1; k[(size_t)w] = 1; }
                for (int g = 0; g < nwg; ++g)
                    if (wg_free[(size_t)g] >= kk && wg_fol[(size_t)g] + kk - 1 <= kLdsMaxFollowers && (best < 0 || wg_load[(size_t)g] < wg_load[(size_t)best])) best = g;
            }
            if (best < 0) return false;
            wg_load[(size_t)best] += wt[(size_t)w];
            wg_free[(size_t)best] -= kk;
            wg_fol[(size_t)best] += kk - 1;
            wg_items[(size_t)best].push_back(w);
        }
        if (extra > 0) parts_out.assign((size_t)nwg * cap, 0u); else k.clear();
        for (int g = 0; g < nwg; ++g)
            if (!lds_deal_workgroup(g, maxw, wg_items[(size_t)g], k, wt, order, parts_out, nsplit)) return false;
        if (nsplit == 0) parts_out.clear();
        return true;
    }
    const std::vector<double>& wt = exact;   // (the tiles a window costs THIS stream: window_tiles_kernel)
    double total = 0;
    for (int w = 0; w < nw; ++w) total += wt[(size_t)w];
    std::vector<uint8_t> k;
    const int extra = mode == kPlaceLocalSplit ? lds_split_parts(p, maxw, &k, &exact) : 0;
    if (extra > 0) {
        // the stream has nwg * cap slots (lds_workgroups counted the parts with the modelled weights; the exact ones may ask for
        // more): take parts back, from the most divided windows first, until everything fits
        int64_t slots = 0;
        for (int w = 0; w < nw; ++w) slots += k[(size_t)w];
        for (int level = kLdsMaxParts; slots > (int64_t)nwg * cap && level > 1; --level)
            for (int w = 0; w < nw && slots > (int64_t)nwg * cap; ++w)
                if (k[(size_t)w] == level) { --k[(size_t)w]; --slots; }
        parts_out.assign((size_t)nwg * cap, 0u);
    } else k.clear();
    std::vector<int64_t> slots_after((size_t)nw + 1, 0);   // slots window w and the windows after it need (an upper bound: parts may still be taken back)
    for (int w = nw - 1; w >= 0; --w) slots_after[(size_t)w] = slots_after[(size_t)w + 1] + (k.empty() ? 1 : k[(size_t)w]);
    std::vector<int32_t> blk;   // windows of the block being dealt
    double acc = 0;
    int wg = 0, blk_slots = 0, blk_fol = 0;
    bool ok = true;
    auto deal = [&]() {
        // Even windows are dealt in their own order (least loaded wavefront first = round-robin): a block that spans two communities
        // then gives every wavefront its share of both, and in a range of either community all sixteen are busy.  Sorting by
        // weight first is for blocks with windows far above the others.
        double mx = 0, sum = 0;
        for (const int32_t w : blk) { mx = std::max(mx, wt[(size_t)w]); sum += wt[(size_t)w]; }
        if (mx * (double)blk.size() > 1.5 * sum) {   // the windows far above the mean first, heaviest first; the others keep their order
            const double heavy = 2.0 * sum / (double)blk.size();
            auto mid = std::stable_partition(blk.begin(), blk.end(), [&](int32_t x) { return wt[(size_t)x] > heavy; });
            std::stable_sort(blk.begin(), mid, [&](int32_t x, int32_t y) { return wt[(size_t)x] > wt[(size_t)y]; });
        }
        ok = lds_deal_workgroup(wg, maxw, blk, k, wt, order, parts_out, nsplit) && ok;
        blk.clear(); blk_slots = 0; blk_fol = 0;
    };
    // invariant: the slots still needed fit into the free slots of this block plus the workgroups left
    for (int w = 0; w < nw && ok; ++w) {
        int kk = k.empty() ? 1 : k[(size_t)w];
        const int wgs_left0 = nwg - (wg + 1);
        if (kk > 1 && blk_fol + kk - 1 > kLdsMaxFollowers) { k[(size_t)w] = 1; kk = 1; }            // (scratch of the workgroup is full: this one stays whole)
        if (blk_slots + kk > cap) {
            // closing the block leaves its free slots unused: only if what is left still fits into the workgroups behind it
            if (wgs_left0 > 0 && slots_after[(size_t)w] <= (int64_t)wgs_left0 * cap) { deal(); ++wg; }
            else { if (kk > 1) k[(size_t)w] = 1; kk = 1; }
            if (blk_slots + kk > cap) { ok = false; break; }
        }
        blk.push_back(w);
        blk_slots += kk; blk_fol += kk - 1;
        acc += wt[(size_t)w];
        const int wgs_left = nwg - (wg + 1);
        const bool full = blk_slots == cap;
        const bool heavy_enough = acc >= total * (double)(wg + 1) / nwg;
        if (wgs_left > 0 && (full || (heavy_enough && slots_after[(size_t)w + 1] <= (int64_t)wgs_left * cap))) { deal(); ++wg; }
    }
    if (ok && !blk.empty()) deal();
    if (nsplit == 0) parts_out.clear();
    return ok;
}

// ---- build_lds_cells: a cell stream built in named steps over one CellBuild.  Every step is fallible and owns what it allocates
// through the context's DevBufs; cells_publish, last, cannot fail: a failed build leaves the plan's slot exactly as it found it.

// A candidate placement: window slots, columns per cell, columns and busiest-wavefront tiles per (workgroup, range) pair, and from
// those an estimate of the kernel time (+ the cold remainder's); the cheapest is built.
struct CellPlacement {
    int mode = kPlaceLocal, nsplit = 0;
    uint32_t hot_min = 1u;
    double est_us = 0;
    std::vector<int32_t> sorder;
    std::vector<uint32_t> sparts, paircols, pairmax, pairover, pairtiles;   // pairover: [2][pairs] columns beyond 32 / 64 per cell
    DevBuf<uint32_t> d_cellcols, d_firstq, d_parts;
    DevBuf<int32_t> d_sorder;
};
// Entries of a flat stream (tcgnn_lds_flat.inc): per workgroup its normal entries first - one per hot pair, in range order - then
// the dense entries of its dense pairs, grouped by pair.  ent2[2 k] = normal entry of pair k, ent2[2 k + 1] = its first dense entry
// (-1: not a dense pair); entry numbers are global (a workgroup's entries are contiguous: wg_first).
struct FlatEntries {
    std::vector<int32_t> ent2, nd, wg_first;
    std::vector<uint32_t> xbase, rl2;   // (records only) first extra tile of every cell among its wavefront's; the entry records
    int64_t nentries = 0;
};
// Pure host function, no HIP call: the entry layout and - records - the entry records of a flat stream from the hot pairs (rbase,
// rlist), the tiles of every hot cell (cnt) and the extra tiles of every pair's busiest wavefront (dense_mx; dense_on: dense pairs
// get dense entries).
static FlatEntries flat_entries(int nwg, int maxw, const std::vector<int32_t>& rbase, const std::vector<int32_t>& rlist, const std::vector<uint32_t>& cnt,
                                const std::vector<uint32_t>& dense_mx, bool dense_on, bool records) {
    FlatEntries f;
    const int64_t npairs = rbase[(size_t)nwg];
    f.ent2.assign((size_t)npairs * 2 + 2, -1); f.nd.assign((size_t)npairs, 0); f.wg_first.assign((size_t)nwg + 1, 0);
    int32_t eidx = 0;
    for (int wg = 0; wg < nwg; ++wg) {
        f.wg_first[(size_t)wg] = eidx;
        for (int64_t k = rbase[(size_t)wg]; k < rbase[(size_t)wg + 1]; ++k) f.ent2[(size_t)k * 2] = eidx++;
        for (int64_t k = rbase[(size_t)wg]; k < rbase[(size_t)wg + 1]; ++k) {
            f.nd[(size_t)k] = dense_on ? (int32_t)((dense_mx[(size_t)k] + maxw - 1) / maxw) : 0;
            f.ent2[(size_t)k * 2 + 1] = f.nd[(size_t)k] ? eidx : -1;
            eidx += f.nd[(size_t)k];
        }
    }
    f.wg_first[(size_t)nwg] = eidx;
    f.nentries = eidx;
    if (!records) return f;
    const std::vector<int32_t>& nd = f.nd;
    std::vector<uint32_t>& xbase = f.xbase;
    if (dense_on) {
        xbase.assign((size_t)(npairs * kLdsWaves * maxw), 0u);
        for (int64_t k = 0; k < npairs; ++k) {
            if (!nd[(size_t)k]) continue;
            for (int v = 0; v < kLdsWaves; ++v) {
                uint32_t run = 0;
                for (int j = 0; j < maxw; ++j) { const size_t c = (size_t)((k * kLdsWaves + v) * maxw + j); xbase[c] = run; run += cnt[c] > 1u ? cnt[c] - 1u : 0u; }
            }
        }
    }
    // entry words: w0 = range | bit 31 dense | bit 30 another range than the entry before; w1 = dense: tiles per window slot;
    // w2 = range to fetch at the top of the entry (~0: none); w3 = 0
    // (layout: [entries][4] records - w0, w2, normal entries of the workgroup, 0: the same for every wavefront, 16 bytes per entry,
    //  L2-resident - followed by [entries][16 wavefronts] descriptor words w1, read in the dense phase only.  The kernels load the
    //  FIRST TWO words of a record and use both: a loaded word nobody reads is a register the allocator hands to another value
    //  while the load is in flight, and hipcc then waits vmcnt(0) before writing it - at the top of every entry, right behind the
    //  range fill (r05: the edge-valued walk ran 26 % slower for one such word, the remainder layouts of the binary walk too).
    //  A per-(entry, wavefront) record of all three words was 10 MB per stream and a DRAM miss per wavefront and entry: the uniform
    //  Reddit shape ran 5 % slower for it)
    const int64_t nrec = std::max<int64_t>(f.nentries, 1);
    f.rl2.assign((size_t)nrec * (4 + kLdsWaves), 0u);
    auto put = [&](int64_t en, int v, uint32_t w0, uint32_t w1, uint32_t w2) {
        uint32_t* q = &f.rl2[(size_t)(en * 4)];
        q[0] = w0; q[1] = w2; q[3] = 0u;   // (q[2]: normal entries of the entry's workgroup, written below)
        f.rl2[(size_t)(nrec * 4 + en * kLdsWaves + v)] = w1;
    };
    for (int wg = 0; wg < nwg; ++wg)   // record word 2: how many NORMAL entries the entry's workgroup has (its dense entries follow them: val_permute_kernel)
        for (int64_t en = f.wg_first[(size_t)wg]; en < f.wg_first[(size_t)wg + 1]; ++en) f.rl2[(size_t)(en * 4 + 2)] = (uint32_t)(rbase[(size_t)wg + 1] - rbase[(size_t)wg]);
    for (int wg = 0; wg < nwg; ++wg) {
        const int64_t k0 = rbase[(size_t)wg], k1 = rbase[(size_t)wg + 1];
        std::vector<int64_t> dk;   // the workgroup's dense pairs, in order
        for (int64_t k = k0; k < k1; ++k) if (nd[(size_t)k]) dk.push_back(k);
        for (int64_t k = k0; k < k1; ++k) {
            const uint32_t r = (uint32_t)rlist[(size_t)k];
            const uint32_t nextr = k + 1 < k1 ? (uint32_t)rlist[(size_t)k + 1] : (dk.empty() ? 0xffffffffu : (uint32_t)rlist[(size_t)dk[0]]);
            for (int v = 0; v < kLdsWaves; ++v) put(f.ent2[(size_t)k * 2], v, r | (k > k0 ? 0x40000000u : 0u), 0u, nextr);
        }
        for (size_t gi = 0; gi < dk.size(); ++gi) {
            const int64_t k = dk[gi];
            const uint32_t r = (uint32_t)rlist[(size_t)k];
            const uint32_t nextr = gi + 1 < dk.size() ? (uint32_t)rlist[(size_t)dk[gi + 1]] : 0xffffffffu;
            for (int64_t d = 0; d < nd[(size_t)k]; ++d)
                for (int v = 0; v < kLdsWaves; ++v) {
                    uint32_t desc = 0u;   // tiles of every window slot among this wavefront's extras [maxw d, maxw (d + 1))
                    for (int j = 0; j < maxw; ++j) {
                        const size_t c = (size_t)((k * kLdsWaves + v) * maxw + j);
                        const int64_t lo = xbase[c], hi = lo + (cnt[c] > 1u ? cnt[c] - 1u : 0u);
                        const int64_t a0 = std::max<int64_t>(lo, d * maxw), a1 = std::min<int64_t>(hi, (d + 1) * maxw);
                        if (a1 > a0) desc |= (uint32_t)(a1 - a0) << (4 * j);
                    }
                    put(f.ent2[(size_t)k * 2 + 1] + d, v, r | 0x80000000u | (d == 0 ? 0x40000000u : 0u), desc, d == 0 ? nextr : 0xffffffffu);
                }
        }
    }
    return f;
}

// The build context: what the stream is cut from, its geometry, the host tables the steps hand each other (they also outlive the
// copies enqueued from them) and the device buffers still alive.  What is left in it when the build returns is freed.
struct CellBuild {
    tcgnn_plan* p; hipStream_t stream; int slot;
    // the source: the packed tile stream (cols / mask) or, slot kLdsValSlot, the single-edge one, whose K slots also carry the CSR
    // position of their edge: that index follows every slot into the tiles (s_eidx / d_eidx)
    bool val;
    const int64_t* s_wb; const int32_t* s_cols; const uint32_t* s_mask; const int32_t* s_eidx;
    int maxw, rows, nranges, per_wg, nwg, nw;   // rows: data rows of a range; nw: window SLOTS of this stream
    int64_t ncell, npairs_all;
    bool verbose;
    // host tables, in the order the steps fill them
    std::vector<double> exact;                      // exact weight of every window in THIS stream: the tiles it will cost
    CellPlacement best;
    std::vector<int32_t> kmap, rbase, rlist;        // hot pairs: compact number of pair (wg, range) or -1; per workgroup; their ranges
    int64_t npairs = 0, ncell_hot = 0, hot_cols = 0, cold_cols = 0;
    std::vector<uint32_t> cnt;                      // tiles of every hot cell (ordinary count; on the host from cells_entries on); an ordinary stream's cell table once summed
    std::vector<uint32_t> pair_extra, pair_cellmx;  // per hot pair: extra tiles of its busiest wavefront, tiles of its fullest cell (cell_dense_stats_kernel)
    std::vector<uint32_t> dense_mx;                 // extra tiles of the pair's busiest wavefront (0: not a dense pair)
    int64_t over_dense = 0, dense_steps = 0, ndense_pairs = 0, ndense_entries = 0;
    int flat_tpc = 0;
    int64_t over_cols = 0;
    FlatEntries ent;
    int64_t ntiles = 0, nwords = 0, cold_tiles = 0, cold_max = 0;
    std::vector<int64_t> cptr;                      // first cold tile of every window
    std::vector<int32_t> wptr;
    std::vector<uint32_t> wlist;
    // device buffers (the placement's are in best)
    DevBuf<int32_t> d_kmap, d_rbase, d_rlist, d_ent, d_ccols, d_eidx, d_cold_eidx, d_wcold_ptr;
    DevBuf<uint32_t> d_cnt, d_tiles, d_flat, d_rl2, d_xbase, d_cmask, d_wcold;
    DevBuf<int64_t> d_cold_ptr;
    // what the choice between the two range lengths of whole 64-column chunks reads (cells_price): the ordinary stream's steps, the
    // cold tiles the flat cap leaves (trial_tiles; worst_tail: those of the worst wavefront BEYOND what its walk admits - one per entry,
    // the long walk one per kLongTurn entries - i.e. its serial loop behind the walk)
    int64_t classic_steps = 0, trial_tiles = 0, worst_tail = 0;
    double price = 0;
    bool long_ranges() const { return slot == kLdsLongSlot; }
    bool with_dense() const { return flat_tpc == 1 && ndense_pairs > 0; }
};

// step 1: exact weight of every window (window_tiles_kernel; at least one, so empty windows still take a slot's worth)
static int cells_window_weights(CellBuild& b) {
    const tcgnn_plan* p = b.p;
    b.exact.assign((size_t)p->nw_eff, 1.0);
    DevBuf<uint32_t> d_wt;
    std::vector<uint32_t> h_wt((size_t)p->nw_eff, 0u);
    hipError_t e = d_wt.alloc(h_wt.size());
    if (e == hipSuccess) e = hipMemsetAsync(d_wt, 0, h_wt.size() * sizeof(uint32_t), b.stream);
    if (e == hipSuccess) {
        const int64_t nth = (int64_t)p->nw_eff * b.nranges;
        hipLaunchKernelGGL(window_tiles_kernel, dim3((unsigned)((nth + 255) / 256)), dim3(256), 0, b.stream, b.s_wb, b.s_cols, p->nw_eff, b.nranges, p->Nc, b.rows, d_wt.ptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_wt.data(), d_wt, h_wt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b.stream);
    if (e != hipSuccess) return fail(hip_rc(e), "window weights: %s", hipGetErrorString(e));
    for (size_t w = 0; w < h_wt.size(); ++w) b.exact[w] = std::max<double>(1.0, h_wt[w]);
    return TCGNN_OK;
}
// step 2a: one candidate: the placement (host), its count tables (cell_count_kernel, cell_pair_cols_kernel) and its estimate
static hipError_t cells_prepare_placement(const CellBuild& b, int mode, CellPlacement& c) {
    const tcgnn_plan* p = b.p;
    const int nwg = b.nwg, nranges = b.nranges, maxw = b.maxw;
    const int64_t npairs_all = b.npairs_all;
    c.mode = mode;
    if (!lds_place_windows(p, nwg, maxw, c.sorder, c.sparts, c.nsplit, b.exact, mode)) {   // (a placement with parts that ran out of slots)
        c.mode = kPlaceLocal;
        if (!lds_place_windows(p, nwg, maxw, c.sorder, c.sparts, c.nsplit, b.exact, kPlaceLocal)) return hipErrorInvalidValue;
    }
    // threshold: a range step costs a workgroup ~1.7 us (8-window layout, two passes over 256 CUs: ~13 ns of chip time) or
    // ~1 us (4-window layout, one pass: ~4 ns), a column in the gather walk ~10 ps of chip time.  Forcing the LDS-resident walk
    // (mode 3: tests, timing) keeps every pair that holds a column, and so does the graph-wide placement (no locality to split
    // on: every pair holds about the same share); TCGNN_LDS_HOT_COLS overrides.
    c.hot_min = maxw == kLdsMaxW2 ? 1000u : 400u;
    if (spmm_mode_of(p) == 3 || c.mode == kPlaceGlobal) c.hot_min = 1u;
    if (const char* env = test_knob("TCGNN_LDS_HOT_COLS")) c.hot_min = (uint32_t)std::max(1, atoi(env));
    DevBuf<uint32_t> d_pc, d_pm, d_po, d_pt;
    hipError_t e = c.d_cellcols.alloc((size_t)(b.ncell + 1));
    if (e == hipSuccess && c.nsplit > 0) {
        e = c.d_parts.alloc(c.sparts.size());
        if (e == hipSuccess) e = hipMemcpyAsync(c.d_parts, c.sparts.data(), c.sparts.size() * sizeof(uint32_t), hipMemcpyHostToDevice, b.stream);
    }
    if (e == hipSuccess) e = c.d_firstq.alloc((size_t)b.nw * nranges);
    if (e == hipSuccess) e = c.d_sorder.alloc(c.sorder.size());
    if (e == hipSuccess) e = d_pc.alloc((size_t)npairs_all);
    if (e == hipSuccess) e = d_pm.alloc((size_t)npairs_all);
    if (e == hipSuccess) e = d_po.alloc((size_t)npairs_all * 2);
    if (e == hipSuccess) e = d_pt.alloc((size_t)npairs_all);
    if (e == hipSuccess) e = hipMemcpyAsync(c.d_sorder, c.sorder.data(), c.sorder.size() * sizeof(int32_t), hipMemcpyHostToDevice, b.stream);
    if (e == hipSuccess) e = hipMemsetAsync(c.d_cellcols, 0, (size_t)(b.ncell + 1) * sizeof(uint32_t), b.stream);
    c.pairmax.resize((size_t)npairs_all);
    c.paircols.resize((size_t)npairs_all);
    c.pairover.resize((size_t)npairs_all * 2);
    c.pairtiles.resize((size_t)npairs_all);
    if (e == hipSuccess) {
        const int64_t nthreads = (int64_t)b.nw * nranges;
        hipLaunchKernelGGL(cell_count_kernel, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, b.stream, b.s_wb, c.d_sorder.ptr, b.s_cols, b.nw, nwg,
                           nranges, p->Nc, maxw, b.rows, c.d_cellcols.ptr, c.d_firstq.ptr, c.d_parts.ptr);
        hipLaunchKernelGGL(cell_pair_cols_kernel, dim3((unsigned)((npairs_all + 255) / 256)), dim3(256), 0, b.stream, c.d_cellcols.ptr, npairs_all, b.per_wg, maxw, d_pc.ptr, d_pm.ptr,
                           d_po.ptr, d_pt.ptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(c.paircols.data(), d_pc, c.paircols.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c.pairover.data(), d_po, c.pairover.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c.pairtiles.data(), d_pt, c.pairtiles.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c.pairmax.data(), d_pm, c.pairmax.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b.stream);
    if (e != hipSuccess) return e;
    // every range ends at a barrier: a workgroup's time is the sum over its hot ranges of a fixed part and its busiest
    // wavefront's tiles (constants of lds_estimate_us); the kernel lasts as long as its slowest workgroup, times the rounds
    // beyond one workgroup per CU; the cold remainder's columns go through a gather walk at ~20 ps each.
    const double rounds = std::max(1.0, std::ceil((double)nwg * (maxw == kLdsMaxW2 ? 2 : 1) / std::max(p->num_cus, 1)));
    auto estimate = [&](uint32_t hot_min) {
        double worst = 0, cold = 0;
        for (int wg = 0; wg < nwg; ++wg) {
            double t = 0;
            for (int r = 0; r < nranges; ++r) {
                const size_t k = (size_t)wg * nranges + r;
                if (c.paircols[k] >= hot_min) t += 0.80 + 0.135 * c.pairmax[k]; else cold += c.paircols[k];
            }
            worst = std::max(worst, t);
        }
        return worst * rounds + cold * 20e-6;
    };
    c.est_us = estimate(c.hot_min);
    if (b.verbose && c.mode != kPlaceGlobal)
        for (uint32_t h : {1u, 125u, 250u, 500u, 1000u, 2000u}) fprintf(stderr, "[tcgnn]   placement %d, hot threshold %u: estimated %.0f us\n", c.mode, h, estimate(h));
    return hipSuccess;
}
// step 2: the placement that is built: the forced one, contiguous blocks for graphs without hubs, else the cheaper of longest-first
// over the graph and contiguous blocks with split hub windows
static int cells_choose_placement(CellBuild& b) {
    const int forced = lds_place_forced();
    const bool hubs = lds_has_hubs(b.p);
    hipError_t e = cells_prepare_placement(b, forced >= 0 ? forced : (hubs ? kPlaceGlobal : kPlaceLocal), b.best);
    if (e == hipSuccess && forced < 0 && hubs) {
        CellPlacement other;
        e = cells_prepare_placement(b, kPlaceLocalSplit, other);
        if (b.verbose) fprintf(stderr, "[tcgnn] cell stream %d: estimated %.0f us longest-first over the graph, %.0f us contiguous blocks (+ cold remainder)\n", b.slot, b.best.est_us, other.est_us);
        if (e == hipSuccess && other.est_us < b.best.est_us) std::swap(b.best, other);
    }
    if (e != hipSuccess) return fail(hip_rc(e), "cell table: %s", hipGetErrorString(e));
    return TCGNN_OK;
}
// step 3: hot / cold: a (workgroup, range) pair is worth a range fill only if enough of the workgroup's columns fall into it.  Then
// the tiles of every hot cell (ordinary count: ceil(columns / 32); cell_compact_kernel) on the host: the ordinary stream's cell
// table is their prefix sum, and a flat stream's DENSE entries (tcgnn_lds_flat.inc) are laid out from them
static int cells_hot_pairs(CellBuild& b) {
    const std::vector<uint32_t>& paircols = b.best.paircols;
    hipError_t e = b.d_kmap.alloc((size_t)b.npairs_all);
    if (e != hipSuccess) return fail(hip_rc(e), "cell table: %s", hipGetErrorString(e));
    b.kmap.assign((size_t)b.npairs_all, -1); b.rbase.assign((size_t)b.nwg + 1, 0);
    std::vector<int32_t>& rlist = b.rlist;
    for (int wg = 0; wg < b.nwg; ++wg) {
        b.rbase[(size_t)wg] = (int32_t)rlist.size();
        for (int r = 0; r < b.nranges; ++r) {
            const uint32_t c = paircols[(size_t)wg * b.nranges + r];
            if (c >= b.best.hot_min) { b.kmap[(size_t)wg * b.nranges + r] = (int32_t)rlist.size(); rlist.push_back(r); b.hot_cols += c; }
            else b.cold_cols += c;
        }
    }
    b.rbase[(size_t)b.nwg] = (int32_t)rlist.size();
    b.npairs = (int64_t)rlist.size();
    rlist.resize(rlist.size() + 4, 0);
    b.ncell_hot = b.npairs * b.per_wg;
    e = b.d_cnt.alloc((size_t)(b.ncell_hot + 1));
    if (e == hipSuccess) e = b.d_rbase.alloc(b.rbase.size());
    if (e == hipSuccess) e = b.d_rlist.alloc(rlist.size());
    if (e == hipSuccess) e = hipMemsetAsync(b.d_cnt, 0, (size_t)(b.ncell_hot + 1) * sizeof(uint32_t), b.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(b.d_kmap, b.kmap.data(), b.kmap.size() * sizeof(int32_t), hipMemcpyHostToDevice, b.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(b.d_rbase, b.rbase.data(), b.rbase.size() * sizeof(int32_t), hipMemcpyHostToDevice, b.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(b.d_rlist, rlist.data(), rlist.size() * sizeof(int32_t), hipMemcpyHostToDevice, b.stream);
    if (e != hipSuccess) return fail(hip_rc(e), "cell table: %s", hipGetErrorString(e));
    if (b.ncell > 0) hipLaunchKernelGGL(cell_compact_kernel, dim3((unsigned)((b.ncell + 255) / 256)), dim3(256), 0, b.stream, b.best.d_cellcols.ptr, b.d_kmap.ptr, b.npairs_all, b.per_wg, b.d_cnt.ptr);
    e = hipGetLastError();
    // (the table itself - 4 bytes per hot cell, 20 MB on the Reddit shape - goes to the host in cells_entries, for the stream that is
    //  built; what is decided before that reads two words per pair)
    DevBuf<uint32_t> d_stats;
    b.pair_extra.assign((size_t)b.npairs, 0u); b.pair_cellmx.assign((size_t)b.npairs, 0u);
    if (e == hipSuccess && b.npairs > 0) {
        e = d_stats.alloc((size_t)b.npairs * 2);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(cell_dense_stats_kernel, dim3((unsigned)((b.npairs + 255) / 256)), dim3(256), 0, b.stream, b.d_cnt.ptr, b.npairs, b.maxw, d_stats.ptr, d_stats.ptr + b.npairs);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(b.pair_extra.data(), d_stats, (size_t)b.npairs * sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(b.pair_cellmx.data(), d_stats.ptr + b.npairs, (size_t)b.npairs * sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(b.stream);
    if (e != hipSuccess) return fail(TCGNN_ERR_HIP, "cell count: %s", hipGetErrorString(e));
    return TCGNN_OK;
}
// step 4 (host): dense pairs (flat streams with one tile per cell): a hot pair whose cells overflow their one tile by `dense_min`
// columns or more keeps ALL its columns in the LDS-resident walk - the tiles beyond each cell's first go into dense entries behind
// the pair's normal entry, T = maxw of them per wavefront and entry - instead of leaving them to the cold remainder.
// (a community's own ranges on the SBM calibrated to real Reddit: ~27 000 overflow columns per pair against ~2 elsewhere;
//  a thin overflow is better off re-condensed per window across all ranges: 32 columns to a cold tile, whatever their range)
// ... and so does a pair in which SOME cell holds three tiles or more (a workgroup at a community's border has one or two windows
// in it: their six dense cells are 40 cold tiles for one window - the hub-row trial sent the whole stream back to the ordinary
// format for them; on the uniform graph a 65-column cell does not occur)
static void cells_dense_pairs(CellBuild& b) {
    const int maxw = b.maxw;
    uint32_t dense_min = 1024u, dense_cell_tiles = 3u;
    if (const char* env = test_knob("TCGNN_LDS_DENSE_COLS")) { dense_min = (uint32_t)std::max(1, atoi(env)); dense_cell_tiles = 0xffffffffu; }   // (tests: dense entries on graphs the oracle can handle)
    if (!flat_dense_ok(lds_stream_nt(b.slot), maxw, 1)) dense_min = dense_cell_tiles = 0xffffffffu;   // (layouts whose kernel has no dense walk)
    std::vector<int64_t> kall_of((size_t)b.npairs, 0);
    for (int64_t ka = 0; ka < b.npairs_all; ++ka) if (b.kmap[(size_t)ka] >= 0) kall_of[(size_t)b.kmap[(size_t)ka]] = ka;
    b.dense_mx.assign((size_t)b.npairs, 0u);
    for (int64_t k = 0; k < b.npairs; ++k) {
        if (dense_min == 0xffffffffu && dense_cell_tiles == 0xffffffffu) break;
        const uint32_t mx = b.pair_extra[(size_t)k], cell_mx = b.pair_cellmx[(size_t)k];
        if (!mx || (b.best.pairover[(size_t)kall_of[(size_t)k]] < dense_min && cell_mx < dense_cell_tiles)) continue;
        b.dense_mx[(size_t)k] = mx;
        b.over_dense += b.best.pairover[(size_t)kall_of[(size_t)k]];
        b.dense_steps += mx; ++b.ndense_pairs; b.ndense_entries += (mx + maxw - 1) / maxw;
    }
}
// step 5 (host): flat or ordinary (tcgnn_lds_flat.inc): a flat stream gives every cell of a hot pair exactly tpc tiles and sends
// what a cell holds beyond 32 tpc columns to the cold remainder (one tile per cell: or, for dense pairs, to dense entries).  Taken
// when that costs few columns (the cold remainder of a flat stream is added by a latency-bound kernel) and no more tile steps than
// the ordinary stream's; never with split hub windows (their cells are nowhere near uniform).  TCGNN_LDS_FLAT=0 / 1 / 2 forces
// ordinary / one / two tiles per cell.
static void cells_flat_or_ordinary(CellBuild& b) {
    const CellPlacement& best = b.best;
    const int maxw = b.maxw;
    const int64_t npairs = b.npairs, npairs_all = b.npairs_all;
    // (what a range lasts is its busiest wavefront's tile steps - every range ends at a barrier: pairmax for the ordinary
    //  stream, maxw x tpc for a flat one, whose empty window slots are skipped but whose wavefronts all wait for a full one)
    int64_t classic_tiles = 0, classic_steps = 0, over[2] = {0, 0};
    for (int64_t k = 0; k < npairs_all; ++k)
        if (b.kmap[(size_t)k] >= 0) { classic_tiles += best.pairtiles[(size_t)k]; classic_steps += best.pairmax[(size_t)k];
                                      over[0] += best.pairover[(size_t)k]; over[1] += best.pairover[(size_t)(npairs_all + k)]; }
    b.classic_steps = classic_steps;
    const char* fenv = test_knob("TCGNN_LDS_FLAT");
    const int forced_flat = fenv ? atoi(fenv) : -1;
    if (best.nsplit == 0 && npairs > 0 && forced_flat != 0) {
        double best_cost = 0.0;
        for (int tpc = 1; tpc <= 2; ++tpc) {
            if (maxw * tpc > 16 || (b.val && tpc != 1)) break;   // (spmm_lds_val_kernel walks one tile per cell only)
            // (one tile per cell: the overflow of the dense pairs stays in the walk, as dense entries; their steps count)
            const int64_t kept = tpc == 1 ? b.over_dense : 0, extra_steps = tpc == 1 ? b.dense_steps : 0;
            const bool few_cold = (double)(b.cold_cols + over[tpc - 1] - kept) <= 0.04 * (double)std::max<int64_t>(b.hot_cols + b.cold_cols, 1);
            // (a flat step costs ~0.75 of an ordinary one - 1.46 against 1.84 us per range of ~8 steps on the Reddit shape - and a
            //  stream of nearly-empty cells, a wide row shard, ties on the count: 627 712 flat steps against 627 699)
            const bool no_more_steps = (double)(npairs * maxw * tpc + extra_steps) <= 1.2 * (double)std::max<int64_t>(classic_steps, 1);
            if (forced_flat == tpc) { b.flat_tpc = tpc; b.over_cols = over[tpc - 1] - kept; break; }
            if (forced_flat >= 0 || !few_cold || !no_more_steps) continue;
            // Both forms may qualify - the one-plane layout on the Reddit shape: 51 columns per 1 528-row cell, which one tile per cell
            // only holds with 93 % of the pairs dense (0.40 ms) and two tiles per cell hold as they are (0.21 ms) - so they are
            // priced: a flat step = 1, a dense entry's run-time step ~1.6 (31 instructions against 19), + ~4 steps per dense entry
            // (its barrier, metadata block and descriptor words).  Dense entries are for the EXCEPTIONS of a stream.
            const double cost = (double)(npairs * maxw * tpc) + (tpc == 1 ? 1.6 * (double)b.dense_steps + 4.0 * (double)b.ndense_entries : 0.0);
            if (!b.flat_tpc || cost < best_cost) { b.flat_tpc = tpc; b.over_cols = over[tpc - 1] - kept; best_cost = cost; }
        }
    }
    if (b.verbose) fprintf(stderr, "[tcgnn] cell stream %d: %lld tiles ordinary, %lld steps of the busiest wavefronts; flat would take %lld steps (+%lld columns cold; %lld dense pairs keep %lld columns "
                                   "in %lld dense entries, %lld steps) / %lld (+%lld): %s\n", b.slot,
                           (long long)classic_tiles, (long long)classic_steps, (long long)(npairs * maxw), (long long)(over[0] - b.over_dense), (long long)b.ndense_pairs, (long long)b.over_dense,
                           (long long)b.ndense_entries, (long long)b.dense_steps, (long long)(2 * npairs * maxw), (long long)over[1],
                           b.flat_tpc ? (b.flat_tpc == 1 ? "flat, 1 tile per cell" : "flat, 2 tiles per cell") : "ordinary");
}
// step 6: ... nor flat where ONE window would leave a long remainder behind (a hub row: its cells overflow in every range, and the
// remainder of a window is one wavefront's serial work - a 24 k-degree hub cost the flat walk 0.72 ms against 0.61): the remainder
// is counted with the flat cap before anything is built (cell_cold_count_kernel).  The counts leave the dense pairs' overflow out:
// they read the entry table, which therefore goes to the device first.
static int cells_hub_row_trial(CellBuild& b) {
    hipError_t e = hipSuccess;
    if (b.with_dense()) {
        b.ent = flat_entries(b.nwg, b.maxw, b.rbase, b.rlist, b.cnt, b.dense_mx, true, false);
        e = b.d_ent.alloc(b.ent.ent2.size());
        if (e == hipSuccess) e = hipMemcpyAsync(b.d_ent, b.ent.ent2.data(), b.ent.ent2.size() * sizeof(int32_t), hipMemcpyHostToDevice, b.stream);
        if (e != hipSuccess) return fail(hip_rc(e), "flat stream entries: %s", hipGetErrorString(e));
    }
    if (!b.flat_tpc || test_knob("TCGNN_LDS_FLAT")) return TCGNN_OK;
    DevBuf<uint32_t> d_trial;
    std::vector<uint32_t> trial((size_t)b.p->nw_eff, 0u);
    e = d_trial.alloc(trial.size());
    if (e == hipSuccess) e = hipMemsetAsync(d_trial, 0, trial.size() * sizeof(uint32_t), b.stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(cell_cold_count_kernel, dim3((unsigned)((b.nw + 255) / 256)), dim3(256), 0, b.stream, b.best.d_cellcols.ptr, b.d_kmap.ptr, b.best.d_sorder.ptr, b.nw, b.nranges, b.maxw,
                           d_trial.ptr, (uint32_t)(32 * b.flat_tpc), b.d_ent.ptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(trial.data(), d_trial, trial.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b.stream);
    if (e != hipSuccess) return fail(hip_rc(e), "cell table: %s", hipGetErrorString(e));
    uint32_t worst = 0;
    for (uint32_t c : trial) worst = std::max(worst, (c + 31u) / 32u);
    // ... counted against what the walk ADMITS: a wavefront multiplies one cold tile per entry - the long walk, whose four gather tiles
    // are shared, one per kLongTurn entries - and the rest of its list in a serial loop behind the walk: the same 16-tile bound
    const int turn = b.long_ranges() ? kLongTurn : 1;
    for (int g2 = 0; g2 < b.nwg; ++g2) {
        const int64_t entries = b.with_dense() ? b.ent.wg_first[(size_t)g2 + 1] - b.ent.wg_first[(size_t)g2] : b.rbase[(size_t)g2 + 1] - b.rbase[(size_t)g2];
        for (int v = 0; v < kLdsWaves; ++v) {
            int64_t tiles = 0;
            for (int j = 0; j < b.maxw; ++j) {
                const int w = b.best.sorder[(size_t)cell_position(g2, v, j, b.maxw)];
                if (w >= 0) tiles += (trial[(size_t)w] + 31u) / 32u;
            }
            b.trial_tiles += tiles;
            b.worst_tail = std::max(b.worst_tail, tiles - entries / turn);
        }
    }
    if (worst > 16u || (b.long_ranges() && b.worst_tail > 16)) {
        if (b.verbose) fprintf(stderr, "[tcgnn] cell stream %d: ordinary after all - one window would leave %u cold tiles behind, one wavefront %lld beyond its walk\n", b.slot, worst,
                               (long long)b.worst_tail);
        b.flat_tpc = 0; b.over_cols = 0;
    }
    return TCGNN_OK;
}
// step 7: the entries of the stream as it will be built (flat_entries) and, flat streams, their records on the device
static int cells_entries(CellBuild& b) {
    if (!b.with_dense()) { (void)hipStreamSynchronize(b.stream); b.d_ent.reset(); }   // (the trial may have sent the stream back to ordinary)
    b.cnt.resize((size_t)b.ncell_hot + 1);   // the hot cells' tile counts: the dense entries' records, an ordinary stream's cell table
    {
        hipError_t ec = hipMemcpyAsync(b.cnt.data(), b.d_cnt, b.cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream);
        if (ec == hipSuccess) ec = hipStreamSynchronize(b.stream);
        if (ec != hipSuccess) return fail(TCGNN_ERR_HIP, "cell count: %s", hipGetErrorString(ec));
    }
    FlatEntries ent = flat_entries(b.nwg, b.maxw, b.rbase, b.rlist, b.cnt, b.dense_mx, b.with_dense(), b.flat_tpc != 0);
    hipError_t e = hipSuccess;
    if (b.flat_tpc) {
        e = b.d_rl2.alloc(ent.rl2.size());
        if (e == hipSuccess) e = hipMemcpyAsync(b.d_rl2, ent.rl2.data(), ent.rl2.size() * sizeof(uint32_t), hipMemcpyHostToDevice, b.stream);
        if (e == hipSuccess && b.with_dense()) {
            e = b.d_xbase.alloc(ent.xbase.size());
            if (e == hipSuccess) e = hipMemcpyAsync(b.d_xbase, ent.xbase.data(), ent.xbase.size() * sizeof(uint32_t), hipMemcpyHostToDevice, b.stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(b.stream);
    }
    if (e != hipSuccess) return fail(hip_rc(e), "flat stream entries: %s", hipGetErrorString(e));
    b.ent = std::move(ent);   // (behind a synchronisation: the table the trial read was copied from the old one)
    return TCGNN_OK;
}
// step 8: the tiles (cell_init / cell_fill / cell_optimize) and, flat streams, their per-(pair, wavefront) metadata blocks
// (flat_transpose), after which the ordinary tiles and the cell table go
static int cells_fill_tiles(CellBuild& b) {
    const tcgnn_plan* p = b.p;
    const int flat_tpc = b.flat_tpc;
    b.hot_cols -= b.over_cols; b.cold_cols += b.over_cols;
    uint64_t run = 0;
    if (flat_tpc) run = (uint64_t)b.ent.nentries * (uint64_t)b.per_wg * (uint64_t)flat_tpc;   // (positions are computed: the table is not kept)
    else for (size_t k = 0; k < b.cnt.size(); ++k) { const uint32_t c = b.cnt[k]; b.cnt[k] = (uint32_t)run; run += c; }
    if (run >= (1ull << 32)) return fail(TCGNN_ERR_BAD_GRAPH, "LDS-range SpMM: %llu tiles overflow the 32-bit cell table", (unsigned long long)run);
    const int64_t ntiles = b.ntiles = (int64_t)run;
    const int64_t nwords = b.nwords = std::max<int64_t>(ntiles, 1) * kCellWords;
    hipError_t e = b.d_tiles.alloc((size_t)nwords);
    if (e == hipSuccess) e = hipMemcpyAsync(b.d_cnt, b.cnt.data(), b.cnt.size() * sizeof(uint32_t), hipMemcpyHostToDevice, b.stream);
    if (e != hipSuccess) return fail(hip_rc(e), "cell stream (%lld tiles): %s", (long long)ntiles, hipGetErrorString(e));
    hipLaunchKernelGGL(cell_init_kernel, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, b.stream, b.d_tiles.ptr, nwords, b.rows);
    if (b.val) {   // (flat only: build_lds_cells gives the stream up otherwise)
        e = b.d_eidx.alloc((size_t)std::max<int64_t>(ntiles, 1) * 32);
        if (e == hipSuccess) e = hipMemsetAsync(b.d_eidx, 0xff, b.d_eidx.bytes, b.stream);
        if (e != hipSuccess) return fail(hip_rc(e), "edge index of the cell stream: %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL(cell_fill_kernel, dim3((unsigned)b.nw), dim3(256), 0, b.stream, b.s_wb, b.best.d_sorder.ptr, b.s_cols, b.s_mask, b.nwg, b.nranges, p->Nc,
                       b.maxw, b.rows, b.d_cnt.ptr, b.best.d_firstq.ptr, b.d_tiles.ptr, b.d_kmap.ptr, b.best.d_parts.ptr, b.best.d_cellcols.ptr, flat_tpc, b.s_eidx, b.d_eidx.ptr, b.d_ent.ptr, b.d_xbase.ptr);
    if (ntiles > 0) hipLaunchKernelGGL(cell_optimize_kernel, dim3((unsigned)((ntiles + 255) / 256)), dim3(256), 0, b.stream, b.d_tiles.ptr, ntiles, b.rows, b.d_eidx.ptr);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(hip_rc(e), "cell fill: %s", hipGetErrorString(e));
    if (!flat_tpc) return TCGNN_OK;
    e = b.d_flat.alloc((size_t)nwords);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(flat_transpose_kernel, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, b.stream, b.d_tiles.ptr, b.d_flat.ptr, b.ent.nentries * kLdsWaves, b.maxw * flat_tpc, b.d_rl2.ptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(b.stream);
    b.d_tiles.reset();
    b.d_cnt.reset();
    if (e != hipSuccess) return fail(hip_rc(e), "flat cell stream: %s", hipGetErrorString(e));
    return TCGNN_OK;
}
// step 9: the cold remainder, re-condensed per window for the gather walk
static int cells_cold_remainder(CellBuild& b) {
    if (b.cold_cols <= 0) return TCGNN_OK;
    const tcgnn_plan* p = b.p;
    const int nwe = p->nw_eff;
    const uint32_t cap = (uint32_t)(32 * b.flat_tpc);
    std::vector<uint32_t> coldc((size_t)nwe, 0);
    DevBuf<uint32_t> d_coldcols;
    hipError_t e = d_coldcols.alloc((size_t)nwe);
    if (e == hipSuccess) e = hipMemsetAsync(d_coldcols, 0, (size_t)nwe * sizeof(uint32_t), b.stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(cell_cold_count_kernel, dim3((unsigned)((b.nw + 255) / 256)), dim3(256), 0, b.stream, b.best.d_cellcols.ptr, b.d_kmap.ptr, b.best.d_sorder.ptr, b.nw, b.nranges, b.maxw,
                           d_coldcols.ptr, cap, b.d_ent.ptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(coldc.data(), d_coldcols, coldc.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b.stream);
    b.cptr.assign((size_t)nwe + 1, 0);
    for (int w = 0; w < nwe; ++w) { b.cptr[(size_t)w + 1] = b.cptr[(size_t)w] + (coldc[(size_t)w] + 31) / 32; b.cold_max = std::max<int64_t>(b.cold_max, (coldc[(size_t)w] + 31) / 32); }
    b.cold_tiles = b.cptr[(size_t)nwe];
    const size_t ncold = (size_t)std::max<int64_t>(b.cold_tiles, 1);
    if (e == hipSuccess) e = b.d_cold_ptr.alloc(b.cptr.size());
    if (e == hipSuccess) e = b.d_ccols.alloc(ncold * kWbCols);
    if (e == hipSuccess) e = b.d_cmask.alloc(ncold * kWinRows);
    if (e == hipSuccess) e = hipMemcpyAsync(b.d_cold_ptr, b.cptr.data(), b.d_cold_ptr.bytes, hipMemcpyHostToDevice, b.stream);
    if (e == hipSuccess) e = hipMemsetAsync(b.d_cmask, 0, b.d_cmask.bytes, b.stream);
    if (e == hipSuccess) {
        // (padding columns of a window's last tile point at the all-zero sentinel row, like pack_kernel's)
        const int64_t nfill = (int64_t)ncold * kWbCols;
        hipLaunchKernelGGL(fill_i32_kernel, dim3((unsigned)std::min<int64_t>((nfill + 255) / 256, 65535)), dim3(256), 0, b.stream, b.d_ccols.ptr, nfill, p->Nc);
        e = hipGetLastError();
    }
    if (e == hipSuccess && b.val) {
        e = b.d_cold_eidx.alloc(ncold * 32);
        if (e == hipSuccess) e = hipMemsetAsync(b.d_cold_eidx, 0xff, b.d_cold_eidx.bytes, b.stream);
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(cell_cold_fill_kernel, dim3((unsigned)b.nw), dim3(256), 0, b.stream, b.s_wb, b.best.d_sorder.ptr, b.s_cols, b.s_mask, b.d_kmap.ptr, b.nranges, p->Nc,
                           b.maxw, b.rows, b.d_cold_ptr.ptr, b.d_ccols.ptr, b.d_cmask.ptr, b.best.d_parts.ptr, b.best.d_firstq.ptr, cap, b.s_eidx, b.d_cold_eidx.ptr, b.d_ent.ptr);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return fail(hip_rc(e), "cell fill: %s", hipGetErrorString(e));
    return TCGNN_OK;
}
// step 10: a flat stream whose layout leaves 16 x NT KB of LDS: the remainder as per-wavefront record lists, multiplied inside the
// flat kernel one tile per range (tcgnn_lds_flat.inc: cold_step) instead of by spmm_cold_planar_kernel afterwards.  Ends with the
// synchronisation every host table of the build waits for.
static int cells_wavefront_cold_lists(CellBuild& b) {
    hipError_t e = hipSuccess;
    if (!b.val && b.flat_tpc && b.cold_tiles > 0 && b.cold_tiles < (1ll << 28) && flat_cold_fits(lds_stream_nt(b.slot), b.maxw, b.flat_tpc, b.long_ranges())) {
        std::vector<int32_t>& wptr = b.wptr;
        std::vector<uint32_t>& wlist = b.wlist;
        wptr.assign((size_t)b.nwg * kLdsWaves + 1, 0);
        wlist.reserve((size_t)b.cold_tiles);
        for (int g2 = 0; g2 < b.nwg; ++g2)
            for (int v = 0; v < kLdsWaves; ++v) {
                wptr[(size_t)g2 * kLdsWaves + v] = (int32_t)wlist.size();
                for (int j = 0; j < b.maxw; ++j) {
                    const int w = b.best.sorder[(size_t)cell_position(g2, v, j, b.maxw)];
                    if (w < 0) continue;
                    for (int64_t t = b.cptr[(size_t)w]; t < b.cptr[(size_t)w + 1]; ++t) wlist.push_back((uint32_t)t | ((uint32_t)j << 28));
                }
            }
        wptr[(size_t)b.nwg * kLdsWaves] = (int32_t)wlist.size();
        DevBuf<uint32_t> d_wlist;
        e = b.d_wcold_ptr.alloc(wptr.size());
        if (e == hipSuccess) e = d_wlist.alloc(std::max<size_t>(wlist.size(), 1));
        if (e == hipSuccess) e = b.d_wcold.alloc(std::max<size_t>(wlist.size(), 1) * 64);
        if (e == hipSuccess) e = hipMemcpyAsync(b.d_wcold_ptr, wptr.data(), wptr.size() * sizeof(int32_t), hipMemcpyHostToDevice, b.stream);
        if (e == hipSuccess && !wlist.empty()) e = hipMemcpyAsync(d_wlist, wlist.data(), wlist.size() * sizeof(uint32_t), hipMemcpyHostToDevice, b.stream);
        if (e == hipSuccess && !wlist.empty()) {
            const int64_t nwordsw = (int64_t)wlist.size() * 64;
            hipLaunchKernelGGL(flat_cold_records_kernel, dim3((unsigned)((nwordsw + 255) / 256)), dim3(256), 0, b.stream, d_wlist.ptr, (int64_t)wlist.size(), b.d_ccols.ptr, b.d_cmask.ptr, b.d_wcold.ptr);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(b.stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(b.stream);   // host vectors must outlive their copies
    if (e != hipSuccess) return fail(hip_rc(e), "cell fill: %s", hipGetErrorString(e));
    return TCGNN_OK;
}
// step 11, the last fallible one: a flat stream is indexed by ENTRY: rbase[wg] = the workgroup's first entry
static int cells_flat_rbase(CellBuild& b) {
    if (!b.flat_tpc) return TCGNN_OK;
    hipError_t e = hipMemcpyAsync(b.d_rbase, b.ent.wg_first.data(), b.ent.wg_first.size() * sizeof(int32_t), hipMemcpyHostToDevice, b.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b.stream);
    if (e != hipSuccess) return fail(TCGNN_ERR_HIP, "flat stream entries: %s", hipGetErrorString(e));
    return TCGNN_OK;
}
// step 12: publication.  Cannot fail, and is the only writer of plan->lds[slot]: every fallible operation lies before it, so a
// failed build leaves the slot exactly as it found it (nothing the plan points at is ever freed by the build, nothing is freed
// twice).  The stream's arrays leave their DevBufs for the plan, the bytes they hand over are what plan->bytes grows by, and nranges
// is stored last, with release ordering: a reader that sees it sees the stream.  *build_only_bytes (if asked for): the part of
// those bytes the caller will release again (the 32-bit edge index of the single-edge stream).
static void cells_publish(CellBuild& b, size_t* build_only_bytes) {
    tcgnn_plan::CellStream& cs = b.p->lds[b.slot];
    const int64_t nentries = b.ent.nentries;
    const bool wcold = b.d_wcold_ptr != nullptr;
    size_t bytes = 0, build_only = 0;
    bytes += b.best.d_sorder.release(cs.d_order);
    bytes += b.d_cnt.release(cs.d_cell_ptr);
    bytes += b.d_tiles.release(cs.d_cell_tiles);
    bytes += b.d_flat.release(cs.d_flat);
    bytes += b.d_wcold_ptr.release(cs.d_wcold_ptr);
    bytes += b.d_wcold.release(cs.d_wcold);
    build_only += b.d_eidx.release(cs.d_eidx);
    build_only += b.d_cold_eidx.release(cs.d_cold_eidx);
    bytes += b.d_rbase.release(cs.d_rbase);
    bytes += b.d_rlist.release(cs.d_rlist);
    bytes += b.d_rl2.release(cs.d_rl2);
    bytes += b.best.d_parts.release(cs.d_parts);
    bytes += b.d_cold_ptr.release(cs.d_cold_ptr);
    bytes += b.d_ccols.release(cs.d_cold_cols);
    bytes += b.d_cmask.release(cs.d_cold_mask);
    cs.flat_tpc = b.flat_tpc;
    cs.nwg = b.nwg; cs.tiles = b.ntiles;
    cs.npairs = (int32_t)nentries; cs.dense_entries = (int32_t)(nentries - b.npairs);
    cs.cold_tiles = b.cold_tiles; cs.hot_cols = b.hot_cols; cs.cold_cols = b.cold_cols; cs.cold_max = b.cold_max;
    cs.nsplit = b.best.nsplit;
    if (b.verbose)
        fprintf(stderr, "[tcgnn] cell stream %d (%d windows per wavefront, %d-row ranges): %d workgroups x %d ranges, %lld of %lld pairs hot (>= %u columns), "
                        "%lld columns hot / %lld cold, %lld tiles + %lld cold gather tiles, placement %s\n",
                b.slot, b.maxw, b.rows, b.nwg, b.nranges, (long long)b.npairs, (long long)b.npairs_all, b.best.hot_min, (long long)b.hot_cols, (long long)b.cold_cols,
                (long long)b.ntiles, (long long)b.cold_tiles, b.best.mode == kPlaceGlobal ? "longest-first over the graph" : "contiguous blocks");
    if (b.verbose && b.flat_tpc) fprintf(stderr, "[tcgnn]   flat: %d tile(s) per cell, %lld entries (%lld dense), %lld columns beyond the cells' tiles moved to the cold remainder (%s)\n", b.flat_tpc,
                                         (long long)nentries, (long long)(nentries - b.npairs), (long long)b.over_cols,
                                         wcold ? "multiplied inside the kernel, one tile per range" : "added by spmm_cold_planar_kernel");
    if (b.verbose && b.best.nsplit) fprintf(stderr, "[tcgnn]   %d windows split over several wavefronts\n", b.best.nsplit);
    b.p->bytes += bytes + build_only;
    if (build_only_bytes) *build_only_bytes = build_only;
    cs.nranges.store(b.nranges, std::memory_order_release);
}

// the arrays of a cell stream, all of them: what tcgnn_plan_destroy frees
static void release_cell_stream(tcgnn_plan::CellStream& cs) {
    for (void* q : {(void*)cs.d_order, (void*)cs.d_rbase, (void*)cs.d_rlist, (void*)cs.d_rl2, (void*)cs.d_parts, (void*)cs.d_cold_ptr, (void*)cs.d_cold_cols, (void*)cs.d_cold_mask,
                    (void*)cs.d_cell_ptr, (void*)cs.d_cell_tiles, (void*)cs.d_flat, (void*)cs.d_wcold_ptr, (void*)cs.d_wcold, (void*)cs.d_eidx, (void*)cs.d_cold_eidx, (void*)cs.d_eidx16,
                    (void*)cs.d_cold_eidx16}) (void)hipFree(q);
}

// (a walk of fewer entries per workgroup is over before the per-entry fixed cost adds up: not worth planning a second stream)
static constexpr int kLongMinEntries = 32;
// the geometry of slot `slot`'s stream and what it is cut from
static void cells_begin(CellBuild& b, tcgnn_plan* p, hipStream_t stream, int slot) {
    b.p = p; b.stream = stream; b.slot = slot;
    b.val = slot == kLdsValSlot;
    b.s_wb = b.val ? p->d_xwb_ptr : p->d_wb_ptr;
    b.s_cols = b.val ? p->d_xcols : p->d_cols;
    b.s_mask = b.val ? p->d_xmask : p->d_mask;
    b.s_eidx = b.val ? p->d_xeidx : nullptr;
    b.maxw = lds_stream_maxw(slot);
    b.rows = lds_stream_buf_rows(slot) - 8;
    b.nranges = (p->Nc + b.rows - 1) / b.rows;
    b.per_wg = kLdsWaves * b.maxw;
    b.nwg = lds_workgroups(p, b.maxw);
    b.nw = b.nwg * b.per_wg;
    b.ncell = (int64_t)b.nwg * b.nranges * b.per_wg;
    b.npairs_all = (int64_t)b.nwg * b.nranges;
    b.verbose = verbose_level() > 0;
}
// What a stream will cost a workgroup on average, in flat tile steps, from the counts made before anything is built: a flat step is
// 1, an ordinary stream's step 1 / 0.75, a dense entry's step 1.6 + 4 per dense entry (cells_flat_or_ordinary's weights); every entry
// costs the fixed ~1500 cycles tcgnn_lds_spmm.inc quotes on top - metadata latency, end-of-entry wait, barrier: 6 steps of ~260 cycles;
// a cold tile inside the walk ~2 steps, one in the serial loop behind the walk a memory round trip, ~10.
static double cells_price(const CellBuild& b) {
    const double entries = (double)b.npairs + (b.flat_tpc == 1 ? (double)b.ndense_entries : 0.0);
    double steps;
    if (b.flat_tpc == 1) steps = (double)(b.npairs * b.maxw) + 1.6 * (double)b.dense_steps + 4.0 * (double)b.ndense_entries;
    else if (b.flat_tpc == 2) steps = 2.0 * (double)(b.npairs * b.maxw);
    else steps = (double)b.classic_steps / 0.75;
    const double per_wg = (6.0 * entries + steps) / std::max(b.nwg, 1);
    return per_wg + 2.0 * (double)b.trial_tiles / ((double)std::max(b.nwg, 1) * kLdsWaves) + 10.0 * (double)std::max<int64_t>(b.worst_tail, 0);
}
// steps 1 - 6: everything that is decided before anything is built, and the stream's price
static int cells_plan(CellBuild& b) {
    if (const int rc = cells_window_weights(b)) return rc;
    if (const int rc = cells_choose_placement(b)) return rc;
    if (const int rc = cells_hot_pairs(b)) return rc;
    cells_dense_pairs(b);
    cells_flat_or_ordinary(b);
    if (const int rc = cells_hub_row_trial(b)) return rc;
    b.price = cells_price(b);
    return TCGNN_OK;
}
static int build_lds_cells(tcgnn_plan* p, hipStream_t stream, int slot, size_t* build_only_bytes = nullptr) {
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    const bool two_lengths = slot == lds_stream_of(2, kLdsMaxW2) || slot == kLdsLongSlot;
    int8_t decided = two_lengths ? p->lds_long.load(std::memory_order_acquire) : (int8_t)0;
    if (two_lengths) slot = lds_stream_of(2, kLdsMaxW2, decided == 1);
    if (p->lds[slot].nranges > 0) return TCGNN_OK;
    if (p->nw_eff <= 0 || p->Nc <= 0) return fail(TCGNN_ERR_INVALID_ARG, "LDS-range SpMM: empty graph");
    if (slot == kLdsValSlot && !p->d_xwb_ptr) return fail(TCGNN_ERR_INVALID_ARG, "edge-valued LDS-resident SpMM: the single-edge stream has not been built");
    std::unique_ptr<CellBuild> bp(new CellBuild);
    cells_begin(*bp, p, stream, slot);
    if (const int rc = cells_plan(*bp)) return rc;
    if (two_lengths && decided < 0) {
        // 760- or 952-row ranges: the long stream is priced too - unless its cells would plainly overflow their one tile (the uniform
        // Reddit shape: 25.7 columns per 760-row cell are 32 per 952-row cell) - and the cheaper one is built; the other's tables go
        // before anything is (plan_bytes carries one stream)
        CellBuild& s = *bp;
        const double cells = (double)std::max<int64_t>(s.npairs, 1) * std::min<double>(s.per_wg, std::ceil((double)p->nw_eff / std::max(s.nwg, 1)));
        const double fill_long = (double)(s.hot_cols - s.over_dense) / cells * (double)(lds_stream_buf_rows(kLdsLongSlot) - 8) / (double)s.rows;
        bool take_long = false;
        const int knob = lds_long_knob();
        if (knob == 0) { if (s.verbose) fprintf(stderr, "[tcgnn] range length: 760 rows (TCGNN_LDS_LONG=0)\n"); }
        else if (knob < 0 && s.npairs < (int64_t)kLongMinEntries * s.nwg) {
            if (s.verbose) fprintf(stderr, "[tcgnn] range length: 760 rows; 952-row ranges not priced: %lld entries in %d workgroups\n", (long long)s.npairs, s.nwg);
        } else if (knob < 0 && fill_long > 30.0) {
            if (s.verbose) fprintf(stderr, "[tcgnn] range length: 760 rows, price %.0f steps per workgroup; 952-row ranges not priced: their ordinary cells would hold %.1f columns of 32\n", s.price, fill_long);
        } else {
            std::unique_ptr<CellBuild> bl(new CellBuild);
            cells_begin(*bl, p, stream, kLdsLongSlot);
            if (const int rc = cells_plan(*bl)) return rc;
            const bool buildable = bl->flat_tpc == 1;
            take_long = buildable && (knob == 1 || bl->price < s.price);
            if (s.verbose) fprintf(stderr, "[tcgnn] range length: 760 rows: %lld entries, price %.0f steps per workgroup; 952 rows: %lld entries, price %.0f%s: %d-row ranges%s\n",
                                   (long long)(s.npairs + (s.flat_tpc == 1 ? s.ndense_entries : 0)), s.price, (long long)(bl->npairs + (bl->flat_tpc == 1 ? bl->ndense_entries : 0)), bl->price,
                                   buildable ? "" : " (not a flat stream with one tile per cell: cannot be built)", take_long ? 952 : 760, knob == 1 ? " (TCGNN_LDS_LONG=1)" : "");
            (void)hipStreamSynchronize(stream);
            if (take_long) { bp = std::move(bl); slot = kLdsLongSlot; }
        }
        p->lds_long.store(take_long ? 1 : 0, std::memory_order_release);
    }
    CellBuild& b = *bp;
    if (const int rc = cells_entries(b)) return rc;
    if (b.val && b.flat_tpc != 1)   // (spmm_lds_val_kernel walks flat streams with one tile per cell only; the caller keeps the gather walks)
        return fail(TCGNN_ERR_UNSUPPORTED, "edge-valued LDS-resident SpMM: the single-edge cells of this graph are not uniform enough for a flat stream");
    if (const int rc = cells_fill_tiles(b)) return rc;
    if (const int rc = cells_cold_remainder(b)) return rc;
    if (const int rc = cells_wavefront_cold_lists(b)) return rc;
    if (const int rc = cells_flat_rbase(b)) return rc;
    cells_publish(b, build_only_bytes);
    return TCGNN_OK;
}

// ---- the edge-valued LDS-resident walk (tcgnn_lds_val.inc): single-edge tile stream + its flat cell stream (slot kLdsValSlot).
// Built on the first edge-valued call that would use it (allocates and synchronises: never inside a graph capture); the answer -
// usable or not - is remembered in plan->val_choice.
// step 1: the single-edge source stream, handed to the plan (build_lds_cells cuts slot kLdsValSlot from it).  *usable = false: the
// graph has a window the stream cannot hold; *bytes: what the plan was handed.
static int val_source_stream(tcgnn_plan* p, hipStream_t stream, bool* usable, size_t* bytes) {
    const int nw = p->nw_eff;
    *usable = false; *bytes = 0;
    DevBuf<int32_t> d_ew, d_flags, d_xc, d_xe;
    DevBuf<int64_t> d_xp;
    DevBuf<uint32_t> d_xm;
    std::vector<int32_t> ew((size_t)nw, 0);
    hipError_t e = d_ew.alloc((size_t)nw);
    if (e == hipSuccess) e = d_flags.alloc(1);
    if (e == hipSuccess) e = hipMemsetAsync(d_flags, 0, sizeof(int32_t), stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(window_edges_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, stream, p->rowptr, p->N, nw, d_ew.ptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(ew.data(), d_ew, (size_t)nw * sizeof(int32_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    d_ew.reset();
    std::vector<int64_t> xptr((size_t)nw + 1, 0);
    for (int w = 0; w < nw; ++w) xptr[(size_t)w + 1] = xptr[(size_t)w] + (ew[(size_t)w] + kWbCols - 1) / kWbCols;
    const int64_t total = std::max<int64_t>(xptr[(size_t)nw], 1);
    if (e == hipSuccess) e = d_xp.alloc(xptr.size());
    if (e == hipSuccess) e = d_xc.alloc((size_t)total * kWbCols);
    if (e == hipSuccess) e = d_xe.alloc((size_t)total * kWbCols);
    if (e == hipSuccess) e = d_xm.alloc((size_t)total * kWinRows);
    if (e == hipSuccess) e = hipMemcpyAsync(d_xp, xptr.data(), xptr.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_xe, 0xff, d_xe.bytes, stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_xm, 0, d_xm.bytes, stream);
    if (e == hipSuccess) {   // (padding slots point at the all-zero sentinel row, like pack_kernel's; filled on the device - ADVICE r04: a 460 MB host vector)
        const int64_t nfill = total * kWbCols;
        hipLaunchKernelGGL(fill_i32_kernel, dim3((unsigned)std::min<int64_t>((nfill + 255) / 256, 65535)), dim3(256), 0, stream, d_xc.ptr, nfill, p->Nc);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(stream);   // (xptr must outlive its copy)
    }
    int32_t bad = 0;
    if (e == hipSuccess && nw > 0) {
        hipLaunchKernelGGL(expand_edges_kernel, dim3((unsigned)nw), dim3(256), 0, stream, p->d_wb_ptr, p->d_cols, p->d_mask, p->d_ebase, d_xp.ptr, d_xc.ptr, d_xm.ptr, d_xe.ptr, p->Nc, d_flags.ptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_flags, sizeof(int32_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(hip_rc(e), "single-edge tile stream: %s", hipGetErrorString(e));
    if (bad) return TCGNN_OK;
    *bytes = d_xp.release(p->d_xwb_ptr) + d_xc.release(p->d_xcols) + d_xm.release(p->d_xmask) + d_xe.release(p->d_xeidx);
    p->total_xwb = xptr[(size_t)nw];
    p->bytes += *bytes;
    *usable = true;
    return TCGNN_OK;
}
// step 3 (step 2 is build_lds_cells): CSR positions -> 16-bit offsets into each window's run of edges (half the index bytes per
// call and in the plan); returns whether the stream can be used
static bool val_index16(tcgnn_plan* p, hipStream_t stream) {
    tcgnn_plan::CellStream& cs = p->lds[kLdsValSlot];
    const size_t nt = (size_t)std::max<int64_t>(cs.tiles, 1), nc = (size_t)std::max<int64_t>(cs.cold_tiles, 1);
    DevBuf<uint16_t> d_e16, d_cold_e16;
    DevBuf<int32_t> d_bad;
    int32_t bad = 0;
    hipError_t e = d_e16.alloc(nt * 32);
    if (e == hipSuccess) e = d_cold_e16.alloc(nc * 32);
    if (e == hipSuccess) e = d_bad.alloc(1);
    if (e == hipSuccess) e = hipMemsetAsync(d_bad, 0, sizeof(int32_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_e16, 0xff, d_e16.bytes, stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(val_index16_kernel, dim3((unsigned)(cs.nwg * kLdsWaves * kLdsMaxW2)), dim3(256), 0, stream, p->rowptr, cs.d_order, cs.d_eidx, cs.d_rbase, d_e16.ptr, p->N,
                           kLdsMaxW2, cs.cold_tiles > 0 ? cs.d_cold_ptr : nullptr, cs.d_cold_eidx, d_cold_e16.ptr, d_bad.ptr, cs.d_rl2, std::max(cs.npairs, 1));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, sizeof(int32_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess || bad) return false;
    p->bytes += d_e16.release(cs.d_eidx16) + d_cold_e16.release(cs.d_cold_eidx16);
    return true;
}
static int build_val_stream(tcgnn_plan* p, hipStream_t stream) {
    // (ADVICE r04: ONE lock over the whole build - the single-edge source, the cell stream cut from it and the frees behind it; two
    //  threads making a plan's first edge-valued call used to be able to build, and free, the same arrays twice)
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    if (p->val_choice.load(std::memory_order_acquire) >= 0) return TCGNN_OK;
    bool usable;
    size_t source_bytes, eidx_bytes = 0;
    const int src = val_source_stream(p, stream, &usable, &source_bytes);
    if (!usable) { p->val_choice.store(0, std::memory_order_release); return src; }
    const int rc = build_lds_cells(p, stream, kLdsValSlot, &eidx_bytes);
    tcgnn_plan::CellStream& cs = p->lds[kLdsValSlot];
    const bool ok = rc == TCGNN_OK && cs.nranges > 0 && cs.flat_tpc == 1 && cs.nsplit == 0 && cs.d_eidx && val_index16(p, stream);
    if (cs.d_eidx) {   // (the 32-bit index is build-time only)
        (void)hipStreamSynchronize(stream);
        p->bytes -= eidx_bytes;
        (void)hipFree(cs.d_eidx); (void)hipFree(cs.d_cold_eidx); cs.d_eidx = nullptr; cs.d_cold_eidx = nullptr;
    }
    // (the single-edge source is only needed to cut the cell stream: 0.9 GB on the Reddit shape, released here)
    (void)hipStreamSynchronize(stream);
    p->bytes -= source_bytes;
    (void)hipFree(p->d_xwb_ptr); (void)hipFree(p->d_xcols); (void)hipFree(p->d_xmask); (void)hipFree(p->d_xeidx);
    p->d_xwb_ptr = nullptr; p->d_xcols = nullptr; p->d_xmask = nullptr; p->d_xeidx = nullptr;
    p->val_choice.store(ok ? 1 : 0, std::memory_order_release);
    return (rc == TCGNN_ERR_OOM || rc == TCGNN_ERR_HIP) ? rc : TCGNN_OK;
}
// bytes the per-call slot values take behind the planar image (the stream's tiles and its cold tiles, 64 bytes each)
static size_t val_stream_bytes(const tcgnn_plan* p) {
    const tcgnn_plan::CellStream& cs = p->lds[kLdsValSlot];
    if (p->val_choice.load(std::memory_order_acquire) != 1) return 0;
    return ((size_t)(std::max<int64_t>(cs.tiles, 1) + std::max<int64_t>(cs.cold_tiles, 0)) * 64 + 255) / 256 * 256;
}
