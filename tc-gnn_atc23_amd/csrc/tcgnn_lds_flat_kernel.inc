// tcgnn_lds_flat_kernel.inc - the body of spmm_lds_flat_kernel (tcgnn_lds_flat.inc), included twice: as the plain kernel and as
// spmm_lds_flat_epi_kernel, the same walk with tcgnn_spmm_scaled's row scale / bias in the final store.  The macros expand, for the
// plain kernel, to exactly the tokens it was written with, so its code does not change.
// TCGNN_KERNEL_LONG = true: the same walk over 952-row ranges (960-row buffers, cell stream slot kLdsLongSlot) - a kernel of its own name
// rather than one more template parameter, which would rename every existing instantiation.  Everything it does differently stands
// under `if constexpr (LONG)`: the buffer rows, and the cold remainder's gather tiles, of which the 160 KB then hold four, shared.
template <int NT, int MAXW, int TPC, bool DBG, bool WITH_DENSE>
__global__ __launch_bounds__(kLdsWaves * 64) void TCGNN_KERNEL_NAME(TCGNN_KERNEL_PARAM) {
    TCGNN_KERNEL_PROLOGUE
    if (range_is_wide(a.hdr, 0)) { lds_own_fallback(a.fb); return; }   // (range guard: the fp32 walk does the work - here, or in a launch behind this one)
    const int dbg = DBG ? a.dbg : 0;
    constexpr bool LONG = TCGNN_KERNEL_LONG;
    static_assert(!LONG || (NT == 2 && MAXW == 8 && TPC == 1), "the long ranges exist for whole 64-column chunks only");
    constexpr int kLdsBufRows = lds_buf_rows(NT, MAXW, LONG), kLdsRows = kLdsBufRows - 8;
    constexpr int T = MAXW * TPC, PADB = T * 128, kLdsChunkDims = lds_chunk_dims(MAXW);
    static_assert(NT * MAXW <= 16, "accumulators: NT * MAXW * 4 VGPRs");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int PLANEB = kLdsBufRows * 32, BUFB = NT * PLANEB;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, i = lane & 15;
    const int wg = blockIdx.x;
    const int chunk_id = a.chunk0 + (int)blockIdx.y;
    const int coloff = chunk_id * kLdsChunkDims;
    const uint32_t lds0 = (uint32_t)(uintptr_t)((LDS_AS char*)smem);
    const uint32_t pad0 = lds0 + 2 * BUFB + (uint32_t)wave * (2 * PADB);
    const int kx = scale_exp_from_bits(a.hdr[kHdrMaxX]);

    // (the window ids are read again in the epilogue instead of living through the walk: eight scalar registers the entry words and
    //  the dense walk need - the kernel spilled scalars into a vector register's lanes)
    floatx4 acc[MAXW][NT];
#pragma unroll
    for (int j = 0; j < MAXW; ++j) {
#pragma unroll
        for (int s = 0; s < NT; ++s) acc[j][s] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    const bool last_valid = MAXW == 1 || __builtin_amdgcn_readfirstlane(a.order[cell_position(wg, wave, MAXW - 1, MAXW)]) >= 0;   // (slots fill in order: an empty one is the last)
    const uint32_t last_on = (uint32_t)__builtin_amdgcn_readfirstlane(last_valid ? 1 : 0);   // (an SGPR for the "s" operand of lds_flat_step_if)
    const uint32_t lanebase = lds0 + (uint32_t)(i & 3) * 8u;
    const uint32_t idoff = (uint32_t)(4 * g + (i >> 2)) * (uint32_t)(T * 4);
    const uint32_t moff = (uint32_t)(64 * T) + (uint32_t)lane * (uint32_t)T;
    // who fills: the wavefronts whose last window slot is empty, if there are enough of them (FlatRangeFiller); the sixteen flags
    // meet in the first bytes of LDS before anything else lands there
    int fill_rank = wave, fill_n = kLdsWaves;
    {
        LDS_AS uint32_t* flags = (LDS_AS uint32_t*)smem;
        if (lane == 0) flags[wave] = last_valid ? 1u : 0u;
        __syncthreads();
        const uint32_t full = (uint32_t)(__ballot(lane < kLdsWaves && flags[lane < kLdsWaves ? lane : 0] != 0u) & 0xffffull);
        __syncthreads();                                             // (the flags are read before the first fill may overwrite them)
        const uint32_t light = ~full & 0xffffu;
        const int nlight = __builtin_popcount(light);
        if (nlight >= FlatRangeFiller<NT, kLdsBufRows>::kMinFillers && nlight < kLdsWaves && a.fill_quota) {
            fill_n = nlight;
            fill_rank = last_valid ? -1 : __builtin_popcount(light & ((1u << wave) - 1u));
        }
    }
    const FlatRangeFiller<NT, kLdsBufRows> filler(a.x16, a.xrows, chunk_id * (kLdsChunkDims / 16), a.stride, fill_rank, fill_n, lane);
    const int rb = a.rbase[wg], nr = a.rbase[wg + 1] - rb;
    const char* const bb0 = reinterpret_cast<const char*>(a.blocks) + ((int64_t)rb * kLdsWaves + wave) * PADB;
    const uint32_t lane16 = (uint32_t)lane * 16u;
    // metadata block of this wavefront in pair rb + r -> pad
    auto meta_dma = [&](int r, uint32_t padaddr) {
        const char* src = bb0 + (int64_t)r * (kLdsWaves * PADB);
#pragma unroll
        for (int q = 0; q < (PADB + 1023) / 1024; ++q)
            if (lane16 + 1024u * q < (uint32_t)PADB)
                __builtin_amdgcn_global_load_lds((GLB_AS const void*)(src + 1024 * q + lane16), (LDS_AS void*)(uintptr_t)(padaddr + 1024u * q), 16, 0, 0);
    };
    // the words of entry rb + r for this wavefront: every lane loads the same 16 bytes with an ORDINARY load, requested with the
    // metadata at the end of an entry and used after the next end-of-entry wait (a scalar load would sit in front of the first LDS
    // block's lgkmcnt(0))
    // (exactly the two words the kernel reads are loaded: a register of a wider load that nobody reads is handed to other values while
    //  the load is in flight, and hipcc then waits vmcnt(0) before writing it - with a 16-byte load in the middle of the walk, the
    //  uniform Reddit shape 0.52 -> 0.63 ms; with a 12-byte load whose middle word was unused, at the top of every entry right behind
    //  the range fill in every instantiation but <2, 8, 1>, and in the edge-valued walk: 0.56 -> 0.70 ms there)
    const uint32_t* const rlp = a.rl2 + (int64_t)rb * 4;
    auto load_info = [&](int r_) -> uintx2 { return *reinterpret_cast<const uintx2*>(rlp + (int64_t)r_ * 4); };
    // a dense entry's descriptor word of this wavefront (dense phase only)
    const uint32_t* const dscp = a.rl2 + (int64_t)a.nent * 4 + ((int64_t)rb * kLdsWaves + wave);
    auto load_desc = [&](int r_) -> uint32_t { return dscp[(int64_t)r_ * kLdsWaves]; };
    // (dense entries exist in streams with one tile per cell and at most two planes - what whole 64-column chunks and the one- and
    //  two-plane remainders use; the three- and four-plane passes have no register for the entry words: flat_dense_ok, build_lds_cells)
    constexpr bool DENSE = WITH_DENSE && flat_dense_ok(NT, MAXW, TPC);

    // ---- the cold remainder inside the kernel.  A cell's columns beyond its tiles (~1 % on the Reddit shape) used to be added by a
    // second kernel (69 - 105 us: ~3 tiles per window, every one a chain of memory round trips, plus a read-modify-write of all of
    // Y).  Here every wavefront owns the cold tiles of its own windows and multiplies ONE per range, at the end-of-range point where
    // it waits for its loads anyway: the record (column ids, mask words, window slot) is requested two ranges ahead with ordinary
    // loads, the 32 rows are gathered one range ahead by NT LDS-DMA instructions into a private 32 x NT x 32-byte tile in the same
    // planar format as the range buffers, and the tile step runs behind the wait that retires them - nothing new is waited for.
    // LONG: the LDS behind the pads holds kLongPoolTiles = 4 gather tiles, not sixteen.  Wavefront v uses tile v >> 2 and may ISSUE a
    // gather only at the end of an entry r with (r & 7) == 2 (v & 3); it multiplies the tile at the end of entry r + 1, as ever, and the
    // tile's next user issues at the end of entry r + 2 - behind the barrier that ends entry r + 1.  No two wavefronts ever have the
    // same tile in flight and nothing new is waited for; the test is wave-uniform scalar code.  A wavefront so retires at most one cold
    // tile per eight entries (a private tile was in use in 1 - 2 % of the entries); what it cannot place in the walk is left to the
    // loop behind it, where every wavefront has a private tile again: the range buffers are free by then.
    constexpr bool CAN_COLD = flat_cold_fits(NT, MAXW, TPC, LONG);
    uint32_t cbuf = lds0 + (uint32_t)flat_lds_main(NT, MAXW, TPC, LONG) + (uint32_t)(LONG ? wave >> 2 : wave) * (NT * 1024u);
    const int cold_turn = 2 * (wave & 3);   // (LONG)
    int cold_c = 0, cold_n = 0, j_cur = 0;
    bool have_g = false, have_n = false;
    uint32_t cid_n = 0u, mw_n = 0u, mw_cur = 0u;   // (cid_n: row id | window slot << 28)
    auto cold_request = [&]() {   // the next record of this wavefront's list -> registers (ordinary loads, first read behind the next end-of-range wait)
        have_n = cold_c < cold_n;
        if (have_n) {
            const uint32_t* rec = a.wcold + (int64_t)cold_c * 64;
            const uint32_t l2 = lane_id_now();
            cid_n = rec[l2 >> 1]; mw_n = rec[32 + (l2 & 15u)];
            ++cold_c;
        }
    };
    auto cold_step = [&](bool issue_ok) {      // (behind a wait_vm0; issue_ok: always, but for LONG outside this wavefront's turn)
        if (have_g) {             // the tile gathered during the range that just ended
            // (the lane id is re-derived here - mbcnt - so that this address is recomputed at its rare uses instead of living
            //  through the main loop: the kernel has exactly the 128 registers sixteen wavefronts per CU leave, and hipcc spilled it)
            const uint32_t l2 = lane_id_now();
            const uint32_t ad0 = cbuf + ((l2 >> 4) * 8u + ((l2 & 15u) >> 2)) * 32u + (l2 & 3u) * 8u;
            half4 lo[NT], hi[NT];
            flat_issue<NT, 1024>(ad0, ad0 + 128u, lo, hi);
            flat_drain<NT>(lo, hi);
            const half8 af = afrag_from_byte((mw_cur >> (8 * g)) & 0xffu);
            // (the window slot is only known at run time: the product goes to a scratch accumulator and is ADDED to the slot's under
            //  a wave-uniform branch - MFMAs on acc[j_cur] under eight branches made hipcc shuttle the accumulators through copies)
            floatx4 cacc[NT];
#pragma unroll
            for (int s = 0; s < NT; ++s) {
                const half8 bf = __builtin_shufflevector(lo[s], hi[s], 0, 1, 2, 3, 4, 5, 6, 7);
                cacc[s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf, floatx4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            }
#pragma unroll
            for (int jj = 0; jj < MAXW; ++jj) {
                if (j_cur == jj) {
#pragma unroll
                    for (int s = 0; s < NT; ++s) acc[jj][s] += cacc[s];
                }
            }
        }
        const bool go = have_n && issue_ok;
        have_g = go;
        if (go) {                 // gather the rows of the record requested a range ago: lane l fetches half l % 2 of row l / 2, one plane per instruction
            const int plane0 = chunk_id * (kLdsChunkDims / 16);
#pragma unroll
            for (int s = 0; s < NT; ++s) {
                const bool real = plane0 + s < a.stride;
                const int64_t recrow = real ? (int64_t)(plane0 + s) * a.xrows + (int64_t)(cid_n & 0x0fffffffu) : (int64_t)a.xrows - 1;   // (a plane beyond the matrix: the zero row)
                const char* src = reinterpret_cast<const char*>(a.x16) + (recrow << 5) + (lane & 1) * 16;
                __builtin_amdgcn_global_load_lds((GLB_AS const void*)src, (LDS_AS void*)(uintptr_t)(cbuf + (uint32_t)s * 1024u), 16, 0, 0);
            }
            mw_cur = mw_n;
            j_cur = __builtin_amdgcn_readfirstlane((int)(cid_n >> 28));
        }
        if (issue_ok) cold_request();   // (a record that has to wait for its turn stays where it is)
    };
    if constexpr (CAN_COLD) {
        if (a.wcold_ptr) {
            cold_c = a.wcold_ptr[wg * kLdsWaves + wave];
            cold_n = a.wcold_ptr[wg * kLdsWaves + wave + 1];
            cold_request();
        }
    }
    // ---- the walk: this workgroup's entries rb .. rb + nr - 1, NORMAL entries first (one per hot pair, in range order), then the
    //      DENSE entries of its dense pairs, grouped by pair.  Two loops, one per kind: with both bodies in one loop hipcc kept two
    //      sets of sites that modify the 64 accumulators apart by spilling them (208 bytes of scratch in the <2, 8, 1> kernel).
    //      Entry words (one 8-byte load per wavefront and entry, requested an entry ahead): w0 = column range | bit 31 dense |
    //      bit 30 "another range than the entry before: the other buffer"; w1 = dense: tiles per window slot, 4 bits each (a descriptor word behind the records);
    //      w2 (record word 1) = the range to fetch at the top of this entry into the other buffer (the next normal entry's; for the first entry of
    //      a dense group the next group's; ~0: none).
    uint32_t ew0 = 0u, ew1 = 0u, ew2 = ~0u;   // the current entry's words (SGPRs)
    uintx2 einfo = {0u, ~0u};             // the next entry's, in flight
    if (nr > 0) {
        const uintx2 e0 = load_info(0);
        ew0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)e0[0]);
        ew2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)e0[1]);
        meta_dma(0, pad0);
        if (nr > 1) meta_dma(1, pad0 + PADB);
        filler.fill((int)(ew0 & 0x3fffffffu) * kLdsRows, lds0);
        einfo = load_info(nr > 1 ? 1 : 0);
    }
    wait_vm0();
    __syncthreads();
    uint32_t ph[4] = {0, 0, 0, 0};   // (32-bit cycle sums: the timing instantiation has no registers to spare either)
    uint32_t buf = 0u;               // range buffer of the current entry
    int r = 0;
    uint32_t t0 = 0u, t1 = 0u, t2 = 0u;
    // top of an entry: the fill its w2 names goes out, into the buffer the entries before this one have finished with
    auto entry_top = [&]() {
        t0 = (dbg & 16) ? (uint32_t)__builtin_readcyclecounter() : 0u;
        if (ew2 != ~0u && !(dbg & 1)) filler.fill((int)((dbg & 128) ? (ew2 & 7u) : ew2) * kLdsRows, lds0 + (buf ^ 1u) * BUFB);   // (128: every fill from the same 8 ranges - an L2-resident source, for the ingest-rate measurement)
        t1 = (dbg & 16) ? (uint32_t)__builtin_readcyclecounter() : 0u;
    };
    // end of an entry: wait for what was requested an entry ago, take the next entry's words, the cold remainder's step, the requests
    // for the entry after next, barrier
    uint32_t dnext = 0u;   // dense phase: the next entry's descriptor word, in flight
    auto entry_end = [&](uint32_t padaddr, bool dense_phase) {
        t2 = (dbg & 16) ? (uint32_t)__builtin_readcyclecounter() : 0u;
        wait_vm0();   // the range fetched at the top has landed (this wavefront's share), the metadata block of entry r + 1 and its words
        // (every word an ordinary load brought is READ here, straight behind our own wait and BEFORE anything new is requested:
        //  hipcc puts a vmcnt(0) in front of the first use of an ordinary load's result - at the top of the next entry, or behind
        //  the cold remainder's requests, it would wait for what was issued a moment ago)
        const bool more = r + 2 < nr;
        ew0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)einfo[0]);     // entry r + 1
        ew2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)einfo[1]);
        if (dense_phase) ew1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)dnext);
        if (ew0 & 0x40000000u) buf ^= 1u;                                   // (another range: it sits in the other buffer)
        if constexpr (CAN_COLD && LONG) { const bool turn = (r & 7) == cold_turn; if (have_g || (have_n && turn)) cold_step(turn); }
        else if constexpr (CAN_COLD) { if (have_g || have_n) cold_step(true); }
        if (more) {
            einfo = load_info(r + 2);
            if (dense_phase) dnext = load_desc(r + 2);
            if (!(dbg & 4)) meta_dma(r + 2, padaddr);       // into the pad this entry has just read
        }
        const uint32_t t3 = (dbg & 16) ? (uint32_t)__builtin_readcyclecounter() : 0u;
        if (!(dbg & 8)) __builtin_amdgcn_s_barrier();
        if (dbg & 16) { const uint32_t t4 = (uint32_t)__builtin_readcyclecounter(); ph[0] += t1 - t0; ph[1] += t2 - t1; ph[2] += t3 - t2; ph[3] += t4 - t3; }
    };
    for (; r < nr && !(ew0 >> 31); ++r) {   // ---- normal entries
        entry_top();
        const uint32_t padaddr = pad0 + (uint32_t)(r & 1) * PADB, bb = lanebase + buf * BUFB;
        if (!(dbg & 2)) {
            FlatMeta<T> m;
            flat_meta_block<T>(padaddr + idoff, padaddr + moff, m);
            // Two register sets: tile x+1's transposed reads are issued before tile x's are waited for (counted lgkmcnt), so a
            // wavefront's LDS round trip is covered by its own A-fragment arithmetic and MFMAs, not only by the three other
            // wavefronts of its SIMD (phase timers before: 260 cycles per tile step per wavefront of which ~150 waiting on LDS).
            // (four planes: a second set of 16 registers does not fit beside 64 accumulators under the 128 registers sixteen
            //  wavefronts per CU leave each - that pass waits for each tile's reads before the next are issued)
            constexpr bool PIPE = NT <= 3;
            constexpr int SETS = PIPE ? 2 : 1;
            // Windows are dealt to the least loaded wavefront, so a wavefront's empty slots are its LAST ones - on the Reddit shape (7.1
            // windows per wavefront) nine wavefronts in ten have seven windows.  The tiles of an empty last slot are skipped under ONE
            // wave-uniform test (no LDS reads, A fragment or MFMAs: those wavefronts then wait at the barrier for the full ones, but
            // leave them the SIMD's issue slots and the LDS pipe meanwhile).  (Two instantiations of the whole walk - for MAXW and
            // MAXW - 1 windows - made hipcc merge all 64 accumulators through copies and spill.)
            half4 lo[SETS][NT], hi[SETS][NT];
            if constexpr (PIPE) flat_issue<NT, PLANEB>(bb + (m.idw[0] & 0xffffu), bb + (m.idw[0] >> 16), lo[0], hi[0]);
#pragma unroll
            for (int x = 0; x < T; ++x) {
                if (x / TPC == MAXW - 1 && !last_valid) break;      // (the first comparison folds once unrolled; nothing is in flight here: lds_flat_step_if)
                // (priority falls as a wavefront advances through its windows: whoever is behind on the SIMD goes first)
                if (x % TPC == 0 && !(dbg & 32)) set_wave_priority(3 - (x / TPC) * 4 / MAXW);
                const int cs = PIPE ? (x & 1) : 0;
                if constexpr (!PIPE) { flat_issue<NT, PLANEB>(bb + (m.idw[x] & 0xffffu), bb + (m.idw[x] >> 16), lo[0], hi[0]); flat_drain<NT>(lo[0], hi[0]); }
                else if (x + 1 < T && (x + 1) / TPC == MAXW - 1 && x / TPC != MAXW - 1)   // the step in front of the last slot: its reads only if the slot holds a window
                    flat_step_if<NT, PLANEB>(last_on, bb + (m.idw[x + 1] & 0xffffu), bb + (m.idw[x + 1] >> 16), lo[(x + 1) & 1], hi[(x + 1) & 1], lo[cs], hi[cs]);
                else if (x + 1 < T) flat_step<NT, PLANEB>(bb + (m.idw[x + 1] & 0xffffu), bb + (m.idw[x + 1] >> 16), lo[(x + 1) & 1], hi[(x + 1) & 1], lo[cs], hi[cs]);
                else flat_drain<NT>(lo[cs], hi[cs]);
                half8 af;
                switch (x & 3) {   // (x is a compile-time constant once unrolled)
                    case 0: af = flat_afrag<0>(m.mk[x >> 2]); break;
                    case 1: af = flat_afrag<1>(m.mk[x >> 2]); break;
                    case 2: af = flat_afrag<2>(m.mk[x >> 2]); break;
                    default: af = flat_afrag<3>(m.mk[x >> 2]); break;
                }
#pragma unroll
                for (int s = 0; s < NT; ++s) {
                    const half8 bf = __builtin_shufflevector(lo[cs][s], hi[cs][s], 0, 1, 2, 3, 4, 5, 6, 7);
                    acc[x / TPC][s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf, acc[x / TPC][s], 0, 0, 0);
                }
            }
        }
        entry_end(padaddr, false);
    }
    if constexpr (DENSE) {
    // (the dense phase is marked UNLIKELY: hipcc then shapes the registers of the kernel around the normal loop and puts what the two
    //  loops disagree about into this one - the calibrated SBM graph, where 14 % of the entries are dense: 0.536 -> 0.522 ms)
    if (__builtin_expect(r < nr, 0)) {   // the descriptor words of the first two dense entries: fetched here, once (the normal phase reads none)
        const uint32_t d0 = load_desc(r), d1 = load_desc(r + 1 < nr ? r + 1 : r);
        wait_vm0();
        ew1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)d0);
        dnext = d1;
    }
    for (; __builtin_expect(r < nr, 0); ++r) {                   // ---- dense entries
        entry_top();
        const uint32_t padaddr = pad0 + (uint32_t)(r & 1) * PADB, bb = lanebase + buf * BUFB;
        if (!(dbg & 2)) {
            // ---- a dense entry: up to T ordinary-format tiles of this wavefront in the pad, ew1 = tiles per window slot (4 bits each)
            // (this lane's id word and mask byte inside a 128-byte tile, as spmm_lds_kernel; the lane id is re-derived - mbcnt - so that
            //  the two offsets are recomputed at their rare uses instead of living through the main loop)
            const uint32_t l2 = lane_id_now();
            const uint32_t gd = l2 >> 4, id_ = l2 & 15u;
            uint32_t idaddr = padaddr + (4u * gd + (id_ >> 2)) * 4u, maddr = padaddr + 64u + id_ * 4u + gd, idw, mb;
            lds_cell_ids(idaddr, maddr, idw, mb);
#pragma unroll
            for (int j = 0; j < MAXW; ++j) {
                const int nj = (int)((ew1 >> (4 * j)) & 15u);
                if (nj) {
                    floatx4 cacc[NT];
#pragma unroll
                    for (int s = 0; s < NT; ++s) cacc[s] = floatx4{0.f, 0.f, 0.f, 0.f};
                    for (int t = 0; t < nj; ++t) {
                        const uint32_t ad0 = bb + (idw & 0xffffu), ad1 = bb + (idw >> 16);
                        const half8 af = afrag_from_byte(mb);
                        half4 lo[NT], hi[NT];
                        uint32_t nidw, nmb;
                        lds_cell_block<NT, PLANEB>(ad0, ad1, idaddr, maddr, lo, hi, nidw, nmb);   // (+ the next tile's id word and mask byte: the pad has a tile's room behind its last one)
#pragma unroll
                        for (int s = 0; s < NT; ++s) {
                            const half8 bf = __builtin_shufflevector(lo[s], hi[s], 0, 1, 2, 3, 4, 5, 6, 7);
                            cacc[s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf, cacc[s], 0, 0, 0);
                        }
                        idw = nidw; mb = nmb;
                        idaddr += 128u; maddr += 128u;
                    }
#pragma unroll
                    for (int s = 0; s < NT; ++s) acc[j][s] += cacc[s];
                }
            }
        }
        entry_end(padaddr, true);
    }
    }
    if (!(dbg & 32)) __builtin_amdgcn_s_setprio(0);
    if constexpr (CAN_COLD) {   // what is left of the list (its last two tiles; all of it beyond the workgroup's ranges)
        if constexpr (LONG) {   // the tile still in flight in the pool first; then private tiles, in the range buffers (every wavefront is past the walk's last barrier: nobody reads or fills them any more)
            if (have_g) { wait_vm0(); cold_step(false); }
            cbuf = lds0 + (uint32_t)wave * (NT * 1024u);
        }
        while (have_g || have_n) { wait_vm0(); cold_step(true); }
    }
    if (dbg & 16) {   // measurement run: no results, the wavefronts of workgroup 0 report their phase totals
        if (wg == 0 && blockIdx.y == 0 && lane == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) a.y[wave * 8 + k] = (float)ph[k];
            a.y[wave * 8 + 7] = (float)(nr * T);
        }
        return;
    }

    const float inv1 = pow2f(-kx - 1);   // (the A fragment holds 2.0 per edge)
    int wj[MAXW];
#pragma unroll
    for (int j = 0; j < MAXW; ++j) wj[j] = __builtin_amdgcn_readfirstlane(a.order[cell_position(wg, wave, j, MAXW)]);
    if (a.w) {
        // f3: the dense update behind the aggregation (as in spmm_lds_kernel)
        __syncthreads();
        constexpr int DIN = NT * 16, LDP = DIN + 1;
        float* scratch = reinterpret_cast<float*>(smem) + wave * (16 * LDP);
        const int din = a.D - coloff < DIN ? a.D - coloff : DIN;
        const int tiles = (a.dout + 15) >> 4;
#pragma unroll
        for (int j = 0; j < MAXW; ++j) {
            if (wj[j] < 0) continue;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();   // (the previous slot's reads are done)
#pragma unroll
            for (int s = 0; s < NT; ++s)
#pragma unroll
                for (int ii = 0; ii < 4; ++ii) scratch[(4 * g + ii) * LDP + 16 * s + i] = acc[j][s][ii] * inv1;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();
            const int64_t row0 = (int64_t)wj[j] * kWinRows + 4 * g;
            for (int t = 0; t < tiles; ++t) {
                const floatx4 c = dense_update_tile(scratch, LDP, din, a.w, coloff, a.dout, t, g, i);
                const int colg = 16 * t + i;
                if (colg < a.dout) {
#pragma unroll
                    for (int ii = 0; ii < 4; ++ii) {
                        if (row0 + ii >= a.N) continue;
                        float* dst = a.y + (row0 + ii) * (int64_t)a.dout + colg;
                        if (a.accumulate) atomicAdd(dst, c[ii]);
                        else *dst = relu_if(a.relu, c[ii]);
                    }
                }
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < MAXW; ++j) {
        if (wj[j] < 0) continue;
        const int64_t row0 = (int64_t)wj[j] * kWinRows + 4 * g;
#pragma unroll
        for (int s = 0; s < NT; ++s) {
            const int colg = coloff + 16 * s + i;
            if (colg < a.D) {
#pragma unroll
                for (int ii = 0; ii < 4; ++ii)
                    if (row0 + ii < a.N) a.y[(row0 + ii) * a.D + colg] = TCGNN_KERNEL_STORE(a.relu, row0 + ii, colg, acc[j][s][ii] * inv1);
            }
        }
    }
}
