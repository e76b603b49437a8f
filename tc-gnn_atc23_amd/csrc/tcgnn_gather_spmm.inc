// tcgnn_gather_spmm.inc - the gather walks of the SpMM (TileWalker, spmm_kernel, spmm_blocked_kernel): binary and edge-valued A.
// Included by tcgnn_device.hip.
// ------------------------------------------------------------------------------------------
// SpMM:  Y[window] = A_tile-stream * X16
// ------------------------------------------------------------------------------------------
struct SpmmArgs {
    const int64_t* wb_ptr;
    const int32_t* order;
    const int32_t* cols;
    const uint32_t* mask;
    const int32_t* ebase;
    const _Float16* x16;
    const float* edge_val;
    const uint32_t* hdr;
    float* y;
    int32_t N, D, stride, chunk0;
    int64_t E;
    int32_t xrows;   // rows of X16 including the zero sentinel row
    int32_t relu;    // fused epilogue: Y = max(A X, 0) (binary SpMM only)
    int32_t ldy;     // row stride of Y in floats (== D unless this call is one column block of a wider matrix)
    int32_t big;     // the fp16 image is 4 GB or more: gathers use 64-bit lane addresses (a buffer descriptor's index * stride wraps at 2^32)
    const float* w;  // f3: dense update fused behind the aggregation, Y[N, dout] = (A X) W with W [D, dout] fp32 row-major (nullptr: Y = A X)
    int32_t dout;
    int32_t accumulate;   // Y += A X: the cold remainder of a plan whose dense part the LDS-resident kernel has already stored
    int32_t unguarded;    // the image was staged by the CALLER (tcgnn_spmm_staged): its header carries no range words - never "wide", bytes 4 .. 255 are not read
};

// ---- f3: the dense update in the aggregation kernel's epilogue (gnn_conv.py:92-97: X' = TCGNN.forward(X); X' = mm(X', W)).
// A window's aggregated rows Acc[16][din] (fp32, true scale) sit in LDS scratch `acc_lds` (row-major, leading dimension ldp, odd:
// conflict-free column reads); one wavefront multiplies them by the W columns of output tile t on the fp32 matrix pipe
// (v_mfma_f32_16x16x4_f32: exact fp32 fma chain, the precision of the torch.mm it replaces) and returns C[row 4g+ii][col 16t+i].
// W (<= 128 x 128 floats) is read through the caches: every window re-reads the same 64 KB at most.
__device__ __forceinline__ floatx4 dense_update_tile(const float* acc_lds, int ldp, int din, const float* __restrict__ w, int k0, int dout,
                                                     int t, int g, int i) {
    floatx4 c = {0.f, 0.f, 0.f, 0.f};
    const int n = 16 * t + i;
    for (int kk = 0; kk < din; kk += 4) {
        const int k = kk + g;
        const float av = k < din ? acc_lds[i * ldp + k] : 0.0f;
        const float bv = (k < din && n < dout) ? w[(int64_t)(k0 + k) * dout + n] : 0.0f;
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, c, 0, 0, 0);
    }
    return c;
}

// ---- memory pipeline discipline -----------------------------------------------------------------
// With an LDS-DMA in flight hipcc waits vmcnt(0) at the first use of ANY ordinary load result and
// before any LDS read it can see (cdna_hip_programming.md 5, trap (b)) - that drained the next
// tile's gather in the first version of these kernels.  Hiding loads in inline asm avoids the
// drain, but a VGPR with an asm load in flight is a trap of its own: the register allocator may
// copy it before our wait (found by tools/audit_hidden_loads.py: `v_mov_b32 v2, v3` scheduled
// above the s_waitcnt).  So the rule here is: NO VGPR EVER HAS A LOAD IN FLIGHT OUTSIDE ONE ASM
// STATEMENT.
//   * global -> LDS: LDS-DMA builtins only (per-tile metadata, gathered rows, edge values, SDDMM
//     operands).  No VGPR destination; in flight across loop iterations; retired by wait_vm0().
//   * LDS -> VGPR: the generated blocks of tcgnn_lds_blocks.inc, whose s_waitcnt lgkmcnt(0) is in
//     the same asm statement as the reads (early-clobber outputs).
typedef uint32_t uintx4 __attribute__((ext_vector_type(4)));
#include "tcgnn_lds_blocks.inc"

__device__ __forceinline__ void wait_vm0() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// LDS store issued from asm (no destination register, so nothing can be in flight into a VGPR);
// LDS operations of one wavefront execute in order, a later block read sees the data.
// (mask & a) | (~mask & b) in one instruction (hipcc otherwise spends a compare and a select on the loop-invariant b)
__device__ __forceinline__ uint32_t bitfield_select(uint32_t mask, uint32_t a, uint32_t b) {
    uint32_t r;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(mask), "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ void lds_write_b32(uint32_t lds_byte_addr, float v) {
    asm volatile("ds_write_b32 %0, %1" ::"v"(lds_byte_addr), "v"(v) : "memory");
}

template <int N> __device__ __forceinline__ void lds_ids_block(const uint32_t* ad, uint32_t* v, uint32_t qaddr, uintx4& q) {
    if constexpr (N == 1) lds_ids_block1(ad, v, qaddr, q);
    else if constexpr (N == 2) lds_ids_block2(ad, v, qaddr, q);
    else if constexpr (N == 3) lds_ids_block3(ad, v, qaddr, q);
    else if constexpr (N == 4) lds_ids_block4(ad, v, qaddr, q);
    else if constexpr (N == 5) lds_ids_block5(ad, v, qaddr, q);
    else if constexpr (N == 6) lds_ids_block6(ad, v, qaddr, q);
    else if constexpr (N == 7) lds_ids_block7(ad, v, qaddr, q);
    else if constexpr (N == 8) lds_ids_block8(ad, v, qaddr, q);
    else if constexpr (N == 9) lds_ids_block9(ad, v, qaddr, q);
    else lds_ids_block10(ad, v, qaddr, q);
}
template <int N, int OFF> __device__ __forceinline__ void lds_q_block(const uint32_t* ad, uintx4* q) {
    if constexpr (N == 1) lds_q_block1<OFF>(ad, q);
    else if constexpr (N == 2) lds_q_block2<OFF>(ad, q);
    else if constexpr (N == 3) lds_q_block3<OFF>(ad, q);
    else if constexpr (N == 4) lds_q_block4<OFF>(ad, q);
    else if constexpr (N == 5) lds_q_block5<OFF>(ad, q);
    else if constexpr (N == 6) lds_q_block6<OFF>(ad, q);
    else if constexpr (N == 7) lds_q_block7<OFF>(ad, q);
    else if constexpr (N == 8) lds_q_block8<OFF>(ad, q);
    else if constexpr (N == 9) lds_q_block9<OFF>(ad, q);
    else lds_q_block10<OFF>(ad, q);
}
template <int K, int OFF> __device__ __forceinline__ void lds_tr_block(const uint32_t (*ad)[2], half4* lo, half4* hi) {
    if constexpr (K == 1) lds_tr_block1<OFF>(ad, lo, hi);
    else if constexpr (K == 2) lds_tr_block2<OFF>(ad, lo, hi);
    else if constexpr (K == 3) lds_tr_block3<OFF>(ad, lo, hi);
    else if constexpr (K == 4) lds_tr_block4<OFF>(ad, lo, hi);
    else { lds_tr_block4<OFF>(ad, lo, hi); lds_tr_block<K - 4, OFF>(ad + 4, lo + 4, hi + 4); }
}

// 256-entry table: byte of adjacency bits -> the eight fp16 {0,1} values of a binary A fragment.
// One LDS read replaces ~28 VALU instructions per tile.
__device__ __forceinline__ void fill_afrag_table(char* tab) {
    for (int e = threadIdx.x; e < 256; e += blockDim.x) {
        half8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = ((e >> j) & 1) ? (_Float16)1.0f : (_Float16)0.0f;
        *reinterpret_cast<half8*>(tab + e * 16) = v;
    }
}

// Per-tile metadata travels as ONE 256-byte DMA: lane l < 32 fetches cols[t][l], lanes 32..47
// mask[t][l-32], lanes 48..63 ebase[t][l-48]; it lands lane-linear in a per-wavefront pad.
#ifndef TCGNN_NT_STORES
#define TCGNN_NT_STORES 0   // 1: the fused AGNN kernel's score / slice-addend stores are non-temporal (A/B experiments)
#endif
template <typename T> __device__ __forceinline__ void st_stream(T* p, T v) {
#if TCGNN_NT_STORES
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}
#ifndef TCGNN_META_AUX
#define TCGNN_META_AUX 0   // cache policy of the metadata stream (bit 1 = nt): A/B experiments
#endif
struct MetaSource {
    const char* base;   // this lane's element of tile 0
    int shift;          // log2(bytes per tile) of the array this lane reads
    __device__ __forceinline__ MetaSource(const int32_t* cols, const uint32_t* mask, const int32_t* ebase, int lane) {
        if (lane < 32) { base = reinterpret_cast<const char*>(cols + lane); shift = 7; }
        else if (lane < 48) { base = reinterpret_cast<const char*>(mask + (lane - 32)); shift = 6; }
        else { base = reinterpret_cast<const char*>(ebase + (lane - 48)); shift = 6; }
    }
    __device__ __forceinline__ void dma(int64_t t, uint32_t pad_lds) const {
        const char* src = base + (t << shift);
        __builtin_amdgcn_global_load_lds((GLB_AS const void*)src, (LDS_AS void*)(uintptr_t)pad_lds, 4, 0, TCGNN_META_AUX);
    }
};
static constexpr int kPadBytes = 256;

// eight 4-byte LDS reads at per-lane addresses, retired before anything else is issued (agnn_kernel backward: the saved scores of
// this lane's eight tile columns; TileWalker: its edge values - picked out of the lane's run by address instead of by a cascade of selects)
__device__ __forceinline__ void lds_read8_b32(const uint32_t (&ad)[8], uint32_t (&v)[8]) {
    asm volatile("ds_read_b32 %0, %8\n\t"
                 "ds_read_b32 %1, %9\n\t"
                 "ds_read_b32 %2, %10\n\t"
                 "ds_read_b32 %3, %11\n\t"
                 "ds_read_b32 %4, %12\n\t"
                 "ds_read_b32 %5, %13\n\t"
                 "ds_read_b32 %6, %14\n\t"
                 "ds_read_b32 %7, %15\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7])
                 : "v"(ad[0]), "v"(ad[1]), "v"(ad[2]), "v"(ad[3]), "v"(ad[4]), "v"(ad[5]), "v"(ad[6]), "v"(ad[7])
                 : "memory");
}

// Per-lane constants and the software-pipelined walk over a run of wide blocks, shared by the
// per-window kernel (run = every WAVES-th tile of one window) and the range-blocked kernel
// (run = the tiles of one window inside one column range).
// NBUF = 2: tile t+1 is gathered into the other buffer while tile t is multiplied.  NBUF = 1 (r06, the slice-synchronised walk beyond 64
// columns): ONE buffer per wavefront - the B fragments of tile t are read into registers, then the gather of t+1 is issued into the same
// buffer and flies under the MFMAs.  Half the LDS per wavefront: twelve wavefronts per CU instead of eight where the tile is 8 KB, and
// what a CU has in flight is what this walk is bound by (PMC: wavefronts parked on the gather 64 % of their cycles at 74 % L2 hits).
// LDS of one TileWalker wavefront: tile buffer(s), metadata pad, edge values (2 x 4 per lane), and with ONE buffer the run list of walk_list
static constexpr int kTileMaxRuns = 128;
static constexpr int tile_wave_lds(int nt, bool val, int nbuf) { return nbuf * nt * 1024 + kPadBytes + (val ? 2048 : 0) + (nbuf == 1 ? kTileMaxRuns * 16 : 0); }
template <int NT, bool VAL, int NBUF = 2>
struct TileWalker {
    static constexpr int TILE_BYTES = NT * 1024;
    static constexpr int kMaxRuns = kTileMaxRuns;
    static constexpr int WAVE_LDS = tile_wave_lds(NT, VAL, NBUF);
    static constexpr int NIDS = NT + 1 + (VAL ? 1 : 0);
    using Img = TileImage<NT>;
    const SpmmArgs& a;
    __amdgpu_buffer_rsrc_t xrsrc; // X16 as a structured buffer: record = one fp16 row (pitch bytes);
                                  // the gather address row*pitch + offset is formed by the hardware
    MetaSource meta;
    uint32_t ring, pad, vpad, atab, runs; // LDS byte addresses: tile buffers, metadata pad, edge-value pad, A table, run list (NBUF = 1)
    int lane, g, i;
    uint32_t doff[NT];            // byte offset inside a gathered row: first feature column of the pass + 16-byte piece
    uint32_t idaddr[NIDS];        // LDS addresses in the pad: row id of DMA k for this lane, mask word, edge offset
    uint32_t raddr[NT][2];        // LDS address (buffer 0) this lane hands ds_read_b64_tr_b16 for slice s, K half h
    float sa;                     // edge-value scale (VAL)

    __device__ __forceinline__ TileWalker(const SpmmArgs& args, char* wave_lds, char* atab_ptr, int coloff, float sa_)
        : a(args), meta(args.cols, args.mask, args.ebase, threadIdx.x & 63), sa(sa_) {
        lane = threadIdx.x & 63;
        g = lane >> 4;
        i = lane & 15;
        xrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a.x16, (short)(a.stride * 2), a.xrows, 0x00020000);
        ring = (uint32_t)(uintptr_t)((LDS_AS char*)wave_lds);
        pad = ring + NBUF * TILE_BYTES;
        vpad = pad + kPadBytes;
        runs = vpad + (VAL ? 2048u : 0u);
        atab = (uint32_t)(uintptr_t)((LDS_AS char*)atab_ptr);
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            int row, c;
            Img::unslot(k * 64 + lane, row, c);
            idaddr[k] = pad + (uint32_t)row * 4u;
            doff[k] = (uint32_t)(coloff * 2 + c * 16);
        }
        idaddr[NT] = pad + 128u + (uint32_t)i * 4u;
        if constexpr (VAL) idaddr[NT + 1] = pad + 192u + (uint32_t)i * 4u;
        // lane (g, i) receives K = 8g + 4h + {0..3} of column 16s + i when it points the transpose
        // read at row 8g + 4h + (i >> 2), halves 16s + 4(i & 3) .. +3
        const int rrow = 8 * g + (i >> 2);
#pragma unroll
        for (int s = 0; s < NT; ++s) {
            const int c = 2 * s + ((i >> 1) & 1);
            raddr[s][0] = ring + (uint32_t)(Img::slot(rrow, c) * 16 + (i & 1) * 8);
            raddr[s][1] = ring + (uint32_t)(Img::slot(rrow + 4, c) * 16 + (i & 1) * 8);
        }
    }

    struct Cur {            // the tile being multiplied: its mask word, edge offset, value-window shift; wide: eight values fetched
        uint32_t m, eb;
        int shift;
        bool wide;
    };
    template <int BUF> __device__ __forceinline__ void dma_gather(const uint32_t* cid) const {
        if (a.big) {   // (wave-uniform: a kernel argument)
            const char* const xb = reinterpret_cast<const char*>(a.x16);
            const uint64_t pitchb = (uint64_t)a.stride * 2u;
#pragma unroll
            for (int k = 0; k < NT; ++k)
                __builtin_amdgcn_global_load_lds((GLB_AS const void*)(xb + (uint64_t)cid[k] * pitchb + doff[k]),
                                                 (LDS_AS void*)(uintptr_t)(ring + BUF * TILE_BYTES + k * 1024), 16, 0, 0);
            return;
        }
#pragma unroll
        for (int k = 0; k < NT; ++k)
            __builtin_amdgcn_struct_ptr_buffer_load_lds(xrsrc, (LDS_AS void*)(uintptr_t)(ring + BUF * TILE_BYTES + k * 1024), 16,
                                                        (int)cid[k], (int)doff[k], 0, 0, 0);
    }
    // edge values of this lane's byte of row i: consecutive floats starting at the first edge of the byte (a row's edges inside
    // eight columns are one run of the CSR), clamped so the read stays inside edge_val; they land in this lane's slot of the value
    // pad.  Four cover the run almost always; when some lane's run is longer (hub rows: every second column is an edge) a second
    // DMA fetches the next four - wave-uniform, decided from the mask.
    __device__ __forceinline__ void dma_vals(Cur& c) const {
        const int64_t e0 = (int64_t)c.eb + __popc(c.m & ((1u << (8 * g)) - 1u));
        int64_t lo = e0 < a.E - 8 ? e0 : a.E - 8;
        if (lo < 0) lo = 0;
        c.shift = (int)(e0 - lo);
        c.wide = a.E >= 8 && __any(__popc((c.m >> (8 * g)) & 0xffu) + c.shift > 4);
        __builtin_amdgcn_global_load_lds((GLB_AS const void*)(a.edge_val + lo), (LDS_AS void*)(uintptr_t)vpad, 16, 0, 0);
        if (c.wide) __builtin_amdgcn_global_load_lds((GLB_AS const void*)(a.edge_val + lo + 4), (LDS_AS void*)(uintptr_t)(vpad + 1024u), 16, 0, 0);
    }

    __device__ __forceinline__ half8 a_fragment(const Cur& cur, const uintx4& q, const uint32_t (&sv)[8]) const {
        half8 af;
        if constexpr (VAL) {
            const uint32_t mb = (cur.m >> (8 * g)) & 0xffu;
            const int nb = __popc(mb);
            if (!cur.wide && __builtin_expect(__any(nb + cur.shift > 4), 0)) {
                // (fewer than eight edges in the whole matrix) ordinary loads; the compiler drains the DMA queue for them
                const int64_t e0 = (int64_t)cur.eb + __popc(cur.m & ((1u << (8 * g)) - 1u));
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const bool on = (mb >> j) & 1u;
                    const float v = on ? a.edge_val[e0 + __popc(mb & ((1u << j) - 1u))] * sa : 0.0f;
                    af[j] = to_half_rna(v);
                }
            } else {
                // sv[j]: the value of tile column j of my eight, read from the fetched run BY ADDRESS in stage() (r03: the cascade of
                // selects over the fetched registers cost ~10 VALU instructions per column of a loop that is VALU-bound)
#pragma unroll
                for (int j = 0; j < 8; ++j) af[j] = ((mb >> j) & 1u) ? to_half_rna(__uint_as_float(sv[j]) * sa) : (_Float16)0.0f;
            }
        } else {
            af = __builtin_bit_cast(half8, q);   // table entry of this lane's adjacency byte
        }
        return af;
    }
    template <int BUF> __device__ __forceinline__ void multiply(const Cur& cur, const uintx4& q, const uint32_t (&sv)[8], floatx4 (&acc)[NT]) const {
        const half8 af = a_fragment(cur, q, sv);
        half4 lo[NT], hi[NT];
        lds_tr_block<NT, BUF * TILE_BYTES>(raddr, lo, hi);
        mfma_tile(af, lo, hi, acc);
    }
    __device__ __forceinline__ void mfma_tile(const half8& af, const half4 (&lo)[NT], const half4 (&hi)[NT], floatx4 (&acc)[NT]) const {
#pragma unroll
        for (int s = 0; s < NT; ++s) {
            const half8 bf = __builtin_shufflevector(lo[s], hi[s], 0, 1, 2, 3, 4, 5, 6, 7);
            acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf, acc[s], 0, 0, 0);
        }
    }

    // One pipeline stage, tile t in tile buffer BUF.  On entry the DMA queue holds gather(t),
    // [edge values(t)] and the metadata of the next tile; after ONE wait everything is read from LDS
    // (ids of the next tile + A fragment or edge values of this one), the next gather, the next edge
    // values and the metadata of the tile after that are issued, and tile t is multiplied underneath.
    // Returns false when t was the last tile of the run.
    template <int BUF>
    __device__ __forceinline__ bool stage(int64_t& t, int64_t& tn, const int64_t te, const int64_t step, const int64_t t_after,
                                          Cur& cur, floatx4 (&acc)[NT]) const {
        wait_vm0();
        uint32_t v[NIDS];
        uintx4 q;
        const uint32_t qaddr = VAL ? vpad + (uint32_t)lane * 16u : atab + (((cur.m >> (8 * g)) & 0xffu) << 4);
        lds_ids_block<NIDS>(idaddr, v, qaddr, q);
        [[maybe_unused]] uint32_t sv[8];
        if constexpr (VAL) {   // (before the next tile's values overwrite the pad)
            const uint32_t mb = (cur.m >> (8 * g)) & 0xffu, vbase = vpad + (uint32_t)lane * 16u;
            uint32_t va = vbase + ((uint32_t)cur.shift << 2), ad[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                ad[j] = va;
                va -= (uint32_t)((int32_t)(mb << (31 - j)) >> 31) << 2;                 // + 4 where the edge exists
            }
            if (cur.wide) {   // (wave-uniform: some lane's run crosses into the second block of four)
#pragma unroll
                for (int j = 0; j < 8; ++j) ad[j] += (((ad[j] - vbase) >> 4) & 1u) * 1008u;
            }
            lds_read8_b32(ad, sv);
        }
        const bool more = tn < te;
        Cur nx;
        nx.m = v[NT];
        nx.eb = VAL ? v[NT + (VAL ? 1 : 0)] : 0u;
        nx.shift = 0;
        nx.wide = false;
        const int64_t tnn = tn + step;
        [[maybe_unused]] half4 lo[NT], hi[NT];
        if constexpr (NBUF == 1) lds_tr_block<NT, 0>(raddr, lo, hi);   // (its lgkmcnt(0) is inside the block: the buffer is free behind it)
        if (more) {
            dma_gather<NBUF == 1 ? 0 : (BUF ^ 1)>(v);
            if constexpr (VAL) dma_vals(nx);
            const int64_t tf = tnn < te ? tnn : t_after;   // metadata two tiles ahead; at the end of the run: the caller's next run
            if (tf >= 0) meta.dma(tf, pad);
        }
        if constexpr (NBUF == 1) mfma_tile(a_fragment(cur, q, sv), lo, hi, acc);
        else multiply<BUF>(cur, q, sv, acc);
        cur = nx;
        t = tn;
        tn = tnn;
        return more;
    }

    // acc += A(tiles t, t+step, ... < te) * X16 rows.  `pad_tile` is the tile whose metadata the pad
    // holds (or has in flight) on entry, and on return; passing the caller's next run's first tile as
    // t_after lets the last stage prefetch it.
    __device__ __forceinline__ void walk(int64_t t, const int64_t te, const int64_t step, floatx4 (&acc)[NT], int64_t& pad_tile,
                                         const int64_t t_after) const {
        if (t >= te) return;
        if (pad_tile != t) meta.dma(t, pad);
        wait_vm0();
        uint32_t v[NIDS];
        uintx4 q;
        lds_ids_block<NIDS>(idaddr, v, atab, q);   // (the 16-byte read is a dummy here)
        Cur cur;
        cur.m = v[NT];
        cur.eb = VAL ? v[NT + (VAL ? 1 : 0)] : 0u;
        cur.shift = 0;
        cur.wide = false;
        dma_gather<0>(v);
        if constexpr (VAL) dma_vals(cur);
        int64_t tn = t + step;
        const int64_t tf = tn < te ? tn : t_after;
        if (tf >= 0) meta.dma(tf, pad);
        for (;;) {   // ping-pong over the two tile buffers: static LDS offsets, no register rotation
            if (!stage<0>(t, tn, te, step, t_after, cur, acc)) break;
            if constexpr (NBUF == 2) { if (!stage<1>(t, tn, te, step, t_after, cur, acc)) break; }
        }
        pad_tile = t_after;
    }

    // ---- r06: ONE pipeline over a LIST of runs (NBUF = 1; the slice-synchronised walk).  walk() above ends every run with nothing in
    // flight and starts the next one behind two round trips (metadata, first gather) - and on the products shape a (window, phase) run
    // is ~4.6 tiles, so a quarter of a wavefront's time was run starts.  Here the wavefront's runs - (first tile, length, window slot)
    // records it wrote to its own LDS - are walked as one tile sequence: the gather of the next tile and the metadata of the one after
    // are issued whether or not they belong to the same run; only the accumulator set changes at a boundary.  Three cursors (multiply,
    // gather, metadata) step through the list; a record is read from LDS by the metadata cursor only, inside one asm statement.
    struct RunCursor { int k, n, j; int64_t t, te; };
    __device__ __forceinline__ void run_put(int k, int64_t t, uint32_t len, int j) const {   // (before the pipeline starts: nothing in flight)
        const uintx4 w = {(uint32_t)(uint64_t)t, (uint32_t)((uint64_t)t >> 32), len, (uint32_t)j};
        asm volatile("ds_write_b128 %0, %1" ::"v"(runs + 16u * (uint32_t)k), "v"(w) : "memory");
    }
    __device__ __forceinline__ void cursor_load(RunCursor& c) const {
        if (c.k >= c.n) return;
        uintx4 w;
        asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(w) : "v"(runs + 16u * (uint32_t)c.k) : "memory");
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)w[0]), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)w[1]);
        c.t = (int64_t)(((uint64_t)hi << 32) | lo);
        c.te = c.t + (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)w[2]);
        c.j = __builtin_amdgcn_readfirstlane((int)w[3]);
    }
    __device__ __forceinline__ void cursor_next(RunCursor& c) const { if (++c.t == c.te) { ++c.k; cursor_load(c); } }

    template <int MAXW>
    __device__ __forceinline__ void walk_list(const int nruns, floatx4 (&acc)[MAXW][NT]) const {
        static_assert(NBUF == 1, "walk_list: single-buffer walker only");
        if (nruns <= 0) return;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (the list's stores have landed)
        RunCursor ca{0, nruns, 0, 0, 0};
        cursor_load(ca);
        RunCursor cb = ca;
        cursor_next(cb);
        RunCursor cm = cb;
        if (cm.k < cm.n) cursor_next(cm);
        meta.dma(ca.t, pad);
        wait_vm0();
        uint32_t v[NIDS];
        uintx4 q;
        lds_ids_block<NIDS>(idaddr, v, atab, q);   // (the 16-byte read is a dummy here)
        Cur cur;
        cur.m = v[NT];
        cur.eb = VAL ? v[NT + (VAL ? 1 : 0)] : 0u;
        cur.shift = 0;
        cur.wide = false;
        dma_gather<0>(v);
        if constexpr (VAL) dma_vals(cur);
        if (cb.k < cb.n) meta.dma(cb.t, pad);
        for (;;) {
            wait_vm0();
            const uint32_t qaddr = VAL ? vpad + (uint32_t)lane * 16u : atab + (((cur.m >> (8 * g)) & 0xffu) << 4);
            lds_ids_block<NIDS>(idaddr, v, qaddr, q);      // ids + mask of the NEXT tile of the list (stale words when there is none), A fragment / values of this one
            [[maybe_unused]] uint32_t sv[8];
            if constexpr (VAL) {
                const uint32_t mb = (cur.m >> (8 * g)) & 0xffu, vbase = vpad + (uint32_t)lane * 16u;
                uint32_t va = vbase + ((uint32_t)cur.shift << 2), ad[8];
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) {
                    ad[jj] = va;
                    va -= (uint32_t)((int32_t)(mb << (31 - jj)) >> 31) << 2;
                }
                if (cur.wide) {
#pragma unroll
                    for (int jj = 0; jj < 8; ++jj) ad[jj] += (((ad[jj] - vbase) >> 4) & 1u) * 1008u;
                }
                lds_read8_b32(ad, sv);
            }
            Cur nx;
            nx.m = v[NT];
            nx.eb = VAL ? v[NT + (VAL ? 1 : 0)] : 0u;
            nx.shift = 0;
            nx.wide = false;
            half4 lo[NT], hi[NT];
            lds_tr_block<NT, 0>(raddr, lo, hi);            // (its lgkmcnt(0) is inside the block: the buffer is free behind it)
            const bool more = cb.k < cb.n;
            if (more) {
                dma_gather<0>(v);
                if constexpr (VAL) dma_vals(nx);
                if (cm.k < cm.n) meta.dma(cm.t, pad);
            }
            const half8 af = a_fragment(cur, q, sv);
#pragma unroll
            for (int jj = 0; jj < MAXW; ++jj)
                if (ca.j == jj) {   // (wave-uniform: the accumulator set of the run this tile belongs to)
                    asm volatile("" ::: "memory");   // a REAL branch: if-converted, every set would be multiplied into a copy and selected - 32 more registers per set
                    mfma_tile(af, lo, hi, acc[jj]);
                }
            if (!more) break;
            cur = nx;
            ca = cb;
            cb = cm;
            if (cm.k < cm.n) cursor_next(cm);
        }
    }
};

// (second launch-bound argument = waves per SIMD: keeps the register budget at 128 / 256 so the
// accumulators are allocated as VGPRs - with the default budget hipcc split them into AGPRs and
// spent 24 v_accvgpr_* moves per tile shuffling them)
// spmm_kernel's launch geometry: one workgroup of `waves` wavefronts per window; behind the wavefronts' LDS the 4 KB A table
static constexpr LaunchGeom spmm_geom(int nt, int waves, bool val) { return {waves * 64, waves * tile_wave_lds(nt, val, 2) + 4096, nt <= 4 ? 4 : 2, 0}; }
// EPI: tcgnn_spmm_scaled's row scale / bias in the final store - kernels of their own (spmm_epi_kernel), so that the plain ones
// keep their code and registers
template <int NT, int WAVES, bool VAL, bool EPI>
__device__ __forceinline__ void spmm_body(const SpmmArgs& a, const Epi& epi) {
    if (!a.unguarded && (VAL ? range_is_wide_val(a.hdr) : range_is_wide(a.hdr, 0))) return;   // (range guard: the fp32 fallback launched behind this kernel does the work)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, i = lane & 15;
    const int w = a.order[blockIdx.x];
    const int coloff = (a.chunk0 + (int)blockIdx.y) * kMaxChunkDims; // first feature column of this pass
    const int64_t tb = a.wb_ptr[w], te = a.wb_ptr[w + 1];
    if (a.accumulate && !a.relu && !EPI && tb == te) return;   // nothing to add to what the LDS-resident kernel stored
    const int kx = scale_exp_from_bits(a.hdr[kHdrMaxX]);
    const int ka = VAL ? scale_exp_from_bits(a.hdr[kHdrMaxVal]) : 0;

    floatx4 acc[NT];
#pragma unroll
    for (int s = 0; s < NT; ++s) acc[s] = floatx4{0.f, 0.f, 0.f, 0.f};
    {
        using TW = TileWalker<NT, VAL>;
        char* atab = smem + WAVES * TW::WAVE_LDS;
        fill_afrag_table(atab);
        __syncthreads();
        const TW tw(a, smem + wave * TW::WAVE_LDS, atab, coloff, pow2f(ka));
        int64_t pad_tile = -1;
        tw.walk(tb + wave, te, WAVES, acc, pad_tile, -1);
    }

    // ---- combine the wavefronts' partial sums in a fixed order and store
    const float inv1 = pow2f(-kx), inv2 = VAL ? pow2f(-ka) : 1.0f; // |kx + ka| may exceed 126: two factors
    const int64_t row0 = (int64_t)w * kWinRows + 4 * g;
    if constexpr (!VAL) {
        if (a.w) {   // f3: Y[window] = (A X)[window] W   (one pass: the launcher only takes this path for D <= 128)
            const int din = NT * 16;                               // (padding columns of X16 are zero)
            const int ldp = din + 1;
            float* accT = reinterpret_cast<float*>(smem) + (WAVES > 1 ? WAVES * NT * 256 : 0);   // behind the reduction buffer
            __syncthreads(); // every wave is done with its ring
            if constexpr (WAVES > 1) {
                floatx4* red = reinterpret_cast<floatx4*>(smem);
#pragma unroll
                for (int s = 0; s < NT; ++s) red[(wave * NT + s) * 64 + lane] = acc[s];
                __syncthreads();
                for (int s = wave; s < NT; s += WAVES) {
                    floatx4 v = red[s * 64 + lane];
#pragma unroll
                    for (int ww = 1; ww < WAVES; ++ww) {
                        const floatx4 o = red[(ww * NT + s) * 64 + lane];
                        v[0] += o[0]; v[1] += o[1]; v[2] += o[2]; v[3] += o[3];
                    }
#pragma unroll
                    for (int ii = 0; ii < 4; ++ii) accT[(4 * g + ii) * ldp + 16 * s + i] = v[ii] * inv1;
                }
            } else {
#pragma unroll
                for (int s = 0; s < NT; ++s)
#pragma unroll
                    for (int ii = 0; ii < 4; ++ii) accT[(4 * g + ii) * ldp + 16 * s + i] = acc[s][ii] * inv1;
            }
            __syncthreads();
            const int tiles = (a.dout + 15) >> 4;
            for (int t = wave; t < tiles; t += WAVES) {
                const floatx4 c = dense_update_tile(accT, ldp, a.D < din ? a.D : din, a.w, 0, a.dout, t, g, i);
                const int colg = 16 * t + i;
                if (colg < a.dout) {
#pragma unroll
                    for (int ii = 0; ii < 4; ++ii)
                        if (row0 + ii < a.N) a.y[(row0 + ii) * a.ldy + colg] = relu_if(a.relu, c[ii]);
                }
            }
            return;
        }
    }
    if constexpr (WAVES > 1) {
        __syncthreads(); // every wave is done with its ring
        floatx4* red = reinterpret_cast<floatx4*>(smem);
#pragma unroll
        for (int s = 0; s < NT; ++s) red[(wave * NT + s) * 64 + lane] = acc[s];
        __syncthreads();
        for (int s = wave; s < NT; s += WAVES) {
            floatx4 v = red[s * 64 + lane];
#pragma unroll
            for (int ww = 1; ww < WAVES; ++ww) {
                const floatx4 o = red[(ww * NT + s) * 64 + lane];
                v[0] += o[0]; v[1] += o[1]; v[2] += o[2]; v[3] += o[3];
            }
            const int colg = coloff + 16 * s + i;
            if (colg < a.D) {
#pragma unroll
                for (int ii = 0; ii < 4; ++ii)
                    if (row0 + ii < a.N) {
                        float* dst = a.y + (row0 + ii) * a.ldy + colg;
                        *dst = EPI ? epi_apply(a.relu, epi, row0 + ii, colg, v[ii] * inv1 * inv2 + (a.accumulate ? *dst : 0.0f))
                                    : relu_if(a.relu, v[ii] * inv1 * inv2 + (a.accumulate ? *dst : 0.0f));
                    }
            }
        }
    } else {
#pragma unroll
        for (int s = 0; s < NT; ++s) {
            const int colg = coloff + 16 * s + i;
            if (colg < a.D) {
#pragma unroll
                for (int ii = 0; ii < 4; ++ii)
                    if (row0 + ii < a.N) {
                        float* dst = a.y + (row0 + ii) * a.ldy + colg;
                        *dst = EPI ? epi_apply(a.relu, epi, row0 + ii, colg, acc[s][ii] * inv1 * inv2 + (a.accumulate ? *dst : 0.0f))
                                    : relu_if(a.relu, acc[s][ii] * inv1 * inv2 + (a.accumulate ? *dst : 0.0f));
                    }
            }
        }
    }
}
template <int NT, int WAVES, bool VAL>
__global__ __launch_bounds__(spmm_geom(NT, WAVES, VAL).threads, spmm_geom(NT, WAVES, VAL).waves_per_simd) void spmm_kernel(const SpmmArgs a) { spmm_body<NT, WAVES, VAL, false>(a, Epi{nullptr, nullptr}); }
struct SpmmEpiArgs { SpmmArgs a; Epi epi; };
template <int NT, int WAVES>
__global__ __launch_bounds__(spmm_geom(NT, WAVES, false).threads, spmm_geom(NT, WAVES, false).waves_per_simd) void spmm_epi_kernel(const SpmmEpiArgs e) { spmm_body<NT, WAVES, false, true>(e.a, e.epi); }

template <int WAVES, bool VAL>
static hipError_t launch_spmm_waves(int nt, const SpmmArgs& args, int nwin, int nchunks, hipStream_t stream, const Epi& epi) {
    const dim3 grid((unsigned)nwin, (unsigned)nchunks);
    return with_width<8>(nt, [&](auto NT) {
        constexpr LaunchGeom g = spmm_geom(NT, WAVES, VAL);
        if constexpr (VAL) return launch_kernel<spmm_kernel<NT, WAVES, true>>(grid, g, stream, args);
        else return launch_plain_or_twin<spmm_kernel<NT, WAVES, false>, spmm_epi_kernel<NT, WAVES>>(grid, g, stream, args, epi);
    });
}
static hipError_t launch_spmm_any(bool val, int waves, int nt, const SpmmArgs& args, int nwin, int nchunks, hipStream_t stream,
                                  const Epi& epi = Epi{nullptr, nullptr}) {
    if (waves == 4) return val ? launch_spmm_waves<4, true>(nt, args, nwin, nchunks, stream, epi) : launch_spmm_waves<4, false>(nt, args, nwin, nchunks, stream, epi);
    return val ? launch_spmm_waves<1, true>(nt, args, nwin, nchunks, stream, epi) : launch_spmm_waves<1, false>(nt, args, nwin, nchunks, stream, epi);
}

// ------------------------------------------------------------------------------------------
// Range-blocked SpMM for graphs whose fp16 feature image does not fit the 4 MB per-XCD L2.
//
// PMC on the plain kernel (profiles/r01): 34 % L2 hit rate, 10 GB of fabric reads per launch for
// 0.58 GB of algorithmic bytes - every window sweeps all of X16, and X16 (29.8 MB at Reddit D=64)
// only fits the Infinity Cache, whose random-row gather rate (8.3 TB/s, tools/gather_bench) is
// less than half the L2's (18 TB/s).  Here the columns are cut into R ranges of ~2 MB of X16.
// A wavefront owns up to MAXW windows for its whole life and keeps their accumulators in
// registers; it walks range 0 of all its windows, then range 1, ...  All resident wavefronts
// start together and advance at the same average pace, so the rows being gathered at any moment
// belong to one or two ranges and stay L2-resident on every XCD.  No partial sums leave the
// registers, no atomics: the result is as deterministic as the plain kernel's.
// ------------------------------------------------------------------------------------------
struct SpmmBlockedArgs {
    SpmmArgs base;
    const uint32_t* bptr;
    int32_t nbuckets, gsel, nranges, nw, ngroups;
};

__global__ void bucket_ptr_kernel(const int64_t* __restrict__ wb_ptr, const int32_t* __restrict__ cols, int32_t nw,
                                  int32_t nbuckets, int32_t bucket_rows, uint32_t* bptr) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)nw * (nbuckets + 1)) return;
    const int w = (int)(idx / (nbuckets + 1)), k = (int)(idx % (nbuckets + 1));
    const int64_t tb = wb_ptr[w];
    const int64_t n = wb_ptr[w + 1] - tb;
    int64_t lo = 0, hi = n;
    if (k == nbuckets) lo = n;
    else
        while (lo < hi) {  // tiles are ordered by column: first tile whose first column is in bucket >= k
            const int64_t mid = (lo + hi) >> 1;
            if (cols[(tb + mid) * kWbCols] / bucket_rows >= k) hi = mid; else lo = mid + 1;
        }
    bptr[idx] = (uint32_t)lo;
}

// spmm_blocked_kernel's launch geometry: four persistent wavefronts, each owning maxw windows (accumulators: maxw * nt * 4 registers)
static constexpr LaunchGeom blocked_geom(int nt, bool val) { return {256, 4 * tile_wave_lds(nt, val, 2) + 4096, nt <= 4 ? 4 : 2, (nt <= 4 && !val) ? 4 : 2}; }
// (pinned: resident workgroups per CU at 1 .. 8 tiles of width)
static_assert(widths_give([](int nt) { return blocked_geom(nt, false).wgs_per_cu(); }, {4, 4, 4, 4, 2, 2, 2, 2}), "spmm_blocked_kernel, binary A");
static_assert(widths_give([](int nt) { return blocked_geom(nt, true).wgs_per_cu(); }, {4, 4, 4, 3, 2, 2, 2, 2}), "spmm_blocked_kernel, edge values");
#define TCGNN_KERNEL_NAME spmm_blocked_kernel
#define TCGNN_KERNEL_PARAM const SpmmBlockedArgs b
#define TCGNN_KERNEL_PROLOGUE
#define TCGNN_KERNEL_STORE(relu, row, col, v) relu_if(relu, v)
#include "tcgnn_blocked_kernel.inc"
#undef TCGNN_KERNEL_NAME
#undef TCGNN_KERNEL_PARAM
#undef TCGNN_KERNEL_PROLOGUE
#undef TCGNN_KERNEL_STORE
// tcgnn_spmm_scaled on this walk (binary A only: VAL = false)
struct SpmmBlockedEpiArgs { SpmmBlockedArgs b; Epi epi; };
#define TCGNN_KERNEL_NAME spmm_blocked_epi_kernel
#define TCGNN_KERNEL_PARAM const SpmmBlockedEpiArgs e
#define TCGNN_KERNEL_PROLOGUE const SpmmBlockedArgs& b = e.b;
#define TCGNN_KERNEL_STORE(relu, row, col, v) epi_apply(relu, e.epi, row, col, v)
#include "tcgnn_blocked_kernel.inc"
#undef TCGNN_KERNEL_NAME
#undef TCGNN_KERNEL_PARAM
#undef TCGNN_KERNEL_PROLOGUE
#undef TCGNN_KERNEL_STORE

template <int NT, bool VAL>
static hipError_t launch_blocked_one(const SpmmBlockedArgs& args, int nwg, int nchunks, hipStream_t stream, const Epi& epi) {
    constexpr LaunchGeom g = blocked_geom(NT, VAL);
    const dim3 grid((unsigned)nwg, (unsigned)nchunks);
    if constexpr (VAL) return launch_kernel<spmm_blocked_kernel<NT, g.maxw, true>>(grid, g, stream, args);
    else return launch_plain_or_twin<spmm_blocked_kernel<NT, g.maxw, false>, spmm_blocked_epi_kernel<NT, g.maxw, false>>(grid, g, stream, args, epi);
}
static hipError_t launch_blocked_any(bool val, int nt, const SpmmBlockedArgs& args, int nwg, int nchunks, hipStream_t stream, const Epi& epi) {
    return with_width<8>(nt, [&](auto NT) {
        return val ? launch_blocked_one<NT, true>(args, nwg, nchunks, stream, epi) : launch_blocked_one<NT, false>(args, nwg, nchunks, stream, epi);
    });
}
