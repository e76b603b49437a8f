// tcgnn_pack.inc - plan-time kernels over the legacy metadata (fill, longest row, locality of the numbering, pack: the five legacy
// arrays -> the packed tile stream).  Included by tcgnn_device.hip.
// ------------------------------------------------------------------------------------------
// pack: legacy (nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow) -> tile stream
// ------------------------------------------------------------------------------------------
// Locality of the numbering: how many condensed columns lie within `reach` rows of their own window.  A uniform random graph gives
// 2 reach / num_cols (1/8 at reach = num_cols / 16), a graph whose communities are numbered consecutively nearly all of them.
// Decides between the per-window walk in XCD-contiguous order (co-resident workgroups share their gathered rows in L2) and the
// range-blocked walk (which picks its windows strided over the whole graph).
// grid-stride fill of an int32 array (padding column ids of re-condensed tile streams: the all-zero sentinel row)
__global__ __launch_bounds__(256) void fill_i32_kernel(int32_t* __restrict__ dst, int64_t n, int32_t v) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) dst[k] = v;
}

// longest row of the CSR (grid-stride; one atomic per workgroup)
__global__ __launch_bounds__(256) void max_degree_kernel(const int32_t* __restrict__ rowptr, int32_t N, uint32_t* out) {
    uint32_t m = 0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < N; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t d = rowptr[r + 1] - rowptr[r];
        m = max(m, d > 0 ? (uint32_t)d : 0u);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off));
    __shared__ uint32_t wm[4];
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) { m = max(max(wm[0], wm[1]), max(wm[2], wm[3])); if (m) atomicMax(out, m); }
}

__global__ __launch_bounds__(256) void locality_kernel(const int64_t* __restrict__ wb_ptr, const int32_t* __restrict__ cols, int32_t nw, int32_t Nc,
                                                       int32_t row_off, int32_t reach, unsigned long long* __restrict__ out) {
    const int w = blockIdx.x;
    if (w >= nw) return;
    const int64_t tb = wb_ptr[w] * kWbCols, n = (wb_ptr[w + 1] - wb_ptr[w]) * kWbCols;
    const int64_t centre = (int64_t)row_off + (int64_t)w * kWinRows + kWinRows / 2;
    unsigned near = 0, all = 0;
    for (int64_t q = threadIdx.x; q < n; q += blockDim.x) {
        const int32_t c = cols[tb + q];
        if (c >= Nc) continue;
        ++all;
        const int64_t d = (int64_t)c - centre;
        near += (d < 0 ? -d : d) <= reach;
    }
    for (int o = 32; o > 0; o >>= 1) { near += __shfl_down(near, o); all += __shfl_down(all, o); }
    if ((threadIdx.x & 63) == 0 && all) { atomicAdd(&out[0], (unsigned long long)near); atomicAdd(&out[1], (unsigned long long)all); }
}

__global__ __launch_bounds__(256) void pack_kernel(const int32_t* __restrict__ rowptr,
                                                   const int32_t* __restrict__ col,
                                                   const int32_t* __restrict__ e2c,
                                                   const int32_t* __restrict__ e2r,
                                                   const int64_t* __restrict__ wb_ptr, int32_t N,
                                                   int32_t Nc, int32_t* cols, uint32_t* mask,
                                                   int32_t* ebase, int32_t* flags) {
    const int w = blockIdx.x;
    const int64_t n0 = (int64_t)w * kWinRows;
    const int64_t n1 = n0 + kWinRows < N ? n0 + kWinRows : N;
    const int64_t base = wb_ptr[w];
    const int64_t nwb = wb_ptr[w + 1] - base;
    for (int64_t k = threadIdx.x; k < nwb * kWbCols; k += blockDim.x) cols[base * kWbCols + k] = Nc; // zero sentinel row
    for (int64_t k = threadIdx.x; k < nwb * kWinRows; k += blockDim.x) {
        mask[base * kWinRows + k] = 0u;
        ebase[base * kWinRows + k] = 0;
    }
    __syncthreads();
    if (n0 >= N) return;
    const int64_t e0 = rowptr[n0], e1 = rowptr[n1];
    for (int64_t e = e0 + threadIdx.x; e < e1; e += blockDim.x) {
        const int c = e2c[e];
        const int r = e2r[e] - (int)n0;
        const int v = col[e];
        if (c < 0 || (int64_t)c >= nwb * kWbCols || r < 0 || r >= kWinRows || v < 0 || v >= Nc) {
            flags[0] = 1;
            continue;
        }
        const int64_t tile = base + (c >> 5);
        cols[tile * kWbCols + (c & 31)] = v; // duplicates of a column write the same id
        atomicOr(&mask[tile * kWinRows + r], 1u << (c & 31));
        bool first_in_tile_row = true;
        if (e > e0 && e2r[e - 1] - (int)n0 == r) {
            const int cp = e2c[e - 1];
            if (cp >= c) flags[1] = 1; // row not strictly increasing: edge-offset table unusable
            first_in_tile_row = (cp >> 5) != (c >> 5);
        }
        if (first_in_tile_row) ebase[tile * kWinRows + r] = (int32_t)e;
    }
}
