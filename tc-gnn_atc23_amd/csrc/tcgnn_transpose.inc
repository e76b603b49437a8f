// tcgnn_transpose.inc - the hand-written kernels of the device CSR transpose (tcgnn_transpose.hip holds the rocPRIM sort and the
// entry points).  Included by tcgnn_device.hip so that `make audit` lists them with every other kernel of the library.
//
// Every index these kernels derive from the caller's CSR is clamped to the arrays: the transpose validates the graph only behind its
// one read-back, and nothing may be read or written out of bounds before that.

namespace {

// rowid[e] = the CSR row of position e: one wavefront per row (row pointers beyond [0, E] are clamped; a non-monotone array leaves
// positions unwritten, which only changes values, never an address, and is reported behind the read-back)
__global__ __launch_bounds__(256) void transpose_row_id_kernel(const int32_t* __restrict__ rowptr, int32_t N, int64_t E, int32_t* __restrict__ rowid) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    int64_t lo = rowptr[row], hi = rowptr[row + 1];
    if (lo < 0) lo = 0;
    if (hi > E) hi = E;
    for (int64_t e = lo + (threadIdx.x & 63); e < hi; e += 64) rowid[e] = (int32_t)row;
}

// rowptr_t[c] = number of sorted keys below c (lower bound), c = 0 .. N: the row pointers of A^T.  A binary search per entry stays
// inside [0, E] whatever the keys hold.
__global__ __launch_bounds__(256) void transpose_row_pointer_kernel(const uint32_t* __restrict__ keys, int64_t E, int32_t N, int32_t* __restrict__ rowptr_t) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c > N) return;
    int64_t lo = 0, hi = E;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)keys[mid] < c) lo = mid + 1; else hi = mid;
    }
    rowptr_t[c] = (int32_t)lo;
}

// col_t[eT] = rowid[perm[eT]]: A^T's column ids are A's row ids in the sorted order
__global__ __launch_bounds__(256) void transpose_gather_rows_kernel(const int32_t* __restrict__ perm, const int32_t* __restrict__ rowid, int64_t E,
                                                                    int32_t* __restrict__ col_t) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E) return;
    uint32_t p = (uint32_t)perm[i];
    if (p >= (uint64_t)E) p = 0;
    col_t[i] = rowid[p];
}

// The validation words and the symmetry test in one grid-stride pass over max(N + 1, E) slots:
//   res[0], res[1] = nodePointer[0], nodePointer[N];  res[2] |= a descending pair of row pointers;  res[3] |= a column id outside
//   [0, N);  res[4] |= a difference between (rowptr_t, col_t) and (rowptr, col).  A thread ORs its slots' flags together and each
//   wavefront issues at most one atomic per word at the end: on a directed graph nearly every slot differs, and one atomic per
//   wavefront of slots on one word (1.8 M at Reddit size) serialised to ~20 ms
__global__ __launch_bounds__(256) void transpose_check_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                              const int32_t* __restrict__ rowptr_t, const int32_t* __restrict__ col_t,
                                                              int32_t N, int64_t E, int64_t slots, uint32_t* res) {
    bool bad_ptr = false, bad_id = false, diff = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < N) bad_ptr |= rowptr[i] > rowptr[i + 1];
        if (i <= N) diff |= rowptr_t[i] != rowptr[i];
        if (i < E) {
            const int32_t c = col[i];
            bad_id |= (uint32_t)c >= (uint32_t)N;
            diff |= col_t[i] != c;
        }
        if (i == 0) {
            res[0] = (uint32_t)rowptr[0];
            res[1] = (uint32_t)rowptr[N];
        }
    }
    const uint64_t mp = __ballot(bad_ptr), mi = __ballot(bad_id), md = __ballot(diff);
    if ((threadIdx.x & 63) == 0) {
        if (mp) atomicOr(&res[2], 1u);
        if (mi) atomicOr(&res[3], 1u);
        if (md) atomicOr(&res[4], 1u);
    }
}

// out[eT] = val[perm[eT]]: the edge values of A in A^T's order.  Bound by the scattered 4-byte reads of val (the writes and the
// perm reads are streamed); a perm entry outside [0, E) - not one tcgnn_transpose_ws wrote - reads val[0] instead of beyond the array
__global__ __launch_bounds__(256) void permute_values_kernel(const float* __restrict__ val, const int32_t* __restrict__ perm, int64_t E, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E) return;
    uint32_t p = (uint32_t)perm[i];
    if (p >= (uint64_t)E) p = 0;
    out[i] = val[p];
}

inline unsigned transpose_grid(int64_t n) { return (unsigned)((n + 255) / 256); }

} // namespace

namespace tcgnn {

int transpose_row_ids(const int32_t* rowptr, int32_t N, int64_t E, int32_t* rowid, void* stream) {
    if (N > 0 && E > 0)
        hipLaunchKernelGGL(transpose_row_id_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), rowptr, N, E, rowid);
    return (int)hipGetLastError();
}

int transpose_row_pointers(const uint32_t* sorted_keys, int64_t E, int32_t N, int32_t* rowptr_t, void* stream) {
    hipLaunchKernelGGL(transpose_row_pointer_kernel, dim3(transpose_grid((int64_t)N + 1)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       sorted_keys, E, N, rowptr_t);
    return (int)hipGetLastError();
}

int transpose_gather_rows(const int32_t* perm, const int32_t* rowid, int64_t E, int32_t* col_t, void* stream) {
    if (E > 0)
        hipLaunchKernelGGL(transpose_gather_rows_kernel, dim3(transpose_grid(E)), dim3(256), 0, static_cast<hipStream_t>(stream), perm, rowid, E, col_t);
    return (int)hipGetLastError();
}

int transpose_check(const int32_t* rowptr, const int32_t* col, const int32_t* rowptr_t, const int32_t* col_t, int32_t N, int64_t E,
                    uint32_t* res, void* stream) {
    const int64_t slots = std::max<int64_t>((int64_t)N + 1, E);
    // 2048 workgroups (8 per CU, 16 K atomics at most per word) stream the slots
    hipLaunchKernelGGL(transpose_check_kernel, dim3(std::min(transpose_grid(slots), 2048u)), dim3(256), 0, static_cast<hipStream_t>(stream), rowptr,
                       col, rowptr_t, col_t, N, E, slots, res);
    return (int)hipGetLastError();
}

int permute_edge_values(const float* val, const int32_t* perm, int64_t E, float* out, void* stream) {
    if (E > 0)
        hipLaunchKernelGGL(permute_values_kernel, dim3(transpose_grid(E)), dim3(256), 0, static_cast<hipStream_t>(stream), val, perm, E, out);
    return (int)hipGetLastError();
}

} // namespace tcgnn
