// tcgnn_transpose.hip - the CSR of A^T on the GPU, and the permutation between A's and A^T's edge positions.
//
// The reference's layers back-propagate through A (gnn_conv.py:46,80,110,143): correct only on a symmetric graph.  The transposed
// product A^T X runs on the same plans and kernels as A X once A^T's CSR exists; this file builds it from A's CSR without leaving
// the device:
//   sort      rocPRIM radix_sort_pairs of (column id, CSR position), stable, over the bits of N - 1: entry eT of A^T is the
//             eT-th (column, position) pair in that order, so perm[eT] = its position in A and the rows of A^T come out sorted
//             (A's duplicate entries stay, next to each other)
//   rowptr_t  a lower-bound search of every c = 0 .. N in the sorted keys
//   col_t     the CSR row of every position (one wavefront per row) gathered through perm
//   check     nodePointer[0] = 0, monotone, nodePointer[N] = E, every id in [0, N), and whether (rowptr_t, col_t) = (rowptr, col)
//             - one pass, read back with ONE stream synchronisation
// The hand-written kernels are in tcgnn_transpose.inc (compiled into tcgnn_device.hip, where `make audit` sees them).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring> // rocprim/iterator/texture_cache_iterator.hpp calls memset unqualified

#include <rocprim/rocprim.hpp>

#include "tcgnn.h"
#include "tcgnn_internal.h"

using namespace tcgnn;

namespace {

// read-back words: nodePointer[0], nodePointer[N], a descending pair, an id outside [0, N), a difference from A
struct TransposeResult { uint32_t start, end, bad_ptr, bad_id, differs, pad[3]; };

// workspace layout (256-byte aligned parts): result words, sorted keys [E], row ids [E], rocPRIM scratch
struct TransposeLayout { size_t off_res, off_keys, off_rowid, off_tmp, tmp_bytes, total; };
inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }

// bits of the largest valid id, N - 1 (at least one: rocPRIM sorts a non-empty bit range)
unsigned id_bits(int32_t num_nodes) {
    unsigned b = 1;
    while (b < 32 && (1ull << b) < (unsigned long long)std::max(num_nodes, 1)) ++b;
    return b;
}

int transpose_layout(int32_t num_nodes, int64_t num_edges, TransposeLayout* L) {
    const size_t E = (size_t)num_edges;
    size_t tb = 0;
    if (E > 0) {   // (the size query takes the sort's own bit range)
        rocprim::counting_iterator<int32_t> vin(0);
        if (rocprim::radix_sort_pairs(nullptr, tb, (const uint32_t*)nullptr, (uint32_t*)nullptr, vin, (int32_t*)nullptr, (unsigned)E, 0u,
                                      id_bits(num_nodes), (hipStream_t)0) != hipSuccess) return 1;
    }
    size_t o = 0;
    L->off_res = o; o += up256(sizeof(TransposeResult));
    L->off_keys = o; o += up256(E * 4);
    L->off_rowid = o; o += up256(E * 4);
    L->tmp_bytes = up256(tb + 256);
    L->off_tmp = o; o += L->tmp_bytes;
    L->total = o;
    return 0;
}

} // namespace

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        const int e_ = (int)(expr);                                                         \
        if (e_ != (int)hipSuccess) return fail(e_ == (int)hipErrorOutOfMemory ? TCGNN_ERR_OOM : TCGNN_ERR_HIP, "%s -> %s", #expr, hipGetErrorString((hipError_t)e_)); \
    } while (0)

extern "C" int tcgnn_transpose_workspace_bytes(int32_t num_nodes, int64_t num_edges, size_t* bytes) {
    if (!bytes || num_nodes < 0 || num_edges < 0) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_transpose_workspace_bytes: null pointer or bad size");
    if (num_edges > 0x7fffffffLL) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_transpose: int32 CSR positions only (E = %lld)", (long long)num_edges);
    TransposeLayout L;
    if (transpose_layout(num_nodes, num_edges, &L)) return fail(TCGNN_ERR_HIP, "tcgnn_transpose_workspace_bytes: rocPRIM size query failed");
    *bytes = L.total;
    return TCGNN_OK;
}

extern "C" int tcgnn_transpose_ws(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges,
                                  int32_t* d_nodePointer_t, int32_t* d_edgeList_t, int32_t* d_perm, void* d_workspace, size_t workspace_bytes,
                                  int32_t* symmetric, void* stream_v) {
    if (!d_nodePointer || !d_nodePointer_t || num_nodes < 0 || num_edges < 0 || (num_edges > 0 && (!d_edgeList || !d_edgeList_t || !d_perm)))
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_transpose_ws: null array or bad size");
    if (num_edges > 0x7fffffffLL) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_transpose: int32 CSR positions only (E = %lld)", (long long)num_edges);
    TransposeLayout L;
    if (transpose_layout(num_nodes, num_edges, &L)) return fail(TCGNN_ERR_HIP, "tcgnn_transpose_ws: rocPRIM size query failed");
    if (!d_workspace || workspace_bytes < L.total || (reinterpret_cast<uintptr_t>(d_workspace) & 255))
        return fail(TCGNN_ERR_WORKSPACE, "tcgnn_transpose_ws: workspace needs %zu bytes 256-aligned (tcgnn_transpose_workspace_bytes), got %zu at %p",
                    L.total, workspace_bytes, d_workspace);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    char* const ws = static_cast<char*>(d_workspace);
    TransposeResult* const d_res = reinterpret_cast<TransposeResult*>(ws + L.off_res);
    uint32_t* const keys = reinterpret_cast<uint32_t*>(ws + L.off_keys);
    int32_t* const rowid = reinterpret_cast<int32_t*>(ws + L.off_rowid);
    const int64_t E = num_edges;

    HIP_TRY(hipMemsetAsync(d_res, 0, sizeof(TransposeResult), stream));
    if (E > 0) {
        // ids at or beyond N have bits above the sorted range: their order is wrong, but every write stays inside [0, E) and the
        // check below reports them
        rocprim::counting_iterator<int32_t> vin(0);
        size_t tb = L.tmp_bytes;
        HIP_TRY(rocprim::radix_sort_pairs(ws + L.off_tmp, tb, reinterpret_cast<const uint32_t*>(d_edgeList), keys, vin, d_perm, (unsigned)E, 0u,
                                          id_bits(num_nodes), stream));
        HIP_TRY(transpose_row_ids(d_nodePointer, num_nodes, E, rowid, stream));
        HIP_TRY(transpose_gather_rows(d_perm, rowid, E, d_edgeList_t, stream));
    }
    HIP_TRY(transpose_row_pointers(keys, E, num_nodes, d_nodePointer_t, stream));
    HIP_TRY(transpose_check(d_nodePointer, d_edgeList, d_nodePointer_t, d_edgeList_t, num_nodes, E, reinterpret_cast<uint32_t*>(d_res), stream));
    TransposeResult res;
    HIP_TRY(hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (res.start != 0) return fail(TCGNN_ERR_BAD_GRAPH, "tcgnn_transpose: nodePointer[0] = %d, expected 0", (int32_t)res.start);
    if ((int64_t)(int32_t)res.end != E)
        return fail(TCGNN_ERR_BAD_GRAPH, "tcgnn_transpose: nodePointer[num_nodes] = %d but edgeList holds %lld entries", (int32_t)res.end, (long long)E);
    if (res.bad_ptr) return fail(TCGNN_ERR_BAD_GRAPH, "tcgnn_transpose: nodePointer is not monotone");
    if (res.bad_id) return fail(TCGNN_ERR_BAD_GRAPH, "tcgnn_transpose: a column id lies outside [0, num_nodes = %d)", num_nodes);
    if (symmetric) *symmetric = res.differs ? 0 : 1;
    return TCGNN_OK;
}

extern "C" int tcgnn_permute_edge_values(const float* d_val, const int32_t* d_perm, int64_t num_edges, float* d_out, void* stream) {
    if (num_edges < 0 || (num_edges > 0 && (!d_val || !d_perm || !d_out)))
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_permute_edge_values: null array or bad size");
    HIP_TRY(permute_edge_values(d_val, d_perm, num_edges, d_out, stream));
    return TCGNN_OK;
}
