// tcgnn_subgraph.hip - entry points of subgraph sampling (include/tcgnn.h): a seeded random walk over a CSR, and the node-induced
// subgraph of a CSR over a node list - what GraphSAINT's and Cluster-GCN's mini-batches are made of.  The induced subgraph is a square
// CSR over its M nodes in which every row is used, so one block serves every layer of a model.
//   random_walk    one launch: no workspace, no synchronisation, no report
//   induce_count   the count of every listed row, their saturating scan into nodePointer_b - four launches of fixed order that also
//                  validate the listed rows - and ONE stream synchronisation to read back E_b and the validation words
//   induce         the same walk over the listed rows, writing edgeList_b and eid - no allocation, no synchronisation
// on caller scratch; nothing here allocates.  The scan is the library's own for the reason tcgnn_sample.hip gives: the workspace size is
// answered without a device.  The kernels and their launch geometry are in tcgnn_subgraph.inc.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tcgnn.h"
#include "tcgnn_internal.h"

using namespace tcgnn;

#include "tcgnn_subgraph.inc"

namespace {

// read-back words: a listed id out of range, a listed pointer out of range, a descending listed pair, a column of a listed row out of
// range, E_b (saturating)
struct InduceResult { uint32_t bad_id, bad_ptr, descending, bad_col, total, pad[3]; };

// workspace layout (256-byte aligned parts): result words, one partial sum per block of list slots
struct InduceLayout { size_t off_res, off_sums, total; };
inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }

InduceLayout induce_layout(int32_t num_kept) {
    InduceLayout L;
    L.off_res = 0;
    L.off_sums = up256(sizeof(InduceResult));
    L.total = L.off_sums + up256((size_t)induce_scan_blocks(num_kept) * 4);
    return L;
}

} // namespace

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        const int e_ = (int)(expr);                                                         \
        if (e_ != (int)hipSuccess) return fail(e_ == (int)hipErrorOutOfMemory ? TCGNN_ERR_OOM : TCGNN_ERR_HIP, "%s -> %s", #expr, hipGetErrorString((hipError_t)e_)); \
    } while (0)

extern "C" int tcgnn_random_walk(const int32_t* d_nodePointer, const int32_t* d_edgeList, const int32_t* d_starts, int32_t num_walks,
                                 int32_t num_nodes, int64_t num_edges, int32_t length, uint64_t seed, int32_t* d_walks, void* stream) {
    if (!d_nodePointer || num_walks < 0 || num_nodes < 0 || num_edges < 0 || length < 0 || (num_walks > 0 && (!d_starts || !d_walks)) ||
        (num_edges > 0 && !d_edgeList))
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_random_walk: null pointer or bad size");
    if (num_edges > 0x7fffffffLL) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_random_walk: int32 CSR positions only (E = %lld)", (long long)num_edges);
    if ((int64_t)num_walks * ((int64_t)length + 1) > 0x7fffffffLL)
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_random_walk: %d walks of %d steps hold more than 2^31 - 1 entries", num_walks, length);
    if (num_walks == 0) return TCGNN_OK;   // (nothing to write)
    HIP_TRY(random_walk(d_nodePointer, d_edgeList, d_starts, num_walks, num_nodes, num_edges, length, seed, d_walks, static_cast<hipStream_t>(stream)));
    return TCGNN_OK;
}

extern "C" int tcgnn_induce_workspace_bytes(int32_t num_kept, size_t* bytes) {
    if (!bytes || num_kept < 0) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_induce_workspace_bytes: null pointer or bad size");
    *bytes = induce_layout(num_kept).total;
    return TCGNN_OK;
}

extern "C" int tcgnn_induce_count(const int32_t* d_nodePointer, const int32_t* d_edgeList, const int32_t* d_nodes, const int32_t* d_new_id,
                                  int32_t num_kept, int32_t num_nodes, int64_t num_edges, int32_t* d_nodePointer_b, void* d_workspace,
                                  size_t workspace_bytes, int64_t* num_induced, void* stream_v) {
    if (!d_nodePointer || !d_nodePointer_b || !num_induced || num_kept < 0 || num_nodes < 0 || num_edges < 0 || num_kept > num_nodes ||
        (num_kept > 0 && !d_nodes) || (num_nodes > 0 && !d_new_id) || (num_edges > 0 && !d_edgeList))
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_induce_count: null pointer or bad size");
    if (num_edges > 0x7fffffffLL) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_induce_count: int32 CSR positions only (E = %lld)", (long long)num_edges);
    const InduceLayout L = induce_layout(num_kept);
    if (!d_workspace || workspace_bytes < L.total || (reinterpret_cast<uintptr_t>(d_workspace) & 255))
        return fail(TCGNN_ERR_WORKSPACE, "tcgnn_induce_count: workspace needs %zu bytes 256-aligned (tcgnn_induce_workspace_bytes), got %zu at %p",
                    L.total, workspace_bytes, d_workspace);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (num_kept == 0) {   // a graph of no nodes: its one row pointer, no launch
        HIP_TRY(hipMemsetAsync(d_nodePointer_b, 0, sizeof(int32_t), stream));
        *num_induced = 0;
        return TCGNN_OK;
    }
    char* const ws = static_cast<char*>(d_workspace);
    uint32_t* const d_res = reinterpret_cast<uint32_t*>(ws + L.off_res);
    uint32_t* const sums = reinterpret_cast<uint32_t*>(ws + L.off_sums);

    HIP_TRY(hipMemsetAsync(d_res, 0, sizeof(InduceResult), stream));
    HIP_TRY(induce_count(d_nodePointer, d_edgeList, d_nodes, d_new_id, num_kept, num_nodes, num_edges, sums, d_res, d_nodePointer_b, stream));
    InduceResult res;
    HIP_TRY(hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (res.bad_id) return fail(TCGNN_ERR_BAD_GRAPH, "tcgnn_induce_count: a listed node id lies outside [0, %d)", num_nodes);
    if (res.bad_ptr) return fail(TCGNN_ERR_BAD_GRAPH, "tcgnn_induce_count: nodePointer of a listed row lies outside [0, %lld]", (long long)num_edges);
    if (res.descending) return fail(TCGNN_ERR_BAD_GRAPH, "tcgnn_induce_count: nodePointer descends at a listed row");
    if (res.bad_col) return fail(TCGNN_ERR_BAD_GRAPH, "tcgnn_induce_count: a listed row holds a column id outside [0, %d)", num_nodes);
    if (res.total > 0x7fffffffu)
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_induce_count: the listed rows keep more than 2^31 - 1 edges (int32 positions only)");
    *num_induced = (int64_t)res.total;
    return TCGNN_OK;
}

extern "C" int tcgnn_induce(const int32_t* d_nodePointer, const int32_t* d_edgeList, const int32_t* d_nodes, const int32_t* d_new_id,
                            const int32_t* d_nodePointer_b, int32_t num_kept, int32_t num_nodes, int64_t num_edges, int64_t num_induced,
                            int32_t* d_edgeList_b, int32_t* d_eid, void* stream) {
    if (!d_nodePointer || !d_nodePointer_b || num_kept < 0 || num_nodes < 0 || num_edges < 0 || num_induced < 0 || num_kept > num_nodes ||
        (num_kept > 0 && !d_nodes) || (num_nodes > 0 && !d_new_id) || (num_edges > 0 && !d_edgeList) ||
        (num_induced > 0 && (!d_edgeList_b || !d_eid)))
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_induce: null pointer or bad size");
    if (num_edges > 0x7fffffffLL) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_induce: int32 CSR positions only (E = %lld)", (long long)num_edges);
    if (num_induced > 0x7fffffffLL)
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_induce: int32 CSR positions only (E_b = %lld)", (long long)num_induced);
    if (num_kept == 0 || num_induced == 0 || num_edges == 0) return TCGNN_OK;   // (nothing is kept: nothing is written)
    HIP_TRY(induce_write(d_nodePointer, d_edgeList, d_nodes, d_new_id, num_kept, num_nodes, num_edges, num_induced,
                         const_cast<int32_t*>(d_nodePointer_b), d_edgeList_b, d_eid, static_cast<hipStream_t>(stream)));
    return TCGNN_OK;
}
