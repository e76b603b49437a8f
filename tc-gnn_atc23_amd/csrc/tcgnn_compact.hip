// tcgnn_compact.hip - entry points of the relabelled mini-batch blocks (include/tcgnn.h): the layer graphs of one mini-batch, which keep
// all N rows, become square CSRs over the M nodes they touch.  The relabelling is monotone, so rows keep their edges in their order and
// every operator of the library takes the result as it takes any square CSR.  One mini-batch is
//   begin   clear the validation word of the workspace
//   mark    once per layer graph: rows with edges and in-range columns into the caller's byte mask (no synchronisation)
//   count   new_id = the exclusive scan of the mask, and ONE stream synchronisation to read back M and the validation word
//   nodes   the kept ids, M entries (no synchronisation)
//   graph   once per layer graph: M + 1 row pointers and E relabelled columns (no synchronisation)
// on caller scratch; nothing here allocates.  The scan is the library's own for the reason tcgnn_sample.hip gives: the workspace size is
// answered without a device.  The kernels and their launch geometry are in tcgnn_compact.inc.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tcgnn.h"
#include "tcgnn_internal.h"

using namespace tcgnn;

#include "tcgnn_compact.inc"

namespace {

// read-back words: a mark call saw a bad id or pointer, M
struct CompactResult { uint32_t bad, total, pad[6]; };

// workspace layout (256-byte aligned parts): result words, one partial sum per block of mask entries
struct CompactLayout { size_t off_res, off_sums, total; };
inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }

CompactLayout compact_layout(int32_t num_nodes) {
    CompactLayout L;
    L.off_res = 0;
    L.off_sums = up256(sizeof(CompactResult));
    L.total = L.off_sums + up256((size_t)compact_scan_blocks(num_nodes) * 4);
    return L;
}

// the workspace's parts, or null when it is missing, short or misaligned
uint32_t* compact_res(void* d_workspace, size_t workspace_bytes, int32_t num_nodes, uint32_t** sums) {
    const CompactLayout L = compact_layout(num_nodes);
    if (!d_workspace || workspace_bytes < L.total || (reinterpret_cast<uintptr_t>(d_workspace) & 255)) return nullptr;
    char* const ws = static_cast<char*>(d_workspace);
    if (sums) *sums = reinterpret_cast<uint32_t*>(ws + L.off_sums);
    return reinterpret_cast<uint32_t*>(ws + L.off_res);
}

} // namespace

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        const int e_ = (int)(expr);                                                         \
        if (e_ != (int)hipSuccess) return fail(e_ == (int)hipErrorOutOfMemory ? TCGNN_ERR_OOM : TCGNN_ERR_HIP, "%s -> %s", #expr, hipGetErrorString((hipError_t)e_)); \
    } while (0)

#define WORKSPACE_TRY(res, name, num_nodes)                                                                                              \
    if (!(res))                                                                                                                          \
        return fail(TCGNN_ERR_WORKSPACE, name ": workspace needs %zu bytes 256-aligned (tcgnn_compact_workspace_bytes), got %zu at %p", \
                    compact_layout(num_nodes).total, workspace_bytes, d_workspace)

extern "C" int tcgnn_compact_workspace_bytes(int32_t num_nodes, size_t* bytes) {
    if (!bytes || num_nodes < 0) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_compact_workspace_bytes: null pointer or bad size");
    *bytes = compact_layout(num_nodes).total;
    return TCGNN_OK;
}

extern "C" int tcgnn_compact_begin(int32_t num_nodes, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (num_nodes < 0) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_compact_begin: bad size");
    uint32_t* const d_res = compact_res(d_workspace, workspace_bytes, num_nodes, nullptr);
    WORKSPACE_TRY(d_res, "tcgnn_compact_begin", num_nodes);
    HIP_TRY(hipMemsetAsync(d_res, 0, sizeof(CompactResult), static_cast<hipStream_t>(stream)));
    return TCGNN_OK;
}

extern "C" int tcgnn_compact_mark(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges, uint8_t* d_keep,
                                  void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!d_nodePointer || num_nodes < 0 || num_edges < 0 || (num_nodes > 0 && !d_keep) || (num_edges > 0 && !d_edgeList))
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_compact_mark: null pointer or bad size");
    if (num_edges > 0x7fffffffLL) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_compact_mark: int32 CSR positions only (E = %lld)", (long long)num_edges);
    uint32_t* const d_res = compact_res(d_workspace, workspace_bytes, num_nodes, nullptr);
    WORKSPACE_TRY(d_res, "tcgnn_compact_mark", num_nodes);
    HIP_TRY(compact_mark(d_nodePointer, d_edgeList, num_nodes, num_edges, d_keep, d_res, static_cast<hipStream_t>(stream)));
    return TCGNN_OK;
}

extern "C" int tcgnn_compact_count(const uint8_t* d_keep, int32_t num_nodes, int32_t* d_new_id, void* d_workspace, size_t workspace_bytes,
                                   int32_t* num_kept, void* stream_v) {
    if (!num_kept || num_nodes < 0 || (num_nodes > 0 && (!d_keep || !d_new_id)))
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_compact_count: null pointer or bad size");
    uint32_t* sums = nullptr;
    uint32_t* const d_res = compact_res(d_workspace, workspace_bytes, num_nodes, &sums);
    WORKSPACE_TRY(d_res, "tcgnn_compact_count", num_nodes);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    HIP_TRY(compact_count(d_keep, num_nodes, sums, d_res, d_new_id, stream));
    CompactResult res;
    HIP_TRY(hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemsetAsync(d_res, 0, sizeof(CompactResult), stream));   // (the next mini-batch's mark calls start from a clear word)
    HIP_TRY(hipStreamSynchronize(stream));
    if (res.bad)
        return fail(TCGNN_ERR_BAD_GRAPH, "tcgnn_compact_count: a marked graph has a column id outside [0, num_nodes) or malformed row pointers "
                                         "(nodePointer[0] = 0, monotone, nodePointer[num_nodes] = num_edges)");
    *num_kept = (int32_t)res.total;
    return TCGNN_OK;
}

extern "C" int tcgnn_compact_nodes(const int32_t* d_new_id, int32_t num_nodes, int32_t num_kept, int32_t* d_nodes, void* stream) {
    if (num_nodes < 0 || num_kept < 0 || num_kept > num_nodes || (num_nodes > 0 && !d_new_id) || (num_kept > 0 && !d_nodes))
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_compact_nodes: null pointer or bad size");
    HIP_TRY(compact_nodes(d_new_id, num_nodes, num_kept, d_nodes, static_cast<hipStream_t>(stream)));
    return TCGNN_OK;
}

extern "C" int tcgnn_compact_graph(const int32_t* d_nodePointer, const int32_t* d_edgeList, const int32_t* d_new_id, const int32_t* d_nodes,
                                   int32_t num_nodes, int32_t num_kept, int64_t num_edges, int32_t* d_nodePointer_b, int32_t* d_edgeList_b,
                                   void* stream) {
    if (!d_nodePointer || !d_nodePointer_b || num_nodes < 0 || num_kept < 0 || num_kept > num_nodes || num_edges < 0 ||
        (num_nodes > 0 && !d_new_id) || (num_kept > 0 && !d_nodes) || (num_edges > 0 && (!d_edgeList || !d_edgeList_b)))
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_compact_graph: null pointer or bad size");
    if (num_edges > 0x7fffffffLL) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_compact_graph: int32 CSR positions only (E = %lld)", (long long)num_edges);
    HIP_TRY(compact_graph(d_nodePointer, d_edgeList, d_new_id, d_nodes, num_nodes, num_kept, num_edges, d_nodePointer_b, d_edgeList_b,
                          static_cast<hipStream_t>(stream)));
    return TCGNN_OK;
}

// ---- row-list graphs: mark from lists of ids, and the block of a graph that has one row per listed id instead of num_nodes rows

extern "C" int tcgnn_compact_mark_ids(const int32_t* d_ids, int64_t count, int32_t num_nodes, uint8_t* d_keep, void* d_workspace,
                                      size_t workspace_bytes, void* stream) {
    if (count < 0 || num_nodes < 0 || (count > 0 && !d_ids) || (count > 0 && num_nodes > 0 && !d_keep))
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_compact_mark_ids: null pointer or bad size");
    uint32_t* const d_res = compact_res(d_workspace, workspace_bytes, num_nodes, nullptr);
    WORKSPACE_TRY(d_res, "tcgnn_compact_mark_ids", num_nodes);
    HIP_TRY(compact_mark_ids(d_ids, count, num_nodes, d_keep, d_res, static_cast<hipStream_t>(stream)));
    return TCGNN_OK;
}

extern "C" int tcgnn_compact_rows_graph(const int32_t* d_rows, int32_t num_rows, const int32_t* d_rowPointer_s, const int32_t* d_edgeList_s,
                                        int64_t num_sampled, const int32_t* d_new_id, int32_t num_nodes, int32_t num_kept,
                                        int32_t* d_nodePointer_b, int32_t* d_edgeList_b, void* stream) {
    if (!d_rowPointer_s || !d_nodePointer_b || num_rows < 0 || num_nodes < 0 || num_kept < 0 || num_kept > num_nodes || num_sampled < 0 ||
        (num_rows > 0 && !d_rows) || (num_nodes > 0 && !d_new_id) || (num_sampled > 0 && (!d_edgeList_s || !d_edgeList_b)))
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_compact_rows_graph: null pointer or bad size");
    if (num_sampled > 0x7fffffffLL)
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_compact_rows_graph: int32 CSR positions only (E' = %lld)", (long long)num_sampled);
    HIP_TRY(compact_rows_graph(d_rows, num_rows, d_rowPointer_s, d_edgeList_s, num_sampled, d_new_id, num_nodes, num_kept, d_nodePointer_b,
                               d_edgeList_b, static_cast<hipStream_t>(stream)));
    return TCGNN_OK;
}
