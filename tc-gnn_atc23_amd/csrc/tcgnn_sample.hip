// tcgnn_sample.hip - entry points of the seeded neighbour sampler (include/tcgnn.h): the sampled graph keeps the node set and at most
// `fanout` in-edges per row.  Two calls, so that the caller allocates the outputs at their exact size in between:
//   count   the exclusive sum of min(degree, fanout) * mask into nodePointer_s - three launches of fixed order that also validate
//           nodePointer - and ONE stream synchronisation to read back E' and the validation words.  The scan is the library's own, not
//           rocPRIM's: rocPRIM's scratch-size query needs a device, and tcgnn_sample_workspace_bytes answers without one;
//   select  sample_select_kernel: which edges stay, written in CSR order - no allocation, no synchronisation.
// The hand-written kernels are in tcgnn_sample.inc (compiled into tcgnn_device.hip, where `make audit` sees them).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tcgnn.h"
#include "tcgnn_internal.h"

using namespace tcgnn;

namespace {

// read-back words: nodePointer[0], nodePointer[N], a descending pair, E'
struct SampleResult { uint32_t start, end, bad_ptr, total, pad[4]; };

// workspace layout (256-byte aligned parts): result words, one partial sum per block of rows
struct SampleLayout { size_t off_res, off_sums, total; };
inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }

SampleLayout sample_layout(int32_t num_nodes) {
    SampleLayout L;
    L.off_res = 0;
    L.off_sums = up256(sizeof(SampleResult));
    L.total = L.off_sums + up256((size_t)sample_scan_blocks(num_nodes) * 4);
    return L;
}

} // namespace

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        const int e_ = (int)(expr);                                                         \
        if (e_ != (int)hipSuccess) return fail(e_ == (int)hipErrorOutOfMemory ? TCGNN_ERR_OOM : TCGNN_ERR_HIP, "%s -> %s", #expr, hipGetErrorString((hipError_t)e_)); \
    } while (0)

extern "C" int tcgnn_sample_workspace_bytes(int32_t num_nodes, size_t* bytes) {
    if (!bytes || num_nodes < 0) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_sample_workspace_bytes: null pointer or bad size");
    *bytes = sample_layout(num_nodes).total;
    return TCGNN_OK;
}

extern "C" int tcgnn_sample_neighbors_count(const int32_t* d_nodePointer, const uint8_t* d_row_mask, int32_t num_nodes, int64_t num_edges,
                                            int32_t fanout, int32_t* d_nodePointer_s, void* d_workspace, size_t workspace_bytes,
                                            int64_t* num_sampled, void* stream_v) {
    if (!d_nodePointer || !d_nodePointer_s || !num_sampled || num_nodes < 0 || num_edges < 0)
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_sample_neighbors_count: null pointer or bad size");
    if (fanout < 0) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_sample_neighbors_count: fanout = %d is negative", fanout);
    if (num_edges > 0x7fffffffLL) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_sample_neighbors: int32 CSR positions only (E = %lld)", (long long)num_edges);
    const SampleLayout L = sample_layout(num_nodes);
    if (!d_workspace || workspace_bytes < L.total || (reinterpret_cast<uintptr_t>(d_workspace) & 255))
        return fail(TCGNN_ERR_WORKSPACE, "tcgnn_sample_neighbors_count: workspace needs %zu bytes 256-aligned (tcgnn_sample_workspace_bytes), got %zu at %p",
                    L.total, workspace_bytes, d_workspace);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    char* const ws = static_cast<char*>(d_workspace);
    uint32_t* const d_res = reinterpret_cast<uint32_t*>(ws + L.off_res);
    uint32_t* const sums = reinterpret_cast<uint32_t*>(ws + L.off_sums);

    HIP_TRY(hipMemsetAsync(d_res, 0, sizeof(SampleResult), stream));
    HIP_TRY(sample_count(d_nodePointer, d_row_mask, num_nodes, num_edges, fanout, sums, d_res, d_nodePointer_s, stream));
    SampleResult res;
    HIP_TRY(hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (res.start != 0) return fail(TCGNN_ERR_BAD_GRAPH, "tcgnn_sample_neighbors_count: nodePointer[0] = %d, expected 0", (int32_t)res.start);
    if ((int64_t)(int32_t)res.end != num_edges)
        return fail(TCGNN_ERR_BAD_GRAPH, "tcgnn_sample_neighbors_count: nodePointer[num_nodes] = %d but edgeList holds %lld entries", (int32_t)res.end,
                    (long long)num_edges);
    if (res.bad_ptr) return fail(TCGNN_ERR_BAD_GRAPH, "tcgnn_sample_neighbors_count: nodePointer is not monotone");
    *num_sampled = (int64_t)res.total;
    return TCGNN_OK;
}

extern "C" int tcgnn_sample_neighbors(const int32_t* d_nodePointer, const int32_t* d_edgeList, const uint8_t* d_row_mask,
                                      const int32_t* d_nodePointer_s, int32_t num_nodes, int64_t num_edges, int32_t fanout, uint64_t seed,
                                      int32_t* d_edgeList_s, int32_t* d_eid, void* stream) {
    if (!d_nodePointer || !d_nodePointer_s || num_nodes < 0 || num_edges < 0)
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_sample_neighbors: null pointer or bad size");
    if (fanout < 0) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_sample_neighbors: fanout = %d is negative", fanout);
    if (num_edges > 0x7fffffffLL) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_sample_neighbors: int32 CSR positions only (E = %lld)", (long long)num_edges);
    if (num_edges > 0 && fanout > 0 && (!d_edgeList || !d_edgeList_s || !d_eid))   // (nothing is kept otherwise: nothing is written)
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_sample_neighbors: null edge array");
    HIP_TRY(sample_select(d_nodePointer, d_edgeList, d_row_mask, d_nodePointer_s, num_nodes, num_edges, fanout, seed, d_edgeList_s, d_eid, stream));
    return TCGNN_OK;
}

// ---- seed-list sampling: the same two calls over a list of row ids.  The scan covers the list's num_rows + 1 slots and the select
// launches one workgroup per four slots, so a mini-batch costs its frontier and not num_nodes.

namespace {

// read-back words of the rows count: a listed id out of range, a listed pointer out of range, a descending listed pair, E' (saturating)
struct SampleRowsResult { uint32_t bad_id, bad_ptr, descending, total, pad[4]; };

SampleLayout sample_rows_layout(int32_t num_rows) {
    SampleLayout L;
    L.off_res = 0;
    L.off_sums = up256(sizeof(SampleRowsResult));
    L.total = L.off_sums + up256((size_t)sample_rows_scan_blocks(num_rows) * 4);
    return L;
}

} // namespace

extern "C" int tcgnn_sample_rows_workspace_bytes(int32_t num_rows, size_t* bytes) {
    if (!bytes || num_rows < 0) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_sample_rows_workspace_bytes: null pointer or bad size");
    *bytes = sample_rows_layout(num_rows).total;
    return TCGNN_OK;
}

extern "C" int tcgnn_sample_rows_count(const int32_t* d_nodePointer, const int32_t* d_rows, int32_t num_rows, int32_t num_nodes, int64_t num_edges,
                                       int32_t fanout, int32_t* d_rowPointer_s, void* d_workspace, size_t workspace_bytes, int64_t* num_sampled,
                                       void* stream_v) {
    if (!d_nodePointer || !d_rowPointer_s || !num_sampled || num_rows < 0 || num_nodes < 0 || num_edges < 0 || (num_rows > 0 && !d_rows))
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_sample_rows_count: null pointer or bad size");
    if (fanout < 0) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_sample_rows_count: fanout = %d is negative", fanout);
    if (num_edges > 0x7fffffffLL) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_sample_rows_count: int32 CSR positions only (E = %lld)", (long long)num_edges);
    const SampleLayout L = sample_rows_layout(num_rows);
    if (!d_workspace || workspace_bytes < L.total || (reinterpret_cast<uintptr_t>(d_workspace) & 255))
        return fail(TCGNN_ERR_WORKSPACE, "tcgnn_sample_rows_count: workspace needs %zu bytes 256-aligned (tcgnn_sample_rows_workspace_bytes), got %zu at %p",
                    L.total, workspace_bytes, d_workspace);
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    char* const ws = static_cast<char*>(d_workspace);
    uint32_t* const d_res = reinterpret_cast<uint32_t*>(ws + L.off_res);
    uint32_t* const sums = reinterpret_cast<uint32_t*>(ws + L.off_sums);

    HIP_TRY(hipMemsetAsync(d_res, 0, sizeof(SampleRowsResult), stream));
    HIP_TRY(sample_rows_count(d_nodePointer, d_rows, num_rows, num_nodes, num_edges, fanout, sums, d_res, d_rowPointer_s, stream));
    SampleRowsResult res;
    HIP_TRY(hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (res.bad_id) return fail(TCGNN_ERR_BAD_GRAPH, "tcgnn_sample_rows_count: a listed row id lies outside [0, %d)", num_nodes);
    if (res.bad_ptr)
        return fail(TCGNN_ERR_BAD_GRAPH, "tcgnn_sample_rows_count: nodePointer of a listed row lies outside [0, %lld]", (long long)num_edges);
    if (res.descending) return fail(TCGNN_ERR_BAD_GRAPH, "tcgnn_sample_rows_count: nodePointer descends at a listed row");
    if (res.total > 0x7fffffffu)
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_sample_rows_count: the listed rows keep more than 2^31 - 1 edges (int32 positions only)");
    *num_sampled = (int64_t)res.total;
    return TCGNN_OK;
}

extern "C" int tcgnn_sample_rows(const int32_t* d_nodePointer, const int32_t* d_edgeList, const int32_t* d_rows, const int32_t* d_rowPointer_s,
                                 int32_t num_rows, int32_t num_nodes, int64_t num_edges, int32_t fanout, uint64_t seed, int32_t* d_edgeList_s,
                                 int32_t* d_eid, void* stream) {
    if (!d_nodePointer || !d_rowPointer_s || num_rows < 0 || num_nodes < 0 || num_edges < 0 || (num_rows > 0 && !d_rows))
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_sample_rows: null pointer or bad size");
    if (fanout < 0) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_sample_rows: fanout = %d is negative", fanout);
    if (num_edges > 0x7fffffffLL) return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_sample_rows: int32 CSR positions only (E = %lld)", (long long)num_edges);
    if (num_rows > 0 && num_edges > 0 && fanout > 0 && (!d_edgeList || !d_edgeList_s || !d_eid))   // (nothing is kept otherwise: nothing is written)
        return fail(TCGNN_ERR_INVALID_ARG, "tcgnn_sample_rows: null edge array");
    HIP_TRY(sample_rows_select(d_nodePointer, d_edgeList, d_rows, d_rowPointer_s, num_rows, num_nodes, num_edges, fanout, seed, d_edgeList_s, d_eid,
                               stream));
    return TCGNN_OK;
}
