/*
 * tcgnn.h - C ABI of the MI355X-native TC-GNN aggregation engine (libtcgnn_hip.so).
 *
 * This is the drop-in boundary of the hot path.  Every entry point replaces one function of the
 * reference's `TCGNN` pybind11 module (file:line relative to the reference checkout) and takes
 * plain pointers and sizes only - no torch types.  A Python (ctypes), C++ or any FFI caller can
 * bind it; the binding the reference's maintainers would add is shown in INTEGRATION.md.
 *
 *   reference (TCGNN_conv/TCGNN.cpp)                     this ABI
 *   ---------------------------------------------------  --------------------------------------
 *   preprocess            :172-226 (+ :157-170)          tcgnn_preprocess
 *   preprocess_gpu        :229-256 (unfinished there)    tcgnn_preprocess_gpu
 *   forward  = spmm_forward       :63-86   -> TCGNN_kernel.cu:175-220, :336-454     tcgnn_spmm
 *   forward_AGNN = spmm_forward_AGNN :93-118 -> TCGNN_kernel.cu:227-279, :459-578   tcgnn_spmm_val
 *   forward_ef = sddmm_forward    :126-150 -> TCGNN_kernel.cu:286-327, :584-727     tcgnn_sddmm
 *   backward / backward_ef :270-271 (aliases of forward / forward_ef)               same two calls
 *
 * Conventions
 *   - Every function returns a tcgnn_status (0 = OK) and never aborts the process (the reference
 *     printf()s and exit(-1)s on a launch error, TCGNN_kernel.cu:211-217).  tcgnn_last_error()
 *     returns a thread-local human-readable message for the last non-OK status.
 *   - Device pointers are BORROWED for the duration of the call (the plan borrows the five legacy
 *     arrays for its lifetime, see tcgnn_plan_create); outputs are caller-allocated.
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream).  All device
 *     work is enqueued asynchronously on it.  What synchronises the stream: tcgnn_plan_create (to size its
 *     outputs), tcgnn_preprocess_gpu_ws (ONCE, to read back 24 bytes; it allocates nothing), tcgnn_transpose_ws (ONCE, likewise),
 *     tcgnn_plan_prepare, and - ONLY for a feature width
 *     tcgnn_plan_prepare was not called for - the first tcgnn_spmm / tcgnn_spmm_fused / tcgnn_spmm_gemm
 *     call of that width on a plan whose time model picks the LDS-resident kernel (it builds the
 *     width's cell stream: allocations, a few count-and-place round trips).  Call tcgnn_plan_prepare
 *     for every width a model uses and no hot-path call synchronises, allocates or - inside a HIP
 *     graph capture - takes a different walk than it would outside one.
 *   - Operand range.  The MFMA kernels read a power-of-two-scaled fp16 image of X (one scale per matrix and call): every
 *     element within 2^28 of the largest is rounded bit-for-bit like the reference's TF32 operand (TCGNN_kernel.cu:438-444),
 *     smaller ones lose mantissa bits and, 2^39 below the maximum, are flushed - an absolute error of at most max|X| * 2^-39
 *     per element.  A matrix (or edge-value array) whose largest magnitude is LARGE and which holds nonzero elements more than
 *     2^28 below it is routed - by a test on the device, no read-back - to fp32 fallback kernels that keep fp32's exponent like
 *     the reference does (slow, correct for any magnitudes); everything else stays on the MFMA path.  "Large" is where the
 *     errors one result can collect - at most k = min(longest row of the graph, number of elements of the matrix that lose
 *     bits) of them for an SpMM, min(2 D, that number) for SDDMM and the fused AGNN pair - could leave the contract's
 *     1e-3 max(1, |ref|): max|X| >= 2^29 / k (binary SpMM), max|A| max|X| >= 2^28 / k (edge-valued), max|X|^2 >= 2^29 / k
 *     (SDDMM, fused AGNN).  A training epoch's activations (one stray 1e-5 among 1e4's) stay on the MFMA path.  Images the
 *     CALLER stages (tcgnn_spmm_staged) carry no range words and always take the MFMA path (the kernels
 *     do not look at the rest of such a header).
 *   - Alignment.  Every array needs the alignment of its element type (4 bytes) and no more, with these exceptions, all checked
 *     on the host before anything is enqueued - a refused call has written nothing:
 *       workspaces (d_workspace of every call that takes one)   256 bytes, else TCGNN_ERR_WORKSPACE;
 *       caller-staged images (d_image of tcgnn_spmm_staged / _staged_planar)   256 bytes, d_dst of tcgnn_stage_rows 16 bytes and of
 *         tcgnn_stage_rows_planar 32 bytes, else TCGNN_ERR_INVALID_ARG;
 *       the [N, D] OUTPUT of the plan-based calls - d_Y of tcgnn_spmm / _fused / _scaled / _gemm / _val / _staged / _staged_planar and
 *         of tcgnn_agnn_pair_forward, d_G of tcgnn_agnn_pair_backward -   16 bytes, else TCGNN_ERR_INVALID_ARG (kernels behind the
 *         LDS-resident walks update Y sixteen bytes at a time; any hipMalloc'ed or framework-allocated matrix is aligned far beyond
 *         that - only a view that starts inside another buffer is not);
 *       d_scratch of tcgnn_edge_softmax_backward   8 bytes.
 *     INPUTS of the plan-based calls (X, Z, dY, gate, edge values, row_scale / col_scale / bias, W, the saved ef and ef_absmax, the
 *     scalars d_w / d_beta) and the per-edge / per-word outputs (d_ef, d_ef_absmax, d_dw, d_out of tcgnn_permute_edge_values) may start
 *     at any 4-byte boundary, e.g. a contiguous view one float into a larger tensor: the staging pass takes 16-byte loads only where
 *     the pointer allows them, and the results are bit for bit those of the aligned call.
 *   - Workspace size.  A call that takes d_workspace returns TCGNN_ERR_WORKSPACE, before anything is enqueued, when workspace_bytes
 *     is below what the matching query answers NOW (tcgnn_workspace_bytes for the plan and width - ask again after
 *     tcgnn_plan_prepare[_val] and after a mode switch -, tcgnn_sddmm2_workspace_bytes for tcgnn_sddmm2), whichever walk would run;
 *     no call writes a byte beyond that size.
 *   - Index arrays are int32 (the reference API's dtype); all address arithmetic inside the
 *     kernels is 64-bit, so N*D may exceed 2^32 (the reference overflows there,
 *     TCGNN_kernel.cu:420).
 *   - Tile unit: blockPartition counts 16x8 TC blocks per 16-row window (config.h:4-5); the
 *     kernels consume them four at a time as 16x32 MFMA operand tiles.
 */
#ifndef TCGNN_H
#define TCGNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TCGNN_ABI_VERSION 1
#define TCGNN_BLK_H 16 /* rows per row window          (config.h:4) */
#define TCGNN_BLK_W 8  /* condensed columns per TC block (config.h:5) */

typedef enum tcgnn_status {
    TCGNN_OK = 0,
    TCGNN_ERR_INVALID_ARG = 1, /* null pointer, negative size, unsupported tile shape ... */
    TCGNN_ERR_HIP = 2,         /* a HIP runtime call or kernel launch failed             */
    TCGNN_ERR_OOM = 3,         /* host or device allocation failed                       */
    TCGNN_ERR_BAD_GRAPH = 4,   /* metadata inconsistent with the CSR (out-of-range ids)  */
    TCGNN_ERR_WORKSPACE = 5,   /* workspace pointer null or smaller than required        */
    TCGNN_ERR_UNSUPPORTED = 6  /* the fused entry point does not cover this plan / width  */
} tcgnn_status;

/* Opaque device-resident translation of one graph: the condensed 16x32 tile stream the kernels
 * read (per tile: 32 source-row ids, a 16x32 adjacency bitmask, 16 edge offsets). */
typedef struct tcgnn_plan tcgnn_plan;

typedef struct tcgnn_plan_info {
    int32_t num_nodes;       /* N */
    int32_t num_windows;     /* ceil(N/16) as given by the caller's blockPartition length */
    int64_t num_edges;       /* E = nnz of the CSR */
    int64_t tc_blocks;       /* sum(blockPartition): 16x8 TC blocks (the reference's "TC_Blocks") */
    int64_t wide_blocks;     /* 16x32 operand tiles actually streamed by the kernels */
    int64_t plan_bytes;      /* device bytes owned by the plan */
    int32_t canonical;       /* 1 if every CSR row is strictly increasing (scipy canonical form) */
    int32_t waves_per_window;/* workgroup shape the launcher picked (1 or 4 wavefronts) */
    int32_t column_buckets;  /* > 0: the plan carries the bucket table of the range-blocked SpMM walk */
    int32_t lds_ranges;      /* > 0: the plan carries a cell stream of the LDS-resident column-range SpMM (column ranges of the
                              * finest stream built so far; streams are per pass width and built on first use) */
} tcgnn_plan_info;

int tcgnn_abi_version(void);
const char* tcgnn_status_string(int status);
const char* tcgnn_last_error(void);

/* ---- sparse-graph translation (SGT) ------------------------------------------------------- */

/* Host SGT.  Replaces TCGNN.preprocess (TCGNN.cpp:172-226): fills, in place,
 *   edgeToRow[e]      = row of CSR edge e,
 *   edgeToColumn[e]   = rank of edgeList[e] among the sorted unique column ids of e's row window,
 *   blockPartition[w] = ceil(#unique / blockSize_w), and 1 for a window without edges (what the
 *                       reference's zero-length read yields, TCGNN.cpp:160),
 * for w < bp_len only (the reference writes one slot past the end when N % blockSize_h == 0).
 * *tc_blocks receives the count the reference prints as "TC_Blocks" (including that phantom
 * window).  All pointers are HOST memory.  num_threads <= 0 means "all hardware threads".
 * Rows need not be sorted and may hold duplicate columns. */
int tcgnn_preprocess(const int32_t* edgeList, const int32_t* nodePointer, int32_t num_nodes,
                     int32_t blockSize_h, int32_t blockSize_w, int32_t* blockPartition,
                     int64_t bp_len, int32_t* edgeToColumn, int32_t* edgeToRow,
                     int64_t* tc_blocks, int32_t num_threads);

/* Device SGT.  Same outputs as tcgnn_preprocess, all pointers DEVICE memory.  Finishes what the
 * reference's preprocess_gpu / fill_window only sketch (TCGNN.cpp:229-256,
 * TCGNN_kernel.cu:42-80).
 *
 * tcgnn_preprocess_gpu_ws (r06) runs on CALLER scratch: d_workspace of at least
 * tcgnn_preprocess_gpu_workspace_bytes(num_nodes, num_edges, blockSize_h) bytes, 256-byte aligned (sort keys / positions / flags /
 * ranks of the num_edges edge slots plus rocPRIM's scratch: ~2.3 GB at Reddit size).  It allocates and frees NOTHING and synchronises
 * `stream` ONCE, to read back 24 bytes - nodePointer[0], nodePointer[num_nodes], the largest column id and *tc_blocks.  (A graph with
 * column ids beyond num_nodes - legal, the host path takes them too - is sorted a second time with every key bit: the only way to a
 * second synchronisation.)  Malformed row pointers are reported (TCGNN_ERR_BAD_GRAPH) after that read-back; until then every index
 * derived from them is clamped to the arrays.
 * tcgnn_preprocess_gpu keeps the reference's shape (no scratch argument): it allocates the workspace with hipMalloc, calls the _ws
 * form and frees it - what r01-r05 measured as 5 ms or 95 ms by the allocator's mood. */
int tcgnn_preprocess_gpu_workspace_bytes(int32_t num_nodes, int64_t num_edges, int32_t blockSize_h, size_t* bytes);
int tcgnn_preprocess_gpu_ws(const int32_t* d_edgeList, const int32_t* d_nodePointer,
                            int32_t num_nodes, int64_t num_edges, int32_t blockSize_h,
                            int32_t blockSize_w, int32_t* d_blockPartition, int64_t bp_len,
                            int32_t* d_edgeToColumn, int32_t* d_edgeToRow, void* d_workspace,
                            size_t workspace_bytes, int64_t* tc_blocks, void* stream);
int tcgnn_preprocess_gpu(const int32_t* d_edgeList, const int32_t* d_nodePointer,
                         int32_t num_nodes, int64_t num_edges, int32_t blockSize_h,
                         int32_t blockSize_w, int32_t* d_blockPartition, int64_t bp_len,
                         int32_t* d_edgeToColumn, int32_t* d_edgeToRow, int64_t* tc_blocks,
                         void* stream);

/* CSR transpose (no counterpart in the reference, whose layers back-propagate through A, gnn_conv.py:46,80,110,143: right only on
 * a symmetric graph).  From A's CSR (DEVICE memory) it builds A^T's:
 *   d_nodePointer_t [num_nodes + 1], d_edgeList_t [num_edges]: row c of A^T lists the rows r of every entry (r, c) of A in increasing
 *                    CSR position - sorted rows even when A's are not; A's duplicate entries stay, next to each other;
 *   d_perm [num_edges]: perm[eT] = the CSR position in A of A^T's entry eT (a bijection on [0, num_edges));
 *   *symmetric      = 1 exactly when (nodePointer_t, edgeList_t) equal (nodePointer, edgeList), else 0 (may be NULL).
 * The graph must be square: nodePointer[0] = 0, monotone, nodePointer[num_nodes] = num_edges and every id in [0, num_nodes) (the
 * forward path takes larger ids; a transpose can not), else TCGNN_ERR_BAD_GRAPH.  Until that check every index derived from the
 * input is clamped to the arrays.  Runs on CALLER scratch (tcgnn_transpose_workspace_bytes, 256-byte aligned: sorted keys, row ids
 * and rocPRIM's scratch, ~8 num_edges bytes plus the sort's own), allocates nothing and synchronises `stream` ONCE, to read back the
 * validation words and the symmetry flag.
 * tcgnn_permute_edge_values: out[eT] = val[perm[eT]] - the edge values of A in A^T's order, for tcgnn_spmm_val on A^T's plan.
 * Stream-ordered, no allocation, no synchronisation; perm must be one tcgnn_transpose_ws wrote. */
int tcgnn_transpose_workspace_bytes(int32_t num_nodes, int64_t num_edges, size_t* bytes);
int tcgnn_transpose_ws(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges,
                       int32_t* d_nodePointer_t, int32_t* d_edgeList_t, int32_t* d_perm, void* d_workspace,
                       size_t workspace_bytes, int32_t* symmetric, void* stream);
int tcgnn_permute_edge_values(const float* d_val, const int32_t* d_perm, int64_t num_edges, float* d_out, void* stream);

/* Seeded neighbour sampling (no counterpart in the reference): the graph over the SAME num_nodes nodes that keeps at most `fanout`
 * in-edges per row - what fan-out training (GraphSAGE; DGL's sample_neighbors) aggregates over.  Every operator of this header takes
 * the result as it takes any square CSR.  Every CSR position e gets a 64-bit word that depends on (seed, e) alone, all arithmetic
 * modulo 2^64:
 *     G = 0x9E3779B97F4A7C15
 *     mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
 *     h32(seed, e)  = mix(mix(seed + G) + (e + 1) * G) >> 32
 *     word(seed, e) = (h32(seed, e) << 32) | e                       (unique: no tie rule)
 * A row of degree d <= fanout keeps all its edges, a longer one the fanout positions with the smallest words; a row whose d_row_mask
 * byte (uint8 [num_nodes], may be NULL: all ones) is 0 keeps none.  Kept edges stay in CSR order.  Outputs:
 *   d_nodePointer_s [num_nodes + 1], d_edgeList_s [E'], d_eid [E']: eid = the CSR position in the input of every kept edge.
 * A pure function of its inputs (no global atomics): bit-identical on repetition; without replacement, uniform over the
 * fanout-subsets of a row up to collisions of h32.  DEVICE pointers.
 * tcgnn_sample_neighbors_count: writes d_nodePointer_s (an exclusive scan of min(d, fanout) * mask) and *num_sampled = E', on CALLER
 *   scratch (tcgnn_sample_workspace_bytes, 256-byte aligned; allocates nothing), and synchronises `stream` ONCE to read back E' and the
 *   validation words: nodePointer[0] = 0, monotone, nodePointer[num_nodes] = num_edges, else TCGNN_ERR_BAD_GRAPH.  Until that check
 *   every index derived from nodePointer is clamped to [0, num_edges].
 * tcgnn_sample_neighbors: with the d_nodePointer_s the count call wrote for the same (nodePointer, row_mask, fanout), writes exactly E'
 *   entries of d_edgeList_s and of d_eid.  Stream-ordered, no allocation, no synchronisation; reads the column id of kept edges only.
 * Both return TCGNN_ERR_INVALID_ARG before any launch for num_edges > 2^31 - 1, a negative fanout or a null required pointer, the count
 * call TCGNN_ERR_WORKSPACE for scratch that is too small or not 256-byte aligned. */
int tcgnn_sample_workspace_bytes(int32_t num_nodes, size_t* bytes);
int tcgnn_sample_neighbors_count(const int32_t* d_nodePointer, const uint8_t* d_row_mask, int32_t num_nodes, int64_t num_edges,
                                 int32_t fanout, int32_t* d_nodePointer_s, void* d_workspace, size_t workspace_bytes,
                                 int64_t* num_sampled, void* stream);
int tcgnn_sample_neighbors(const int32_t* d_nodePointer, const int32_t* d_edgeList, const uint8_t* d_row_mask,
                           const int32_t* d_nodePointer_s, int32_t num_nodes, int64_t num_edges, int32_t fanout, uint64_t seed,
                           int32_t* d_edgeList_s, int32_t* d_eid, void* stream);

/* Relabelled mini-batch blocks (no counterpart in the reference): the sampled layer graphs of one mini-batch keep all num_nodes rows;
 * these calls find the M nodes they touch and emit the same graphs over those M nodes.  Inputs: one or more CSRs over the same
 * num_nodes nodes and a byte mask d_keep [num_nodes] that the caller has cleared or filled with the seeds.  The node set is every v for
 * which, in any of the graphs, keep[v] != 0 held beforehand, v has at least one edge, or v is a column id.  Outputs:
 *   d_nodes  int32 [M], strictly increasing: the kept original ids;
 *   d_new_id int32 [num_nodes]: the rank of v in nodes, or -1;
 *   per graph d_nodePointer_b [M + 1], d_edgeList_b [num_edges]:
 *     nodePointer_b[i] = nodePointer[nodes[i]], nodePointer_b[M] = num_edges, edgeList_b[e] = new_id[edgeList[e]].
 * The relabelling is monotone, so the result is a SQUARE CSR over M nodes in which every row keeps its edges in their order: sorted
 * rows stay sorted, the number and order of edges do not change (a sampled graph's eid serves its compact form as it is), and every
 * operator of this header takes it.  A pure function of the inputs, bit-identical on repetition; no global atomics (the mask and the
 * validation word only ever receive concurrent stores of the same value).  DEVICE pointers; caller scratch
 * (tcgnn_compact_workspace_bytes, 256-byte aligned, answered without a device); nothing allocates; everything is stream-ordered.
 * One mini-batch is begin, mark per graph, count, nodes, graph per graph - ONE stream synchronisation in all:
 * tcgnn_compact_begin  clears the workspace's validation word.  Needed before the first mark call on a workspace; the count call leaves
 *                      the word clear again.
 * tcgnn_compact_mark   sets d_keep[v] = 1 for every row with edges and every column id in [0, num_nodes) of the num_edges entries of
 *                      d_edgeList.  A column id outside that range, nodePointer[0] != 0, a descending pair, a pointer outside
 *                      [0, num_edges] or nodePointer[num_nodes] != num_edges sets the validation word; none of them is followed.
 * tcgnn_compact_count  writes all num_nodes entries of d_new_id (the exclusive scan of keep != 0) and *num_kept = M, and synchronises
 *                      `stream` ONCE to read back M and the validation word: TCGNN_ERR_BAD_GRAPH when a mark call on this workspace
 *                      since the last begin / count set it (*num_kept is then left alone).
 * tcgnn_compact_nodes  writes exactly num_kept entries of d_nodes from the d_new_id and M of the count call.
 * tcgnn_compact_graph  writes exactly num_kept + 1 entries of d_nodePointer_b and num_edges of d_edgeList_b.  Contract: d_new_id comes
 *                      from a mask the mark call saw THIS graph with.  For any other input the call stays memory-safe - every index is
 *                      checked or clamped, a column without a new id is written as 0 - and the result is unspecified.
 * All before any launch: a null required pointer, a negative size, num_kept > num_nodes or num_edges > 2^31 - 1 is
 * TCGNN_ERR_INVALID_ARG; a workspace that is null, short or not 256-byte aligned TCGNN_ERR_WORKSPACE; num_nodes = 0 and
 * num_edges = 0 give TCGNN_OK (arrays of no entries may be NULL). */
int tcgnn_compact_workspace_bytes(int32_t num_nodes, size_t* bytes);
int tcgnn_compact_begin(int32_t num_nodes, void* d_workspace, size_t workspace_bytes, void* stream);
int tcgnn_compact_mark(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges, uint8_t* d_keep,
                       void* d_workspace, size_t workspace_bytes, void* stream);
int tcgnn_compact_count(const uint8_t* d_keep, int32_t num_nodes, int32_t* d_new_id, void* d_workspace, size_t workspace_bytes,
                        int32_t* num_kept, void* stream);
int tcgnn_compact_nodes(const int32_t* d_new_id, int32_t num_nodes, int32_t num_kept, int32_t* d_nodes, void* stream);
int tcgnn_compact_graph(const int32_t* d_nodePointer, const int32_t* d_edgeList, const int32_t* d_new_id, const int32_t* d_nodes,
                        int32_t num_nodes, int32_t num_kept, int64_t num_edges, int32_t* d_nodePointer_b, int32_t* d_edgeList_b,
                        void* stream);

/* Seed-list sampling (no counterpart in the reference): the two sections above from LISTS of row ids, so that one mini-batch costs the
 * rows it touches and not num_nodes (DGL's and PyG's loaders sample from a list of seed nodes).  A row-list graph has one row per
 * entry of d_rows (int32 [num_rows], any order, an id may repeat: every occurrence has its own slot):
 *   d_rowPointer_s [num_rows + 1]: rowPointer_s[i] = the sum over j < i of min(deg(rows[j]), fanout);
 *   d_edgeList_s [E'], d_eid [E']: slot i holds what row rows[i] of tcgnn_sample_neighbors(..., fanout, seed) holds - the same words
 *     h32(seed, e), the same rule (the fanout smallest words of the row, kept in CSR order), eid = the position in the FULL CSR.
 * nodePointer[r] and nodePointer[r + 1] are read for listed r ONLY: the pointers of unlisted rows are neither read nor validated.
 * Pure functions of their inputs (no global atomics), bit-identical on repetition.  DEVICE pointers.
 * tcgnn_sample_rows_workspace_bytes: answered without a device - the result words plus one partial sum per 1 024 of the list's
 *   num_rows + 1 slots (256-byte aligned parts).
 * tcgnn_sample_rows_count: writes d_rowPointer_s and *num_sampled = E' on CALLER scratch and synchronises `stream` ONCE to read back E'
 *   and the validation words.  A listed id outside [0, num_nodes), a descending pointer pair at a listed row or a pointer of a listed
 *   row outside [0, num_edges] is TCGNN_ERR_BAD_GRAPH, reported behind the read-back; until then such an id is an empty row and every
 *   index derived from nodePointer is clamped to [0, num_edges].  A list whose rows keep more than 2^31 - 1 edges (possible with
 *   repeats) is TCGNN_ERR_INVALID_ARG, also behind the read-back: the sums saturate, nothing wraps.
 * tcgnn_sample_rows: with the d_rowPointer_s the count call wrote for the same (nodePointer, rows, fanout), writes exactly E' entries
 *   of d_edgeList_s and of d_eid; a row never writes beyond the slot rowPointer_s gives it.  Stream-ordered, no allocation, no
 *   synchronisation; one workgroup per four list slots.
 * Both return TCGNN_ERR_INVALID_ARG before any launch for num_edges > 2^31 - 1, a negative size or fanout or a null required pointer
 * (d_rows may be NULL when num_rows = 0), the count call TCGNN_ERR_WORKSPACE for scratch that is too small or not 256-byte aligned.
 *
 * The node set and the blocks of row-list graphs, with tcgnn_compact_begin / _count / _nodes and their workspace as above:
 * tcgnn_compact_mark_ids    sets d_keep[id] = 1 for `count` ids (the seeds; the d_edgeList_s of a row-list graph).  An id outside
 *                           [0, num_nodes) sets the workspace's validation word and is not followed, as tcgnn_compact_mark treats a
 *                           bad column; tcgnn_compact_count reports it.  Concurrent stores only ever write the same value.
 * tcgnn_compact_rows_graph  the square block over the num_kept = M nodes of a row-list graph whose d_rows are STRICTLY INCREASING (as
 *                           tcgnn_compact_nodes emits them): writes exactly M + 1 entries of d_nodePointer_b and num_sampled of
 *                           d_edgeList_b, nodePointer_b[j] = rowPointer_s[#{i : new_id[rows[i]] < j}] (a node of the batch that is
 *                           not listed gets an empty row), nodePointer_b[M] = num_sampled, edgeList_b[e] = new_id[edgeList_s[e]].
 *                           One writer per slot, no synchronisation.  Under rows that are not increasing or a d_new_id that never saw
 *                           the graph the call stays memory-safe - every index is checked or clamped, a column without a new id is
 *                           written as 0 - and the result is unspecified.
 * Null pointers, negative sizes and workspaces are refused as in the section above. */
int tcgnn_sample_rows_workspace_bytes(int32_t num_rows, size_t* bytes);
int tcgnn_sample_rows_count(const int32_t* d_nodePointer, const int32_t* d_rows, int32_t num_rows, int32_t num_nodes, int64_t num_edges,
                            int32_t fanout, int32_t* d_rowPointer_s, void* d_workspace, size_t workspace_bytes, int64_t* num_sampled,
                            void* stream);
int tcgnn_sample_rows(const int32_t* d_nodePointer, const int32_t* d_edgeList, const int32_t* d_rows, const int32_t* d_rowPointer_s,
                      int32_t num_rows, int32_t num_nodes, int64_t num_edges, int32_t fanout, uint64_t seed, int32_t* d_edgeList_s,
                      int32_t* d_eid, void* stream);
int tcgnn_compact_mark_ids(const int32_t* d_ids, int64_t count, int32_t num_nodes, uint8_t* d_keep, void* d_workspace,
                           size_t workspace_bytes, void* stream);
int tcgnn_compact_rows_graph(const int32_t* d_rows, int32_t num_rows, const int32_t* d_rowPointer_s, const int32_t* d_edgeList_s,
                             int64_t num_sampled, const int32_t* d_new_id, int32_t num_nodes, int32_t num_kept, int32_t* d_nodePointer_b,
                             int32_t* d_edgeList_b, void* stream);

/* Subgraph sampling (no counterpart in the reference): the other family of mini-batches - a node set drawn by random walks (GraphSAINT)
 * or taken as a range of ids (Cluster-GCN) and the subgraph the full graph INDUCES on it (DGL's random_walk / node_subgraph, PyG's
 * subgraph).  The induced subgraph is a square CSR over its M nodes in which every row is used: one block serves every layer.
 * Both operations take DEVICE pointers, are pure functions of their inputs (no global atomics), bit-identical on repetition, run on
 * caller scratch, allocate nothing and are stream-ordered.
 *
 * tcgnn_random_walk: d_walks int32 [num_walks, length + 1], row-major.  walks[w][0] = starts[w]; for t = 0 .. length - 1, with
 *   v = walks[w][t]:  v outside [0, num_nodes): the walk stays on it, walks[w][t + 1] = v, and nothing is read through it;
 *   otherwise lo, hi = nodePointer[v], nodePointer[v + 1], each clamped to [0, num_edges], d = hi - lo;  d <= 0: the walk stays on v
 *   (torch_cluster's rule for a node without edges, so every entry of walks is an id and needs no filtering);  otherwise
 *     walks[w][t + 1] = edgeList[lo + ((h32(seed, w * length + t) * d) >> 32)]
 *   with h32 of the sampling section above, its second argument a 64-bit integer (arithmetic modulo 2^64); the product is a 64-bit one,
 *   below 2^63 because d <= 2^31 - 1.  A column id outside [0, num_nodes) is written and then not followed.  Rows hold IN-edges, so a
 *   walk moves from a node to one of its SOURCES - the direction neighbour sampling expands in.  One lane per walk; no workspace, no
 *   synchronisation and no report: an id out of range reaches tcgnn_compact_mark_ids, which sets the validation word that
 *   tcgnn_compact_count reports.  TCGNN_ERR_INVALID_ARG before any launch: a null required pointer (d_starts and d_walks may be NULL
 *   when num_walks = 0, d_edgeList when num_edges = 0), a negative size or length, num_edges > 2^31 - 1,
 *   num_walks * (length + 1) > 2^31 - 1.
 *
 * tcgnn_induce_*: the node-induced subgraph of a CSR over a node list.  Inputs: d_nodePointer, d_edgeList; d_nodes int32 [num_kept = M],
 *   STRICTLY INCREASING, as tcgnn_compact_nodes emits it; d_new_id int32 [num_nodes], from the tcgnn_compact_count of the same mask.
 *   Outputs: d_nodePointer_b [M + 1], d_edgeList_b [E_b], d_eid [E_b].  Row i of the result holds, in CSR order, the positions e in
 *   [nodePointer[nodes[i]], nodePointer[nodes[i] + 1]) with new_id[edgeList[e]] >= 0; for each of them edgeList_b = new_id[edgeList[e]]
 *   and eid = e, the position in the FULL CSR (edge values of the block are val[eid]).  The relabelling is monotone: sorted rows stay
 *   sorted, the block is square over M nodes and every operator of this header takes it.
 * tcgnn_induce_workspace_bytes: answered without a device - 256 bytes for the result words plus, rounded up to 256 bytes, one 4-byte
 *   partial sum per 1 024 of the list's num_kept + 1 slots.
 * tcgnn_induce_count: writes d_nodePointer_b and *num_induced = E_b on CALLER scratch and synchronises `stream` ONCE to read back E_b
 *   and the validation words.  nodePointer is read, and validated, at LISTED rows only.  A listed id outside [0, num_nodes), a
 *   descending pointer pair at a listed row, a pointer of a listed row outside [0, num_edges] or a column id outside [0, num_nodes) in
 *   a listed row is TCGNN_ERR_BAD_GRAPH, reported behind the read-back; until then such a row is empty or such an edge dropped, and
 *   every index is clamped.  The sums saturate: a list with repeats (outside the contract) whose rows keep more than 2^31 - 1 edges is
 *   TCGNN_ERR_INVALID_ARG behind the read-back, nothing wraps.
 * tcgnn_induce: with the d_nodePointer_b and num_induced = E_b of the count call for the same inputs, writes exactly E_b entries of
 *   d_edgeList_b and of d_eid.  No allocation, no synchronisation; a row never writes beyond the slot nodePointer_b gives it, nor
 *   beyond E_b.  One wavefront per listed row of up to 1 024 edges, four rows per workgroup; the whole workgroup takes a longer row.
 * Outside the contract - nodes not increasing, a new_id of another mask, values >= M in it - both calls stay memory-safe: every index
 * is checked or clamped, a new id outside [0, M) is written as 0; the result is then unspecified.
 * Before any launch both refuse a null required pointer (arrays of no entries may be NULL), a negative size, num_kept > num_nodes and
 * num_edges > 2^31 - 1 with TCGNN_ERR_INVALID_ARG; the count call refuses a workspace that is null, short or not 256-byte aligned with
 * TCGNN_ERR_WORKSPACE.  num_kept = 0 gives TCGNN_OK (nodePointer_b[0] = 0, E_b = 0). */
int tcgnn_random_walk(const int32_t* d_nodePointer, const int32_t* d_edgeList, const int32_t* d_starts, int32_t num_walks,
                      int32_t num_nodes, int64_t num_edges, int32_t length, uint64_t seed, int32_t* d_walks, void* stream);
int tcgnn_induce_workspace_bytes(int32_t num_kept, size_t* bytes);
int tcgnn_induce_count(const int32_t* d_nodePointer, const int32_t* d_edgeList, const int32_t* d_nodes, const int32_t* d_new_id,
                       int32_t num_kept, int32_t num_nodes, int64_t num_edges, int32_t* d_nodePointer_b, void* d_workspace,
                       size_t workspace_bytes, int64_t* num_induced, void* stream);
int tcgnn_induce(const int32_t* d_nodePointer, const int32_t* d_edgeList, const int32_t* d_nodes, const int32_t* d_new_id,
                 const int32_t* d_nodePointer_b, int32_t num_kept, int32_t num_nodes, int64_t num_edges, int64_t num_induced,
                 int32_t* d_edgeList_b, int32_t* d_eid, void* stream);

/* Tile statistics of the translation - what the reference's counting scripts report
 * (3_cnt_TC_blk_SpMM.py:38-94 with 16x8 tiles, 3_cnt_TC_blk_SDDMM.py with 16x16; logs/16x8_reduction.csv,
 * logs/reduce_blocks.csv): per window of tile_h rows, U = sorted unique neighbour ids;
 * condensed tiles = ceil(|U|/tile_w), sliding tiles = greedy cover of U by intervals of tile_w ids.
 * HOST pointers; rows need not be sorted.  num_threads <= 0 means "all hardware threads". */
typedef struct tcgnn_tile_stats_t {
    int64_t windows;                 /* ceil(N / tile_h) */
    int64_t nonempty_windows;
    int64_t edges;                   /* nnz of the CSR (duplicates included) */
    int64_t unique_columns;          /* sum over windows of |U| */
    int64_t sliding_tiles;           /* the scripts' "origin" column */
    int64_t condensed_tiles;         /* the scripts' "reduced" column */
    int64_t max_sliding_per_window;
    int64_t max_condensed_per_window;
} tcgnn_tile_stats_t;
int tcgnn_tile_stats(const int32_t* edgeList, const int32_t* nodePointer, int32_t num_nodes,
                     int32_t tile_h, int32_t tile_w, tcgnn_tile_stats_t* out, int32_t num_threads);

/* ---- plan: legacy metadata -> packed tile stream (device) --------------------------------- */

/* Builds the packed tile stream on the device from the five legacy arrays every reference entry
 * point receives (TCGNN.cpp:63-70).  The arrays are DEVICE pointers and stay borrowed by the
 * plan until tcgnn_plan_destroy (the fallback kernels for non-canonical CSRs read them).
 * Synchronises `stream` once. */
int tcgnn_plan_create(const int32_t* d_nodePointer, const int32_t* d_edgeList,
                      const int32_t* d_blockPartition, const int32_t* d_edgeToColumn,
                      const int32_t* d_edgeToRow, int32_t num_nodes, int64_t num_edges,
                      int32_t num_windows, void* stream, tcgnn_plan** plan_out);
/* Row-sharded variant for multi-GPU runs (no counterpart in the reference, which is single-GPU):
 * A holds `num_rows` rows (this rank's row windows; nodePointer has num_rows + 1 entries) whose
 * column ids index a feature matrix of `num_cols` rows (the all-gathered X); A's row r is X's row
 * row_offset + r (used by SDDMM).  X passed to the kernels is [num_cols, D], Y is [num_rows, D]. */
int tcgnn_plan_create_sharded(const int32_t* d_nodePointer, const int32_t* d_edgeList,
                              const int32_t* d_blockPartition, const int32_t* d_edgeToColumn,
                              const int32_t* d_edgeToRow, int32_t num_rows, int32_t num_cols,
                              int32_t row_offset, int64_t num_edges, int32_t num_windows,
                              void* stream, tcgnn_plan** plan_out);
/* Builds, now, whatever the hot path would otherwise build on its first call at feature width D (the cell stream(s) of the
 * LDS-resident kernel where the plan's time model picks it for that width; nothing for the gather walks).  Synchronises
 * `stream`.  Idempotent; widths are independent.  No counterpart in the reference (its kernels re-derive their tiles per launch). */
int tcgnn_plan_prepare(tcgnn_plan* plan, int32_t D, void* stream);
/* The same for the EDGE-VALUED SpMM (tcgnn_spmm_val = TCGNN.forward_AGNN, gnn_conv.py:132,143): builds the single-edge cell stream of the
 * LDS-resident edge-valued walk where the plan takes that walk at width D (whole 64-column chunks, alone or followed by a remainder of
 * 33 .. 48 columns - Reddit's 41 classes -, on graphs the time model sends to the LDS-resident kernel; nothing otherwise).  Call it BEFORE tcgnn_workspace_bytes: the answer then includes the per-call slot
 * values, and the first tcgnn_spmm_val of that width neither allocates nor synchronises nor takes the gather walk.  Synchronises
 * `stream`.  Idempotent. */
int tcgnn_plan_prepare_val(tcgnn_plan* plan, int32_t D, void* stream);
int tcgnn_plan_destroy(tcgnn_plan* plan);
int tcgnn_plan_get_info(const tcgnn_plan* plan, tcgnn_plan_info* info);

/* Tuning / test aid: which SpMM walk tcgnn_spmm and tcgnn_spmm_val use.  0 = automatic (default: per plan
 * and feature width, the LDS-resident kernel or the gather walks by their time models - DESIGN.md "Which walk
 * runs"; among the gather walks range-blocked when the fp16 image of X exceeds the L2 and the windows are long;
 * TCGNN_LDS_AUTO=0 in the environment keeps the automatic mode off the LDS-resident kernel), 1 = always the
 * plain per-window kernel, 2 = range-blocked whenever the plan has a bucket table, 3 = the
 * LDS-resident column-range kernel (binary SpMM only; builds its cell stream on first use if the
 * plan was created without one), 4 = the single-launch fp32-MFMA kernel small graphs take automatically
 * (no staging pass; binary SpMM only), 5 = the slice-synchronised range walk (r06: graphs whose communities exceed an XCD's L2 -
 * taken automatically there - from 64 columns, sparse windows, by operator and hot span: DESIGN.md 4.4; forced, it runs wherever the plan built its tables and falls back to the
 * gather walks elsewhere; SDDMM and the fused AGNN pair follow the same switch).  Process-wide; the environment variable TCGNN_SPMM_MODE sets the initial value. */
int tcgnn_set_spmm_mode(int32_t mode);
/* The same switch for ONE plan: mode 0 .. 5 as above, -1 = follow the process-wide value (the default).  Two plans of one process may
 * walk differently. */
int tcgnn_plan_set_spmm_mode(tcgnn_plan* plan, int32_t mode);

/* The range guard (see "Operand range" above), process-wide level (environment TCGNN_RANGE_GUARD sets the initial one):
 *   0  off - every call stays on the MFMA path;
 *   1  the aggregation operators are guarded: tcgnn_spmm / _fused / _gemm and tcgnn_spmm_val, whose error bound is LINEAR in
 *      max|X| - k max 2^-39 - and which ordinary training tensors never reach;
 *   2  (default since r04) also tcgnn_sddmm and the fused AGNN pair, whose bound is QUADRATIC - min(2 D, lost elements)
 *      max|X|^2 2^-39 - for what training produces: with the reference's unscaled weights an AGNN epoch's activations (max ~3e4,
 *      ONE element 2^28 below) cross that bound now and then.  Such a matrix has "dirty" rows - rows of X holding elements that lose
 *      bits in the image; the conversion pass marks them in a bitmap behind the image - and the MFMA kernels run as usual while one
 *      more launch scans the edges and recomputes, in fp32 with the reference's operand rounding, exactly the edges that touch a
 *      dirty row (scores, their share of the aggregate and of d_w): ~0.2 ms of scan plus a wavefront's work per such edge when it
 *      happens, a launch that returns at once when it does not.  Any number of dirty rows (r04 patched at most 48 and left a matrix
 *      with more - hub rows of a power-law graph under unscaled weights - to the bound above: closed in r05).  On a structurally
 *      symmetric graph (checked once, at plan creation) up to 256 dirty rows are patched without the scan: a dirty row's own edges
 *      and their mirrors, ~10 us - what a training epoch usually meets;
 *   3  strict: a wide matrix is computed in plain fp32, CSR order, by SDDMM and the fused AGNN pair as well (correct for any
 *      magnitudes, ~50x slower than the MFMA path on a Reddit-sized graph; level 2 gives the same guarantee at the cost of the dirty edges).
 * tcgnn_range_mode reports which way the LAST staged call on this workspace went: *wide_x = 1 if its feature matrix took the fp32
 * fallback as a binary SpMM / SDDMM / fused AGNN operand, 2 if it stayed on the MFMA path with its dirty rows patched (SDDMM /
 * fused AGNN), *wide_val (optional) = 1 if it took the fallback as an edge-valued SpMM.  Reads 40 bytes of the workspace header
 * back: synchronises `stream` (a test / diagnosis aid, like tcgnn_plan_last_kernel - the hot path never reads anything back). */
int tcgnn_set_range_guard(int32_t level);
/* The guard level of ONE plan: 0 .. 3 as above, -1 = follow the process-wide level (the default). */
int tcgnn_plan_set_range_guard(tcgnn_plan* plan, int32_t level);
int tcgnn_range_mode(const void* d_workspace, void* stream, int32_t* wide_x, int32_t* wide_val);

/* One-pass staging.  A call that stages X as the planar image of the LDS-resident kernels (D a multiple of 16, X and the gate 16-byte
 * aligned) reads X once: the plan remembers the power-of-two scale of the last matrix staged per kind of call, the pass converts
 * with it while it takes the abs-max, and a second, short launch checks the guess - converting again only when max |X| has crossed a
 * power of two (a "miss").  Results do not depend on it: image, header and Y are bit for bit those of the two-pass staging.
 * tcgnn_set_stage_onepass(0) keeps every call on the two-pass staging (process-wide, read per call; the environment variable
 * TCGNN_STAGE_ONEPASS sets the initial value, default 1).  tcgnn_plan_stage_stats reports how many of the plan's calls so far hit and
 * missed; it reads two device words back and synchronises `stream` (a test / diagnosis aid, like tcgnn_range_mode). */
int tcgnn_set_stage_onepass(int32_t on);
int tcgnn_plan_stage_stats(const tcgnn_plan* plan, void* stream, int64_t* hits, int64_t* misses);

/* Measurement aid: reserve HIP event pairs for up to `max_calls` kernel calls (0 = off).  While
 * enabled, tcgnn_spmm / tcgnn_spmm_val / tcgnn_sddmm bracket their main kernel (not the fp16
 * staging pass) with events recorded on the caller's stream, without synchronising.
 * tcgnn_plan_read_timing waits for the recorded calls, returns their durations in milliseconds
 * (call order) and rearms the pairs. */
int tcgnn_plan_set_timing(tcgnn_plan* plan, int32_t max_calls);
/* Measurement aid: name of the main kernel the most recent hot-path call on this plan launched ("spmm_lds_kernel",
 * "spmm_blocked_kernel", "spmm_kernel", "spmm_small_kernel", "sddmm_kernel", "agnn_kernel", ...; "" before the first call) -
 * so a benchmark line names the kernel that ran instead of re-deriving the launcher's choice.  Static storage. */
const char* tcgnn_plan_last_kernel(const tcgnn_plan* plan);
int tcgnn_plan_read_timing(tcgnn_plan* plan, float* ms_out, int32_t capacity, int32_t* count);

/* Scratch bytes the three kernels need for feature width D (fp16 staging copy of X with one
 * zero sentinel row, plus the scale words).  The caller owns the scratch; it must be 256-byte
 * aligned device memory and may be reused across calls on the same stream. */
size_t tcgnn_workspace_bytes(const tcgnn_plan* plan, int32_t D);

/* ---- the hot path ------------------------------------------------------------------------- */

/* Y[N,D] = A_bin * X.  Replaces TCGNN.forward / TCGNN.backward (TCGNN.cpp:63-86).
 * X, Y: fp32 row-major device arrays [N, D]; Y is fully overwritten (rows without edges = 0).
 * Operands are rounded to a 10-bit mantissa (fp16, per-call power-of-two scaled) exactly as the
 * reference rounds to TF32; products accumulate in fp32 on MFMA. Any D >= 1. */
int tcgnn_spmm(const tcgnn_plan* plan, const float* d_X, float* d_Y, int32_t D,
               void* d_workspace, size_t workspace_bytes, void* stream);

/* f3 - the dense update's element-wise steps fused around the aggregation (the reference runs them as separate torch
 * kernels: F.relu after the layer, main_tcgnn.py:100-139; its backward mask before gnn_conv.py:80):
 *   flags & TCGNN_FUSE_RELU : Y = max(A_bin * X, 0)                      (ReLU epilogue in the kernels' stores)
 *   d_gate != NULL          : X'[r,c] = d_gate[r,c] > 0 ? X[r,c] : 0     (applied while X is staged to fp16: with
 *                             d_gate = the forward output this is the ReLU backward mask on dY).  [N, D] like X.
 * Results are bit-identical to max(tcgnn_spmm(X), 0) and tcgnn_spmm(X * (gate > 0)). */
#define TCGNN_FUSE_RELU 1
int tcgnn_spmm_fused(const tcgnn_plan* plan, const float* d_X, const float* d_gate, float* d_Y, int32_t D,
                     int32_t flags, void* d_workspace, size_t workspace_bytes, void* stream);

/* The GCN layer's degree normalisation and bias fused around the aggregation (DGL GraphConv, norm='both' / 'right' / 'left', bias):
 *   Y[r, :] = act( row_scale[r] * sum_{c in N(r)} col_scale[c] * X'[c, :] + bias[:] )
 *     X'[c, k] = d_gate[c, k] > 0 ? X[c, k] : 0   (d_gate as in tcgnn_spmm_fused)
 *     act = max(., 0) with TCGNN_FUSE_RELU
 * Each of d_col_scale [N], d_gate [N, D], d_row_scale [N] and d_bias [D] may be NULL, which leaves that step out.
 * With all four NULL and flags = 0 this is tcgnn_spmm.
 * Results are bit-identical to the unfused composition in fp32, in this order: Y = tcgnn_spmm(col_scale * X'), Y *= row_scale,
 * Y += bias, ReLU.  The column scale is multiplied in while X is staged (before the power-of-two scale and the rounding: the range
 * guard sees col_scale * X', the matrix actually rounded); the row scale, bias and ReLU are applied where the final kernel stores Y.
 * Same walk as tcgnn_spmm for the plan and width, same workspace (tcgnn_workspace_bytes), no allocation, no synchronisation. */
int tcgnn_spmm_scaled(const tcgnn_plan* plan, const float* d_X, const float* d_col_scale, const float* d_gate,
                      const float* d_row_scale, const float* d_bias, float* d_Y, int32_t D, int32_t flags,
                      void* d_workspace, size_t workspace_bytes, void* stream);

/* f3, the dense update itself: Y[N, D_out] = (A_bin * X) * W in one launch - the GIN order of the reference
 * (gnn_conv.py:92-97: X' = TCGNN.forward(X, ...)[0]; X' = torch.mm(X', weights)), which the harness also uses for a GCN layer that
 * narrows (A (H W) = (A H) W).  X [N, D_in] and W [D_in, D_out] fp32 row-major, D_in, D_out <= 128.  The aggregated rows never
 * leave the chip: each window's 16 x D_in fp32 sums go through LDS into the fp32 matrix pipe (v_mfma_f32_16x16x4_f32 - the exact
 * fp32 products and fp32 accumulation of the torch.mm it replaces) against W, which is read through the caches.  On the
 * LDS-resident kernel a 64-column input is two 32-column passes whose products are added into a zeroed Y (two addends: the
 * result does not depend on their order).  flags: TCGNN_FUSE_RELU (not when the product is accumulated over passes: the call
 * then returns TCGNN_ERR_UNSUPPORTED, as it does for wider matrices, and the caller composes tcgnn_spmm with its own GEMM). */
int tcgnn_spmm_gemm(const tcgnn_plan* plan, const float* d_X, const float* d_W, float* d_Y, int32_t D_in, int32_t D_out, int32_t flags,
                    void* d_workspace, size_t workspace_bytes, void* stream);

/* Pre-staged operand (no counterpart in the reference, which is single-GPU).  The kernels read a scaled fp16 image of X that
 * tcgnn_spmm builds per call inside the workspace.  A caller may build it itself - in a row-sharded run every rank converts
 * only ITS rows and the fp16 image, not fp32 X, crosses the fabric (half the bytes of the all-gather, no staging of the
 * gathered matrix on every rank):
 *   image  = 256-byte header (word 0: bit pattern of max|X| over the WHOLE matrix, e.g. after an all-reduce(MAX) of the
 *            per-rank words) followed by (plan's num_cols + 1) rows of tcgnn_x16_pitch(D) halves, the last row all zero;
 *   tcgnn_stage_absmax : atomicMax of the |X| bit patterns of n elements into *d_word (zero it first);
 *   tcgnn_stage_rows   : `rows` rows of X -> rows + 1 image rows at d_dst (the extra row is zero), scaled by *d_absmax_word
 *                        exactly as tcgnn_spmm would;
 *   tcgnn_spmm_staged  : Y = A_bin * X from such an image (gather walks; results identical to tcgnn_spmm on the same walk).
 *                        Only word 0 of the header is read (a staged image is never "wide": bytes 4 .. 255 are ignored and may hold
 *                        anything).  The image is READ-ONLY to the call: one image may feed several streams or ranks at once. */
int tcgnn_x16_pitch(int32_t D);
/* r06 - the same for the LDS-RESIDENT kernel, so that a row-sharded call keeps the fast walk.  That kernel reads a PLANAR image:
 *   256-byte header (word 0 as above; words 1 .. 63 ZERO) followed by ceil(D / 16) planes of (num_cols + 1) records of 16 halves
 *   (32 bytes): plane p, record r = columns 16 p .. 16 p + 15 of row r; record num_cols of every plane and all padding zero.
 *   tcgnn_spmm_staged_layout : 1 if tcgnn_spmm would run the LDS-resident kernel on this plan at this width and can take a planar
 *                              staged image (builds the width's cell streams if missing: may synchronise `stream` once), else 0 -
 *                              stage row-major;
 *   tcgnn_stage_rows_planar  : `rows` rows of X -> their records in every plane: d_dst = the slice's first record in plane 0,
 *                              plane p lies plane_rows (= num_cols + 1) records further on per plane.  Writes nothing else;
 *   tcgnn_spmm_staged_planar : Y = A_bin * X from such an image on the LDS-resident kernel (results identical to tcgnn_spmm in
 *                              mode 3 on the same matrix); TCGNN_ERR_UNSUPPORTED where tcgnn_spmm_staged_layout says 0.
 * A rank's slice of a plane is contiguous, so the exchange is one all-gather per plane. */
int tcgnn_spmm_staged_layout(const tcgnn_plan* plan, int32_t D, void* stream);
int tcgnn_stage_rows_planar(const float* d_X, int32_t rows, int32_t D, const uint32_t* d_absmax_word, void* d_dst, int64_t plane_rows, void* stream);
int tcgnn_spmm_staged_planar(const tcgnn_plan* plan, const void* d_image, float* d_Y, int32_t D, void* stream);
int tcgnn_stage_absmax(const float* d_X, int64_t n, uint32_t* d_word, void* stream);
int tcgnn_stage_rows(const float* d_X, int32_t rows, int32_t D, const uint32_t* d_absmax_word, void* d_dst, void* stream);
int tcgnn_spmm_staged(const tcgnn_plan* plan, const void* d_image, float* d_Y, int32_t D, void* stream);

/* Y[N,D] = A_val * X with A_val[r,c] = d_edge_val[e] for CSR edge e = (r,c).
 * Replaces TCGNN.forward_AGNN (TCGNN.cpp:93-118); d_edge_val is row 0 of edgeAttention[H,E]. */
int tcgnn_spmm_val(const tcgnn_plan* plan, const float* d_X, const float* d_edge_val, float* d_Y,
                   int32_t D, void* d_workspace, size_t workspace_bytes, void* stream);

/* The edge-valued SpMM for H heads at once (multi-head GAT; no counterpart in the reference, whose n_heads is the constant 1):
 *   Y[:, hF:(h+1)F] = A_val(d_edge_val[h, :]) * X[:, hF:(h+1)F]   for h < H.
 * X and Y are fp32 [N, H F] row-major; d_edge_val is fp32 [H, E] head-major - what tcgnn_gat_softmax writes, the reference's
 * edgeAttention layout.  Works on any plan: on A^T's plan with the values in A^T's order (tcgnn_permute_edge_values per head) it is
 * the gradient with respect to X.  The contract is tcgnn_spmm_val's: Y is fully overwritten (rows without edges: 0); the caller
 * owns the workspace - tcgnn_spmm_heads_workspace_bytes(plan, H, F) bytes, 256-byte aligned - and the call neither allocates nor
 * synchronises (capturable in a HIP graph); a repeated call returns the same bits (fixed-order reductions, no atomics); d_Y is
 * 16-byte aligned.  X is rounded with ONE power-of-two scale and the edge values with ONE scale over all H E of them; the range
 * guard ("Operand range", the edge-valued rule) decides once for the whole call.
 * The library picks its way from the plan and (H, F) alone - tcgnn_plan_last_kernel tells which:
 *   H == 1                                 exactly tcgnn_spmm_val (bit-identical, every walk it has);
 *   F in {8, 16, 24, 32}, canonical CSR, E >= 4, an image below 4 GB
 *                                          "spmm_heads_kernel": one fp16 image of X, one walk of the tile stream per pass of whole
 *                                          heads (at most 4 heads and 64 columns a pass) - one gather feeds every head of the pass;
 *   otherwise                              head by head inside the library, each head a column block of X and Y on the gather
 *                                          walks of tcgnn_spmm_val (one abs-max pass for the whole call); a non-canonical CSR or
 *                                          E < 4: one plain-fp32 CSR launch for all heads.
 * H < 1, F < 1, H F beyond int32 or a null array with N > 0: TCGNN_ERR_INVALID_ARG.  N = 0 or E = 0: TCGNN_OK (Y zeroed where N > 0;
 * d_edge_val may then be NULL).  A workspace too small or misaligned: TCGNN_ERR_WORKSPACE before anything is enqueued. */
size_t tcgnn_spmm_heads_workspace_bytes(const tcgnn_plan* plan, int32_t H, int32_t F);
int tcgnn_spmm_heads(const tcgnn_plan* plan, const float* d_X, const float* d_edge_val, float* d_Y, int32_t H, int32_t F,
                     void* d_workspace, size_t workspace_bytes, void* stream);

/* ef[e] = <X[row(e),:], X[col(e),:]> for every CSR edge.  Replaces TCGNN.forward_ef /
 * TCGNN.backward_ef (TCGNN.cpp:126-150).  d_ef: fp32 [E], fully overwritten. */
int tcgnn_sddmm(const tcgnn_plan* plan, const float* d_X, float* d_ef, int32_t D,
                void* d_workspace, size_t workspace_bytes, void* stream);

/* ef[e] = <X[row(e),:], Z[col(e),:]> for every CSR edge: the SDDMM with two different operands (no counterpart in the reference).
 * It is what the gradient of an edge-weighted aggregation Y = A_val * H with respect to its edge values is, <dY[row e], H[col e]>.
 * X (the window operand, read once per row window) and Z (the gathered operand) are fp32 [N, D]; each is staged as its own fp16
 * image with its own power-of-two scale, so the two may differ in magnitude by any factor.  Same walks as tcgnn_sddmm, chosen by
 * the same rules and switches (tcgnn_plan_last_kernel names them the same way); tcgnn_sddmm2(X, X) equals tcgnn_sddmm(X) bit for bit
 * on every walk - unless the range guard takes X for wide (level >= 2): the single-operand call then patches the edges of the dirty
 * rows behind the MFMA result, this one recomputes every edge in fp32 (another summation order; both hold the contract's bounds).
 * Range guard (level >= 2): when either operand holds elements that lose bits in its image and the product of the two maxima is
 * large enough for that to matter (the rule of "Operand range" with max|X| max|Z| in place of max|X|^2), the WHOLE call is computed
 * in fp32, CSR order, operands rounded like the reference's - decided on the device, no read-back.  That kernel is launched behind
 * every level >= 2 call and returns at once otherwise; when it does the work it takes one wavefront per row, serial over the row's
 * edges (a wide operand is a rare input: correct for any magnitudes, far from fast on a hub row).
 * Workspace: tcgnn_sddmm2_workspace_bytes (two images), 256-byte aligned.  No allocation, no synchronisation. */
size_t tcgnn_sddmm2_workspace_bytes(const tcgnn_plan* plan, int32_t D);
int tcgnn_sddmm2(const tcgnn_plan* plan, const float* d_X, const float* d_Z, float* d_ef, int32_t D,
                 void* d_workspace, size_t workspace_bytes, void* stream);

/* The two-operand SDDMM for H heads at once (multi-head dot-product attention scores; the gradient of tcgnn_spmm_heads with respect
 * to its edge values):
 *   ef[h, e] = <X[row(e), hF:(h+1)F], Z[col(e), hF:(h+1)F]>   for h < H and every CSR edge e.
 * X (the window operand) and Z (the gathered operand) are fp32 [N, H F] row-major; d_ef is fp32 [H, E] head-major - what
 * tcgnn_gat_softmax writes and tcgnn_spmm_heads reads.  The contract is tcgnn_sddmm2's and tcgnn_spmm_heads': every element of
 * ef[0:H, 0:E] is written and nothing else (scores of row windows the plan was not handed: 0); the caller owns the workspace -
 * tcgnn_sddmm_heads_workspace_bytes(plan, H, F) bytes, 256-byte aligned - and the call neither allocates nor synchronises
 * (capturable in a HIP graph); a repeated call returns the same bits, and so does every walk; X, Z and ef may sit at any 4-byte
 * boundary.  X and Z are each rounded with ONE power-of-two scale over all H F columns, and the range guard (tcgnn_sddmm2's rule on
 * the two headers, with H F terms a score - the conservative count) decides once for the whole call: behind every level >= 2 call,
 * fused or head by head, ONE launch of the fp32 CSR kernel covers all heads and returns at once unless an operand is wide.
 * The library picks its way from the plan and (H, F) alone - tcgnn_plan_last_kernel tells which:
 *   H == 1                                 exactly tcgnn_sddmm2 (bit-identical, every walk it has);
 *   H >= 2, F in {8, 16, 32, 64}, H F <= 128, canonical CSR with row windows, E >= 4, an image below 4 GB
 *                                          "sddmm_heads_kernel" (with tcgnn_sddmm2's suffix for the walk): each operand staged once,
 *                                          and on tcgnn_sddmm2's walk for H F columns one gather of the neighbour rows feeds the dot
 *                                          products of every head of a pass (at most 4 heads and 128 columns a pass);
 *   a non-canonical CSR or E < 4           one plain-fp32 CSR launch for all heads;
 *   otherwise                              head by head inside the library, each head a column block of X and Z on tcgnn_sddmm2's
 *                                          walks for F columns (one abs-max pass per operand for the whole call; F > 128:
 *                                          "sddmm_wide_kernel").
 * H < 1, F < 1, H F beyond int32 or a null array with E > 0: TCGNN_ERR_INVALID_ARG.  N = 0 or E = 0: TCGNN_OK.  A workspace too
 * small or misaligned: TCGNN_ERR_WORKSPACE before anything is enqueued. */
size_t tcgnn_sddmm_heads_workspace_bytes(const tcgnn_plan* plan, int32_t H, int32_t F);
int tcgnn_sddmm_heads(const tcgnn_plan* plan, const float* d_X, const float* d_Z, float* d_ef, int32_t H, int32_t F,
                      void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- softmax over a node's incoming edges (DGL's edge_softmax; no counterpart in the reference) ------------------------------
 *
 * A row is the segment nodePointer[r] .. nodePointer[r + 1] of the edge array (softmax by destination node).  Planless, like
 * tcgnn_permute_edge_values: device pointers, the caller's stream, no allocation, no synchronisation (capturable in a HIP graph).
 *   forward   p[e]  = exp(b s[e] - m_r) / sum_{e' in row r} exp(b s[e'] - m_r),  m_r = max over row r of b s;
 *             b = *d_beta, a DEVICE scalar (NULL: 1).  The maximum is always subtracted: scores of any magnitude are safe.
 *   backward  g[e]  = p[e] (dp[e] - sum_{row} p dp);  ds[e] = b g[e];  *d_dbeta = sum_e s[e] g[e]
 *             d_dbeta (a device scalar) may be NULL; when given, d_score must be too, and d_scratch must hold
 *             tcgnn_edge_softmax_workspace_bytes(num_nodes, num_edges) bytes (one fp64 partial per workgroup, 8-byte aligned).
 * Results are bit-identical on repetition: every sum is a fixed-order reduction, none uses atomics.  d_p may alias d_score and d_ds
 * may alias d_dp.  Empty rows touch nothing; num_edges = 0 or num_nodes = 0 returns TCGNN_OK (and zeroes *d_dbeta).  Row pointers
 * are clamped to [0, num_edges] and a descending pair counts as an empty row: nothing outside [0, num_edges) is ever written. */
size_t tcgnn_edge_softmax_workspace_bytes(int32_t num_nodes, int64_t num_edges);
int tcgnn_edge_softmax(const int32_t* d_nodePointer, int32_t num_nodes, int64_t num_edges, const float* d_score,
                       const float* d_beta, float* d_p, void* stream);
int tcgnn_edge_softmax_backward(const int32_t* d_nodePointer, int32_t num_nodes, int64_t num_edges, const float* d_p,
                                const float* d_dp, const float* d_score, const float* d_beta, float* d_ds, float* d_dbeta,
                                void* d_scratch, size_t scratch_bytes, void* stream);

/* ---- multi-head GAT attention (DGL's GATConv scores; no counterpart in the reference, whose n_heads is the constant 1) ----------
 *
 * CSR row = destination node, column = source node.  H = num_heads.  Per-node terms d_el (source side, read at col(e)) and d_er
 * (destination side, read at row(e)) are fp32 [num_nodes, H] row-major; per-edge arrays are head-major [H, num_edges] - the
 * reference's edgeAttention layout, so a head's row is what tcgnn_spmm_val takes.  Planless like tcgnn_edge_softmax: device pointers,
 * the caller's stream, no allocation, no synchronisation (capturable in a HIP graph); bit-identical on repetition (fixed-order
 * reductions, no atomics).
 *   tcgnn_gat_softmax           s[h,e] = lrelu(fl32(el[col e, h] + er[row e, h])), lrelu(x) = x > 0 ? x : fl32(x * negative_slope);
 *                               p[h,.] = softmax of s[h,.] over every CSR row, the maximum always subtracted.  The scores never reach
 *                               memory; each is rounded to fp32 before the maximum is subtracted (p is the softmax of the score a
 *                               composition of separate operators would form).
 *   tcgnn_gat_softmax_backward  g = p (dp - sum_row p dp);  ds[h,e] = g * (raw > 0 ? 1 : negative_slope), raw recomputed from el / er;
 *                               d_er[r,h] = sum_{e in row r} ds[h,e] in the same kernel: EVERY row is written, an empty one with 0.
 *                               d_ds may alias d_dp.
 *   tcgnn_edge_colsum           out[c,h] = sum_{eT in row c of A^T} val[h, perm[eT]]: the per-source-node sum of per-edge values given
 *                               in A's order; d_nodePointer_t and d_perm are what tcgnn_transpose_ws wrote.  With val = ds: d_el.
 * Row pointers are clamped to [0, num_edges] and a descending pair is an empty row.  For every read they index, a column id is clamped to
 * the nearer end of [0, num_nodes) and a perm entry outside [0, num_edges) reads position 0 (as tcgnn_permute_edge_values does): safe
 * reads either way, values of no meaning for an array that holds such entries.  Nothing outside [0, num_edges) of a head's row of p / ds, or outside
 * [0, num_nodes * H) of d_er / out, is written.  num_edges = 0 or num_nodes = 0 returns TCGNN_OK (d_er / out zeroed where
 * num_nodes > 0 and the pointer is given); H < 1, a negative size or a null array otherwise: TCGNN_ERR_INVALID_ARG. */
int tcgnn_gat_softmax(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges,
                      int32_t num_heads, const float* d_el, const float* d_er, float negative_slope, float* d_p, void* stream);
int tcgnn_gat_softmax_backward(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges,
                               int32_t num_heads, const float* d_el, const float* d_er, float negative_slope, const float* d_p,
                               const float* d_dp, float* d_ds, float* d_der, void* stream);
int tcgnn_edge_colsum(const int32_t* d_nodePointer_t, const int32_t* d_perm, int32_t num_nodes, int64_t num_edges,
                      int32_t num_heads, const float* d_val, float* d_out, void* stream);

/* ---- element-wise maximum over a node's incoming edges (GraphSAGE's max / pool aggregation; no counterpart in the reference) ----
 *
 * CSR row = destination node, column = source node; X, Y, dY, dX are fp32 [num_nodes, D] row-major, arg is int32 [num_nodes, D].
 * Planless like tcgnn_edge_softmax: device pointers, the caller's stream, no allocation, no synchronisation (capturable in a HIP
 * graph); no atomics and every order fixed: bit-identical on repetition.  X is read as fp32 - no fp16 image, no range guard: the
 * forward is EXACT.
 *   tcgnn_segment_max           the winner of two (value, CSR position) pairs is the greater value; among equal values (-0.0 == +0.0)
 *                               the smaller position; a NaN beats every number, among NaNs the smaller position wins - numpy.argmax over
 *                               the row's slice.  Y[i,d] has the BITS of X[col(arg[i,d]), d] (sign of zero, NaN payload).  Duplicate
 *                               column ids in a row are distinct positions.  An empty row: Y = 0, arg = -1.  d_arg may be NULL.
 *   tcgnn_segment_max_backward  the gradient with respect to X over the rows of A^T: d_nodePointer_t, d_edgeList_t and d_perm are what
 *                               tcgnn_transpose_ws wrote.  fp64 sums, rounded once.  A source node nobody chose: 0.
 * Rows are read with 16-byte loads when D % 4 == 0 and the base address (d_X; d_arg in backward) is 16-byte aligned, with 4-byte loads
 * otherwise: the same results either way.  Row pointers are clamped to [0, num_edges] and a descending pair is an empty row.  For
 * every read they index, a column id is clamped to the nearer end of [0, num_nodes) and a perm entry outside [0, num_edges) reads
 * position 0: safe reads either way, values of no meaning for an array that holds such entries.  Nothing outside [0, num_nodes * D) of
 * Y / arg / dX is written, and every element of them is.  num_nodes = 0, num_edges = 0 or D = 0 returns TCGNN_OK (Y / dX zeroed and
 * arg set to -1 where they have elements and the pointer is given); a negative size, num_edges >= 2^31 or a null array otherwise:
 * TCGNN_ERR_INVALID_ARG before anything is written. */
/* Y[i,d] = max over e in row i of X[col(e), d];  arg[i,d] = the CSR position e that supplied it (-1 and Y = 0 for an empty row) */
int tcgnn_segment_max(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges,
                      const float* d_X, int32_t D, float* d_Y, int32_t* d_arg /* may be NULL */, void* stream);
/* dX[j,d] = sum over eT in row j of A^T, in a fixed order, of dY[i,d] where i = edgeList_t[eT] and arg[i,d] == perm[eT] */
int tcgnn_segment_max_backward(const int32_t* d_nodePointer_t, const int32_t* d_edgeList_t, const int32_t* d_perm,
                               int32_t num_nodes, int64_t num_edges, const int32_t* d_arg, const float* d_dY, int32_t D,
                               float* d_dX, void* stream);

/* ---- mean, standard deviation, maximum and minimum over a node's incoming edges in one walk (PNA's aggregators; no counterpart in
 * the reference) ----
 *
 * The conventions of tcgnn_segment_max: the same arrays, clamps, alignment rule (d_X; in backward d_a, d_b, d_argmax and d_argmin,
 * as far as they are given), degenerate sizes and refusals.  One gather of every neighbour row feeds all the outputs that are given.
 *   tcgnn_segment_stats           for a row i with k > 0 edges and x_e = X[col(e), d]:  mean = sum x_e / k;  std = sqrt(max(var, 0) + eps)
 *                                 with var the population variance (divided by k);  max / argmax exactly tcgnn_segment_max's;  min /
 *                                 argmin the mirror image (numpy.argmin: the smaller value, among equal values the smaller position, a NaN
 *                                 beats every number, among NaNs the first).  A row without edges: +0 in all four value outputs - std
 *                                 included - and -1 in both args.  Any output may be NULL: nothing is computed or written for it;
 *                                 d_argmax without d_max, d_argmin without d_min or no output at all is TCGNN_ERR_INVALID_ARG.
 *                                 The moments are fp64 sums of t = x_e - s and t^2 from the fp32 inputs, s = X[col(rowptr[i]), d] the row's
 *                                 first neighbour:  mean = s + S1 / k,  var = S2 / k - (S1 / k)^2, each rounded to fp32 once.
 *   tcgnn_segment_stats_backward  over the rows of A^T (what tcgnn_transpose_ws wrote), with i = edgeList_t[eT] and e = perm[eT]:
 *                                 dZ[j,d] = sum over eT in row j of  a[i,d] + b[i,d] Z[j,d] + [argmax[i,d] == e] dmax[i,d]
 *                                                                    + [argmin[i,d] == e] dmin[i,d],
 *                                 the terms formed and summed in fp64 in a fixed order, rounded once.  The caller folds the gradients of
 *                                 mean and std into a and b per destination row (k > 0):  b = d_std / (k std),  a = d_mean / k - b mean.
 *                                 Nullable groups: d_a;  d_b with d_Z;  d_argmax with d_dmax;  d_argmin with d_dmin - half of a group is
 *                                 TCGNN_ERR_INVALID_ARG; with every group NULL dZ is zeroed.  dmax / dmin are read only where the arg
 *                                 names the edge. */
int tcgnn_segment_stats(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges,
                        const float* d_X, int32_t D, float eps,
                        float* d_mean, float* d_std, float* d_max, int32_t* d_argmax, float* d_min, int32_t* d_argmin, void* stream);
int tcgnn_segment_stats_backward(const int32_t* d_nodePointer_t, const int32_t* d_edgeList_t, const int32_t* d_perm,
                                 int32_t num_nodes, int64_t num_edges, const float* d_Z,
                                 const float* d_a, const float* d_b,
                                 const int32_t* d_argmax, const float* d_dmax, const int32_t* d_argmin, const float* d_dmin,
                                 int32_t D, float* d_dZ, void* stream);

/* ---- GATv2 attention (Brody et al.; DGL's / PyG's GATv2Conv; no counterpart in the reference) -------------------------------------
 *
 * CSR row = destination node, column = source node.  d_xl (read at col(e)) and d_xr (read at row(e)) are fp32 [num_nodes, H F]
 * row-major and may be the same pointer; d_attn is fp32 [H, F]; per-edge arrays are head-major [H, num_edges] (a head's row is what
 * tcgnn_spmm_heads takes).  Planless like tcgnn_gat_softmax: device pointers, the caller's stream, no allocation, no synchronisation
 * (capturable in a HIP graph); no atomics and every reduction order fixed: bit-identical on repetition.  Everything is read as fp32 -
 * no fp16 image, no range guard.  Any H >= 1 and F >= 1.
 *   the activation term  z = fl32(xl[col e, hF+f] + xr[row e, hF+f]);  l = z > 0 ? z : fl32(z * negative_slope) - GAT's two roundings,
 *                        the product contracted with nothing.
 *   tcgnn_gatv2_softmax           s[h,e] = fl32(sum_f (double)attn[h,f] * (double)l): exact fp64 products, an fp64 sum in a fixed order,
 *                                 rounded once; every neighbour row is gathered once and every score formed once.  p[h,.] = softmax of
 *                                 those rounded scores over every CSR row, the maximum always subtracted - the exponential, the fp64 row sum
 *                                 and the fp64 quotient are tcgnn_edge_softmax's with beta = 1.  The scores are parked in their slots of
 *                                 d_p and normalised in place in the same launch.  d_score (may be NULL) receives the rounded scores; d_p
 *                                 is bit-identical with and without it.
 *   tcgnn_gatv2_softmax_backward  g = p * (float)((double)dp - sum_row p dp), the dot product in fp64 and fixed order, as
 *                                 tcgnn_gat_softmax_backward forms it; d_g may alias d_dp.  With c = z > 0 ? attn[h,f] : fl32(attn[h,f] *
 *                                 negative_slope):  d_dxr[i, hF+f] = fl32(sum_{e in row i} (double)fl32(g[h,e] * c)) - EVERY row is
 *                                 written, an empty one with 0;  d_dattn[h,f] = fl32(sum_e (double)g[h,e] * (double)l), each workgroup's
 *                                 fp64 partials in d_scratch (tcgnn_gatv2_workspace_bytes bytes, 8-byte aligned), added in workgroup order
 *                                 by a second small launch.
 *   tcgnn_gatv2_source_grad       over the rows of A^T (d_nodePointer_t, d_edgeList_t, d_perm: what tcgnn_transpose_ws wrote):
 *                                 d_dxl[j, hF+f] = fl32(sum_{eT in row j} (double)fl32(g[h, perm eT] * c)), z = fl32(xl[j] + xr[col_t eT]);
 *                                 a source nobody reads gets 0.
 * Rows are read with 16-byte loads when F % 4 == 0 and d_xl, d_xr and d_attn are 16-byte aligned, with 4-byte loads otherwise: the
 * same bits either way.  Row pointers are clamped to [0, num_edges] and a descending pair is an empty row.  For every read they index,
 * a column id is clamped to the nearer end of [0, num_nodes) and a perm entry outside [0, num_edges) reads position 0: safe reads
 * either way, values of no meaning for an array that holds such entries.  Nothing outside [0, num_edges) of a head's row of p / score /
 * g and nothing outside [0, num_nodes * H * F) of the node arrays is written.  num_nodes = 0 or num_edges = 0 returns TCGNN_OK (d_dxr /
 * d_dxl / d_dattn zeroed where they have elements and the pointer is given); H < 1, F < 1, a negative size, num_edges >= 2^31 or a null
 * array where one is needed: TCGNN_ERR_INVALID_ARG before anything is written; a scratch buffer too small: TCGNN_ERR_WORKSPACE.  A hub
 * row stays on one workgroup, as in tcgnn_edge_softmax and tcgnn_gat_softmax. */
size_t tcgnn_gatv2_workspace_bytes(int32_t num_nodes, int64_t num_edges, int32_t H, int32_t F);
int tcgnn_gatv2_softmax(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges, int32_t H,
                        int32_t F, const float* d_xl, const float* d_xr, const float* d_attn, float negative_slope,
                        float* d_score /* may be NULL */, float* d_p, void* stream);
int tcgnn_gatv2_softmax_backward(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges,
                                 int32_t H, int32_t F, const float* d_xl, const float* d_xr, const float* d_attn,
                                 float negative_slope, const float* d_p, const float* d_dp, float* d_g, float* d_dxr,
                                 float* d_dattn, void* d_scratch, size_t scratch_bytes, void* stream);
int tcgnn_gatv2_source_grad(const int32_t* d_nodePointer_t, const int32_t* d_edgeList_t, const int32_t* d_perm, int32_t num_nodes,
                            int64_t num_edges, int32_t H, int32_t F, const float* d_xl, const float* d_xr, const float* d_attn,
                            float negative_slope, const float* d_g, float* d_dxl, void* stream);

/* ---- message passing with a feature vector per edge (DGL's u_add_e / sum and copy_e / sum, the message of PyG's GINEConv; no
 * counterpart in the reference) ----
 *
 * CSR row = destination node, column = source node.  X, Y and dY are fp32 [num_nodes, D] row-major; Ef, dM and M are fp32
 * [num_edges, D] row-major in CSR POSITION order, the order of every other per-edge array of this header.  act: TCGNN_ACT_IDENTITY or
 * TCGNN_ACT_RELU.  Planless like tcgnn_segment_max: device pointers, the caller's stream, no allocation, no synchronisation
 * (capturable in a HIP graph); no atomics and every order fixed: bit-identical on repetition.  Everything is read as fp32 - no fp16
 * image, no range guard.
 *   tcgnn_edge_message           z = fl32(X[col(e), d] + Ef[e, d]);  m = act(z);  Y[i, d] = fl32(sum over e in row i of (double)m), an
 *                                fp64 sum in a fixed order, rounded once; an empty row: 0.  ReLU as torch.relu: a NaN z stays NaN.
 *   tcgnn_edge_message_backward  dM[e, d] = dY[row(e), d] where act is the identity or !(z <= 0) - torch's threshold_backward: a NaN z
 *                                passes the gradient, -0.0 and +0.0 block it - and +0.0 otherwise.  EXACT: the bits of dY or zero.
 *                                dM is the gradient with respect to Ef and the per-edge gradient of the message: the gradient with
 *                                respect to X is tcgnn_edge_sum over A^T through perm.  With TCGNN_ACT_IDENTITY d_edgeList, d_X and
 *                                d_Ef are not read and may be NULL.  A position in front of nodePointer[0] or behind
 *                                nodePointer[num_nodes] (a canonical CSR has none) belongs to no row: its row of dM is zeroed.
 *   tcgnn_edge_sum               Y[r, d] = fl32(sum over the positions t of row r of (double)M[perm ? perm[t] : t, d]), an fp64 sum in a
 *                                fixed order, rounded once; an empty row: 0.  With d_nodePointer_t and d_perm of tcgnn_transpose_ws:
 *                                the sum of M's rows by SOURCE node; with d_perm = NULL: by destination node (copy_e / sum).
 * Rows are read and written with 16-byte accesses when D % 4 == 0 and every [., D] array the call touches is 16-byte aligned, with
 * 4-byte accesses otherwise: the same bits either way.  Row pointers are clamped to [0, num_edges] and a descending pair is an empty
 * row.  For every read they index, a column id is clamped to the nearer end of [0, num_nodes) and a perm entry outside [0, num_edges)
 * reads position 0: safe reads either way, values of no meaning for an array that holds such entries.  Every element of Y / dM is
 * written and nothing outside it.  A size of 0 returns TCGNN_OK with the output, where it has elements, zeroed; a negative size,
 * num_edges >= 2^31, an unknown act or a null array otherwise: TCGNN_ERR_INVALID_ARG before anything is written.  A hub row stays on
 * one workgroup, as in tcgnn_segment_max. */
#define TCGNN_ACT_IDENTITY 0
#define TCGNN_ACT_RELU 1
int tcgnn_edge_message(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges,
                       const float* d_X, const float* d_Ef, int32_t D, int32_t act, float* d_Y, void* stream);
int tcgnn_edge_message_backward(const int32_t* d_nodePointer, const int32_t* d_edgeList, int32_t num_nodes, int64_t num_edges,
                                const float* d_X, const float* d_Ef, const float* d_dY, int32_t D, int32_t act, float* d_dM,
                                void* stream);
int tcgnn_edge_sum(const int32_t* d_nodePointer, const int32_t* d_perm /* may be NULL */, int32_t num_nodes, int64_t num_edges,
                   const float* d_M, int32_t D, float* d_Y, void* stream);

/* ---- fused AGNN layer products (one gather of the neighbour rows feeds both) ----------------
 *
 * The reference's AGNN layer (gnn_conv.py:115-158) calls forward_ef and forward_AGNN back to back on
 * the same matrix, and again in backward; each call gathers every neighbour row once.  These two
 * entry points compute the same results with ONE pass over the tile stream.
 *
 * forward:   ef[e] = <X[row e], X[col e]>                         (= tcgnn_sddmm)
 *            Y     = A_att * X,  att[e] = fl32(w * ef[e])          (= tcgnn_spmm_val on w * ef)
 *            d_ef_absmax: 1 + N device words the caller allocates - word 0 = bit pattern of max |ef|, words 1 .. N = the power-of-two
 *            exponent each row's edge weights were scaled by (r05: one fp16 scale per ROW of A, so that small rows of a matrix whose
 *            weights spread over 2^30 and more keep their mantissas) - consumed by the backward call
 * backward:  G     = A_att * dY, att[e] = fl32(w * ef[e]) with the saved ef   (gnn_conv.py:143)
 *            *d_dw = sum_e <dY[row e], dY[col e]> * (float)col(e)             (gnn_conv.py:150-153:
 *                    the reference's d_attention_w, mm(backward_ef(dY)[None,:], column_index[:,None].float()))
 * d_w is the attention weight as a DEVICE scalar (no host read-back).  Rounding is the same as in
 * the separate calls (10-bit mantissa operands, fp32 accumulate); the power-of-two scale of row r's att comes
 * from a bound (|w| D max|x_r| max|X|) instead of a pass over E, so results equal the separate calls bit for bit unless an
 * edge weight is more than 2^-20 below its row's bound (a row whose neighbours' magnitudes spread that far).  d_dw is a fixed-order reduction (deterministic).
 * Supported for canonical plans (sorted, duplicate-free rows), D <= 128, E >= 8:
 * tcgnn_agnn_supported() tells; otherwise the calls return TCGNN_ERR_UNSUPPORTED and the caller
 * uses the three separate entry points. */
int tcgnn_agnn_supported(const tcgnn_plan* plan, int32_t D);
/* (r06, ADVICE r05: these two replace r04 / r05's tcgnn_agnn_forward / tcgnn_agnn_backward, whose d_ef_absmax grew from 1 word to 1 + N
 *  words in r05 under an unchanged signature - a caller built against the older header would have been written 4 N bytes past its word.
 *  The names are gone, so such a caller fails to resolve them; the new ones take the element count of d_ef_absmax and return
 *  TCGNN_ERR_INVALID_ARG when it is below 1 + N.) */
int tcgnn_agnn_pair_forward(const tcgnn_plan* plan, const float* d_X, const float* d_w, float* d_ef,
                            uint32_t* d_ef_absmax, int64_t ef_absmax_words, float* d_Y, int32_t D, void* d_workspace,
                            size_t workspace_bytes, void* stream);
int tcgnn_agnn_pair_backward(const tcgnn_plan* plan, const float* d_dY, const float* d_w, const float* d_ef,
                             const uint32_t* d_ef_absmax, int64_t ef_absmax_words, float* d_G, float* d_dw, int32_t D,
                             void* d_workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TCGNN_H */
