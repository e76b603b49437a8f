// TCGNN_binding.cpp - the pybind11 torch extension INTEGRATION.md section B describes, complete and compiled.
//
// What a maintainer of the reference would keep of TCGNN_conv/TCGNN.cpp: the module (same seven names, TCGNN.cpp:260-272), the
// torch-typed wrappers with their CHECK_INPUT lines (TCGNN.cpp:54-56, :63-150, :172-256) - and nothing else.  The bodies that
// called the *_cuda launchers of TCGNN_kernel.cu (declared at TCGNN.cpp:13-52) call the C ABI of include/tcgnn.h instead;
// TCGNN_kernel.cu, nvcc and thrust are gone.  Built by integration/setup.py as a plain CppExtension (no .cu file, so torch's
// hipify step never runs) that links libtcgnn_hip.so.  tests/test_binding.py drives the three kernels through THIS module
// as a second backend next to the ctypes one (tc-gnn_atc23_amd/TCGNN.py).
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <c10/core/DeviceGuard.h>
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <list>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include <tcgnn.h>

#define CHECK_CUDA(x) TORCH_CHECK(x.is_cuda(), #x " must be a CUDA tensor")            // TCGNN.cpp:54
#define CHECK_CONTIGUOUS(x) TORCH_CHECK(x.is_contiguous(), #x " must be contiguous")   // TCGNN.cpp:55
#define CHECK_INPUT(x) CHECK_CUDA(x); CHECK_CONTIGUOUS(x)                              // TCGNN.cpp:56

namespace {

void tcgnn_check(int st, const char* what) {
  TORCH_CHECK(st == TCGNN_OK, what, " failed: ", tcgnn_status_string(st), " (", tcgnn_last_error(), ")");
}

void* current_stream(const torch::Tensor& t) { return c10::hip::getCurrentHIPStream(t.get_device()).stream(); }

// the extension works on the device its tensors live on, not on whatever device happens to be current (plan allocations and
// kernel launches follow the current device) - what torch's own operators do with a device guard (r2 ADVICE)
using DeviceGuard = c10::DeviceGuard;   // (dispatches to the HIP guard registered for "cuda" tensors on ROCm)

// X must hold one row per node of the graph: a shorter matrix would be read out of bounds by the staging pass and the gathers
// (the reference indexes input by the same row ids, TCGNN_kernel.cu:417-427, without a check)
void check_rows(const torch::Tensor& input, const torch::Tensor& nodePointer) {
  TORCH_CHECK(input.dim() == 2, "input must be a 2-D [num_nodes, dim] matrix");
  TORCH_CHECK(nodePointer.numel() >= 1 && input.size(0) == nodePointer.numel() - 1, "input has ", input.size(0), " rows, the graph has ",
              nodePointer.numel() - 1, " nodes");
}

// One plan per graph.  The reference hands the same five tensors to every call (gnn_conv.py:31,56), so the packed tile stream
// is built at first sight and found again by (address, length, in-place version) of each; the entry keeps the tensors alive,
// so an address cannot be recycled under it.
// Not in the reference: what transpose=True calls run on (A^T's CSR, metadata and plan - or A's own plan on a symmetric graph - and
// the permutation of the edge positions), built at first use and kept in A's entry, so it leaves the cache with A's plan.
struct TransposedEntry {
  bool built = false, symmetric = false;
  std::vector<torch::Tensor> keep;   // A^T's five metadata tensors (not symmetric)
  torch::Tensor perm;
  tcgnn_plan* own = nullptr;         // A^T's plan when the graph is not symmetric
};

struct PlanEntry {
  std::vector<std::tuple<const void*, int64_t, int64_t>> key;
  std::vector<torch::Tensor> keep;
  tcgnn_plan* plan = nullptr;
  TransposedEntry t;
};
std::list<PlanEntry>& plan_cache() { static std::list<PlanEntry> c; return c; }
constexpr size_t kPlanCacheSize = 8;

void destroy_entry(PlanEntry& e) {
  tcgnn_plan_destroy(e.plan);
  if (e.t.own) tcgnn_plan_destroy(e.t.own);
}

PlanEntry& entry_for(const torch::Tensor& nodePointer, const torch::Tensor& edgeList, const torch::Tensor& blockPartition,
                     const torch::Tensor& edgeToColumn, const torch::Tensor& edgeToRow) {
  const torch::Tensor* ts[5] = {&nodePointer, &edgeList, &blockPartition, &edgeToColumn, &edgeToRow};
  std::vector<std::tuple<const void*, int64_t, int64_t>> key;
  for (auto* t : ts) key.emplace_back(t->data_ptr(), t->numel(), (int64_t)t->_version());
  auto& cache = plan_cache();
  for (auto it = cache.begin(); it != cache.end(); ++it)
    if (it->key == key) { cache.splice(cache.begin(), cache, it); return cache.front(); }
  for (auto* t : ts) TORCH_CHECK(t->scalar_type() == torch::kInt32, "expected scalar type Int");   // what data_ptr<int>() raises in the reference
  TORCH_CHECK(edgeToColumn.numel() >= edgeList.numel() && edgeToRow.numel() >= edgeList.numel(), "edgeToColumn / edgeToRow are shorter than edgeList");
  PlanEntry e;
  e.key = key;
  for (auto* t : ts) e.keep.push_back(*t);
  tcgnn_check(tcgnn_plan_create(nodePointer.data_ptr<int>(), edgeList.data_ptr<int>(), blockPartition.data_ptr<int>(),
                                edgeToColumn.data_ptr<int>(), edgeToRow.data_ptr<int>(), (int32_t)(nodePointer.size(0) - 1),
                                edgeList.size(0), (int32_t)blockPartition.size(0), current_stream(nodePointer), &e.plan),
              "tcgnn_plan_create");
  cache.push_front(std::move(e));
  while (cache.size() > kPlanCacheSize) {
    (void)hipDeviceSynchronize();   // kernels still reading the evicted plan - on ANY stream - finish first
    destroy_entry(cache.back());
    cache.pop_back();
  }
  return cache.front();
}

tcgnn_plan* plan_for(const torch::Tensor& nodePointer, const torch::Tensor& edgeList, const torch::Tensor& blockPartition,
                     const torch::Tensor& edgeToColumn, const torch::Tensor& edgeToRow) {
  return entry_for(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow).plan;
}

torch::Tensor aligned_scratch(size_t bytes, const torch::Tensor& like, void** ptr) {
  torch::Tensor buf = torch::empty({(int64_t)bytes + 256}, like.options().dtype(torch::kUInt8));
  *ptr = reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(buf.data_ptr()) + 255) & ~(uintptr_t)255);
  return buf;
}

// A^T's CSR, one per (nodePointer, edgeList): tcgnn_transpose_ws at first sight, then cached.  edge_colsum sums over it and
// transposed_for builds A^T's plan from it, so a graph is transposed once and holds one perm.
struct TransposedCsr {
  std::vector<std::tuple<const void*, int64_t, int64_t>> key;
  torch::Tensor nodePointer, edgeList, rp_t, col_t, perm;
  bool symmetric = false;
};
std::list<TransposedCsr>& csr_cache() { static std::list<TransposedCsr> c; return c; }

TransposedCsr& transposed_csr(const torch::Tensor& nodePointer, const torch::Tensor& edgeList) {
  std::vector<std::tuple<const void*, int64_t, int64_t>> key;
  for (auto* t : {&nodePointer, &edgeList}) key.emplace_back(t->data_ptr(), t->numel(), (int64_t)t->_version());
  auto& cache = csr_cache();
  for (auto it = cache.begin(); it != cache.end(); ++it)
    if (it->key == key) { cache.splice(cache.begin(), cache, it); return cache.front(); }
  const int32_t N = (int32_t)(nodePointer.numel() - 1);
  const int64_t E = edgeList.numel();
  auto opts = nodePointer.options().dtype(torch::kInt32);
  TransposedCsr c;
  c.key = key;
  c.nodePointer = nodePointer;
  c.edgeList = edgeList;
  c.rp_t = torch::empty({(int64_t)N + 1}, opts);
  c.perm = torch::empty({E}, opts);
  c.col_t = torch::empty({E}, opts);
  int32_t sym = 0;
  size_t need = 0;
  void* ws = nullptr;
  tcgnn_check(tcgnn_transpose_workspace_bytes(N, E, &need), "tcgnn_transpose_workspace_bytes");
  torch::Tensor buf = aligned_scratch(need, nodePointer, &ws);
  tcgnn_check(tcgnn_transpose_ws(nodePointer.data_ptr<int>(), edgeList.data_ptr<int>(), N, E, c.rp_t.data_ptr<int>(), c.col_t.data_ptr<int>(),
                                 c.perm.data_ptr<int>(), ws, need, &sym, current_stream(nodePointer)), "tcgnn_transpose_ws");
  c.symmetric = sym != 0;
  if (c.symmetric) { c.rp_t = nodePointer; c.col_t = edgeList; }   // A^T = A: its arrays are A's own
  cache.push_front(std::move(c));
  while (cache.size() > kPlanCacheSize) cache.pop_back();   // (tcgnn_transpose_ws synchronised; torch's allocator orders the reuse of the rest)
  return cache.front();
}

// A^T of the entry's graph: its CSR from csr_cache(), then (not symmetric) the device SGT of A^T and its plan - as TCGNN.py does
TransposedEntry& transposed_for(PlanEntry& e) {
  TransposedEntry& t = e.t;
  if (t.built) return t;
  const torch::Tensor& nodePointer = e.keep[0];
  const TransposedCsr& c = transposed_csr(nodePointer, e.keep[1]);
  if (!c.symmetric) {
    const int32_t N = (int32_t)(nodePointer.numel() - 1);
    const int64_t E = e.keep[1].numel(), bp_len = e.keep[2].numel();
    auto opts = nodePointer.options().dtype(torch::kInt32);
    torch::Tensor bp_t = torch::zeros({bp_len}, opts), e2c_t = torch::empty({E}, opts), e2r_t = torch::empty({E}, opts);
    size_t need = 0;
    void* ws = nullptr;
    tcgnn_check(tcgnn_preprocess_gpu_workspace_bytes(N, E, TCGNN_BLK_H, &need), "tcgnn_preprocess_gpu_workspace_bytes");
    int64_t tc_blocks = 0;
    {
      torch::Tensor buf = aligned_scratch(need, nodePointer, &ws);
      tcgnn_check(tcgnn_preprocess_gpu_ws(c.col_t.data_ptr<int>(), c.rp_t.data_ptr<int>(), N, E, TCGNN_BLK_H, TCGNN_BLK_W, bp_t.data_ptr<int>(), bp_len,
                                          e2c_t.data_ptr<int>(), e2r_t.data_ptr<int>(), ws, need, &tc_blocks, current_stream(nodePointer)),
                  "tcgnn_preprocess_gpu_ws");
    }
    tcgnn_check(tcgnn_plan_create(c.rp_t.data_ptr<int>(), c.col_t.data_ptr<int>(), bp_t.data_ptr<int>(), e2c_t.data_ptr<int>(), e2r_t.data_ptr<int>(),
                                  N, E, (int32_t)bp_len, current_stream(nodePointer), &t.own), "tcgnn_plan_create");
    t.keep = {c.rp_t, c.col_t, bp_t, e2c_t, e2r_t};
  }
  t.perm = c.perm;   // (the entry holds the tensors it uses: csr_cache() may drop its own reference first)
  t.symmetric = c.symmetric;
  t.built = true;
  return t;
}

// the plan a call runs on: A's, or with transpose the one of A^T (A's own on a symmetric graph)
tcgnn_plan* plan_of(PlanEntry& e, bool transpose) {
  if (!transpose) return e.plan;
  TransposedEntry& t = transposed_for(e);
  return t.own ? t.own : e.plan;
}

struct Workspace {
  torch::Tensor buf;
  char* ptr;
  size_t bytes;
  Workspace(tcgnn_plan* plan, int D, const torch::Tensor& like) {
    const size_t need = tcgnn_workspace_bytes(plan, D);
    buf = torch::empty({(int64_t)need + 256}, like.options().dtype(torch::kUInt8));   // torch's caching allocator: no hipMalloc per call
    ptr = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(buf.data_ptr()) + 255) & ~(uintptr_t)255);
    bytes = (size_t)buf.numel() - (size_t)(ptr - static_cast<char*>(buf.data_ptr()));
  }
};

}  // namespace

// TCGNN.cpp:63-86 (transpose, not in the reference: A^T @ input, the metadata still describing A)
std::vector<torch::Tensor> spmm_forward(torch::Tensor input, torch::Tensor nodePointer, torch::Tensor edgeList,
                                        torch::Tensor blockPartition, torch::Tensor edgeToColumn, torch::Tensor edgeToRow, bool transpose) {
  CHECK_INPUT(input); CHECK_INPUT(nodePointer); CHECK_INPUT(edgeList);
  CHECK_INPUT(blockPartition); CHECK_INPUT(edgeToColumn); CHECK_INPUT(edgeToRow);
  TORCH_CHECK(input.scalar_type() == torch::kFloat32, "expected scalar type Float");
  check_rows(input, nodePointer);
  DeviceGuard guard(input.device());
  auto output = torch::empty_like(input);                          // fully overwritten by the kernels (every row is a node's)
  if (input.numel() == 0) return {output};
  auto* plan = plan_of(entry_for(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow), transpose);
  const int D = (int)input.size(1);
  Workspace ws(plan, D, input);
  tcgnn_check(tcgnn_spmm(plan, input.data_ptr<float>(), output.data_ptr<float>(), D, ws.ptr, ws.bytes, current_stream(input)), "tcgnn_spmm");
  return {output};
}

// TCGNN.cpp:93-118 (edgeAttention sits between edgeList and blockPartition, call site gnn_conv.py:132)
std::vector<torch::Tensor> spmm_forward_AGNN(torch::Tensor input, torch::Tensor nodePointer, torch::Tensor edgeList,
                                             torch::Tensor edgeAttention, torch::Tensor blockPartition, torch::Tensor edgeToColumn,
                                             torch::Tensor edgeToRow, bool transpose) {
  CHECK_INPUT(input); CHECK_INPUT(nodePointer); CHECK_INPUT(edgeList); CHECK_INPUT(edgeAttention);
  CHECK_INPUT(blockPartition); CHECK_INPUT(edgeToColumn); CHECK_INPUT(edgeToRow);
  TORCH_CHECK(input.scalar_type() == torch::kFloat32 && edgeAttention.scalar_type() == torch::kFloat32, "expected scalar type Float");
  TORCH_CHECK(edgeAttention.numel() >= edgeList.numel(), "edgeAttention holds fewer values than there are edges");
  check_rows(input, nodePointer);
  DeviceGuard guard(input.device());
  auto output = torch::empty_like(input);
  if (input.numel() == 0) return {output};
  PlanEntry& entry = entry_for(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow);
  auto* plan = plan_of(entry, transpose);
  const int D = (int)input.size(1);
  Workspace ws(plan, D, input);
  // every "head" launch of the reference reads row 0 of edgeAttention and overwrites the same output (TCGNN_kernel.cu:253-268, :529)
  const float* val = edgeAttention.data_ptr<float>();
  torch::Tensor val_t;
  if (transpose) {   // row 0 in A^T's order
    val_t = torch::empty({std::max<int64_t>(edgeList.numel(), 1)}, input.options());
    tcgnn_check(tcgnn_permute_edge_values(val, entry.t.perm.data_ptr<int>(), edgeList.numel(), val_t.data_ptr<float>(), current_stream(input)),
                "tcgnn_permute_edge_values");
    val = val_t.data_ptr<float>();
  }
  tcgnn_check(tcgnn_spmm_val(plan, input.data_ptr<float>(), val, output.data_ptr<float>(), D, ws.ptr, ws.bytes,
                             current_stream(input)), "tcgnn_spmm_val");
  return {output};
}

// Not in the reference: the edge-valued SpMM for every head at once, Y[:, hF:(h+1)F] = A_val(edgeAttention[h]) input[:, hF:(h+1)F]
// (tcgnn_spmm_heads; TCGNN.forward_heads of the ctypes module).  transpose: every head's row permuted into A^T's order, A^T's plan
std::vector<torch::Tensor> spmm_forward_heads(torch::Tensor input, torch::Tensor nodePointer, torch::Tensor edgeList,
                                              torch::Tensor edgeAttention, torch::Tensor blockPartition, torch::Tensor edgeToColumn,
                                              torch::Tensor edgeToRow, int64_t heads, bool transpose) {
  CHECK_INPUT(input); CHECK_INPUT(nodePointer); CHECK_INPUT(edgeList); CHECK_INPUT(edgeAttention);
  CHECK_INPUT(blockPartition); CHECK_INPUT(edgeToColumn); CHECK_INPUT(edgeToRow);
  TORCH_CHECK(input.scalar_type() == torch::kFloat32 && edgeAttention.scalar_type() == torch::kFloat32, "expected scalar type Float");
  check_rows(input, nodePointer);
  const int64_t E = edgeList.numel(), D = input.size(1);
  TORCH_CHECK(heads >= 1 && D % heads == 0, "input has ", D, " columns, which ", heads, " heads do not divide");
  TORCH_CHECK(edgeAttention.dim() == 2 && edgeAttention.size(0) == heads && edgeAttention.size(1) == E && edgeAttention.device() == input.device(),
              "edgeAttention must be [heads, num_edges] on the input's device");
  DeviceGuard guard(input.device());
  auto output = torch::empty_like(input);
  if (input.numel() == 0) return {output};
  PlanEntry& entry = entry_for(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow);
  auto* plan = plan_of(entry, transpose);
  const int H = (int)heads, F = (int)(D / heads);
  void* ws = nullptr;
  const size_t need = tcgnn_spmm_heads_workspace_bytes(plan, H, F);
  torch::Tensor buf = aligned_scratch(need, input, &ws);
  const float* val = edgeAttention.data_ptr<float>();
  torch::Tensor val_t;
  if (transpose) {
    val_t = torch::empty({std::max<int64_t>(heads * E, 1)}, input.options());
    for (int64_t h = 0; h < heads; ++h)
      tcgnn_check(tcgnn_permute_edge_values(val + h * E, entry.t.perm.data_ptr<int>(), E, val_t.data_ptr<float>() + h * E, current_stream(input)),
                  "tcgnn_permute_edge_values");
    val = val_t.data_ptr<float>();
  }
  tcgnn_check(tcgnn_spmm_heads(plan, input.data_ptr<float>(), val, output.data_ptr<float>(), H, F, ws, need, current_stream(input)), "tcgnn_spmm_heads");
  return {output};
}

// TCGNN.cpp:126-150
std::vector<torch::Tensor> sddmm_forward(torch::Tensor input, torch::Tensor nodePointer, torch::Tensor edgeList,
                                         torch::Tensor blockPartition, torch::Tensor edgeToColumn, torch::Tensor edgeToRow) {
  CHECK_INPUT(input); CHECK_INPUT(nodePointer); CHECK_INPUT(edgeList);
  CHECK_INPUT(blockPartition); CHECK_INPUT(edgeToColumn); CHECK_INPUT(edgeToRow);
  TORCH_CHECK(input.scalar_type() == torch::kFloat32, "expected scalar type Float");
  check_rows(input, nodePointer);
  DeviceGuard guard(input.device());
  auto ef = torch::empty({edgeList.size(0)}, input.options());
  if (edgeList.size(0) == 0) return {ef};
  if (input.size(1) == 0) return {ef.zero_()};
  auto* plan = plan_for(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow);
  const int D = (int)input.size(1);
  Workspace ws(plan, D, input);
  tcgnn_check(tcgnn_sddmm(plan, input.data_ptr<float>(), ef.data_ptr<float>(), D, ws.ptr, ws.bytes, current_stream(input)), "tcgnn_sddmm");
  return {ef};
}

// Not in the reference: the SDDMM with two operands, ef[e] = <X[row e], Z[col e]> (tcgnn_sddmm2; TCGNN.forward_ef2 of the ctypes module)
std::vector<torch::Tensor> sddmm2_forward(torch::Tensor X, torch::Tensor Z, torch::Tensor nodePointer, torch::Tensor edgeList,
                                          torch::Tensor blockPartition, torch::Tensor edgeToColumn, torch::Tensor edgeToRow) {
  CHECK_INPUT(X); CHECK_INPUT(Z); CHECK_INPUT(nodePointer); CHECK_INPUT(edgeList);
  CHECK_INPUT(blockPartition); CHECK_INPUT(edgeToColumn); CHECK_INPUT(edgeToRow);
  TORCH_CHECK(X.scalar_type() == torch::kFloat32 && Z.scalar_type() == torch::kFloat32, "expected scalar type Float");
  check_rows(X, nodePointer);
  TORCH_CHECK(Z.sizes() == X.sizes() && Z.device() == X.device(), "Z must have the shape and device of X");
  DeviceGuard guard(X.device());
  auto ef = torch::empty({edgeList.size(0)}, X.options());
  if (edgeList.size(0) == 0) return {ef};
  if (X.size(1) == 0) return {ef.zero_()};
  auto* plan = plan_for(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow);
  const int D = (int)X.size(1);
  void* ws = nullptr;
  const size_t need = tcgnn_sddmm2_workspace_bytes(plan, D);
  torch::Tensor buf = aligned_scratch(need, X, &ws);
  tcgnn_check(tcgnn_sddmm2(plan, X.data_ptr<float>(), Z.data_ptr<float>(), ef.data_ptr<float>(), D, ws, need, current_stream(X)), "tcgnn_sddmm2");
  return {ef};
}

// Not in the reference: the two-operand SDDMM for every head at once, ef[h, e] = <X[row e, hF:(h+1)F], Z[col e, hF:(h+1)F]>, [heads, E]
// (tcgnn_sddmm_heads; TCGNN.forward_ef_heads of the ctypes module)
std::vector<torch::Tensor> sddmm_heads_forward(torch::Tensor X, torch::Tensor Z, torch::Tensor nodePointer, torch::Tensor edgeList,
                                               torch::Tensor blockPartition, torch::Tensor edgeToColumn, torch::Tensor edgeToRow, int64_t heads) {
  CHECK_INPUT(X); CHECK_INPUT(Z); CHECK_INPUT(nodePointer); CHECK_INPUT(edgeList);
  CHECK_INPUT(blockPartition); CHECK_INPUT(edgeToColumn); CHECK_INPUT(edgeToRow);
  TORCH_CHECK(X.scalar_type() == torch::kFloat32 && Z.scalar_type() == torch::kFloat32, "expected scalar type Float");
  check_rows(X, nodePointer);
  TORCH_CHECK(Z.sizes() == X.sizes() && Z.device() == X.device(), "Z must have the shape and device of X");
  const int64_t E = edgeList.numel(), D = X.size(1);
  TORCH_CHECK(heads >= 1 && D % heads == 0, "X has ", D, " columns, which ", heads, " heads do not divide");
  DeviceGuard guard(X.device());
  auto ef = torch::empty({heads, E}, X.options());
  if (E == 0) return {ef};
  if (D == 0) return {ef.zero_()};
  auto* plan = plan_for(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow);
  const int H = (int)heads, F = (int)(D / heads);
  void* ws = nullptr;
  const size_t need = tcgnn_sddmm_heads_workspace_bytes(plan, H, F);
  torch::Tensor buf = aligned_scratch(need, X, &ws);
  tcgnn_check(tcgnn_sddmm_heads(plan, X.data_ptr<float>(), Z.data_ptr<float>(), ef.data_ptr<float>(), H, F, ws, need, current_stream(X)), "tcgnn_sddmm_heads");
  return {ef};
}

namespace {
const float* beta_ptr(const c10::optional<torch::Tensor>& beta, const torch::Tensor& like) {
  if (!beta.has_value()) return nullptr;
  TORCH_CHECK(beta->is_cuda() && beta->is_contiguous() && beta->scalar_type() == torch::kFloat32 && beta->numel() == 1 && beta->device() == like.device(),
              "beta must hold one fp32 value on score's device");
  return beta->data_ptr<float>();
}
void check_edge_vector(const torch::Tensor& t, const char* name, const torch::Tensor& nodePointer) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous(), name, " must be a contiguous CUDA tensor");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32 && t.dim() == 1, name, " must be a 1-D fp32 tensor of one value per edge");
  TORCH_CHECK(nodePointer.numel() >= 1 && nodePointer.scalar_type() == torch::kInt32 && nodePointer.device() == t.device(),
              "nodePointer must hold num_nodes + 1 int32 entries on ", name, "'s device");
}
}  // namespace

// Not in the reference: softmax over every node's incoming edges (tcgnn_edge_softmax; TCGNN.edge_softmax of the ctypes module)
torch::Tensor edge_softmax(torch::Tensor score, torch::Tensor nodePointer, c10::optional<torch::Tensor> beta, c10::optional<torch::Tensor> out) {
  CHECK_INPUT(nodePointer);
  check_edge_vector(score, "score", nodePointer);
  const float* b = beta_ptr(beta, score);
  torch::Tensor p = out.has_value() ? *out : torch::empty_like(score);
  TORCH_CHECK(p.sizes() == score.sizes() && p.scalar_type() == torch::kFloat32 && p.device() == score.device() && p.is_contiguous(),
              "out must be a contiguous fp32 tensor of score's shape on its device");
  DeviceGuard guard(score.device());
  tcgnn_check(tcgnn_edge_softmax(nodePointer.data_ptr<int>(), (int32_t)(nodePointer.numel() - 1), score.numel(), score.data_ptr<float>(), b,
                                 p.data_ptr<float>(), current_stream(score)), "tcgnn_edge_softmax");
  return p;
}

// ... and its backward: (ds, dbeta); dbeta is None unless need_dbeta (which needs the scores)
std::tuple<torch::Tensor, c10::optional<torch::Tensor>> edge_softmax_backward(torch::Tensor p, torch::Tensor dp, torch::Tensor nodePointer,
                                                                               c10::optional<torch::Tensor> beta, c10::optional<torch::Tensor> score,
                                                                               bool need_dbeta, c10::optional<torch::Tensor> out) {
  CHECK_INPUT(nodePointer);
  check_edge_vector(p, "p", nodePointer);
  check_edge_vector(dp, "dp", nodePointer);
  TORCH_CHECK(dp.sizes() == p.sizes() && dp.device() == p.device(), "dp must have the shape and device of p");
  const float* b = beta_ptr(beta, p);
  const float* s = nullptr;
  if (need_dbeta) {
    TORCH_CHECK(score.has_value(), "dbeta needs the scores the softmax was taken of");
    check_edge_vector(*score, "score", nodePointer);
    TORCH_CHECK(score->sizes() == p.sizes() && score->device() == p.device(), "score must have the shape and device of p");
    s = score->data_ptr<float>();
  }
  torch::Tensor ds = out.has_value() ? *out : torch::empty_like(dp);
  TORCH_CHECK(ds.sizes() == dp.sizes() && ds.scalar_type() == torch::kFloat32 && ds.device() == dp.device() && ds.is_contiguous(),
              "out must be a contiguous fp32 tensor of dp's shape on its device");
  DeviceGuard guard(p.device());
  const int32_t N = (int32_t)(nodePointer.numel() - 1);
  c10::optional<torch::Tensor> dbeta;
  void* scratch = nullptr;
  size_t need = 0;
  torch::Tensor buf;
  if (need_dbeta) {
    dbeta = torch::empty({1}, p.options());
    need = tcgnn_edge_softmax_workspace_bytes(N, p.numel());
    buf = aligned_scratch(need, p, &scratch);
  }
  tcgnn_check(tcgnn_edge_softmax_backward(nodePointer.data_ptr<int>(), N, p.numel(), p.data_ptr<float>(), dp.data_ptr<float>(), s, b, ds.data_ptr<float>(),
                                          need_dbeta ? dbeta->data_ptr<float>() : nullptr, scratch, need, current_stream(p)), "tcgnn_edge_softmax_backward");
  return {ds, dbeta};
}

// ---- not in the reference: multi-head GAT attention (tcgnn_gat_softmax / _backward / tcgnn_edge_colsum; the ctypes module's
// gat_softmax, gat_softmax_backward and edge_colsum) ------------------------------------------------------------------------------
namespace {
// (N, E, H) of a GAT call, after the checks of the ctypes module
std::tuple<int32_t, int64_t, int32_t> gat_args(const torch::Tensor& el, const torch::Tensor& er, const torch::Tensor& nodePointer,
                                               const torch::Tensor& edgeList) {
  CHECK_INPUT(el); CHECK_INPUT(er); CHECK_INPUT(nodePointer); CHECK_INPUT(edgeList);
  TORCH_CHECK(el.scalar_type() == torch::kFloat32 && er.scalar_type() == torch::kFloat32, "expected scalar type Float");
  TORCH_CHECK(nodePointer.scalar_type() == torch::kInt32 && edgeList.scalar_type() == torch::kInt32, "expected scalar type Int");
  TORCH_CHECK(nodePointer.numel() >= 1, "nodePointer must hold num_nodes + 1 entries");
  const int64_t N = nodePointer.numel() - 1;
  TORCH_CHECK(el.dim() == 2 && el.size(0) == N && el.size(1) >= 1 && er.sizes() == el.sizes(), "el and er must be [num_nodes, heads] (heads >= 1)");
  TORCH_CHECK(er.device() == el.device() && nodePointer.device() == el.device() && edgeList.device() == el.device(),
              "el, er, nodePointer and edgeList must be on one device");
  return {(int32_t)N, edgeList.numel(), (int32_t)el.size(1)};
}
void check_head_major(const torch::Tensor& t, const char* name, int64_t H, int64_t E, const torch::Tensor& like) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == torch::kFloat32 && t.dim() == 2 && t.size(0) == H && t.size(1) == E &&
              t.device() == like.device(), name, " must be a contiguous fp32 [heads, num_edges] tensor on the device of el");
}

}  // namespace

torch::Tensor gat_softmax(torch::Tensor el, torch::Tensor er, torch::Tensor nodePointer, torch::Tensor edgeList, double negative_slope,
                          c10::optional<torch::Tensor> out) {
  auto [N, E, H] = gat_args(el, er, nodePointer, edgeList);
  torch::Tensor p = out.has_value() ? *out : torch::empty({(int64_t)H, E}, el.options());
  check_head_major(p, "out", H, E, el);
  DeviceGuard guard(el.device());
  tcgnn_check(tcgnn_gat_softmax(nodePointer.data_ptr<int>(), edgeList.data_ptr<int>(), N, E, H, el.data_ptr<float>(), er.data_ptr<float>(),
                                (float)negative_slope, p.data_ptr<float>(), current_stream(el)), "tcgnn_gat_softmax");
  return p;
}

std::tuple<torch::Tensor, torch::Tensor> gat_softmax_backward(torch::Tensor p, torch::Tensor dp, torch::Tensor el, torch::Tensor er,
                                                              torch::Tensor nodePointer, torch::Tensor edgeList, double negative_slope,
                                                              c10::optional<torch::Tensor> out) {
  auto [N, E, H] = gat_args(el, er, nodePointer, edgeList);
  check_head_major(p, "p", H, E, el);
  check_head_major(dp, "dp", H, E, el);
  torch::Tensor ds = out.has_value() ? *out : torch::empty_like(dp);
  check_head_major(ds, "out", H, E, el);
  DeviceGuard guard(el.device());
  torch::Tensor d_er = torch::empty({(int64_t)N, (int64_t)H}, el.options());
  tcgnn_check(tcgnn_gat_softmax_backward(nodePointer.data_ptr<int>(), edgeList.data_ptr<int>(), N, E, H, el.data_ptr<float>(), er.data_ptr<float>(),
                                         (float)negative_slope, p.data_ptr<float>(), dp.data_ptr<float>(), ds.data_ptr<float>(),
                                         d_er.data_ptr<float>(), current_stream(el)), "tcgnn_gat_softmax_backward");
  return {ds, d_er};
}

torch::Tensor edge_colsum(torch::Tensor val, torch::Tensor nodePointer, torch::Tensor edgeList) {
  CHECK_INPUT(val); CHECK_INPUT(nodePointer); CHECK_INPUT(edgeList);
  TORCH_CHECK(val.scalar_type() == torch::kFloat32, "expected scalar type Float");
  TORCH_CHECK(nodePointer.scalar_type() == torch::kInt32 && edgeList.scalar_type() == torch::kInt32, "expected scalar type Int");
  TORCH_CHECK(nodePointer.numel() >= 1, "nodePointer must hold num_nodes + 1 entries");
  TORCH_CHECK(val.dim() == 2 && val.size(0) >= 1 && val.size(1) == edgeList.numel(), "val must be [heads, num_edges] (heads >= 1)");
  TORCH_CHECK(val.device() == nodePointer.device() && edgeList.device() == nodePointer.device(), "val, nodePointer and edgeList must be on one device");
  DeviceGuard guard(val.device());
  TransposedCsr& t = transposed_csr(nodePointer, edgeList);
  const int64_t N = nodePointer.numel() - 1, H = val.size(0);
  torch::Tensor out = torch::empty({N, H}, val.options());
  tcgnn_check(tcgnn_edge_colsum(t.rp_t.data_ptr<int>(), t.perm.data_ptr<int>(), (int32_t)N, edgeList.numel(), (int32_t)H, val.data_ptr<float>(),
                                out.data_ptr<float>(), current_stream(val)), "tcgnn_edge_colsum");
  return out;
}

// ---- not in the reference: GATv2 attention (tcgnn_gatv2_softmax / _backward / tcgnn_gatv2_source_grad; the ctypes module's
// gatv2_softmax, gatv2_softmax_backward and gatv2_source_grad) ----------------------------------------------------------------------
namespace {
// (N, E, H, F) of a GATv2 call, after the checks of the ctypes module
std::tuple<int32_t, int64_t, int32_t, int32_t> gatv2_args(const torch::Tensor& xl, const torch::Tensor& xr, const torch::Tensor& attn,
                                                          const torch::Tensor& nodePointer, const torch::Tensor& edgeList) {
  CHECK_INPUT(xl); CHECK_INPUT(xr); CHECK_INPUT(attn); CHECK_INPUT(nodePointer); CHECK_INPUT(edgeList);
  TORCH_CHECK(xl.scalar_type() == torch::kFloat32 && xr.scalar_type() == torch::kFloat32 && attn.scalar_type() == torch::kFloat32,
              "expected scalar type Float");
  TORCH_CHECK(nodePointer.scalar_type() == torch::kInt32 && edgeList.scalar_type() == torch::kInt32, "expected scalar type Int");
  TORCH_CHECK(nodePointer.numel() >= 1, "nodePointer must hold num_nodes + 1 entries");
  TORCH_CHECK(attn.dim() == 2 && attn.size(0) >= 1 && attn.size(1) >= 1, "attn must be [heads, features] (heads >= 1, features >= 1)");
  const int64_t N = nodePointer.numel() - 1, H = attn.size(0), F = attn.size(1);
  TORCH_CHECK(xl.dim() == 2 && xl.size(0) == N && xl.size(1) == H * F && xr.sizes() == xl.sizes(), "xl and xr must be [num_nodes, heads * features]");
  TORCH_CHECK(xr.device() == xl.device() && attn.device() == xl.device() && nodePointer.device() == xl.device() && edgeList.device() == xl.device(),
              "xl, xr, attn, nodePointer and edgeList must be on one device");
  return {(int32_t)N, edgeList.numel(), (int32_t)H, (int32_t)F};
}
}  // namespace

torch::Tensor gatv2_softmax(torch::Tensor xl, torch::Tensor xr, torch::Tensor attn, torch::Tensor nodePointer, torch::Tensor edgeList,
                            double negative_slope, c10::optional<torch::Tensor> out, c10::optional<torch::Tensor> score_out) {
  auto [N, E, H, F] = gatv2_args(xl, xr, attn, nodePointer, edgeList);
  torch::Tensor p = out.has_value() ? *out : torch::empty({(int64_t)H, E}, xl.options());
  check_head_major(p, "out", H, E, xl);
  if (score_out.has_value()) check_head_major(*score_out, "score_out", H, E, xl);
  DeviceGuard guard(xl.device());
  tcgnn_check(tcgnn_gatv2_softmax(nodePointer.data_ptr<int>(), edgeList.data_ptr<int>(), N, E, H, F, xl.data_ptr<float>(), xr.data_ptr<float>(),
                                  attn.data_ptr<float>(), (float)negative_slope, score_out.has_value() ? score_out->data_ptr<float>() : nullptr,
                                  p.data_ptr<float>(), current_stream(xl)), "tcgnn_gatv2_softmax");
  return p;
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> gatv2_softmax_backward(torch::Tensor p, torch::Tensor dp, torch::Tensor xl, torch::Tensor xr,
                                                                               torch::Tensor attn, torch::Tensor nodePointer, torch::Tensor edgeList,
                                                                               double negative_slope, c10::optional<torch::Tensor> out) {
  auto [N, E, H, F] = gatv2_args(xl, xr, attn, nodePointer, edgeList);
  check_head_major(p, "p", H, E, xl);
  check_head_major(dp, "dp", H, E, xl);
  torch::Tensor g = out.has_value() ? *out : torch::empty_like(dp);
  check_head_major(g, "out", H, E, xl);
  DeviceGuard guard(xl.device());
  torch::Tensor d_xr = torch::empty({(int64_t)N, (int64_t)H * F}, xl.options());
  torch::Tensor d_attn = torch::empty({(int64_t)H, (int64_t)F}, xl.options());
  void* scratch = nullptr;
  const size_t need = tcgnn_gatv2_workspace_bytes(N, E, H, F);
  torch::Tensor buf = aligned_scratch(need, xl, &scratch);
  tcgnn_check(tcgnn_gatv2_softmax_backward(nodePointer.data_ptr<int>(), edgeList.data_ptr<int>(), N, E, H, F, xl.data_ptr<float>(), xr.data_ptr<float>(),
                                           attn.data_ptr<float>(), (float)negative_slope, p.data_ptr<float>(), dp.data_ptr<float>(), g.data_ptr<float>(),
                                           d_xr.data_ptr<float>(), d_attn.data_ptr<float>(), scratch, need, current_stream(xl)),
              "tcgnn_gatv2_softmax_backward");
  return {g, d_xr, d_attn};
}

torch::Tensor gatv2_source_grad(torch::Tensor g, torch::Tensor xl, torch::Tensor xr, torch::Tensor attn, torch::Tensor nodePointer,
                                torch::Tensor edgeList, double negative_slope) {
  auto [N, E, H, F] = gatv2_args(xl, xr, attn, nodePointer, edgeList);
  check_head_major(g, "g", H, E, xl);
  DeviceGuard guard(xl.device());
  TransposedCsr& t = transposed_csr(nodePointer, edgeList);
  torch::Tensor d_xl = torch::empty({(int64_t)N, (int64_t)H * F}, xl.options());
  tcgnn_check(tcgnn_gatv2_source_grad(t.rp_t.data_ptr<int>(), t.col_t.data_ptr<int>(), t.perm.data_ptr<int>(), N, E, H, F, xl.data_ptr<float>(),
                                      xr.data_ptr<float>(), attn.data_ptr<float>(), (float)negative_slope, g.data_ptr<float>(), d_xl.data_ptr<float>(),
                                      current_stream(xl)), "tcgnn_gatv2_source_grad");
  return d_xl;
}

// ---- not in the reference: element-wise maximum over a node's incoming edges (tcgnn_segment_max / _backward; the ctypes module's
// forward_max and backward_max) ---------------------------------------------------------------------------------------------------
namespace {
// (N, E, D) of a max-aggregation call, after the checks of the ctypes module
std::tuple<int32_t, int64_t, int32_t> max_args(const torch::Tensor& t, const char* name, const torch::Tensor& nodePointer, const torch::Tensor& edgeList) {
  TORCH_CHECK(t.is_cuda(), name, " must be a CUDA tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  CHECK_INPUT(nodePointer); CHECK_INPUT(edgeList);
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, "expected scalar type Float");
  TORCH_CHECK(nodePointer.scalar_type() == torch::kInt32 && edgeList.scalar_type() == torch::kInt32, "expected scalar type Int");
  TORCH_CHECK(nodePointer.numel() >= 1, "nodePointer must hold num_nodes + 1 entries");
  const int64_t N = nodePointer.numel() - 1;
  TORCH_CHECK(t.dim() == 2 && t.size(0) == N, name, " must be [num_nodes, embedding_dim]");
  TORCH_CHECK(nodePointer.device() == t.device() && edgeList.device() == t.device(), name, ", nodePointer and edgeList must be on one device");
  return {(int32_t)N, edgeList.numel(), (int32_t)t.size(1)};
}
torch::Tensor out_like(const c10::optional<torch::Tensor>& out, const torch::Tensor& t, const char* name) {
  if (!out.has_value()) return torch::empty_like(t);
  TORCH_CHECK(out->is_cuda() && out->is_contiguous() && out->scalar_type() == torch::kFloat32 && out->sizes() == t.sizes() && out->device() == t.device(),
              "out must be a contiguous fp32 tensor of ", name, "'s shape on its device");
  return *out;
}
}  // namespace

std::tuple<torch::Tensor, c10::optional<torch::Tensor>> forward_max(torch::Tensor input, torch::Tensor nodePointer, torch::Tensor edgeList, bool return_arg,
                                                                    c10::optional<torch::Tensor> out) {
  auto [N, E, D] = max_args(input, "input", nodePointer, edgeList);
  torch::Tensor Y = out_like(out, input, "input");
  DeviceGuard guard(input.device());
  c10::optional<torch::Tensor> arg;
  if (return_arg) arg = torch::empty({(int64_t)N, (int64_t)D}, input.options().dtype(torch::kInt32));
  tcgnn_check(tcgnn_segment_max(nodePointer.data_ptr<int>(), edgeList.data_ptr<int>(), N, E, input.data_ptr<float>(), D, Y.data_ptr<float>(),
                                arg.has_value() ? arg->data_ptr<int>() : nullptr, current_stream(input)), "tcgnn_segment_max");
  return {Y, arg};
}

torch::Tensor backward_max(torch::Tensor dY, torch::Tensor arg, torch::Tensor nodePointer, torch::Tensor edgeList, c10::optional<torch::Tensor> out) {
  auto [N, E, D] = max_args(dY, "dY", nodePointer, edgeList);
  CHECK_INPUT(arg);
  TORCH_CHECK(arg.scalar_type() == torch::kInt32, "expected scalar type Int");
  TORCH_CHECK(arg.sizes() == dY.sizes() && arg.device() == dY.device(), "arg must have the shape and device of dY");
  torch::Tensor dX = out_like(out, dY, "dY");
  DeviceGuard guard(dY.device());
  TransposedCsr& t = transposed_csr(nodePointer, edgeList);
  tcgnn_check(tcgnn_segment_max_backward(t.rp_t.data_ptr<int>(), t.col_t.data_ptr<int>(), t.perm.data_ptr<int>(), N, E, arg.data_ptr<int>(),
                                         dY.data_ptr<float>(), D, dX.data_ptr<float>(), current_stream(dY)), "tcgnn_segment_max_backward");
  return dX;
}

// ---- not in the reference: mean / std / max / min over a node's incoming edges in one walk (tcgnn_segment_stats / _backward; the
// ctypes module's forward_stats and backward_stats, whose element-wise steps these repeat operation for operation) -----------------
namespace {
using TensorMap = std::map<std::string, c10::optional<torch::Tensor>>;
bool stats_name(const std::string& a) { return a == "mean" || a == "std" || a == "max" || a == "min"; }
const torch::Tensor* given(const TensorMap& m, const char* key) {
  auto it = m.find(key);
  return it != m.end() && it->second.has_value() ? &*it->second : nullptr;
}
const torch::Tensor& saved_tensor(const TensorMap& m, const char* key) {
  const torch::Tensor* t = given(m, key);
  TORCH_CHECK(t != nullptr, "saved has no '", key, "'");
  return *t;
}
template <typename T>
const T* ptr_or_null(const torch::Tensor* t) { return t ? t->data_ptr<T>() : nullptr; }
}  // namespace

py::dict forward_stats(torch::Tensor input, torch::Tensor nodePointer, torch::Tensor edgeList, std::vector<std::string> aggregators, double eps,
                       bool return_arg) {
  if (aggregators.empty()) throw py::value_error("aggregators must name at least one of mean, std, max, min");
  for (const std::string& a : aggregators)
    if (!stats_name(a)) throw py::value_error("aggregators must be among mean, std, max, min, got '" + a + "'");
  auto [N, E, D] = max_args(input, "input", nodePointer, edgeList);
  DeviceGuard guard(input.device());
  auto asked = [&](const char* a) { return std::find(aggregators.begin(), aggregators.end(), a) != aggregators.end(); };
  std::map<std::string, torch::Tensor> out;
  for (const char* a : {"mean", "std", "max", "min"})
    if (asked(a)) out[a] = torch::empty({(int64_t)N, (int64_t)D}, input.options());
  if (return_arg)
    for (const char* a : {"max", "min"})
      if (asked(a)) out[std::string("arg") + a] = torch::empty({(int64_t)N, (int64_t)D}, input.options().dtype(torch::kInt32));
  auto f = [&](const char* k) { auto it = out.find(k); return it != out.end() ? it->second.data_ptr<float>() : nullptr; };
  auto i = [&](const char* k) { auto it = out.find(k); return it != out.end() ? it->second.data_ptr<int>() : nullptr; };
  if (N && D)   // (a tensor without elements has no address to give)
    tcgnn_check(tcgnn_segment_stats(nodePointer.data_ptr<int>(), edgeList.data_ptr<int>(), N, E, input.data_ptr<float>(), D, (float)eps, f("mean"), f("std"),
                                    f("max"), i("argmax"), f("min"), i("argmin"), current_stream(input)), "tcgnn_segment_stats");
  py::dict d;
  for (auto& kv : out) d[py::str(kv.first)] = kv.second;
  return d;
}

torch::Tensor backward_stats(TensorMap grads, TensorMap saved, torch::Tensor nodePointer, torch::Tensor edgeList, c10::optional<torch::Tensor> out) {
  for (auto& kv : grads)
    if (!stats_name(kv.first)) throw py::value_error("grads must be keyed by mean, std, max, min, got '" + kv.first + "'");
  const torch::Tensor& Z = saved_tensor(saved, "Z");
  auto [N, E, D] = max_args(Z, "Z", nodePointer, edgeList);
  for (auto& kv : grads)
    if (kv.second.has_value()) {
      CHECK_INPUT((*kv.second));
      TORCH_CHECK(kv.second->scalar_type() == torch::kFloat32, "expected scalar type Float");
      TORCH_CHECK(kv.second->sizes() == Z.sizes() && kv.second->device() == Z.device(), "grads['", kv.first, "'] must have the shape and device of Z");
    }
  const torch::Tensor *g_mean = given(grads, "mean"), *g_std = given(grads, "std"), *g_max = given(grads, "max"), *g_min = given(grads, "min");
  const torch::Tensor *argmax = nullptr, *argmin = nullptr;
  for (auto [g, key, slot] : {std::make_tuple(g_max, "argmax", &argmax), std::make_tuple(g_min, "argmin", &argmin)})
    if (g) {
      const torch::Tensor& arg = saved_tensor(saved, key);
      CHECK_INPUT(arg);
      TORCH_CHECK(arg.scalar_type() == torch::kInt32, "expected scalar type Int");
      TORCH_CHECK(arg.sizes() == Z.sizes() && arg.device() == Z.device(), key, " must have the shape and device of Z");
      *slot = &arg;
    }
  torch::Tensor dZ = out_like(out, Z, "Z");
  if (!(N && D)) return dZ;
  DeviceGuard guard(Z.device());
  torch::Tensor a, b;
  if (g_mean || g_std) {
    using torch::indexing::Slice;
    using torch::indexing::None;
    torch::Tensor hi = nodePointer.index({Slice(1, None)}), lo = nodePointer.index({Slice(None, -1)});
    torch::Tensor has = (hi > lo).unsqueeze(1);
    torch::Tensor inv_k = has.to(torch::kFloat32) / (hi - lo).clamp_min(1).to(torch::kFloat32).unsqueeze(1);
    if (g_std) {
      b = (*g_std * inv_k) / torch::where(has, saved_tensor(saved, "std"), 1.0);
      const torch::Tensor& mean = saved_tensor(saved, "mean");
      a = g_mean ? (*g_mean * inv_k - b * mean) : -(b * mean);
    } else {
      a = *g_mean * inv_k;
    }
  }
  TransposedCsr& t = transposed_csr(nodePointer, edgeList);
  tcgnn_check(tcgnn_segment_stats_backward(t.rp_t.data_ptr<int>(), t.col_t.data_ptr<int>(), t.perm.data_ptr<int>(), N, E,
                                           b.defined() ? Z.data_ptr<float>() : nullptr, a.defined() ? a.data_ptr<float>() : nullptr,
                                           b.defined() ? b.data_ptr<float>() : nullptr, ptr_or_null<int>(argmax), ptr_or_null<float>(g_max),
                                           ptr_or_null<int>(argmin), ptr_or_null<float>(g_min), D, dZ.data_ptr<float>(), current_stream(Z)),
              "tcgnn_segment_stats_backward");
  return dZ;
}

// ---- not in the reference: a feature vector per edge (tcgnn_edge_message / _backward, tcgnn_edge_sum; the ctypes module's forward_ue,
// backward_ue and edge_sum) and the cached transpose their autograd Function asks for (the ctypes module's transpose_graph) ---------
namespace {
int ue_act(const c10::optional<std::string>& act) {
  if (!act.has_value() || *act == "identity") return TCGNN_ACT_IDENTITY;
  if (*act == "relu") return TCGNN_ACT_RELU;
  throw py::value_error("act must be 'relu', 'identity' or None, got '" + *act + "'");
}
void check_edge_rows(const torch::Tensor& t, const char* name, int64_t E, int64_t D, const torch::Tensor& like) {
  TORCH_CHECK(t.is_cuda(), name, " must be a CUDA tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, "expected scalar type Float");
  TORCH_CHECK(t.dim() == 2 && t.size(0) == E && t.size(1) == D && t.device() == like.device(), name,
              " must be a contiguous fp32 [num_edges, embedding_dim] = [", E, ", ", D, "] tensor on the device of nodePointer");
}
void check_out_apart(const c10::optional<torch::Tensor>& out, std::initializer_list<const torch::Tensor*> inputs) {
  if (!out.has_value() || !out->numel()) return;
  const char* lo = static_cast<const char*>(out->data_ptr());
  const char* hi = lo + out->numel() * out->element_size();
  for (const torch::Tensor* t : inputs)
    if (t && t->defined() && t->numel()) {
      const char* a = static_cast<const char*>(t->data_ptr());
      TORCH_CHECK(!(a < hi && lo < a + t->numel() * t->element_size()), "out must not share memory with an input");
    }
}
}  // namespace

torch::Tensor forward_ue(torch::Tensor X, torch::Tensor Ef, torch::Tensor nodePointer, torch::Tensor edgeList, c10::optional<std::string> act,
                         c10::optional<torch::Tensor> out) {
  auto [N, E, D] = max_args(X, "X", nodePointer, edgeList);
  const int code = ue_act(act);
  check_edge_rows(Ef, "Ef", E, D, nodePointer);
  torch::Tensor Y = out_like(out, X, "X");
  check_out_apart(out, {&X, &Ef});
  DeviceGuard guard(X.device());
  tcgnn_check(tcgnn_edge_message(nodePointer.data_ptr<int>(), edgeList.data_ptr<int>(), N, E, X.data_ptr<float>(), Ef.data_ptr<float>(), D, code,
                                 Y.data_ptr<float>(), current_stream(X)), "tcgnn_edge_message");
  return Y;
}

torch::Tensor backward_ue(torch::Tensor dY, c10::optional<torch::Tensor> X, c10::optional<torch::Tensor> Ef, torch::Tensor nodePointer,
                          torch::Tensor edgeList, c10::optional<std::string> act, c10::optional<torch::Tensor> out) {
  auto [N, E, D] = max_args(dY, "dY", nodePointer, edgeList);
  const int code = ue_act(act);
  if (code != TCGNN_ACT_IDENTITY) {
    TORCH_CHECK(X.has_value() && Ef.has_value(), "X and Ef are needed to recompute the activation's mask");
    CHECK_INPUT((*X));
    TORCH_CHECK(X->scalar_type() == torch::kFloat32, "expected scalar type Float");
    TORCH_CHECK(X->sizes() == dY.sizes() && X->device() == dY.device(), "X must have the shape and device of dY");
    check_edge_rows(*Ef, "Ef", E, D, nodePointer);
  }
  torch::Tensor dM;
  if (out.has_value()) {
    check_edge_rows(*out, "out", E, D, nodePointer);
    dM = *out;
  } else {
    dM = torch::empty({E, (int64_t)D}, dY.options());
  }
  const bool masked = code != TCGNN_ACT_IDENTITY;
  check_out_apart(out, {&dY, masked ? &*X : nullptr, masked ? &*Ef : nullptr});
  DeviceGuard guard(dY.device());
  tcgnn_check(tcgnn_edge_message_backward(nodePointer.data_ptr<int>(), edgeList.data_ptr<int>(), N, E, masked ? X->data_ptr<float>() : nullptr,
                                          masked ? Ef->data_ptr<float>() : nullptr, dY.data_ptr<float>(), D, code, dM.data_ptr<float>(),
                                          current_stream(dY)), "tcgnn_edge_message_backward");
  return dM;
}

torch::Tensor edge_sum(torch::Tensor M, torch::Tensor nodePointer, c10::optional<torch::Tensor> perm, c10::optional<torch::Tensor> out) {
  CHECK_INPUT(nodePointer);
  TORCH_CHECK(nodePointer.scalar_type() == torch::kInt32, "expected scalar type Int");
  TORCH_CHECK(nodePointer.numel() >= 1, "nodePointer must hold num_nodes + 1 entries");
  CHECK_INPUT(M);
  TORCH_CHECK(M.scalar_type() == torch::kFloat32, "expected scalar type Float");
  TORCH_CHECK(M.dim() == 2 && M.device() == nodePointer.device(), "M must be [num_edges, embedding_dim] on nodePointer's device");
  const int64_t N = nodePointer.numel() - 1, E = M.size(0), D = M.size(1);
  if (perm.has_value()) {
    CHECK_INPUT((*perm));
    TORCH_CHECK(perm->scalar_type() == torch::kInt32, "expected scalar type Int");
    TORCH_CHECK(perm->dim() == 1 && perm->numel() == E && perm->device() == M.device(), "perm must hold num_edges entries on M's device");
  }
  torch::Tensor Y;
  if (out.has_value()) {
    TORCH_CHECK(out->is_cuda() && out->is_contiguous() && out->scalar_type() == torch::kFloat32 && out->dim() == 2 && out->size(0) == N &&
                out->size(1) == D && out->device() == M.device(), "out must be a contiguous fp32 [num_nodes, embedding_dim] tensor on M's device");
    Y = *out;
  } else {
    Y = torch::empty({N, D}, M.options());
  }
  check_out_apart(out, {&M});
  DeviceGuard guard(M.device());
  tcgnn_check(tcgnn_edge_sum(nodePointer.data_ptr<int>(), perm.has_value() ? perm->data_ptr<int>() : nullptr, (int32_t)N, E, M.data_ptr<float>(),
                             (int32_t)D, Y.data_ptr<float>(), current_stream(M)), "tcgnn_edge_sum");
  return Y;
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, bool> transpose_graph(torch::Tensor nodePointer, torch::Tensor edgeList) {
  CHECK_INPUT(nodePointer); CHECK_INPUT(edgeList);
  TORCH_CHECK(nodePointer.scalar_type() == torch::kInt32 && edgeList.scalar_type() == torch::kInt32, "expected scalar type Int");
  TORCH_CHECK(nodePointer.numel() >= 1, "nodePointer must hold num_nodes + 1 entries");
  TORCH_CHECK(edgeList.device() == nodePointer.device(), "nodePointer and edgeList must be on one device");
  DeviceGuard guard(nodePointer.device());
  TransposedCsr& t = transposed_csr(nodePointer, edgeList);
  return {t.rp_t, t.col_t, t.perm, t.symmetric};
}

// Not in the reference: seeded neighbour sampling (tcgnn_sample_neighbors_count + tcgnn_sample_neighbors; TCGNN.sample_neighbors of the
// ctypes module).  The graph over the same nodes with at most `fanout` in-edges per row: (nodePointer_s, edgeList_s, eid).  fanout = None
// keeps every edge.  seed: any Python int, taken modulo 2^64.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> sample_neighbors(torch::Tensor nodePointer, torch::Tensor edgeList, c10::optional<int64_t> fanout,
                                                                         py::int_ seed, c10::optional<torch::Tensor> row_mask) {
  CHECK_INPUT(nodePointer); CHECK_INPUT(edgeList);
  TORCH_CHECK(nodePointer.scalar_type() == torch::kInt32 && edgeList.scalar_type() == torch::kInt32, "expected scalar type Int");
  TORCH_CHECK(nodePointer.numel() >= 1, "nodePointer must hold num_nodes + 1 entries");
  TORCH_CHECK(edgeList.device() == nodePointer.device(), "nodePointer and edgeList must be on one device");
  const int64_t N = nodePointer.numel() - 1, E = edgeList.numel();
  const uint8_t* mask = nullptr;
  torch::Tensor mask_keep;
  if (row_mask.has_value()) {
    CHECK_INPUT((*row_mask));
    TORCH_CHECK(row_mask->scalar_type() == torch::kUInt8 || row_mask->scalar_type() == torch::kBool, "row_mask must be uint8 or bool");
    TORCH_CHECK(row_mask->numel() == N && row_mask->device() == nodePointer.device(), "row_mask must hold one entry per node on nodePointer's device");
    mask_keep = *row_mask;
    mask = static_cast<const uint8_t*>(mask_keep.data_ptr());
  }
  TORCH_CHECK(!fanout.has_value() || *fanout >= 0, "fanout must be None or >= 0");
  const int32_t k = (int32_t)std::min<int64_t>(fanout.value_or(0x7fffffff), 0x7fffffff);
  const uint64_t seed64 = py::cast<uint64_t>(seed.attr("__and__")(py::int_(0xFFFFFFFFFFFFFFFFull)));
  DeviceGuard guard(nodePointer.device());
  size_t need = 0;
  tcgnn_check(tcgnn_sample_workspace_bytes((int32_t)N, &need), "tcgnn_sample_workspace_bytes");
  torch::Tensor ws = torch::empty({(int64_t)need + 256}, nodePointer.options().dtype(torch::kUInt8));
  char* wsp = static_cast<char*>(ws.data_ptr());
  wsp += (256 - reinterpret_cast<uintptr_t>(wsp) % 256) % 256;
  torch::Tensor rp_s = torch::empty({N + 1}, nodePointer.options());
  int64_t kept = 0;
  tcgnn_check(tcgnn_sample_neighbors_count(nodePointer.data_ptr<int>(), mask, (int32_t)N, E, k, rp_s.data_ptr<int>(), wsp, need, &kept,
                                           current_stream(nodePointer)), "tcgnn_sample_neighbors_count");
  torch::Tensor col_s = torch::empty({kept}, edgeList.options()), eid = torch::empty({kept}, edgeList.options());
  if (kept > 0)
    tcgnn_check(tcgnn_sample_neighbors(nodePointer.data_ptr<int>(), edgeList.data_ptr<int>(), mask, rp_s.data_ptr<int>(), (int32_t)N, E, k, seed64,
                                       col_s.data_ptr<int>(), eid.data_ptr<int>(), current_stream(nodePointer)), "tcgnn_sample_neighbors");
  return {rp_s, col_s, eid};
}

// Not in the reference: relabelled mini-batch blocks (tcgnn_compact_*; TCGNN.compact_nodes / compact_graph of the ctypes module).
// compact_nodes: the node set of the layer graphs of one mini-batch, (nodes, new_id) - one stream synchronisation however many graphs.
static void check_csr_pair(const torch::Tensor& nodePointer, const torch::Tensor& edgeList) {
  CHECK_INPUT(nodePointer); CHECK_INPUT(edgeList);
  TORCH_CHECK(nodePointer.scalar_type() == torch::kInt32 && edgeList.scalar_type() == torch::kInt32, "expected scalar type Int");
  TORCH_CHECK(nodePointer.numel() >= 1, "nodePointer must hold num_nodes + 1 entries");
  TORCH_CHECK(edgeList.device() == nodePointer.device(), "nodePointer and edgeList must be on one device");
}

std::tuple<torch::Tensor, torch::Tensor> compact_nodes(std::vector<std::vector<torch::Tensor>> graphs, c10::optional<torch::Tensor> keep) {
  TORCH_CHECK(!graphs.empty(), "compact_nodes needs at least one (nodePointer, edgeList) pair");
  for (const auto& g : graphs) {
    TORCH_CHECK(g.size() >= 2, "every graph is a (nodePointer, edgeList) pair");
    check_csr_pair(g[0], g[1]);
    TORCH_CHECK(g[0].device() == graphs[0][0].device(), "every graph must be on one device");
    TORCH_CHECK(g[0].numel() == graphs[0][0].numel(), "every graph must have the same number of nodes");
  }
  const torch::Tensor& first = graphs[0][0];
  const int64_t N = first.numel() - 1;
  if (keep.has_value()) {
    CHECK_INPUT((*keep));
    TORCH_CHECK(keep->scalar_type() == torch::kUInt8 || keep->scalar_type() == torch::kBool, "keep must be uint8 or bool");
    TORCH_CHECK(keep->numel() == N && keep->device() == first.device(), "keep must hold one entry per node on nodePointer's device");
  }
  DeviceGuard guard(first.device());
  void* stream = current_stream(first);
  torch::Tensor mask = keep.has_value() ? keep->reshape({-1}).to(torch::kUInt8, /*non_blocking=*/false, /*copy=*/true)
                                        : torch::zeros({N}, first.options().dtype(torch::kUInt8));
  size_t need = 0;
  tcgnn_check(tcgnn_compact_workspace_bytes((int32_t)N, &need), "tcgnn_compact_workspace_bytes");
  torch::Tensor ws = torch::empty({(int64_t)need + 256}, first.options().dtype(torch::kUInt8));
  char* wsp = static_cast<char*>(ws.data_ptr());
  wsp += (256 - reinterpret_cast<uintptr_t>(wsp) % 256) % 256;
  tcgnn_check(tcgnn_compact_begin((int32_t)N, wsp, need, stream), "tcgnn_compact_begin");
  for (const auto& g : graphs)
    tcgnn_check(tcgnn_compact_mark(g[0].data_ptr<int>(), g[1].data_ptr<int>(), (int32_t)N, g[1].numel(), static_cast<uint8_t*>(mask.data_ptr()), wsp, need,
                                   stream), "tcgnn_compact_mark");
  torch::Tensor new_id = torch::empty({N}, first.options());
  int32_t kept = 0;
  tcgnn_check(tcgnn_compact_count(static_cast<const uint8_t*>(mask.data_ptr()), (int32_t)N, new_id.data_ptr<int>(), wsp, need, &kept, stream),
              "tcgnn_compact_count");
  torch::Tensor nodes = torch::empty({(int64_t)kept}, first.options());
  tcgnn_check(tcgnn_compact_nodes(new_id.data_ptr<int>(), (int32_t)N, kept, nodes.data_ptr<int>(), stream), "tcgnn_compact_nodes");
  return {nodes, new_id};
}

// compact_graph: (nodePointer_b [M + 1], edgeList_b [E]) of a graph that compact_nodes was given.  No synchronisation.
std::tuple<torch::Tensor, torch::Tensor> compact_graph(torch::Tensor nodePointer, torch::Tensor edgeList, torch::Tensor nodes, torch::Tensor new_id) {
  check_csr_pair(nodePointer, edgeList);
  CHECK_INPUT(nodes); CHECK_INPUT(new_id);
  TORCH_CHECK(nodes.scalar_type() == torch::kInt32 && new_id.scalar_type() == torch::kInt32, "expected scalar type Int");
  TORCH_CHECK(nodes.device() == nodePointer.device() && new_id.device() == nodePointer.device(), "nodes and new_id must be on nodePointer's device");
  const int64_t N = nodePointer.numel() - 1, E = edgeList.numel(), M = nodes.numel();
  TORCH_CHECK(new_id.numel() == N, "new_id must hold one entry per node");
  TORCH_CHECK(M <= N, "nodes holds more entries than the graph has nodes");
  DeviceGuard guard(nodePointer.device());
  torch::Tensor rp_b = torch::empty({M + 1}, nodePointer.options()), col_b = torch::empty({E}, edgeList.options());
  tcgnn_check(tcgnn_compact_graph(nodePointer.data_ptr<int>(), edgeList.data_ptr<int>(), new_id.data_ptr<int>(), nodes.data_ptr<int>(), (int32_t)N,
                                  (int32_t)M, E, rp_b.data_ptr<int>(), col_b.data_ptr<int>(), current_stream(nodePointer)), "tcgnn_compact_graph");
  return {rp_b, col_b};
}

// Not in the reference: seed-list sampling (tcgnn_sample_rows*, tcgnn_compact_mark_ids, tcgnn_compact_rows_graph; TCGNN.sample_rows /
// extend_nodes / compact_rows_graph of the ctypes module).  A mini-batch costs the rows it touches, not the graph's.
static void check_ids(const torch::Tensor& t, const torch::Device& dev, const char* name) {
  CHECK_INPUT(t);
  TORCH_CHECK(t.scalar_type() == torch::kInt32, "expected scalar type Int (", name, ")");
  TORCH_CHECK(t.device() == dev, name, " must be on the other tensors' device");
}

// sample_rows: sample_neighbors from a list of row ids - (rowPointer_s [R + 1], edgeList_s, eid), slot i = row rows[i].
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> sample_rows(torch::Tensor nodePointer, torch::Tensor edgeList, torch::Tensor rows,
                                                                    c10::optional<int64_t> fanout, py::int_ seed) {
  check_csr_pair(nodePointer, edgeList);
  check_ids(rows, nodePointer.device(), "rows");
  TORCH_CHECK(!fanout.has_value() || *fanout >= 0, "fanout must be None or >= 0");
  const int64_t N = nodePointer.numel() - 1, E = edgeList.numel(), R = rows.numel();
  const int32_t k = (int32_t)std::min<int64_t>(fanout.value_or(0x7fffffff), 0x7fffffff);
  const uint64_t seed64 = py::cast<uint64_t>(seed.attr("__and__")(py::int_(0xFFFFFFFFFFFFFFFFull)));
  DeviceGuard guard(nodePointer.device());
  size_t need = 0;
  tcgnn_check(tcgnn_sample_rows_workspace_bytes((int32_t)R, &need), "tcgnn_sample_rows_workspace_bytes");
  torch::Tensor ws = torch::empty({(int64_t)need + 256}, nodePointer.options().dtype(torch::kUInt8));
  char* wsp = static_cast<char*>(ws.data_ptr());
  wsp += (256 - reinterpret_cast<uintptr_t>(wsp) % 256) % 256;
  torch::Tensor rp_s = torch::empty({R + 1}, nodePointer.options());
  int64_t kept = 0;
  tcgnn_check(tcgnn_sample_rows_count(nodePointer.data_ptr<int>(), rows.data_ptr<int>(), (int32_t)R, (int32_t)N, E, k, rp_s.data_ptr<int>(), wsp, need,
                                      &kept, current_stream(nodePointer)), "tcgnn_sample_rows_count");
  torch::Tensor col_s = torch::empty({kept}, edgeList.options()), eid = torch::empty({kept}, edgeList.options());
  if (kept > 0)
    tcgnn_check(tcgnn_sample_rows(nodePointer.data_ptr<int>(), edgeList.data_ptr<int>(), rows.data_ptr<int>(), rp_s.data_ptr<int>(), (int32_t)R,
                                  (int32_t)N, E, k, seed64, col_s.data_ptr<int>(), eid.data_ptr<int>(), current_stream(nodePointer)),
                "tcgnn_sample_rows");
  return {rp_s, col_s, eid};
}

// extend_nodes: marks lists of ids into the caller's uint8 mask IN PLACE; (nodes, new_id) of the mask afterwards.  One synchronisation.
std::tuple<torch::Tensor, torch::Tensor> extend_nodes(torch::Tensor keep, py::object ids) {
  CHECK_INPUT(keep);
  TORCH_CHECK(keep.scalar_type() == torch::kUInt8, "keep must be uint8 (it is written in place)");
  std::vector<torch::Tensor> lists;
  if (THPVariable_Check(ids.ptr())) lists.push_back(py::cast<torch::Tensor>(ids));
  else lists = py::cast<std::vector<torch::Tensor>>(ids);
  for (const auto& t : lists) check_ids(t, keep.device(), "ids");
  const int64_t N = keep.numel();
  DeviceGuard guard(keep.device());
  void* stream = current_stream(keep);
  size_t need = 0;
  tcgnn_check(tcgnn_compact_workspace_bytes((int32_t)N, &need), "tcgnn_compact_workspace_bytes");
  torch::Tensor ws = torch::empty({(int64_t)need + 256}, keep.options());
  char* wsp = static_cast<char*>(ws.data_ptr());
  wsp += (256 - reinterpret_cast<uintptr_t>(wsp) % 256) % 256;
  uint8_t* const mask = static_cast<uint8_t*>(keep.data_ptr());
  tcgnn_check(tcgnn_compact_begin((int32_t)N, wsp, need, stream), "tcgnn_compact_begin");
  for (const auto& t : lists)
    tcgnn_check(tcgnn_compact_mark_ids(t.data_ptr<int>(), t.numel(), (int32_t)N, mask, wsp, need, stream), "tcgnn_compact_mark_ids");
  torch::Tensor new_id = torch::empty({N}, keep.options().dtype(torch::kInt32));
  int32_t kept = 0;
  tcgnn_check(tcgnn_compact_count(mask, (int32_t)N, new_id.data_ptr<int>(), wsp, need, &kept, stream), "tcgnn_compact_count");
  torch::Tensor nodes = torch::empty({(int64_t)kept}, new_id.options());
  tcgnn_check(tcgnn_compact_nodes(new_id.data_ptr<int>(), (int32_t)N, kept, nodes.data_ptr<int>(), stream), "tcgnn_compact_nodes");
  return {nodes, new_id};
}

// compact_rows_graph: (nodePointer_b [M + 1], edgeList_b [E']) of a sample_rows graph whose rows are strictly increasing.  No synchronisation.
std::tuple<torch::Tensor, torch::Tensor> compact_rows_graph(torch::Tensor rows, torch::Tensor rowPointer_s, torch::Tensor edgeList_s,
                                                            torch::Tensor nodes, torch::Tensor new_id) {
  CHECK_INPUT(rows);
  const torch::Device dev = rows.device();
  check_ids(rows, dev, "rows"); check_ids(rowPointer_s, dev, "rowPointer_s"); check_ids(edgeList_s, dev, "edgeList_s");
  check_ids(nodes, dev, "nodes"); check_ids(new_id, dev, "new_id");
  const int64_t R = rows.numel(), E = edgeList_s.numel(), M = nodes.numel(), N = new_id.numel();
  TORCH_CHECK(rowPointer_s.numel() == R + 1, "rowPointer_s must hold one entry per listed row and one more");
  TORCH_CHECK(M <= N, "nodes holds more entries than new_id has nodes");
  DeviceGuard guard(dev);
  torch::Tensor rp_b = torch::empty({M + 1}, rows.options()), col_b = torch::empty({E}, rows.options());
  tcgnn_check(tcgnn_compact_rows_graph(rows.data_ptr<int>(), (int32_t)R, rowPointer_s.data_ptr<int>(), edgeList_s.data_ptr<int>(), E,
                                       new_id.data_ptr<int>(), (int32_t)N, (int32_t)M, rp_b.data_ptr<int>(), col_b.data_ptr<int>(),
                                       current_stream(rows)), "tcgnn_compact_rows_graph");
  return {rp_b, col_b};
}

// Not in the reference: subgraph sampling (tcgnn_random_walk, tcgnn_induce_*; TCGNN.random_walk / induce_subgraph of the ctypes module).
// random_walk: walks int32 [W, length + 1], one seeded walk per entry of starts, towards a row's sources.  No synchronisation.
torch::Tensor random_walk(torch::Tensor nodePointer, torch::Tensor edgeList, torch::Tensor starts, int64_t length, py::int_ seed) {
  check_csr_pair(nodePointer, edgeList);
  check_ids(starts, nodePointer.device(), "starts");
  TORCH_CHECK(length >= 0 && length < 0x7fffffff, "length must be >= 0");
  const int64_t N = nodePointer.numel() - 1, E = edgeList.numel(), W = starts.numel();
  const uint64_t seed64 = py::cast<uint64_t>(seed.attr("__and__")(py::int_(0xFFFFFFFFFFFFFFFFull)));
  DeviceGuard guard(nodePointer.device());
  torch::Tensor walks = torch::empty({W, length + 1}, nodePointer.options());
  tcgnn_check(tcgnn_random_walk(nodePointer.data_ptr<int>(), E ? edgeList.data_ptr<int>() : nullptr, W ? starts.data_ptr<int>() : nullptr, (int32_t)W,
                                (int32_t)N, E, (int32_t)length, seed64, W ? walks.data_ptr<int>() : nullptr, current_stream(nodePointer)),
              "tcgnn_random_walk");
  return walks;
}

// induce_subgraph: (nodePointer_b [M + 1], edgeList_b [E_b], eid [E_b]) - what the graph induces on the nodes of extend_nodes.  One synchronisation.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> induce_subgraph(torch::Tensor nodePointer, torch::Tensor edgeList, torch::Tensor nodes,
                                                                        torch::Tensor new_id) {
  check_csr_pair(nodePointer, edgeList);
  check_ids(nodes, nodePointer.device(), "nodes"); check_ids(new_id, nodePointer.device(), "new_id");
  const int64_t N = nodePointer.numel() - 1, E = edgeList.numel(), M = nodes.numel();
  TORCH_CHECK(new_id.numel() == N, "new_id must hold one entry per node");
  TORCH_CHECK(M <= N, "nodes holds more entries than the graph has nodes");
  DeviceGuard guard(nodePointer.device());
  void* stream = current_stream(nodePointer);
  size_t need = 0;
  tcgnn_check(tcgnn_induce_workspace_bytes((int32_t)M, &need), "tcgnn_induce_workspace_bytes");
  torch::Tensor ws = torch::empty({(int64_t)need + 256}, nodePointer.options().dtype(torch::kUInt8));
  char* wsp = static_cast<char*>(ws.data_ptr());
  wsp += (256 - reinterpret_cast<uintptr_t>(wsp) % 256) % 256;
  const int* col = E ? edgeList.data_ptr<int>() : nullptr;
  const int* list = M ? nodes.data_ptr<int>() : nullptr;
  const int* ids = N ? new_id.data_ptr<int>() : nullptr;
  torch::Tensor rp_b = torch::empty({M + 1}, nodePointer.options());
  int64_t kept = 0;
  tcgnn_check(tcgnn_induce_count(nodePointer.data_ptr<int>(), col, list, ids, (int32_t)M, (int32_t)N, E, rp_b.data_ptr<int>(), wsp, need, &kept, stream),
              "tcgnn_induce_count");
  torch::Tensor col_b = torch::empty({kept}, edgeList.options()), eid = torch::empty({kept}, edgeList.options());
  if (kept > 0)
    tcgnn_check(tcgnn_induce(nodePointer.data_ptr<int>(), col, list, ids, rp_b.data_ptr<int>(), (int32_t)M, (int32_t)N, E, kept, col_b.data_ptr<int>(),
                             eid.data_ptr<int>(), stream), "tcgnn_induce");
  return {rp_b, col_b, eid};
}

// Not in the reference: the normalised GCN aggregation, Y = act(row_scale * (A @ (col_scale * X')) + bias) (tcgnn_spmm_scaled;
// TCGNN.forward_scaled of the ctypes module).  Every optional tensor is fp32, contiguous and on input's device; the error names it.
std::vector<torch::Tensor> spmm_forward_scaled(torch::Tensor input, torch::Tensor nodePointer, torch::Tensor edgeList,
                                               torch::Tensor blockPartition, torch::Tensor edgeToColumn, torch::Tensor edgeToRow,
                                               c10::optional<torch::Tensor> row_scale, c10::optional<torch::Tensor> col_scale,
                                               c10::optional<torch::Tensor> bias, bool relu, c10::optional<torch::Tensor> gate, bool transpose) {
  CHECK_INPUT(input); CHECK_INPUT(nodePointer); CHECK_INPUT(edgeList);
  CHECK_INPUT(blockPartition); CHECK_INPUT(edgeToColumn); CHECK_INPUT(edgeToRow);
  TORCH_CHECK(input.scalar_type() == torch::kFloat32, "expected scalar type Float");
  check_rows(input, nodePointer);
  const int64_t N = input.size(0), D = input.size(1);
  auto opt = [&](const c10::optional<torch::Tensor>& t, const char* name, int64_t n) -> const float* {
    if (!t.has_value()) return nullptr;
    TORCH_CHECK(t->is_cuda(), name, " must be a CUDA tensor");
    TORCH_CHECK(t->is_contiguous(), name, " must be contiguous");
    TORCH_CHECK(t->scalar_type() == torch::kFloat32, name, ": expected scalar type Float");
    TORCH_CHECK(t->device() == input.device(), name, " is not on input's device");
    if (n >= 0) {
      TORCH_CHECK(t->dim() == 1 && t->numel() == n, name, " must be a 1-D tensor of ", n, " elements");
    } else {
      TORCH_CHECK(t->sizes() == input.sizes(), name, " must have the shape of input");
    }
    return t->data_ptr<float>();
  };
  const float* rs = opt(row_scale, "row_scale", N);
  const float* cs = opt(col_scale, "col_scale", N);
  const float* b = opt(bias, "bias", D);
  const float* g = opt(gate, "gate", -1);
  DeviceGuard guard(input.device());
  auto output = torch::empty_like(input);
  if (input.numel() == 0) return {output};
  auto* plan = plan_of(entry_for(nodePointer, edgeList, blockPartition, edgeToColumn, edgeToRow), transpose);
  Workspace ws(plan, (int)D, input);
  tcgnn_check(tcgnn_spmm_scaled(plan, input.data_ptr<float>(), cs, g, rs, b, output.data_ptr<float>(), (int)D, relu ? TCGNN_FUSE_RELU : 0,
                                ws.ptr, ws.bytes, current_stream(input)), "tcgnn_spmm_scaled");
  return {output};
}

// TCGNN.cpp:172-226: host tensors, outputs written in place, two lines on C stdout
void preprocess(torch::Tensor edgeList, torch::Tensor nodePointer, int num_nodes, int blockSize_h, int blockSize_w,
                torch::Tensor blockPartition, torch::Tensor edgeToColumn, torch::Tensor edgeToRow) {
  for (auto* t : {&edgeList, &nodePointer, &blockPartition, &edgeToColumn, &edgeToRow}) {
    TORCH_CHECK(!t->is_cuda(), "preprocess takes CPU tensors (preprocess_gpu takes device tensors)");
    TORCH_CHECK(t->is_contiguous(), "metadata tensors must be contiguous");
    TORCH_CHECK(t->scalar_type() == torch::kInt32, "expected scalar type Int");
  }
  TORCH_CHECK(nodePointer.numel() >= (int64_t)num_nodes + 1, "nodePointer must hold num_nodes + 1 entries");
  const int64_t E = nodePointer.data_ptr<int>()[num_nodes];
  TORCH_CHECK(edgeList.numel() >= E && edgeToColumn.numel() >= E && edgeToRow.numel() >= E, "edge arrays are shorter than nodePointer[num_nodes]");
  int64_t tc_blocks = 0;
  tcgnn_check(tcgnn_preprocess(edgeList.data_ptr<int>(), nodePointer.data_ptr<int>(), num_nodes, blockSize_h, blockSize_w,
                               blockPartition.data_ptr<int>(), blockPartition.numel(), edgeToColumn.data_ptr<int>(),
                               edgeToRow.data_ptr<int>(), &tc_blocks, 0), "tcgnn_preprocess");
  printf("TC_Blocks:\t%lld\nExp_Edges:\t%lld\n", (long long)tc_blocks, (long long)tc_blocks * 8 * 16);   // TCGNN.cpp:225
  fflush(stdout);
}

// TCGNN.cpp:229-256 (a stub in the reference: fill_window is empty, TCGNN_kernel.cu:42-80)
void preprocess_gpu(torch::Tensor edgeList, torch::Tensor nodePointer, int num_nodes, int blockSize_h, int blockSize_w,
                    torch::Tensor blockPartition, torch::Tensor edgeToColumn, torch::Tensor edgeToRow) {
  CHECK_INPUT(edgeList); CHECK_INPUT(nodePointer); CHECK_INPUT(blockPartition); CHECK_INPUT(edgeToColumn); CHECK_INPUT(edgeToRow);
  for (auto* t : {&edgeList, &nodePointer, &blockPartition, &edgeToColumn, &edgeToRow})
    TORCH_CHECK(t->scalar_type() == torch::kInt32, "expected scalar type Int");
  TORCH_CHECK(nodePointer.numel() >= (int64_t)num_nodes + 1, "nodePointer must hold num_nodes + 1 entries");
  TORCH_CHECK(edgeToColumn.numel() >= edgeList.numel() && edgeToRow.numel() >= edgeList.numel(), "edgeToColumn / edgeToRow are shorter than edgeList");
  DeviceGuard guard(edgeList.device());
  int64_t tc_blocks = 0;
  // scratch from torch's caching allocator: the library call allocates nothing and synchronises once (tcgnn_preprocess_gpu_ws)
  size_t need = 0;
  tcgnn_check(tcgnn_preprocess_gpu_workspace_bytes(num_nodes, edgeList.numel(), blockSize_h, &need), "tcgnn_preprocess_gpu_workspace_bytes");
  torch::Tensor ws = torch::empty({(int64_t)std::max<size_t>(need, 256)}, torch::TensorOptions().dtype(torch::kUInt8).device(edgeList.device()));
  tcgnn_check(tcgnn_preprocess_gpu_ws(edgeList.data_ptr<int>(), nodePointer.data_ptr<int>(), num_nodes, edgeList.numel(), blockSize_h, blockSize_w,
                                      blockPartition.data_ptr<int>(), blockPartition.numel(), edgeToColumn.data_ptr<int>(),
                                      edgeToRow.data_ptr<int>(), ws.data_ptr(), (size_t)ws.numel(), &tc_blocks, current_stream(edgeList)), "tcgnn_preprocess_gpu_ws");
  printf("TC_Blocks:\t%lld\nExp_Edges:\t%lld\n", (long long)tc_blocks, (long long)tc_blocks * 8 * 16);
  fflush(stdout);
}

void clear_plan_cache() {
  for (auto& e : plan_cache()) {
    if (!e.keep.empty() && e.keep[0].is_cuda()) { DeviceGuard guard(e.keep[0].device()); (void)hipDeviceSynchronize(); }   // nothing may still be reading the plan
    destroy_entry(e);
  }
  plan_cache().clear();
  csr_cache().clear();
}

// TCGNN.cpp:260-272
PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("preprocess", &preprocess, "Preprocess Step (CPU)");
  m.def("preprocess_gpu", &preprocess_gpu, "Preprocess Step (CUDA)");
  // (transpose: not in the reference - A^T in place of A, the metadata still describing A)
  m.def("forward", &spmm_forward, "TC-GNN SPMM forward (CUDA)", py::arg("input"), py::arg("nodePointer"), py::arg("edgeList"),
        py::arg("blockPartition"), py::arg("edgeToColumn"), py::arg("edgeToRow"), py::arg("transpose") = false);
  m.def("forward_ef", &sddmm_forward, "TC-GNN SDDMM forward (CUDA)");
  m.def("forward_AGNN", &spmm_forward_AGNN, "TC-GNN SPMM (AGNN) forward (CUDA)", py::arg("input"), py::arg("nodePointer"), py::arg("edgeList"),
        py::arg("edgeAttention"), py::arg("blockPartition"), py::arg("edgeToColumn"), py::arg("edgeToRow"), py::arg("transpose") = false);
  m.def("forward_heads", &spmm_forward_heads, "edge-valued SpMM for every head at once (not in the reference)", py::arg("input"), py::arg("nodePointer"),
        py::arg("edgeList"), py::arg("edgeAttention"), py::arg("blockPartition"), py::arg("edgeToColumn"), py::arg("edgeToRow"), py::arg("heads"),
        py::arg("transpose") = false);
  m.def("backward", &spmm_forward, "TC-GNN SPMM backward (CUDA)", py::arg("input"), py::arg("nodePointer"), py::arg("edgeList"),
        py::arg("blockPartition"), py::arg("edgeToColumn"), py::arg("edgeToRow"), py::arg("transpose") = false);
  m.def("backward_ef", &sddmm_forward, "TC-GNN SDDMM backward (CUDA)");
  m.def("clear_plan_cache", &clear_plan_cache, "release the device plans (not in the reference)");
  m.def("forward_scaled", &spmm_forward_scaled, "normalised GCN aggregation with scales / bias / ReLU fused (not in the reference)",
        py::arg("input"), py::arg("nodePointer"), py::arg("edgeList"), py::arg("blockPartition"), py::arg("edgeToColumn"), py::arg("edgeToRow"),
        py::arg("row_scale") = py::none(), py::arg("col_scale") = py::none(), py::arg("bias") = py::none(), py::arg("relu") = false,
        py::arg("gate") = py::none(), py::arg("transpose") = false);
  m.def("forward_ef2", &sddmm2_forward, "SDDMM with two operands, ef[e] = <X[row e], Z[col e]> (not in the reference)");
  m.def("forward_ef_heads", &sddmm_heads_forward, "two-operand SDDMM for every head at once, ef[heads, E] (not in the reference)", py::arg("X"), py::arg("Z"),
        py::arg("nodePointer"), py::arg("edgeList"), py::arg("blockPartition"), py::arg("edgeToColumn"), py::arg("edgeToRow"), py::arg("heads"));
  m.def("edge_softmax", &edge_softmax,"softmax over every node's incoming edges (not in the reference)", py::arg("score"), py::arg("nodePointer"),
        py::arg("beta") = py::none(), py::arg("out") = py::none());
  m.def("edge_softmax_backward", &edge_softmax_backward, "backward of edge_softmax: (ds, dbeta) (not in the reference)", py::arg("p"), py::arg("dp"),
        py::arg("nodePointer"), py::arg("beta") = py::none(), py::arg("score") = py::none(), py::arg("need_dbeta") = false, py::arg("out") = py::none());
  m.def("gat_softmax", &gat_softmax, "multi-head GAT attention, p[heads, E] (not in the reference)", py::arg("el"), py::arg("er"), py::arg("nodePointer"),
        py::arg("edgeList"), py::arg("negative_slope") = 0.2, py::arg("out") = py::none());
  m.def("gat_softmax_backward", &gat_softmax_backward, "backward of gat_softmax: (ds, d_er) (not in the reference)", py::arg("p"), py::arg("dp"),
        py::arg("el"), py::arg("er"), py::arg("nodePointer"), py::arg("edgeList"), py::arg("negative_slope") = 0.2, py::arg("out") = py::none());
  m.def("edge_colsum", &edge_colsum, "per-source-node sums of per-edge values, [N, heads] (not in the reference)", py::arg("val"), py::arg("nodePointer"),
        py::arg("edgeList"));
  m.def("forward_max", &forward_max, "element-wise maximum over every node's incoming edges: (Y, arg) (not in the reference)", py::arg("input"),
        py::arg("nodePointer"), py::arg("edgeList"), py::arg("return_arg") = true, py::arg("out") = py::none());
  m.def("backward_max", &backward_max, "backward of forward_max: dX (not in the reference)", py::arg("dY"), py::arg("arg"), py::arg("nodePointer"),
        py::arg("edgeList"), py::arg("out") = py::none());
  m.def("forward_stats", &forward_stats, "mean / std / max / min over every node's incoming edges in one walk: a dict (not in the reference)",
        py::arg("input"), py::arg("nodePointer"), py::arg("edgeList"), py::arg("aggregators") = std::vector<std::string>{"mean", "std", "max", "min"},
        py::arg("eps") = 1e-5, py::arg("return_arg") = true);
  m.def("backward_stats", &backward_stats, "backward of forward_stats: dZ (not in the reference)", py::arg("grads"), py::arg("saved"),
        py::arg("nodePointer"), py::arg("edgeList"), py::arg("out") = py::none());
  m.def("gatv2_softmax", &gatv2_softmax, "GATv2 attention, p[heads, E] (not in the reference)", py::arg("xl"), py::arg("xr"), py::arg("attn"),
        py::arg("nodePointer"), py::arg("edgeList"), py::arg("negative_slope") = 0.2, py::arg("out") = py::none(), py::arg("score_out") = py::none());
  m.def("gatv2_softmax_backward", &gatv2_softmax_backward, "row side of gatv2_softmax's backward: (g, d_xr, d_attn) (not in the reference)", py::arg("p"),
        py::arg("dp"), py::arg("xl"), py::arg("xr"), py::arg("attn"), py::arg("nodePointer"), py::arg("edgeList"), py::arg("negative_slope") = 0.2,
        py::arg("out") = py::none());
  m.def("gatv2_source_grad", &gatv2_source_grad, "source side of gatv2_softmax's backward: d_xl (not in the reference)", py::arg("g"), py::arg("xl"),
        py::arg("xr"), py::arg("attn"), py::arg("nodePointer"), py::arg("edgeList"), py::arg("negative_slope") = 0.2);
  m.def("forward_ue", &forward_ue, "sum over a node's incoming edges of act(X[col e] + Ef[e]), Ef [E, D] (not in the reference)", py::arg("X"), py::arg("Ef"),
        py::arg("nodePointer"), py::arg("edgeList"), py::arg("act") = "relu", py::arg("out") = py::none());
  m.def("backward_ue", &backward_ue, "per-edge gradient of forward_ue: dM [E, D] (not in the reference)", py::arg("dY"), py::arg("X"), py::arg("Ef"),
        py::arg("nodePointer"), py::arg("edgeList"), py::arg("act") = "relu", py::arg("out") = py::none());
  m.def("edge_sum", &edge_sum, "per-edge rows summed into nodes, optionally through perm (not in the reference)", py::arg("M"), py::arg("nodePointer"),
        py::arg("perm") = py::none(), py::arg("out") = py::none());
  m.def("sample_neighbors", &sample_neighbors, "seeded fan-out sampling over the same nodes: (nodePointer_s, edgeList_s, eid) (not in the reference)",
        py::arg("nodePointer"), py::arg("edgeList"), py::arg("fanout"), py::arg("seed"), py::arg("row_mask") = py::none());
  m.def("compact_nodes", &compact_nodes, "the node set of one mini-batch's layer graphs: (nodes, new_id) (not in the reference)", py::arg("graphs"),
        py::arg("keep") = py::none());
  m.def("compact_graph", &compact_graph, "a graph over the nodes of compact_nodes: (nodePointer_b, edgeList_b) (not in the reference)",
        py::arg("nodePointer"), py::arg("edgeList"), py::arg("nodes"), py::arg("new_id"));
  m.def("sample_rows", &sample_rows, "sample_neighbors from a list of row ids: (rowPointer_s, edgeList_s, eid) (not in the reference)",
        py::arg("nodePointer"), py::arg("edgeList"), py::arg("rows"), py::arg("fanout"), py::arg("seed"));
  m.def("extend_nodes", &extend_nodes, "marks ids into the uint8 mask in place: (nodes, new_id) of the mask afterwards (not in the reference)",
        py::arg("keep"), py::arg("ids"));
  m.def("compact_rows_graph", &compact_rows_graph, "the block of a sample_rows graph over the nodes of extend_nodes: (nodePointer_b, edgeList_b) "
        "(not in the reference)", py::arg("rows"), py::arg("rowPointer_s"), py::arg("edgeList_s"), py::arg("nodes"), py::arg("new_id"));
  m.def("random_walk", &random_walk, "one seeded random walk per start, towards a row's sources: walks [W, length + 1] (not in the reference)",
        py::arg("nodePointer"), py::arg("edgeList"), py::arg("starts"), py::arg("length"), py::arg("seed"));
  m.def("induce_subgraph", &induce_subgraph, "the subgraph induced on the nodes of extend_nodes: (nodePointer_b, edgeList_b, eid) (not in the reference)",
        py::arg("nodePointer"), py::arg("edgeList"), py::arg("nodes"), py::arg("new_id"));
  m.def("transpose_graph", &transpose_graph, "the cached CSR of A^T: (nodePointer_t, edgeList_t, perm, symmetric) (not in the reference)",
        py::arg("nodePointer"), py::arg("edgeList"));
}
