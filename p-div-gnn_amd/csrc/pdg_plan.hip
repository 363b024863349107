// Graph plan on the device: the CSR views pdg/plan.py builds with torch.sort / bincount /
// searchsorted, built here without a host read.
//
//   pdg_graph_plan  edge_index -> dst-sorted edges (perm, src, dst, rowptr_dst) and their
//                   grouping by source (perm_src, rowptr_src)            (plan.py GraphPlan.__init__)
//   pdg_div_plan    COO divergence operator -> CSR by row (a_*) and CSR^T by global node (at_*),
//                   columns beyond 2 N_g of the row's graph dropped      (plan.py _build_div)
//
// One routine (pdg_group.hpp) does all four groupings: "group items by a major key, order a
// group by (minor key, item position)" -- a histogram of the major keys, the exclusive scan of
// pdg_scan.hpp, an atomic fill of packed 64-bit slots and a sort of every row by itself.  The
// result does not depend on the atomics' order and is the stable sort torch computes.
//
// An endpoint outside [0, n_nodes) sets *status and is treated as node 0; a divergence entry
// whose row, graph or node cannot be indexed sets *status and is dropped.  No kernel indexes
// with an unchecked value, so every output is a valid in-range plan whatever the input.
// Counters and *status are cleared by a kernel (no memset node on a path that may be captured).
#include <stdint.h>

#include <algorithm>

#include "pdg_group.hpp"
#include "pdg_runtime.hpp"
#include "pdg_scan.hpp"

using namespace pdg;

namespace {

struct Scratch {
  int* fill;     // [2][N] per-row fill counters of the two groupings
  int* bsum;     // [scan blocks + 2]
  u64* slots;    // [max(E, nnz)]
};

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

size_t layout(int n, long m, Scratch* s, char* base) {
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + o : nullptr;
    o += align_up(bytes);
    return p;
  };
  int* fill = (int*)take(sizeof(int) * 2 * (size_t)n);
  int* bsum = (int*)take(sizeof(int) * scan_bsum_len(n));
  u64* slots = (u64*)take(sizeof(u64) * (size_t)std::max<long>(m, 1));
  if (s) *s = Scratch{fill, bsum, slots};
  return o;
}

// ------------------------------------------------------------------------------------ edges
__device__ __forceinline__ int endpoint(int64_t v, int n, int& bad) {
  if (v < 0 || v >= n) {
    bad = 1;
    return 0;
  }
  return (int)v;
}

__global__ __launch_bounds__(PT) void edge_count_kernel(long m, const int64_t* __restrict__ es,
                                                        const int64_t* __restrict__ ed, int n,
                                                        int* __restrict__ cnt_dst, int* __restrict__ cnt_src,
                                                        int* __restrict__ status) {
  int bad = 0;
  for (long i = (long)blockIdx.x * PT + threadIdx.x; i < m; i += (long)gridDim.x * PT) {
    atomicAdd(&cnt_dst[endpoint(ed[i], n, bad)], 1);
    atomicAdd(&cnt_src[endpoint(es[i], n, bad)], 1);
  }
  if (bad) atomicOr(status, 1);
}

// The input edges grouped by destination, a group ordered by (source, edge id).
struct ByDst {
  const int64_t* es;
  const int64_t* ed;
  int n;
  int* perm;
  int* src;
  int* dst;
  __device__ bool item(long i, int& major, unsigned& minor) const {
    int bad = 0;
    major = endpoint(ed[i], n, bad);
    minor = (unsigned)endpoint(es[i], n, bad);
    return true;
  }
  __device__ void emit(long k, int row, u64 slot) const {
    perm[k] = (int)(slot & 0xffffffffu);
    src[k] = (int)(slot >> 32);
    dst[k] = row;
  }
};

// The dst-sorted edges grouped by source, a group ordered by (destination, sorted position).
struct BySrc {
  const int* src;
  const int* dst;
  int* perm_src;
  __device__ bool item(long i, int& major, unsigned& minor) const {
    major = src[i];
    minor = (unsigned)dst[i];
    return true;
  }
  __device__ void emit(long k, int, u64 slot) const { perm_src[k] = (int)(slot & 0xffffffffu); }
};

// ------------------------------------------------------------------------------- divergence
struct DivIn {
  const int64_t* rows;
  const int64_t* cols;
  const float* vals;
  const int* ptr;   // [ng + 1] node offsets of the graphs
  int ng;
  int n;
};

// Entry i of the COO operator: its graph g = searchsorted(ptr, row, right=True) - 1, kept when
// col < 2 N_g (gnn_train.py:74); node = ptr[g] + (col mod N_g), comp = col >= N_g.
__device__ __forceinline__ bool div_entry(const DivIn& d, long i, int& row, int& node, int& comp, int& bad) {
  const int64_t r = d.rows[i], c = d.cols[i];
  if (r < 0 || r >= d.n || c < 0) {
    bad = 1;
    return false;
  }
  int lo = 0, hi = d.ng + 1;          // number of ptr entries <= r
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (d.ptr[mid] <= r) lo = mid + 1;
    else hi = mid;
  }
  const int g = lo - 1;
  if (g < 0 || g >= d.ng) {
    bad = 1;
    return false;
  }
  const int off = d.ptr[g], ngn = d.ptr[g + 1] - off;
  if (c >= 2 * (int64_t)ngn) return false;   // the reference's [:, :2N_i] slice, not an error
  comp = c >= ngn;
  const int64_t v = off + (comp ? c - ngn : c);
  if (v < 0 || v >= d.n) {
    bad = 1;
    return false;
  }
  row = (int)r;
  node = (int)v;
  return true;
}

__global__ __launch_bounds__(PT) void div_count_kernel(long m, DivIn d, int* __restrict__ cnt_row,
                                                       int* __restrict__ cnt_node, int* __restrict__ status) {
  int bad = 0;
  for (long i = (long)blockIdx.x * PT + threadIdx.x; i < m; i += (long)gridDim.x * PT) {
    int row, node, comp;
    if (div_entry(d, i, row, node, comp, bad)) {
      atomicAdd(&cnt_row[row], 1);
      atomicAdd(&cnt_node[node], 1);
    }
  }
  if (bad) atomicOr(status, 1);
}

// Kept entries grouped by row, a group in entry order (the COO need not be coalesced).
struct DivByRow {
  DivIn d;
  int* a_col;
  float* a_val;
  __device__ bool item(long i, int& major, unsigned& minor) const {
    int node, comp, bad = 0;
    minor = 0;
    return div_entry(d, i, major, node, comp, bad);
  }
  __device__ void emit(long k, int, u64 slot) const {
    const long i = (long)(slot & 0xffffffffu);
    a_col[k] = (int)d.cols[i];
    a_val[k] = d.vals[i];
  }
};

// Kept entries grouped by global node (the transpose), a group in entry order.
struct DivByNode {
  DivIn d;
  int* at_row;
  int* at_comp;
  float* at_val;
  __device__ bool item(long i, int& major, unsigned& minor) const {
    int row, comp, bad = 0;
    minor = 0;
    return div_entry(d, i, row, major, comp, bad);
  }
  __device__ void emit(long k, int, u64 slot) const {
    const long i = (long)(slot & 0xffffffffu);
    int row = 0, node, comp = 0, bad = 0;
    div_entry(d, i, row, node, comp, bad);   // kept once, so kept again: row and comp are set
    at_row[k] = row;
    at_comp[k] = comp;
    at_val[k] = d.vals[i];
  }
};

bool sizes_ok(int n_nodes, long m) {
  // the scan indexes base + i < n + SCAN_BLOCK in int32
  return n_nodes > 0 && m >= 0 && m < 0x7fffffffL && (long)n_nodes + SCAN_BLOCK < 0x7fffffffL;
}

}  // namespace

extern "C" long pdg_graph_plan_scratch_bytes(int n_nodes, long n_edges, long nnz) {
  if (!sizes_ok(n_nodes, n_edges) || !sizes_ok(n_nodes, nnz)) return -1;
  return (long)layout(n_nodes, std::max(n_edges, nnz), nullptr, nullptr);
}

extern "C" int pdg_graph_plan(int n_nodes, long n_edges, const int64_t* edge_src, const int64_t* edge_dst, int* perm,
                              int* src, int* dst, int* rowptr_dst, int* perm_src, int* rowptr_src, int* status,
                              void* scratch, long scratch_bytes, void* stream) {
  PDG_CHECK_ARG(sizes_ok(n_nodes, n_edges),
                "pdg_graph_plan: bad sizes (n_nodes > 0, 0 <= n_edges < 2^31, n_nodes + 1024 < 2^31)");
  PDG_CHECK_ARG(rowptr_dst && rowptr_src && status && scratch, "pdg_graph_plan: null argument");
  PDG_CHECK_ARG(n_edges == 0 || (edge_src && edge_dst && perm && src && dst && perm_src),
                "pdg_graph_plan: null argument");
  PDG_CHECK_ARG(scratch_bytes >= (long)layout(n_nodes, n_edges, nullptr, nullptr), "pdg_graph_plan: scratch too small");
  hipStream_t st = (hipStream_t)stream;
  Scratch s;
  layout(n_nodes, n_edges, &s, (char*)scratch);
  const long n1 = (long)n_nodes + 1;
  hipLaunchKernelGGL(clear_kernel, dim3(grid_for(n1)), dim3(PT), 0, st, rowptr_dst, n1, rowptr_src, n1, s.fill,
                     2L * n_nodes, status);
  if (n_edges > 0)
    hipLaunchKernelGGL(edge_count_kernel, dim3(grid_for(n_edges)), dim3(PT), 0, st, n_edges, edge_src, edge_dst,
                       n_nodes, rowptr_dst, rowptr_src, status);
  group(ByDst{edge_src, edge_dst, n_nodes, perm, src, dst}, n_edges, n_nodes, rowptr_dst, s.fill, s.bsum, s.slots, st);
  group(BySrc{src, dst, perm_src}, n_edges, n_nodes, rowptr_src, s.fill + n_nodes, s.bsum, s.slots, st);
  PDG_CHECK_LAUNCH("pdg_graph_plan");
  return PDG_OK;
}

extern "C" int pdg_div_plan(int n_nodes, int n_graphs, const int* ptr, long nnz, const int64_t* rows,
                            const int64_t* cols, const float* vals, int* a_rowptr, int* a_col, float* a_val,
                            int* at_rowptr, int* at_row, int* at_comp, float* at_val, int* status, int clear_status,
                            void* scratch, long scratch_bytes, void* stream) {
  PDG_CHECK_ARG(sizes_ok(n_nodes, nnz) && n_graphs > 0,
                "pdg_div_plan: bad sizes (n_nodes > 0, n_graphs > 0, 0 <= nnz < 2^31, n_nodes + 1024 < 2^31)");
  PDG_CHECK_ARG(ptr && a_rowptr && at_rowptr && status && scratch, "pdg_div_plan: null argument");
  PDG_CHECK_ARG(nnz == 0 || (rows && cols && vals && a_col && a_val && at_row && at_comp && at_val),
                "pdg_div_plan: null argument");
  PDG_CHECK_ARG(scratch_bytes >= (long)layout(n_nodes, nnz, nullptr, nullptr), "pdg_div_plan: scratch too small");
  hipStream_t st = (hipStream_t)stream;
  Scratch s;
  layout(n_nodes, nnz, &s, (char*)scratch);
  const long n1 = (long)n_nodes + 1;
  hipLaunchKernelGGL(clear_kernel, dim3(grid_for(n1)), dim3(PT), 0, st, a_rowptr, n1, at_rowptr, n1, s.fill,
                     2L * n_nodes, clear_status ? status : nullptr);
  const DivIn d{rows, cols, vals, ptr, n_graphs, n_nodes};
  if (nnz > 0)
    hipLaunchKernelGGL(div_count_kernel, dim3(grid_for(nnz)), dim3(PT), 0, st, nnz, d, a_rowptr, at_rowptr, status);
  group(DivByRow{d, a_col, a_val}, nnz, n_nodes, a_rowptr, s.fill, s.bsum, s.slots, st);
  group(DivByNode{d, at_row, at_comp, at_val}, nnz, n_nodes, at_rowptr, s.fill + n_nodes, s.bsum, s.slots, st);
  PDG_CHECK_LAUNCH("pdg_div_plan");
  return PDG_OK;
}
