// Graph plan on the device: the CSR views pdg/plan.py builds with torch.sort / bincount /
// searchsorted, built here without a host read.
//
//   pdg_graph_plan  edge_index -> dst-sorted edges (perm, src, dst, rowptr_dst) and their
//                   grouping by source (perm_src, rowptr_src)            (plan.py GraphPlan.__init__)
//   pdg_div_plan    COO divergence operator -> CSR by row (a_*) and CSR^T by global node (at_*),
//                   columns beyond 2 N_g of the row's graph dropped      (plan.py _build_div)
//
// One routine does all four groupings: "group items by a major key, order a group by
// (minor key, item position)".  A histogram of the major keys (atomics), the exclusive scan of
// pdg_scan.hpp (it becomes the row pointer), an atomic fill of packed 64-bit slots
// (minor << 32 | position) into the rows in any order, then every row is sorted by itself and
// written out.  Slots of a row are distinct (positions are), so the sorted order is total:
// the result does not depend on the atomics' order and is the stable sort torch computes.
//
// Rows are sorted by their length:
//   <= SHORT_MAX slots  one thread, insertion sort (mesh rows hold ~6-14 slots);
//   <= TILE_MAX slots   one workgroup, bitonic network in LDS;
//   longer              one workgroup, the same network on the row in global memory.
// The network is the all-ascending form (a "flip" step i <-> i ^ (k - 1), then "disperse"
// steps i <-> i ^ j), so slots past the row's end behave as +inf without being stored and a
// row of any length m costs O(m log^2 m / 256) per thread: a hub node never becomes an
// O(m^2) loop in one thread.
//
// An endpoint outside [0, n_nodes) sets *status and is treated as node 0; a divergence entry
// whose row, graph or node cannot be indexed sets *status and is dropped.  No kernel indexes
// with an unchecked value, so every output is a valid in-range plan whatever the input.
// Counters and *status are cleared by a kernel (no memset node on a path that may be captured).
#include <stdint.h>

#include <algorithm>

#include "pdg_runtime.hpp"
#include "pdg_scan.hpp"

using namespace pdg;

namespace {

typedef unsigned long long u64;

constexpr int PT = 256;            // threads per block
constexpr int SHORT_MAX = 32;      // longest row one thread sorts by insertion
constexpr int TILE_MAX = 2048;     // longest row sorted in LDS (16 KB of slots)

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

int grid_for(long work) {
  long g = (work + PT - 1) / PT;
  const long cap = (long)device_cus() * 8;
  return (int)(g < 1 ? 1 : g > cap ? cap : g);
}

__global__ __launch_bounds__(PT) void clear_kernel(int* __restrict__ a, long na, int* __restrict__ b, long nb,
                                                   int* __restrict__ c, long nc, int* __restrict__ status) {
  const long stride = (long)gridDim.x * PT;
  const long t0 = (long)blockIdx.x * PT + threadIdx.x;
  for (long i = t0; i < na; i += stride) a[i] = 0;
  for (long i = t0; i < nb; i += stride) b[i] = 0;
  for (long i = t0; i < nc; i += stride) c[i] = 0;
  if (status && t0 == 0) *status = 0;
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

// ---------------------------------------------------------------------------- the grouping
// Slot of item i in its row: rowptr[major] + (arrival order).  The count kernels took the same
// item() decisions, so a row never receives more slots than the scan reserved for it.
template <class P>
__global__ __launch_bounds__(PT) void fill_kernel(P p, long m, const int* __restrict__ rowptr, int* __restrict__ fill,
                                                  u64* __restrict__ slots) {
  for (long i = (long)blockIdx.x * PT + threadIdx.x; i < m; i += (long)gridDim.x * PT) {
    int major;
    unsigned minor;
    if (p.item(i, major, minor))
      slots[(long)rowptr[major] + atomicAdd(&fill[major], 1)] = ((u64)minor << 32) | (u64)(unsigned)i;
  }
}

__device__ __forceinline__ void cswap(u64* a, long i, long l) {
  const u64 x = a[i], y = a[l];
  if (x > y) {
    a[i] = y;
    a[l] = x;
  }
}

// Ascending sort of a[0..m) by the whole workgroup (a in LDS or in global memory).  Bitonic
// network over the next power of two with every comparator ascending; a comparator whose upper
// end is past m is skipped (that end is +inf and stays).
__device__ void block_sort(u64* a, long m) {
  long np2 = 1;
  while (np2 < m) np2 <<= 1;
  const long half = np2 >> 1;
  for (long k = 2; k <= np2; k <<= 1) {
    const long hk = k >> 1;
    for (long t = threadIdx.x; t < half; t += PT) {            // flip: i <-> i ^ (k - 1)
      const long lowb = t & (hk - 1);
      const long i = (t - lowb) * 2 + lowb;
      const long l = i ^ (k - 1);
      if (l < m) cswap(a, i, l);
    }
    __syncthreads();
    for (long j = k >> 2; j > 0; j >>= 1) {                    // disperse: i <-> i + j
      for (long t = threadIdx.x; t < half; t += PT) {
        const long lowb = t & (j - 1);
        const long i = (t - lowb) * 2 + lowb;
        const long l = i + j;
        if (l < m) cswap(a, i, l);
      }
      __syncthreads();
    }
  }
}

// Sort every row's slots and write the row out.  A block takes PT consecutive rows at a time:
// each thread sorts its own row when it is short, the long rows of the chunk are listed in LDS
// and sorted one after the other by the whole block.
template <class P>
__global__ __launch_bounds__(PT) void sort_emit_kernel(P p, int n, const int* __restrict__ rowptr,
                                                       u64* slots) {
  __shared__ u64 tile[TILE_MAX];
  __shared__ int longrow[PT];
  __shared__ int nlong;
  for (long base = (long)blockIdx.x * PT; base < n; base += (long)gridDim.x * PT) {
    if (threadIdx.x == 0) nlong = 0;
    __syncthreads();
    const long r = base + threadIdx.x;
    if (r < n) {
      const long b = rowptr[r];
      const int m = rowptr[r + 1] - rowptr[r];
      if (m > SHORT_MAX) {
        longrow[atomicAdd(&nlong, 1)] = (int)r;
      } else {
        u64* a = slots + b;
        for (int i = 1; i < m; ++i) {
          const u64 x = a[i];
          int j = i - 1;
          while (j >= 0 && a[j] > x) {
            a[j + 1] = a[j];
            --j;
          }
          a[j + 1] = x;
        }
        for (int i = 0; i < m; ++i) p.emit(b + i, (int)r, a[i]);
      }
    }
    __syncthreads();
    const int nl = nlong;
    for (int q = 0; q < nl; ++q) {
      const int row = longrow[q];
      const long b = rowptr[row];
      const long m = rowptr[row + 1] - rowptr[row];
      u64* a = slots + b;
      if (m <= TILE_MAX) {
        for (long i = threadIdx.x; i < m; i += PT) tile[i] = a[i];
        __syncthreads();
        block_sort(tile, m);
        for (long i = threadIdx.x; i < m; i += PT) p.emit(b + i, row, tile[i]);
      } else {
        block_sort(a, m);
        for (long i = threadIdx.x; i < m; i += PT) p.emit(b + i, row, a[i]);
      }
      __syncthreads();
    }
  }
}

template <class P>
void group(const P& p, long m, int n, int* rowptr, int* fill, const Scratch& s, hipStream_t st) {
  scan(n, rowptr, s.bsum, st);
  if (m == 0) return;
  hipLaunchKernelGGL(fill_kernel<P>, dim3(grid_for(m)), dim3(PT), 0, st, p, m, rowptr, fill, s.slots);
  hipLaunchKernelGGL(sort_emit_kernel<P>, dim3(grid_for(n)), dim3(PT), 0, st, p, n, rowptr, s.slots);
}

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
  group(ByDst{edge_src, edge_dst, n_nodes, perm, src, dst}, n_edges, n_nodes, rowptr_dst, s.fill, s, st);
  group(BySrc{src, dst, perm_src}, n_edges, n_nodes, rowptr_src, s.fill + n_nodes, s, st);
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
  group(DivByRow{d, a_col, a_val}, nnz, n_nodes, a_rowptr, s.fill, s, st);
  group(DivByNode{d, at_row, at_comp, at_val}, nnz, n_nodes, at_rowptr, s.fill + n_nodes, s, st);
  PDG_CHECK_LAUNCH("pdg_div_plan");
  return PDG_OK;
}
