// Mesh graph construction on the device: the "with preprocessing"
// path of the reference (benchmark_gnn_fem.py:388-415, datasets.py:247-263):
//   mesh_to_graph     (convert_utils.py:47-81, PyG FaceToEdge: the 3 edges of every
//                      triangle in both directions, coalesced; _quad_face_to_edge: the 4
//                      sides of every quad, never a diagonal -- the kernels that read a
//                      face are templates on NV, the vertices per face),
//   edge lengths      (datasets.py:182-188, |pos[row] - pos[col]| over all coordinates),
//   compute_periodic_graph (datasets.py:39-119: left<->right and lower<->upper side nodes
//                      paired in (y, x) order, the 4 corners paired with the opposite
//                      corner, zero edge attribute for the new edges, coalesced with
//                      sum-reduced attributes).
//
// No global sort: the result is a per-row (CSR) object.  Directed edges are counted per
// source row, scattered into the rows' slots in any order (atomics), every row is sorted
// and de-duplicated by itself (rows are short), and a prefix sum places the unique edges.
// The sorted-within-row, rows-in-order result is exactly PyG's coalesce order (by
// row * N + col).  A coalesced attribute is the sum over duplicates of (length for a mesh
// edge, 0 for a periodic one) = the length if the pair is a mesh edge, else 0, so the
// length is computed once per unique edge.  Everything is integer-exact and independent
// of the atomics' order; the lengths are fp32 in torch.linalg.vector_norm's CPU order
// (s = dx*dx, s = fma(dy, dy, s) [, fma(dz, dz, s)], correctly rounded sqrt: bitwise equal).
//
// The side lists are sorted by one workgroup (bitonic, in LDS): each side holds at most
// PDG_SIDE_MAX nodes (a 4096 x 4096 grid).  Invalid periodic geometry (unequal opposite
// sides, a corner that is not exactly one node, a side longer than PDG_SIDE_MAX) is
// reported as *n_edges = -1.  A face with an index outside [0, n_nodes) is never dereferenced:
// its edges are dropped (validity is decided per face) and *n_edges = -2 reports it.
#include <cfloat>

#include "pdg_bbox.hpp"     // bbox_kernel, bbox_load
#include "pdg_common.hpp"
#include "pdg_runtime.hpp"
#include "pdg_scan.hpp"   // scan_local / scan_blocks / scan_add kernels and scan()

#ifndef PDG_SIDE_MAX
#define PDG_SIDE_MAX 4096
#endif

using namespace pdg;

namespace {

constexpr int GT = 256;                  // threads per block of the elementwise kernels
constexpr int SIDE_MAX = PDG_SIDE_MAX;   // nodes per periodic side
constexpr int SORT_THREADS = 1024;

// Scratch layout (int32 words unless noted), see pdg_mesh_graph_scratch_bytes.
struct Scratch {
  float* bbox;     // [GT_BLOCKS_MAX][4] per-block (min x, min y, max x, max y)
  int* ctr;        // [16]: side counts (4), corner counts (4), corners (4), npairs, error, face out of range
  int* side;       // [4][SIDE_MAX]
  int* prow;       // [2 * 2 * SIDE_MAX + 4]
  int* pcol;
  int* deg;        // [N + 1] -> exclusive offsets
  int* fill;       // [N]
  int* ucnt;       // [N + 1] -> row pointer of the result
  int* bsum;       // [scan blocks + 1]
  int* nb;         // [2 NV F + pairs] slot array: 2 * col + (1 if periodic else 0)
};

__device__ __forceinline__ float nmul(float a, float b) { return __fmul_rn(a, b); }

// Side membership (exact float equality, as the reference's ==), compaction into the 4
// side lists (left, right, lower, upper: the concatenation order of datasets.py:85-100)
// and the 4 corners (left-lower, left-upper, right-lower, right-upper).
__global__ __launch_bounds__(GT) void sides_kernel(int n, const float* __restrict__ p, int dim,
                                                   const float* __restrict__ part, int nparts, int* __restrict__ ctr,
                                                   int* __restrict__ side) {
  __shared__ float bb[4];
  bbox_load(part, nparts, bb);
  const float mnx = bb[0], mny = bb[1], mxx = bb[2], mxy = bb[3];
  for (int i = blockIdx.x * GT + threadIdx.x; i < n; i += gridDim.x * GT) {
    const float x = p[(size_t)i * dim], y = p[(size_t)i * dim + 1];
    const bool on[4] = {x == mnx, x == mxx, y == mny, y == mxy};
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (on[s]) {
        const int k = atomicAdd(&ctr[s], 1);
        if (k < SIDE_MAX) side[s * SIDE_MAX + k] = i;
      }
    const int c = on[0] && on[2] ? 0 : on[0] && on[3] ? 1 : on[1] && on[2] ? 2 : on[1] && on[3] ? 3 : -1;
    if (c >= 0) {
      atomicAdd(&ctr[4 + c], 1);
      ctr[8 + c] = i;   // meaningful only when the count is exactly 1
    }
  }
}

// One workgroup: sort each side by (y, x, node id) -- np.lexsort((x, y)) is stable, so equal
// (y, x) keep node order -- validate, and emit the periodic pairs in the reference's order.
__global__ __launch_bounds__(SORT_THREADS) void pairs_kernel(const float* __restrict__ p, int dim, int* __restrict__ ctr,
                                                             int* __restrict__ side, int* __restrict__ prow,
                                                             int* __restrict__ pcol) {
  __shared__ float ky[SIDE_MAX], kx[SIDE_MAX];
  __shared__ int ki[SIDE_MAX];
  __shared__ int bad;
  if (threadIdx.x == 0) {
    bad = 0;
    for (int s = 0; s < 4; ++s) bad |= ctr[s] > SIDE_MAX || ctr[s] == 0;
    for (int c = 0; c < 4; ++c) bad |= ctr[4 + c] != 1;
    bad |= ctr[0] != ctr[1] || ctr[2] != ctr[3];
  }
  __syncthreads();
  if (bad) {
    if (threadIdx.x == 0) ctr[13] = 1;
    return;
  }
  for (int s = 0; s < 4; ++s) {
    const int c = ctr[s];
    int np2 = 1;
    while (np2 < c) np2 <<= 1;
    for (int i = threadIdx.x; i < np2; i += blockDim.x) {
      if (i < c) {
        const int v = side[s * SIDE_MAX + i];
        ky[i] = p[(size_t)v * dim + 1];
        kx[i] = p[(size_t)v * dim];
        ki[i] = v;
      } else {
        ky[i] = FLT_MAX;
        kx[i] = FLT_MAX;
        ki[i] = 0x7fffffff;
      }
    }
    __syncthreads();
    for (int k = 2; k <= np2; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = threadIdx.x; i < np2; i += blockDim.x) {
          const int o = i ^ j;
          if (o > i) {
            const bool asc = (i & k) == 0;
            const bool gt = ky[i] > ky[o] || (ky[i] == ky[o] && (kx[i] > kx[o] || (kx[i] == kx[o] && ki[i] > ki[o])));
            if (gt == asc) {
              float t = ky[i]; ky[i] = ky[o]; ky[o] = t;
              t = kx[i]; kx[i] = kx[o]; kx[o] = t;
              const int u = ki[i]; ki[i] = ki[o]; ki[o] = u;
            }
          }
        }
        __syncthreads();
      }
    for (int i = threadIdx.x; i < c; i += blockDim.x) side[s * SIDE_MAX + i] = ki[i];
    __syncthreads();
  }
  // rows = [left, right, lower, upper, corners], cols = [right, left, upper, lower, corners reversed]
  const int nl = ctr[0], nd = ctr[2];
  const int* L0 = side;
  const int* R0 = side + SIDE_MAX;
  const int* D0 = side + 2 * SIDE_MAX;
  const int* U0 = side + 3 * SIDE_MAX;
  for (int i = threadIdx.x; i < nl; i += blockDim.x) {
    prow[i] = L0[i];
    pcol[i] = R0[i];
    prow[nl + i] = R0[i];
    pcol[nl + i] = L0[i];
  }
  for (int i = threadIdx.x; i < nd; i += blockDim.x) {
    prow[2 * nl + i] = D0[i];
    pcol[2 * nl + i] = U0[i];
    prow[2 * nl + nd + i] = U0[i];
    pcol[2 * nl + nd + i] = D0[i];
  }
  if (threadIdx.x < 4) {
    prow[2 * nl + 2 * nd + threadIdx.x] = ctr[8 + threadIdx.x];
    pcol[2 * nl + 2 * nd + threadIdx.x] = ctr[8 + 3 - threadIdx.x];
  }
  if (threadIdx.x == 0) ctr[12] = 2 * nl + 2 * nd + 4;
}

// Directed edge j of face f, j = 2 * side + direction: the sides (0,1) (1,2) .. (NV-2,NV-1) (0,NV-1), each in
// both directions -- (a,b) (b,a) (b,c) (c,b) (a,c) (c,a) of a triangle (FaceToEdge's three edges, made undirected),
// (f0,f1) (f1,f2) (f2,f3) (f0,f3) and their reverses of a quad (_quad_face_to_edge).  False for a face with an index
// outside [0, n): nothing of it is used.  Pairs k: (prow[k], pcol[k]).
template <int NV>
__device__ __forceinline__ bool face_edge(const int64_t* __restrict__ faces, int n, int f, int j, int& u, int& v) {
  const int64_t* t = faces + NV * (size_t)f;
  bool ok = true;
#pragma unroll
  for (int i = 0; i < NV; ++i) ok = ok && t[i] >= 0 && t[i] < n;
  if (!ok) return false;
  const int s = j >> 1;
  const int a = (int)t[s == NV - 1 ? 0 : s], b = (int)t[s == NV - 1 ? NV - 1 : s + 1];
  u = (j & 1) ? b : a;
  v = (j & 1) ? a : b;
  return true;
}

template <int NV>
__global__ __launch_bounds__(GT) void count_kernel(int n, int nf, const int64_t* __restrict__ faces, int* ctr,
                                                   const int* __restrict__ prow, int* __restrict__ deg,
                                                   int* __restrict__ fill, int periodic) {
  const int np = periodic && !ctr[13] ? ctr[12] : 0;
  const long ne = 2L * NV * nf;
  const long total = ne + np;
  for (long k = (long)blockIdx.x * GT + threadIdx.x; k < total; k += (long)gridDim.x * GT) {
    int u, v;
    if (k < ne) {
      if (!face_edge<NV>(faces, n, (int)(k / (2 * NV)), (int)(k % (2 * NV)), u, v)) {
        ctr[14] = 1;   // every writer stores the same value; read by finish_kernel, launches later
        continue;
      }
    } else {
      u = prow[k - ne];
    }
    atomicAdd(&deg[u], 1);
  }
  for (int i = blockIdx.x * GT + threadIdx.x; i < n; i += gridDim.x * GT) fill[i] = 0;
}

template <int NV>
__global__ __launch_bounds__(GT) void fill_kernel(int n, int nf, const int64_t* __restrict__ faces,
                                                  const int* __restrict__ ctr, const int* __restrict__ prow,
                                                  const int* __restrict__ pcol, const int* __restrict__ off,
                                                  int* __restrict__ fill, int* __restrict__ nb, int periodic) {
  const int np = periodic && !ctr[13] ? ctr[12] : 0;
  const long ne = 2L * NV * nf;
  const long total = ne + np;
  for (long k = (long)blockIdx.x * GT + threadIdx.x; k < total; k += (long)gridDim.x * GT) {
    int u, v, flag = 0;
    if (k < ne) {
      if (!face_edge<NV>(faces, n, (int)(k / (2 * NV)), (int)(k % (2 * NV)), u, v)) continue;
    } else {
      u = prow[k - ne];
      v = pcol[k - ne];
      flag = 1;
    }
    nb[off[u] + atomicAdd(&fill[u], 1)] = 2 * v + flag;
  }
}

// Sort each row's slots (insertion sort: rows are short), count the distinct columns.
__global__ __launch_bounds__(GT) void row_sort_kernel(int n, const int* __restrict__ off, int* __restrict__ nb,
                                                      int* __restrict__ ucnt) {
  for (int r = blockIdx.x * GT + threadIdx.x; r < n; r += gridDim.x * GT) {
    int* a = nb + off[r];
    const int m = off[r + 1] - off[r];
    for (int i = 1; i < m; ++i) {
      const int x = a[i];
      int j = i - 1;
      while (j >= 0 && a[j] > x) {
        a[j + 1] = a[j];
        --j;
      }
      a[j + 1] = x;
    }
    int u = 0;
    for (int i = 0; i < m; ++i) u += i == 0 || (a[i] >> 1) != (a[i - 1] >> 1);
    ucnt[r] = u;
  }
}

// Emit row r's distinct columns at rowptr[r]: attribute = length if any slot of the column
// came from a face (flag 0; it sorts first), else 0.
__global__ __launch_bounds__(GT) void emit_kernel(int n, const float* __restrict__ p, int dim,
                                                  const int* __restrict__ off, const int* __restrict__ nb,
                                                  const int* __restrict__ rowptr, int64_t* __restrict__ rows,
                                                  int64_t* __restrict__ cols, float* __restrict__ attr) {
  for (int r = blockIdx.x * GT + threadIdx.x; r < n; r += gridDim.x * GT) {
    const int* a = nb + off[r];
    const int m = off[r + 1] - off[r];
    int k = rowptr[r];
    for (int i = 0; i < m; ++i) {
      const int v = a[i] >> 1;
      if (i > 0 && v == (a[i - 1] >> 1)) continue;
      float len = 0.f;
      if ((a[i] & 1) == 0) {   // a mesh edge: |pos[r] - pos[v]| (datasets.py:182-188)
        // torch.linalg.vector_norm's CPU order: s = t0 * t0, then s = fma(tk, tk, s), then sqrt
        float s = 0.f;
        for (int d = 0; d < dim; ++d) {
          const float t = p[(size_t)r * dim + d] - p[(size_t)v * dim + d];
          s = d == 0 ? nmul(t, t) : fmaf(t, t, s);
        }
        len = __fsqrt_rn(s);
      }
      rows[k] = r;
      cols[k] = v;
      attr[k] = len;
      ++k;
    }
  }
}

__global__ void finish_kernel(int n, const int* __restrict__ ctr, const int* __restrict__ rowptr, int periodic,
                              int* __restrict__ n_edges) {
  *n_edges = ctr[14] ? -2 : periodic && ctr[13] ? -1 : rowptr[n];
}

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

size_t layout(int n, int nf, int nv, Scratch* s, char* base) {
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + o : nullptr;
    o += align_up(bytes);
    return p;
  };
  const int nscan = (n + SCAN_BLOCK - 1) / SCAN_BLOCK + 1;
  const size_t pmax = 4 * (size_t)SIDE_MAX + 4;
  float* bbox = (float*)take(4 * sizeof(float) * BBOX_BLOCKS);
  int* ctr = (int*)take(16 * sizeof(int));
  int* side = (int*)take(4 * sizeof(int) * SIDE_MAX);
  int* prow = (int*)take(sizeof(int) * pmax);
  int* pcol = (int*)take(sizeof(int) * pmax);
  int* deg = (int*)take(sizeof(int) * ((size_t)n + 1));
  int* fill = (int*)take(sizeof(int) * (size_t)n);
  int* ucnt = (int*)take(sizeof(int) * ((size_t)n + 1));
  int* bsum = (int*)take(sizeof(int) * (size_t)(nscan + 1));
  int* nbp = (int*)take(sizeof(int) * (2 * (size_t)nv * (size_t)nf + pmax));
  if (s) *s = Scratch{bbox, ctr, side, prow, pcol, deg, fill, ucnt, bsum, nbp};
  return o;
}

int grid_for(long work) {
  long g = (work + GT - 1) / GT;
  const long cap = (long)device_cus() * 8;
  return (int)(g < 1 ? 1 : g > cap ? cap : g);
}

template <int NV>
void graph_launch(int n_nodes, const float* points, int dim, int n_faces, const int64_t* faces, int periodic,
                  int64_t* edge_rows, int64_t* edge_cols, float* edge_attr, int* n_edges, void* scratch,
                  hipStream_t st) {
  Scratch s;
  layout(n_nodes, n_faces, NV, &s, (char*)scratch);
  const int nbb = bbox_blocks(n_nodes);
  hipLaunchKernelGGL(bbox_kernel, dim3(nbb), dim3(BBOX_T), 0, st, n_nodes, points, dim, s.bbox, s.ctr);
  if (periodic) {
    hipLaunchKernelGGL(sides_kernel, dim3(grid_for(n_nodes)), dim3(GT), 0, st, n_nodes, points, dim, s.bbox, nbb,
                       s.ctr, s.side);
    hipLaunchKernelGGL(pairs_kernel, dim3(1), dim3(SORT_THREADS), 0, st, points, dim, s.ctr, s.side, s.prow, s.pcol);
  }
  (void)hipMemsetAsync(s.deg, 0, sizeof(int) * ((size_t)n_nodes + 1), st);
  const long work = 2L * NV * n_faces + (periodic ? 4L * SIDE_MAX + 4 : 0);
  hipLaunchKernelGGL(count_kernel<NV>, dim3(grid_for(std::max<long>(work, n_nodes))), dim3(GT), 0, st, n_nodes,
                     n_faces, faces, s.ctr, s.prow, s.deg, s.fill, periodic);
  scan(n_nodes, s.deg, s.bsum, st);
  hipLaunchKernelGGL(fill_kernel<NV>, dim3(grid_for(work)), dim3(GT), 0, st, n_nodes, n_faces, faces, s.ctr, s.prow,
                     s.pcol, s.deg, s.fill, s.nb, periodic);
  hipLaunchKernelGGL(row_sort_kernel, dim3(grid_for(n_nodes)), dim3(GT), 0, st, n_nodes, s.deg, s.nb, s.ucnt);
  scan(n_nodes, s.ucnt, s.bsum, st);
  hipLaunchKernelGGL(emit_kernel, dim3(grid_for(n_nodes)), dim3(GT), 0, st, n_nodes, points, dim, s.deg, s.nb, s.ucnt,
                     edge_rows, edge_cols, edge_attr);
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(1), 0, st, n_nodes, s.ctr, s.ucnt, periodic, n_edges);
}

long graph_bytes(int n_nodes, int n_faces, int nv) {
  if (n_nodes <= 0 || n_faces < 0 || (nv != 3 && nv != 4)) return -1;
  return (long)layout(n_nodes, n_faces, nv, nullptr, nullptr);
}

// Every check runs on the host before any HIP call, under the entry point's own name.
int graph_run(const char* name, int nv, int n_nodes, const float* points, int dim, int n_faces, const int64_t* faces,
              int periodic, int64_t* edge_rows, int64_t* edge_cols, float* edge_attr, long capacity, int* n_edges,
              void* scratch, long scratch_bytes, void* stream) {
  PDG_CHECK_ARG(nv == 3 || nv == 4, "%s: nv must be 3 (triangles) or 4 (quads), got %d", name, nv);
  PDG_CHECK_ARG(n_nodes > 0 && n_faces >= 0 && (dim == 2 || dim == 3), "%s: bad sizes", name);
  PDG_CHECK_ARG(points && edge_rows && edge_cols && edge_attr && n_edges && scratch && (faces || n_faces == 0),
                "%s: null argument", name);
  PDG_CHECK_ARG((long)n_nodes * 2 + 1 < 0x7fffffffL && 2L * nv * n_faces + 4L * SIDE_MAX + 4 < 0x7fffffffL,
                "%s: sizes beyond int32 indexing", name);
  PDG_CHECK_ARG(scratch_bytes >= graph_bytes(n_nodes, n_faces, nv), "%s: scratch too small", name);
  PDG_CHECK_ARG(capacity >= 2L * nv * n_faces + (periodic ? 4L * SIDE_MAX + 4 : 0),
                "%s: capacity below %d * faces (+ periodic pairs)", name, 2 * nv);
  hipStream_t st = (hipStream_t)stream;
  if (nv == 3)
    graph_launch<3>(n_nodes, points, dim, n_faces, faces, periodic, edge_rows, edge_cols, edge_attr, n_edges, scratch,
                    st);
  else
    graph_launch<4>(n_nodes, points, dim, n_faces, faces, periodic, edge_rows, edge_cols, edge_attr, n_edges, scratch,
                    st);
  PDG_CHECK_LAUNCH(name);
  return PDG_OK;
}

}  // namespace

extern "C" long pdg_mesh_graph_scratch_bytes(int n_nodes, int n_faces) { return graph_bytes(n_nodes, n_faces, 3); }

extern "C" int pdg_mesh_graph(int n_nodes, const float* points, int dim, int n_faces, const int64_t* faces,
                              int periodic, int64_t* edge_rows, int64_t* edge_cols, float* edge_attr, long capacity,
                              int* n_edges, void* scratch, long scratch_bytes, void* stream) {
  return graph_run("pdg_mesh_graph", 3, n_nodes, points, dim, n_faces, faces, periodic, edge_rows, edge_cols,
                   edge_attr, capacity, n_edges, scratch, scratch_bytes, stream);
}

// The same call for faces of nv vertices: (n_faces, nv) int64, nv == 3 (bitwise the call above) or 4.
extern "C" long pdg_mesh_graph_cells_scratch_bytes(int n_nodes, int n_faces, int nv) {
  return graph_bytes(n_nodes, n_faces, nv);
}

extern "C" int pdg_mesh_graph_cells(int n_nodes, const float* points, int dim, int n_faces, int nv,
                                    const int64_t* faces, int periodic, int64_t* edge_rows, int64_t* edge_cols,
                                    float* edge_attr, long capacity, int* n_edges, void* scratch, long scratch_bytes,
                                    void* stream) {
  return graph_run("pdg_mesh_graph_cells", nv, n_nodes, points, dim, n_faces, faces, periodic, edge_rows, edge_cols,
                   edge_attr, capacity, n_edges, scratch, scratch_bytes, stream);
}
