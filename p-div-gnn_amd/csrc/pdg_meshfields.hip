// Per-node fields of a bare triangle or quad mesh on the device: what the reference's published
// workload derives on the host before the model runs, and what the divergence check needs.
// Every kernel that reads a face is a template on NV, the vertices per face (3 or 4): the triangle
// instances are the code the triangle entry points always ran, the quad instances serve the *_cells
// entry points (pdg/meshgen.py's quad restatements: the four sides, never a diagonal; the mean Q1
// gradients; the exact Q1 nodal integrals).  Below, the counts are written for triangles: read NV for
// 3 and NV^2 for 9.
//
//   pdg_node_labels      compute_node_labels (datasets.py:122-179): +1 on the external boundary,
//                        -1 on an internal boundary (a hole's rim), 0 elsewhere
//   pdg_p1_div_operator  the area-averaged P1 nodal divergence operator A = [Dx | Dy] (N x 2N) of
//                        pdg/meshgen.py p1_divergence_operator, as COO sorted by (row, col)
//   pdg_nodal_areas      the lumped nodal areas sum area_f / 3 of pdg/meshgen.py nodal_areas (the reference's
//                        quadrature weights gathered to the nodes, generate_dataset.py:73-82) and the bounding box
//   pdg_boundary_vectors the lumped outward boundary vectors bvec[n] = 1/2 sum length * n_outward and lengths
//                        blen[n] = 1/2 sum length over the boundary edges at n, of pdg/meshgen.py boundary_vectors:
//                        sigma(n) . bvec[n] is the nodal boundary force (the lumped traction integral)
//
// All are the grouping of pdg_group.hpp (histogram, exclusive scan, atomic fill of 64-bit slots,
// bounded per-row sort) followed by one thread per row walking its sorted slots.
//
// Labels.  The 3 F undirected edges are grouped by their smaller endpoint and ordered by the larger
// one, so the copies of an edge are neighbours in a row: an edge seen once is a boundary edge
// (pyvista's extract_feature_edges(boundary_edges=True)).  The boundary edges are compacted in row
// order, and one workgroup labels the connected components of the boundary by min-label
// propagation over that list with pointer jumping, until a pass changes nothing.  A pass moves
// the smallest id of a component at least one edge further, so passes <= boundary edges + 1: the
// loop's cap; it never ends a search that has not converged (status bit 2 says if it did).  The
// converged labels are the smallest node id of each component, whatever the atomics' order.
// A component with a node on the bounding box (exact fp32 equality with the min / max of the
// same array, pdg_bbox.hpp) is external.
//
// Operator.  The 9 F (row node, column node) pairs of the faces are grouped by row and ordered by
// (column node, face), so the faces that contribute to one entry are neighbours, in face order.
// Each row's thread sums the entry in fp64 in that order and rounds once to fp32.  The fp64
// expressions are meshgen's, evaluated without contraction.
//
// Areas.  The 3 F (node, face) items are grouped by node and ordered by face; each node's thread sums
// area_f / 3 in fp64 in that order and rounds once to fp32.  A face of zero area adds 0 and is no error here.
//
// Boundary vectors.  The labels' boundary-edge pass (the same device code) marks the boundary edges among the
// sorted slots; their 2 endpoint items are grouped by node and ordered by the other endpoint, and each node's
// thread sums its edges' r = length * n_outward and |r| in fp64 in that order and rounds once to fp32.
//
// A face with an index outside [0, n_nodes) sets a status bit and is ignored: validity is decided
// once per face (fok[]) before anything indexes with its entries.  Every loop is bounded by a row
// length, a list length or the cap above.  Counters and outputs' counters are cleared by a kernel
// (no memset node), there is no grid-wide barrier, and atomics only count or claim slots that are
// sorted afterwards.
#include <stdint.h>

#include <algorithm>

#include "pdg_bbox.hpp"
#include "pdg_cell.hpp"
#include "pdg_group.hpp"
#include "pdg_runtime.hpp"
#include "pdg_scan.hpp"

using namespace pdg;

namespace {

constexpr int CT = 1024;   // threads of the component search's single workgroup

enum { ST_RANGE = 1, ST_NONMANIFOLD = 2, ST_CAP = 4 };   // info[2] of pdg_node_labels
enum { DV_DEGENERATE = 1, DV_RANGE = 2 };                // *status of pdg_p1_div_operator
enum { AR_RANGE = 1 };                                   // *status of pdg_nodal_areas
enum { BV_RANGE = 1, BV_NONMANIFOLD = 2, BV_FLAT = 4 };  // *status of pdg_boundary_vectors

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

struct LabelScratch {
  float* bbox;   // [BBOX_BLOCKS][4]
  int* ctr;      // [16] (cleared by bbox_kernel; unused here)
  int* zero;     // cleared block: cnt [n + 1] | fill [n] | bdeg [n] | ext [n] | bcnt [n + 1]
  int* lab;      // [n] component label (smallest node id) of a boundary node
  int* bsum;     // [scan blocks + 2]
  int* fok;      // [F] face has three indices in range
  int* be_u;     // [3F] boundary edges, smaller endpoint
  int* be_v;     // [3F] ... larger endpoint
  u64* slots;    // [3F]
  u64* sorted;   // [3F]
};

struct DivScratch {
  int* zero;     // cleared block: cnt [n + 1] | fill [n] | ucnt [n + 1]
  int* bsum;
  int* fok;      // [F] face is in range and has det != 0
  u64* slots;    // [9F]
  u64* sorted;   // [9F]
};

struct BvecScratch {
  int* zero;     // cleared block: cnt [n + 1] | fill [n] | cnt2 [n + 1] | fill2 [n]
  int* bsum;
  int* fok;      // [F]
  int* brow;     // [3F] the row (smaller endpoint) of sorted slot k when it is a boundary edge, else -1
  u64* slots;    // [6F] (the edges' grouping uses the first 3F)
  u64* sorted;   // [3F] the edges by smaller endpoint
  u64* sorted2;  // [6F] the boundary edges' endpoints by node
};

size_t label_layout(int n, int nf, int nv, LabelScratch* s, char* base) {
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + o : nullptr;
    o += align_up(bytes);
    return p;
  };
  const size_t e = (size_t)nv * (size_t)std::max(nf, 1);
  LabelScratch t;
  t.bbox = (float*)take(4 * sizeof(float) * BBOX_BLOCKS);
  t.ctr = (int*)take(16 * sizeof(int));
  t.zero = (int*)take(sizeof(int) * (5 * (size_t)n + 2));
  t.lab = (int*)take(sizeof(int) * (size_t)n);
  t.bsum = (int*)take(sizeof(int) * scan_bsum_len(n));
  t.fok = (int*)take(sizeof(int) * (size_t)std::max(nf, 1));
  t.be_u = (int*)take(sizeof(int) * e);
  t.be_v = (int*)take(sizeof(int) * e);
  t.slots = (u64*)take(sizeof(u64) * e);
  t.sorted = (u64*)take(sizeof(u64) * e);
  if (s) *s = t;
  return o;
}

size_t bvec_layout(int n, int nf, int nv, BvecScratch* s, char* base) {
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + o : nullptr;
    o += align_up(bytes);
    return p;
  };
  const size_t e = (size_t)nv * (size_t)std::max(nf, 1);
  BvecScratch t;
  t.zero = (int*)take(sizeof(int) * (4 * (size_t)n + 2));
  t.bsum = (int*)take(sizeof(int) * scan_bsum_len(n));
  t.fok = (int*)take(sizeof(int) * (size_t)std::max(nf, 1));
  t.brow = (int*)take(sizeof(int) * e);
  t.slots = (u64*)take(sizeof(u64) * 2 * e);
  t.sorted = (u64*)take(sizeof(u64) * e);
  t.sorted2 = (u64*)take(sizeof(u64) * 2 * e);
  if (s) *s = t;
  return o;
}

size_t div_layout(int n, int nf, int nv, DivScratch* s, char* base) {
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + o : nullptr;
    o += align_up(bytes);
    return p;
  };
  const size_t e = (size_t)(nv * nv) * (size_t)std::max(nf, 1);
  DivScratch t;
  t.zero = (int*)take(sizeof(int) * (3 * (size_t)n + 2));
  t.bsum = (int*)take(sizeof(int) * scan_bsum_len(n));
  t.fok = (int*)take(sizeof(int) * (size_t)std::max(nf, 1));
  t.slots = (u64*)take(sizeof(u64) * e);
  t.sorted = (u64*)take(sizeof(u64) * e);
  if (s) *s = t;
  return o;
}

bool sizes_ok(int n_nodes, int n_faces, int nv) {
  // the scan indexes base + i < n + SCAN_BLOCK in int32; an item position (< nv^2 F) fills a slot's low word
  return (nv == 3 || nv == 4) && n_nodes > 0 && n_faces >= 0 && (long)n_nodes + SCAN_BLOCK < 0x7fffffffL &&
         (long)(nv * nv) * n_faces + SCAN_BLOCK < 0x7fffffffL;
}

// The vertex after / before vertex v in the face's own cyclic order.
template <int NV>
__device__ __forceinline__ unsigned next_of(unsigned v) {
  return v == NV - 1 ? 0 : v + 1;
}
template <int NV>
__device__ __forceinline__ unsigned prev_of(unsigned v) {
  return v == 0 ? NV - 1 : v - 1;
}

// ----------------------------------------------------------------------------------- labels
template <int NV>
__global__ __launch_bounds__(PT) void label_face_kernel(int nf, const int64_t* __restrict__ faces, int n,
                                                        int* __restrict__ fok, int* __restrict__ cnt,
                                                        int* __restrict__ status) {
  int bad = 0;
  for (long f = (long)blockIdx.x * PT + threadIdx.x; f < nf; f += (long)gridDim.x * PT) {
    const int64_t* t = faces + NV * f;
    const int ok = in_range<NV>(t, n);
    fok[f] = ok;
    if (ok) {
#pragma unroll
      for (int j = 0; j < NV; ++j) atomicAdd(&cnt[min((int)t[j], (int)t[j == NV - 1 ? 0 : j + 1])], 1);
    } else {
      bad = 1;
    }
  }
  if (bad) atomicOr(status, ST_RANGE);   // ST_RANGE == BV_RANGE
}

// Undirected edge j of face f (j = i % NV: the side (j, j + 1), cyclic; (0,1), (1,2), (2,0) of a triangle) under its
// smaller endpoint.
template <int NV>
struct EdgeByMin {
  const int64_t* faces;
  const int* fok;
  u64* sorted;
  __device__ bool item(long i, int& major, unsigned& minor) const {
    const long f = i / NV;
    if (!fok[f]) return false;
    const int j = (int)(i - NV * f);
    const int a = (int)faces[NV * f + j], b = (int)faces[NV * f + (j == NV - 1 ? 0 : j + 1)];
    major = min(a, b);
    minor = (unsigned)max(a, b);
    return true;
  }
  __device__ void emit(long k, int, u64 slot) const { sorted[k] = slot; }
};

// Row r's boundary edges: the larger endpoints that occur exactly once among its sorted slots.  fn(k, v, c): sorted
// slot k is the row's c-th boundary edge (r, v).  Returns their number.  The one definition of a boundary edge on the
// device, shared by the labels and the boundary vectors.
template <class F>
__device__ __forceinline__ int for_boundary_edges(int r, const int* __restrict__ rowptr,
                                                  const u64* __restrict__ sorted, F fn) {
  const int b = rowptr[r], e = rowptr[r + 1];
  int c = 0;
  for (int k = b; k < e;) {
    const int v = (int)(sorted[k] >> 32);
    int len = 1;
    while (k + len < e && (int)(sorted[k + len] >> 32) == v) ++len;
    if (len == 1) {
      fn(k, v, c);
      ++c;
    }
    k += len;
  }
  return c;
}

// write == 0: count them into bcnt[r], add them to both endpoints' boundary degree, start r's
// label at r.  write != 0: store them at bptr[r] (the scanned counts).
__global__ __launch_bounds__(PT) void boundary_kernel(int n, const int* __restrict__ rowptr,
                                                      const u64* __restrict__ sorted, int write,
                                                      int* __restrict__ bdeg, int* __restrict__ bcnt,
                                                      int* __restrict__ lab, const int* __restrict__ bptr,
                                                      int* __restrict__ be_u, int* __restrict__ be_v) {
  for (int r = blockIdx.x * PT + threadIdx.x; r < n; r += gridDim.x * PT) {
    const int c = for_boundary_edges(r, rowptr, sorted, [&](int, int v, int j) {
      if (write) {
        be_u[bptr[r] + j] = r;
        be_v[bptr[r] + j] = v;
      } else {
        atomicAdd(&bdeg[r], 1);
        atomicAdd(&bdeg[v], 1);
      }
    });
    if (!write) {
      bcnt[r] = c;
      lab[r] = r;
    }
  }
}

__device__ __forceinline__ int lab_load(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One workgroup.  lab[x] is always the id of a node of x's component, <= x.  A pass hands the
// smaller label across every boundary edge, then replaces every endpoint's label by its label's
// label.  When a pass sees equal labels across every edge nothing was written during it, every
// component carries one label, and that label is its own label: the component's smallest id.
__global__ __launch_bounds__(CT) void components_kernel(int n, const int* __restrict__ bptr,
                                                        const int* __restrict__ be_u, const int* __restrict__ be_v,
                                                        int* lab, int* __restrict__ info) {
  const int nbe = bptr[n];
  const long cap = (long)nbe + 2;
  long pass = 0;
  int again;
  do {
    int changed = 0;
    for (int e = threadIdx.x; e < nbe; e += CT) {
      const int u = be_u[e], v = be_v[e];
      const int lu = lab_load(lab + u), lv = lab_load(lab + v);
      if (lu < lv) {
        atomicMin(lab + v, lu);
        changed = 1;
      } else if (lv < lu) {
        atomicMin(lab + u, lv);
        changed = 1;
      }
    }
    __threadfence();
    __syncthreads();
    for (int e = threadIdx.x; e < nbe; e += CT) {
      const int u = be_u[e], v = be_v[e];
      const int lu = lab_load(lab + u), lv = lab_load(lab + v);
      const int pu = lab_load(lab + lu), pv = lab_load(lab + lv);
      if (pu < lu) atomicMin(lab + u, pu);
      if (pv < lv) atomicMin(lab + v, pv);
    }
    __threadfence();
    again = __syncthreads_or(changed);
  } while (again && ++pass < cap);
  if (again && threadIdx.x == 0) atomicOr(&info[2], ST_CAP);
}

// A component is external when one of its nodes lies on the bounding box.
__global__ __launch_bounds__(PT) void external_kernel(int n, const float* __restrict__ p, int dim,
                                                      const float* __restrict__ part, int nparts,
                                                      const int* __restrict__ bdeg, const int* __restrict__ lab,
                                                      int* __restrict__ ext, int* __restrict__ info) {
  __shared__ float bb[4];
  bbox_load(part, nparts, bb);
  const float mnx = bb[0], mny = bb[1], mxx = bb[2], mxy = bb[3];
  int bad = 0;
  for (int i = blockIdx.x * PT + threadIdx.x; i < n; i += gridDim.x * PT) {
    const int d = bdeg[i];
    if (d == 0) continue;
    bad |= d != 2;
    const float x = p[(size_t)i * dim], y = p[(size_t)i * dim + 1];
    if (x == mnx || x == mxx || y == mny || y == mxy) ext[lab[i]] = 1;
  }
  if (bad) atomicOr(&info[2], ST_NONMANIFOLD);
}

__global__ __launch_bounds__(PT) void labels_kernel(int n, const int* __restrict__ bdeg, const int* __restrict__ lab,
                                                    const int* __restrict__ ext, int64_t* __restrict__ labels,
                                                    int* __restrict__ info) {
  for (int i = blockIdx.x * PT + threadIdx.x; i < n; i += gridDim.x * PT) {
    int64_t out = 0;
    if (bdeg[i] > 0) {
      const int root = lab[i];
      out = ext[root] ? 1 : -1;
      if (root == i) {            // one node per component: its smallest id
        atomicAdd(&info[0], 1);
        if (ext[i]) atomicAdd(&info[1], 1);
      }
    }
    labels[i] = out;
  }
}

// --------------------------------------------------------------------------------- operator
// A vertex's coordinate by a run-time index: selects over registers (the loops are unrolled), no indexed array.
template <int NV>
__device__ __forceinline__ double pick(const double (&a)[NV], unsigned k) {
  double r = a[0];
#pragma unroll
  for (int v = 1; v < NV; ++v) r = k == (unsigned)v ? a[v] : r;
  return r;
}

template <int NV>
__global__ __launch_bounds__(PT) void div_face_kernel(int nf, const int64_t* __restrict__ faces, int n,
                                                      const float* __restrict__ p, int dim, int* __restrict__ fok,
                                                      int* __restrict__ cnt, int* __restrict__ status) {
  int bad = 0;
  for (long f = (long)blockIdx.x * PT + threadIdx.x; f < nf; f += (long)gridDim.x * PT) {
    const int64_t* t = faces + NV * f;
    int ok = in_range<NV>(t, n);
    if (!ok) {
      bad |= DV_RANGE;
    } else if (cell_of<NV>(p, dim, t).det == 0.0) {
      bad |= DV_DEGENERATE;
      ok = 0;
    }
    fok[f] = ok;
    if (ok)
      for (int v = 0; v < NV; ++v) atomicAdd(&cnt[(int)t[v]], NV);
  }
  if (bad) atomicOr(status, bad);
}

// Item i = NV^2 f + NV vi + vn: face f's contribution to row faces[f][vi] at column node faces[f][vn].
template <int NV>
struct PairByRow {
  const int64_t* faces;
  const int* fok;
  u64* sorted;
  __device__ bool item(long i, int& major, unsigned& minor) const {
    const long f = i / (NV * NV);
    if (!fok[f]) return false;
    const int r = (int)(i - NV * NV * f);
    major = (int)faces[NV * f + r / NV];
    minor = (unsigned)faces[NV * f + r % NV];
    return true;
  }
  __device__ void emit(long k, int, u64 slot) const { sorted[k] = slot; }
};

__global__ __launch_bounds__(PT) void div_count_kernel(int n, const int* __restrict__ rowptr,
                                                       const u64* __restrict__ sorted, int* __restrict__ ucnt) {
  for (int r = blockIdx.x * PT + threadIdx.x; r < n; r += gridDim.x * PT) {
    const int b = rowptr[r], e = rowptr[r + 1];
    int u = 0;
    for (int k = b; k < e; ++k) u += k == b || (sorted[k] >> 32) != (sorted[k - 1] >> 32);
    ucnt[r] = u;
  }
}

// Row r: its distinct column nodes c_0 < c_1 < ... give the entries (r, c_j) then (r, c_j + N).
template <int NV>
__global__ __launch_bounds__(PT) void div_emit_kernel(int n, const float* __restrict__ p, int dim,
                                                      const int64_t* __restrict__ faces,
                                                      const int* __restrict__ rowptr, const u64* __restrict__ sorted,
                                                      const int* __restrict__ uptr, int64_t* __restrict__ rows,
                                                      int64_t* __restrict__ cols, float* __restrict__ vals,
                                                      int* __restrict__ nnz) {
#pragma clang fp contract(off)
  for (int r = blockIdx.x * PT + threadIdx.x; r < n; r += gridDim.x * PT) {
    if (r == 0) *nnz = 2 * uptr[n];
    const int b = rowptr[r], e = rowptr[r + 1];
    const int nu = uptr[r + 1] - uptr[r];
    // the node's summed incident area, faces in index order: the pairs with vi == vn (column r)
    double wsum = 0.0;
    for (int k = b; k < e; ++k) {
      const unsigned id = (unsigned)(sorted[k] & 0xffffffffu);
      const unsigned f = id / (NV * NV), q = id - NV * NV * f;
      if (q / NV == q % NV) wsum += 0.5 * fabs(cell_of<NV>(p, dim, faces + NV * (size_t)f).det);
    }
    const long o = 2L * uptr[r];
    int j = 0;
    for (int k = b; k < e; ++j) {
      const unsigned c = (unsigned)(sorted[k] >> 32);
      double ax = 0.0, ay = 0.0;
      for (; k < e && (unsigned)(sorted[k] >> 32) == c; ++k) {
        const unsigned id = (unsigned)(sorted[k] & 0xffffffffu);
        const unsigned f = id / (NV * NV), vn = (id - NV * NV * f) % NV;
        const Cell<NV> t = cell_of<NV>(p, dim, faces + NV * (size_t)f);
        const double area = 0.5 * fabs(t.det);
        // area * g[vn] = the integral of grad N_vn over the face: (y[vn + 1] - y[vn - 1], x[vn - 1] - x[vn + 1]) / 2,
        // the P1 gradient of a triangle and the mean Q1 gradient of a quad
        const unsigned nx = next_of<NV>(vn), pv = prev_of<NV>(vn);
        const double dy = pick<NV>(t.y, nx) - pick<NV>(t.y, pv);
        const double dx = pick<NV>(t.x, pv) - pick<NV>(t.x, nx);
        ax += area * (dy / t.det) / wsum;
        ay += area * (dx / t.det) / wsum;
      }
      rows[o + j] = r;
      cols[o + j] = c;
      vals[o + j] = (float)ax;
      rows[o + nu + j] = r;
      cols[o + nu + j] = (int64_t)c + n;
      vals[o + nu + j] = (float)ay;
    }
  }
}

// ------------------------------------------------------------------------------ nodal areas
template <int NV>
__global__ __launch_bounds__(PT) void area_face_kernel(int nf, const int64_t* __restrict__ faces, int n,
                                                       int* __restrict__ fok, int* __restrict__ cnt,
                                                       int* __restrict__ status) {
  int bad = 0;
  for (long f = (long)blockIdx.x * PT + threadIdx.x; f < nf; f += (long)gridDim.x * PT) {
    const int64_t* t = faces + NV * f;
    const int ok = in_range<NV>(t, n);
    fok[f] = ok;
    if (ok)
      for (int v = 0; v < NV; ++v) atomicAdd(&cnt[(int)t[v]], 1);
    else
      bad = 1;
  }
  if (bad) atomicOr(status, AR_RANGE);
}

// Item i = NV f + v: face f under its vertex faces[f][v], ordered by face (then by v: a face that names a node
// twice gives it two terms, as the host's add.at over faces.ravel() does).
template <int NV>
struct FaceByNode {
  const int64_t* faces;
  const int* fok;
  u64* sorted;
  __device__ bool item(long i, int& major, unsigned& minor) const {
    const long f = i / NV;
    if (!fok[f]) return false;
    major = (int)faces[i];
    minor = (unsigned)f;
    return true;
  }
  __device__ void emit(long k, int, u64 slot) const { sorted[k] = slot; }
};

// Row r: the sum of its faces' shares in fp64, in face order, rounded once; a node of no face gets exactly 0.  A
// triangle's share is area / 3.  A quad's share at its corner k is the integral of the bilinear N_k over it,
// (|det| + sgn(det) t_k) / 12 with t_k = (p[k+1] - p[k]) x (p[k-1] - p[k]), twice the signed corner triangle
// (area / 4 on a parallelogram); det == 0 gives 0.
// Block 0 also writes the bounding box as (xmin, xmax, ymin, ymax).
template <int NV>
__global__ __launch_bounds__(PT) void area_emit_kernel(int n, const float* __restrict__ p, int dim,
                                                       const int64_t* __restrict__ faces,
                                                       const int* __restrict__ rowptr, const u64* __restrict__ sorted,
                                                       const float* __restrict__ part, int nparts,
                                                       float* __restrict__ area, float* __restrict__ bbox) {
#pragma clang fp contract(off)
  __shared__ float bb[4];
  if (blockIdx.x == 0) {   // uniform over the block: bbox_load's barrier is reached by all of it or none
    bbox_load(part, nparts, bb);
    if (threadIdx.x == 0) {
      bbox[0] = bb[0];
      bbox[1] = bb[2];
      bbox[2] = bb[1];
      bbox[3] = bb[3];
    }
  }
  for (int r = blockIdx.x * PT + threadIdx.x; r < n; r += gridDim.x * PT) {
    const int b = rowptr[r], e = rowptr[r + 1];
    double a = 0.0;
    for (int k = b; k < e; ++k) {
      const unsigned f = (unsigned)(sorted[k] >> 32);
      const Cell<NV> t = cell_of<NV>(p, dim, faces + NV * (size_t)f);
      if constexpr (NV == 3) {
        a += 0.5 * fabs(t.det) / 3.0;
      } else {
        const unsigned v = (unsigned)(sorted[k] & 0xffffffffu) - NV * f;   // the corner: item position - NV f
        const unsigned nx = next_of<NV>(v), pv = prev_of<NV>(v);
        const double xk = pick<NV>(t.x, v), yk = pick<NV>(t.y, v);
        const double e0 = (pick<NV>(t.x, nx) - xk) * (pick<NV>(t.y, pv) - yk);
        const double e1 = (pick<NV>(t.y, nx) - yk) * (pick<NV>(t.x, pv) - xk);
        const double tk = e0 - e1;
        a += t.det == 0.0 ? 0.0 : (fabs(t.det) + (t.det > 0.0 ? tk : -tk)) / 12.0;
      }
    }
    area[r] = (float)a;
  }
}

// ------------------------------------------------------------------------- boundary vectors
// brow[k] = r where sorted slot k is a boundary edge of row r, -1 elsewhere (every k < rowptr[n] lies in one row);
// cnt2: the boundary edges at each node, both endpoints counted.
__global__ __launch_bounds__(PT) void bvec_mark_kernel(int n, const int* __restrict__ rowptr,
                                                       const u64* __restrict__ sorted, int* __restrict__ brow,
                                                       int* __restrict__ cnt2) {
  for (int r = blockIdx.x * PT + threadIdx.x; r < n; r += gridDim.x * PT) {
    for (int k = rowptr[r]; k < rowptr[r + 1]; ++k) brow[k] = -1;
    for_boundary_edges(r, rowptr, sorted, [&](int k, int v, int) {
      brow[k] = r;
      atomicAdd(&cnt2[r], 1);
      atomicAdd(&cnt2[v], 1);
    });
  }
}

// Item i = 2 k + side: boundary edge k (a sorted slot of the edges' grouping) under its smaller (side 0) or larger
// (side 1) endpoint, ordered by the other endpoint.
struct EndByNode {
  const int* rowptr;   // of the edges' grouping: rowptr[n] slots are in use
  int n;
  const int* brow;
  const u64* sorted;
  u64* sorted2;
  __device__ bool item(long i, int& major, unsigned& minor) const {
    const long k = i >> 1;
    if (k >= rowptr[n] || brow[k] < 0) return false;
    const int u = brow[k], v = (int)(sorted[k] >> 32);
    major = (i & 1) ? v : u;
    minor = (unsigned)((i & 1) ? u : v);
    return true;
  }
  __device__ void emit(long k, int, u64 slot) const { sorted2[k] = slot; }
};

// Node r: its boundary edges in ascending order of the other endpoint.  Edge (a, b) of face (a, b, c[, d]), in the
// face's own order (c: the vertex after b): r = (yb - ya, -(xb - xa)), negated when r . (pc - pa) > 0 so that it
// points away from c; bvec = 1/2 sum r, blen = 1/2 sum |r|, fp64 sums rounded once.  A node of no boundary edge gets
// exact zeros.
template <int NV>
__global__ __launch_bounds__(PT) void bvec_emit_kernel(int n, const float* __restrict__ p, int dim,
                                                       const int64_t* __restrict__ faces,
                                                       const int* __restrict__ rowptr2,
                                                       const u64* __restrict__ sorted2,
                                                       const u64* __restrict__ sorted, float* __restrict__ bvec,
                                                       float* __restrict__ blen, int* __restrict__ status) {
#pragma clang fp contract(off)
  int bad = 0;
  for (int r = blockIdx.x * PT + threadIdx.x; r < n; r += gridDim.x * PT) {
    const int b = rowptr2[r], e = rowptr2[r + 1];
    double sx = 0.0, sy = 0.0, sl = 0.0;
    if (e > b && e - b != 2) bad |= BV_NONMANIFOLD;
    for (int q = b; q < e; ++q) {
      const unsigned k = (unsigned)(sorted2[q] & 0xffffffffu) >> 1;
      const unsigned pos = (unsigned)(sorted[k] & 0xffffffffu);
      const unsigned f = pos / NV, j = pos - NV * f;
      const int64_t* t = faces + NV * (size_t)f;
      const size_t ia = (size_t)t[j], ib = (size_t)t[next_of<NV>(j)], ic = (size_t)t[next_of<NV>(next_of<NV>(j))];
      const double xa = p[ia * dim], ya = p[ia * dim + 1];
      const double xb = p[ib * dim], yb = p[ib * dim + 1];
      const double xc = p[ic * dim], yc = p[ic * dim + 1];
      double rx = yb - ya, ry = -(xb - xa);
      sl += sqrt(rx * rx + ry * ry);
      if (cell_of<NV>(p, dim, t).det == 0.0) {
        bad |= BV_FLAT;
        continue;
      }
      if (rx * (xc - xa) + ry * (yc - ya) > 0.0) {
        rx = -rx;
        ry = -ry;
      }
      sx += rx;
      sy += ry;
    }
    bvec[2 * (size_t)r] = (float)(0.5 * sx);
    bvec[2 * (size_t)r + 1] = (float)(0.5 * sy);
    blen[r] = (float)(0.5 * sl);
  }
  if (bad) atomicOr(status, bad);
}


// ------------------------------------------------------------------------------------ launchers
template <int NV>
void labels_launch(int n_nodes, const float* points, int dim, int n_faces, const int64_t* faces, int64_t* labels,
                   int* info, void* scratch, hipStream_t st) {
  LabelScratch s;
  label_layout(n_nodes, n_faces, NV, &s, (char*)scratch);
  const long n = n_nodes;
  int* cnt = s.zero;             // [n + 1]
  int* fill = cnt + n + 1;       // [n]
  int* bdeg = fill + n;          // [n]
  int* ext = bdeg + n;           // [n]
  int* bcnt = ext + n;           // [n + 1]
  const int nbb = bbox_blocks(n_nodes);
  hipLaunchKernelGGL(bbox_kernel, dim3(nbb), dim3(BBOX_T), 0, st, n_nodes, points, dim, s.bbox, s.ctr);
  hipLaunchKernelGGL(clear_kernel, dim3(grid_for(5 * n + 2)), dim3(PT), 0, st, s.zero, 5 * n + 2, info, 3L,
                     (int*)nullptr, 0L, (int*)nullptr);
  if (n_faces > 0)
    hipLaunchKernelGGL(label_face_kernel<NV>, dim3(grid_for(n_faces)), dim3(PT), 0, st, n_faces, faces, n_nodes, s.fok,
                       cnt, info + 2);
  group(EdgeByMin<NV>{faces, s.fok, s.sorted}, (long)NV * n_faces, n_nodes, cnt, fill, s.bsum, s.slots, st);
  hipLaunchKernelGGL(boundary_kernel, dim3(grid_for(n)), dim3(PT), 0, st, n_nodes, cnt, s.sorted, 0, bdeg, bcnt, s.lab,
                     (const int*)nullptr, (int*)nullptr, (int*)nullptr);
  scan(n_nodes, bcnt, s.bsum, st);
  hipLaunchKernelGGL(boundary_kernel, dim3(grid_for(n)), dim3(PT), 0, st, n_nodes, cnt, s.sorted, 1, (int*)nullptr,
                     (int*)nullptr, (int*)nullptr, bcnt, s.be_u, s.be_v);
  hipLaunchKernelGGL(components_kernel, dim3(1), dim3(CT), 0, st, n_nodes, bcnt, s.be_u, s.be_v, s.lab, info);
  hipLaunchKernelGGL(external_kernel, dim3(grid_for(n)), dim3(PT), 0, st, n_nodes, points, dim, s.bbox, nbb, bdeg,
                     s.lab, ext, info);
  hipLaunchKernelGGL(labels_kernel, dim3(grid_for(n)), dim3(PT), 0, st, n_nodes, bdeg, s.lab, ext, labels, info);
}

template <int NV>
void div_launch(int n_nodes, const float* points, int dim, int n_faces, const int64_t* faces, int64_t* rows,
                int64_t* cols, float* vals, int* nnz, int* status, void* scratch, hipStream_t st) {
  DivScratch s;
  div_layout(n_nodes, n_faces, NV, &s, (char*)scratch);
  const long n = n_nodes;
  int* cnt = s.zero;             // [n + 1]
  int* fill = cnt + n + 1;       // [n]
  int* ucnt = fill + n;          // [n + 1]
  hipLaunchKernelGGL(clear_kernel, dim3(grid_for(3 * n + 2)), dim3(PT), 0, st, s.zero, 3 * n + 2, nnz, 1L,
                     (int*)nullptr, 0L, status);
  if (n_faces > 0)
    hipLaunchKernelGGL(div_face_kernel<NV>, dim3(grid_for(n_faces)), dim3(PT), 0, st, n_faces, faces, n_nodes, points,
                       dim, s.fok, cnt, status);
  group(PairByRow<NV>{faces, s.fok, s.sorted}, (long)(NV * NV) * n_faces, n_nodes, cnt, fill, s.bsum, s.slots, st);
  hipLaunchKernelGGL(div_count_kernel, dim3(grid_for(n)), dim3(PT), 0, st, n_nodes, cnt, s.sorted, ucnt);
  scan(n_nodes, ucnt, s.bsum, st);
  hipLaunchKernelGGL(div_emit_kernel<NV>, dim3(grid_for(n)), dim3(PT), 0, st, n_nodes, points, dim, faces, cnt,
                     s.sorted, ucnt, rows, cols, vals, nnz);
}

template <int NV>
void areas_launch(int n_nodes, const float* points, int dim, int n_faces, const int64_t* faces, float* area,
                  float* bbox, int* status, void* scratch, hipStream_t st) {
  LabelScratch s;   // the labels' layout holds all that is needed here: bbox, cnt | fill, bsum, fok, NV F slots twice
  label_layout(n_nodes, n_faces, NV, &s, (char*)scratch);
  const long n = n_nodes;
  int* cnt = s.zero;             // [n + 1]
  int* fill = cnt + n + 1;       // [n]
  const int nbb = bbox_blocks(n_nodes);
  hipLaunchKernelGGL(bbox_kernel, dim3(nbb), dim3(BBOX_T), 0, st, n_nodes, points, dim, s.bbox, s.ctr);
  hipLaunchKernelGGL(clear_kernel, dim3(grid_for(2 * n + 1)), dim3(PT), 0, st, s.zero, 2 * n + 1, (int*)nullptr, 0L,
                     (int*)nullptr, 0L, status);
  if (n_faces > 0)
    hipLaunchKernelGGL(area_face_kernel<NV>, dim3(grid_for(n_faces)), dim3(PT), 0, st, n_faces, faces, n_nodes, s.fok,
                       cnt, status);
  group(FaceByNode<NV>{faces, s.fok, s.sorted}, (long)NV * n_faces, n_nodes, cnt, fill, s.bsum, s.slots, st);
  hipLaunchKernelGGL(area_emit_kernel<NV>, dim3(grid_for(n)), dim3(PT), 0, st, n_nodes, points, dim, faces, cnt,
                     s.sorted, s.bbox, nbb, area, bbox);
}

template <int NV>
void bvec_launch(int n_nodes, const float* points, int dim, int n_faces, const int64_t* faces, float* bvec,
                 float* blen, int* status, void* scratch, hipStream_t st) {
  BvecScratch s;
  bvec_layout(n_nodes, n_faces, NV, &s, (char*)scratch);
  const long n = n_nodes;
  int* cnt = s.zero;             // [n + 1]
  int* fill = cnt + n + 1;       // [n]
  int* cnt2 = fill + n;          // [n + 1]
  int* fill2 = cnt2 + n + 1;     // [n]
  hipLaunchKernelGGL(clear_kernel, dim3(grid_for(4 * n + 2)), dim3(PT), 0, st, s.zero, 4 * n + 2, (int*)nullptr, 0L,
                     (int*)nullptr, 0L, status);
  if (n_faces > 0)
    hipLaunchKernelGGL(label_face_kernel<NV>, dim3(grid_for(n_faces)), dim3(PT), 0, st, n_faces, faces, n_nodes, s.fok,
                       cnt, status);
  group(EdgeByMin<NV>{faces, s.fok, s.sorted}, (long)NV * n_faces, n_nodes, cnt, fill, s.bsum, s.slots, st);
  hipLaunchKernelGGL(bvec_mark_kernel, dim3(grid_for(n)), dim3(PT), 0, st, n_nodes, cnt, s.sorted, s.brow, cnt2);
  group(EndByNode{cnt, n_nodes, s.brow, s.sorted, s.sorted2}, 2L * NV * n_faces, n_nodes, cnt2, fill2, s.bsum, s.slots,
        st);
  hipLaunchKernelGGL(bvec_emit_kernel<NV>, dim3(grid_for(n)), dim3(PT), 0, st, n_nodes, points, dim, faces, cnt2,
                     s.sorted2, s.sorted, bvec, blen, status);
}

long fields_bytes(int n_nodes, int n_faces, int nv) {
  if (!sizes_ok(n_nodes, n_faces, nv)) return -1;
  return (long)std::max(label_layout(n_nodes, n_faces, nv, nullptr, nullptr),
                        div_layout(n_nodes, n_faces, nv, nullptr, nullptr));
}

long bvec_bytes(int n_nodes, int n_faces, int nv) {
  if (!sizes_ok(n_nodes, n_faces, nv)) return -1;
  return (long)bvec_layout(n_nodes, n_faces, nv, nullptr, nullptr);
}

// The host checks every entry point makes before any HIP call, under the entry point's own name (nv == 3 for the
// triangle entry points).
#define PDG_CHECK_MESH(name, nv, n_nodes, n_faces, dim)                                                               \
  do {                                                                                                                \
    PDG_CHECK_ARG((nv) == 3 || (nv) == 4, "%s: nv must be 3 (triangles) or 4 (quads), got %d", name, (int)(nv));      \
    PDG_CHECK_ARG(sizes_ok(n_nodes, n_faces, nv) && ((dim) == 2 || (dim) == 3),                                       \
                  "%s: bad sizes (n_nodes > 0, n_faces >= 0, dim 2 or 3, n_nodes + 1024 and %d n_faces + 1024 < "     \
                  "2^31)", name, (int)((nv) * (nv)));                                                                 \
  } while (0)

int labels_run(const char* name, int nv, int n_nodes, const float* points, int dim, int n_faces, const int64_t* faces,
               int64_t* labels, int* info, void* scratch, long scratch_bytes, void* stream) {
  PDG_CHECK_MESH(name, nv, n_nodes, n_faces, dim);
  PDG_CHECK_ARG(points && labels && info && scratch && (faces || n_faces == 0), "%s: null argument", name);
  PDG_CHECK_ARG(scratch_bytes >= fields_bytes(n_nodes, n_faces, nv), "%s: scratch too small", name);
  hipStream_t st = (hipStream_t)stream;
  if (nv == 3)
    labels_launch<3>(n_nodes, points, dim, n_faces, faces, labels, info, scratch, st);
  else
    labels_launch<4>(n_nodes, points, dim, n_faces, faces, labels, info, scratch, st);
  PDG_CHECK_LAUNCH(name);
  return PDG_OK;
}

int div_run(const char* name, int nv, int n_nodes, const float* points, int dim, int n_faces, const int64_t* faces,
            int64_t* rows, int64_t* cols, float* vals, long capacity, int* nnz, int* status, void* scratch,
            long scratch_bytes, void* stream) {
  PDG_CHECK_MESH(name, nv, n_nodes, n_faces, dim);
  PDG_CHECK_ARG(points && nnz && status && scratch && (faces || n_faces == 0), "%s: null argument", name);
  PDG_CHECK_ARG(n_faces == 0 || (rows && cols && vals), "%s: null argument", name);
  PDG_CHECK_ARG(scratch_bytes >= fields_bytes(n_nodes, n_faces, nv), "%s: scratch too small", name);
  PDG_CHECK_ARG(capacity >= 2L * nv * nv * n_faces, "%s: capacity below %d * faces", name, 2 * nv * nv);
  hipStream_t st = (hipStream_t)stream;
  if (nv == 3)
    div_launch<3>(n_nodes, points, dim, n_faces, faces, rows, cols, vals, nnz, status, scratch, st);
  else
    div_launch<4>(n_nodes, points, dim, n_faces, faces, rows, cols, vals, nnz, status, scratch, st);
  PDG_CHECK_LAUNCH(name);
  return PDG_OK;
}

int areas_run(const char* name, int nv, int n_nodes, const float* points, int dim, int n_faces, const int64_t* faces,
              float* area, float* bbox, int* status, void* scratch, long scratch_bytes, void* stream) {
  PDG_CHECK_MESH(name, nv, n_nodes, n_faces, dim);
  PDG_CHECK_ARG(points && area && bbox && status && scratch && (faces || n_faces == 0), "%s: null argument", name);
  PDG_CHECK_ARG(scratch_bytes >= fields_bytes(n_nodes, n_faces, nv), "%s: scratch too small", name);
  hipStream_t st = (hipStream_t)stream;
  if (nv == 3)
    areas_launch<3>(n_nodes, points, dim, n_faces, faces, area, bbox, status, scratch, st);
  else
    areas_launch<4>(n_nodes, points, dim, n_faces, faces, area, bbox, status, scratch, st);
  PDG_CHECK_LAUNCH(name);
  return PDG_OK;
}

int bvec_run(const char* name, int nv, int n_nodes, const float* points, int dim, int n_faces, const int64_t* faces,
             float* bvec, float* blen, int* status, void* scratch, long scratch_bytes, void* stream) {
  PDG_CHECK_MESH(name, nv, n_nodes, n_faces, dim);
  PDG_CHECK_ARG(points && bvec && blen && status && scratch && (faces || n_faces == 0), "%s: null argument", name);
  PDG_CHECK_ARG(scratch_bytes >= bvec_bytes(n_nodes, n_faces, nv), "%s: scratch too small", name);
  hipStream_t st = (hipStream_t)stream;
  if (nv == 3)
    bvec_launch<3>(n_nodes, points, dim, n_faces, faces, bvec, blen, status, scratch, st);
  else
    bvec_launch<4>(n_nodes, points, dim, n_faces, faces, bvec, blen, status, scratch, st);
  PDG_CHECK_LAUNCH(name);
  return PDG_OK;
}

}  // namespace

// The triangle entry points: nv == 3 of the same code, with the sizes they always had.
extern "C" long pdg_mesh_fields_scratch_bytes(int n_nodes, int n_faces) { return fields_bytes(n_nodes, n_faces, 3); }

extern "C" int pdg_node_labels(int n_nodes, const float* points, int dim, int n_faces, const int64_t* faces,
                               int64_t* labels, int* info, void* scratch, long scratch_bytes, void* stream) {
  return labels_run("pdg_node_labels", 3, n_nodes, points, dim, n_faces, faces, labels, info, scratch, scratch_bytes,
                    stream);
}

extern "C" int pdg_p1_div_operator(int n_nodes, const float* points, int dim, int n_faces, const int64_t* faces,
                                   int64_t* rows, int64_t* cols, float* vals, long capacity, int* nnz, int* status,
                                   void* scratch, long scratch_bytes, void* stream) {
  return div_run("pdg_p1_div_operator", 3, n_nodes, points, dim, n_faces, faces, rows, cols, vals, capacity, nnz,
                 status, scratch, scratch_bytes, stream);
}

extern "C" int pdg_nodal_areas(int n_nodes, const float* points, int dim, int n_faces, const int64_t* faces,
                               float* area, float* bbox, int* status, void* scratch, long scratch_bytes,
                               void* stream) {
  return areas_run("pdg_nodal_areas", 3, n_nodes, points, dim, n_faces, faces, area, bbox, status, scratch,
                   scratch_bytes, stream);
}

extern "C" long pdg_boundary_vectors_scratch_bytes(int n_nodes, int n_faces) {
  return bvec_bytes(n_nodes, n_faces, 3);
}

extern "C" int pdg_boundary_vectors(int n_nodes, const float* points, int dim, int n_faces, const int64_t* faces,
                                    float* bvec, float* blen, int* status, void* scratch, long scratch_bytes,
                                    void* stream) {
  return bvec_run("pdg_boundary_vectors", 3, n_nodes, points, dim, n_faces, faces, bvec, blen, status, scratch,
                  scratch_bytes, stream);
}

// The same calls for faces of nv vertices: (n_faces, nv) int64, nv == 3 (bitwise the calls above) or 4.
extern "C" long pdg_mesh_fields_cells_scratch_bytes(int n_nodes, int n_faces, int nv) {
  return fields_bytes(n_nodes, n_faces, nv);
}

extern "C" int pdg_node_labels_cells(int n_nodes, const float* points, int dim, int n_faces, int nv,
                                     const int64_t* faces, int64_t* labels, int* info, void* scratch,
                                     long scratch_bytes, void* stream) {
  return labels_run("pdg_node_labels_cells", nv, n_nodes, points, dim, n_faces, faces, labels, info, scratch,
                    scratch_bytes, stream);
}

extern "C" int pdg_div_operator_cells(int n_nodes, const float* points, int dim, int n_faces, int nv,
                                      const int64_t* faces, int64_t* rows, int64_t* cols, float* vals, long capacity,
                                      int* nnz, int* status, void* scratch, long scratch_bytes, void* stream) {
  return div_run("pdg_div_operator_cells", nv, n_nodes, points, dim, n_faces, faces, rows, cols, vals, capacity, nnz,
                 status, scratch, scratch_bytes, stream);
}

extern "C" int pdg_nodal_areas_cells(int n_nodes, const float* points, int dim, int n_faces, int nv,
                                     const int64_t* faces, float* area, float* bbox, int* status, void* scratch,
                                     long scratch_bytes, void* stream) {
  return areas_run("pdg_nodal_areas_cells", nv, n_nodes, points, dim, n_faces, faces, area, bbox, status, scratch,
                   scratch_bytes, stream);
}

extern "C" long pdg_boundary_vectors_cells_scratch_bytes(int n_nodes, int n_faces, int nv) {
  return bvec_bytes(n_nodes, n_faces, nv);
}

extern "C" int pdg_boundary_vectors_cells(int n_nodes, const float* points, int dim, int n_faces, int nv,
                                          const int64_t* faces, float* bvec, float* blen, int* status, void* scratch,
                                          long scratch_bytes, void* stream) {
  return bvec_run("pdg_boundary_vectors_cells", nv, n_nodes, points, dim, n_faces, faces, bvec, blen, status, scratch,
                  scratch_bytes, stream);
}
