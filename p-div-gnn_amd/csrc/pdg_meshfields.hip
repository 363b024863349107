// Per-node fields of a bare triangle mesh on the device: what the reference's published
// workload derives on the host before the model runs, and what the divergence check needs.
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

size_t label_layout(int n, int nf, LabelScratch* s, char* base) {
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + o : nullptr;
    o += align_up(bytes);
    return p;
  };
  const size_t e = 3 * (size_t)std::max(nf, 1);
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

size_t bvec_layout(int n, int nf, BvecScratch* s, char* base) {
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + o : nullptr;
    o += align_up(bytes);
    return p;
  };
  const size_t e = 3 * (size_t)std::max(nf, 1);
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

size_t div_layout(int n, int nf, DivScratch* s, char* base) {
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + o : nullptr;
    o += align_up(bytes);
    return p;
  };
  const size_t e = 9 * (size_t)std::max(nf, 1);
  DivScratch t;
  t.zero = (int*)take(sizeof(int) * (3 * (size_t)n + 2));
  t.bsum = (int*)take(sizeof(int) * scan_bsum_len(n));
  t.fok = (int*)take(sizeof(int) * (size_t)std::max(nf, 1));
  t.slots = (u64*)take(sizeof(u64) * e);
  t.sorted = (u64*)take(sizeof(u64) * e);
  if (s) *s = t;
  return o;
}

bool sizes_ok(int n_nodes, int n_faces) {
  // the scan indexes base + i < n + SCAN_BLOCK in int32; an item position (< 9 F) fills a slot's low word
  return n_nodes > 0 && n_faces >= 0 && (long)n_nodes + SCAN_BLOCK < 0x7fffffffL &&
         9L * n_faces + SCAN_BLOCK < 0x7fffffffL;
}

__device__ __forceinline__ bool in_range(const int64_t* __restrict__ t, int n) {
  return t[0] >= 0 && t[0] < n && t[1] >= 0 && t[1] < n && t[2] >= 0 && t[2] < n;
}

// ----------------------------------------------------------------------------------- labels
__global__ __launch_bounds__(PT) void label_face_kernel(int nf, const int64_t* __restrict__ faces, int n,
                                                        int* __restrict__ fok, int* __restrict__ cnt,
                                                        int* __restrict__ status) {
  int bad = 0;
  for (long f = (long)blockIdx.x * PT + threadIdx.x; f < nf; f += (long)gridDim.x * PT) {
    const int64_t* t = faces + 3 * f;
    const int ok = in_range(t, n);
    fok[f] = ok;
    if (ok) {
      const int a = (int)t[0], b = (int)t[1], c = (int)t[2];
      atomicAdd(&cnt[min(a, b)], 1);
      atomicAdd(&cnt[min(b, c)], 1);
      atomicAdd(&cnt[min(c, a)], 1);
    } else {
      bad = 1;
    }
  }
  if (bad) atomicOr(status, ST_RANGE);   // ST_RANGE == BV_RANGE
}

// Undirected edge j of face f (j = i % 3: (0,1), (1,2), (2,0)) under its smaller endpoint.
struct EdgeByMin {
  const int64_t* faces;
  const int* fok;
  u64* sorted;
  __device__ bool item(long i, int& major, unsigned& minor) const {
    const long f = i / 3;
    if (!fok[f]) return false;
    const int j = (int)(i - 3 * f);
    const int a = (int)faces[3 * f + j], b = (int)faces[3 * f + (j == 2 ? 0 : j + 1)];
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
struct Tri {
  double xa, ya, xb, yb, xc, yc, det;
};

// meshgen.p1_divergence_operator's fp64 expressions, one rounding per operation.
__device__ __forceinline__ Tri triangle(const float* __restrict__ p, int dim, const int64_t* __restrict__ t) {
#pragma clang fp contract(off)
  Tri q;
  q.xa = p[(size_t)t[0] * dim];
  q.ya = p[(size_t)t[0] * dim + 1];
  q.xb = p[(size_t)t[1] * dim];
  q.yb = p[(size_t)t[1] * dim + 1];
  q.xc = p[(size_t)t[2] * dim];
  q.yc = p[(size_t)t[2] * dim + 1];
  const double m0 = (q.xb - q.xa) * (q.yc - q.ya);
  const double m1 = (q.xc - q.xa) * (q.yb - q.ya);
  q.det = m0 - m1;   // 2 * signed area
  return q;
}

__global__ __launch_bounds__(PT) void div_face_kernel(int nf, const int64_t* __restrict__ faces, int n,
                                                      const float* __restrict__ p, int dim, int* __restrict__ fok,
                                                      int* __restrict__ cnt, int* __restrict__ status) {
  int bad = 0;
  for (long f = (long)blockIdx.x * PT + threadIdx.x; f < nf; f += (long)gridDim.x * PT) {
    const int64_t* t = faces + 3 * f;
    int ok = in_range(t, n);
    if (!ok) {
      bad |= DV_RANGE;
    } else if (triangle(p, dim, t).det == 0.0) {
      bad |= DV_DEGENERATE;
      ok = 0;
    }
    fok[f] = ok;
    if (ok)
      for (int v = 0; v < 3; ++v) atomicAdd(&cnt[(int)t[v]], 3);
  }
  if (bad) atomicOr(status, bad);
}

// Item i = 9 f + 3 vi + vn: face f's contribution to row faces[f][vi] at column node faces[f][vn].
struct PairByRow {
  const int64_t* faces;
  const int* fok;
  u64* sorted;
  __device__ bool item(long i, int& major, unsigned& minor) const {
    const long f = i / 9;
    if (!fok[f]) return false;
    const int r = (int)(i - 9 * f);
    major = (int)faces[3 * f + r / 3];
    minor = (unsigned)faces[3 * f + r % 3];
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
      const unsigned f = id / 9, q = id - 9 * f;
      if (q / 3 == q % 3) wsum += 0.5 * fabs(triangle(p, dim, faces + 3 * (size_t)f).det);
    }
    const long o = 2L * uptr[r];
    int j = 0;
    for (int k = b; k < e; ++j) {
      const unsigned c = (unsigned)(sorted[k] >> 32);
      double ax = 0.0, ay = 0.0;
      for (; k < e && (unsigned)(sorted[k] >> 32) == c; ++k) {
        const unsigned id = (unsigned)(sorted[k] & 0xffffffffu);
        const unsigned f = id / 9, vn = (id - 9 * f) % 3;
        const Tri t = triangle(p, dim, faces + 3 * (size_t)f);
        const double area = 0.5 * fabs(t.det);
        const double dy = vn == 0 ? t.yb - t.yc : vn == 1 ? t.yc - t.ya : t.ya - t.yb;
        const double dx = vn == 0 ? t.xc - t.xb : vn == 1 ? t.xa - t.xc : t.xb - t.xa;
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
__global__ __launch_bounds__(PT) void area_face_kernel(int nf, const int64_t* __restrict__ faces, int n,
                                                       int* __restrict__ fok, int* __restrict__ cnt,
                                                       int* __restrict__ status) {
  int bad = 0;
  for (long f = (long)blockIdx.x * PT + threadIdx.x; f < nf; f += (long)gridDim.x * PT) {
    const int64_t* t = faces + 3 * f;
    const int ok = in_range(t, n);
    fok[f] = ok;
    if (ok)
      for (int v = 0; v < 3; ++v) atomicAdd(&cnt[(int)t[v]], 1);
    else
      bad = 1;
  }
  if (bad) atomicOr(status, AR_RANGE);
}

// Item i = 3 f + v: face f under its vertex faces[f][v], ordered by face (then by v: a face that names a node
// twice gives it two terms, as the host's add.at over faces.ravel() does).
struct FaceByNode {
  const int64_t* faces;
  const int* fok;
  u64* sorted;
  __device__ bool item(long i, int& major, unsigned& minor) const {
    const long f = i / 3;
    if (!fok[f]) return false;
    major = (int)faces[i];
    minor = (unsigned)f;
    return true;
  }
  __device__ void emit(long k, int, u64 slot) const { sorted[k] = slot; }
};

// Row r: the sum of its faces' area / 3 in fp64, in face order, rounded once; a node of no face gets exactly 0.
// Block 0 also writes the bounding box as (xmin, xmax, ymin, ymax).
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
      a += 0.5 * fabs(triangle(p, dim, faces + 3 * (size_t)f).det) / 3.0;
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

// Node r: its boundary edges in ascending order of the other endpoint.  Edge (a, b) of face (a, b, c), in the
// face's own order: r = (yb - ya, -(xb - xa)), negated when r . (pc - pa) > 0 so that it points away from c;
// bvec = 1/2 sum r, blen = 1/2 sum |r|, fp64 sums rounded once.  A node of no boundary edge gets exact zeros.
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
      const unsigned f = pos / 3, j = pos - 3 * f;
      const int64_t* t = faces + 3 * (size_t)f;
      const size_t ia = (size_t)t[j], ib = (size_t)t[j == 2 ? 0 : j + 1], ic = (size_t)t[j == 0 ? 2 : j - 1];
      const double xa = p[ia * dim], ya = p[ia * dim + 1];
      const double xb = p[ib * dim], yb = p[ib * dim + 1];
      const double xc = p[ic * dim], yc = p[ic * dim + 1];
      double rx = yb - ya, ry = -(xb - xa);
      sl += sqrt(rx * rx + ry * ry);
      if (triangle(p, dim, t).det == 0.0) {
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

}  // namespace

extern "C" long pdg_mesh_fields_scratch_bytes(int n_nodes, int n_faces) {
  if (!sizes_ok(n_nodes, n_faces)) return -1;
  return (long)std::max(label_layout(n_nodes, n_faces, nullptr, nullptr),
                        div_layout(n_nodes, n_faces, nullptr, nullptr));
}

extern "C" int pdg_node_labels(int n_nodes, const float* points, int dim, int n_faces, const int64_t* faces,
                               int64_t* labels, int* info, void* scratch, long scratch_bytes, void* stream) {
  PDG_CHECK_ARG(sizes_ok(n_nodes, n_faces) && (dim == 2 || dim == 3),
                "pdg_node_labels: bad sizes (n_nodes > 0, n_faces >= 0, dim 2 or 3, n_nodes + 1024 and "
                "9 n_faces + 1024 < 2^31)");
  PDG_CHECK_ARG(points && labels && info && scratch && (faces || n_faces == 0), "pdg_node_labels: null argument");
  PDG_CHECK_ARG(scratch_bytes >= pdg_mesh_fields_scratch_bytes(n_nodes, n_faces),
                "pdg_node_labels: scratch too small");
  hipStream_t st = (hipStream_t)stream;
  LabelScratch s;
  label_layout(n_nodes, n_faces, &s, (char*)scratch);
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
    hipLaunchKernelGGL(label_face_kernel, dim3(grid_for(n_faces)), dim3(PT), 0, st, n_faces, faces, n_nodes, s.fok, cnt,
                       info + 2);
  group(EdgeByMin{faces, s.fok, s.sorted}, 3L * n_faces, n_nodes, cnt, fill, s.bsum, s.slots, st);
  hipLaunchKernelGGL(boundary_kernel, dim3(grid_for(n)), dim3(PT), 0, st, n_nodes, cnt, s.sorted, 0, bdeg, bcnt, s.lab,
                     (const int*)nullptr, (int*)nullptr, (int*)nullptr);
  scan(n_nodes, bcnt, s.bsum, st);
  hipLaunchKernelGGL(boundary_kernel, dim3(grid_for(n)), dim3(PT), 0, st, n_nodes, cnt, s.sorted, 1, (int*)nullptr,
                     (int*)nullptr, (int*)nullptr, bcnt, s.be_u, s.be_v);
  hipLaunchKernelGGL(components_kernel, dim3(1), dim3(CT), 0, st, n_nodes, bcnt, s.be_u, s.be_v, s.lab, info);
  hipLaunchKernelGGL(external_kernel, dim3(grid_for(n)), dim3(PT), 0, st, n_nodes, points, dim, s.bbox, nbb, bdeg,
                     s.lab, ext, info);
  hipLaunchKernelGGL(labels_kernel, dim3(grid_for(n)), dim3(PT), 0, st, n_nodes, bdeg, s.lab, ext, labels, info);
  PDG_CHECK_LAUNCH("pdg_node_labels");
  return PDG_OK;
}

extern "C" int pdg_p1_div_operator(int n_nodes, const float* points, int dim, int n_faces, const int64_t* faces,
                                   int64_t* rows, int64_t* cols, float* vals, long capacity, int* nnz, int* status,
                                   void* scratch, long scratch_bytes, void* stream) {
  PDG_CHECK_ARG(sizes_ok(n_nodes, n_faces) && (dim == 2 || dim == 3),
                "pdg_p1_div_operator: bad sizes (n_nodes > 0, n_faces >= 0, dim 2 or 3, n_nodes + 1024 and "
                "9 n_faces + 1024 < 2^31)");
  PDG_CHECK_ARG(points && nnz && status && scratch && (faces || n_faces == 0), "pdg_p1_div_operator: null argument");
  PDG_CHECK_ARG(n_faces == 0 || (rows && cols && vals), "pdg_p1_div_operator: null argument");
  PDG_CHECK_ARG(scratch_bytes >= pdg_mesh_fields_scratch_bytes(n_nodes, n_faces),
                "pdg_p1_div_operator: scratch too small");
  PDG_CHECK_ARG(capacity >= 18L * n_faces, "pdg_p1_div_operator: capacity below 18 * faces");
  hipStream_t st = (hipStream_t)stream;
  DivScratch s;
  div_layout(n_nodes, n_faces, &s, (char*)scratch);
  const long n = n_nodes;
  int* cnt = s.zero;             // [n + 1]
  int* fill = cnt + n + 1;       // [n]
  int* ucnt = fill + n;          // [n + 1]
  hipLaunchKernelGGL(clear_kernel, dim3(grid_for(3 * n + 2)), dim3(PT), 0, st, s.zero, 3 * n + 2, nnz, 1L,
                     (int*)nullptr, 0L, status);
  if (n_faces > 0)
    hipLaunchKernelGGL(div_face_kernel, dim3(grid_for(n_faces)), dim3(PT), 0, st, n_faces, faces, n_nodes, points, dim,
                       s.fok, cnt, status);
  group(PairByRow{faces, s.fok, s.sorted}, 9L * n_faces, n_nodes, cnt, fill, s.bsum, s.slots, st);
  hipLaunchKernelGGL(div_count_kernel, dim3(grid_for(n)), dim3(PT), 0, st, n_nodes, cnt, s.sorted, ucnt);
  scan(n_nodes, ucnt, s.bsum, st);
  hipLaunchKernelGGL(div_emit_kernel, dim3(grid_for(n)), dim3(PT), 0, st, n_nodes, points, dim, faces, cnt, s.sorted,
                     ucnt, rows, cols, vals, nnz);
  PDG_CHECK_LAUNCH("pdg_p1_div_operator");
  return PDG_OK;
}

extern "C" int pdg_nodal_areas(int n_nodes, const float* points, int dim, int n_faces, const int64_t* faces,
                               float* area, float* bbox, int* status, void* scratch, long scratch_bytes,
                               void* stream) {
  PDG_CHECK_ARG(sizes_ok(n_nodes, n_faces) && (dim == 2 || dim == 3),
                "pdg_nodal_areas: bad sizes (n_nodes > 0, n_faces >= 0, dim 2 or 3, n_nodes + 1024 and "
                "9 n_faces + 1024 < 2^31)");
  PDG_CHECK_ARG(points && area && bbox && status && scratch && (faces || n_faces == 0),
                "pdg_nodal_areas: null argument");
  PDG_CHECK_ARG(scratch_bytes >= pdg_mesh_fields_scratch_bytes(n_nodes, n_faces),
                "pdg_nodal_areas: scratch too small");
  hipStream_t st = (hipStream_t)stream;
  LabelScratch s;   // the labels' layout holds all that is needed here: bbox, cnt | fill, bsum, fok, 3 F slots twice
  label_layout(n_nodes, n_faces, &s, (char*)scratch);
  const long n = n_nodes;
  int* cnt = s.zero;             // [n + 1]
  int* fill = cnt + n + 1;       // [n]
  const int nbb = bbox_blocks(n_nodes);
  hipLaunchKernelGGL(bbox_kernel, dim3(nbb), dim3(BBOX_T), 0, st, n_nodes, points, dim, s.bbox, s.ctr);
  hipLaunchKernelGGL(clear_kernel, dim3(grid_for(2 * n + 1)), dim3(PT), 0, st, s.zero, 2 * n + 1, (int*)nullptr, 0L,
                     (int*)nullptr, 0L, status);
  if (n_faces > 0)
    hipLaunchKernelGGL(area_face_kernel, dim3(grid_for(n_faces)), dim3(PT), 0, st, n_faces, faces, n_nodes, s.fok, cnt,
                       status);
  group(FaceByNode{faces, s.fok, s.sorted}, 3L * n_faces, n_nodes, cnt, fill, s.bsum, s.slots, st);
  hipLaunchKernelGGL(area_emit_kernel, dim3(grid_for(n)), dim3(PT), 0, st, n_nodes, points, dim, faces, cnt, s.sorted,
                     s.bbox, nbb, area, bbox);
  PDG_CHECK_LAUNCH("pdg_nodal_areas");
  return PDG_OK;
}

extern "C" long pdg_boundary_vectors_scratch_bytes(int n_nodes, int n_faces) {
  if (!sizes_ok(n_nodes, n_faces)) return -1;
  return (long)bvec_layout(n_nodes, n_faces, nullptr, nullptr);
}

extern "C" int pdg_boundary_vectors(int n_nodes, const float* points, int dim, int n_faces, const int64_t* faces,
                                    float* bvec, float* blen, int* status, void* scratch, long scratch_bytes,
                                    void* stream) {
  PDG_CHECK_ARG(sizes_ok(n_nodes, n_faces) && (dim == 2 || dim == 3),
                "pdg_boundary_vectors: bad sizes (n_nodes > 0, n_faces >= 0, dim 2 or 3, n_nodes + 1024 and "
                "9 n_faces + 1024 < 2^31)");
  PDG_CHECK_ARG(points && bvec && blen && status && scratch && (faces || n_faces == 0),
                "pdg_boundary_vectors: null argument");
  PDG_CHECK_ARG(scratch_bytes >= pdg_boundary_vectors_scratch_bytes(n_nodes, n_faces),
                "pdg_boundary_vectors: scratch too small");
  hipStream_t st = (hipStream_t)stream;
  BvecScratch s;
  bvec_layout(n_nodes, n_faces, &s, (char*)scratch);
  const long n = n_nodes;
  int* cnt = s.zero;             // [n + 1]
  int* fill = cnt + n + 1;       // [n]
  int* cnt2 = fill + n;          // [n + 1]
  int* fill2 = cnt2 + n + 1;     // [n]
  hipLaunchKernelGGL(clear_kernel, dim3(grid_for(4 * n + 2)), dim3(PT), 0, st, s.zero, 4 * n + 2, (int*)nullptr, 0L,
                     (int*)nullptr, 0L, status);
  if (n_faces > 0)
    hipLaunchKernelGGL(label_face_kernel, dim3(grid_for(n_faces)), dim3(PT), 0, st, n_faces, faces, n_nodes, s.fok, cnt,
                       status);
  group(EdgeByMin{faces, s.fok, s.sorted}, 3L * n_faces, n_nodes, cnt, fill, s.bsum, s.slots, st);
  hipLaunchKernelGGL(bvec_mark_kernel, dim3(grid_for(n)), dim3(PT), 0, st, n_nodes, cnt, s.sorted, s.brow, cnt2);
  group(EndByNode{cnt, n_nodes, s.brow, s.sorted, s.sorted2}, 6L * n_faces, n_nodes, cnt2, fill2, s.bsum, s.slots, st);
  hipLaunchKernelGGL(bvec_emit_kernel, dim3(grid_for(n)), dim3(PT), 0, st, n_nodes, points, dim, faces, cnt2, s.sorted2,
                     s.sorted, bvec, blen, status);
  PDG_CHECK_LAUNCH("pdg_boundary_vectors");
  return PDG_OK;
}
