// The sampling operator S of a mesh: a nodal field's values at arbitrary query points, and S^T.
//
//   pdg_cell_bins         a uniform gx x gy grid over the mesh's bounding box; bin b = by gx + bx lists the cells
//                         whose own bounding box, inflated by the containment tolerance, overlaps it (CSR)
//   pdg_locate_points     one thread per query: the containing cell (-1: none) and the interpolation weights
//   pdg_sample_field      out[q, c] = sum_k w[q, k] field[node_offset + faces[cell[q], k], c]
//   pdg_sample_csr        the node-major CSR of S: rowptr (n_nodes + 1) and entries q nv + k, ascending in a row
//   pdg_sample_field_bwd  gfield[n, c] = sum over the entries of n of w gout[q, c]: S^T, without atomics
//
// Bins.  The bounding box is pdg_bbox.hpp's.  bin_of() maps a coordinate to a bin index with one fp64 expression,
// monotone in the coordinate and clamped to the grid; the cells' kernel and the queries' kernel call the same
// function with the same box, so a query whose coordinate lies between a cell's inflated extremes falls into a
// bin between the bins of those extremes, which are the bins the cell entered.  The inflation: all weights >=
// -TOL and sum w = 1 give x - min x_k = sum w_k (x_k - min x_k) >= -(NV - 1) TOL (max x_k - min x_k), in exact
// arithmetic; the extents are inflated by 8 TOL times themselves, which leaves the rounding of the weights
// (~ 32 u d^2 / |A|, far below TOL = 2^-40 for any cell a mesher produces) as much room again.  Count (atomics
// on the bin counters), pdg_scan.hpp's exclusive scan, fill (atomics claim the slots).  The order of the cells
// inside a bin is whatever the atomics gave; nothing reads it as an order (below).  Cells of zero area (det == 0
// with pdg_cell.hpp's det, the mesh fields') and cells with a vertex index outside [0, n_nodes) enter no bin and are counted
// in info.  The total is kept in 64 bits; a slot is written only when its position is inside [0, capacity).
//
// Location.  Triangles: w_k = [(p_k+1 - p) x (p_k+2 - p)] / det, signed sub-area over signed area, so either
// orientation works and a query that is bitwise vertex k gets w_k = 1 and exact zeros elsewhere.  Quads: the CLOSED
// FORM of the inverse bilinear map, not Newton.  With e = b - a, f = d - a, g = a - b + c - d, h = p - a the map
// is h = e s + f t + g s t; eliminating s leaves F(t) = k2 t^2 + k1 t + k0 = 0, k2 = g x f, k1 = e x f + h x g,
// k0 = h x e, and at a root F'(t) = (e + g t) x (f + g s) = det J(s, t).  A convex quad has det J of one sign, the
// sign sg of its area, on the whole unit square, so the root wanted is the one with F'(t) = sg sqrt(disc):
//   t = -2 k0 / (k1 + sg sqrt(disc))   when sg k1 >= 0 (no cancellation; holds for k2 == 0, a trapezoid in t),
//   t = (sg sqrt(disc) - k1) / (2 k2)  otherwise (no cancellation either),
// then s = (h - f t) . v / v . v with v = e + g t, the segment between the two sides at t (not 0 for a convex quad).
// No iteration, so no count to justify; disc < 0, a zero denominator or v == 0 mean "not in this cell".  A
// non-convex quad has det J of both signs: the branch taken is the one on which det J has the sign of the whole
// area, so points of its well-oriented part are found, and points the bilinear map covers twice (past the reflex
// corner) or only on the other branch are reported as not contained.  Nothing is indexed with s or t.
// A cell contains the query iff every weight >= -TOL.  Among the containing cells of the bin the one with the
// largest smallest weight wins, the lowest cell id among equals: a total order on (smallest weight, id), so the
// result does not depend on the order inside the bin.
//
// Transpose.  The n_q NV items (q, k) of the located queries are grouped by node with pdg_group.hpp (minor key
// 0, so a row is in ascending q nv + k whatever the atomics' order; rows of any length, the bitonic network for the
// long ones).  pdg_sample_field_bwd walks a row in that order in fp64 and rounds once: bitwise reproducible.
//
// Arithmetic is fp64 from the fp32 inputs without contraction, each result rounded to fp32 once.  Every index read
// from memory (a face's vertices, a bin's range and cells, a query's cell, a row's range and entries) is checked
// against its array's length before it is used.  Kernel launches only, no host read.
#include <stdint.h>

#include <algorithm>
#include <cfloat>

#include "pdg_bbox.hpp"
#include "pdg_cell.hpp"
#include "pdg_group.hpp"
#include "pdg_runtime.hpp"
#include "pdg_scan.hpp"

using namespace pdg;

namespace {

constexpr double TOL = 0x1p-40;   // containment tolerance on a weight

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// ------------------------------------------------------------------------------------- bins
struct BinScratch {
  float* part;   // [BBOX_BLOCKS][4]
  int* ctr;      // [16], cleared by bbox_kernel: 0-1 the total (64 bits), 2 degenerate cells, 3 cells out of range
  int* fill;     // [gx gy]
  int* bsum;     // [scan blocks + 2]
};

size_t bin_layout(long nb, BinScratch* s, char* base) {
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + o : nullptr;
    o += align_up(bytes);
    return p;
  };
  BinScratch t;
  t.part = (float*)take(4 * sizeof(float) * BBOX_BLOCKS);
  t.ctr = (int*)take(16 * sizeof(int));
  t.fill = (int*)take(sizeof(int) * (size_t)nb);
  t.bsum = (int*)take(sizeof(int) * scan_bsum_len((int)nb));
  if (s) *s = t;
  return o;
}

bool grid_ok(int gx, int gy) {
  // the scan indexes base + i < gx gy + SCAN_BLOCK in int32
  return gx >= 1 && gy >= 1 && (long)gx * gy + SCAN_BLOCK < 0x7fffffffL;
}

// an item position q nv + k is an int32
bool nq_ok(long n_q, int nv) { return n_q >= 0 && n_q < 0x7fffffffL && n_q * nv < 0x7fffffffL; }

bool mesh_ok(int n_nodes, int n_faces, int nv, int dim) {
  return n_nodes > 0 && n_faces >= 0 && (long)nv * n_faces < 0x7fffffffL && (dim == 2 || dim == 3);
}

// The grid over the box: (x0, y0) the lower corner, (lx, ly) the extents, (ix, iy) = bins per unit length.
struct Box {
  double x0, y0, x1, y1, lx, ly, ix, iy;
  bool ok;   // both extents > 0
};

__device__ __forceinline__ Box box_of(const float* __restrict__ bbox, int gx, int gy) {
#pragma clang fp contract(off)
  Box b;
  b.x0 = bbox[0];
  b.y0 = bbox[1];
  b.x1 = bbox[2];
  b.y1 = bbox[3];
  b.lx = b.x1 - b.x0;
  b.ly = b.y1 - b.y0;
  b.ok = b.lx > 0.0 && b.ly > 0.0;
  b.ix = b.ok ? (double)gx / b.lx : 0.0;
  b.iy = b.ok ? (double)gy / b.ly : 0.0;
  return b;
}

// Bin of coordinate x along one axis: monotone in x, inside [0, g).
__device__ __forceinline__ int bin_of(double x, double x0, double inv, int g) {
#pragma clang fp contract(off)
  const double f = (x - x0) * inv;
  if (!(f >= 0.0)) return 0;
  if (f >= (double)g) return g - 1;
  return (int)f;
}

enum { CELL_OK = 0, CELL_DEGENERATE = 1, CELL_RANGE = 2 };

// The bins [bx0, bx1] x [by0, by1] cell f enters; CELL_OK when it enters any.
template <int NV>
__device__ __forceinline__ int cell_bin_range(const float* __restrict__ p, int dim, const int64_t* __restrict__ t,
                                              int n_nodes, const Box& b, int gx, int gy, int& bx0, int& bx1,
                                              int& by0, int& by1) {
#pragma clang fp contract(off)
  if (!in_range<NV>(t, n_nodes)) return CELL_RANGE;
  const Cell<NV> c = cell_of<NV>(p, dim, t);
  if (!(c.det != 0.0) || !b.ok) return CELL_DEGENERATE;   // a NaN det is degenerate too
  double mnx = c.x[0], mxx = c.x[0], mny = c.y[0], mxy = c.y[0];
#pragma unroll
  for (int v = 1; v < NV; ++v) {
    mnx = fmin(mnx, c.x[v]);
    mxx = fmax(mxx, c.x[v]);
    mny = fmin(mny, c.y[v]);
    mxy = fmax(mxy, c.y[v]);
  }
  const double ex = 8.0 * TOL * (mxx - mnx), ey = 8.0 * TOL * (mxy - mny);
  bx0 = bin_of(mnx - ex, b.x0, b.ix, gx);
  bx1 = bin_of(mxx + ex, b.x0, b.ix, gx);
  by0 = bin_of(mny - ey, b.y0, b.iy, gy);
  by1 = bin_of(mxy + ey, b.y0, b.iy, gy);
  return CELL_OK;
}

// Clears the counters and the row pointer; block 0 folds the box.
__global__ __launch_bounds__(PT) void bins_init_kernel(long nb, int* __restrict__ bin_ptr, int* __restrict__ fill,
                                                       const float* __restrict__ part, int nparts,
                                                       float* __restrict__ bbox) {
  const long stride = (long)gridDim.x * PT;
  const long t0 = (long)blockIdx.x * PT + threadIdx.x;
  for (long i = t0; i <= nb; i += stride) bin_ptr[i] = 0;
  for (long i = t0; i < nb; i += stride) fill[i] = 0;
  if (blockIdx.x == 0) {
    __shared__ float bb[4];
    bbox_load(part, nparts, bb);
    if (threadIdx.x < 4) bbox[threadIdx.x] = bb[threadIdx.x];
  }
}

template <int NV>
__global__ __launch_bounds__(PT) void bins_count_kernel(int nf, const int64_t* __restrict__ faces, int n_nodes,
                                                        const float* __restrict__ p, int dim,
                                                        const float* __restrict__ bbox, int gx, int gy,
                                                        int* __restrict__ bin_ptr, int* __restrict__ ctr) {
  const Box b = box_of(bbox, gx, gy);
  unsigned long long total = 0;
  int ndeg = 0, nbad = 0;
  for (long f = (long)blockIdx.x * PT + threadIdx.x; f < nf; f += (long)gridDim.x * PT) {
    int bx0, bx1, by0, by1;
    const int why = cell_bin_range<NV>(p, dim, faces + NV * f, n_nodes, b, gx, gy, bx0, bx1, by0, by1);
    if (why == CELL_OK) {
      for (int by = by0; by <= by1; ++by)
        for (int bx = bx0; bx <= bx1; ++bx) atomicAdd(&bin_ptr[(long)by * gx + bx], 1);
      total += (unsigned long long)(by1 - by0 + 1) * (unsigned long long)(bx1 - bx0 + 1);
    } else if (why == CELL_DEGENERATE) {
      ++ndeg;
    } else {
      ++nbad;
    }
  }
  if (total) atomicAdd((unsigned long long*)ctr, total);
  if (ndeg) atomicAdd(&ctr[2], ndeg);
  if (nbad) atomicAdd(&ctr[3], nbad);
}

template <int NV>
__global__ __launch_bounds__(PT) void bins_fill_kernel(int nf, const int64_t* __restrict__ faces, int n_nodes,
                                                       const float* __restrict__ p, int dim,
                                                       const float* __restrict__ bbox, int gx, int gy,
                                                       const int* __restrict__ bin_ptr, int* __restrict__ fill,
                                                       int* __restrict__ bin_cells, long capacity,
                                                       const int* __restrict__ ctr, int* __restrict__ info) {
  const Box b = box_of(bbox, gx, gy);
  for (long f = (long)blockIdx.x * PT + threadIdx.x; f < nf; f += (long)gridDim.x * PT) {
    int bx0, bx1, by0, by1;
    if (cell_bin_range<NV>(p, dim, faces + NV * f, n_nodes, b, gx, gy, bx0, bx1, by0, by1) != CELL_OK) continue;
    for (int by = by0; by <= by1; ++by)
      for (int bx = bx0; bx <= bx1; ++bx) {
        const long bin = (long)by * gx + bx;
        const long pos = (long)bin_ptr[bin] + atomicAdd(&fill[bin], 1);
        if (pos >= 0 && pos < capacity) bin_cells[pos] = (int)f;
      }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const unsigned long long total = *(const unsigned long long*)ctr;
    info[0] = total > 0x7fffffffULL ? 0x7fffffff : (int)total;
    info[1] = total > (unsigned long long)capacity ? 1 : 0;
    info[2] = ctr[2];
    info[3] = ctr[3];
  }
}

// ---------------------------------------------------------------------------------- weights
// false: the point is in no relation to the cell that weights could express (never for a triangle of det != 0).
template <int NV>
__device__ __forceinline__ bool cell_weights(const Cell<NV>& c, double px, double py, double (&w)[NV]) {
#pragma clang fp contract(off)
  if constexpr (NV == 3) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
      const double m0 = (c.x[k1] - px) * (c.y[k2] - py);
      const double m1 = (c.x[k2] - px) * (c.y[k1] - py);
      w[k] = (m0 - m1) / c.det;
    }
    return true;
  } else {
    const double ex = c.x[1] - c.x[0], ey = c.y[1] - c.y[0];
    const double fx = c.x[3] - c.x[0], fy = c.y[3] - c.y[0];
    const double gx = (c.x[0] - c.x[1]) + (c.x[2] - c.x[3]), gy = (c.y[0] - c.y[1]) + (c.y[2] - c.y[3]);
    const double hx = px - c.x[0], hy = py - c.y[0];
    const double k2 = gx * fy - gy * fx;
    const double k1 = (ex * fy - ey * fx) + (hx * gy - hy * gx);
    const double k0 = hx * ey - hy * ex;
    const double disc = k1 * k1 - 4.0 * k0 * k2;
    if (!(disc >= 0.0)) return false;
    const double sr = c.det > 0.0 ? sqrt(disc) : -sqrt(disc);
    double t;
    if ((c.det > 0.0) == (k1 >= 0.0) || k1 == 0.0) {
      const double den = k1 + sr;
      if (den == 0.0) return false;
      t = -2.0 * k0 / den;
    } else {
      if (k2 == 0.0) return false;
      t = (sr - k1) / (2.0 * k2);
    }
    const double vx = ex + gx * t, vy = ey + gy * t;
    const double vv = vx * vx + vy * vy;
    if (!(vv > 0.0)) return false;
    const double s = ((hx - fx * t) * vx + (hy - fy * t) * vy) / vv;
    w[0] = (1.0 - s) * (1.0 - t);
    w[1] = s * (1.0 - t);
    w[2] = s * t;
    w[3] = (1.0 - s) * t;
    return true;
  }
}

struct LocateArgs {
  int n_nodes, dim, n_faces, gx, gy, periodic;
  long capacity, n_q;
  const float* points;
  const int64_t* faces;
  const int* bin_ptr;
  const int* bin_cells;
  const float* bbox;
  const float* queries;
  int* cell;
  float* weights;
  int* n_outside;
};

template <int NV>
__global__ __launch_bounds__(PT) void locate_kernel(LocateArgs a) {
#pragma clang fp contract(off)
  __shared__ int s_out;
  if (threadIdx.x == 0) s_out = 0;
  __syncthreads();
  const Box b = box_of(a.bbox, a.gx, a.gy);
  int nout = 0;
  for (long q = (long)blockIdx.x * PT + threadIdx.x; q < a.n_q; q += (long)gridDim.x * PT) {
    double x = a.queries[2 * q], y = a.queries[2 * q + 1];
    bool in = b.ok;
    if (in && a.periodic) {
      x = x - floor((x - b.x0) / b.lx) * b.lx;
      y = y - floor((y - b.y0) / b.ly) * b.ly;
      in = x == x && y == y;   // a NaN or infinite query wraps to NaN
    } else if (in) {
      in = x >= b.x0 && x <= b.x1 && y >= b.y0 && y <= b.y1;
    }
    int best = -1;
    double bmin = 0.0, bw[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) bw[k] = 0.0;
    if (in) {
      const long bin = (long)bin_of(y, b.y0, b.iy, a.gy) * a.gx + bin_of(x, b.x0, b.ix, a.gx);
      long beg = a.bin_ptr[bin], end = a.bin_ptr[bin + 1];
      beg = beg < 0 ? 0 : beg;
      end = end > a.capacity ? a.capacity : end;
      for (long e = beg; e < end; ++e) {
        const int f = a.bin_cells[e];
        if (f < 0 || f >= a.n_faces) continue;
        const int64_t* t = a.faces + (long)NV * f;
        if (!in_range<NV>(t, a.n_nodes)) continue;
        const Cell<NV> c = cell_of<NV>(a.points, a.dim, t);
        if (!(c.det != 0.0)) continue;
        double w[NV];
        if (!cell_weights<NV>(c, x, y, w)) continue;
        double mn = w[0];
        bool ok = w[0] >= -TOL;
#pragma unroll
        for (int k = 1; k < NV; ++k) {
          ok = ok && w[k] >= -TOL;   // false for a NaN weight
          mn = fmin(mn, w[k]);
        }
        if (ok && (best < 0 || mn > bmin || (mn == bmin && f < best))) {
          best = f;
          bmin = mn;
#pragma unroll
          for (int k = 0; k < NV; ++k) bw[k] = w[k];
        }
      }
    }
    a.cell[q] = best;
#pragma unroll
    for (int k = 0; k < NV; ++k) a.weights[NV * q + k] = bw[k] > 0.0 ? (float)bw[k] : 0.0f;
    nout += best < 0;
  }
  if (nout) atomicAdd(&s_out, nout);
  __syncthreads();
  if (threadIdx.x == 0 && s_out) atomicAdd(a.n_outside, s_out);
}

__global__ void clear_word_kernel(int* __restrict__ w) { *w = 0; }

// ----------------------------------------------------------------------------------- sample
__global__ __launch_bounds__(PT) void sample_kernel(long n_q, int nv, int n_faces, const int64_t* __restrict__ faces,
                                                    const int* __restrict__ cell, const float* __restrict__ weights,
                                                    const float* __restrict__ field, long n_rows, int n_cols,
                                                    long node_offset, float fill, float* __restrict__ out) {
  const long total = n_q * n_cols;
  for (long i = (long)blockIdx.x * PT + threadIdx.x; i < total; i += (long)gridDim.x * PT) {
    const long q = i / n_cols;
    const int c = (int)(i - q * n_cols);
    const int f = cell[q];
    bool ok = f >= 0 && f < n_faces;
    double acc = 0.0;
    for (int k = 0; ok && k < nv; ++k) {
      const int64_t v = faces[(long)nv * f + k];
      const long row = node_offset + (long)v;
      ok = v >= 0 && row >= 0 && row < n_rows;
      if (ok) acc += (double)weights[nv * q + k] * (double)field[row * n_cols + c];   // the product is exact
    }
    out[i] = ok ? (float)acc : fill;
  }
}

// -------------------------------------------------------------------------------- transpose
struct CsrScratch {
  int* fill;    // [n_nodes]
  int* bsum;    // [scan blocks + 2]
  u64* slots;   // [n_q nv]
};

size_t csr_layout(int n, long m, CsrScratch* s, char* base) {
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + o : nullptr;
    o += align_up(bytes);
    return p;
  };
  CsrScratch t;
  t.fill = (int*)take(sizeof(int) * (size_t)n);
  t.bsum = (int*)take(sizeof(int) * scan_bsum_len(n));
  t.slots = (u64*)take(sizeof(u64) * (size_t)std::max<long>(m, 1));
  if (s) *s = t;
  return o;
}

bool csr_ok(int n_nodes, long n_q, int nv) {
  // the scan indexes base + i < n + SCAN_BLOCK in int32; an item position q nv + k fills a slot's low word
  return (nv == 3 || nv == 4) && n_nodes > 0 && (long)n_nodes + SCAN_BLOCK < 0x7fffffffL && nq_ok(n_q, nv);
}

// The items (q, k) of the located queries grouped by node, a row in ascending q nv + k.
struct ByNode {
  const int64_t* faces;
  const int* cell;
  int nv, n_faces, n_nodes;
  int* entries;
  // 0: kept, 1: the query is outside, 2: an index is out of range
  __device__ int look(long i, int& node) const {
    const long q = i / nv;
    const int f = cell[q];
    if (f == -1) return 1;
    if (f < 0 || f >= n_faces) return 2;
    const int64_t v = faces[(long)nv * f + (i - q * nv)];
    if (v < 0 || v >= n_nodes) return 2;
    node = (int)v;
    return 0;
  }
  __device__ bool item(long i, int& major, unsigned& minor) const {
    minor = 0;
    return look(i, major) == 0;
  }
  __device__ void emit(long k, int, u64 slot) const { entries[k] = (int)(slot & 0xffffffffu); }
};

__global__ __launch_bounds__(PT) void csr_count_kernel(ByNode p, long m, int* __restrict__ cnt,
                                                       int* __restrict__ status) {
  int bad = 0;
  for (long i = (long)blockIdx.x * PT + threadIdx.x; i < m; i += (long)gridDim.x * PT) {
    int node;
    const int r = p.look(i, node);
    if (r == 0) atomicAdd(&cnt[node], 1);
    bad |= r == 2;
  }
  if (bad) atomicOr(status, 1);
}

__global__ __launch_bounds__(PT) void sample_bwd_kernel(int n_nodes, long m, int nv, const int* __restrict__ rowptr,
                                                        const int* __restrict__ entries,
                                                        const float* __restrict__ weights,
                                                        const float* __restrict__ gout, int n_cols,
                                                        float* __restrict__ gfield) {
  const long total = (long)n_nodes * n_cols;
  for (long i = (long)blockIdx.x * PT + threadIdx.x; i < total; i += (long)gridDim.x * PT) {
    const long n = i / n_cols;
    const int c = (int)(i - n * n_cols);
    long beg = rowptr[n], end = rowptr[n + 1];
    beg = beg < 0 ? 0 : beg;
    end = end > m ? m : end;
    double acc = 0.0;
    for (long e = beg; e < end; ++e) {
      const int it = entries[e];
      if (it < 0 || it >= m) continue;
      acc += (double)weights[it] * (double)gout[(long)(it / nv) * n_cols + c];   // the product is exact
    }
    gfield[i] = (float)acc;
  }
}

}  // namespace

#define SAMPLE_CHECK_NV(name, nv) \
  PDG_CHECK_ARG((nv) == 3 || (nv) == 4, "%s: nv must be 3 (triangles) or 4 (quads), got %d", name, (int)(nv))

extern "C" long pdg_cell_bins_scratch_bytes(int gx, int gy) {
  if (!grid_ok(gx, gy)) return -1;
  return (long)bin_layout((long)gx * gy, nullptr, nullptr);
}

extern "C" int pdg_cell_bins(int n_nodes, const float* points, int dim, int n_faces, int nv, const int64_t* faces,
                             int gx, int gy, int* bin_ptr, int* bin_cells, long capacity, float* bbox, int* info,
                             void* scratch, long scratch_bytes, void* stream) {
  SAMPLE_CHECK_NV("pdg_cell_bins", nv);
  PDG_CHECK_ARG(mesh_ok(n_nodes, n_faces, nv, dim) && grid_ok(gx, gy) && capacity >= 1 && capacity < 0x7fffffffL,
                "pdg_cell_bins: bad sizes (n_nodes > 0, n_faces >= 0, dim 2 or 3, gx, gy >= 1, nv n_faces, "
                "gx gy + 1024 and 1 <= capacity < 2^31)");
  PDG_CHECK_ARG(points && bin_ptr && bin_cells && bbox && info && scratch && (faces || n_faces == 0),
                "pdg_cell_bins: null argument");
  const long nb = (long)gx * gy;
  PDG_CHECK_ARG(scratch_bytes >= (long)bin_layout(nb, nullptr, nullptr), "pdg_cell_bins: scratch too small");
  hipStream_t st = (hipStream_t)stream;
  BinScratch s;
  bin_layout(nb, &s, (char*)scratch);
  const int nparts = bbox_blocks(n_nodes);
  hipLaunchKernelGGL(bbox_kernel, dim3(nparts), dim3(BBOX_T), 0, st, n_nodes, points, dim, s.part, s.ctr);
  hipLaunchKernelGGL(bins_init_kernel, dim3(grid_for(nb + 1)), dim3(PT), 0, st, nb, bin_ptr, s.fill, s.part, nparts,
                     bbox);
  const int g = grid_for(n_faces);
  if (nv == 3)
    hipLaunchKernelGGL(bins_count_kernel<3>, dim3(g), dim3(PT), 0, st, n_faces, faces, n_nodes, points, dim, bbox, gx,
                       gy, bin_ptr, s.ctr);
  else
    hipLaunchKernelGGL(bins_count_kernel<4>, dim3(g), dim3(PT), 0, st, n_faces, faces, n_nodes, points, dim, bbox, gx,
                       gy, bin_ptr, s.ctr);
  scan((int)nb, bin_ptr, s.bsum, st);
  if (nv == 3)
    hipLaunchKernelGGL(bins_fill_kernel<3>, dim3(g), dim3(PT), 0, st, n_faces, faces, n_nodes, points, dim, bbox, gx,
                       gy, bin_ptr, s.fill, bin_cells, capacity, s.ctr, info);
  else
    hipLaunchKernelGGL(bins_fill_kernel<4>, dim3(g), dim3(PT), 0, st, n_faces, faces, n_nodes, points, dim, bbox, gx,
                       gy, bin_ptr, s.fill, bin_cells, capacity, s.ctr, info);
  PDG_CHECK_LAUNCH("pdg_cell_bins");
  return PDG_OK;
}

extern "C" int pdg_locate_points(int n_nodes, const float* points, int dim, int n_faces, int nv, const int64_t* faces,
                                 int gx, int gy, const int* bin_ptr, const int* bin_cells, long capacity,
                                 const float* bbox, int periodic, long n_q, const float* queries, int* cell,
                                 float* weights, int* n_outside, void* stream) {
  SAMPLE_CHECK_NV("pdg_locate_points", nv);
  PDG_CHECK_ARG(mesh_ok(n_nodes, n_faces, nv, dim) && grid_ok(gx, gy) && capacity >= 1 && capacity < 0x7fffffffL &&
                    nq_ok(n_q, nv),
                "pdg_locate_points: bad sizes (n_nodes > 0, n_faces >= 0, dim 2 or 3, gx, gy >= 1, n_q >= 0, "
                "nv n_faces, nv n_q, gx gy + 1024 and 1 <= capacity < 2^31)");
  PDG_CHECK_ARG(points && bin_ptr && bin_cells && bbox && n_outside && (faces || n_faces == 0),
                "pdg_locate_points: null argument");
  PDG_CHECK_ARG(n_q == 0 || (queries && cell && weights), "pdg_locate_points: null argument");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(clear_word_kernel, dim3(1), dim3(1), 0, st, n_outside);
  if (n_q > 0) {
    const LocateArgs a{n_nodes, dim,   n_faces,   gx,   gy,      periodic ? 1 : 0, capacity, n_q,      points,
                       faces,   bin_ptr, bin_cells, bbox, queries, cell,             weights,  n_outside};
    if (nv == 3)
      hipLaunchKernelGGL(locate_kernel<3>, dim3(grid_for(n_q)), dim3(PT), 0, st, a);
    else
      hipLaunchKernelGGL(locate_kernel<4>, dim3(grid_for(n_q)), dim3(PT), 0, st, a);
  }
  PDG_CHECK_LAUNCH("pdg_locate_points");
  return PDG_OK;
}

extern "C" int pdg_sample_field(long n_q, int n_faces, int nv, const int64_t* faces, const int* cell,
                                const float* weights, const float* field, long n_rows, int n_cols, long node_offset,
                                float fill, float* out, void* stream) {
  SAMPLE_CHECK_NV("pdg_sample_field", nv);
  PDG_CHECK_ARG(nq_ok(n_q, nv) && n_faces >= 0 && (long)nv * n_faces < 0x7fffffffL &&
                    n_rows > 0 && n_cols >= 1 && node_offset >= 0 && node_offset < n_rows,
                "pdg_sample_field: bad sizes (n_q >= 0, n_faces >= 0, nv n_q and nv n_faces < 2^31, n_rows > 0, "
                "n_cols >= 1, 0 <= node_offset < n_rows)");
  PDG_CHECK_ARG(field && (faces || n_faces == 0) && (n_q == 0 || (cell && weights && out)),
                "pdg_sample_field: null argument");
  if (n_q > 0)
    hipLaunchKernelGGL(sample_kernel, dim3(grid_for(n_q * n_cols)), dim3(PT), 0, (hipStream_t)stream, n_q, nv,
                       n_faces, faces, cell, weights, field, n_rows, n_cols, node_offset, fill, out);
  PDG_CHECK_LAUNCH("pdg_sample_field");
  return PDG_OK;
}

extern "C" long pdg_sample_csr_scratch_bytes(int n_nodes, long n_q, int nv) {
  if (!csr_ok(n_nodes, n_q, nv)) return -1;
  return (long)csr_layout(n_nodes, n_q * nv, nullptr, nullptr);
}

extern "C" int pdg_sample_csr(int n_nodes, int n_faces, int nv, const int64_t* faces, long n_q, const int* cell,
                              int* rowptr, int* entries, int* status, void* scratch, long scratch_bytes,
                              void* stream) {
  SAMPLE_CHECK_NV("pdg_sample_csr", nv);
  PDG_CHECK_ARG(csr_ok(n_nodes, n_q, nv) && n_faces >= 0 && (long)nv * n_faces < 0x7fffffffL,
                "pdg_sample_csr: bad sizes (n_nodes > 0, n_faces >= 0, n_q >= 0, n_nodes + 1024, nv n_faces and "
                "nv n_q < 2^31)");
  PDG_CHECK_ARG(rowptr && status && scratch && (faces || n_faces == 0) && (n_q == 0 || (cell && entries)),
                "pdg_sample_csr: null argument");
  const long m = n_q * nv;
  PDG_CHECK_ARG(scratch_bytes >= (long)csr_layout(n_nodes, m, nullptr, nullptr), "pdg_sample_csr: scratch too small");
  hipStream_t st = (hipStream_t)stream;
  CsrScratch s;
  csr_layout(n_nodes, m, &s, (char*)scratch);
  const long n1 = (long)n_nodes + 1;
  hipLaunchKernelGGL(clear_kernel, dim3(grid_for(n1)), dim3(PT), 0, st, rowptr, n1, s.fill, (long)n_nodes,
                     (int*)nullptr, 0L, status);
  const ByNode p{faces, cell, nv, n_faces, n_nodes, entries};
  if (m > 0) hipLaunchKernelGGL(csr_count_kernel, dim3(grid_for(m)), dim3(PT), 0, st, p, m, rowptr, status);
  group(p, m, n_nodes, rowptr, s.fill, s.bsum, s.slots, st);
  PDG_CHECK_LAUNCH("pdg_sample_csr");
  return PDG_OK;
}

extern "C" int pdg_sample_field_bwd(int n_nodes, long n_q, int nv, const int* rowptr, const int* entries,
                                    const float* weights, const float* gout, int n_cols, float* gfield,
                                    void* stream) {
  SAMPLE_CHECK_NV("pdg_sample_field_bwd", nv);
  PDG_CHECK_ARG(n_nodes > 0 && nq_ok(n_q, nv) && n_cols >= 1,
                "pdg_sample_field_bwd: bad sizes (n_nodes > 0, n_q >= 0, nv n_q < 2^31, n_cols >= 1)");
  PDG_CHECK_ARG(rowptr && gfield && (n_q == 0 || (entries && weights && gout)),
                "pdg_sample_field_bwd: null argument");
  hipLaunchKernelGGL(sample_bwd_kernel, dim3(grid_for((long)n_nodes * n_cols)), dim3(PT), 0, (hipStream_t)stream,
                     n_nodes, n_q * nv, nv, rowptr, entries, weights, gout, n_cols, gfield);
  PDG_CHECK_LAUNCH("pdg_sample_field_bwd");
  return PDG_OK;
}
