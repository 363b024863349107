// Boundary residuals of a plane-stress field: what the field does where the physics is set, on the boundary of the
// periodic cell.  With the lumped outward boundary vectors of pdg_boundary_vectors (pdg_meshfields.hip), the nodal
// boundary force is f(n) = sigma(n) . bvec[n] (the lumped traction integral).  Per graph: the integral of the
// squared traction over the hole's edge (zero for a traction-free hole), the net forces on the hole and on the
// cell, and the mean-square jump of sigma across the periodic connections (the zero-length edges of
// compute_periodic_graph, datasets.py:39-119); and the gradient of the two mean squares with respect to sigma.
// As the stress criteria (pdg_criteria.hip) and the homogenisation (pdg_homog.hip): segmented by the batch's node
// offsets `ptr`, fp64 arithmetic from the fp32 inputs in a fixed order, no atomics, nothing allocated, no memset
// (both calls can be captured).
//
// pdg_boundary_residuals: one workgroup per graph.  Thread t owns the graph's rows t, t + 1024, ... in that order,
// the block's sums are folded in a fixed order and the maximum with a rule that does not depend on the order
// (larger value, then lower index), so what a graph gets depends on its own rows, their position inside the graph
// and their incoming edges only: bitwise the same alone and inside any batch, and from call to call.
//
// pdg_boundary_residuals_bwd: node-parallel; a row depends on its own inputs, its neighbours' sigma and its
// graph's table row only, so the grid is free (BD_CHUNKS blocks per graph).
//
// Every per-node formula is compiled without contraction into fused multiply-adds: the forward and the backward
// evaluate a node's force from the same fp32 rows and get the same fp64 value as the host restatement's.
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "pdg_common.hpp"
#include "pdg_reduce.hpp"
#include "pdg_runtime.hpp"
#include "pdg_sym3.hpp"

using namespace pdg;

namespace {

constexpr int BD_T = 1024;      // threads per graph of boundary_residuals_kernel
constexpr int BD_COLS = 9;      // table columns
constexpr int BD_CT = 256;      // threads per block of boundary_residuals_bwd_kernel
constexpr int BD_CHUNKS = 16;   // its blocks per graph

// A node takes part in the traction sums iff its label is +-1 and its boundary length is > 0 (false for NaN).
__device__ __forceinline__ bool takes_part(int64_t label, float bl) { return (label == 1 || label == -1) && bl > 0.f; }

// Sums s[0..8]: L_int, L_ext, T2, F_int (2), F_ext (2), the jump sum and the edge count (both halved at the end);
// s[9] counts the participating nodes with a NaN traction.
__global__ __launch_bounds__(BD_T) void boundary_residuals_kernel(
    const int* __restrict__ ptr, const float* __restrict__ sig, const float* __restrict__ bvec,
    const float* __restrict__ blen, const int64_t* __restrict__ labels, const int* __restrict__ rowptr,
    const int* __restrict__ src, const int* __restrict__ perm, const float* __restrict__ eattr,
    double* __restrict__ table, int* __restrict__ argmax) {
#pragma clang fp contract(off)
  __shared__ double red[10 * 16];
  __shared__ double redv[16];
  __shared__ int redi[16];
  const int g = blockIdx.x;
  const int n0 = ptr[g], n1 = ptr[g + 1];
  if (n1 <= n0) {   // no rows: zeros (uniform over the block: no barrier is skipped)
    if (threadIdx.x < BD_COLS) table[(size_t)g * BD_COLS + threadIdx.x] = 0.0;
    if (threadIdx.x == 0) argmax[g] = -1;
    return;
  }
  double s[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) s[k] = 0.0;
  double best = -1.0;   // every |f| / blen is >= 0
  int besti = INT_MAX;
  for (int i = n0 + (int)threadIdx.x; i < n1; i += BD_T) {
    const Sym3 a = load_row(sig, i);
    const int64_t lab = labels[i];
    const float bl = blen[i];
    if (takes_part(lab, bl)) {
      double fx, fy;
      force(a, (double)bvec[(size_t)i * 2], (double)bvec[(size_t)i * 2 + 1], fx, fy);
      const double f2 = fx * fx + fy * fy;
      if (f2 != f2) s[9] += 1.0;
      if (lab == -1) {
        s[0] += (double)bl;
        s[2] += f2 / (double)bl;
        s[3] += fx;
        s[4] += fy;
        const double q = sqrt(f2) / (double)bl;
        if (q > best) {   // rows in increasing order: the first of equal values stays
          best = q;
          besti = i - n0;
        }
      } else {
        s[1] += (double)bl;
        s[5] += fx;
        s[6] += fy;
      }
    }
    if (rowptr) {
      for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) {   // the periodic connections of i (pdg_sym3.hpp)
        if (eattr[perm[k]] != 0.f) continue;
        const int j = src[k];
        if (j < n0 || j >= n1) continue;
        const Sym3 b = load_row(sig, j);
        const double dx = a.x - b.x, dy = a.y - b.y, dxy = a.xy - b.xy;
        s[7] += dx * dx + dy * dy + dxy * dxy;
        s[8] += 1.0;
      }
    }
  }
  block_sum_k<10>(s, red);
  block_best(best, besti, redv, redi);
  if (threadIdx.x == 0) {
    double* row = table + (size_t)g * BD_COLS;
#pragma unroll
    for (int k = 0; k < 7; ++k) row[k] = s[k];
    row[7] = 0.5 * s[7];
    row[8] = 0.5 * s[8];
    argmax[g] = (s[9] > 0.0 || besti == INT_MAX) ? -1 : besti;   // a plain maximum would hide a NaN traction
  }
}

__global__ __launch_bounds__(BD_CT) void boundary_residuals_bwd_kernel(
    const int* __restrict__ ptr, const float* __restrict__ sig, const float* __restrict__ bvec,
    const float* __restrict__ blen, const int64_t* __restrict__ labels, const int* __restrict__ rowptr,
    const int* __restrict__ src, const int* __restrict__ perm, const float* __restrict__ eattr,
    const double* __restrict__ table, const double* __restrict__ g_traction, const double* __restrict__ g_periodic,
    float* __restrict__ out) {
#pragma clang fp contract(off)
  const int g = blockIdx.x / BD_CHUNKS, chunk = blockIdx.x % BD_CHUNKS;
  const int n0 = ptr[g], n1 = ptr[g + 1];
  if (n1 <= n0) return;
  const double L = table[(size_t)g * BD_COLS], np = table[(size_t)g * BD_COLS + 8];
  const double gt = g_traction ? g_traction[g] : 0.0, gp = g_periodic ? g_periodic[g] : 0.0;
  // a zero weight switches its term off; a denominator that is not > 0 under a non-zero weight gives NaN
  const double ct = gt == 0.0 ? 0.0 : (L > 0.0 ? gt / L : (double)NAN);
  const double cp = gp == 0.0 ? 0.0 : (np > 0.0 ? gp / np : (double)NAN);
  for (int i = n0 + chunk * BD_CT + (int)threadIdx.x; i < n1; i += BD_CHUNKS * BD_CT) {
    const Sym3 a = load_row(sig, i);
    double o[3] = {0.0, 0.0, 0.0};   // a row that takes no part: exact zeros
    const float bl = blen[i];
    if (ct != 0.0 && labels[i] == -1 && bl > 0.f)
      traction_grad(a, (double)bvec[(size_t)i * 2], (double)bvec[(size_t)i * 2 + 1], bl, ct, o);
    if (cp != 0.0 && rowptr) {
      double d[3] = {0.0, 0.0, 0.0};
      int cnt = 0;
      for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) {   // the periodic connections of i (pdg_sym3.hpp)
        if (eattr[perm[k]] != 0.f) continue;
        const int j = src[k];
        if (j < n0 || j >= n1) continue;
        const Sym3 b = load_row(sig, j);
        d[0] += a.x - b.x;
        d[1] += a.y - b.y;
        d[2] += a.xy - b.xy;
        ++cnt;
      }
      if (cnt > 0)
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] += cp * (2.0 * d[k]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) out[(size_t)i * 3 + k] = (float)o[k];
  }
}

}  // namespace

extern "C" int pdg_boundary_residuals(int n_graphs, const int* ptr, const float* sigma, const float* bvec,
                                      const float* blen, const int64_t* labels, const int* rowptr_dst,
                                      const int* src, const int* perm, const float* edge_attr, double* table,
                                      int* argmax, void* stream) {
  PDG_CHECK_ARG(n_graphs > 0, "pdg_boundary_residuals: bad sizes (n_graphs > 0)");
  PDG_CHECK_ARG(ptr && sigma && bvec && blen && labels && table && argmax,
                "pdg_boundary_residuals: null argument (ptr, sigma, bvec, blen, labels, table and argmax are required)");
  PDG_CHECK_ARG(all_or_none({rowptr_dst, src, perm, edge_attr}),
                "pdg_boundary_residuals: partial edge arguments (rowptr_dst, src, perm and edge_attr are given "
                "together or all NULL)");
  hipLaunchKernelGGL(boundary_residuals_kernel, dim3(n_graphs), dim3(BD_T), 0, (hipStream_t)stream, ptr, sigma, bvec,
                     blen, labels, rowptr_dst, src, perm, edge_attr, table, argmax);
  PDG_CHECK_LAUNCH("pdg_boundary_residuals");
  return PDG_OK;
}

extern "C" int pdg_boundary_residuals_bwd(int n_graphs, const int* ptr, const float* sigma, const float* bvec,
                                          const float* blen, const int64_t* labels, const int* rowptr_dst,
                                          const int* src, const int* perm, const float* edge_attr,
                                          const double* table, const double* g_traction, const double* g_periodic,
                                          float* out, void* stream) {
  PDG_CHECK_ARG(n_graphs > 0 && n_graphs < (1 << 27), "pdg_boundary_residuals_bwd: bad sizes (0 < n_graphs < 2^27)");
  PDG_CHECK_ARG(ptr && sigma && bvec && blen && labels && table && out,
                "pdg_boundary_residuals_bwd: null argument (ptr, sigma, bvec, blen, labels, table and out are "
                "required)");
  PDG_CHECK_ARG(all_or_none({rowptr_dst, src, perm, edge_attr}),
                "pdg_boundary_residuals_bwd: partial edge arguments (rowptr_dst, src, perm and edge_attr are given "
                "together or all NULL)");
  hipLaunchKernelGGL(boundary_residuals_bwd_kernel, dim3(n_graphs * BD_CHUNKS), dim3(BD_CT), 0, (hipStream_t)stream,
                     ptr, sigma, bvec, blen, labels, rowptr_dst, src, perm, edge_attr, table, g_traction, g_periodic,
                     out);
  PDG_CHECK_LAUNCH("pdg_boundary_residuals_bwd");
  return PDG_OK;
}
