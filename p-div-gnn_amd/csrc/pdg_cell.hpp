// A mesh cell (triangle NV = 3, quad NV = 4) from int64 faces and fp32 points: the range check of its vertex ids
// and its fp64 corners with det.  Shared by the mesh fields (pdg_meshfields.hip) and the point sampler
// (pdg_sample.hip), which must agree on which cells are degenerate.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pdg {

template <int NV>
__device__ __forceinline__ bool in_range(const int64_t* __restrict__ t, int n) {
  bool ok = true;
#pragma unroll
  for (int v = 0; v < NV; ++v) ok = ok && t[v] >= 0 && t[v] < n;
  return ok;
}

template <int NV>
struct Cell {
  double x[NV], y[NV], det;
};

// meshgen.p1_divergence_operator's / q1_divergence_operator's fp64 expressions, one rounding per operation.
// det = 2 * signed area: (xb - xa)(yc - ya) - (xc - xa)(yb - ya) of a triangle, the diagonals' cross product
// (xc - xa)(yd - yb) - (xd - xb)(yc - ya) of a quad.
template <int NV>
__device__ __forceinline__ Cell<NV> cell_of(const float* __restrict__ p, int dim, const int64_t* __restrict__ t) {
#pragma clang fp contract(off)
  Cell<NV> q;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    q.x[v] = p[(size_t)t[v] * dim];
    q.y[v] = p[(size_t)t[v] * dim + 1];
  }
  if constexpr (NV == 3) {
    const double m0 = (q.x[1] - q.x[0]) * (q.y[2] - q.y[0]);
    const double m1 = (q.x[2] - q.x[0]) * (q.y[1] - q.y[0]);
    q.det = m0 - m1;
  } else {
    const double m0 = (q.x[2] - q.x[0]) * (q.y[3] - q.y[1]);
    const double m1 = (q.x[3] - q.x[1]) * (q.y[2] - q.y[0]);
    q.det = m0 - m1;
  }
  return q;
}

}  // namespace pdg
