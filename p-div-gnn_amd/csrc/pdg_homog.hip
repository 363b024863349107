// Homogenisation of a nodal field: per-graph weighted integrals and averages (the reference's
// mean_stress = integrate_field(sigma) / bounding_box.volume and mean_stress_material = integrate_field(sigma) /
// integrate_field(1), scripts/generate_dataset.py:278-289, with the lumped nodal areas of pdg_nodal_areas as the
// quadrature weights) and the constant per-graph shift that makes a field's average equal a target.  As the
// stress criteria (pdg_criteria.hip): segmented by the batch's node offsets `ptr`, fp64 arithmetic from the fp32
// inputs in a fixed order, no float atomics, nothing allocated, no memset (both calls can be captured).
//
// pdg_graph_wmean: one workgroup per graph.  Thread t owns the graph's rows t, t + 1024, ... in that order and the
// block's sums are folded in a fixed order, so what a graph gets depends on its own rows and their position inside
// the graph only: bitwise the same alone and inside any batch, and from call to call.  A row takes part iff its
// weight is > 0 (the criteria's rule).
//
// pdg_mean_correct: element-wise; an output element depends on its own input and its graph's table row only, so
// the grid is free (HM_CHUNKS blocks per graph) and `out` may alias `sigma`.
#include <math.h>

#include "pdg_common.hpp"
#include "pdg_reduce.hpp"
#include "pdg_runtime.hpp"

using namespace pdg;

namespace {

constexpr int HM_T = 1024;     // threads per graph of graph_wmean_kernel
constexpr int HM_MAXC = 9;     // most columns of a field (the localisation tensor's 3 x 3)
constexpr int HM_CT = 256;     // threads per block of mean_correct_kernel
constexpr int HM_CHUNKS = 16;  // its blocks per graph

// table[g] = (W, S_0 .. S_{C-1}).  A graph without rows, or without a participating one, gets zeros.
template <int C>
__global__ __launch_bounds__(HM_T) void graph_wmean_kernel(const int* __restrict__ ptr, const float* __restrict__ rows,
                                                           const float* __restrict__ wts, double* __restrict__ table) {
#pragma clang fp contract(off)
  __shared__ double red[(C + 1) * 16];
  const int g = blockIdx.x;
  const int n0 = ptr[g], n1 = ptr[g + 1];
  double s[C + 1];
#pragma unroll
  for (int k = 0; k <= C; ++k) s[k] = 0.0;
  for (int i = n0 + (int)threadIdx.x; i < n1; i += HM_T) {
    const float w = wts ? wts[i] : 1.f;
    if (!(w > 0.f)) continue;   // 0, negative and NaN weights take no part
    s[0] += (double)w;
#pragma unroll
    for (int c = 0; c < C; ++c) s[1 + c] += (double)w * (double)rows[(size_t)i * C + c];
  }
  block_sum_k<C + 1>(s, red);
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k <= C; ++k) table[(size_t)g * (C + 1) + k] = s[k];
}

template <int C>
void launch_wmean(int n_graphs, const int* ptr, const float* rows, const float* wts, double* table, hipStream_t st) {
  hipLaunchKernelGGL(graph_wmean_kernel<C>, dim3(n_graphs), dim3(HM_T), 0, st, ptr, rows, wts, table);
}

// sigma and out may be the same array: no __restrict__ on either.
__global__ __launch_bounds__(HM_CT) void mean_correct_kernel(const int* __restrict__ ptr, const float* sigma,
                                                             const double* __restrict__ table,
                                                             const float* __restrict__ target,
                                                             const double* __restrict__ denom, float* out) {
#pragma clang fp contract(off)
  const int g = blockIdx.x / HM_CHUNKS, chunk = blockIdx.x % HM_CHUNKS;
  const long e0 = 3L * ptr[g], e1 = 3L * ptr[g + 1];
  if (e1 <= e0) return;
  const double* row = table + (size_t)g * 4;
  const double W = row[0];
  const double D = denom ? denom[g] : W;
  double shift[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)   // W is a sum of weights > 0: anything else (0, NaN) is a graph without an average
    shift[c] = W > 0.0 ? ((double)target[(size_t)g * 3 + c] * D - row[1 + c]) / W : (double)NAN;
  for (long e = e0 + (long)chunk * HM_CT + threadIdx.x; e < e1; e += (long)HM_CHUNKS * HM_CT) {
    const int c = (int)(e % 3);
    out[e] = (float)((double)sigma[e] + (c == 0 ? shift[0] : c == 1 ? shift[1] : shift[2]));
  }
}

}  // namespace

extern "C" int pdg_graph_wmean(int n_graphs, const int* ptr, const float* rows, int n_cols, const float* weights,
                               double* table, void* stream) {
  PDG_CHECK_ARG(n_graphs > 0 && n_cols >= 1 && n_cols <= HM_MAXC,
                "pdg_graph_wmean: bad sizes (n_graphs > 0, 1 <= n_cols <= 9)");
  PDG_CHECK_ARG(ptr && rows && table, "pdg_graph_wmean: null argument (ptr, rows and table are required)");
  hipStream_t st = (hipStream_t)stream;
  switch (n_cols) {
    case 1: launch_wmean<1>(n_graphs, ptr, rows, weights, table, st); break;
    case 2: launch_wmean<2>(n_graphs, ptr, rows, weights, table, st); break;
    case 3: launch_wmean<3>(n_graphs, ptr, rows, weights, table, st); break;
    case 4: launch_wmean<4>(n_graphs, ptr, rows, weights, table, st); break;
    case 5: launch_wmean<5>(n_graphs, ptr, rows, weights, table, st); break;
    case 6: launch_wmean<6>(n_graphs, ptr, rows, weights, table, st); break;
    case 7: launch_wmean<7>(n_graphs, ptr, rows, weights, table, st); break;
    case 8: launch_wmean<8>(n_graphs, ptr, rows, weights, table, st); break;
    default: launch_wmean<9>(n_graphs, ptr, rows, weights, table, st); break;
  }
  PDG_CHECK_LAUNCH("pdg_graph_wmean");
  return PDG_OK;
}

extern "C" int pdg_mean_correct(int n_graphs, const int* ptr, const float* sigma, const double* table,
                                const float* target, const double* denom, float* out, void* stream) {
  PDG_CHECK_ARG(n_graphs > 0 && n_graphs < (1 << 27), "pdg_mean_correct: bad sizes (0 < n_graphs < 2^27)");
  PDG_CHECK_ARG(ptr && sigma && table && target && out,
                "pdg_mean_correct: null argument (ptr, sigma, table, target and out are required)");
  hipLaunchKernelGGL(mean_correct_kernel, dim3(n_graphs * HM_CHUNKS), dim3(HM_CT), 0, (hipStream_t)stream, ptr, sigma,
                     table, target, denom, out);
  PDG_CHECK_LAUNCH("pdg_mean_correct");
  return PDG_OK;
}
