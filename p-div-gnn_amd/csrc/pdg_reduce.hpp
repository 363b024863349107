// Block reductions of the per-graph physics kernels (loss, metrics, criteria, homogenisation, boundary residuals,
// physics loss, equilibration, FEM): the one place that states the fold order behind "a graph scores bitwise the
// same alone and inside any batch".  A kernel that owns a graph per workgroup includes this; it does not restate it.
//
// Contract of every function here:
//   - all threads of the block call it (it holds two barriers); the result is valid in EVERY thread, so a decision
//     taken from it is uniform over the block;
//   - `red` is LDS of 16 K doubles (16 for the scalar form, 16 entries each of rv / ri): at most 16 waves, a
//     block of 1024 threads;
//   - a sum is folded in one fixed order: the xor butterfly of wave_sum inside a wave (offsets 32, 16, .. 1), then
//     the waves' sums added in wave order 0, 1, .. nw - 1, starting from +0, each of the K columns on its own;
//   - the maximum is folded by `better`, which is commutative and associative: no order to fix.
// pdg_common.hpp's block_sum2 is a different tool: two sums, valid in thread 0 only, LDS layout red[2 w + {0, 1}];
// the message-passing kernels' LayerNorm partials use it and it stays there.
#pragma once
#include "pdg_common.hpp"

namespace pdg {

__device__ __forceinline__ double block_sum(double x, double* red) {
  x = wave_sum(x);
  const int w = wave_id(), nw = blockDim.x >> 6;
  __syncthreads();
  if (lane_id() == 0) red[w] = x;
  __syncthreads();
  double s = 0;
  for (int i = 0; i < nw; ++i) s += red[i];
  return s;
}

// K sums at once (one LDS round instead of K), column-major: red[k * 16 + w].
template <int K>
__device__ __forceinline__ void block_sum_k(double (&x)[K], double* red) {
#pragma unroll
  for (int k = 0; k < K; ++k) x[k] = wave_sum(x[k]);
  const int w = wave_id(), nw = blockDim.x >> 6;
  __syncthreads();
  if (lane_id() == 0)
#pragma unroll
    for (int k = 0; k < K; ++k) red[k * 16 + w] = x[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double s = 0;
    for (int i = 0; i < nw; ++i) s += red[k * 16 + i];
    x[k] = s;
  }
}

// The same K sums, wave-major: red[w * K + k], one pass over the waves adding all K columns.  Each column is added
// in the same order as block_sum_k's, so the two give the same bits.  Only pdg_fem.hip uses it: with block_sum_k
// its persistent solver compiles to other, longer code (EXPERIMENTS.md section 11), which no timing has cleared.
template <int K>
__device__ __forceinline__ void block_sum_k_wave_major(double (&x)[K], double* red) {
#pragma unroll
  for (int k = 0; k < K; ++k) x[k] = wave_sum(x[k]);
  const int w = wave_id(), nw = blockDim.x >> 6;
  __syncthreads();
  if (lane_id() == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[w * K + k] = x[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) x[k] = 0;
  for (int i = 0; i < nw; ++i) {
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] += red[i * K + k];
  }
}

// (v, i) <- the better of (v, i) and (ov, oi): the larger value, the lower index on equal values.  Commutative
// and associative, so the block's result does not depend on the folding order.
__device__ __forceinline__ void better(double& v, int& i, double ov, int oi) {
  if (ov > v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

// The block's best (value, index).  `rv` / `ri` hold 16 entries each.
__device__ __forceinline__ void block_best(double& v, int& i, double* rv, int* ri) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(i, o);
    better(v, i, ov, oi);
  }
  const int w = wave_id(), nw = blockDim.x >> 6;
  __syncthreads();
  if (lane_id() == 0) {
    rv[w] = v;
    ri[w] = i;
  }
  __syncthreads();
  v = rv[0];
  i = ri[0];
  for (int k = 1; k < nw; ++k) better(v, i, rv[k], ri[k]);
}

// The graph of a node, for the node-parallel kernels: the last g in [0, B) with ptr[g] <= node.
__device__ __forceinline__ int graph_of(const int* __restrict__ ptr, int B, int node) {
  int lo = 0, hi = B;  // ptr[lo] <= node < ptr[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ptr[mid] <= node) lo = mid; else hi = mid;
  }
  return lo;
}

}  // namespace pdg
