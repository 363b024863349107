// Bounding box of a mesh's (x, y) on the device, shared by pdg_graph.hip (periodic sides) and
// pdg_meshfields.hip (external boundary).  Included once per translation unit.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

namespace {

constexpr int BBOX_T = 256;        // threads per block of bbox_kernel
constexpr int BBOX_BLOCKS = 256;   // most blocks (rows of `part`) a launch may use

// part[b] = block b's (min x, min y, max x, max y) over a grid-stride share of the points;
// block 0 also clears the 16 counters of `ctr`.
__global__ __launch_bounds__(BBOX_T) void bbox_kernel(int n, const float* __restrict__ p, int dim,
                                                      float* __restrict__ part, int* __restrict__ ctr) {
  __shared__ float red[4][BBOX_T];
  float mnx = FLT_MAX, mny = FLT_MAX, mxx = -FLT_MAX, mxy = -FLT_MAX;
  for (int i = blockIdx.x * BBOX_T + threadIdx.x; i < n; i += gridDim.x * BBOX_T) {
    const float x = p[(size_t)i * dim], y = p[(size_t)i * dim + 1];
    mnx = fminf(mnx, x);
    mny = fminf(mny, y);
    mxx = fmaxf(mxx, x);
    mxy = fmaxf(mxy, y);
  }
  red[0][threadIdx.x] = mnx;
  red[1][threadIdx.x] = mny;
  red[2][threadIdx.x] = mxx;
  red[3][threadIdx.x] = mxy;
  __syncthreads();
  for (int s = BBOX_T / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      red[0][threadIdx.x] = fminf(red[0][threadIdx.x], red[0][threadIdx.x + s]);
      red[1][threadIdx.x] = fminf(red[1][threadIdx.x], red[1][threadIdx.x + s]);
      red[2][threadIdx.x] = fmaxf(red[2][threadIdx.x], red[2][threadIdx.x + s]);
      red[3][threadIdx.x] = fmaxf(red[3][threadIdx.x], red[3][threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x < 4) part[4 * blockIdx.x + threadIdx.x] = red[threadIdx.x][0];
  if (blockIdx.x == 0 && threadIdx.x < 16) ctr[threadIdx.x] = 0;
}

// The whole box from the nparts block results, into bb[4] (LDS) = (min x, min y, max x, max y):
// called by every thread of a block, which may read bb after it returns.
__device__ __forceinline__ void bbox_load(const float* __restrict__ part, int nparts, float* bb) {
  if (threadIdx.x < 4) {
    float v = part[threadIdx.x];
    for (int b = 1; b < nparts; ++b)
      v = threadIdx.x < 2 ? fminf(v, part[4 * b + threadIdx.x]) : fmaxf(v, part[4 * b + threadIdx.x]);
    bb[threadIdx.x] = v;
  }
  __syncthreads();
}

inline int bbox_blocks(int n) {
  const long g = ((long)n + BBOX_T - 1) / BBOX_T;
  return (int)(g < BBOX_BLOCKS ? g : BBOX_BLOCKS);
}

}  // namespace
