// Exclusive prefix sum of an int32 array on the device, shared by the CSR builders
// (pdg_graph.hip, pdg_plan.hip, pdg_meshfields.hip).  Included once per translation unit; everything lives in an
// unnamed namespace, so each unit carries its own copy of the three kernels.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int SCAN_BLOCK = 1024;         // elements per scan block (256 threads x 4)

// Exclusive prefix sum of a[0..n) into a (a[n] = total), three passes (block sums, their scan
// in one block, add-back).  Integer, so the result is exact.
__global__ __launch_bounds__(256) void scan_local_kernel(int n, int* __restrict__ a, int* __restrict__ bsum) {
  __shared__ int s[SCAN_BLOCK];
  const int base = blockIdx.x * SCAN_BLOCK;
  for (int i = threadIdx.x; i < SCAN_BLOCK; i += 256) s[i] = base + i < n ? a[base + i] : 0;
  __syncthreads();
  // Hillis-Steele over 1024 entries, 4 per thread
  for (int off = 1; off < SCAN_BLOCK; off <<= 1) {
    int t[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = threadIdx.x + 256 * u;
      t[u] = i >= off ? s[i - off] : 0;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) s[threadIdx.x + 256 * u] += t[u];
    __syncthreads();
  }
  for (int i = threadIdx.x; i < SCAN_BLOCK; i += 256)
    if (base + i < n) a[base + i] = i ? s[i - 1] : 0;   // exclusive within the block
  if (threadIdx.x == 0) bsum[blockIdx.x] = s[SCAN_BLOCK - 1];
}

__global__ __launch_bounds__(1024) void scan_blocks_kernel(int nb, int* __restrict__ bsum) {
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int b = 0; b < nb; ++b) {
      const int v = bsum[b];
      bsum[b] = acc;
      acc += v;
    }
    bsum[nb] = acc;
  }
}

__global__ __launch_bounds__(256) void scan_add_kernel(int n, int* __restrict__ a, const int* __restrict__ bsum, int nb) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) a[i] += bsum[i / SCAN_BLOCK];
  if (i == 0) a[n] = bsum[nb];
}

// Entries of the block-sum array a scan of n elements needs.
inline size_t scan_bsum_len(int n) { return (size_t)((n + SCAN_BLOCK - 1) / SCAN_BLOCK) + 2; }

// a: n + 1 entries (counts in a[0..n), a[n] receives the total); bsum: scan_bsum_len(n) entries.
inline void scan(int n, int* a, int* bsum, hipStream_t st) {
  const int nb = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
  hipLaunchKernelGGL(scan_local_kernel, dim3(nb > 0 ? nb : 1), dim3(256), 0, st, n, a, bsum);
  hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(1024), 0, st, nb, bsum);
  hipLaunchKernelGGL(scan_add_kernel, dim3((n + 256) / 256), dim3(256), 0, st, n, a, bsum, nb);
}

}  // namespace
