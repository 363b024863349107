// "Group items by a major key, order a group by (minor key, item position)", shared by the CSR
// builders on the device (pdg_plan.hip, pdg_meshfields.hip).  Included once per translation
// unit; everything lives in an unnamed namespace, as pdg_scan.hpp's kernels do.
//
// A histogram of the major keys (the caller's count kernel, atomics), the exclusive scan of
// pdg_scan.hpp (it becomes the row pointer), an atomic fill of packed 64-bit slots
// (minor << 32 | position) into the rows in any order, then every row is sorted by itself and
// written out.  Slots of a row are distinct (positions are), so the sorted order is total:
// the result does not depend on the atomics' order.
//
// Rows are sorted by their length:
//   <= SHORT_MAX slots  one thread, insertion sort (mesh rows hold ~6-14 slots);
//   <= TILE_MAX slots   one workgroup, bitonic network in LDS;
//   longer              one workgroup, the same network on the row in global memory.
// The network is the all-ascending form (a "flip" step i <-> i ^ (k - 1), then "disperse"
// steps i <-> i ^ j), so slots past the row's end behave as +inf without being stored and a
// row of any length m costs O(m log^2 m / 256) per thread: a hub node never becomes an
// O(m^2) loop in one thread.
//
// A policy P supplies
//   bool item(long i, int& major, unsigned& minor)   item i's keys (false: the item is dropped;
//                                                    the count kernel must decide the same way),
//   void emit(long k, int row, u64 slot)             sorted slot k of `row` (position = low word).
#pragma once
#include <stdint.h>

#include "pdg_runtime.hpp"
#include "pdg_scan.hpp"

namespace {

typedef unsigned long long u64;

constexpr int PT = 256;            // threads per block
constexpr int SHORT_MAX = 32;      // longest row one thread sorts by insertion
constexpr int TILE_MAX = 2048;     // longest row sorted in LDS (16 KB of slots)

int grid_for(long work) {
  long g = (work + PT - 1) / PT;
  const long cap = (long)pdg::device_cus() * 8;
  return (int)(g < 1 ? 1 : g > cap ? cap : g);
}

// Counters and *status are cleared by a kernel (no memset node on a path that may be captured).
__global__ __launch_bounds__(PT) void clear_kernel(int* __restrict__ a, long na, int* __restrict__ b, long nb,
                                                   int* __restrict__ c, long nc, int* __restrict__ status) {
  const long stride = (long)gridDim.x * PT;
  const long t0 = (long)blockIdx.x * PT + threadIdx.x;
  for (long i = t0; i < na; i += stride) a[i] = 0;
  for (long i = t0; i < nb; i += stride) b[i] = 0;
  for (long i = t0; i < nc; i += stride) c[i] = 0;
  if (status && t0 == 0) *status = 0;
}

// Slot of item i in its row: rowptr[major] + (arrival order).  The count kernels took the same
// item() decisions, so a row never receives more slots than the scan reserved for it.
template <class P>
__global__ __launch_bounds__(PT) void fill_kernel(P p, long m, const int* __restrict__ rowptr, int* __restrict__ fill,
                                                  u64* __restrict__ slots) {
  for (long i = (long)blockIdx.x * PT + threadIdx.x; i < m; i += (long)gridDim.x * PT) {
    int major;
    unsigned minor;
    if (p.item(i, major, minor))
      slots[(long)rowptr[major] + atomicAdd(&fill[major], 1)] = ((u64)minor << 32) | (u64)(unsigned)i;
  }
}

__device__ __forceinline__ void cswap(u64* a, long i, long l) {
  const u64 x = a[i], y = a[l];
  if (x > y) {
    a[i] = y;
    a[l] = x;
  }
}

// Ascending sort of a[0..m) by the whole workgroup (a in LDS or in global memory).  Bitonic
// network over the next power of two with every comparator ascending; a comparator whose upper
// end is past m is skipped (that end is +inf and stays).
__device__ void block_sort(u64* a, long m) {
  long np2 = 1;
  while (np2 < m) np2 <<= 1;
  const long half = np2 >> 1;
  for (long k = 2; k <= np2; k <<= 1) {
    const long hk = k >> 1;
    for (long t = threadIdx.x; t < half; t += PT) {            // flip: i <-> i ^ (k - 1)
      const long lowb = t & (hk - 1);
      const long i = (t - lowb) * 2 + lowb;
      const long l = i ^ (k - 1);
      if (l < m) cswap(a, i, l);
    }
    __syncthreads();
    for (long j = k >> 2; j > 0; j >>= 1) {                    // disperse: i <-> i + j
      for (long t = threadIdx.x; t < half; t += PT) {
        const long lowb = t & (j - 1);
        const long i = (t - lowb) * 2 + lowb;
        const long l = i + j;
        if (l < m) cswap(a, i, l);
      }
      __syncthreads();
    }
  }
}

// Sort every row's slots and write the row out.  A block takes PT consecutive rows at a time:
// each thread sorts its own row when it is short, the long rows of the chunk are listed in LDS
// and sorted one after the other by the whole block.
template <class P>
__global__ __launch_bounds__(PT) void sort_emit_kernel(P p, int n, const int* __restrict__ rowptr,
                                                       u64* slots) {
  __shared__ u64 tile[TILE_MAX];
  __shared__ int longrow[PT];
  __shared__ int nlong;
  for (long base = (long)blockIdx.x * PT; base < n; base += (long)gridDim.x * PT) {
    if (threadIdx.x == 0) nlong = 0;
    __syncthreads();
    const long r = base + threadIdx.x;
    if (r < n) {
      const long b = rowptr[r];
      const int m = rowptr[r + 1] - rowptr[r];
      if (m > SHORT_MAX) {
        longrow[atomicAdd(&nlong, 1)] = (int)r;
      } else {
        u64* a = slots + b;
        for (int i = 1; i < m; ++i) {
          const u64 x = a[i];
          int j = i - 1;
          while (j >= 0 && a[j] > x) {
            a[j + 1] = a[j];
            --j;
          }
          a[j + 1] = x;
        }
        for (int i = 0; i < m; ++i) p.emit(b + i, (int)r, a[i]);
      }
    }
    __syncthreads();
    const int nl = nlong;
    for (int q = 0; q < nl; ++q) {
      const int row = longrow[q];
      const long b = rowptr[row];
      const long m = rowptr[row + 1] - rowptr[row];
      u64* a = slots + b;
      if (m <= TILE_MAX) {
        for (long i = threadIdx.x; i < m; i += PT) tile[i] = a[i];
        __syncthreads();
        block_sort(tile, m);
        for (long i = threadIdx.x; i < m; i += PT) p.emit(b + i, row, tile[i]);
      } else {
        block_sort(a, m);
        for (long i = threadIdx.x; i < m; i += PT) p.emit(b + i, row, a[i]);
      }
      __syncthreads();
    }
  }
}

// rowptr holds the histogram of the m items' major keys over n rows (n + 1 entries) and becomes
// the row pointer; fill: n zeroed counters; bsum: scan_bsum_len(n) ints; slots: m entries.
template <class P>
void group(const P& p, long m, int n, int* rowptr, int* fill, int* bsum, u64* slots, hipStream_t st) {
  scan(n, rowptr, bsum, st);
  if (m == 0) return;
  hipLaunchKernelGGL(fill_kernel<P>, dim3(grid_for(m)), dim3(PT), 0, st, p, m, rowptr, fill, slots);
  hipLaunchKernelGGL(sort_emit_kernel<P>, dim3(grid_for(n)), dim3(PT), 0, st, p, n, rowptr, slots);
}

}  // namespace
