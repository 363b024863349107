// Fused physics loss of a training step: the hole traction, the periodic jump and the mean-consistency defect of
// the trainer's STANDARDISED prediction y, as penalties with a gradient that accumulates into the step's g_y.
// The diagnostics (pdg_boundary.hip, pdg_homog.hip) take the unstandardised field and write NaN for a graph
// that lacks a term; here every term is evaluated on z = y + mean / std (= sigma / std, formed in fp64 from the
// device pair affine = (std, mean), so nothing is read on the host and dz / dy = 1), and a term a graph lacks is
// absent: loss exactly 0, gradient rows exactly 0.  A NaN in a participating input still gives a NaN loss.
// As the diagnostics: segmented by the batch's node offsets `ptr`, fp64 arithmetic from the fp32 inputs in a
// fixed order, no atomics, nothing allocated, no memset (every call can be captured).
//
// pdg_phys_loss_fwd: one workgroup per graph.  Thread t owns the graph's rows t, t + 1024, ... in that order and
// the block's sums are folded in a fixed order, so what a graph gets depends on its own rows, their position
// inside the graph and their incoming edges only: bitwise the same alone and inside any batch, and from call to
// call.  The participation rules are the diagnostics': a traction node has label -1 and blen > 0, a periodic
// connection is an incoming edge of length exactly 0 whose source lies in the node's graph, a row enters the
// average iff its area is > 0.
//
// pdg_phys_loss_bwd: node-parallel; a row depends on its own inputs, its neighbours' y and its graph's table row.
//
// The per-node formulas are pdg_boundary.hip's (pdg_sym3.hpp) and the block sum is every per-graph kernel's
// (pdg_reduce.hpp).  Every per-node formula is compiled without contraction into fused multiply-adds, so the
// forward, the backward and the host restatement form the same fp64 values.
#include <math.h>
#include <stdint.h>

#include "pdg_common.hpp"
#include "pdg_reduce.hpp"
#include "pdg_runtime.hpp"
#include "pdg_sym3.hpp"

using namespace pdg;

namespace {

constexpr int PL_T = 1024;    // threads per graph of phys_loss_fwd_kernel
constexpr int PL_COLS = 12;   // table columns
constexpr int PL_CT = 256;    // threads per block of phys_loss_bwd_kernel

// table columns
enum { C_L = 0, C_T2, C_P2, C_NP, C_W, C_SXX, C_SYY, C_SXY, C_D, C_LT, C_LP, C_LM };

// z = y + mean / std, one fp64 addition per component
__device__ __forceinline__ Sym3 load_z(const float* __restrict__ y, int i, double off) {
#pragma clang fp contract(off)
  return Sym3{(double)y[(size_t)i * 3] + off, (double)y[(size_t)i * 3 + 1] + off, (double)y[(size_t)i * 3 + 2] + off};
}

// Sums s[0..7]: L_int, T2, the jump sum and the edge count (both halved at the end), W, S_xx, S_yy, S_xy.
__global__ __launch_bounds__(PL_T) void phys_loss_fwd_kernel(
    const int* __restrict__ ptr, const float* __restrict__ y, const float* __restrict__ affine,
    const float* __restrict__ bvec, const float* __restrict__ blen, const int64_t* __restrict__ labels,
    const int* __restrict__ rowptr, const int* __restrict__ src, const int* __restrict__ perm,
    const float* __restrict__ eattr, const float* __restrict__ area, const double* __restrict__ denom,
    const float* __restrict__ target, double* __restrict__ table, float* __restrict__ loss) {
#pragma clang fp contract(off)
  __shared__ double red[8 * 16];
  const int g = blockIdx.x;
  const int n0 = ptr[g], n1 = ptr[g + 1];
  const double sd = (double)affine[0];
  const double off = (double)affine[1] / sd;
  double s[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = 0.0;
  for (int i = n0 + (int)threadIdx.x; i < n1; i += PL_T) {   // a graph without rows: every sum stays 0
    const Sym3 a = load_z(y, i, off);
    if (bvec) {
      const float bl = blen[i];
      if (labels[i] == -1 && bl > 0.f) {   // false for a NaN length
        double fx, fy;
        force(a, (double)bvec[(size_t)i * 2], (double)bvec[(size_t)i * 2 + 1], fx, fy);
        s[0] += (double)bl;
        s[1] += (fx * fx + fy * fy) / (double)bl;
      }
    }
    if (rowptr) {
      for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) {   // the periodic connections of i (pdg_sym3.hpp)
        if (eattr[perm[k]] != 0.f) continue;
        const int j = src[k];
        if (j < n0 || j >= n1) continue;
        const Sym3 b = load_z(y, j, off);
        const double dx = a.x - b.x, dy = a.y - b.y, dxy = a.xy - b.xy;
        s[2] += dx * dx + dy * dy + dxy * dxy;
        s[3] += 1.0;
      }
    }
    if (area) {
      const float w = area[i];
      if (w > 0.f) {   // 0, negative and NaN areas take no part
        s[4] += (double)w;
        s[5] += (double)w * a.x;
        s[6] += (double)w * a.y;
        s[7] += (double)w * a.xy;
      }
    }
  }
  block_sum_k<8>(s, red);
  if (threadIdx.x == 0) {
    double* row = table + (size_t)g * PL_COLS;
    const double L = s[0], T2 = s[1], P2 = 0.5 * s[2], np = 0.5 * s[3], W = s[4];
    const double D = area ? (denom ? denom[g] : W) : 0.0;
    // the training rule: a term whose denominator is not > 0 is absent (exactly 0), never NaN
    const double lt = L > 0.0 ? T2 / L : 0.0;
    const double lp = np > 0.0 ? P2 / np : 0.0;
    double lm = 0.0;
    if (area && D > 0.0 && W > 0.0)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double d = s[5 + c] / D - (double)target[(size_t)g * 3 + c] / sd;
        lm += d * d;
      }
    row[C_L] = L;
    row[C_T2] = T2;
    row[C_P2] = P2;
    row[C_NP] = np;
    row[C_W] = W;
    row[C_SXX] = s[5];
    row[C_SYY] = s[6];
    row[C_SXY] = s[7];
    row[C_D] = D;
    row[C_LT] = lt;
    row[C_LP] = lp;
    row[C_LM] = lm;
    loss[(size_t)g * 3] = (float)lt;
    loss[(size_t)g * 3 + 1] = (float)lp;
    loss[(size_t)g * 3 + 2] = (float)lm;
  }
}

__global__ __launch_bounds__(PL_CT) void phys_loss_bwd_kernel(
    int B, const int* __restrict__ ptr, int N, const float* __restrict__ y, const float* __restrict__ affine,
    const float* __restrict__ bvec, const float* __restrict__ blen, const int64_t* __restrict__ labels,
    const int* __restrict__ rowptr, const int* __restrict__ src, const int* __restrict__ perm,
    const float* __restrict__ eattr, const float* __restrict__ area, const float* __restrict__ target,
    const double* __restrict__ table, const float* __restrict__ scale, int accumulate, float* __restrict__ gy) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * PL_CT + (int)threadIdx.x;
  if (i >= N) return;
  const int g = graph_of(ptr, B, i);
  const int n0 = ptr[g], n1 = ptr[g + 1];
  const double* row = table + (size_t)g * PL_COLS;
  const double sd = (double)affine[0];
  const double off = (double)affine[1] / sd;
  const float wt = scale[0], wp = scale[1], wm = scale[2];
  // a weight of exactly 0 switches its term off whatever the table holds; so does a denominator that is not > 0
  const double L = row[C_L], np = row[C_NP], W = row[C_W], D = row[C_D];
  const bool on_t = wt != 0.f && bvec && L > 0.0;
  const bool on_p = wp != 0.f && rowptr && np > 0.0;
  const bool on_m = wm != 0.f && area && D > 0.0 && W > 0.0;
  double o[3] = {0.0, 0.0, 0.0};   // a row that takes no part: exact zeros
  if (on_t || on_p || on_m) {
    const Sym3 a = load_z(y, i, off);
    if (on_t) {
      const float bl = blen[i];
      if (labels[i] == -1 && bl > 0.f)
        traction_grad(a, (double)bvec[(size_t)i * 2], (double)bvec[(size_t)i * 2 + 1], bl, (double)wt / L, o);
    }
    if (on_p) {
      const double cp = (double)wp / np;
      double d[3] = {0.0, 0.0, 0.0};
      int cnt = 0;
      for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) {   // the periodic connections of i (pdg_sym3.hpp)
        if (eattr[perm[k]] != 0.f) continue;
        const int j = src[k];
        if (j < n0 || j >= n1) continue;
        const Sym3 b = load_z(y, j, off);
        d[0] += a.x - b.x;
        d[1] += a.y - b.y;
        d[2] += a.xy - b.xy;
        ++cnt;
      }
      if (cnt > 0)
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] += cp * (2.0 * d[k]);
    }
    if (on_m) {
      const float w = area[i];
      if (w > 0.f) {
        const double c = (double)wm * (2.0 * (double)w / D);
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] += c * (row[C_SXX + k] / D - (double)target[(size_t)g * 3 + k] / sd);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const size_t e = (size_t)i * 3 + k;
    gy[e] = accumulate ? (float)((double)gy[e] + o[k]) : (float)o[k];   // one rounding
  }
}

// pdg_loss.hip's loss_reduce_kernel with the three physics sums.
__global__ void loss_reduce_phys_kernel(int B, const float* __restrict__ ln, const float* __restrict__ ld,
                                        const float* __restrict__ lp, float sn, float sdv,
                                        const float* __restrict__ sp, const float* __restrict__ nz,
                                        float* __restrict__ out) {
  __shared__ double red[5 * 16];
  double v[5] = {0, 0, 0, 0, 0};
  for (int g = threadIdx.x; g < B; g += blockDim.x) {
    v[0] += (double)ln[g];
    if (ld) v[1] += (double)ld[g];
    if (lp)
#pragma unroll
      for (int k = 0; k < 3; ++k) v[2 + k] += (double)lp[(size_t)g * 3 + k];
  }
  block_sum_k<5>(v, red);
  if (threadIdx.x == 0) {
#pragma clang fp contract(off)
    const float fn = (float)v[0] * sn;
    const float fd = ld ? (float)v[1] * sdv : 0.f;
    // pdg_loss_reduce's out[1] + out[2] as its compiled code forms it: the NMSE product is contracted into the
    // addition (one rounding).  Written out here, so that with all three weights 0 the total is bitwise
    // pdg_loss_reduce's (tests/test_gpu_physloss_trainer.py holds the two together).
    float total = __fmaf_rn((float)v[0], sn, fd);
    out[0] = nz ? *nz : 1.f;
    out[1] = fn;
    out[2] = fd;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float w = (lp && sp) ? sp[k] : 0.f;
      const float f = w != 0.f ? (float)v[2 + k] * w : 0.f;   // a zero weight: an exact 0, a NaN sum included
      out[4 + k] = f;
      total += f;
    }
    out[3] = total;
  }
}

}  // namespace

#define PL_CHECK_GROUPS(name)                                                                                       \
  PDG_CHECK_ARG(all_or_none({bvec, blen, labels}),                                                                  \
                name ": partial boundary arguments (bvec, blen and labels are given together or all NULL)");        \
  PDG_CHECK_ARG(all_or_none({rowptr_dst, src, perm, edge_attr}),                                                    \
                name ": partial edge arguments (rowptr_dst, src, perm and edge_attr are given together or all "     \
                     "NULL)");                                                                                      \
  PDG_CHECK_ARG((area != nullptr) == (target != nullptr) && (area != nullptr || denom == nullptr),                  \
                name ": partial mean arguments (area and target are given together or all NULL, denom only with "   \
                     "them)")

extern "C" int pdg_phys_loss_fwd(int n_graphs, const int* ptr, const float* y, const float* affine, const float* bvec,
                                 const float* blen, const int64_t* labels, const int* rowptr_dst, const int* src,
                                 const int* perm, const float* edge_attr, const float* area, const double* denom,
                                 const float* target, double* table, float* loss, void* stream) {
  PDG_CHECK_ARG(n_graphs > 0, "pdg_phys_loss_fwd: bad sizes (n_graphs > 0)");
  PDG_CHECK_ARG(ptr && y && affine && table && loss,
                "pdg_phys_loss_fwd: null argument (ptr, y, affine, table and loss are required)");
  PL_CHECK_GROUPS("pdg_phys_loss_fwd");
  hipLaunchKernelGGL(phys_loss_fwd_kernel, dim3(n_graphs), dim3(PL_T), 0, (hipStream_t)stream, ptr, y, affine, bvec,
                     blen, labels, rowptr_dst, src, perm, edge_attr, area, denom, target, table, loss);
  PDG_CHECK_LAUNCH("pdg_phys_loss_fwd");
  return PDG_OK;
}

extern "C" int pdg_phys_loss_bwd(int n_graphs, const int* ptr, int n_nodes, const float* y, const float* affine,
                                 const float* bvec, const float* blen, const int64_t* labels, const int* rowptr_dst,
                                 const int* src, const int* perm, const float* edge_attr, const float* area,
                                 const double* denom, const float* target, const double* table, const float* scale,
                                 int accumulate, float* g_y, void* stream) {
  PDG_CHECK_ARG(n_graphs > 0 && n_nodes > 0, "pdg_phys_loss_bwd: bad sizes (n_graphs > 0, n_nodes > 0)");
  PDG_CHECK_ARG(ptr && y && affine && table && scale && g_y,
                "pdg_phys_loss_bwd: null argument (ptr, y, affine, table, scale and g_y are required)");
  PL_CHECK_GROUPS("pdg_phys_loss_bwd");
  hipLaunchKernelGGL(phys_loss_bwd_kernel, dim3((n_nodes + PL_CT - 1) / PL_CT), dim3(PL_CT), 0, (hipStream_t)stream,
                     n_graphs, ptr, n_nodes, y, affine, bvec, blen, labels, rowptr_dst, src, perm, edge_attr, area,
                     target, table, scale, accumulate, g_y);
  PDG_CHECK_LAUNCH("pdg_phys_loss_bwd");
  return PDG_OK;
}

extern "C" int pdg_loss_reduce_phys(int n_graphs, const float* loss_nmse, const float* loss_div,
                                    const float* loss_phys, float scale_nmse, float scale_div,
                                    const float* scale_phys, const float* zero_flag, float* out, void* stream) {
  PDG_CHECK_ARG(n_graphs > 0, "pdg_loss_reduce_phys: bad sizes (n_graphs > 0)");
  PDG_CHECK_ARG(loss_nmse && out && (loss_phys != nullptr) == (scale_phys != nullptr),
                "pdg_loss_reduce_phys: null argument (loss_nmse and out are required; loss_phys and scale_phys are "
                "given together or both NULL)");
  hipLaunchKernelGGL(loss_reduce_phys_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, n_graphs, loss_nmse,
                     loss_div, loss_phys, scale_nmse, scale_div, scale_phys, zero_flag, out);
  PDG_CHECK_LAUNCH("pdg_loss_reduce_phys");
  return PDG_OK;
}
