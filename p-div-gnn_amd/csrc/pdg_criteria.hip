// Failure criteria of a plane-stress field (von Mises as the reference's von_mises_stress,
// gnn_local_stress/datasets.py:82; Tresca; Rankine), their per-graph aggregates (max and its location, weighted
// mean, p-norm, Kreisselmeier-Steinhauser) and the aggregates' gradients with respect to the field.  As the
// evaluation metrics (pdg_metrics.hip): segmented by the batch's node offsets `ptr`, one workgroup per graph,
// fp64 arithmetic from the fp32 inputs in a fixed order, no float atomics, nothing allocated, no memset (both
// calls can be captured).
//
// Thread t of a graph's block owns the graph's rows t, t + 1024, ... in that order; the block's sums are folded
// in a fixed order and the maximum is folded with a rule that does not depend on the order (larger value, then
// lower index), so what a graph gets depends on its own rows and their position inside the graph only: it scores
// bitwise the same alone and inside any batch.
//
// Every per-node formula is compiled without contraction into fused multiply-adds: the forward's two passes and
// the backward evaluate a node's criterion from the same fp32 row and must get the same fp64 value (the
// backward's one-hot, p-norm and KS weights are relative to the forward's maximum).
#include <limits.h>
#include <math.h>

#include <cmath>

#include "pdg_common.hpp"
#include "pdg_reduce.hpp"
#include "pdg_runtime.hpp"

using namespace pdg;

namespace {

constexpr int CR_T = 1024;   // threads per graph
// The first CR_C rows of a thread (CR_C * 1024 = 4,096 nodes per graph) keep their criterion value and weight in
// registers between the forward's two passes; rows beyond are read and evaluated again.  The same values and
// sums in the same order either way.
constexpr int CR_C = 4;

struct Crit {
  double vm, s1, s2, d, r, c;   // von Mises, principal stresses, (sx - sy) / 2, in-plane maximum shear, criterion
};

// crit: 0 von Mises, 1 Tresca (out-of-plane principal stress 0; branch order 2r, |s1|, |s2|, the first wins on
// an exact tie), 2 Rankine.  A NaN row gives a NaN criterion under every id.
__device__ __forceinline__ Crit crit_eval(double x, double y, double xy, int crit) {
#pragma clang fp contract(off)
  Crit q;
  q.vm = sqrt(0.5 * ((x - y) * (x - y) + x * x + y * y + 6.0 * (xy * xy)));
  const double m = (x + y) / 2.0;
  q.d = (x - y) / 2.0;
  q.r = sqrt(q.d * q.d + xy * xy);
  q.s1 = m + q.r;
  q.s2 = m - q.r;
  if (crit == 0) {
    q.c = q.vm;
  } else if (crit == 1) {
    const double t2 = 2.0 * q.r, a1 = fabs(q.s1), a2 = fabs(q.s2);
    q.c = (t2 >= a1 && t2 >= a2) ? t2 : (a1 >= a2 ? a1 : a2);
  } else {
    q.c = !(q.s1 <= 0.0) ? q.s1 : 0.0;   // max(s1, 0) that keeps a NaN
  }
  return q;
}

__device__ __forceinline__ double sign0(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); }

// d criterion / d (sx, sy, sxy): the gradient of the branch crit_eval chose; 0 at von Mises' and r's kinks.
__device__ __forceinline__ void crit_grad(double x, double y, double xy, int crit, const Crit& q, double (&g)[3]) {
#pragma clang fp contract(off)
  if (crit == 0) {
    if (q.vm == 0.0) {
      g[0] = g[1] = g[2] = 0.0;
    } else {
      const double h = 2.0 * q.vm;
      g[0] = (2.0 * x - y) / h;
      g[1] = (2.0 * y - x) / h;
      g[2] = (6.0 * xy) / h;
    }
    return;
  }
  double dr[3] = {0.0, 0.0, 0.0};
  if (q.r != 0.0) {
    dr[0] = q.d / (2.0 * q.r);
    dr[1] = -dr[0];
    dr[2] = xy / q.r;
  }
  double sg, pm;   // g = sg * ((1/2, 1/2, 0) * |pm| + pm * dr), or 2 dr on Tresca's first branch
  if (crit == 2) {
    sg = q.s1 > 0.0 ? 1.0 : 0.0;
    pm = 1.0;
  } else {
    const double t2 = 2.0 * q.r, a1 = fabs(q.s1), a2 = fabs(q.s2);
    if (t2 >= a1 && t2 >= a2) {
      g[0] = 2.0 * dr[0];
      g[1] = 2.0 * dr[1];
      g[2] = 2.0 * dr[2];
      return;
    }
    if (a1 >= a2) {
      sg = sign0(q.s1);
      pm = 1.0;
    } else {
      sg = sign0(q.s2);
      pm = -1.0;
    }
  }
  g[0] = sg * (0.5 + pm * dr[0]);
  g[1] = sg * (0.5 + pm * dr[1]);
  g[2] = sg * (pm * dr[2]);
}

__global__ __launch_bounds__(CR_T) void stress_criteria_kernel(const int* __restrict__ ptr,
                                                              const float* __restrict__ sig,
                                                              const float* __restrict__ wts, int crit, double p,
                                                              double rho, double* __restrict__ table,
                                                              int* __restrict__ argmax, float* __restrict__ fields) {
  __shared__ double red[3 * 16];
  __shared__ double redv[16];
  __shared__ int redi[16];
  const int g = blockIdx.x;
  const int n0 = ptr[g], n1 = ptr[g + 1];
  if (n1 <= n0) {   // no nodes: NaN row, no field row touched (uniform over the block: no barrier is skipped)
    if (threadIdx.x < 4) table[(size_t)g * 4 + threadIdx.x] = NAN;
    if (threadIdx.x == 0) argmax[g] = -1;
    return;
  }
  const int first = n0 + (int)threadIdx.x;
  const int rest = first + CR_C * CR_T;

  // pass 1: the fields; W = sum w, sum w c, the count of NaN criteria; the first maximum.  Participation: w > 0
  // (false for a NaN weight).  `wp` is the weight of a participating row, 0 otherwise.
  double s[3] = {0, 0, 0};
  double best = -1.0;   // every criterion is >= 0
  int besti = INT_MAX;
  auto visit = [&](int i, double& c, float& wp) {
    const double x = (double)sig[(size_t)i * 3], y = (double)sig[(size_t)i * 3 + 1], xy = (double)sig[(size_t)i * 3 + 2];
    const Crit q = crit_eval(x, y, xy, crit);
    if (fields) {
      float* f = fields + (size_t)i * 6;
      f[0] = (float)q.vm;
      f[1] = (float)q.s1;
      f[2] = (float)q.s2;
      f[3] = (float)q.r;
      f[4] = (float)(0.5 * atan2(xy, q.d));
      f[5] = (float)q.c;
    }
    const float w = wts ? wts[i] : 1.f;
    c = q.c;
    wp = w > 0.f ? w : 0.f;
    if (wp > 0.f) {
      if (c != c) {
        s[2] += 1.0;
      } else {
        s[0] += (double)wp;
        s[1] += (double)wp * c;
        if (c > best) {   // rows in increasing order: the first of equal values stays
          best = c;
          besti = i - n0;
        }
      }
    }
  };
  double cc[CR_C];
  float cw[CR_C];
#pragma unroll
  for (int k = 0; k < CR_C; ++k) {
    cc[k] = 0.0;
    cw[k] = 0.f;
    if (first + k * CR_T < n1) visit(first + k * CR_T, cc[k], cw[k]);
  }
  for (int i = rest; i < n1; i += CR_T) {
    double c;
    float wp;
    visit(i, c, wp);
  }
  block_sum_k<3>(s, red);
  block_best(best, besti, redv, redi);
  if (s[2] > 0.0 || besti == INT_MAX) {   // a NaN criterion, or no participating node (uniform: no barrier skipped)
    if (threadIdx.x < 4) table[(size_t)g * 4 + threadIdx.x] = NAN;
    if (threadIdx.x == 0) argmax[g] = -1;
    return;
  }

  // pass 2, relative to the maximum M: sum w (c / M)^p and sum w exp(rho (c - M)), every term <= w
  const double M = best;
  double t[2] = {0, 0};
  auto acc = [&](double c, float wp) {
    if (wp > 0.f) {
      if (M > 0.0) t[0] += (double)wp * pow(c / M, p);
      t[1] += (double)wp * exp(rho * (c - M));
    }
  };
#pragma unroll
  for (int k = 0; k < CR_C; ++k) acc(cc[k], cw[k]);
  for (int i = rest; i < n1; i += CR_T) {
    const float w = wts ? wts[i] : 1.f;
    if (!(w > 0.f)) continue;
    const Crit q = crit_eval((double)sig[(size_t)i * 3], (double)sig[(size_t)i * 3 + 1], (double)sig[(size_t)i * 3 + 2], crit);
    acc(q.c, w);
  }
  block_sum_k<2>(t, red);
  if (threadIdx.x == 0) {
    double* row = table + (size_t)g * 4;
    const double W = s[0];
    row[0] = M;
    row[1] = s[1] / W;
    row[2] = M > 0.0 ? M * pow(t[0] / W, 1.0 / p) : 0.0;
    row[3] = M + log(t[1] / W) / rho;
    argmax[g] = besti;
  }
}

// The KS weights need sum w exp(rho (c - M)) again: one block sum here, not a fifth table column (the table
// stays the four documented values, and the mean and the p-norm need W, which takes the same block sum).
__global__ __launch_bounds__(CR_T) void stress_criteria_bwd_kernel(const int* __restrict__ ptr,
                                                                  const float* __restrict__ sig,
                                                                  const float* __restrict__ wts, int crit, int agg,
                                                                  double p, double rho,
                                                                  const double* __restrict__ table,
                                                                  const int* __restrict__ argmax,
                                                                  const float* __restrict__ g_value,
                                                                  float* __restrict__ g_sigma) {
  __shared__ double red[2 * 16];
  const int g = blockIdx.x;
  const int n0 = ptr[g], n1 = ptr[g + 1];
  if (n1 <= n0) return;
  const int am = argmax[g];   // < 0: a NaN graph, or one without a participating node
  const double M = table[(size_t)g * 4], J = table[(size_t)g * 4 + agg];
  const double gv = g_value ? (double)g_value[g] : 1.0;
  double s[2] = {0, 0};   // W, sum w exp(rho (c - M))
  if (am >= 0 && agg != 0) {   // uniform over the block
    for (int i = n0 + (int)threadIdx.x; i < n1; i += CR_T) {
      const float w = wts ? wts[i] : 1.f;
      if (!(w > 0.f)) continue;
      s[0] += (double)w;
      if (agg == 3) {
        const Crit q = crit_eval((double)sig[(size_t)i * 3], (double)sig[(size_t)i * 3 + 1], (double)sig[(size_t)i * 3 + 2], crit);
        s[1] += (double)w * exp(rho * (q.c - M));
      }
    }
    block_sum_k<2>(s, red);
  }
  for (int i = n0 + (int)threadIdx.x; i < n1; i += CR_T) {
    const float w = wts ? wts[i] : 1.f;
    float o[3] = {0.f, 0.f, 0.f};   // a row that takes no part: exact zeros
    if (w > 0.f) {
      if (am < 0) {
        o[0] = o[1] = o[2] = NAN;
      } else if (agg != 0 || i - n0 == am) {
        const double x = (double)sig[(size_t)i * 3], y = (double)sig[(size_t)i * 3 + 1], xy = (double)sig[(size_t)i * 3 + 2];
        const Crit q = crit_eval(x, y, xy, crit);
        double dc[3];
        crit_grad(x, y, xy, crit, q, dc);
        double wn;   // d J / d c of this node
        if (agg == 0) wn = 1.0;   // a subgradient: all of it at the first maximum
        else if (agg == 1) wn = (double)w / s[0];
        else if (agg == 2) wn = J == 0.0 ? 0.0 : ((double)w / s[0]) * pow(q.c / J, p - 1.0);
        else wn = ((double)w * exp(rho * (q.c - M))) / s[1];
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = (float)(gv * (wn * dc[k]));
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) g_sigma[(size_t)i * 3 + k] = o[k];
  }
}

}  // namespace

extern "C" int pdg_stress_criteria(int n_graphs, const int* ptr, const float* sigma, const float* weights,
                                   int criterion, double p, double rho, double* table, int* argmax, float* fields,
                                   void* stream) {
  PDG_CHECK_ARG(n_graphs > 0, "pdg_stress_criteria: n_graphs must be > 0");
  PDG_CHECK_ARG(ptr && sigma && table && argmax,
                "pdg_stress_criteria: null argument (ptr, sigma, table and argmax are required)");
  PDG_CHECK_ARG(criterion >= 0 && criterion <= 2, "pdg_stress_criteria: criterion must be 0, 1 or 2");
  PDG_CHECK_ARG(std::isfinite(p) && p >= 1.0, "pdg_stress_criteria: p must be finite and >= 1");
  PDG_CHECK_ARG(std::isfinite(rho) && rho > 0.0, "pdg_stress_criteria: rho must be finite and > 0");
  hipLaunchKernelGGL(stress_criteria_kernel, dim3(n_graphs), dim3(CR_T), 0, (hipStream_t)stream, ptr, sigma, weights,
                     criterion, p, rho, table, argmax, fields);
  PDG_CHECK_LAUNCH("pdg_stress_criteria");
  return PDG_OK;
}

extern "C" int pdg_stress_criteria_bwd(int n_graphs, const int* ptr, const float* sigma, const float* weights,
                                       int criterion, int aggregate, double p, double rho, const double* table,
                                       const int* argmax, const float* g_value, float* g_sigma, void* stream) {
  PDG_CHECK_ARG(n_graphs > 0, "pdg_stress_criteria_bwd: n_graphs must be > 0");
  PDG_CHECK_ARG(ptr && sigma && table && argmax && g_sigma,
                "pdg_stress_criteria_bwd: null argument (ptr, sigma, table, argmax and g_sigma are required)");
  PDG_CHECK_ARG(criterion >= 0 && criterion <= 2, "pdg_stress_criteria_bwd: criterion must be 0, 1 or 2");
  PDG_CHECK_ARG(aggregate >= 0 && aggregate <= 3, "pdg_stress_criteria_bwd: aggregate must be 0, 1, 2 or 3");
  PDG_CHECK_ARG(std::isfinite(p) && p >= 1.0, "pdg_stress_criteria_bwd: p must be finite and >= 1");
  PDG_CHECK_ARG(std::isfinite(rho) && rho > 0.0, "pdg_stress_criteria_bwd: rho must be finite and > 0");
  hipLaunchKernelGGL(stress_criteria_bwd_kernel, dim3(n_graphs), dim3(CR_T), 0, (hipStream_t)stream, ptr, sigma,
                     weights, criterion, aggregate, p, rho, table, argmax, g_value, g_sigma);
  PDG_CHECK_LAUNCH("pdg_stress_criteria_bwd");
  return PDG_OK;
}
