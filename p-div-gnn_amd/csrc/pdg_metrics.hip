// Evaluation metrics of a prediction against the FEM solution: the numeric part of the reference's
// scripts/compare_results.py (main, lines 1098-1245, with the helpers at 122-141, 333-364, 647-673,
// 713-726), segmented by the batch's node offsets `ptr` instead of the script's Python loop over the
// dataset with numpy / scipy.  As the loss kernels (pdg_loss.hip): one workgroup per graph, fp64
// accumulation in a fixed order, no float atomics, nothing allocated, no memset (both calls can be
// captured).
//
// Thread t of a graph's block owns the graph's rows t, t + 1024, ... in that order and the block's
// sums are folded in a fixed order, so what a graph gets depends on its own rows and their position
// inside the graph only: it scores bitwise the same alone and inside any batch.
#include <math.h>

#include "pdg_common.hpp"
#include "pdg_reduce.hpp"
#include "pdg_runtime.hpp"

using namespace pdg;

namespace {

constexpr int EV_T = 1024;   // threads per graph

// compare_results.py:713-726 in fp64.
__device__ __forceinline__ double von_mises(double x, double y, double xy) {
  return sqrt(0.5 * ((x - y) * (x - y) + x * x + y * y + 6.0 * (xy * xy)));
}

struct Node3 {
  float t[3], p[3];
};

__device__ __forceinline__ Node3 load_node(const float* __restrict__ gt, const float* __restrict__ pred, int i) {
  Node3 v;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    v.t[c] = gt[(size_t)i * 3 + c];
    v.p[c] = pred[(size_t)i * 3 + c];
  }
  return v;
}

// The first EV_C rows of a thread (EV_C * 1024 = 4,096 nodes per graph) stay in registers over the three
// passes (means; sums; fields), so the datasets' graphs (about 1,000 to 5,041 nodes) read gt / pred
// once or nearly so; rows beyond are read again in each pass.  The same sums in the same order either way.
constexpr int EV_C = 4;

__global__ __launch_bounds__(EV_T) void eval_nmse_kernel(const int* __restrict__ ptr, const float* __restrict__ gt,
                                                        const float* __restrict__ pred, double* __restrict__ table,
                                                        float* __restrict__ err, float* __restrict__ vm_gt,
                                                        float* __restrict__ vm_pred) {
  __shared__ double red[8 * 16];
  const int g = blockIdx.x;
  const int n0 = ptr[g], n1 = ptr[g + 1];
  if (n1 <= n0) {   // no nodes: NaN row, no field row touched (uniform over the block: no barrier is skipped)
    if (threadIdx.x < 6) table[(size_t)g * 6 + threadIdx.x] = NAN;
    return;
  }
  const double n = (double)(n1 - n0);
  const int first = n0 + (int)threadIdx.x;
  const int rest = first + EV_C * EV_T;
  Node3 c[EV_C];
#pragma unroll
  for (int k = 0; k < EV_C; ++k) {
    const int i = first + k * EV_T;
    if (i < n1) c[k] = load_node(gt, pred, i);
    else c[k] = Node3{{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  }

  // pass 1: column sums of gt and of its von Mises field
  double m[4] = {0, 0, 0, 0};
  auto acc_mean = [&](const Node3& v) {
#pragma unroll
    for (int k = 0; k < 3; ++k) m[k] += (double)v.t[k];
    m[3] += von_mises((double)v.t[0], (double)v.t[1], (double)v.t[2]);
  };
#pragma unroll
  for (int k = 0; k < EV_C; ++k)
    if (first + k * EV_T < n1) acc_mean(c[k]);
  for (int i = rest; i < n1; i += EV_T) acc_mean(load_node(gt, pred, i));
  block_sum_k<4>(m, red);
#pragma unroll
  for (int k = 0; k < 4; ++k) m[k] /= n;   // gt.mean(axis=0)

  // pass 2: s[k] = sum (gt - pred)^2, s[4 + k] = sum (gt - mean gt)^2; k = 3 is von Mises
  double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  auto acc_sums = [&](const Node3& v, int i) {
    double t[4], p[4];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      t[k] = (double)v.t[k];
      p[k] = (double)v.p[k];
    }
    t[3] = von_mises(t[0], t[1], t[2]);
    p[3] = von_mises(p[0], p[1], p[2]);
    if (vm_gt) vm_gt[i] = (float)t[3];
    if (vm_pred) vm_pred[i] = (float)p[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double d = t[k] - p[k], mm = t[k] - m[k];
      s[k] += d * d;
      s[4 + k] += mm * mm;
    }
  };
#pragma unroll
  for (int k = 0; k < EV_C; ++k)
    if (first + k * EV_T < n1) acc_sums(c[k], first + k * EV_T);
  for (int i = rest; i < n1; i += EV_T) acc_sums(load_node(gt, pred, i), i);
  block_sum_k<8>(s, red);

  if (threadIdx.x == 0) {
    double* row = table + (size_t)g * 6;
    const double r0 = s[0] / s[4], r1 = s[1] / s[5], r2 = s[2] / s[6];   // IEEE on a zero denominator
    const double mean = (r0 + r1 + r2) / 3.0;
    row[0] = r0;
    row[1] = r1;
    row[2] = r2;
    row[3] = mean;
    row[4] = s[3] / s[7];
    row[5] = 1.0 - mean;
  }
  if (err == nullptr) return;

  // pass 3: the element-wise field (compare_results.py:351-364), columns xx, yy, xy, von Mises
  auto put_err = [&](const Node3& v, int i) {
    double t[4], p[4];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      t[k] = (double)v.t[k];
      p[k] = (double)v.p[k];
    }
    t[3] = von_mises(t[0], t[1], t[2]);
    p[3] = von_mises(p[0], p[1], p[2]);
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double d = t[k] - p[k];
      o[k] = (float)((d * d) / s[4 + k]);
    }
    *reinterpret_cast<f32x4*>(err + (size_t)i * 4) = o;
  };
#pragma unroll
  for (int k = 0; k < EV_C; ++k)
    if (first + k * EV_T < n1) put_err(c[k], first + k * EV_T);
  for (int i = rest; i < n1; i += EV_T) put_err(load_node(gt, pred, i), i);
}

// One thread per row walks the row's entries once and forms the divergence of sigma and of the
// standardised field (sigma - mean) / std side by side, each product and sum in fp64.  The second
// is not the first over std: the operator's row sums are not zero on boundary rows.
__global__ __launch_bounds__(EV_T) void eval_div_kernel(const int* __restrict__ ptr, const int* __restrict__ arp,
                                                       const int* __restrict__ acol, const float* __restrict__ aval,
                                                       const int64_t* __restrict__ types,
                                                       const float* __restrict__ sig, double mean, double sd, int rabs,
                                                       double* __restrict__ table, float* __restrict__ norm,
                                                       float* __restrict__ norm_std) {
  __shared__ double red[4 * 16];
  const int g = blockIdx.x;
  const int n0 = ptr[g], n1 = ptr[g + 1];
  const int n = n1 - n0;
  if (n <= 0) {
    if (threadIdx.x < 2) table[(size_t)g * 2 + threadIdx.x] = NAN;
    return;
  }
  const bool fields = norm != nullptr || norm_std != nullptr;
  double s[4] = {0, 0, 0, 0};   // raw x, raw y, standardised x, standardised y
  for (int v = n0 + (int)threadIdx.x; v < n1; v += EV_T) {
    const int64_t t = types[v];
    double d0 = 0, d1 = 0, e0 = 0, e1 = 0;
    // an external-boundary row is zero everywhere; an internal-boundary one only in the scalars
    if (t != 1 && (t != -1 || fields)) {
      for (int j = arp[v]; j < arp[v + 1]; ++j) {
        const unsigned c = (unsigned)acol[j];
        const double a = (double)aval[j];
        if (c >= 2u * (unsigned)n) continue;   // beyond [:, :2 n_g] (the plan drops these; never dereferenced)
        const bool x = c < (unsigned)n;
        const float* sv = sig + (size_t)(n0 + (int)(x ? c : c - (unsigned)n)) * 3;
        // x block: (sxx, sxy); y block: (sxy, syy)
        const double u0 = (double)(x ? sv[0] : sv[2]), u1 = (double)(x ? sv[2] : sv[1]);
        d0 = fma(a, u0, d0);
        d1 = fma(a, u1, d1);
        e0 = fma(a, (u0 - mean) / sd, e0);
        e1 = fma(a, (u1 - mean) / sd, e1);
      }
    }
    if (norm) norm[v] = (float)sqrt(d0 * d0 + d1 * d1);
    if (norm_std) norm_std[v] = (float)sqrt(e0 * e0 + e1 * e1);
    if (t != -1) {
      s[0] += rabs ? fabs(d0) : d0 * d0;
      s[1] += rabs ? fabs(d1) : d1 * d1;
      s[2] += rabs ? fabs(e0) : e0 * e0;
      s[3] += rabs ? fabs(e1) : e1 * e1;
    }
  }
  block_sum_k<4>(s, red);
  if (threadIdx.x == 0) {
    const double nn = (double)n;
    table[(size_t)g * 2] = s[0] / nn + s[1] / nn;       // mean over all n_g rows, summed over x and y
    table[(size_t)g * 2 + 1] = s[2] / nn + s[3] / nn;
  }
}

}  // namespace

extern "C" int pdg_eval_nmse(int n_graphs, const int* ptr, const float* gt, const float* pred, double* table,
                             float* err_field, float* vm_gt, float* vm_pred, void* stream) {
  PDG_CHECK_ARG(n_graphs > 0, "pdg_eval_nmse: n_graphs must be > 0");
  PDG_CHECK_ARG(ptr && gt && pred && table, "pdg_eval_nmse: null argument (ptr, gt, pred and table are required)");
  PDG_CHECK_ARG(PDG_ALIGNED(err_field), "pdg_eval_nmse: err_field must be 16-byte aligned");
  hipLaunchKernelGGL(eval_nmse_kernel, dim3(n_graphs), dim3(EV_T), 0, (hipStream_t)stream, ptr, gt, pred, table,
                     err_field, vm_gt, vm_pred);
  PDG_CHECK_LAUNCH("pdg_eval_nmse");
  return PDG_OK;
}

extern "C" int pdg_eval_div(int n_graphs, const int* ptr, const int* a_rowptr, const int* a_col, const float* a_val,
                            const int64_t* node_types, const float* sigma, float mean, float std, int reduce_abs,
                            double* table, float* norm, float* norm_std, void* stream) {
  PDG_CHECK_ARG(n_graphs > 0, "pdg_eval_div: n_graphs must be > 0");
  PDG_CHECK_ARG(ptr && a_rowptr && a_col && a_val && node_types && sigma && table,
                "pdg_eval_div: null argument (only norm and norm_std may be NULL)");
  PDG_CHECK_ARG(std != 0.f, "pdg_eval_div: std must be non-zero");
  hipLaunchKernelGGL(eval_div_kernel, dim3(n_graphs), dim3(EV_T), 0, (hipStream_t)stream, ptr, a_rowptr, a_col, a_val,
                     node_types, sigma, (double)mean, (double)std, reduce_abs, table, norm, norm_std);
  PDG_CHECK_LAUNCH("pdg_eval_div");
  return PDG_OK;
}
