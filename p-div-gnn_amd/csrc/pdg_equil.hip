// Equilibration of a stress field: the W-closest field whose divergence vanishes at the interior nodes, and the
// transpose of that projection (include/pdivgnn.h, "equilibration").  With A = [Dx | Dy] the operator pdg_div_fwd
// reads, m the mask node_types == 0 and W = diag(w, w, 2 w) on (xx, yy, xy):
//
//   (C s)_x[v] = m_v sum_c (Dx[v,c] sxx[c] + Dy[v,c] sxy[c]),   (C s)_y[v] = m_v sum_c (Dx[v,c] sxy[c] + Dy[v,c] syy[c])
//   S = C W^-1 C^T,   forward:   S lam = C in,        out = in - W^-1 C^T lam
//                     transpose: S lam = C W^-1 in,   out = in - C^T lam
//
// solved per graph by conjugate gradients on S.  As the metrics and homogenisation kernels: one workgroup per
// graph over the node segments ptr[0..B], thread t owning the graph's rows t, t + 1024, ... in that order, every
// inner product an fp64 block sum folded in a fixed order, no float atomics, nothing allocated, no memset: a graph
// gets bitwise the same rows and table row alone and inside any batch, and the call can be captured.
//
// The workgroup is persistent: it runs the whole iteration, the stopping decision included, and block barriers
// separate the phases.  The vectors are fp32 in the caller's scratch (lam, r, p, S p: 2 per node; the 3-per-node
// work field W^-1 C^T p): 44 bytes a node, L2-resident at the project's mesh sizes.  Each row of a product is
// accumulated in fp64 by the one thread that owns it and rounded once.  Row-wise passes (C .) walk a_rowptr,
// node-wise passes (C^T .) walk at_rowptr; neither scatters.  One iteration is two such gather passes, two block
// sums and six barriers, so the time of a solve is iterations x the latency of that chain, on one CU per graph.
#include <math.h>

#include "pdg_common.hpp"
#include "pdg_reduce.hpp"
#include "pdg_runtime.hpp"

using namespace pdg;

namespace {

constexpr int EQ_T = 1024;            // threads per graph
constexpr int EQ_FLOATS = 11;         // scratch floats per node: lam, r, p, sp (2 each) and work (3)

struct Op {
  const int* arp;
  const int* acol;
  const float* aval;
  const int* atp;
  const int* atrow;
  const int* atcomp;
  const float* atval;
  const float* wts;   // NULL: 1
  int n0, n;
};

__device__ __forceinline__ double inv_weight(const Op& o, int node) { return o.wts ? 1.0 / (double)o.wts[node] : 1.0; }

// Row v of A applied to the field f (N, 3), or to W^-1 f with `pre`: pdg_div_fwd's walk, fp64.  Entries with
// col >= 2 n (or negative) are skipped before anything is addressed with them.
__device__ __forceinline__ void row_apply(const Op& o, int v, const float* f, bool pre, double& d0, double& d1) {
  d0 = 0;
  d1 = 0;
  for (int j = o.arp[v]; j < o.arp[v + 1]; ++j) {
    const unsigned c = (unsigned)o.acol[j];
    if (c >= 2u * (unsigned)o.n) continue;
    const bool x = c < (unsigned)o.n;
    const int node = o.n0 + (int)(x ? c : c - (unsigned)o.n);
    const float* sv = f + (size_t)node * 3;
    // x block: (sxx, sxy); y block: (sxy, syy)
    double u0 = (double)(x ? sv[0] : sv[2]), u1 = (double)(x ? sv[2] : sv[1]);
    if (pre) {
      const double iw = inv_weight(o, node);
      u0 *= x ? iw : 0.5 * iw;
      u1 *= x ? 0.5 * iw : iw;
    }
    const double a = (double)o.aval[j];
    d0 = fma(a, u0, d0);
    d1 = fma(a, u1, d1);
  }
}

// Node c of C^T q, q (N, 2) over global rows (zero on the masked rows), or of W^-1 C^T q with `post`:
// pdg_div_bwd's walk, fp64.  An entry whose row lies outside the graph is skipped.
__device__ __forceinline__ void node_apply(const Op& o, int c, const float* q, bool post, double (&t)[3]) {
  double txx = 0, tyy = 0, txy = 0;
  for (int j = o.atp[c]; j < o.atp[c + 1]; ++j) {
    const int v = o.atrow[j];
    if ((unsigned)(v - o.n0) >= (unsigned)o.n) continue;
    const double a = (double)o.atval[j];
    const double qx = (double)q[(size_t)v * 2], qy = (double)q[(size_t)v * 2 + 1];
    if (o.atcomp[j] == 0) {
      txx = fma(a, qx, txx);
      txy = fma(a, qy, txy);
    } else {
      txy = fma(a, qx, txy);
      tyy = fma(a, qy, tyy);
    }
  }
  if (post) {
    const double iw = inv_weight(o, c);
    txx *= iw;
    tyy *= iw;
    txy *= 0.5 * iw;
  }
  t[0] = txx;
  t[1] = tyy;
  t[2] = txy;
}

// The scratch vectors and `out` are written by one thread and read by others after a barrier: no __restrict__.
__global__ __launch_bounds__(EQ_T) void equilibrate_kernel(
    const int* __restrict__ ptr, const int* __restrict__ arp, const int* __restrict__ acol,
    const float* __restrict__ aval, const int* __restrict__ atp, const int* __restrict__ atrow,
    const int* __restrict__ atcomp, const float* __restrict__ atval, const int64_t* __restrict__ types,
    const float* __restrict__ wts, const float* __restrict__ in, int transpose, float rtol, int max_iter, float* out,
    double* __restrict__ table, float* lam, float* r, float* p, float* sp, float* work) {
#pragma clang fp contract(off)
  __shared__ double red[16];
  const int g = blockIdx.x, tid = (int)threadIdx.x;
  const int n0 = ptr[g], n1 = ptr[g + 1];
  const int n = n1 - n0;
  double* row = table + (size_t)g * 4;
  if (n <= 0) {
    if (tid < 4) row[tid] = NAN;
    return;
  }
  const Op o{arp, acol, aval, atp, atrow, atcomp, atval, wts, n0, n};
  const bool tr = transpose != 0;
  const size_t e0 = (size_t)n0 * 3, e1 = (size_t)n1 * 3;

  int bad = 0;
  if (wts)
    for (int v = n0 + tid; v < n1; v += EQ_T) {
      const float w = wts[v];
      if (!(w > 0.f) || !(w < INFINITY)) bad = 1;
    }
  if (__syncthreads_or(bad)) {   // a weight <= 0 or not finite: W has no inverse
    for (size_t e = e0 + tid; e < e1; e += EQ_T) out[e] = in[e];
    if (tid == 0) {
      row[0] = NAN;
      row[1] = NAN;
      row[2] = 0.0;
      row[3] = 4.0;
    }
    return;
  }

  // b = C in (transpose: C W^-1 in); lam = 0, r = p = b
  double s = 0;
  for (int v = n0 + tid; v < n1; v += EQ_T) {
    double d0 = 0, d1 = 0;
    if (types[v] == 0) row_apply(o, v, in, tr, d0, d1);
    const size_t k = (size_t)v * 2;
    lam[k] = 0.f;
    lam[k + 1] = 0.f;
    r[k] = p[k] = (float)d0;
    r[k + 1] = p[k + 1] = (float)d1;
    s += d0 * d0 + d1 * d1;
  }
  double rr = block_sum(s, red);
  const double bnorm = sqrt(rr);
  if (rr == 0.0) {   // nothing to remove: no interior node, no operator entry, or a field C annihilates
    for (size_t e = e0 + tid; e < e1; e += EQ_T) out[e] = in[e];
    if (tid < 4) row[tid] = 0.0;
    return;
  }

  const double tol = (double)rtol * bnorm;
  double res = bnorm;
  int it = 0;
  while (it < max_iter && !(res <= tol)) {   // every thread holds the same rr: the decision is uniform
    __syncthreads();
    for (int c = n0 + tid; c < n1; c += EQ_T) {   // work = W^-1 C^T p
      double t[3];
      node_apply(o, c, p, true, t);
      float* wv = work + (size_t)c * 3;
      wv[0] = (float)t[0];
      wv[1] = (float)t[1];
      wv[2] = (float)t[2];
    }
    __syncthreads();
    s = 0;
    for (int v = n0 + tid; v < n1; v += EQ_T) {   // S p = C work
      if (types[v] != 0) continue;
      double d0, d1;
      row_apply(o, v, work, false, d0, d1);
      const size_t k = (size_t)v * 2;
      const float q0 = (float)d0, q1 = (float)d1;
      sp[k] = q0;
      sp[k + 1] = q1;
      s += (double)p[k] * (double)q0 + (double)p[k + 1] * (double)q1;
    }
    const double pSp = block_sum(s, red);
    if (!(pSp > 0.0)) break;   // breakdown (p in the null space of C^T, or a non-finite input)
    const double alpha = rr / pSp;
    s = 0;
    for (int v = n0 + tid; v < n1; v += EQ_T) {
      if (types[v] != 0) continue;
      const size_t k = (size_t)v * 2;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        lam[k + i] = (float)((double)lam[k + i] + alpha * (double)p[k + i]);
        const float ri = (float)((double)r[k + i] - alpha * (double)sp[k + i]);
        r[k + i] = ri;
        s += (double)ri * (double)ri;
      }
    }
    const double rrn = block_sum(s, red);
    const double beta = rrn / rr;
    rr = rrn;
    res = sqrt(rr);
    for (int v = n0 + tid; v < n1; v += EQ_T) {
      if (types[v] != 0) continue;
      const size_t k = (size_t)v * 2;
      p[k] = (float)((double)r[k] + beta * (double)p[k]);
      p[k + 1] = (float)((double)r[k + 1] + beta * (double)p[k + 1]);
    }
    ++it;
  }

  __syncthreads();
  if (it == 0) {
    for (size_t e = e0 + tid; e < e1; e += EQ_T) out[e] = in[e];
  } else {
    for (int c = n0 + tid; c < n1; c += EQ_T) {   // out = in - W^-1 C^T lam (transpose: in - C^T lam), rounded once
      double t[3];
      node_apply(o, c, lam, !tr, t);
      const size_t e = (size_t)c * 3;
      out[e] = (float)((double)in[e] - t[0]);
      out[e + 1] = (float)((double)in[e + 1] - t[1]);
      out[e + 2] = (float)((double)in[e + 2] - t[2]);
    }
  }
  __syncthreads();
  s = 0;
  for (int v = n0 + tid; v < n1; v += EQ_T) {   // the true residual, from the stored fp32 out
    if (types[v] != 0) continue;
    double d0, d1;
    row_apply(o, v, out, tr, d0, d1);
    s += d0 * d0 + d1 * d1;
  }
  const double tres = sqrt(block_sum(s, red));
  if (tid == 0) {
    row[0] = bnorm;
    row[1] = tres;
    row[2] = (double)it;
    row[3] = (double)((res <= tol ? 0 : 1) | (tres <= 2.0 * tol ? 0 : 2));
  }
}

constexpr long EQ_MAX_NODES = (1L << 31) / 4;   // 3 n and n + 1024 stay int32

long scratch_bytes(int n_nodes, int n_graphs) {
  if (n_nodes <= 0 || n_graphs <= 0 || (long)n_nodes >= EQ_MAX_NODES) return -1;
  return (((long)EQ_FLOATS * 4 * n_nodes + 255) / 256) * 256;
}

}  // namespace

extern "C" long pdg_equilibrate_scratch_bytes(int n_nodes, int n_graphs) { return scratch_bytes(n_nodes, n_graphs); }

extern "C" int pdg_equilibrate(int n_graphs, const int* ptr, int n_nodes, const int* a_rowptr, const int* a_col,
                               const float* a_val, const int* at_rowptr, const int* at_row, const int* at_comp,
                               const float* at_val, const int64_t* node_types, const float* weights, const float* in,
                               int transpose, float rtol, int max_iter, float* out, double* table, void* scratch,
                               long scratch_bytes_, void* stream) {
  const long need = scratch_bytes(n_nodes, n_graphs);
  PDG_CHECK_ARG(need > 0, "pdg_equilibrate: bad sizes (n_graphs > 0, 0 < n_nodes < 2^29)");
  PDG_CHECK_ARG(ptr && a_rowptr && a_col && a_val && at_rowptr && at_row && at_comp && at_val && node_types && in &&
                    out && table && scratch,
                "pdg_equilibrate: null argument (only weights may be NULL)");
  PDG_CHECK_ARG(rtol > 0.f && rtol < INFINITY, "pdg_equilibrate: rtol must be finite and > 0");
  PDG_CHECK_ARG(max_iter >= 0, "pdg_equilibrate: max_iter must be >= 0");
  PDG_CHECK_ARG(scratch_bytes_ >= need, "pdg_equilibrate: scratch too small");
  const uintptr_t lo_in = (uintptr_t)in, lo_out = (uintptr_t)out, span = (uintptr_t)n_nodes * 3 * sizeof(float);
  PDG_CHECK_ARG(lo_out + span <= lo_in || lo_in + span <= lo_out, "pdg_equilibrate: out may not alias in");
  float* f = (float*)scratch;
  const size_t N = (size_t)n_nodes;
  hipLaunchKernelGGL(equilibrate_kernel, dim3(n_graphs), dim3(EQ_T), 0, (hipStream_t)stream, ptr, a_rowptr, a_col,
                     a_val, at_rowptr, at_row, at_comp, at_val, node_types, weights, in, transpose, rtol, max_iter, out,
                     table, f, f + 2 * N, f + 4 * N, f + 6 * N, f + 8 * N);
  PDG_CHECK_LAUNCH("pdg_equilibrate");
  return PDG_OK;
}
