// The periodic hyperelastic cell problem on P1 triangles (include/pdivgnn.h, "Hyperelastic FEM targets"): compressible
// neo-Hookean in plane strain under a finite mean deformation,
//
//   u(X) = (Fbar - I) X + ut(X),  ut periodic,   F_e = Fbar + sum_k ut_k (x) g_k,   F3 = diag(F, 1),
//   W = mu / 2 (J^(-2/3) I1 - 3) + U(J),   I1 = tr(F^T F) + 1,   J = det F,
//   P = dW/dF = a F + c G,   a = mu J^(-2/3),  c = U'(J) - mu I1 J^(-5/3) / 3,  G = dJ/dF = J F^-T,
//   A = dP/dF = a I + k1 (F G^T + G F^T) + k2 G G^T + c dG/dF,   k1 = -2 mu J^(-5/3) / 3,
//                                                                k2 = 5 mu I1 J^(-8/3) / 9 + U''(J),
//
// on the 4-vector (F00, F01, F10, F11); A is symmetric, 10 values.  The balance sum_e area P_e g_c = 0 at every
// periodic representative is solved, per (graph, load case), by load stepping around a line-search Newton iteration
// around the matrix-free Jacobi-preconditioned conjugate gradients of pdg_fem.hip, the tangent applied from the A_e an
// element pass stored.  As pdg_fem.hip: one persistent workgroup of 1024 threads per problem, thread t owning the
// graph's rows t, t + 1024, ... and faces f0 + t, f0 + t + 1024, ..., every row gathered by its owner through the
// item rows, every sum an fp64 block sum folded in a fixed order, no float atomics, nothing allocated, no memset: a
// graph gets bitwise the same rows and table row alone and inside any batch, and the call can be captured.
//
// Every decision (convergence, truncation of the inner solve, acceptance of a step, every status) is taken from block
// sums every thread holds alike, so the barriers stay uniform, and every loop has a hard cap: load steps, Newton
// iterations per step, conjugate-gradient iterations per Newton iteration, 11 trial steps per line search.
//
// The element pass and the gathers are separate loops: the 4 x 4 tangent is formed and stored by the face's thread (14
// doubles a face and case in the caller's scratch, beside seven 2 N vectors), the rows read it back.
#include <math.h>

#include "pdg_common.hpp"
#include "pdg_femmesh.hpp"
#include "pdg_reduce.hpp"
#include "pdg_runtime.hpp"

using namespace pdg;

// Every expression below is evaluated as written: a trial state x + alpha d and the accepted x are the same bits.
#pragma clang fp contract(off)

namespace {

constexpr int HY_T = 1024;            // threads per (graph, case)
constexpr int HY_ELEM = 8;            // pdg_fem_elements' row: det, area, gx[3], gy[3]
constexpr int HY_ES = 14;             // per face and case: P (4), A (10: the upper triangle, row-major)
constexpr int HY_VECS = 7;            // x, g (the Newton residual), d, r (the inner residual), p, A p, 1 / diag
constexpr int HY_MAX_STEPS = 10000;
constexpr int HY_MAX_NEWTON = 1000;
constexpr int HY_MAX_PCG = 100000;
constexpr int HY_HALVINGS = 10;       // alpha = 1, 1/2, .. 2^-10
constexpr double HY_ARMIJO = 1e-4;
// The energies of two states are compared as rounded sums: a difference below 32 ulp of the sum of the terms'
// magnitudes before their cancellation (W takes 3 mu / 2 off, U takes J off) is rounding, not an increase.
constexpr double HY_PHI_NOISE = 32.0 * 2.220446049250313e-16;

enum { ST_CONVERGED = 0, ST_MAX_ITER = 2, ST_BREAKDOWN = 3 };   // pdg_fem_solve's codes; 1 (TRIVIAL) is not used

struct Law {
  double mu, kappa;
  int vol;   // 0: U = kappa (J ln J - J + 1), 1: U = kappa / 2 (J - 1)^2
};

// The thread's index as a value the optimiser cannot see through: a pass that starts from it forms its row addresses
// itself, where from threadIdx.x they are hoisted out of every solver loop, seven 64-bit addresses and more kept
// alive across the element passes, beyond the 128 registers a thread of a 1024-thread workgroup has.
__device__ __forceinline__ int own_index() {
  int t = (int)threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

__device__ __forceinline__ double jm23(double J) {   // J^(-2/3)
  const double c = cbrt(J);
  return 1.0 / (c * c);
}

__device__ __forceinline__ double trace1(const double (&F)[4]) {   // I1 of diag(F, 1)
  return ((F[0] * F[0] + F[1] * F[1]) + (F[2] * F[2] + F[3] * F[3])) + 1.0;
}

// W and the magnitude of its terms before they cancel.
__device__ __forceinline__ void energy(const Law& w, const double (&F)[4], double J, double& W, double& mag) {
  const double i1 = trace1(F), iso = jm23(J) * i1;
  const double jl = J * log(J);
  const double u = w.vol == 0 ? w.kappa * ((jl - J) + 1.0) : 0.5 * w.kappa * ((J - 1.0) * (J - 1.0));
  W = 0.5 * w.mu * (iso - 3.0) + u;
  mag = 0.5 * w.mu * (iso + 3.0) + w.kappa * ((fabs(jl) + J) + 1.0);
}

// P, and with TANGENT the upper triangle of A, row-major: 00 01 02 03 11 12 13 22 23 33.
template <bool TANGENT>
__device__ __forceinline__ void stress_tangent(const Law& w, const double (&F)[4], double J, double (&P)[4],
                                               double* A) {
  const double G[4] = {F[3], -F[2], -F[1], F[0]};
  const double i1 = trace1(F);
  const double a = w.mu * jm23(J);
  const double j53 = a / J;   // mu J^(-5/3)
  const double up = w.vol == 0 ? w.kappa * log(J) : w.kappa * (J - 1.0);
  const double c = up - (i1 / 3.0) * j53;
#pragma unroll
  for (int i = 0; i < 4; ++i) P[i] = a * F[i] + c * G[i];
  if (TANGENT) {
    const double upp = w.vol == 0 ? w.kappa / J : w.kappa;
    const double k1 = -(2.0 / 3.0) * j53;
    const double k2 = (5.0 / 9.0) * i1 * (j53 / J) + upp;
    int n = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int q = p; q < 4; ++q) {
        double v = k1 * (F[p] * G[q] + G[p] * F[q]) + k2 * (G[p] * G[q]);
        if (p == q) v += a;
        if (p == 0 && q == 3) v += c;
        if (p == 1 && q == 2) v -= c;
        A[n++] = v;
      }
  }
}

// F of face f from the field q (2 per node) read at the three nodes idx[3 f + k]: Fb + sum_k q_k (x) g_k, or with TRIAL
// from q + alpha d, each value formed as the accepted step forms it.  False when a node lies outside [n0, n1).
template <bool TRIAL>
__device__ __forceinline__ bool face_F(const double* e, const int* idx, int f, int n0, int n1, const double (&Fb)[4],
                                       const double* q, const double* d, double alpha, double (&F)[4]) {
  double ux[3], uy[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int rv = idx[3 * f + k];
    if (rv < n0 || rv >= n1) return false;
    ux[k] = q[(size_t)rv * 2];
    uy[k] = q[(size_t)rv * 2 + 1];
    if (TRIAL) {
      ux[k] = ux[k] + alpha * d[(size_t)rv * 2];
      uy[k] = uy[k] + alpha * d[(size_t)rv * 2 + 1];
    }
  }
  F[0] = Fb[0] + ((e[2] * ux[0] + e[3] * ux[1]) + e[4] * ux[2]);
  F[1] = Fb[1] + ((e[5] * ux[0] + e[6] * ux[1]) + e[7] * ux[2]);
  F[2] = Fb[2] + ((e[2] * uy[0] + e[3] * uy[1]) + e[4] * uy[2]);
  F[3] = Fb[3] + ((e[5] * uy[0] + e[6] * uy[1]) + e[7] * uy[2]);
  return true;
}

// 0 a sound element, 1 an inverted one (J <= 0), 2 a value that is not finite.
__device__ __forceinline__ int face_state(const double (&F)[4], double J) {
  if (!(trace1(F) < INFINITY) || !(J < INFINITY) || !(J > -INFINITY)) return 2;
  return J > 0.0 ? 0 : 1;
}

struct Problem {
  Mesh m;
  Law w;
  int f0, f1;    // the graph's face segment, inside the mesh
  double* es;    // (F, 14) of this case
};

// The element pass: P_e and A_e of the graph's faces at x (or at x + alpha d) into es; out = Phi, the magnitude behind
// it, the inverted elements, the non-finite ones, valid in every thread; d and alpha with TRIAL only.  A face that is
// skipped (a node outside the graph), inverted or not finite stores zeros: it adds no force and no stiffness.  Starts
// with a barrier (x and d are written by their owners, the load factor by thread 0) and ends with the block sum's: es
// is visible to every row after it.
template <bool TRIAL>
__device__ __forceinline__ void element_pass(const Problem& pb, const double* fbar, const double* load,
                                             const double* x, double* red, double (&out)[4],
                                             const double* d = nullptr, double alpha = 0.0) {
  __syncthreads();
  // Fbar(t) = I + t (Fbar - I), formed here from the problem's row and the load factor thread 0 left in LDS before
  // this barrier (neither is carried in registers across the solver's loops); Fbar itself, to the bit, at t = 1
  const double t = *load;
  const double Fb[4] = {t * fbar[0] + (1.0 - t), t * fbar[1], t * fbar[2], t * fbar[3] + (1.0 - t)};
  double s[4] = {0, 0, 0, 0};
  for (int f = pb.f0 + own_index(); f < pb.f1; f += HY_T) {
    const double* e = pb.m.elem + (size_t)f * HY_ELEM;
    double* o = pb.es + (size_t)f * HY_ES;
    double F[4];
    int state = 3;
    double J = 0;
    if (face_F<TRIAL>(e, pb.m.rverts, f, pb.m.n0, pb.m.n1, Fb, x, d, alpha, F)) {
      J = F[0] * F[3] - F[1] * F[2];
      state = face_state(F, J);
    }
    if (state != 0) {
#pragma unroll
      for (int i = 0; i < HY_ES; ++i) o[i] = 0.0;
      s[2] += state == 1 ? 1.0 : 0.0;
      s[3] += state == 2 ? 1.0 : 0.0;
      continue;
    }
    double W, mag, P[4];
    energy(pb.w, F, J, W, mag);
    stress_tangent<true>(pb.w, F, J, P, o + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = P[i];
    s[0] += e[1] * W;
    s[1] += e[1] * mag;
  }
  block_sum_k_wave_major(s, red);
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = s[i];
}

// Row v of r = -sum area P_e g_c, of f_abs (the same sums of the terms' absolute values) and of diag of the tangent:
// the items in ascending order.
__device__ __forceinline__ void residual_row(const Problem& pb, int v, double& rx, double& ry, double& ax, double& ay,
                                             double& dx, double& dy) {
  rx = ry = ax = ay = dx = dy = 0;
  int j0, j1;
  row_range(pb.m, v, j0, j1);
  for (int j = j0; j < j1; ++j) {
    int f, c;
    if (!item_of(pb.m, j, f, c)) continue;
    const double* e = pb.m.elem + (size_t)f * HY_ELEM;
    const double* s = pb.es + (size_t)f * HY_ES;
    const double area = e[1], gx = e[2 + c], gy = e[5 + c];
    const double fx = area * (s[0] * gx + s[1] * gy), fy = area * (s[2] * gx + s[3] * gy);
    rx -= fx;
    ry -= fy;
    ax += fabs(fx);
    ay += fabs(fy);
    dx += area * ((s[4] * (gx * gx) + 2.0 * s[5] * (gx * gy)) + s[8] * (gy * gy));
    dy += area * ((s[11] * (gx * gx) + 2.0 * s[12] * (gx * gy)) + s[13] * (gy * gy));
  }
}

// Row v of the tangent applied to q (2 per node, read at the representatives): the items in ascending order.
__device__ __forceinline__ void tangent_row(const Problem& pb, int v, const double* q, double& ax, double& ay) {
  ax = 0;
  ay = 0;
  int j0, j1;
  row_range(pb.m, v, j0, j1);
  for (int j = j0; j < j1; ++j) {
    int f, c;
    if (!item_of(pb.m, j, f, c)) continue;
    const double* e = pb.m.elem + (size_t)f * HY_ELEM;
    const double zero[4] = {0, 0, 0, 0};
    double dF[4];
    if (!face_F<false>(e, pb.m.rverts, f, pb.m.n0, pb.m.n1, zero, q, nullptr, 0.0, dF)) continue;
    const double* s = pb.es + (size_t)f * HY_ES + 4;
    const double p0 = (s[0] * dF[0] + s[1] * dF[1]) + (s[2] * dF[2] + s[3] * dF[3]);
    const double p1 = (s[1] * dF[0] + s[4] * dF[1]) + (s[5] * dF[2] + s[6] * dF[3]);
    const double p2 = (s[2] * dF[0] + s[5] * dF[1]) + (s[7] * dF[2] + s[8] * dF[3]);
    const double p3 = (s[3] * dF[0] + s[6] * dF[1]) + (s[8] * dF[2] + s[9] * dF[3]);
    const double area = e[1], gx = e[2 + c], gy = e[5 + c];
    ax += area * (p0 * gx + p1 * gy);
    ay += area * (p2 * gx + p3 * gy);
  }
}

__device__ __forceinline__ double inverse_diag(double d) {   // > 0 for every active row, whatever the tangent
  const double a = fabs(d);
  return a > 0.0 && a < INFINITY ? 1.0 / a : 1.0;
}

// The scratch vectors and `ut` are written by one thread and read by others after a barrier: no __restrict__.
__global__ __launch_bounds__(HY_T) void hyper_solve_kernel(
    int n_cases, const int* __restrict__ ptr, const int* __restrict__ fptr, int n_nodes, int n_faces,
    const int* __restrict__ rverts, const int* __restrict__ rep, const int* __restrict__ rowptr,
    const int* __restrict__ item, const double* __restrict__ elem, const double* __restrict__ fbar, double mu,
    double kappa, int vol, double rtol, int n_steps, int max_newton, double eta, int max_pcg, double* ut,
    double* __restrict__ table, double* scratch) {
  __shared__ double red[16 * 7];
  // the load factor of the step (read by every element pass); thread 0's own: the last |f_abs|, the step count
  __shared__ double keep[3];
  const int g = blockIdx.x, l = blockIdx.y, tid = (int)threadIdx.x;
  const int n0 = ptr[g], n1 = ptr[g + 1];
  double* row = table + ((size_t)g * n_cases + l) * 6;
  if (n1 <= n0 || n0 < 0 || n1 > n_nodes) {   // an empty graph (or offsets outside the batch): nothing else written
    if (tid < 6) row[tid] = NAN;
    return;
  }
  int f0 = fptr[g], f1 = fptr[g + 1];
  if (f0 < 0) f0 = 0;
  if (f1 > n_faces) f1 = n_faces;
  const size_t N2 = (size_t)n_nodes * 2;
  double* x = scratch + (size_t)l * HY_VECS * N2;
  double* gr = x + N2;
  double* d = gr + N2;
  double* r = d + N2;
  double* p = r + N2;
  double* ap = p + N2;
  double* dinv = ap + N2;
  double* uo = ut + (size_t)l * N2;
  const Problem pb{Mesh{nullptr, 2, n_nodes, n_faces, nullptr, rverts, rep, rowptr, item, elem, n0, n1},
                   Law{mu, kappa, vol}, f0, f1,
                   scratch + (size_t)n_cases * HY_VECS * N2 + (size_t)l * HY_ES * (size_t)n_faces};
  const double* fv = fbar + ((size_t)g * n_cases + l) * 4;

  // x = 0; the rows a thread owns are the representatives with items (`active`, dinv > 0 from here on)
  double nact = 0;
  for (int v = n0 + own_index(); v < n1; v += HY_T) {
    const size_t k = (size_t)v * 2;
    int j0, j1;
    row_range(pb.m, v, j0, j1);
    const bool act = rep[v] == v && j1 > j0;
    x[k] = x[k + 1] = gr[k] = gr[k + 1] = d[k] = d[k + 1] = r[k] = r[k + 1] = 0.0;
    p[k] = p[k + 1] = ap[k] = ap[k + 1] = 0.0;
    dinv[k] = dinv[k + 1] = act ? 1.0 : 0.0;
    nact += act ? 1.0 : 0.0;
  }
  nact = block_sum(nact, red);

  int status = nact > 0.0 ? -1 : ST_BREAKDOWN, steps_done = 0, newtons = 0, pcgs = 0;
  bool nonfinite = false;
  if (tid == 0) keep[1] = 0.0;
  if (n_steps > HY_MAX_STEPS) n_steps = HY_MAX_STEPS;
  if (tid == 0) keep[2] = (double)n_steps;
  if (max_newton > HY_MAX_NEWTON) max_newton = HY_MAX_NEWTON;
  if (max_pcg > HY_MAX_PCG) max_pcg = HY_MAX_PCG;
  for (int step = 1; step <= n_steps && status < 0; ++step) {
    if (tid == 0) keep[0] = (double)step / keep[2];
    double e4[4];
    element_pass<false>(pb, fv, keep, x, red, e4);
    double phi = e4[0], phimag = e4[1];
    if (e4[2] > 0.0 || e4[3] > 0.0 || !(phi < INFINITY)) {   // the last step's solution does not carry the new load
      status = ST_BREAKDOWN;
      nonfinite = e4[3] > 0.0 || !(phi < INFINITY);
      break;
    }
    for (int it = 0;; ++it) {   // ends at convergence, at max_newton or at a breakdown: every thread alike
      // the Newton residual, the diagonal, and the inner iteration's first sums
      double s[7] = {0, 0, 0, 0, 0, 0, 0};
      for (int v = n0 + own_index(); v < n1; v += HY_T) {
        const size_t k = (size_t)v * 2;
        if (!(dinv[k] > 0.0)) continue;
        double rx, ry, ax, ay, dx, dy;
        residual_row(pb, v, rx, ry, ax, ay, dx, dy);
        const double ix = inverse_diag(dx), iy = inverse_diag(dy);
        gr[k] = r[k] = rx;
        gr[k + 1] = r[k + 1] = ry;
        d[k] = d[k + 1] = 0.0;
        dinv[k] = ix;
        dinv[k + 1] = iy;
        s[0] += rx * rx + ry * ry;
        s[1] += ix * rx;
        s[2] += iy * ry;
        s[3] += ix * rx * rx + iy * ry * ry;
        s[4] += rx;
        s[5] += ry;
        s[6] += ax * ax + ay * ay;
      }
      block_sum_k_wave_major(s, red);
      if (!(s[0] < INFINITY) || !(s[6] < INFINITY)) {
        status = ST_BREAKDOWN;
        nonfinite = true;
        break;
      }
      const double rnorm = sqrt(s[0]);
      const double fnorm = sqrt(s[6]);
      if (tid == 0) keep[1] = fnorm;
      if (rnorm <= rtol * fnorm) break;   // the step's balance holds
      if (it >= max_newton) {
        status = ST_MAX_ITER;
        break;
      }

      // d: A d = r by conjugate gradients from 0, to |r_k| <= eta |r_0|, max_pcg iterations or the first direction
      // of no positive curvature; z = D^-1 r - its mean over the active rows, as pdg_fem_solve
      const double tol = eta * rnorm;
      double mx = s[1] / nact, my = s[2] / nact;
      double rz = s[3] - mx * s[4] - my * s[5];
      double res = rnorm;
      for (int v = n0 + own_index(); v < n1; v += HY_T) {
        const size_t k = (size_t)v * 2;
        if (!(dinv[k] > 0.0)) continue;
        p[k] = dinv[k] * r[k] - mx;
        p[k + 1] = dinv[k + 1] * r[k + 1] - my;
      }
      int k_in = 0;
      bool broke = false;
      while (k_in < max_pcg && !(res <= tol)) {
        __syncthreads();
        double q[1] = {0};
        for (int v = n0 + own_index(); v < n1; v += HY_T) {
          const size_t k = (size_t)v * 2;
          if (!(dinv[k] > 0.0)) continue;
          double ax, ay;
          tangent_row(pb, v, p, ax, ay);
          ap[k] = ax;
          ap[k + 1] = ay;
          q[0] += p[k] * ax + p[k + 1] * ay;
        }
        block_sum_k_wave_major(q, red);
        const double pAp = q[0];
        if (!(pAp < INFINITY) || !(pAp > -INFINITY) || !(rz < INFINITY) || !(rz > -INFINITY)) {
          broke = true;
          break;
        }
        if (!(pAp > 0.0)) {   // no positive curvature along p: the iterate so far, or z_0, a descent direction
          if (k_in == 0)
            for (int v = n0 + own_index(); v < n1; v += HY_T) {
              const size_t k = (size_t)v * 2;
              if (!(dinv[k] > 0.0)) continue;
              d[k] = p[k];
              d[k + 1] = p[k + 1];
            }
          break;
        }
        const double alpha = rz / pAp;
        double s6[6] = {0, 0, 0, 0, 0, 0};
        for (int v = n0 + own_index(); v < n1; v += HY_T) {
          const size_t k = (size_t)v * 2;
          const double ix = dinv[k], iy = dinv[k + 1];
          if (!(ix > 0.0)) continue;
          d[k] += alpha * p[k];
          d[k + 1] += alpha * p[k + 1];
          const double rx = r[k] - alpha * ap[k], ry = r[k + 1] - alpha * ap[k + 1];
          r[k] = rx;
          r[k + 1] = ry;
          s6[0] += rx * rx + ry * ry;
          s6[1] += ix * rx;
          s6[2] += iy * ry;
          s6[3] += ix * rx * rx + iy * ry * ry;
          s6[4] += rx;
          s6[5] += ry;
        }
        block_sum_k_wave_major(s6, red);
        ++k_in;
        res = sqrt(s6[0]);
        if (!(s6[0] < INFINITY)) {
          broke = true;
          break;
        }
        mx = s6[1] / nact;
        my = s6[2] / nact;
        const double rzn = s6[3] - mx * s6[4] - my * s6[5];
        const double beta = rzn / rz;
        rz = rzn;
        for (int v = n0 + own_index(); v < n1; v += HY_T) {
          const size_t k = (size_t)v * 2;
          if (!(dinv[k] > 0.0)) continue;
          p[k] = (dinv[k] * r[k] - mx) + beta * p[k];
          p[k + 1] = (dinv[k + 1] * r[k + 1] - my) + beta * p[k + 1];
        }
      }
      pcgs += k_in;
      double rd = 0;
      for (int v = n0 + own_index(); v < n1; v += HY_T) {
        const size_t k = (size_t)v * 2;
        if (!(dinv[k] > 0.0)) continue;
        rd += gr[k] * d[k] + gr[k + 1] * d[k + 1];
      }
      rd = block_sum(rd, red);
      if (broke || !(rd < INFINITY) || !(rd > -INFINITY)) {
        status = ST_BREAKDOWN;
        nonfinite = true;
        break;
      }

      // backtracking on Phi = sum area W: alpha = 1, 1/2, .. 2^-10
      double alpha = 1.0;
      bool accepted = false;
      for (int h = 0; h <= HY_HALVINGS; ++h) {
        element_pass<true>(pb, fv, keep, x, red, e4, d, alpha);
        const double noise = HY_PHI_NOISE * (phimag > e4[1] ? phimag : e4[1]);
        if (e4[2] == 0.0 && e4[3] == 0.0 && e4[0] <= (phi - HY_ARMIJO * alpha * rd) + noise) {
          accepted = true;
          break;
        }
        alpha *= 0.5;
      }
      if (!accepted) {
        status = ST_BREAKDOWN;
        break;
      }
      for (int v = n0 + own_index(); v < n1; v += HY_T) {
        const size_t k = (size_t)v * 2;
        if (!(dinv[k] > 0.0)) continue;
        x[k] = x[k] + alpha * d[k];
        x[k + 1] = x[k + 1] + alpha * d[k + 1];
      }
      phi = e4[0];
      phimag = e4[1];
      ++newtons;
    }
    if (status < 0) steps_done = step;
  }
  if (status < 0) status = ST_CONVERGED;

  // the iterate without its mean over the active rows (it has none but for rounding), the balance recomputed from
  // it under the whole load, then every node's row
  double mean[2] = {0, 0};
  for (int v = n0 + own_index(); v < n1; v += HY_T) {
    const size_t k = (size_t)v * 2;
    if (!(dinv[k] > 0.0)) continue;
    mean[0] += x[k];
    mean[1] += x[k + 1];
  }
  block_sum_k_wave_major(mean, red);
  for (int v = n0 + own_index(); v < n1; v += HY_T) {
    const size_t k = (size_t)v * 2;
    if (!(dinv[k] > 0.0) || !(nact > 0.0)) continue;
    x[k] -= mean[0] / nact;
    x[k + 1] -= mean[1] / nact;
  }
  double e4[4];
  if (tid == 0) keep[0] = 1.0;
  element_pass<false>(pb, fv, keep, x, red, e4);
  double tr[2] = {0, 0};
  for (int v = n0 + own_index(); v < n1; v += HY_T) {
    const size_t k = (size_t)v * 2;
    const int rv = rep[v];
    const bool in = rv >= n0 && rv < n1 && !nonfinite;
    uo[k] = in ? x[(size_t)rv * 2] : NAN;
    uo[k + 1] = in ? x[(size_t)rv * 2 + 1] : NAN;
    if (!(dinv[k] > 0.0)) continue;
    double rx, ry, ax, ay, dx, dy;
    residual_row(pb, v, rx, ry, ax, ay, dx, dy);
    tr[0] += rx * rx + ry * ry;
    tr[1] += ax * ax + ay * ay;
  }
  block_sum_k_wave_major(tr, red);
  if (tid == 0) {
    const bool sound = e4[2] == 0.0 && e4[3] == 0.0 && !nonfinite;
    row[0] = (double)steps_done;
    row[1] = (double)newtons;
    row[2] = (double)pcgs;
    row[3] = keep[1];
    row[4] = !sound ? NAN : tr[0] == 0.0 ? 0.0 : sqrt(tr[0]) / sqrt(tr[1]);
    row[5] = (double)status;
  }
}

// ------------------------------------------------------------------------------------------------------- fields
struct FaceFields {
  double J, P[4];
  double sg[3];   // J sigma = P F^T: xx, yy, xy
  double le[3];   // 1/2 ln(F F^T): xx, yy, 2 xy
};

// The fields of face f from ut at its own nodes.  False when a vertex lies outside the mesh.
__device__ __forceinline__ bool face_fields(const Law& w, const int* verts, const double* elem, int n_nodes,
                                            const double (&Fbar)[4], const double* uo, int f, FaceFields& o) {
  double F[4];
  if (!face_F<false>(elem + (size_t)f * HY_ELEM, verts, f, 0, n_nodes, Fbar, uo, nullptr, 0.0, F)) return false;
  o.J = F[0] * F[3] - F[1] * F[2];
  stress_tangent<false>(w, F, o.J, o.P, nullptr);
  o.sg[0] = o.P[0] * F[0] + o.P[1] * F[1];
  o.sg[1] = o.P[2] * F[2] + o.P[3] * F[3];
  o.sg[2] = o.P[0] * F[2] + o.P[1] * F[3];
  // ln B of the symmetric B = F F^T = m I + (B - m I), whose second term has the eigenvalues +-delta:
  // ln B = (ln l1 + ln l2) / 2 I + (ln l1 - ln l2) / (2 delta) (B - m I), and the factor -> 1 / m as delta -> 0
  const double b00 = F[0] * F[0] + F[1] * F[1], b11 = F[2] * F[2] + F[3] * F[3], b01 = F[0] * F[2] + F[1] * F[3];
  const double m = 0.5 * (b00 + b11), h = 0.5 * (b00 - b11);
  const double delta = sqrt(h * h + b01 * b01);
  const double l2 = m - delta;
  const double half_sum = 0.5 * log((m + delta) * l2);            // ln l1 + ln l2 = ln det B
  const double slope = delta > 0.0 ? log1p(2.0 * delta / l2) / (2.0 * delta) : 1.0 / m;
  o.le[0] = 0.5 * (half_sum + slope * h);
  o.le[1] = 0.5 * (half_sum - slope * h);
  o.le[2] = slope * b01;                                           // 2 * (1/2 ln B)_xy
  return true;
}

__global__ __launch_bounds__(256) void hyper_nodal_kernel(
    int n_graphs, int n_cases, const int* __restrict__ ptr, int n_nodes, int n_faces, const int* __restrict__ verts,
    const int* __restrict__ rep, const int* __restrict__ rowptr, const int* __restrict__ item,
    const double* __restrict__ elem, const double* __restrict__ fbar, const double* __restrict__ ut, double mu,
    double kappa, int vol, int nodal, float* __restrict__ stress, float* __restrict__ strain) {
  const int v = blockIdx.x * 256 + (int)threadIdx.x, l = blockIdx.y;
  if (v >= n_nodes) return;
  float* so = stress + ((size_t)l * n_nodes + v) * 3;
  float* eo = strain + ((size_t)l * n_nodes + v) * 3;
  const int g = graph_of(ptr, n_graphs, v);
  const int rv = rep[v];
  double as[3] = {0, 0, 0}, ae[3] = {0, 0, 0}, w = 0;
  if (v >= ptr[0] && v < ptr[n_graphs] && (unsigned)rv < (unsigned)n_nodes) {
    const Law law{mu, kappa, vol};
    const double* fv = fbar + ((size_t)g * n_cases + l) * 4;
    const double Fbar[4] = {fv[0], fv[1], fv[2], fv[3]};
    const double* uo = ut + (size_t)l * n_nodes * 2;
    int j0 = rowptr[rv], j1 = rowptr[rv + 1];
    if (j0 < 0) j0 = 0;
    if (j1 > 3 * n_faces) j1 = 3 * n_faces;
    for (int j = j0; j < j1; ++j) {   // the node's own corners among its representative's items, ascending
      const unsigned it = (unsigned)item[j];
      if (it >= 3u * (unsigned)n_faces || verts[it] != v) continue;
      const int f = (int)(it / 3u);
      FaceFields ff;
      if (!face_fields(law, verts, elem, n_nodes, Fbar, uo, f, ff)) continue;
      const double wt = nodal == 0 ? elem[(size_t)f * HY_ELEM + 1] * ff.J : 1.0;   // the deformed area
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        as[i] += wt * (ff.sg[i] / ff.J);
        ae[i] += wt * ff.le[i];
      }
      w += wt;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    so[i] = w != 0.0 ? (float)(as[i] / w) : 0.f;
    eo[i] = w != 0.0 ? (float)(ae[i] / w) : 0.f;
  }
}

// sums (B, L, 10): sum area J sigma (3), sum area P (4), sum area J, the material area, the bounding box's area.
__global__ __launch_bounds__(HY_T) void hyper_sums_kernel(
    int n_cases, const int* __restrict__ ptr, const int* __restrict__ fptr, int n_nodes,
    const float* __restrict__ points, int dim, int n_faces, const int* __restrict__ verts,
    const double* __restrict__ elem, const double* __restrict__ fbar, const double* __restrict__ ut, double mu,
    double kappa, int vol, double* __restrict__ sums) {
  __shared__ double red[16 * 9];
  __shared__ float box[16 * 4];
  const int g = blockIdx.x, l = blockIdx.y, tid = (int)threadIdx.x;
  double* row = sums + ((size_t)g * n_cases + l) * 10;
  const int n0 = ptr[g], n1 = ptr[g + 1];
  int f0 = fptr[g], f1 = fptr[g + 1];
  if (n1 <= n0 || n0 < 0 || n1 > n_nodes) {
    if (tid < 10) row[tid] = NAN;
    return;
  }
  if (f0 < 0) f0 = 0;
  if (f1 > n_faces) f1 = n_faces;
  const Law law{mu, kappa, vol};
  const double* fv = fbar + ((size_t)g * n_cases + l) * 4;
  const double Fbar[4] = {fv[0], fv[1], fv[2], fv[3]};
  const double* uo = ut + (size_t)l * n_nodes * 2;
  double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int f = f0 + tid; f < f1; f += HY_T) {
    FaceFields ff;
    if (!face_fields(law, verts, elem, n_nodes, Fbar, uo, f, ff)) continue;
    const double area = elem[(size_t)f * HY_ELEM + 1];
#pragma unroll
    for (int i = 0; i < 3; ++i) s[i] += area * ff.sg[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) s[3 + i] += area * ff.P[i];
    s[7] += area * ff.J;
    s[8] += area;
  }
  block_sum_k_wave_major(s, red);
  float lo_x = INFINITY, hi_x = -INFINITY, lo_y = INFINITY, hi_y = -INFINITY;
  for (int v = n0 + tid; v < n1; v += HY_T) {
    const float x = points[(size_t)v * dim], y = points[(size_t)v * dim + 1];
    lo_x = fminf(lo_x, x);
    hi_x = fmaxf(hi_x, x);
    lo_y = fminf(lo_y, y);
    hi_y = fmaxf(hi_y, y);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo_x = fminf(lo_x, __shfl_xor(lo_x, o));
    hi_x = fmaxf(hi_x, __shfl_xor(hi_x, o));
    lo_y = fminf(lo_y, __shfl_xor(lo_y, o));
    hi_y = fmaxf(hi_y, __shfl_xor(hi_y, o));
  }
  if (lane_id() == 0) {
    float* b = box + wave_id() * 4;
    b[0] = lo_x;
    b[1] = hi_x;
    b[2] = lo_y;
    b[3] = hi_y;
  }
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) {
      lo_x = fminf(lo_x, box[i * 4]);
      hi_x = fmaxf(hi_x, box[i * 4 + 1]);
      lo_y = fminf(lo_y, box[i * 4 + 2]);
      hi_y = fmaxf(hi_y, box[i * 4 + 3]);
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) row[i] = s[i];
    row[9] = ((double)hi_x - (double)lo_x) * ((double)hi_y - (double)lo_y);
  }
}

constexpr long HY_MAX_NODES = (1L << 31) / 4;   // 2 n, 3 f and n + 1024 stay int32
constexpr int HY_MAX_CASES = 64;

bool sizes_ok(int n_nodes, int n_faces) {
  return n_nodes > 0 && n_faces > 0 && (long)n_nodes < HY_MAX_NODES && (long)n_faces < HY_MAX_NODES;
}

long scratch_bytes(int n_nodes, int n_faces, int n_cases) {
  if (!sizes_ok(n_nodes, n_faces) || n_cases <= 0 || n_cases > HY_MAX_CASES) return -1;
  const long doubles = (long)HY_VECS * 2 * n_nodes + (long)HY_ES * n_faces;
  return ((doubles * 8 * n_cases + 255) / 256) * 256;
}

bool law_ok(double mu, double kappa, int vol) {
  return mu > 0.0 && mu < INFINITY && kappa > 0.0 && kappa < INFINITY && (vol == 0 || vol == 1);
}

}  // namespace

extern "C" long pdg_hyper_solve_scratch_bytes(int n_nodes, int n_faces, int n_cases) {
  return scratch_bytes(n_nodes, n_faces, n_cases);
}

extern "C" int pdg_hyper_solve(int n_graphs, int n_cases, const int* ptr, const int* fptr, int n_nodes, int n_faces,
                               const int* rverts, const int* rep, const int* item_rowptr, const int* item,
                               const double* elem, const double* fbar, double mu, double kappa, int volumetric,
                               double rtol, int n_steps, int max_newton, double eta, int max_pcg, double* ut,
                               double* table, void* scratch, long scratch_bytes_, void* stream) {
  const long need = scratch_bytes(n_nodes, n_faces, n_cases);
  PDG_CHECK_ARG(need > 0 && n_graphs > 0 && n_graphs <= 65535,
                "pdg_hyper_solve: bad sizes (0 < n_graphs < 2^16, 0 < n_cases <= 64, 0 < n_nodes, n_faces < 2^29)");
  PDG_CHECK_ARG(ptr && fptr && rverts && rep && item_rowptr && item && elem && fbar && ut && table && scratch,
                "pdg_hyper_solve: null argument");
  PDG_CHECK_ARG(law_ok(mu, kappa, volumetric),
                "pdg_hyper_solve: mu and kappa must be finite and > 0, volumetric 0 (log) or 1 (quadratic)");
  PDG_CHECK_ARG(rtol > 0.0 && rtol < 1.0 && eta > 0.0 && eta < 1.0, "pdg_hyper_solve: rtol and eta must be in (0, 1)");
  PDG_CHECK_ARG(n_steps >= 1 && n_steps <= HY_MAX_STEPS, "pdg_hyper_solve: n_steps must be in [1, 10000]");
  PDG_CHECK_ARG(scratch_bytes_ >= need, "pdg_hyper_solve: scratch too small");
  max_newton = max_newton < 0 ? 0 : max_newton > HY_MAX_NEWTON ? HY_MAX_NEWTON : max_newton;
  max_pcg = max_pcg < 1 ? 1 : max_pcg > HY_MAX_PCG ? HY_MAX_PCG : max_pcg;
  hipLaunchKernelGGL(hyper_solve_kernel, dim3(n_graphs, n_cases), dim3(HY_T), 0, (hipStream_t)stream, n_cases, ptr,
                     fptr, n_nodes, n_faces, rverts, rep, item_rowptr, item, elem, fbar, mu, kappa, volumetric, rtol,
                     n_steps, max_newton, eta, max_pcg, ut, table, (double*)scratch);
  PDG_CHECK_LAUNCH("pdg_hyper_solve");
  return PDG_OK;
}

extern "C" int pdg_hyper_stress(int n_graphs, int n_cases, const int* ptr, const int* fptr, int n_nodes,
                                const float* points, int dim, int n_faces, const int* verts, const int* rep,
                                const int* item_rowptr, const int* item, const double* elem, const double* fbar,
                                const double* ut, double mu, double kappa, int volumetric, int nodal, float* stress,
                                float* strain, double* sums, void* stream) {
  PDG_CHECK_ARG(n_graphs > 0 && n_graphs <= 65535 && n_cases > 0 && n_cases <= HY_MAX_CASES &&
                    sizes_ok(n_nodes, n_faces) && (dim == 2 || dim == 3),
                "pdg_hyper_stress: bad sizes (0 < n_graphs < 2^16, 0 < n_cases <= 64, 0 < n_nodes, n_faces < 2^29, "
                "dim 2 or 3)");
  PDG_CHECK_ARG(ptr && fptr && points && verts && rep && item_rowptr && item && elem && fbar && ut && stress &&
                    strain && sums,
                "pdg_hyper_stress: null argument");
  PDG_CHECK_ARG(law_ok(mu, kappa, volumetric),
                "pdg_hyper_stress: mu and kappa must be finite and > 0, volumetric 0 (log) or 1 (quadratic)");
  PDG_CHECK_ARG(nodal == 0 || nodal == 1, "pdg_hyper_stress: nodal is 0 (deformed-area weights) or 1 (counts)");
  hipLaunchKernelGGL(hyper_nodal_kernel, dim3((n_nodes + 255) / 256, n_cases), dim3(256), 0, (hipStream_t)stream,
                     n_graphs, n_cases, ptr, n_nodes, n_faces, verts, rep, item_rowptr, item, elem, fbar, ut, mu, kappa,
                     volumetric, nodal, stress, strain);
  hipLaunchKernelGGL(hyper_sums_kernel, dim3(n_graphs, n_cases), dim3(HY_T), 0, (hipStream_t)stream, n_cases, ptr,
                     fptr, n_nodes, points, dim, n_faces, verts, elem, fbar, ut, mu, kappa, volumetric, sums);
  PDG_CHECK_LAUNCH("pdg_hyper_stress");
  return PDG_OK;
}
