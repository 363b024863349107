// The periodic hyperelastic cell problem on bilinear (Q1) quads (include/pdivgnn.h, "Q1 hyperelastic FEM targets"):
// pdg_hyper.hip's problem, law (pdg_neohooke.hpp) and solver on meshes of four-corner faces, integrated by the 2 x 2
// Gauss rule of pdg_femq1.hip, whose element table (F, 36) and plan arrays it reads:
//
//   F_g = Fbar + sum_k ut_k (x) grad N_k(g),   w_g = |det J_g|,   Phi = sum_f sum_g w_g W(F_g),
//   r_v = -sum_items sum_g w_g P_g grad N_c(g) = 0 at every periodic representative,
//
// solved, per (graph, load case), by pdg_hyper_solve's load stepping around its line-search Newton iteration around
// its matrix-free Jacobi-preconditioned conjugate gradients, word for word.  One persistent workgroup of 512 threads
// per problem, thread t owning the graph's rows t, t + 512, ... and faces f0 + t, f0 + t + 512, ..., every row
// gathered by its owner through the item rows in ascending order, every sum an fp64 block sum folded in a fixed
// order, no float atomics, nothing allocated, no memset: a graph gets bitwise the same rows and table row alone and
// inside any batch, and the call can be captured.  Every decision is taken from block sums every thread holds alike,
// so the barriers stay uniform, and every loop has pdg_hyper_solve's hard cap.
//
// The element pass stores P_g and A_g of every Gauss point (4 x 14 = 56 doubles a face and case in the caller's
// scratch, beside seven 2 N vectors); the rows read them back.  A face is inverted when any of its four J_g is <= 0
// or not finite.  Every loop over the four Gauss points is kept rolled, and still the solver wants some 158 VGPRs (a
// tangent row holds four representatives' vectors beside one point's gradients and its 4 x 4 tangent; the element
// pass a point's F, P and A beside the face's eight values): at 1024 threads, 128 VGPRs a thread, it spills 29 of
// them into the solver's loops, so the workgroup is 512 threads, 256 VGPRs a thread, and nothing spills.
#include <math.h>

#include "pdg_common.hpp"
#include "pdg_femmesh.hpp"
#include "pdg_neohooke.hpp"
#include "pdg_reduce.hpp"
#include "pdg_runtime.hpp"

using namespace pdg;
using namespace pdg::neohooke;

// Every expression below is evaluated as written: a trial state x + alpha d and the accepted x are the same bits.
#pragma clang fp contract(off)

namespace {

constexpr int HQ_T = 512;             // threads per (graph, case): the ownership stride
constexpr int HQ_GP = 9;              // pdg_femq1_elements' doubles per Gauss point: det J, dN/dx[4], dN/dy[4]
constexpr int HQ_ELEM = 4 * HQ_GP;    // doubles per face of the element table
constexpr int HQ_GS = 14;             // per Gauss point and case: P (4), A (10: the upper triangle, row-major)
constexpr int HQ_ES = 4 * HQ_GS;      // per face and case
constexpr int HQ_VECS = 7;            // x, g (the Newton residual), d, r (the inner residual), p, A p, 1 / diag
constexpr int HQ_MAX_STEPS = 10000;
constexpr int HQ_MAX_NEWTON = 1000;
constexpr int HQ_MAX_PCG = 100000;
constexpr int HQ_HALVINGS = 10;       // alpha = 1, 1/2, .. 2^-10
constexpr double HQ_ARMIJO = 1e-4;
// pdg_hyper.hip's allowance: a difference of two energies below 32 ulp of the sum of the terms' magnitudes before
// their cancellation is rounding, not an increase.
constexpr double HQ_PHI_NOISE = 32.0 * 2.220446049250313e-16;

enum { ST_CONVERGED = 0, ST_MAX_ITER = 2, ST_BREAKDOWN = 3 };   // pdg_fem_solve's codes; 1 (TRIVIAL) is not used

// The thread's index as a value the optimiser cannot see through (pdg_hyper.hip's own_index): a pass that starts from
// it forms its row addresses itself, where from threadIdx.x they are hoisted out of every solver loop and kept alive
// across the element passes, beyond the registers a thread has.
__device__ __forceinline__ int own_index() {
  int t = (int)threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

// The field q (2 per node) at the four nodes idx[4 f + k], or with TRIAL q + alpha d, each value formed as the
// accepted step forms it.  False when a node lies outside [n0, n1).
template <bool TRIAL>
__device__ __forceinline__ bool face_values(const int* idx, int f, int n0, int n1, const double* q, const double* d,
                                            double alpha, double (&ux)[4], double (&uy)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int rv = idx[4 * (size_t)f + k];
    if (rv < n0 || rv >= n1) return false;
    ux[k] = q[(size_t)rv * 2];
    uy[k] = q[(size_t)rv * 2 + 1];
    if (TRIAL) {
      ux[k] = ux[k] + alpha * d[(size_t)rv * 2];
      uy[k] = uy[k] + alpha * d[(size_t)rv * 2 + 1];
    }
  }
  return true;
}

// Fb + sum_k u_k (x) grad N_k at the Gauss point whose row of the element table is eg.
__device__ __forceinline__ void point_F(const double* eg, const double (&Fb)[4], const double (&ux)[4],
                                        const double (&uy)[4], double (&F)[4]) {
  F[0] = Fb[0] + ((eg[1] * ux[0] + eg[2] * ux[1]) + (eg[3] * ux[2] + eg[4] * ux[3]));
  F[1] = Fb[1] + ((eg[5] * ux[0] + eg[6] * ux[1]) + (eg[7] * ux[2] + eg[8] * ux[3]));
  F[2] = Fb[2] + ((eg[1] * uy[0] + eg[2] * uy[1]) + (eg[3] * uy[2] + eg[4] * uy[3]));
  F[3] = Fb[3] + ((eg[5] * uy[0] + eg[6] * uy[1]) + (eg[7] * uy[2] + eg[8] * uy[3]));
}

struct Problem {
  Mesh m;        // elem is (F, 36), verts / rverts / item hold 4 F entries
  Law w;
  int f0, f1;    // the graph's face segment, inside the mesh
  double* es;    // (F, 56) of this case
};

// The element pass: P_g and A_g of the graph's faces at x (or at x + alpha d) into es; out = Phi, the magnitude behind
// it, the inverted faces, the non-finite ones, valid in every thread; d and alpha with TRIAL only.  A face that is
// skipped (a node outside the graph), inverted or not finite at any of its Gauss points stores zeros at all four: it
// adds no force and no stiffness.  Starts with a barrier (x and d are written by their owners, the load factor by
// thread 0) and ends with the block sum's: es is visible to every row after it.
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
  for (int f = pb.f0 + own_index(); f < pb.f1; f += HQ_T) {
    const double* e = pb.m.elem + (size_t)f * HQ_ELEM;
    double* o = pb.es + (size_t)f * HQ_ES;
    double ux[4], uy[4];
    int state = 3;
    double fw = 0, fm = 0;   // the face's sum w_g W and the magnitude behind it, g = 0..3 in that order
    if (face_values<TRIAL>(pb.m.rverts, f, pb.m.n0, pb.m.n1, x, d, alpha, ux, uy)) {
      state = 0;
#pragma unroll 1
      for (int g = 0; g < 4; ++g) {
        const double* eg = e + g * HQ_GP;
        double* og = o + g * HQ_GS;
        double F[4];
        point_F(eg, Fb, ux, uy, F);
        const double J = F[0] * F[3] - F[1] * F[2];
        const int st = face_state(F, J);
        if (st != 0) {   // the face is what its worst point is
          state = st > state ? st : state;
          continue;
        }
        double W, mag, P[4];
        energy(pb.w, F, J, W, mag);
        stress_tangent<true>(pb.w, F, J, P, og + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) og[i] = P[i];
        const double wg = fabs(eg[0]);
        fw += wg * W;
        fm += wg * mag;
      }
    }
    if (state != 0) {
#pragma unroll 1
      for (int i = 0; i < HQ_ES; ++i) o[i] = 0.0;
      s[2] += state == 1 ? 1.0 : 0.0;
      s[3] += state == 2 ? 1.0 : 0.0;
      continue;
    }
    s[0] += fw;
    s[1] += fm;
  }
  block_sum_k_wave_major(s, red);
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = s[i];
}

// Row v of r = -sum_items sum_g w_g P_g grad N_c(g), of f_abs (the same sums of the terms' absolute values) and of
// diag of the tangent: the items in ascending order, g = 0..3 inside an item.
__device__ __forceinline__ void residual_row(const Problem& pb, int v, double& rx, double& ry, double& ax, double& ay,
                                             double& dx, double& dy) {
  rx = ry = ax = ay = dx = dy = 0;
  int j0, j1;
  row_range4(pb.m, v, j0, j1);
  for (int j = j0; j < j1; ++j) {
    int f, c;
    if (!item_of4(pb.m, j, f, c)) continue;
    const double* e = pb.m.elem + (size_t)f * HQ_ELEM;
    const double* sf = pb.es + (size_t)f * HQ_ES;
#pragma unroll 1
    for (int g = 0; g < 4; ++g) {
      const double* eg = e + g * HQ_GP;
      const double* s = sf + g * HQ_GS;
      const double wg = fabs(eg[0]), gx = eg[1 + c], gy = eg[5 + c];
      const double fx = wg * (s[0] * gx + s[1] * gy), fy = wg * (s[2] * gx + s[3] * gy);
      rx -= fx;
      ry -= fy;
      ax += fabs(fx);
      ay += fabs(fy);
      dx += wg * ((s[4] * (gx * gx) + 2.0 * s[5] * (gx * gy)) + s[8] * (gy * gy));
      dy += wg * ((s[11] * (gx * gx) + 2.0 * s[12] * (gx * gy)) + s[13] * (gy * gy));
    }
  }
}

// Row v of the tangent applied to q (2 per node, read at the face's four representatives): the items in ascending
// order, g = 0..3 inside an item, dF_g = sum_k q_k (x) grad N_k(g).
__device__ __forceinline__ void tangent_row(const Problem& pb, int v, const double* q, double& ax, double& ay) {
  ax = 0;
  ay = 0;
  int j0, j1;
  row_range4(pb.m, v, j0, j1);
  for (int j = j0; j < j1; ++j) {
    int f, c;
    if (!item_of4(pb.m, j, f, c)) continue;
    double qx[4], qy[4];
    if (!face_values<false>(pb.m.rverts, f, pb.m.n0, pb.m.n1, q, nullptr, 0.0, qx, qy)) continue;
    const double* e = pb.m.elem + (size_t)f * HQ_ELEM;
    const double* sf = pb.es + (size_t)f * HQ_ES + 4;
#pragma unroll 1
    for (int g = 0; g < 4; ++g) {
      const double* eg = e + g * HQ_GP;
      const double* s = sf + g * HQ_GS;
      const double zero[4] = {0, 0, 0, 0};
      double dF[4];
      point_F(eg, zero, qx, qy, dF);
      const double p0 = (s[0] * dF[0] + s[1] * dF[1]) + (s[2] * dF[2] + s[3] * dF[3]);
      const double p1 = (s[1] * dF[0] + s[4] * dF[1]) + (s[5] * dF[2] + s[6] * dF[3]);
      const double p2 = (s[2] * dF[0] + s[5] * dF[1]) + (s[7] * dF[2] + s[8] * dF[3]);
      const double p3 = (s[3] * dF[0] + s[6] * dF[1]) + (s[8] * dF[2] + s[9] * dF[3]);
      const double wg = fabs(eg[0]), gx = eg[1 + c], gy = eg[5 + c];
      ax += wg * (p0 * gx + p1 * gy);
      ay += wg * (p2 * gx + p3 * gy);
    }
  }
}

// pdg_hyper.hip's hyper_solve_kernel, word for word, on the passes above.  The scratch vectors and `ut` are written
// by one thread and read by others after a barrier: no __restrict__.
__global__ __launch_bounds__(HQ_T) void hyperq1_solve_kernel(
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
  double* x = scratch + (size_t)l * HQ_VECS * N2;
  double* gr = x + N2;
  double* d = gr + N2;
  double* r = d + N2;
  double* p = r + N2;
  double* ap = p + N2;
  double* dinv = ap + N2;
  double* uo = ut + (size_t)l * N2;
  const Problem pb{Mesh{nullptr, 2, n_nodes, n_faces, nullptr, rverts, rep, rowptr, item, elem, n0, n1},
                   Law{mu, kappa, vol}, f0, f1,
                   scratch + (size_t)n_cases * HQ_VECS * N2 + (size_t)l * HQ_ES * (size_t)n_faces};
  const double* fv = fbar + ((size_t)g * n_cases + l) * 4;

  // x = 0; the rows a thread owns are the representatives with items (`active`, dinv > 0 from here on)
  double nact = 0;
  for (int v = n0 + own_index(); v < n1; v += HQ_T) {
    const size_t k = (size_t)v * 2;
    int j0, j1;
    row_range4(pb.m, v, j0, j1);
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
  if (n_steps > HQ_MAX_STEPS) n_steps = HQ_MAX_STEPS;
  if (tid == 0) keep[2] = (double)n_steps;
  if (max_newton > HQ_MAX_NEWTON) max_newton = HQ_MAX_NEWTON;
  if (max_pcg > HQ_MAX_PCG) max_pcg = HQ_MAX_PCG;
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
      for (int v = n0 + own_index(); v < n1; v += HQ_T) {
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
      for (int v = n0 + own_index(); v < n1; v += HQ_T) {
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
        for (int v = n0 + own_index(); v < n1; v += HQ_T) {
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
            for (int v = n0 + own_index(); v < n1; v += HQ_T) {
              const size_t k = (size_t)v * 2;
              if (!(dinv[k] > 0.0)) continue;
              d[k] = p[k];
              d[k + 1] = p[k + 1];
            }
          break;
        }
        const double alpha = rz / pAp;
        double s6[6] = {0, 0, 0, 0, 0, 0};
        for (int v = n0 + own_index(); v < n1; v += HQ_T) {
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
        for (int v = n0 + own_index(); v < n1; v += HQ_T) {
          const size_t k = (size_t)v * 2;
          if (!(dinv[k] > 0.0)) continue;
          p[k] = (dinv[k] * r[k] - mx) + beta * p[k];
          p[k + 1] = (dinv[k + 1] * r[k + 1] - my) + beta * p[k + 1];
        }
      }
      pcgs += k_in;
      double rd = 0;
      for (int v = n0 + own_index(); v < n1; v += HQ_T) {
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

      // backtracking on Phi = sum w_g W: alpha = 1, 1/2, .. 2^-10
      double alpha = 1.0;
      bool accepted = false;
      for (int h = 0; h <= HQ_HALVINGS; ++h) {
        element_pass<true>(pb, fv, keep, x, red, e4, d, alpha);
        const double noise = HQ_PHI_NOISE * (phimag > e4[1] ? phimag : e4[1]);
        if (e4[2] == 0.0 && e4[3] == 0.0 && e4[0] <= (phi - HQ_ARMIJO * alpha * rd) + noise) {
          accepted = true;
          break;
        }
        alpha *= 0.5;
      }
      if (!accepted) {
        status = ST_BREAKDOWN;
        break;
      }
      for (int v = n0 + own_index(); v < n1; v += HQ_T) {
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
  for (int v = n0 + own_index(); v < n1; v += HQ_T) {
    const size_t k = (size_t)v * 2;
    if (!(dinv[k] > 0.0)) continue;
    mean[0] += x[k];
    mean[1] += x[k + 1];
  }
  block_sum_k_wave_major(mean, red);
  for (int v = n0 + own_index(); v < n1; v += HQ_T) {
    const size_t k = (size_t)v * 2;
    if (!(dinv[k] > 0.0) || !(nact > 0.0)) continue;
    x[k] -= mean[0] / nact;
    x[k + 1] -= mean[1] / nact;
  }
  double e4[4];
  if (tid == 0) keep[0] = 1.0;
  element_pass<false>(pb, fv, keep, x, red, e4);
  double tr[2] = {0, 0};
  for (int v = n0 + own_index(); v < n1; v += HQ_T) {
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
struct PointFields {
  double J, P[4];
  double sg[3];   // J sigma = P F^T: xx, yy, xy
  double le[3];   // 1/2 ln(F F^T): xx, yy, 2 xy
};

// ut at the four vertices of face f (its own nodes: an image holds its representative's row).  False when a vertex
// lies outside the mesh.
__device__ __forceinline__ bool face_ut(const int* verts, int n_nodes, const double* uo, int f, double (&ux)[4],
                                        double (&uy)[4]) {
  return face_values<false>(verts, f, 0, n_nodes, uo, nullptr, 0.0, ux, uy);
}

// The fields at the Gauss point whose row of the element table is eg.
__device__ __forceinline__ void point_fields(const Law& w, const double* eg, const double (&Fbar)[4],
                                             const double (&ux)[4], const double (&uy)[4], PointFields& o) {
  double F[4];
  point_F(eg, Fbar, ux, uy, F);
  o.J = F[0] * F[3] - F[1] * F[2];
  stress_tangent<false>(w, F, o.J, o.P, nullptr);
  kirchhoff(F, o.P, o.sg);
  log_strain(F, o.le);
}

__global__ __launch_bounds__(256) void hyperq1_nodal_kernel(
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
    if (j1 > 4 * n_faces) j1 = 4 * n_faces;
    for (int j = j0; j < j1; ++j) {   // the node's own corners among its representative's items, ascending
      const unsigned it = (unsigned)item[j];
      if (it >= 4u * (unsigned)n_faces || verts[it] != v) continue;
      const int f = (int)(it >> 2), c = (int)(it & 3u);
      double ux[4], uy[4];
      if (!face_ut(verts, n_nodes, uo, f, ux, uy)) continue;
      const double* eg = elem + (size_t)f * HQ_ELEM + c * HQ_GP;   // the Gauss point nearest the corner
      PointFields pf;
      point_fields(law, eg, Fbar, ux, uy, pf);
      const double wt = nodal == 0 ? fabs(eg[0]) * pf.J : 1.0;   // the point's deformed weight
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        as[i] += wt * (pf.sg[i] / pf.J);
        ae[i] += wt * pf.le[i];
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

// sums (B, L, 10): sum w_g J sigma (3), sum w_g P (4), sum w_g J, the material area sum w_g, the bounding box's area.
__global__ __launch_bounds__(HQ_T) void hyperq1_sums_kernel(
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
  for (int f = f0 + tid; f < f1; f += HQ_T) {
    double ux[4], uy[4];
    if (!face_ut(verts, n_nodes, uo, f, ux, uy)) continue;
#pragma unroll 1
    for (int gp = 0; gp < 4; ++gp) {
      const double* eg = elem + (size_t)f * HQ_ELEM + gp * HQ_GP;
      PointFields pf;
      point_fields(law, eg, Fbar, ux, uy, pf);
      const double wg = fabs(eg[0]);
#pragma unroll
      for (int i = 0; i < 3; ++i) s[i] += wg * pf.sg[i];
#pragma unroll
      for (int i = 0; i < 4; ++i) s[3 + i] += wg * pf.P[i];
      s[7] += wg * pf.J;
      s[8] += wg;
    }
  }
  block_sum_k_wave_major(s, red);
  float lo_x = INFINITY, hi_x = -INFINITY, lo_y = INFINITY, hi_y = -INFINITY;
  for (int v = n0 + tid; v < n1; v += HQ_T) {
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

constexpr long HQ_MAX_NODES = (1L << 31) / 4;   // 2 n, 4 f and n + 512 stay int32
constexpr int HQ_MAX_CASES = 64;

bool sizes_ok(int n_nodes, int n_faces) {
  return n_nodes > 0 && n_faces > 0 && (long)n_nodes < HQ_MAX_NODES && (long)n_faces < HQ_MAX_NODES;
}

long scratch_bytes(int n_nodes, int n_faces, int n_cases) {
  if (!sizes_ok(n_nodes, n_faces) || n_cases <= 0 || n_cases > HQ_MAX_CASES) return -1;
  const long doubles = (long)HQ_VECS * 2 * n_nodes + (long)HQ_ES * n_faces;
  return ((doubles * 8 * n_cases + 255) / 256) * 256;
}

bool law_ok(double mu, double kappa, int vol) {
  return mu > 0.0 && mu < INFINITY && kappa > 0.0 && kappa < INFINITY && (vol == 0 || vol == 1);
}

}  // namespace

extern "C" long pdg_hyperq1_solve_scratch_bytes(int n_nodes, int n_faces, int n_cases) {
  return scratch_bytes(n_nodes, n_faces, n_cases);
}

extern "C" int pdg_hyperq1_solve(int n_graphs, int n_cases, const int* ptr, const int* fptr, int n_nodes, int n_faces,
                                 const int* rverts, const int* rep, const int* item_rowptr, const int* item,
                                 const double* elem, const double* fbar, double mu, double kappa, int volumetric,
                                 double rtol, int n_steps, int max_newton, double eta, int max_pcg, double* ut,
                                 double* table, void* scratch, long scratch_bytes_, void* stream) {
  const long need = scratch_bytes(n_nodes, n_faces, n_cases);
  PDG_CHECK_ARG(need > 0 && n_graphs > 0 && n_graphs <= 65535,
                "pdg_hyperq1_solve: bad sizes (0 < n_graphs < 2^16, 0 < n_cases <= 64, 0 < n_nodes, n_faces < 2^29)");
  PDG_CHECK_ARG(ptr && fptr && rverts && rep && item_rowptr && item && elem && fbar && ut && table && scratch,
                "pdg_hyperq1_solve: null argument");
  PDG_CHECK_ARG(law_ok(mu, kappa, volumetric),
                "pdg_hyperq1_solve: mu and kappa must be finite and > 0, volumetric 0 (log) or 1 (quadratic)");
  PDG_CHECK_ARG(rtol > 0.0 && rtol < 1.0 && eta > 0.0 && eta < 1.0,
                "pdg_hyperq1_solve: rtol and eta must be in (0, 1)");
  PDG_CHECK_ARG(n_steps >= 1 && n_steps <= HQ_MAX_STEPS, "pdg_hyperq1_solve: n_steps must be in [1, 10000]");
  PDG_CHECK_ARG(scratch_bytes_ >= need, "pdg_hyperq1_solve: scratch too small");
  max_newton = max_newton < 0 ? 0 : max_newton > HQ_MAX_NEWTON ? HQ_MAX_NEWTON : max_newton;
  max_pcg = max_pcg < 1 ? 1 : max_pcg > HQ_MAX_PCG ? HQ_MAX_PCG : max_pcg;
  hipLaunchKernelGGL(hyperq1_solve_kernel, dim3(n_graphs, n_cases), dim3(HQ_T), 0, (hipStream_t)stream, n_cases, ptr,
                     fptr, n_nodes, n_faces, rverts, rep, item_rowptr, item, elem, fbar, mu, kappa, volumetric, rtol,
                     n_steps, max_newton, eta, max_pcg, ut, table, (double*)scratch);
  PDG_CHECK_LAUNCH("pdg_hyperq1_solve");
  return PDG_OK;
}

extern "C" int pdg_hyperq1_stress(int n_graphs, int n_cases, const int* ptr, const int* fptr, int n_nodes,
                                  const float* points, int dim, int n_faces, const int* verts, const int* rep,
                                  const int* item_rowptr, const int* item, const double* elem, const double* fbar,
                                  const double* ut, double mu, double kappa, int volumetric, int nodal, float* stress,
                                  float* strain, double* sums, void* stream) {
  PDG_CHECK_ARG(n_graphs > 0 && n_graphs <= 65535 && n_cases > 0 && n_cases <= HQ_MAX_CASES &&
                    sizes_ok(n_nodes, n_faces) && (dim == 2 || dim == 3),
                "pdg_hyperq1_stress: bad sizes (0 < n_graphs < 2^16, 0 < n_cases <= 64, 0 < n_nodes, n_faces < 2^29, "
                "dim 2 or 3)");
  PDG_CHECK_ARG(ptr && fptr && points && verts && rep && item_rowptr && item && elem && fbar && ut && stress &&
                    strain && sums,
                "pdg_hyperq1_stress: null argument");
  PDG_CHECK_ARG(law_ok(mu, kappa, volumetric),
                "pdg_hyperq1_stress: mu and kappa must be finite and > 0, volumetric 0 (log) or 1 (quadratic)");
  PDG_CHECK_ARG(nodal == 0 || nodal == 1, "pdg_hyperq1_stress: nodal is 0 (deformed weights) or 1 (counts)");
  hipLaunchKernelGGL(hyperq1_nodal_kernel, dim3((n_nodes + 255) / 256, n_cases), dim3(256), 0, (hipStream_t)stream,
                     n_graphs, n_cases, ptr, n_nodes, n_faces, verts, rep, item_rowptr, item, elem, fbar, ut, mu, kappa,
                     volumetric, nodal, stress, strain);
  hipLaunchKernelGGL(hyperq1_sums_kernel, dim3(n_graphs, n_cases), dim3(HQ_T), 0, (hipStream_t)stream, n_cases, ptr,
                     fptr, n_nodes, points, dim, n_faces, verts, elem, fbar, ut, mu, kappa, volumetric, sums);
  PDG_CHECK_LAUNCH("pdg_hyperq1_stress");
  return PDG_OK;
}
