// The periodic elastic cell problem on bilinear (Q1) quads (include/pdivgnn.h, "Q1 FEM targets"): pdg_fem.hip's
// problem, material, load cases and solver on meshes of four-corner faces, integrated by the 2 x 2 Gauss rule.
//
//   K = sum_f sum_g |det J_g| B(g)^T C B(g),   A = P^T K P,   b = -P^T K (eps x),   A x = b,   sum x = 0
//
// The contract is fem_solve_kernel's: one persistent workgroup of 1024 threads per (graph, load case), thread t owning
// the graph's rows t, t + 1024, ... in that order, every product row gathered by its owner over the row's items in
// ascending order (nothing is scattered), every inner product an fp64 block sum folded in a fixed order, no float
// atomics, nothing allocated, no memset: a graph gets bitwise the same rows and table row alone and inside any batch,
// and the call can be captured.  Every decision that ends the iteration is taken from block sums every thread holds
// alike, so the barriers stay uniform and no input makes the workgroup spin.
//
// An item's corner force is a loop over the four Gauss points, 9 doubles of the element table each (det J, dN/dx[4],
// dN/dy[4]); the loop is kept rolled: at 1024 threads a thread has 128 VGPRs, and sixteen unrolled corner-point
// pairs of fp64 do not fit in them.
#include <math.h>

#include "pdg_common.hpp"
#include "pdg_femmesh.hpp"
#include "pdg_reduce.hpp"
#include "pdg_runtime.hpp"

using namespace pdg;

namespace {

constexpr int Q1_T = 1024;          // threads per (graph, case)
constexpr int Q1_GP = 9;            // doubles per Gauss point: det J, dN/dx[4], dN/dy[4]
constexpr int Q1_ELEM = 4 * Q1_GP;  // doubles per face
constexpr int Q1_VECS = 5;          // x, r, p, A p, 1 / diag
constexpr int Q1_MAX_ITER = 100000;
constexpr double Q1_NOISE = 1e-12;  // |b| <= Q1_NOISE |b_abs|: b is rounding noise
constexpr double Q1_GAUSS = 0.57735026918962576451;   // 1 / sqrt(3)

enum { ST_CONVERGED = 0, ST_TRIVIAL = 1, ST_MAX_ITER = 2, ST_BREAKDOWN = 3 };

struct Material {
  double c11, c12, c33;   // C = [[c11, c12, 0], [c12, c11, 0], [0, 0, c33]] on (xx, yy, gamma_xy)
};

__host__ __device__ inline Material material(double young, double poisson) {
  const double c11 = young / (1.0 - poisson * poisson);
  return Material{c11, poisson * c11, c11 * (1.0 - poisson) / 2.0};
}

// ------------------------------------------------------------------------------------------------ element table
__global__ void femq1_clear_status(int* status) { *status = 0; }

__global__ __launch_bounds__(256) void femq1_elements_kernel(int n_nodes, const float* __restrict__ points, int dim,
                                                             int n_faces, const int* __restrict__ verts,
                                                             double* __restrict__ elem, int* __restrict__ status) {
#pragma clang fp contract(off)
  const int f = blockIdx.x * 256 + (int)threadIdx.x;
  if (f >= n_faces) return;
  double* row = elem + (size_t)f * Q1_ELEM;
  double x[4], y[4];
  bool inside = true;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int v = verts[4 * (size_t)f + k];
    if ((unsigned)v >= (unsigned)n_nodes) {
      inside = false;
      x[k] = y[k] = 0;
    } else {
      x[k] = (double)points[(size_t)v * dim];
      y[k] = (double)points[(size_t)v * dim + 1];
    }
  }
  if (!inside) {
    atomicOr(status, 2);
    for (int i = 0; i < Q1_ELEM; ++i) row[i] = NAN;
    return;
  }
  // reference corners (-1, -1), (1, -1), (1, 1), (-1, 1); N_k = (1 + xi xi_k)(1 + eta eta_k) / 4
  const double cx[4] = {-1.0, 1.0, 1.0, -1.0}, cy[4] = {-1.0, -1.0, 1.0, 1.0};
  int pos = 0, neg = 0;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const double xi = cx[g] * Q1_GAUSS, eta = cy[g] * Q1_GAUSS;
    double nxi[4], neta[4];
    double xxi = 0, yxi = 0, xeta = 0, yeta = 0;   // J = [[dx/dxi, dy/dxi], [dx/deta, dy/deta]]
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      nxi[k] = 0.25 * cx[k] * (1.0 + eta * cy[k]);
      neta[k] = 0.25 * cy[k] * (1.0 + xi * cx[k]);
      xxi += nxi[k] * x[k];
      yxi += nxi[k] * y[k];
      xeta += neta[k] * x[k];
      yeta += neta[k] * y[k];
    }
    const double det = xxi * yeta - yxi * xeta;
    pos += det > 0.0 ? 1 : 0;
    neg += det < 0.0 ? 1 : 0;
    double* e = row + g * Q1_GP;
    e[0] = det;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      e[1 + k] = (yeta * nxi[k] - yxi * neta[k]) / det;
      e[5 + k] = (xxi * neta[k] - xeta * nxi[k]) / det;
    }
  }
  if (pos != 4 && neg != 4) atomicOr(status, 1);   // a zero, a non-convex quad, a bow-tie (or a NaN coordinate)
}

// ------------------------------------------------------------------------------------------------------- solver
__device__ __forceinline__ void stress_of(const Material& mt, const double (&ep)[3], double (&sg)[3]) {
  sg[0] = mt.c11 * ep[0] + mt.c12 * ep[1];
  sg[1] = mt.c12 * ep[0] + mt.c11 * ep[1];
  sg[2] = mt.c33 * ep[2];
}

// The strain (xx, yy, gamma_xy) at the Gauss point e from the face's four vertex displacements.
__device__ __forceinline__ void strain_of(const double* e, const double (&ux)[4], const double (&uy)[4],
                                          double (&ep)[3]) {
  ep[0] = (e[1] * ux[0] + e[2] * ux[1]) + (e[3] * ux[2] + e[4] * ux[3]);
  ep[1] = (e[5] * uy[0] + e[6] * uy[1]) + (e[7] * uy[2] + e[8] * uy[3]);
  ep[2] = ((e[5] * ux[0] + e[1] * uy[0]) + (e[6] * ux[1] + e[2] * uy[1])) +
          ((e[7] * ux[2] + e[3] * uy[2]) + (e[8] * ux[3] + e[4] * uy[3]));
}

// sum_g |det J_g| B_c(g)^T C B(g) u: the force of the face's stress at its corner c, g = 0..3 in that order.
__device__ __forceinline__ void corner_force(const double* e, int c, const Material& mt, const double (&ux)[4],
                                             const double (&uy)[4], double& fx, double& fy) {
  fx = 0;
  fy = 0;
#pragma unroll 1
  for (int g = 0; g < 4; ++g) {
    const double* eg = e + g * Q1_GP;
    double ep[3], sg[3];
    strain_of(eg, ux, uy, ep);
    stress_of(mt, ep, sg);
    const double w = fabs(eg[0]), gx = eg[1 + c], gy = eg[5 + c];
    fx += w * (gx * sg[0] + gy * sg[2]);
    fy += w * (gy * sg[1] + gx * sg[2]);
  }
}

// Row v of A applied to the vector q (2 per node, read at the representatives): the items in ascending order.
__device__ __forceinline__ void apply_row(const Mesh& m, const Material& mt, int v, const double* q, double& ax,
                                          double& ay) {
  ax = 0;
  ay = 0;
  int j0, j1;
  row_range4(m, v, j0, j1);
  for (int j = j0; j < j1; ++j) {
    int f, c;
    if (!item_of4(m, j, f, c)) continue;
    double ux[4], uy[4];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int rv = m.rverts[4 * (size_t)f + k];
      if (rv < m.n0 || rv >= m.n1) {
        ok = false;
        ux[k] = uy[k] = 0;
      } else {
        ux[k] = q[(size_t)rv * 2];
        uy[k] = q[(size_t)rv * 2 + 1];
      }
    }
    if (!ok) continue;
    double fx, fy;
    corner_force(m.elem + (size_t)f * Q1_ELEM, c, mt, ux, uy, fx, fy);
    ax += fx;
    ay += fy;
  }
}

// Row v of b = -P^T K (eps x) and of b_abs (the same sums of the items' absolute values), and of diag A.
__device__ __forceinline__ void rhs_row(const Mesh& m, const Material& mt, const double (&eps)[3], int v, double& bx,
                                        double& by, double& abx, double& aby, double& dx, double& dy) {
  bx = by = abx = aby = dx = dy = 0;
  int j0, j1;
  row_range4(m, v, j0, j1);
  for (int j = j0; j < j1; ++j) {
    int f, c;
    if (!item_of4(m, j, f, c)) continue;
    const double* e = m.elem + (size_t)f * Q1_ELEM;
    double ux[4], uy[4];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int nv = m.verts[4 * (size_t)f + k];
      if ((unsigned)nv >= (unsigned)m.n_nodes) {
        ok = false;
        ux[k] = uy[k] = 0;
      } else {
        const double x = (double)m.points[(size_t)nv * m.dim], y = (double)m.points[(size_t)nv * m.dim + 1];
        ux[k] = eps[0] * x + 0.5 * eps[2] * y;
        uy[k] = 0.5 * eps[2] * x + eps[1] * y;
      }
    }
    if (!ok) continue;
    double fx, fy;
    corner_force(e, c, mt, ux, uy, fx, fy);
    bx -= fx;
    by -= fy;
    abx += fabs(fx);
    aby += fabs(fy);
#pragma unroll 1
    for (int g = 0; g < 4; ++g) {
      const double* eg = e + g * Q1_GP;
      const double w = fabs(eg[0]), gx = eg[1 + c], gy = eg[5 + c];
      dx += w * (gx * gx * mt.c11 + gy * gy * mt.c33);
      dy += w * (gy * gy * mt.c11 + gx * gx * mt.c33);
    }
  }
}

// The scratch vectors and `ut` are written by one thread and read by others after a barrier: no __restrict__.
__global__ __launch_bounds__(Q1_T) void femq1_solve_kernel(
    int n_cases, const int* __restrict__ ptr, int n_nodes, const float* __restrict__ points, int dim, int n_faces,
    const int* __restrict__ verts, const int* __restrict__ rverts, const int* __restrict__ rep,
    const int* __restrict__ rowptr, const int* __restrict__ item, const double* __restrict__ elem,
    const double* __restrict__ strains, double young, double poisson, double rtol, int max_iter, double* ut,
    double* __restrict__ table, double* scratch) {
#pragma clang fp contract(off)
  __shared__ double red[16 * 6];
  const int g = blockIdx.x, l = blockIdx.y, tid = (int)threadIdx.x;
  const int n0 = ptr[g], n1 = ptr[g + 1];
  double* row = table + ((size_t)g * n_cases + l) * 4;
  if (n1 <= n0 || n0 < 0 || n1 > n_nodes) {   // an empty graph (or offsets outside the batch): nothing else written
    if (tid < 4) row[tid] = NAN;
    return;
  }
  const Mesh m{points, dim, n_nodes, n_faces, verts, rverts, rep, rowptr, item, elem, n0, n1};
  const Material mt = material(young, poisson);
  const double* sv = strains + ((size_t)g * n_cases + l) * 3;
  const double eps[3] = {sv[0], sv[1], sv[2]};
  const size_t N2 = (size_t)n_nodes * 2;
  double* x = scratch + (size_t)l * Q1_VECS * N2;
  double* r = x + N2;
  double* p = r + N2;
  double* ap = p + N2;
  double* dinv = ap + N2;
  double* uo = ut + (size_t)l * N2;

  // r = b, x = 0, 1 / diag; the rows a thread owns are the representatives with a diagonal (`active`)
  double s[6] = {0, 0, 0, 0, 0, 0};
  double babs2 = 0, nact = 0;
  for (int v = n0 + tid; v < n1; v += Q1_T) {
    const size_t k = (size_t)v * 2;
    double bx = 0, by = 0, abx = 0, aby = 0, dx = 0, dy = 0;
    if (rep[v] == v) rhs_row(m, mt, eps, v, bx, by, abx, aby, dx, dy);
    const bool act = dx > 0.0 && dy > 0.0;
    const double ix = act ? 1.0 / dx : 0.0, iy = act ? 1.0 / dy : 0.0;
    if (!act) bx = by = 0;
    x[k] = x[k + 1] = 0;
    r[k] = bx;
    r[k + 1] = by;
    dinv[k] = ix;
    dinv[k + 1] = iy;
    s[0] += bx * bx + by * by;
    s[1] += ix * bx;
    s[2] += iy * by;
    s[3] += ix * bx * bx + iy * by * by;
    s[4] += bx;
    s[5] += by;
    babs2 += abx * abx + aby * aby;
    nact += act ? 1.0 : 0.0;
  }
  block_sum_k_wave_major(s, red);
  double t2[2] = {babs2, nact};
  block_sum_k_wave_major(t2, red);
  const double bnorm = sqrt(s[0]), babs = sqrt(t2[0]);
  nact = t2[1];

  int status = -1, it = 0;
  if (bnorm <= Q1_NOISE * babs || nact == 0.0) status = ST_TRIVIAL;   // also b == 0 exactly
  else if (!(bnorm < INFINITY)) status = ST_BREAKDOWN;                 // a non-finite right-hand side
  if (status >= 0) {
    if (status == ST_TRIVIAL)
      for (int v = n0 + tid; v < n1; v += Q1_T) uo[(size_t)v * 2] = uo[(size_t)v * 2 + 1] = 0.0;
    else
      for (int v = n0 + tid; v < n1; v += Q1_T) uo[(size_t)v * 2] = uo[(size_t)v * 2 + 1] = NAN;
    if (tid == 0) {
      row[0] = 0.0;
      row[1] = bnorm;
      row[2] = status == ST_TRIVIAL ? 0.0 : NAN;
      row[3] = (double)status;
    }
    return;
  }

  // z = D^-1 r - its mean over the active rows; r . z = sum D^-1 r^2 - mean . sum r, from one pass's sums
  const double tol = rtol * bnorm;
  double mx = s[1] / nact, my = s[2] / nact;
  double rz = s[3] - mx * s[4] - my * s[5];
  double res = bnorm;
  for (int v = n0 + tid; v < n1; v += Q1_T) {
    const size_t k = (size_t)v * 2;
    const bool act = dinv[k] > 0.0;
    p[k] = act ? dinv[k] * r[k] - mx : 0.0;
    p[k + 1] = act ? dinv[k + 1] * r[k + 1] - my : 0.0;
  }
  if (max_iter > Q1_MAX_ITER) max_iter = Q1_MAX_ITER;
  while (it < max_iter && !(res <= tol)) {   // every thread holds the same sums: the decisions are uniform
    __syncthreads();
    double q[1] = {0};
    for (int v = n0 + tid; v < n1; v += Q1_T) {
      const size_t k = (size_t)v * 2;
      if (!(dinv[k] > 0.0)) continue;
      double ax, ay;
      apply_row(m, mt, v, p, ax, ay);
      ap[k] = ax;
      ap[k + 1] = ay;
      q[0] += p[k] * ax + p[k + 1] * ay;
    }
    block_sum_k_wave_major(q, red);
    const double pAp = q[0];
    if (!(pAp > 0.0) || !(pAp < INFINITY) || !(rz < INFINITY) || !(rz > -INFINITY)) {
      status = ST_BREAKDOWN;
      break;
    }
    const double alpha = rz / pAp;
#pragma unroll
    for (int i = 0; i < 6; ++i) s[i] = 0;
    for (int v = n0 + tid; v < n1; v += Q1_T) {
      const size_t k = (size_t)v * 2;
      const double ix = dinv[k], iy = dinv[k + 1];
      if (!(ix > 0.0)) continue;
      x[k] += alpha * p[k];
      x[k + 1] += alpha * p[k + 1];
      const double rx = r[k] - alpha * ap[k], ry = r[k + 1] - alpha * ap[k + 1];
      r[k] = rx;
      r[k + 1] = ry;
      s[0] += rx * rx + ry * ry;
      s[1] += ix * rx;
      s[2] += iy * ry;
      s[3] += ix * rx * rx + iy * ry * ry;
      s[4] += rx;
      s[5] += ry;
    }
    block_sum_k_wave_major(s, red);
    ++it;
    res = sqrt(s[0]);
    if (!(s[0] < INFINITY)) {   // a non-finite residual (NaN included)
      status = ST_BREAKDOWN;
      break;
    }
    mx = s[1] / nact;
    my = s[2] / nact;
    const double rzn = s[3] - mx * s[4] - my * s[5];
    const double beta = rzn / rz;
    rz = rzn;
    for (int v = n0 + tid; v < n1; v += Q1_T) {
      const size_t k = (size_t)v * 2;
      if (!(dinv[k] > 0.0)) continue;
      p[k] = (dinv[k] * r[k] - mx) + beta * p[k];
      p[k + 1] = (dinv[k + 1] * r[k + 1] - my) + beta * p[k + 1];
    }
  }
  if (status < 0) status = res <= tol ? ST_CONVERGED : ST_MAX_ITER;

  // the iterate without its mean over the active rows (it has none but for rounding), then every node's row
  double mu[2] = {0, 0};
  for (int v = n0 + tid; v < n1; v += Q1_T) {
    const size_t k = (size_t)v * 2;
    if (!(dinv[k] > 0.0)) continue;
    mu[0] += x[k];
    mu[1] += x[k + 1];
  }
  block_sum_k_wave_major(mu, red);
  for (int v = n0 + tid; v < n1; v += Q1_T) {
    const size_t k = (size_t)v * 2;
    if (!(dinv[k] > 0.0)) continue;
    x[k] -= mu[0] / nact;
    x[k + 1] -= mu[1] / nact;
  }
  __syncthreads();
  double tr[1] = {0};
  for (int v = n0 + tid; v < n1; v += Q1_T) {
    const size_t k = (size_t)v * 2;
    const int rv = rep[v];
    const bool in = rv >= n0 && rv < n1;
    uo[k] = in ? x[(size_t)rv * 2] : NAN;
    uo[k + 1] = in ? x[(size_t)rv * 2 + 1] : NAN;
    if (!(dinv[k] > 0.0)) continue;
    // the true residual b - A x, both recomputed
    double bx, by, abx, aby, dx, dy, ax, ay;
    rhs_row(m, mt, eps, v, bx, by, abx, aby, dx, dy);
    apply_row(m, mt, v, x, ax, ay);
    tr[0] += (bx - ax) * (bx - ax) + (by - ay) * (by - ay);
  }
  block_sum_k_wave_major(tr, red);
  if (tid == 0) {
    row[0] = (double)it;
    row[1] = bnorm;
    row[2] = sqrt(tr[0]) / bnorm;
    row[3] = (double)status;
  }
}

// ------------------------------------------------------------------------------------------------------- fields
// u = eps x + ut at the four vertices of face f.  False when a vertex lies outside the mesh.
__device__ __forceinline__ bool face_displacements(const float* points, int dim, int n_nodes, const int* verts,
                                                   const double* uo, const double (&eps)[3], int f, double (&ux)[4],
                                                   double (&uy)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int nv = verts[4 * (size_t)f + k];
    if ((unsigned)nv >= (unsigned)n_nodes) return false;
    const double x = (double)points[(size_t)nv * dim], y = (double)points[(size_t)nv * dim + 1];
    ux[k] = (eps[0] * x + 0.5 * eps[2] * y) + uo[(size_t)nv * 2];
    uy[k] = (0.5 * eps[2] * x + eps[1] * y) + uo[(size_t)nv * 2 + 1];
  }
  return true;
}

__global__ __launch_bounds__(256) void femq1_nodal_kernel(
    int n_graphs, int n_cases, const int* __restrict__ ptr, int n_nodes, const float* __restrict__ points, int dim,
    int n_faces, const int* __restrict__ verts, const int* __restrict__ rep, const int* __restrict__ rowptr,
    const int* __restrict__ item, const double* __restrict__ elem, const double* __restrict__ strains,
    const double* __restrict__ ut, double young, double poisson, int nodal, float* __restrict__ stress,
    float* __restrict__ strain) {
#pragma clang fp contract(off)
  const int v = blockIdx.x * 256 + (int)threadIdx.x, l = blockIdx.y;
  if (v >= n_nodes) return;
  float* so = stress + ((size_t)l * n_nodes + v) * 3;
  float* eo = strain + ((size_t)l * n_nodes + v) * 3;
  const int g = graph_of(ptr, n_graphs, v);
  const int rv = rep[v];
  double as[3] = {0, 0, 0}, ae[3] = {0, 0, 0}, w = 0;
  if (v >= ptr[0] && v < ptr[n_graphs] && (unsigned)rv < (unsigned)n_nodes) {
    const Material mt = material(young, poisson);
    const double* sv = strains + ((size_t)g * n_cases + l) * 3;
    const double eps[3] = {sv[0], sv[1], sv[2]};
    const double* uo = ut + (size_t)l * n_nodes * 2;
    int j0 = rowptr[rv], j1 = rowptr[rv + 1];
    if (j0 < 0) j0 = 0;
    if (j1 > 4 * n_faces) j1 = 4 * n_faces;
    for (int j = j0; j < j1; ++j) {   // the node's own corners among its representative's items, ascending
      const unsigned it = (unsigned)item[j];
      if (it >= 4u * (unsigned)n_faces || verts[it] != v) continue;
      const int f = (int)(it >> 2), c = (int)(it & 3u);
      double ux[4], uy[4], ep[3], sg[3];
      if (!face_displacements(points, dim, n_nodes, verts, uo, eps, f, ux, uy)) continue;
      const double* eg = elem + (size_t)f * Q1_ELEM + c * Q1_GP;   // the Gauss point nearest the corner
      strain_of(eg, ux, uy, ep);
      stress_of(mt, ep, sg);
      const double wt = nodal == 0 ? fabs(eg[0]) : 1.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        as[i] += wt * sg[i];
        ae[i] += wt * ep[i];
      }
      w += wt;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    so[i] = w > 0.0 ? (float)(as[i] / w) : 0.f;
    eo[i] = w > 0.0 ? (float)(ae[i] / w) : 0.f;
  }
}

// sums (B, L, 8): sum |det J| sigma (3), sum |det J| eps (3), the material area, the bounding box's area.
__global__ __launch_bounds__(Q1_T) void femq1_sums_kernel(
    int n_cases, const int* __restrict__ ptr, const int* __restrict__ fptr, int n_nodes,
    const float* __restrict__ points, int dim, int n_faces, const int* __restrict__ verts,
    const double* __restrict__ elem, const double* __restrict__ strains, const double* __restrict__ ut, double young,
    double poisson, double* __restrict__ sums) {
#pragma clang fp contract(off)
  __shared__ double red[16 * 7];
  __shared__ float box[16 * 4];
  const int g = blockIdx.x, l = blockIdx.y, tid = (int)threadIdx.x;
  double* row = sums + ((size_t)g * n_cases + l) * 8;
  const int n0 = ptr[g], n1 = ptr[g + 1];
  int f0 = fptr[g], f1 = fptr[g + 1];
  if (n1 <= n0 || n0 < 0 || n1 > n_nodes) {
    if (tid < 8) row[tid] = NAN;
    return;
  }
  if (f0 < 0) f0 = 0;
  if (f1 > n_faces) f1 = n_faces;
  const Material mt = material(young, poisson);
  const double* sv = strains + ((size_t)g * n_cases + l) * 3;
  const double eps[3] = {sv[0], sv[1], sv[2]};
  const double* uo = ut + (size_t)l * n_nodes * 2;
  double s[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int f = f0 + tid; f < f1; f += Q1_T) {
    double ux[4], uy[4];
    if (!face_displacements(points, dim, n_nodes, verts, uo, eps, f, ux, uy)) continue;
#pragma unroll 1
    for (int gp = 0; gp < 4; ++gp) {
      const double* eg = elem + (size_t)f * Q1_ELEM + gp * Q1_GP;
      double ep[3], sg[3];
      strain_of(eg, ux, uy, ep);
      stress_of(mt, ep, sg);
      const double wt = fabs(eg[0]);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        s[i] += wt * sg[i];
        s[3 + i] += wt * ep[i];
      }
      s[6] += wt;
    }
  }
  block_sum_k_wave_major(s, red);
  float lo_x = INFINITY, hi_x = -INFINITY, lo_y = INFINITY, hi_y = -INFINITY;
  for (int v = n0 + tid; v < n1; v += Q1_T) {
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
    for (int i = 0; i < 7; ++i) row[i] = s[i];
    row[7] = ((double)hi_x - (double)lo_x) * ((double)hi_y - (double)lo_y);
  }
}

constexpr long Q1_MAX_NODES = (1L << 31) / 4;   // 2 n, 4 f - 1 and n + 1024 stay int32
constexpr int Q1_MAX_CASES = 64;

bool sizes_ok(int n_nodes, int n_faces) {
  return n_nodes > 0 && n_faces > 0 && (long)n_nodes < Q1_MAX_NODES && (long)n_faces < Q1_MAX_NODES;
}

long scratch_bytes(int n_nodes, int n_cases) {
  if (n_nodes <= 0 || n_cases <= 0 || n_cases > Q1_MAX_CASES || (long)n_nodes >= Q1_MAX_NODES) return -1;
  return (((long)Q1_VECS * 2 * 8 * n_nodes * n_cases + 255) / 256) * 256;
}

bool material_ok(double young, double poisson) {
  return young > 0.0 && young < INFINITY && poisson > -1.0 && poisson < 0.5;
}

}  // namespace

extern "C" int pdg_femq1_elements(int n_nodes, const float* points, int dim, int n_faces, const int* verts,
                                  double* elem, int* status, void* stream) {
  PDG_CHECK_ARG(sizes_ok(n_nodes, n_faces) && (dim == 2 || dim == 3),
                "pdg_femq1_elements: bad sizes (0 < n_nodes, n_faces < 2^29, dim 2 or 3)");
  PDG_CHECK_ARG(points && verts && elem && status, "pdg_femq1_elements: null argument");
  hipLaunchKernelGGL(femq1_clear_status, dim3(1), dim3(1), 0, (hipStream_t)stream, status);
  hipLaunchKernelGGL(femq1_elements_kernel, dim3((n_faces + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_nodes,
                     points, dim, n_faces, verts, elem, status);
  PDG_CHECK_LAUNCH("pdg_femq1_elements");
  return PDG_OK;
}

extern "C" long pdg_femq1_solve_scratch_bytes(int n_nodes, int n_cases) { return scratch_bytes(n_nodes, n_cases); }

extern "C" int pdg_femq1_solve(int n_graphs, int n_cases, const int* ptr, int n_nodes, const float* points, int dim,
                               int n_faces, const int* verts, const int* rverts, const int* rep,
                               const int* item_rowptr, const int* item, const double* elem, const double* strains,
                               double young, double poisson, double rtol, int max_iter, double* ut, double* table,
                               void* scratch, long scratch_bytes_, void* stream) {
  const long need = scratch_bytes(n_nodes, n_cases);
  PDG_CHECK_ARG(need > 0 && n_graphs > 0 && n_graphs <= 65535 && sizes_ok(n_nodes, n_faces) && (dim == 2 || dim == 3),
                "pdg_femq1_solve: bad sizes (0 < n_graphs < 2^16, 0 < n_cases <= 64, 0 < n_nodes, n_faces < 2^29, dim "
                "2 or 3)");
  PDG_CHECK_ARG(ptr && points && verts && rverts && rep && item_rowptr && item && elem && strains && ut && table &&
                    scratch,
                "pdg_femq1_solve: null argument");
  PDG_CHECK_ARG(material_ok(young, poisson), "pdg_femq1_solve: young must be finite and > 0, poisson in (-1, 0.5)");
  PDG_CHECK_ARG(rtol > 0.0 && rtol < 1.0, "pdg_femq1_solve: rtol must be in (0, 1)");
  PDG_CHECK_ARG(scratch_bytes_ >= need, "pdg_femq1_solve: scratch too small");
  max_iter = max_iter < 0 ? 0 : max_iter > Q1_MAX_ITER ? Q1_MAX_ITER : max_iter;
  hipLaunchKernelGGL(femq1_solve_kernel, dim3(n_graphs, n_cases), dim3(Q1_T), 0, (hipStream_t)stream, n_cases, ptr,
                     n_nodes, points, dim, n_faces, verts, rverts, rep, item_rowptr, item, elem, strains, young,
                     poisson, rtol, max_iter, ut, table, (double*)scratch);
  PDG_CHECK_LAUNCH("pdg_femq1_solve");
  return PDG_OK;
}

extern "C" int pdg_femq1_stress(int n_graphs, int n_cases, const int* ptr, const int* fptr, int n_nodes,
                                const float* points, int dim, int n_faces, const int* verts, const int* rep,
                                const int* item_rowptr, const int* item, const double* elem, const double* strains,
                                const double* ut, double young, double poisson, int nodal, float* stress,
                                float* strain, double* sums, void* stream) {
  PDG_CHECK_ARG(n_graphs > 0 && n_graphs <= 65535 && n_cases > 0 && n_cases <= Q1_MAX_CASES &&
                    sizes_ok(n_nodes, n_faces) && (dim == 2 || dim == 3),
                "pdg_femq1_stress: bad sizes (0 < n_graphs < 2^16, 0 < n_cases <= 64, 0 < n_nodes, n_faces < 2^29, "
                "dim 2 or 3)");
  PDG_CHECK_ARG(ptr && fptr && points && verts && rep && item_rowptr && item && elem && strains && ut && stress &&
                    strain && sums,
                "pdg_femq1_stress: null argument");
  PDG_CHECK_ARG(material_ok(young, poisson), "pdg_femq1_stress: young must be finite and > 0, poisson in (-1, 0.5)");
  PDG_CHECK_ARG(nodal == 0 || nodal == 1, "pdg_femq1_stress: nodal is 0 (area weights) or 1 (counts)");
  hipLaunchKernelGGL(femq1_nodal_kernel, dim3((n_nodes + 255) / 256, n_cases), dim3(256), 0, (hipStream_t)stream,
                     n_graphs, n_cases, ptr, n_nodes, points, dim, n_faces, verts, rep, item_rowptr, item, elem,
                     strains, ut, young, poisson, nodal, stress, strain);
  hipLaunchKernelGGL(femq1_sums_kernel, dim3(n_graphs, n_cases), dim3(Q1_T), 0, (hipStream_t)stream, n_cases, ptr,
                     fptr, n_nodes, points, dim, n_faces, verts, elem, strains, ut, young, poisson, sums);
  PDG_CHECK_LAUNCH("pdg_femq1_stress");
  return PDG_OK;
}
