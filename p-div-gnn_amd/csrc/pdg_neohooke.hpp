// The compressible neo-Hookean law in plane strain at one point, shared by the hyperelastic cell solvers on P1
// triangles (pdg_hyper.hip, one point a face) and on Q1 quads (pdg_hyperq1.hip, one point a Gauss point):
//
//   F3 = diag(F, 1),   W = mu / 2 (J^(-2/3) I1 - 3) + U(J),   I1 = tr(F^T F) + 1,   J = det F,
//   P = dW/dF = a F + c G,   a = mu J^(-2/3),  c = U'(J) - mu I1 J^(-5/3) / 3,  G = dJ/dF = J F^-T,
//   A = dP/dF = a I + k1 (F G^T + G F^T) + k2 G G^T + c dG/dF,   k1 = -2 mu J^(-5/3) / 3,
//                                                                k2 = 5 mu I1 J^(-8/3) / 9 + U''(J),
//
// on the 4-vector (F00, F01, F10, F11); A is symmetric, 10 values.  Every expression is evaluated as written.
#pragma once
#include <math.h>

#pragma clang fp contract(off)

namespace pdg {
namespace neohooke {

struct Law {
  double mu, kappa;
  int vol;   // 0: U = kappa (J ln J - J + 1), 1: U = kappa / 2 (J - 1)^2
};

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

// 0 a sound point, 1 an inverted one (J <= 0), 2 a value that is not finite.
__device__ __forceinline__ int face_state(const double (&F)[4], double J) {
  if (!(trace1(F) < INFINITY) || !(J < INFINITY) || !(J > -INFINITY)) return 2;
  return J > 0.0 ? 0 : 1;
}

__device__ __forceinline__ double inverse_diag(double d) {   // > 0 for every active row, whatever the tangent
  const double a = fabs(d);
  return a > 0.0 && a < INFINITY ? 1.0 / a : 1.0;
}

// J sigma = P F^T as xx, yy, xy.
__device__ __forceinline__ void kirchhoff(const double (&F)[4], const double (&P)[4], double (&sg)[3]) {
  sg[0] = P[0] * F[0] + P[1] * F[1];
  sg[1] = P[2] * F[2] + P[3] * F[3];
  sg[2] = P[0] * F[2] + P[1] * F[3];
}

// 1/2 ln(F F^T) as xx, yy, 2 xy.
__device__ __forceinline__ void log_strain(const double (&F)[4], double (&le)[3]) {
  // ln B of the symmetric B = F F^T = m I + (B - m I), whose second term has the eigenvalues +-delta:
  // ln B = (ln l1 + ln l2) / 2 I + (ln l1 - ln l2) / (2 delta) (B - m I), and the factor -> 1 / m as delta -> 0
  const double b00 = F[0] * F[0] + F[1] * F[1], b11 = F[2] * F[2] + F[3] * F[3], b01 = F[0] * F[2] + F[1] * F[3];
  const double m = 0.5 * (b00 + b11), h = 0.5 * (b00 - b11);
  const double delta = sqrt(h * h + b01 * b01);
  const double l2 = m - delta;
  const double half_sum = 0.5 * log((m + delta) * l2);            // ln l1 + ln l2 = ln det B
  const double slope = delta > 0.0 ? log1p(2.0 * delta / l2) / (2.0 * delta) : 1.0 / m;
  le[0] = 0.5 * (half_sum + slope * h);
  le[1] = 0.5 * (half_sum - slope * h);
  le[2] = slope * b01;                                           // 2 * (1/2 ln B)_xy
}

}  // namespace neohooke
}  // namespace pdg
