// Per-node pieces of the boundary terms of a plane-stress field, shared by the diagnostics (pdg_boundary.hip) and
// the training penalties (pdg_physloss.hip): a symmetric 2 x 2 row, the nodal boundary force, the traction term's
// gradient and the rule that says which edges are a node's periodic connections.  Every formula is compiled
// without contraction into fused multiply-adds, so the forward, the backward and the host restatements form the
// same fp64 values.
#pragma once
#include <hip/hip_runtime.h>

namespace pdg {

struct Sym3 {
  double x, y, xy;   // (xx, yy, xy)
};

__device__ __forceinline__ Sym3 load_row(const float* __restrict__ sig, int i) {
  return Sym3{(double)sig[(size_t)i * 3], (double)sig[(size_t)i * 3 + 1], (double)sig[(size_t)i * 3 + 2]};
}

// f = sigma . m: fx = sxx mx + sxy my, fy = sxy mx + syy my (the products of two fp32 values are exact in fp64).
__device__ __forceinline__ void force(const Sym3& s, double mx, double my, double& fx, double& fy) {
#pragma clang fp contract(off)
  fx = s.x * mx + s.xy * my;
  fy = s.xy * mx + s.y * my;
}

// The periodic connections of node i in the graph [n0, n1): its incoming edges k in [rowptr[i], rowptr[i + 1]) (CSR
// by destination, edge k's attribute at perm[k]) of length exactly 0, eattr[perm[k]] == 0, whose source j = src[k]
// lies in [n0, n1).  An edge never leaves its graph; one that does is not read.  The four loops over them (two in
// each of the two files) are written out: a shared walker, with a callback or as a per-edge predicate, changed all
// four kernels' code (EXPERIMENTS.md section 11).  They must stay equal to this rule.

// o = ct * d(|a . m|^2 / bl) / da: the gradient of a traction node's term with respect to its row.
__device__ __forceinline__ void traction_grad(const Sym3& a, double mx, double my, float bl, double ct,
                                              double (&o)[3]) {
#pragma clang fp contract(off)
  double fx, fy;
  force(a, mx, my, fx, fy);
  const double c = 2.0 / (double)bl;
  o[0] = ct * (c * (fx * mx));
  o[1] = ct * (c * (fy * my));
  o[2] = ct * (c * (fx * my + fy * mx));
}

}  // namespace pdg
