// What the per-graph FEM solvers (pdg_fem.hip, pdg_hyper.hip) read of a batch of periodic P1 meshes, and the two
// helpers that walk a representative's item row with every index checked before it addresses anything.  The layout
// is gnn_local_stress.fem.FemPlan's (include/pdivgnn.h, "FEM targets").
#pragma once
#include "pdg_common.hpp"

namespace pdg {

struct Mesh {
  const float* points;
  int dim;
  int n_nodes, n_faces;
  const int* verts;    // (3 F) node of every corner
  const int* rverts;   // (3 F) its periodic representative
  const int* rep;      // (N)
  const int* rowptr;   // (N + 1) items of a representative: the corners that are it or an image of it
  const int* item;     // (3 F) 3 face + corner
  const double* elem;  // (F, 8)
  int n0, n1;          // the graph's node segment
};

// The first and one past the last item of row v, clamped to the item array.
__device__ __forceinline__ void row_range(const Mesh& m, int v, int& j0, int& j1) {
  j0 = m.rowptr[v];
  j1 = m.rowptr[v + 1];
  if (j0 < 0) j0 = 0;
  if (j1 > 3 * m.n_faces) j1 = 3 * m.n_faces;
}

// The face and corner of item j; false for an item outside the mesh (it is skipped before anything is addressed).
__device__ __forceinline__ bool item_of(const Mesh& m, int j, int& f, int& c) {
  const unsigned it = (unsigned)m.item[j];
  if (it >= 3u * (unsigned)m.n_faces) return false;
  f = (int)(it / 3u);
  c = (int)(it - 3u * (unsigned)f);
  return true;
}

// The same two for a mesh of quads (pdg_femq1.hip): verts, rverts and item hold 4 F entries, an item is
// 4 face + corner, elem is (F, 36).
__device__ __forceinline__ void row_range4(const Mesh& m, int v, int& j0, int& j1) {
  j0 = m.rowptr[v];
  j1 = m.rowptr[v + 1];
  if (j0 < 0) j0 = 0;
  if (j1 > 4 * m.n_faces) j1 = 4 * m.n_faces;
}

__device__ __forceinline__ bool item_of4(const Mesh& m, int j, int& f, int& c) {
  const unsigned it = (unsigned)m.item[j];
  if (it >= 4u * (unsigned)m.n_faces) return false;
  f = (int)(it >> 2);
  c = (int)(it & 3u);
  return true;
}

}  // namespace pdg
