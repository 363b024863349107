"""An independent fp64 restatement of the periodic hyperelastic cell problem on bilinear (Q1) quads
(gnn_local_stress/hyperelastic_q1.py, csrc/pdg_hyperq1.hip), test-only: the law of tests/hyper_ref.py (``energy``,
``pk1``, ``tangent``, ``cauchy``, ``log_strain``, in tensor form) evaluated at the four Gauss points of every face of
tests/femq1_ref.py's cell (its shape gradients, weights and periodic reduction), the residual and the tangent
assembled with scipy.sparse and reduced with the periodic map.  The solvers are hyper_ref's own, which ask a problem
for ``energy``, ``residual`` and ``tangent`` only: ``newton_direct`` (load stepping, one representative pinned, sparse
LU, the kernel's backtracking rule) and ``newton_pcg`` (the kernel's inexact Newton iteration step for step, for
iteration counts).  numpy, scipy and the mesh alone.

F_g = Fbar + sum_k ut_k (x) grad N_k(g), weight w_g = |det J_g|, Phi = sum_f sum_g w_g W(F_g).  Degrees of freedom are
interleaved (2 v, 2 v + 1); a 2 x 2 tensor is flattened row-major (00, 01, 10, 11).  Gauss point g is the one nearest
corner g of the face's own vertex order (femq1_ref)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

import femq1_ref
import hyper_ref as H
from hyper_ref import (BREAKDOWN, CONVERGED, KAPPA, LOADS, MAX_ITER, MU, N_STEPS, Solve, cauchy,  # noqa: F401
                       deformation_gradient, energy, log_strain, pk1, tangent)

# what the GPU tests solve: pdg.meshgen.quad_hole_plate(n, r, seed=3) under hyper_ref.LOADS in hyper_ref.N_STEPS steps
MESHES = ((9, 0.25), (13, 0.3), (37, 0.2))
NODES = (72, 132, 1208)


@dataclass
class Problem:
    c: femq1_ref.Cell
    G: np.ndarray          # (F, 4, 4, 8): dF (00, 01, 10, 11) at Gauss point g from the face's 8 displacements
    law: dict

    def point_F(self, Fbar, x):
        """(F, 4, 2, 2) at the Gauss points from the representatives' values x (2 R,)."""
        u = self.c.P @ x
        dF = np.einsum("fgab,fb->fga", self.G, u[self.c.dofs])
        return (np.asarray(Fbar).reshape(4) + dF).reshape(-1, 4, 2, 2)

    def energy(self, Fbar, x):
        """(Phi, its magnitude, the faces with a Gauss point of J <= 0 or of a value that is not finite)."""
        F = self.point_F(Fbar, x)
        J = np.linalg.det(F)
        bad = ~(np.isfinite(F).all((2, 3)) & (J > 0)).all(1)
        if bad.any():
            return np.nan, np.nan, int(bad.sum())
        W, mag = energy(F, **self.law)
        return float((self.c.w * W).sum()), float((self.c.w * mag).sum()), 0

    def residual(self, Fbar, x):
        """r = -P^T f_int and f_abs, the same sums of the absolute values of every (corner, Gauss point) term."""
        P = pk1(self.point_F(Fbar, x), **self.law).reshape(-1, 4, 4)
        fe = self.c.w[:, :, None] * np.einsum("fgab,fga->fgb", self.G, P)        # (F, g, 8)
        n2 = self.c.P.shape[0]
        full, full_abs = np.zeros(n2), np.zeros(n2)
        np.add.at(full, self.c.dofs.ravel(), -fe.sum(1).ravel())
        np.add.at(full_abs, self.c.dofs.ravel(), np.abs(fe).sum(1).ravel())
        return self.c.P.T @ full, self.c.P.T @ full_abs

    def tangent(self, Fbar, x) -> sp.csr_matrix:
        """P^T K_T P, K_T assembled from the Gauss points' A."""
        A = tangent(self.point_F(Fbar, x), **self.law).reshape(-1, 4, 4, 4)
        Ke = np.einsum("fg,fgai,fgab,fgbj->fij", self.c.w, self.G, A, self.G)
        d, n2 = self.c.dofs, self.c.P.shape[0]
        K = sp.coo_matrix((Ke.ravel(), (np.repeat(d, 8, 1).ravel(), np.tile(d, (1, 8)).ravel())), shape=(n2, n2))
        return (self.c.P.T @ K.tocsr() @ self.c.P).tocsr()


def problem(pos, faces, mu=MU, kappa=KAPPA, volumetric="log") -> Problem:
    c = femq1_ref.cell(pos, faces)
    gx, gy = c.B[:, :, 0, 0::2], c.B[:, :, 1, 1::2]          # (F, g, k)
    G = np.zeros((len(c.faces), 4, 4, 8))
    G[:, :, 0, 0::2] = gx
    G[:, :, 1, 0::2] = gy
    G[:, :, 2, 1::2] = gx
    G[:, :, 3, 1::2] = gy
    return Problem(c, G, dict(mu=mu, kappa=kappa, volumetric=volumetric))


def newton_direct(pb: Problem, Fbar, **kw) -> Solve:
    """hyper_ref.newton_direct on the Gauss-point problem: load stepping, Newton with a sparse direct solve (one
    representative pinned) and the backtracking rule."""
    return H.newton_direct(pb, Fbar, **kw)


def newton_pcg(pb: Problem, Fbar, **kw) -> Solve:
    """hyper_ref.newton_pcg on the Gauss-point problem: pdg_hyperq1_solve step for step."""
    return H.newton_pcg(pb, Fbar, **kw)


def residual(pb: Problem, Fbar, ut) -> float:
    """|r|_2 / |f_abs|_2 with x the rows of ``ut`` (N, 2) at the representatives."""
    x = np.asarray(ut, np.float64)[pb.c.reps].ravel()
    r, fa = pb.residual(np.asarray(Fbar, np.float64).reshape(2, 2), x)
    return float(np.linalg.norm(r) / np.linalg.norm(fa))


@dataclass
class Fields:
    F: np.ndarray                # (F, 4, 2, 2) per Gauss point
    stress: np.ndarray           # (N, 3) fp64 nodal Cauchy (xx, yy, xy)
    log_strain: np.ndarray       # (N, 3) nodal (xx, yy, 2 xy)
    mean_stress: np.ndarray      # (3,) over the deformed cell
    mean_stress_material: np.ndarray
    mean_pk1: np.ndarray         # (2, 2) over the undeformed cell
    material_area: float
    cell_area: float


def fields(pb: Problem, Fbar, ut, nodal: str = "area") -> Fields:
    """A node's value: the average over its own corners of the faces' values at the Gauss point nearest the corner
    (corner k of a face takes Gauss point k), weighted by that point's deformed weight w_g J_g ("area") or 1
    ("count")."""
    Fbar = np.asarray(Fbar, np.float64).reshape(2, 2)
    c = pb.c
    u = np.asarray(ut, np.float64).ravel()
    F = (Fbar.reshape(4) + np.einsum("fgab,fb->fga", pb.G, u[c.dofs])).reshape(-1, 4, 2, 2)
    J = np.linalg.det(F)
    P = pk1(F, **pb.law)
    sg = P @ np.swapaxes(F, -1, -2) / J[..., None, None]
    le = log_strain(F)
    es = np.stack([sg[..., 0, 0], sg[..., 1, 1], sg[..., 0, 1]], -1)          # (F, g, 3)
    ee = np.stack([le[..., 0, 0], le[..., 1, 1], 2.0 * le[..., 0, 1]], -1)
    w = c.w * J if nodal == "area" else np.ones_like(c.w)
    n = len(c.pos)
    den = np.zeros(n)
    np.add.at(den, c.faces.ravel(), w.ravel())
    ns, ne = np.zeros((n, 3)), np.zeros((n, 3))
    np.add.at(ns, c.faces.ravel(), (w[:, :, None] * es).reshape(-1, 3))
    np.add.at(ne, c.faces.ravel(), (w[:, :, None] * ee).reshape(-1, 3))
    p32 = np.asarray(c.pos, np.float32)
    cell_area = (float(p32[:, 0].max()) - float(p32[:, 0].min())) * (float(p32[:, 1].max()) - float(p32[:, 1].min()))
    tot = ((c.w * J)[:, :, None] * es).sum((0, 1))
    return Fields(F, ns / den[:, None], ne / den[:, None], tot / (np.linalg.det(Fbar) * cell_area),
                  tot / float((c.w * J).sum()), (c.w[:, :, None, None] * P).sum((0, 1)) / cell_area,
                  float(c.w.sum()), cell_area)
