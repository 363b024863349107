"""An independent fp64 restatement of the periodic elastic cell problem on bilinear (Q1) quads
(gnn_local_stress/fem_q1.py, csrc/pdg_femq1.hip), test-only: the stiffness of the 2 x 2 Gauss rule assembled with
scipy.sparse, the periodic reduction as a matrix, one node pinned and a direct solve; a conjugate-gradient solver with
the kernel's stopping rules; the nodal fields and the volume sums.  Nothing here shares code with the device path:
numpy, scipy and the mesh alone.  The material, the periodic map and the conventions are tests/fem_ref.py's
(``stiffness``, ``representatives``): u(x) = eps x + ut(x), (xx, yy, gamma_xy), dofs interleaved (2 v, 2 v + 1).

Reference corners (-1, -1), (1, -1), (1, 1), (-1, 1) in the face's own vertex order; Gauss point g is the corner g
scaled by 1 / sqrt(3), the one nearest that corner."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from fem_ref import (BREAKDOWN, CONVERGED, MAX_ITER, NOISE, POISSON, TRIVIAL, UNIT, YOUNG, representatives,  # noqa: F401
                     stiffness)

XI = np.array([-1.0, 1.0, 1.0, -1.0])
ETA = np.array([-1.0, -1.0, 1.0, 1.0])


@dataclass
class Cell:
    pos: np.ndarray        # (N, 2) fp64 of the float32 coordinates (plus the shift)
    faces: np.ndarray      # (F, 4)
    rep: np.ndarray        # (N,)
    reps: np.ndarray       # the representatives, ascending
    det: np.ndarray        # (F, 4) det J at the Gauss points
    w: np.ndarray          # (F, 4) |det J|: the weights
    B: np.ndarray          # (F, 4, 3, 8): strain (xx, yy, gamma_xy) at a Gauss point from the face's 8 displacements
    C: np.ndarray          # (3, 3)
    K: sp.csr_matrix       # (2 N, 2 N), the open mesh
    P: sp.csr_matrix       # (2 N, 2 R): node dofs from representative dofs
    A: sp.csr_matrix       # P^T K P

    @property
    def dofs(self) -> np.ndarray:
        """(F, 8) the global dofs of every face."""
        return (2 * self.faces[:, :, None] + np.arange(2)).reshape(-1, 8)


def cell(pos, faces, young: float = YOUNG, poisson: float = POISSON, shift=(0.0, 0.0)) -> Cell:
    """``shift`` translates the mesh in fp64, after the float32 coordinates are read (an exact rigid translation);
    the periodic map is taken from the unshifted coordinates."""
    p = np.asarray(pos, np.float32).astype(np.float64)[:, :2] + np.asarray(shift, np.float64)
    faces = np.asarray(faces, np.int64).reshape(-1, 4)
    n, nf = len(p), len(faces)
    gxi, geta = XI / np.sqrt(3.0), ETA / np.sqrt(3.0)
    # d[g, 0 / 1, k]: dN_k / dxi and dN_k / deta at Gauss point g
    d = np.stack([XI[None, :] * (1.0 + geta[:, None] * ETA[None, :]),
                  ETA[None, :] * (1.0 + gxi[:, None] * XI[None, :])], 1) / 4.0
    J = np.einsum("gak,fkc->fgac", d, p[faces])               # J[a, c] = d x_c / d xi_a
    det = np.linalg.det(J)
    if not (np.all(det > 0, 1) | np.all(det < 0, 1)).all():
        raise ValueError("a face is degenerate or not convex")
    grad = np.einsum("fgca,gak->fgck", np.linalg.inv(J), d)   # [dN/dx; dN/dy] = J^-1 [dN/dxi; dN/deta]
    B = np.zeros((nf, 4, 3, 8))
    B[:, :, 0, 0::2] = grad[:, :, 0]
    B[:, :, 1, 1::2] = grad[:, :, 1]
    B[:, :, 2, 0::2] = grad[:, :, 1]
    B[:, :, 2, 1::2] = grad[:, :, 0]
    C = stiffness(young, poisson)
    w = np.abs(det)
    Ke = np.einsum("fg,fgai,ab,fgbj->fij", w, B, C, B)
    dofs = (2 * faces[:, :, None] + np.arange(2)).reshape(-1, 8)
    K = sp.coo_matrix((Ke.ravel(), (np.repeat(dofs, 8, 1).ravel(), np.tile(dofs, (1, 8)).ravel())),
                      shape=(2 * n, 2 * n)).tocsr()
    rep = representatives(pos)
    reps = np.unique(rep)
    col = np.searchsorted(reps, rep)
    rows = np.arange(2 * n)
    P = sp.coo_matrix((np.ones(2 * n), (rows, 2 * col[rows // 2] + rows % 2)), shape=(2 * n, 2 * len(reps))).tocsr()
    return Cell(p, faces, rep, reps, det, w, B, C, K, P, (P.T @ K @ P).tocsr())


def affine(c: Cell, eps) -> np.ndarray:
    """(2 N,) eps x at every node."""
    exx, eyy, gxy = eps
    x, y = c.pos[:, 0], c.pos[:, 1]
    return np.stack([exx * x + 0.5 * gxy * y, 0.5 * gxy * x + eyy * y], 1).ravel()


def rhs(c: Cell, eps) -> tuple[np.ndarray, np.ndarray]:
    """b = -P^T K (eps x) and b_abs, the same sums of the absolute values of the faces' nodal forces (each the sum
    over the face's four Gauss points)."""
    ua = affine(c, eps)
    fe = np.einsum("fg,fgai,ab,fgb->fi", c.w, c.B, c.C, np.einsum("fgbj,fj->fgb", c.B, ua[c.dofs]))
    full, full_abs = np.zeros(len(ua)), np.zeros(len(ua))
    np.add.at(full, c.dofs.ravel(), -fe.ravel())
    np.add.at(full_abs, c.dofs.ravel(), np.abs(fe).ravel())
    return c.P.T @ full, c.P.T @ full_abs


def is_noise(b, b_abs) -> bool:
    return bool(np.linalg.norm(b) <= NOISE * np.linalg.norm(b_abs))


def expand(c: Cell, x: np.ndarray) -> np.ndarray:
    """(N, 2) the periodic field at every node from the representatives' values."""
    return (c.P @ x).reshape(-1, 2)


def solve_direct(c: Cell, eps) -> tuple[np.ndarray, int]:
    """(ut (N, 2) with zero mean over the representatives, status): one representative pinned, sparse LU."""
    b, b_abs = rhs(c, eps)
    if is_noise(b, b_abs):
        return np.zeros((len(c.pos), 2)), TRIVIAL
    x = np.zeros(len(b))
    x[2:] = spla.spsolve(c.A[2:, 2:].tocsc(), b[2:])
    x = (x.reshape(-1, 2) - x.reshape(-1, 2).mean(0)).ravel()
    return expand(c, x), CONVERGED


def pcg(c: Cell, eps, rtol: float = 1e-10, max_iter: int = 4000):
    """(ut (N, 2), iterations, status): Jacobi-preconditioned CG from 0 with the mean taken off z, the stopping rules
    of pdg_femq1_solve."""
    b, b_abs = rhs(c, eps)
    x = np.zeros(len(b))
    if is_noise(b, b_abs):
        return expand(c, x), 0, TRIVIAL
    dinv = 1.0 / c.A.diagonal()

    def precond(r):
        z = (dinv * r).reshape(-1, 2)
        return (z - z.mean(0)).ravel()

    bnorm = np.linalg.norm(b)
    r = b.copy()
    z = precond(r)
    p = z.copy()
    rz = r @ z
    it, status = 0, MAX_ITER
    while it < max_iter:
        Ap = c.A @ p
        pAp = p @ Ap
        if not (pAp > 0 and np.isfinite(pAp)):
            status = BREAKDOWN
            break
        alpha = rz / pAp
        x += alpha * p
        r -= alpha * Ap
        it += 1
        res = np.linalg.norm(r)
        if not np.isfinite(res):
            status = BREAKDOWN
            break
        if res <= rtol * bnorm:
            status = CONVERGED
            break
        z = precond(r)
        rz, rz0 = r @ z, rz
        p = z + (rz / rz0) * p
    x = (x.reshape(-1, 2) - x.reshape(-1, 2).mean(0)).ravel()
    return expand(c, x), it, status


def residual(c: Cell, eps, ut: np.ndarray) -> float:
    """|b - A x|_2 / |b|_2 with x the rows of ``ut`` (N, 2) at the representatives."""
    b, _ = rhs(c, eps)
    x = np.asarray(ut, np.float64)[c.reps].ravel()
    return float(np.linalg.norm(b - c.A @ x) / np.linalg.norm(b))


@dataclass
class Fields:
    gauss_strain: np.ndarray     # (F, 4, 3)
    gauss_stress: np.ndarray     # (F, 4, 3)
    stress: np.ndarray           # (N, 3) fp64 nodal
    strain: np.ndarray           # (N, 3)
    mean_stress: np.ndarray      # (3,) cell convention
    mean_stress_material: np.ndarray
    material_area: float
    cell_area: float


def fields(c: Cell, eps, ut: np.ndarray, nodal: str = "area") -> Fields:
    """A node's value: the average over its corners of the faces' values at the Gauss point nearest the corner
    (corner k of a face takes Gauss point k), weighted by that point's |det J| ("area") or 1 ("count")."""
    u = affine(c, eps) + np.asarray(ut, np.float64).ravel()
    ee = np.einsum("fgbj,fj->fgb", c.B, u[c.dofs])
    es = ee @ c.C.T
    w = c.w if nodal == "area" else np.ones_like(c.w)
    n = len(c.pos)
    den = np.zeros(n)
    np.add.at(den, c.faces.ravel(), w.ravel())
    ns, ne = np.zeros((n, 3)), np.zeros((n, 3))
    np.add.at(ns, c.faces.ravel(), (w[:, :, None] * es).reshape(-1, 3))
    np.add.at(ne, c.faces.ravel(), (w[:, :, None] * ee).reshape(-1, 3))
    p32 = np.asarray(c.pos, np.float32)
    cell_area = (float(p32[:, 0].max()) - float(p32[:, 0].min())) * (float(p32[:, 1].max()) - float(p32[:, 1].min()))
    tot = (c.w[:, :, None] * es).sum((0, 1))
    return Fields(ee, es, ns / den[:, None], ne / den[:, None], tot / cell_area, tot / c.w.sum(), float(c.w.sum()),
                  cell_area)


def effective_stiffness(c: Cell) -> np.ndarray:
    """(3, 3): column j the cell mean stress under the unit strain j, from direct solves."""
    return np.stack([fields(c, e, solve_direct(c, e)[0]).mean_stress for e in UNIT], 1)
