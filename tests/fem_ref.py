"""An independent fp64 restatement of the periodic elastic cell problem (gnn_local_stress/fem.py,
csrc/pdg_fem.hip), test-only: the stiffness assembled with scipy.sparse, the periodic reduction as a matrix, one node
pinned and a direct solve; and a conjugate-gradient solver with the kernel's stopping rules.  Nothing here shares code
with the device path: numpy, scipy and the mesh alone.

Plane stress, C = E / (1 - nu^2) [[1, nu, 0], [nu, 1, 0], [0, 0, (1 - nu) / 2]] on (xx, yy, gamma_xy),
u(x) = eps x + ut(x), eps = [[exx, gxy / 2], [gxy / 2, eyy]], ut periodic.  Degrees of freedom are interleaved
(2 v, 2 v + 1)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

YOUNG, POISSON = 1e5, 0.3
NOISE = 1e-12
CONVERGED, TRIVIAL, MAX_ITER, BREAKDOWN = 0, 1, 2, 3
UNIT = np.eye(3)


def stiffness(young: float = YOUNG, poisson: float = POISSON) -> np.ndarray:
    c = young / (1.0 - poisson ** 2)
    return np.array([[c, poisson * c, 0.0], [poisson * c, c, 0.0], [0.0, 0.0, c * (1.0 - poisson) / 2.0]])


def representatives(pos: np.ndarray) -> np.ndarray:
    """rep (N,): x == xmax -> the node with x == xmin at the same y, y == ymax -> the node with y == ymin at the same
    x, composed; exact float32 equality.  ValueError("mesh is not periodic") when the sides do not match."""
    p = np.asarray(pos, np.float32)
    n = len(p)

    def side(along, across):
        lo, hi = along.min(), along.max()
        src, dst = np.where(along == hi)[0], np.where(along == lo)[0]
        if len(src) != len(dst) or lo == hi:
            raise ValueError("mesh is not periodic")
        src, dst = src[np.argsort(across[src], kind="stable")], dst[np.argsort(across[dst], kind="stable")]
        if not np.array_equal(across[src], across[dst]):
            raise ValueError("mesh is not periodic")
        m = np.arange(n)
        m[src] = dst
        return m

    return side(p[:, 1], p[:, 0])[side(p[:, 0], p[:, 1])]


@dataclass
class Cell:
    pos: np.ndarray        # (N, 2) fp64 of the float32 coordinates
    faces: np.ndarray      # (F, 3)
    rep: np.ndarray        # (N,)
    reps: np.ndarray       # the representatives, ascending
    area: np.ndarray       # (F,)
    B: np.ndarray          # (F, 3, 6): strain (xx, yy, gamma_xy) from the element's 6 displacements
    C: np.ndarray          # (3, 3)
    K: sp.csr_matrix       # (2 N, 2 N), the open mesh
    P: sp.csr_matrix       # (2 N, 2 R): node dofs from representative dofs
    A: sp.csr_matrix       # P^T K P

    @property
    def dofs(self) -> np.ndarray:
        """(F, 6) the global dofs of every element."""
        return (2 * self.faces[:, :, None] + np.arange(2)).reshape(-1, 6)


def cell(pos, faces, young: float = YOUNG, poisson: float = POISSON) -> Cell:
    p = np.asarray(pos, np.float32).astype(np.float64)[:, :2]
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    n = len(p)
    (xa, ya), (xb, yb), (xc, yc) = (p[faces[:, k]].T for k in range(3))
    det = (xb - xa) * (yc - ya) - (xc - xa) * (yb - ya)
    if np.any(det == 0):
        raise ValueError("a face has zero area")
    area = 0.5 * np.abs(det)
    gx = np.stack([yb - yc, yc - ya, ya - yb], 1) / det[:, None]
    gy = np.stack([xc - xb, xa - xc, xb - xa], 1) / det[:, None]
    B = np.zeros((len(faces), 3, 6))
    B[:, 0, 0::2] = gx
    B[:, 1, 1::2] = gy
    B[:, 2, 0::2] = gy
    B[:, 2, 1::2] = gx
    C = stiffness(young, poisson)
    Ke = area[:, None, None] * np.einsum("fai,ab,fbj->fij", B, C, B)
    dofs = (2 * faces[:, :, None] + np.arange(2)).reshape(-1, 6)
    K = sp.coo_matrix((Ke.ravel(), (np.repeat(dofs, 6, 1).ravel(), np.tile(dofs, (1, 6)).ravel())),
                      shape=(2 * n, 2 * n)).tocsr()
    rep = representatives(pos)
    reps = np.unique(rep)
    col = np.searchsorted(reps, rep)
    rows = np.arange(2 * n)
    P = sp.coo_matrix((np.ones(2 * n), (rows, 2 * col[rows // 2] + rows % 2)), shape=(2 * n, 2 * len(reps))).tocsr()
    return Cell(p, faces, rep, reps, area, B, C, K, P, (P.T @ K @ P).tocsr())


def affine(c: Cell, eps) -> np.ndarray:
    """(2 N,) eps x at every node."""
    exx, eyy, gxy = eps
    x, y = c.pos[:, 0], c.pos[:, 1]
    return np.stack([exx * x + 0.5 * gxy * y, 0.5 * gxy * x + eyy * y], 1).ravel()


def rhs(c: Cell, eps) -> tuple[np.ndarray, np.ndarray]:
    """b = -P^T K (eps x) and b_abs, the same sums of the absolute values of the elements' nodal forces."""
    ua = affine(c, eps)
    fe = c.area[:, None] * np.einsum("fai,ab,fb->fi", c.B, c.C, np.einsum("fbj,fj->fb", c.B, ua[c.dofs]))
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
    of pdg_fem_solve."""
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
    elem_strain: np.ndarray      # (F, 3)
    elem_stress: np.ndarray      # (F, 3)
    stress: np.ndarray           # (N, 3) fp64 nodal
    strain: np.ndarray           # (N, 3)
    mean_stress: np.ndarray      # (3,) cell convention
    mean_stress_material: np.ndarray
    material_area: float
    cell_area: float


def fields(c: Cell, eps, ut: np.ndarray, nodal: str = "area") -> Fields:
    u = affine(c, eps) + np.asarray(ut, np.float64).ravel()
    ee = np.einsum("fbj,fj->fb", c.B, u[c.dofs])
    es = ee @ c.C.T
    w = c.area if nodal == "area" else np.ones(len(c.area))
    n = len(c.pos)
    den = np.zeros(n)
    np.add.at(den, c.faces.ravel(), np.repeat(w, 3))
    ns, ne = np.zeros((n, 3)), np.zeros((n, 3))
    np.add.at(ns, c.faces.ravel(), np.repeat(w[:, None] * es, 3, 0))
    np.add.at(ne, c.faces.ravel(), np.repeat(w[:, None] * ee, 3, 0))
    p32 = c.pos.astype(np.float32)
    cell_area = (float(p32[:, 0].max()) - float(p32[:, 0].min())) * (float(p32[:, 1].max()) - float(p32[:, 1].min()))
    tot = (c.area[:, None] * es).sum(0)
    return Fields(ee, es, ns / den[:, None], ne / den[:, None], tot / cell_area, tot / c.area.sum(),
                  float(c.area.sum()), cell_area)


def effective_stiffness(c: Cell) -> np.ndarray:
    """(3, 3): column j the cell mean stress under the unit strain j, from direct solves."""
    return np.stack([fields(c, e, solve_direct(c, e)[0]).mean_stress for e in UNIT], 1)
