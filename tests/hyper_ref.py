"""An independent fp64 restatement of the periodic hyperelastic cell problem (gnn_local_stress/hyperelastic.py,
csrc/pdg_hyper.hip), test-only: the constitutive law in tensor form, the tangent assembled with scipy.sparse and
reduced with the periodic map of fem_ref.cell, Newton with a sparse direct solve, load stepping and the kernel's
backtracking rule; and ``newton_pcg``, which restates the kernel's inexact Newton step for step (the same inner
conjugate gradients, truncation and stopping rules) so that iteration counts can be compared.  numpy, scipy and the
mesh alone.

Plane strain, F3 = diag(F, 1), I1 = tr(F^T F) + 1, J = det F, W = mu / 2 (J^(-2/3) I1 - 3) + U(J) with
U = kappa (J ln J - J + 1) ("log") or kappa / 2 (J - 1)^2 ("quadratic").  u(X) = (Fbar - I) X + ut(X), ut periodic.
Degrees of freedom are interleaved (2 v, 2 v + 1); a 2 x 2 tensor is flattened row-major (00, 01, 10, 11)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import fem_ref

MU, KAPPA = 3.0, 10.0
# what the GPU tests solve: pdg.meshgen.hole_plate(n, r, seed=3) under these logarithmic strains (exx, eyy, gxy) from
# the reference's +-0.15 box, and one small load; tests/test_hyper_ref.py checks that each converges here
MESHES = ((9, 0.25), (13, 0.3), (37, 0.2))
LOADS = ((0.15, -0.10, 0.08), (-0.08, 0.12, -0.15), (1e-4, -5e-5, 8e-5))
N_STEPS = 4
CONVERGED, MAX_ITER, BREAKDOWN = 0, 2, 3
ARMIJO, HALVINGS = 1e-4, 10
PHI_NOISE = 32.0 * np.finfo(np.float64).eps
I2 = np.eye(2)


def deformation_gradient(strain) -> np.ndarray:
    """Fbar = exp(eps) of the logarithmic strain (exx, eyy, gxy)."""
    exx, eyy, gxy = strain
    return sla.expm(np.array([[exx, gxy / 2.0], [gxy / 2.0, eyy]]))


def _vol(J, kappa, volumetric):
    if volumetric == "log":
        return kappa * (J * np.log(J) - J + 1.0), kappa * np.log(J), kappa / J
    if volumetric == "quadratic":
        return 0.5 * kappa * (J - 1.0) ** 2, kappa * (J - 1.0), kappa * np.ones_like(J)
    raise ValueError(volumetric)


def energy(F, mu=MU, kappa=KAPPA, volumetric="log"):
    """W of F (..., 2, 2), and the magnitude of its terms before they cancel."""
    F = np.asarray(F, np.float64)
    J = np.linalg.det(F)
    iso = J ** (-2.0 / 3.0) * (np.einsum("...ij,...ij->...", F, F) + 1.0)
    U = _vol(J, kappa, volumetric)[0]
    mag = 0.5 * mu * (iso + 3.0) + kappa * (np.abs(J * np.log(J)) + J + 1.0)
    return 0.5 * mu * (iso - 3.0) + U, mag


def pk1(F, mu=MU, kappa=KAPPA, volumetric="log"):
    """P = mu J^(-2/3) (F - I1 / 3 F^-T) + U'(J) J F^-T of F (..., 2, 2)."""
    F = np.asarray(F, np.float64)
    J = np.linalg.det(F)[..., None, None]
    FiT = np.swapaxes(np.linalg.inv(F), -1, -2)
    I1 = (np.einsum("...ij,...ij->...", F, F) + 1.0)[..., None, None]
    return mu * J ** (-2.0 / 3.0) * (F - I1 / 3.0 * FiT) + _vol(J, kappa, volumetric)[1] * J * FiT


def tangent(F, mu=MU, kappa=KAPPA, volumetric="log"):
    """A = dP/dF (..., 2, 2, 2, 2) in tensor form, with d(J F^-T)_ij / dF_kl = (G_ij G_kl - G_il G_kj) / J."""
    F = np.asarray(F, np.float64)
    J = np.linalg.det(F)[..., None, None, None, None]
    G = J[..., 0, 0] * np.swapaxes(np.linalg.inv(F), -1, -2)
    I1 = (np.einsum("...ij,...ij->...", F, F) + 1.0)[..., None, None, None, None]
    _, up, upp = _vol(J, kappa, volumetric)
    a = mu * J ** (-2.0 / 3.0)
    c = up - mu * I1 * J ** (-5.0 / 3.0) / 3.0
    k1 = -2.0 * mu * J ** (-5.0 / 3.0) / 3.0
    k2 = 5.0 * mu * I1 * J ** (-8.0 / 3.0) / 9.0 + upp
    FG = np.einsum("...ij,...kl->...ijkl", F, G)
    GG = np.einsum("...ij,...kl->...ijkl", G, G)
    dG = (GG - np.einsum("...il,...kj->...ijkl", G, G)) / J
    return a * np.einsum("ik,jl->ijkl", I2, I2) + k1 * (FG + np.einsum("...ijkl->...klij", FG)) + k2 * GG + c * dG


def cauchy(F, **law):
    F = np.asarray(F, np.float64)
    return pk1(F, **law) @ np.swapaxes(F, -1, -2) / np.linalg.det(F)[..., None, None]


def log_strain(F):
    """1/2 ln(F F^T) of F (..., 2, 2), by the eigendecomposition."""
    F = np.asarray(F, np.float64)
    lam, vec = np.linalg.eigh(F @ np.swapaxes(F, -1, -2))
    return np.einsum("...ik,...k,...jk->...ij", vec, 0.5 * np.log(lam), vec)


@dataclass
class Problem:
    c: fem_ref.Cell
    G: np.ndarray          # (F, 4, 6): dF (00, 01, 10, 11) from the element's 6 displacements
    law: dict

    def element_F(self, Fbar, x):
        """(F, 2, 2) from the representatives' values x (2 R,)."""
        u = self.c.P @ x
        return (np.asarray(Fbar).reshape(4) + np.einsum("fab,fb->fa", self.G, u[self.c.dofs])).reshape(-1, 2, 2)

    def energy(self, Fbar, x):
        """(Phi, its magnitude, the elements with J <= 0 or a value that is not finite)."""
        F = self.element_F(Fbar, x)
        J = np.linalg.det(F)
        bad = ~(np.isfinite(F).all((1, 2)) & (J > 0))
        if bad.any():
            return np.nan, np.nan, int(bad.sum())
        W, mag = energy(F, **self.law)
        return float(self.c.area @ W), float(self.c.area @ mag), 0

    def residual(self, Fbar, x):
        """r = -P^T f_int and f_abs, the same sums of the absolute values of the elements' nodal forces."""
        P = pk1(self.element_F(Fbar, x), **self.law).reshape(-1, 4)
        fe = self.c.area[:, None] * np.einsum("fab,fa->fb", self.G, P)
        n2 = self.c.P.shape[0]
        full, full_abs = np.zeros(n2), np.zeros(n2)
        np.add.at(full, self.c.dofs.ravel(), -fe.ravel())
        np.add.at(full_abs, self.c.dofs.ravel(), np.abs(fe).ravel())
        return self.c.P.T @ full, self.c.P.T @ full_abs

    def tangent(self, Fbar, x) -> sp.csr_matrix:
        """P^T K_T P, K_T assembled from the elements' A."""
        A = tangent(self.element_F(Fbar, x), **self.law).reshape(-1, 4, 4)
        Ke = self.c.area[:, None, None] * np.einsum("fai,fab,fbj->fij", self.G, A, self.G)
        d, n2 = self.c.dofs, self.c.P.shape[0]
        K = sp.coo_matrix((Ke.ravel(), (np.repeat(d, 6, 1).ravel(), np.tile(d, (1, 6)).ravel())), shape=(n2, n2))
        return (self.c.P.T @ K.tocsr() @ self.c.P).tocsr()


def problem(pos, faces, mu=MU, kappa=KAPPA, volumetric="log") -> Problem:
    c = fem_ref.cell(pos, faces)
    gx, gy = c.B[:, 0, 0::2], c.B[:, 1, 1::2]
    G = np.zeros((len(c.faces), 4, 6))
    G[:, 0, 0::2] = gx
    G[:, 1, 0::2] = gy
    G[:, 2, 1::2] = gx
    G[:, 3, 1::2] = gy
    return Problem(c, G, dict(mu=mu, kappa=kappa, volumetric=volumetric))


def _backtrack(pb, Fb, x, d, phi, mag, rd, noise=PHI_NOISE):
    """(alpha, Phi, magnitude) of the first accepted step of alpha = 1, 1/2, .. 2^-10, or None.  ``noise`` is the
    allowance for the rounding of the two energy sums, as a fraction of their magnitude; 0 is the strict rule."""
    alpha = 1.0
    for _ in range(HALVINGS + 1):
        p1, m1, bad = pb.energy(Fb, x + alpha * d)
        if bad == 0 and p1 <= phi - ARMIJO * alpha * rd + noise * max(mag, m1):
            return alpha, p1, m1
        alpha *= 0.5
    return None


def _zero_mean(x):
    return (x.reshape(-1, 2) - x.reshape(-1, 2).mean(0)).ravel()


@dataclass
class Solve:
    ut: np.ndarray          # (N, 2), zero mean over the representatives
    status: int
    steps: int
    newton: int
    pcg: int
    residual: float         # |r|_2 / |f_abs|_2 at the returned ut under the whole load
    spd: bool               # the reduced tangent was positive definite at every state it was formed at (direct only)


def _finish(pb, Fbar, x, status, steps, newton, pcg, spd=True) -> Solve:
    x = _zero_mean(x)
    r, fa = pb.residual(Fbar, x)
    return Solve(fem_ref.expand(pb.c, x), status, steps, newton, pcg, float(np.linalg.norm(r) / np.linalg.norm(fa)), spd)


def _is_spd(A) -> bool:
    try:
        np.linalg.cholesky(A[2:, 2:].toarray())   # one representative pinned: the translations are out
        return True
    except np.linalg.LinAlgError:
        return False


def newton_direct(pb: Problem, Fbar, rtol=1e-10, n_steps=10, max_newton=25, check_spd=False, noise=PHI_NOISE,
                  accepted=None) -> Solve:
    """Load stepping, Newton with a sparse direct solve (one representative pinned) and the backtracking rule.  With
    ``check_spd`` every tangent is also factorised by Cholesky (dense) and ``spd`` records whether all succeeded.  ``accepted``, a list, receives every accepted step as
    (Fb, x, d, alpha, r . d)."""
    Fbar = np.asarray(Fbar, np.float64).reshape(2, 2)
    x = np.zeros(pb.c.P.shape[1])
    newton, spd = 0, True
    for step in range(1, n_steps + 1):
        t = step / n_steps
        Fb = t * Fbar + (1.0 - t) * I2
        phi, mag, bad = pb.energy(Fb, x)
        if bad:
            return _finish(pb, Fbar, x, BREAKDOWN, step - 1, newton, 0, spd)
        it = 0
        while True:
            r, fa = pb.residual(Fb, x)
            if np.linalg.norm(r) <= rtol * np.linalg.norm(fa):
                break
            if it >= max_newton:
                return _finish(pb, Fbar, x, MAX_ITER, step - 1, newton, 0, spd)
            A = pb.tangent(Fb, x)
            spd = spd and (not check_spd or _is_spd(A))
            d = np.zeros(len(x))
            d[2:] = spla.spsolve(A[2:, 2:].tocsc(), r[2:])
            d = _zero_mean(d)
            got = _backtrack(pb, Fb, x, d, phi, mag, float(r @ d), noise)
            if got is None:
                return _finish(pb, Fbar, x, BREAKDOWN, step - 1, newton, 0, spd)
            alpha, phi, mag = got
            if accepted is not None:
                accepted.append((Fb, x, d, alpha, float(r @ d)))
            x = x + alpha * d
            it += 1
            newton += 1
    return _finish(pb, Fbar, x, CONVERGED, n_steps, newton, 0, spd)


def _pcg(A, r0, eta, max_pcg):
    """(d, iterations): pdg_hyper_solve's inner solve."""
    diag = np.abs(A.diagonal())
    dinv = np.where((diag > 0) & np.isfinite(diag), 1.0 / np.where(diag > 0, diag, 1.0), 1.0)

    def precond(r):
        z = (dinv * r).reshape(-1, 2)
        return (z - z.mean(0)).ravel()

    d = np.zeros(len(r0))
    r = r0.copy()
    p = precond(r)
    rz = r @ p
    tol = eta * np.linalg.norm(r0)
    k = 0
    while k < max_pcg and not np.linalg.norm(r) <= tol:
        Ap = A @ p
        pAp = p @ Ap
        if not pAp > 0:
            return (p.copy() if k == 0 else d), k
        alpha = rz / pAp
        d += alpha * p
        r -= alpha * Ap
        k += 1
        z = precond(r)
        rz, rz0 = r @ z, rz
        p = z + (rz / rz0) * p
    return d, k


def newton_pcg(pb: Problem, Fbar, rtol=1e-10, n_steps=10, max_newton=25, eta=1e-4, max_pcg=4000) -> Solve:
    """pdg_hyper_solve step for step: the inexact Newton iteration with the kernel's inner conjugate gradients."""
    Fbar = np.asarray(Fbar, np.float64).reshape(2, 2)
    x = np.zeros(pb.c.P.shape[1])
    newton = pcg = 0
    for step in range(1, n_steps + 1):
        t = step / n_steps
        Fb = t * Fbar + (1.0 - t) * I2
        phi, mag, bad = pb.energy(Fb, x)
        if bad:
            return _finish(pb, Fbar, x, BREAKDOWN, step - 1, newton, pcg)
        it = 0
        while True:
            r, fa = pb.residual(Fb, x)
            if np.linalg.norm(r) <= rtol * np.linalg.norm(fa):
                break
            if it >= max_newton:
                return _finish(pb, Fbar, x, MAX_ITER, step - 1, newton, pcg)
            d, k = _pcg(pb.tangent(Fb, x), r, eta, max_pcg)
            pcg += k
            got = _backtrack(pb, Fb, x, d, phi, mag, float(r @ d))
            if got is None:
                return _finish(pb, Fbar, x, BREAKDOWN, step - 1, newton, pcg)
            alpha, phi, mag = got
            x = x + alpha * d
            it += 1
            newton += 1
    return _finish(pb, Fbar, x, CONVERGED, n_steps, newton, pcg)


def residual(pb: Problem, Fbar, ut) -> float:
    """|r|_2 / |f_abs|_2 with x the rows of ``ut`` (N, 2) at the representatives."""
    x = np.asarray(ut, np.float64)[pb.c.reps].ravel()
    r, fa = pb.residual(np.asarray(Fbar, np.float64).reshape(2, 2), x)
    return float(np.linalg.norm(r) / np.linalg.norm(fa))


@dataclass
class Fields:
    F: np.ndarray                # (F, 2, 2) per element
    stress: np.ndarray           # (N, 3) fp64 nodal Cauchy (xx, yy, xy)
    log_strain: np.ndarray       # (N, 3) nodal (xx, yy, 2 xy)
    mean_stress: np.ndarray      # (3,) over the deformed cell
    mean_stress_material: np.ndarray
    mean_pk1: np.ndarray         # (2, 2) over the undeformed cell
    material_area: float
    cell_area: float


def fields(pb: Problem, Fbar, ut, nodal: str = "area") -> Fields:
    Fbar = np.asarray(Fbar, np.float64).reshape(2, 2)
    c = pb.c
    u = np.asarray(ut, np.float64).ravel()
    F = (Fbar.reshape(4) + np.einsum("fab,fb->fa", pb.G, u[c.dofs])).reshape(-1, 2, 2)
    J = np.linalg.det(F)
    P = pk1(F, **pb.law)
    sg = P @ np.swapaxes(F, 1, 2) / J[:, None, None]
    le = log_strain(F)
    es = np.stack([sg[:, 0, 0], sg[:, 1, 1], sg[:, 0, 1]], 1)
    ee = np.stack([le[:, 0, 0], le[:, 1, 1], 2.0 * le[:, 0, 1]], 1)
    w = c.area * J if nodal == "area" else np.ones(len(c.area))
    n = len(c.pos)
    den = np.zeros(n)
    np.add.at(den, c.faces.ravel(), np.repeat(w, 3))
    ns, ne = np.zeros((n, 3)), np.zeros((n, 3))
    np.add.at(ns, c.faces.ravel(), np.repeat(w[:, None] * es, 3, 0))
    np.add.at(ne, c.faces.ravel(), np.repeat(w[:, None] * ee, 3, 0))
    p32 = c.pos.astype(np.float32)
    cell_area = (float(p32[:, 0].max()) - float(p32[:, 0].min())) * (float(p32[:, 1].max()) - float(p32[:, 1].min()))
    tot = ((c.area * J)[:, None] * es).sum(0)
    return Fields(F, ns / den[:, None], ne / den[:, None], tot / (np.linalg.det(Fbar) * cell_area),
                  tot / float(c.area @ J), (c.area[:, None, None] * P).sum(0) / cell_area, float(c.area.sum()),
                  cell_area)
