"""CPU checks of the Q1 hyperelastic restatement tests/hyperq1_ref.py, the reference of tests/test_gpu_hyperq1.py: the
assembled residual and tangent against central differences, the tangent positive definite at every state, the
linearisation against the linear Q1 restatement femq1_ref, and the convergence of every (mesh, load) the GPU tests
use.  The meshes are pdg.meshgen.quad_hole_plate(n, r, seed=3) with its default jitter: every pair converges."""
import numpy as np
import pytest

import femq1_ref
import hyper_ref as H
import hyperq1_ref as Q
from pdg import meshgen

EPS = np.finfo(np.float64).eps


def test_the_restatement_states_the_modules_constants():
    from gnn_local_stress import hyperelastic, hyperelastic_q1 as hq
    assert (Q.MU, Q.KAPPA) == (hq.MU, hq.KAPPA) == (hyperelastic.MU, hyperelastic.KAPPA)
    assert (Q.CONVERGED, Q.MAX_ITER, Q.BREAKDOWN) == (hq.CONVERGED, hq.MAX_ITER, hq.BREAKDOWN)
    assert (H.ARMIJO, H.HALVINGS, H.PHI_NOISE) == (hq.ARMIJO, hq.HALVINGS, hq.PHI_NOISE)
    assert hq.COLUMNS is hyperelastic.COLUMNS and hq.STATUS is hyperelastic.STATUS
    assert hq.HyperFields is hyperelastic.HyperFields and hq.HyperSolution is hyperelastic.HyperSolution
    assert hq.deformation_gradient is hyperelastic.deformation_gradient
    assert tuple(meshgen.quad_hole_plate(n, r, seed=3).num_nodes for n, r in Q.MESHES) == Q.NODES


@pytest.mark.parametrize("volumetric", ("log", "quadratic"))
def test_residual_and_tangent_are_the_derivatives_of_the_energy(volumetric):
    """Central differences in a representative's dof with step hx.  A term (face, Gauss point) sees F move along
    delta = (dN/dx, dN/dy) of the corner, |delta|_1 <= gm; hx = 1e-5 / gm keeps every |dF_ij| <= h = 1e-5, the step of
    the point-wise checks of tests/test_hyper_ref.py, whose bounds on the law's derivatives hold on the same set
    (|F_ij| < 2.2, J >= 0.7, asserted): every entry of W''' is < 1e4 and of P''' < 1e5, |W| and |P| < 1e2.
      residual:  |dPhi/dx_i + r_i| <= sum_terms w (hx^2 / 6) 1e4 |delta|_1^3 + rounding
                                   <= (h^2 / 6) 1e4 gm wmax + 16 EPS |Phi|_mag / hx,
      tangent:   |dr_j/dx_i + K_ij| <= (h^2 / 6) 1e5 gm^2 wmax + 16 EPS max f_abs / hx,
    wmax the largest sum of the weights of the terms a representative takes part in, |Phi|_mag and f_abs the sums of
    the magnitudes behind Phi and r (16: a pairwise sum's log2 n and the few roundings of a term)."""
    s = meshgen.quad_hole_plate(*Q.MESHES[0], seed=3)
    pb = Q.problem(s.pos, s.faces, volumetric=volumetric)
    Fb = Q.deformation_gradient(Q.LOADS[0])
    sol = Q.newton_direct(pb, Fb, n_steps=Q.N_STEPS)
    assert sol.status == Q.CONVERGED
    rng = np.random.default_rng(5)
    x = sol.ut[pb.c.reps].ravel()
    x = x + 0.05 * np.abs(x).max() * rng.standard_normal(len(x))       # off balance: r is not zero
    F = pb.point_F(Fb, x)
    assert np.abs(F).max() < 2.2 and np.linalg.det(F).min() >= 0.7
    gm = (np.abs(pb.G[:, :, 0, 0::2]) + np.abs(pb.G[:, :, 1, 0::2])).max()
    h = 1e-5
    hx = h / gm
    wnode = np.zeros(len(pb.c.pos))
    np.add.at(wnode, pb.c.rep[pb.c.faces].ravel(), np.repeat(pb.c.w.sum(1), 4))
    wmax = wnode.max()
    r, fabs_ = pb.residual(Fb, x)
    K = pb.tangent(Fb, x).toarray()
    mag = pb.energy(Fb, x)[1]
    bound_r = h * h / 6 * 1e4 * gm * wmax + 16 * EPS * mag / hx
    bound_k = h * h / 6 * 1e5 * gm * gm * wmax + 16 * EPS * fabs_.max() / hx
    worst_r = worst_k = 0.0
    for i in range(len(x)):
        dx = np.zeros(len(x))
        dx[i] = hx
        dphi = (pb.energy(Fb, x + dx)[0] - pb.energy(Fb, x - dx)[0]) / (2 * hx)
        dr = (pb.residual(Fb, x + dx)[0] - pb.residual(Fb, x - dx)[0]) / (2 * hx)
        worst_r = max(worst_r, abs(dphi + r[i]))
        worst_k = max(worst_k, np.abs(dr + K[:, i]).max())
    print(f"{volumetric}: |dPhi/dx + r| <= {worst_r:.2e} (bound {bound_r:.2e}, |r| up to {np.abs(r).max():.2e}), "
          f"|dr/dx + K| <= {worst_k:.2e} (bound {bound_k:.2e}, |K| up to {np.abs(K).max():.2e})")
    assert worst_r <= bound_r and worst_k <= bound_k
    assert bound_r <= 1e-4 * np.abs(r).max() and bound_k <= 1e-4 * np.abs(K).max()     # the bounds do test something
    assert np.abs(K - K.T).max() <= 1e-13 * np.abs(K).max()


def test_linearisation_is_the_linear_q1_cell_problem():
    """mu = 3, kappa = 4: lambda = kappa - 2 mu / 3 = 2, E = 7.2, nu = 0.2; plane strain is plane stress with
    E* = E / (1 - nu^2), nu* = nu / (1 - nu) = 0.25.  Under the logarithmic strain 1e-6 (1, -0.5, 0.8) the neglected
    terms are O(eps) ~ 1e-6 relative: 1e-4 leaves two decades for the geometry's constants."""
    mu, kappa = 3.0, 4.0
    lam = kappa - 2.0 * mu / 3.0
    young, nu = mu * (3 * lam + 2 * mu) / (lam + mu), lam / (2 * (lam + mu))
    s = meshgen.quad_hole_plate(*Q.MESHES[0], seed=3)
    lin = femq1_ref.cell(s.pos, s.faces, young / (1 - nu * nu), nu / (1 - nu))
    pb = Q.problem(s.pos, s.faces, mu=mu, kappa=kappa)
    eps = 1e-6 * np.array([1.0, -0.5, 0.8])
    want = femq1_ref.solve_direct(lin, eps)[0]
    # P carries a rounding error of ~ eps mu against forces of ~ mu * strain: rtol cannot go below ~ 1e-16 / strain
    sol = Q.newton_direct(pb, Q.deformation_gradient(eps), rtol=1e-8, n_steps=1)
    assert sol.status == Q.CONVERGED
    gap = np.abs(sol.ut - want).max() / np.abs(want).max()
    print(f"relative gap of ut to the linear Q1 solution: {gap:.3e}")
    assert gap <= 1e-4


@pytest.mark.parametrize("mesh", range(len(Q.MESHES)))
def test_every_gpu_load_converges_with_a_positive_definite_tangent(mesh):
    n, r = Q.MESHES[mesh]
    s = meshgen.quad_hole_plate(n, r, seed=3)
    for volumetric in ("log", "quadratic") if mesh == 0 else ("log",):
        pb = Q.problem(s.pos, s.faces, volumetric=volumetric)
        for eps in Q.LOADS:
            Fb = Q.deformation_gradient(eps)
            sol = Q.newton_direct(pb, Fb, n_steps=Q.N_STEPS, check_spd=True)
            print(f"n={n} {volumetric} {eps}: status {sol.status}, {sol.newton} Newton iterations, residual "
                  f"{sol.residual:.2e}, tangent positive definite at every state: {sol.spd}")
            assert sol.status == Q.CONVERGED and sol.steps == Q.N_STEPS and sol.residual <= 2e-10
            assert sol.spd
            assert np.abs(sol.ut[pb.c.reps].mean(0)).max() <= 1e-12 * np.abs(sol.ut).max()
            f = Q.fields(pb, Fb, sol.ut)
            hm = f.mean_pk1 @ Fb.T / np.linalg.det(Fb)                 # Hill-Mandel: <P> Fbar^T / det Fbar = <sigma>
            assert np.abs(np.array([hm[0, 0], hm[1, 1], hm[0, 1]]) - f.mean_stress).max() \
                <= 1e-9 * np.abs(f.mean_stress).max()


def test_the_step_for_step_restatement_agrees_with_the_direct_one():
    s = meshgen.quad_hole_plate(*Q.MESHES[0], seed=3)
    pb = Q.problem(s.pos, s.faces)
    Fb = Q.deformation_gradient(Q.LOADS[0])
    a = Q.newton_direct(pb, Fb, rtol=1e-12, n_steps=Q.N_STEPS)
    b = Q.newton_pcg(pb, Fb, n_steps=Q.N_STEPS)
    assert a.status == b.status == Q.CONVERGED and b.pcg > 0 and b.residual <= 2e-10
    assert np.abs(a.ut - b.ut).max() <= 1e-8 * np.abs(a.ut).max()
    assert Q.residual(pb, Fb, b.ut) == b.residual
    capped = Q.newton_pcg(pb, Fb, n_steps=Q.N_STEPS, max_newton=1)
    assert capped.status == Q.MAX_ITER and capped.steps == 0 and capped.newton == 1


def test_a_jittered_plate_without_a_hole_needs_no_iteration():
    """The 2 x 2 rule integrates grad N det J exactly on any convex quad: under a uniform P the exact residual is 0."""
    s = meshgen.quad_hole_plate(9, 0.0, seed=3)
    pb = Q.problem(s.pos, s.faces)
    assert np.ptp(pb.c.w) > 1e-3 * pb.c.w.mean()                       # jittered: the quads are not all alike
    Fb = Q.deformation_gradient(Q.LOADS[0])
    sol = Q.newton_pcg(pb, Fb, n_steps=Q.N_STEPS)
    assert sol.status == Q.CONVERGED and sol.newton == 0 and not sol.ut.any()
    f = Q.fields(pb, Fb, sol.ut)
    want = Q.cauchy(Fb)
    assert np.abs(f.stress - np.array([want[0, 0], want[1, 1], want[0, 1]])).max() <= 1e-13 * np.abs(want).max()
