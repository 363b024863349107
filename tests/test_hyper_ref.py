"""CPU checks of the hyperelastic restatement tests/hyper_ref.py, the reference of tests/test_gpu_hyper.py: the
constitutive law against central differences, its linearisation against the linear restatement fem_ref, the
Hill-Mandel identity at a converged solution, and the convergence of every load the GPU tests use."""
import numpy as np
import pytest

import fem_ref
import hyper_ref as H
from gnn_local_stress import hyperelastic
from pdg import meshgen

EPS = np.finfo(np.float64).eps


def test_the_restatement_states_the_modules_constants():
    """What the restatement solves by is what gnn_local_stress.hyperelastic documents and passes to the kernel."""
    assert (H.MU, H.KAPPA) == (hyperelastic.MU, hyperelastic.KAPPA)
    assert (H.CONVERGED, H.MAX_ITER, H.BREAKDOWN) == tuple(
        hyperelastic.STATUS.index(k) for k in ("CONVERGED", "MAX_ITER", "BREAKDOWN"))
    assert (H.CONVERGED, H.MAX_ITER, H.BREAKDOWN) == (hyperelastic.CONVERGED, hyperelastic.MAX_ITER,
                                                      hyperelastic.BREAKDOWN)
    assert (H.ARMIJO, H.HALVINGS, H.PHI_NOISE) == (hyperelastic.ARMIJO, hyperelastic.HALVINGS, hyperelastic.PHI_NOISE)
    assert set(hyperelastic.VOLUMETRIC) == {"log", "quadratic"}
    for v in hyperelastic.VOLUMETRIC:
        H._vol(np.array(1.1), H.KAPPA, v)


def _random_F(rng, count):
    out = []
    while len(out) < count:
        F = np.eye(2) + 0.25 * rng.standard_normal((2, 2))
        if 0.7 <= np.linalg.det(F) <= 1.4:
            out.append(F)
    return np.array(out)


@pytest.mark.parametrize("volumetric", ("log", "quadratic"))
def test_stress_and_tangent_are_the_derivatives_of_the_energy(volumetric):
    """Central differences with step h: truncation h^2 / 6 |f'''| plus rounding eps |f| / h.  On the sampled set
    (|F_ij| < 2.2, J >= 0.7, mu = 3, kappa = 10) |W| < 1e2 and |P| < 1e2; every derivative of J^(-2/3) I1 and of U
    multiplies by at most ~ (8/3) |G| / J < 10, so |W'''| < 1e4 and |P'''| < 1e5.  With h = 1e-5 that is
    1.7e-7 + 2.2e-9 for P and 1.7e-6 + 2.2e-9 for A, against entries of order 1 to 10."""
    h = 1e-5
    law = dict(mu=H.MU, kappa=H.KAPPA, volumetric=volumetric)
    Fs = _random_F(np.random.default_rng(5), 40)
    assert np.abs(Fs).max() < 2.2
    bound_p = h * h / 6 * 1e4 + EPS * 1e2 / h
    bound_a = h * h / 6 * 1e5 + EPS * 1e2 / h
    worst_p = worst_a = 0.0
    for F in Fs:
        P, A = H.pk1(F, **law), H.tangent(F, **law)
        assert np.abs(H.energy(F, **law)[0]) < 1e2 and np.abs(P).max() < 1e2
        for k in range(2):
            for l in range(2):
                dF = np.zeros((2, 2))
                dF[k, l] = h
                dW = (H.energy(F + dF, **law)[0] - H.energy(F - dF, **law)[0]) / (2 * h)
                dP = (H.pk1(F + dF, **law) - H.pk1(F - dF, **law)) / (2 * h)
                worst_p = max(worst_p, abs(dW - P[k, l]))
                worst_a = max(worst_a, np.abs(dP - A[:, :, k, l]).max())
        A4 = A.reshape(4, 4)
        assert np.abs(A4 - A4.T).max() <= 1e-13 * np.abs(A4).max()
    print(f"{volumetric}: |dW/dF - P| <= {worst_p:.2e} (bound {bound_p:.2e}), |dP/dF - A| <= {worst_a:.2e} "
          f"(bound {bound_a:.2e})")
    assert worst_p <= bound_p and worst_a <= bound_a
    # the stress-free state
    assert np.abs(H.pk1(np.eye(2), **law)).max() <= 4 * EPS * H.MU and H.energy(np.eye(2), **law)[0] == 0.0


def test_linearisation_is_the_linear_cell_problem():
    """mu = 3, kappa = 4: lambda = kappa - 2 mu / 3 = 2, E = 7.2, nu = 0.2; plane strain is plane stress with
    E* = E / (1 - nu^2), nu* = nu / (1 - nu) = 0.25.  The gap to the linear solution is first order in the strain."""
    mu, kappa = 3.0, 4.0
    lam = kappa - 2.0 * mu / 3.0
    young, nu = mu * (3 * lam + 2 * mu) / (lam + mu), lam / (2 * (lam + mu))
    s = meshgen.hole_plate(9, 0.25, seed=3)
    lin = fem_ref.cell(s.pos, s.faces, young / (1 - nu * nu), nu / (1 - nu))
    pb = H.problem(s.pos, s.faces, mu=mu, kappa=kappa)
    gaps = []
    for scale in (1e-5, 1e-6):
        eps = scale * np.array([1.0, -0.6, 0.8])
        ref = fem_ref.fields(lin, eps, fem_ref.solve_direct(lin, eps)[0])
        Fb = H.deformation_gradient(eps)
        # P carries a rounding error of ~ eps mu against forces of ~ mu * strain: rtol cannot go below ~ 1e-16 / strain
        sol = H.newton_direct(pb, Fb, rtol=1e-8, n_steps=1)
        assert sol.status == H.CONVERGED
        got = H.fields(pb, Fb, sol.ut)
        gaps.append(np.abs(got.stress - ref.stress).max() / np.abs(ref.stress).max())
        assert np.abs(got.log_strain - ref.strain).max() <= 10 * scale * np.abs(ref.strain).max()
    print(f"relative gap to the linear solution: {gaps[0]:.3e} at 1e-5, {gaps[1]:.3e} at 1e-6")
    assert gaps[0] <= 1e-4 and 5.0 <= gaps[0] / gaps[1] <= 20.0


@pytest.mark.parametrize("mesh", range(len(H.MESHES)))
def test_every_gpu_load_converges_and_satisfies_hill_mandel(mesh):
    n, r = H.MESHES[mesh]
    s = meshgen.hole_plate(n, r, seed=3)
    for volumetric in ("log", "quadratic") if mesh == 0 else ("log",):
        pb = H.problem(s.pos, s.faces, volumetric=volumetric)
        for eps in H.LOADS:
            Fb = H.deformation_gradient(eps)
            sol = H.newton_direct(pb, Fb, n_steps=H.N_STEPS, check_spd=True)
            print(f"n={n} {volumetric} {eps}: status {sol.status}, {sol.newton} Newton iterations, residual "
                  f"{sol.residual:.2e}, tangent positive definite at every state: {sol.spd}")
            assert sol.status == H.CONVERGED and sol.steps == H.N_STEPS and sol.residual <= 2e-10
            assert np.abs(sol.ut[pb.c.reps].mean(0)).max() <= 1e-12 * np.abs(sol.ut).max()
            f = H.fields(pb, Fb, sol.ut)
            hm = f.mean_pk1 @ Fb.T / np.linalg.det(Fb)
            assert np.abs(np.array([hm[0, 0], hm[1, 1], hm[0, 1]]) - f.mean_stress).max() \
                <= 1e-9 * np.abs(f.mean_stress).max()
            assert abs(hm[0, 1] - hm[1, 0]) <= 1e-9 * np.abs(f.mean_stress).max()
            # no load of the GPU tests meets an indefinite tangent: there is no negative-curvature case to add
            assert sol.spd


def test_the_step_for_step_restatement_agrees_with_the_direct_one():
    s = meshgen.hole_plate(*H.MESHES[0], seed=3)
    pb = H.problem(s.pos, s.faces)
    Fb = H.deformation_gradient(H.LOADS[0])
    a = H.newton_direct(pb, Fb, rtol=1e-12, n_steps=H.N_STEPS)
    b = H.newton_pcg(pb, Fb, n_steps=H.N_STEPS)
    assert a.status == b.status == H.CONVERGED and b.pcg > 0 and b.residual <= 2e-10
    assert np.abs(a.ut - b.ut).max() <= 1e-8 * np.abs(a.ut).max()
    capped = H.newton_pcg(pb, Fb, n_steps=H.N_STEPS, max_newton=1)
    assert capped.status == H.MAX_ITER and capped.steps == 0 and capped.newton == 1


def test_a_plate_without_a_hole_needs_no_iteration():
    s = meshgen.hole_plate(9, 0.0, seed=3)
    pb = H.problem(s.pos, s.faces)
    Fb = H.deformation_gradient(H.LOADS[0])
    sol = H.newton_pcg(pb, Fb, n_steps=H.N_STEPS)
    assert sol.status == H.CONVERGED and sol.newton == 0 and not sol.ut.any()
    f = H.fields(pb, Fb, sol.ut)
    want = H.cauchy(Fb)
    assert np.abs(f.stress - np.array([want[0, 0], want[1, 1], want[0, 1]])).max() <= 1e-13 * np.abs(want).max()


def _exact_energy(pb, Fb, x):
    """Phi = sum area W at the fp64 state x, evaluated with 50 digits (decimal): the mesh data, Fb and x taken as
    exact."""
    import decimal
    D = decimal.Decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        P = pb.c.P.tocsr()
        assert (np.diff(P.indptr) == 1).all() and (P.data == 1.0).all()   # every node reads one representative
        u = [D(float(v)) for v in x[P.indices]]
        mu, kappa = D(pb.law["mu"]), D(pb.law["kappa"])
        assert pb.law["volumetric"] == "log"
        fb = [D(float(v)) for v in np.asarray(Fb).reshape(4)]
        phi = D(0)
        for f in range(len(pb.c.area)):
            F = [fb[a] + sum(D(float(pb.G[f, a, b])) * u[pb.c.dofs[f, b]] for b in range(6)) for a in range(4)]
            J = F[0] * F[3] - F[1] * F[2]
            iso = (J.ln() * D(-2) / D(3)).exp() * (sum(v * v for v in F) + 1)
            phi += D(float(pb.c.area[f])) * (mu / 2 * (iso - 3) + kappa * (J * J.ln() - J + 1))
        return phi


def test_the_line_search_allowance_is_needed_and_admits_no_energy_increase():
    """The kernel's Armijo test allows PHI_NOISE = 32 ulp of the energy terms' magnitude (hyper_ref._backtrack has the
    same rule).  Under the small load Phi ~ 1e-8 |mag| and a late Newton step lowers it by less than the rounding of
    the two sums: the strict rule (allowance 0) exhausts its halvings and ends in BREAKDOWN, far from balance.  And
    the allowance lets no increase through: at every step the restatement accepts, under the small load and a large
    one, the strict rule holds for the energies of the two fp64 states evaluated with 50 digits."""
    s = meshgen.hole_plate(*H.MESHES[0], seed=3)
    pb = H.problem(s.pos, s.faces)
    small = H.deformation_gradient(H.LOADS[2])
    strict = H.newton_direct(pb, small, n_steps=H.N_STEPS, noise=0.0)
    print(f"strict rule, small load: status {strict.status} after {strict.steps} steps, residual {strict.residual:.2e}")
    assert strict.status == H.BREAKDOWN and strict.steps < H.N_STEPS and strict.residual > 1e-6
    for eps in (H.LOADS[2], H.LOADS[0]):
        steps = []
        sol = H.newton_direct(pb, H.deformation_gradient(eps), n_steps=H.N_STEPS, accepted=steps)
        assert sol.status == H.CONVERGED and len(steps) == sol.newton > 0
        below = 0
        for Fb, x, d, alpha, rd in steps:
            assert rd > 0.0
            before, after = _exact_energy(pb, Fb, x), _exact_energy(pb, Fb, x + alpha * d)
            assert float(before - after) >= H.ARMIJO * alpha * rd * (1 + 1e-12), (eps, alpha, rd, float(after - before))
            mag = pb.energy(Fb, x)[1]
            below += float(before - after) < H.PHI_NOISE * mag
        print(f"{eps}: {len(steps)} accepted steps, {below} with a decrease below the allowance")
