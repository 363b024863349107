"""The Q1 restatement tests/femq1_ref.py checked against what the method itself guarantees, on the CPU: the patch
test, the symmetry of C_eff, the two solvers against each other, and the invariances of the fields.  The device
solver is measured against this file (tests/test_gpu_femq1.py), so it has to stand on its own first.

Bounds.  Everything here is fp64 on meshes of at most 132 nodes with h ~ 8 to 12 and coordinates up to 100 (up to
~ 250 after the shift): an element strain is a difference of displacements of size |eps| |x| over h, rounded at
2^-53 |x| / h ~ 3e-15 relative to the unit strain, and the direct solve's backward error times the condition number
of A (~ 1e3 at these sizes) stays below 1e-11.  1e-10 relative is the bound for everything that is exact but for
rounding; the PCG against the direct solve is held to the device test's own bound, 2^-22 max|sigma|: at
rtol = 1e-10 the iterate's error is ~ 1e-10 x the condition number, well inside it."""
import numpy as np
import pytest

import femq1_ref as R
from pdg import meshgen

EXACT = 1e-10
BOUND = 2.0 ** -22


@pytest.fixture(scope="module")
def plate():
    s = meshgen.quad_hole_plate(9, 0.25, seed=3)
    c = R.cell(s.pos, s.faces)
    ut = [R.solve_direct(c, e)[0] for e in R.UNIT]
    return s, c, ut


def test_q1_passes_the_patch_test():
    s = meshgen.quad_hole_plate(9, 0.0, seed=3)
    assert s.faces.shape == (64, 4)
    c = R.cell(s.pos, s.faces)
    assert c.det.min() > 0                       # jittered, counter-clockwise, convex
    for eps in R.UNIT:
        b, b_abs = R.rhs(c, eps)
        ratio = np.linalg.norm(b) / np.linalg.norm(b_abs)
        print(f"patch test {eps}: |b| / |b_abs| = {ratio:.3e}")
        assert ratio < 1e-12
        ut, status = R.solve_direct(c, eps)
        assert status == R.TRIVIAL and not ut.any()
        assert R.pcg(c, eps)[1:] == (0, R.TRIVIAL)
        f = R.fields(c, eps, ut)
        want = R.stiffness() @ eps
        assert np.abs(f.stress - want).max() <= EXACT * np.abs(want).max()
        assert np.abs(f.mean_stress - want).max() <= EXACT * np.abs(want).max()
    assert abs(R.fields(c, R.UNIT[0], ut).material_area - 1e4) <= EXACT * 1e4


def test_stiffness_is_symmetric_with_the_rigid_modes_in_its_kernel(plate):
    _, c, _ = plate
    scale = np.abs(c.K).max()
    assert np.abs(c.K - c.K.T).max() <= 1e-14 * scale
    n = len(c.pos)
    tx, ty = np.tile([1.0, 0.0], n), np.tile([0.0, 1.0], n)
    rot = np.stack([-c.pos[:, 1], c.pos[:, 0]], 1).ravel()
    for mode in (tx, ty, rot):
        assert np.abs(c.K @ mode).max() <= 1e-12 * scale * np.abs(mode).max()
    # the material area is the plate's less the removed quads', and |det J| sums to each quad's area (shoelace)
    p = c.pos[c.faces]
    x, y = p[:, :, 0], p[:, :, 1]
    shoelace = 0.5 * np.abs((x * np.roll(y, -1, 1) - np.roll(x, -1, 1) * y).sum(1))
    assert np.abs(c.w.sum(1) - shoelace).max() <= 1e-12 * shoelace.max()


def test_effective_stiffness_is_symmetric_and_softer_than_the_material(plate):
    _, c, _ = plate
    ce = R.effective_stiffness(c)
    print(f"C_eff asymmetry {np.abs(ce - ce.T).max() / np.abs(ce).max():.3e}")
    assert np.abs(ce - ce.T).max() <= EXACT * np.abs(ce).max()
    assert np.all(np.linalg.eigvalsh(0.5 * (ce + ce.T)) > 0)
    assert np.all(np.linalg.eigvalsh(R.stiffness() - 0.5 * (ce + ce.T)) > 0)   # a hole softens the cell


def test_direct_solve_and_pcg_agree(plate):
    _, c, direct = plate
    for eps, ut in zip(R.UNIT, direct):
        got, its, status = R.pcg(c, eps, rtol=1e-10)
        assert status == R.CONVERGED and 0 < its < 4000
        assert R.residual(c, eps, got) <= 2e-10 and R.residual(c, eps, ut) <= 1e-12
        a, b = R.fields(c, eps, got), R.fields(c, eps, ut)
        err = np.abs(a.stress - b.stress).max() / np.abs(b.stress).max()
        print(f"case {eps}: {its} iterations, PCG against the direct solve {err:.3e}")
        assert err <= BOUND
        assert np.abs(a.mean_stress - b.mean_stress).max() <= 1e-9 * np.abs(b.mean_stress).max()
        assert np.abs(got[c.reps].mean(0)).max() <= 1e-12 * np.abs(got).max()
        assert np.array_equal(got, got[c.rep])


def test_fields_do_not_move_under_a_rigid_translation(plate):
    s, c, direct = plate
    moved = R.cell(s.pos, s.faces, shift=(128.0, -57.5))
    for eps, ut in zip(R.UNIT, direct):
        a, b = R.fields(moved, eps, R.solve_direct(moved, eps)[0]), R.fields(c, eps, ut)
        for x, y in ((a.stress, b.stress), (a.strain, b.strain), (a.gauss_stress, b.gauss_stress)):
            assert np.abs(x - y).max() <= EXACT * np.abs(y).max()
        assert abs(a.material_area - b.material_area) <= 1e-12 * b.material_area


def test_a_clockwise_copy_gives_the_same_solution(plate):
    s, c, direct = plate
    cw = R.cell(s.pos, s.faces[:, ::-1])
    assert cw.det.max() < 0
    for nodal in ("area", "count"):
        for eps, ut in zip(R.UNIT, direct):
            got = R.solve_direct(cw, eps)[0]
            assert np.abs(got - ut).max() <= EXACT * np.abs(ut).max()
            a, b = R.fields(cw, eps, got, nodal), R.fields(c, eps, ut, nodal)
            assert np.abs(a.stress - b.stress).max() <= EXACT * np.abs(b.stress).max()
            assert np.abs(a.mean_stress - b.mean_stress).max() <= EXACT * np.abs(b.mean_stress).max()


def test_degenerate_faces_are_refused(plate):
    s, _, _ = plate
    bow = s.faces.copy()
    bow[0] = bow[0, [0, 2, 1, 3]]
    flat = s.faces.copy()
    flat[0] = flat[0, [0, 0, 3, 3]]          # collapsed onto a segment: dx/dxi = dy/dxi = 0 exactly, det J == 0
    for faces in (bow, flat):
        with pytest.raises(ValueError, match="degenerate or not convex"):
            R.cell(s.pos, faces)
