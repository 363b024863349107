"""The CPU restatement of the cell problem (tests/fem_ref.py) checked against what any correct solver must satisfy,
so that the GPU tests compare against something that was itself tested.  Meshes: pdg.meshgen.hole_plate(n, r, seed=3).
The patch test, symmetry and the Voigt bound are properties of the continuous problem's Galerkin discretisation;
their tolerances are those of an fp64 sparse direct solve (condition ~ n^2, far below 1e-10)."""
import numpy as np
import pytest

import fem_ref as R
from pdg import meshgen

MESHES = ((9, 0.25), (13, 0.3))


def _cell(n, r):
    s = meshgen.hole_plate(n, r, seed=3)
    return s, R.cell(s.pos, s.faces)


@pytest.fixture(scope="module")
def cells():
    return {m: _cell(*m) for m in MESHES}


def test_representatives_pair_the_sides_and_share_one_corner():
    s = meshgen.hole_plate(9, 0.25, seed=3)
    rep = R.representatives(s.pos)
    assert np.array_equal(rep[rep], rep)
    rows, cols = meshgen.periodic_pairs(s.pos)
    assert np.array_equal(rep[rows], rep[cols])            # every periodic pair shares its representative
    side = 9
    assert len(np.unique(rep)) == s.num_nodes - (2 * side - 1)
    bad = s.pos.copy()
    bad[np.where(s.pos[:, 0] == s.pos[:, 0].max())[0][3], 1] += 0.25
    with pytest.raises(ValueError, match="mesh is not periodic"):
        R.representatives(bad)


def test_patch_test_without_a_hole_is_trivial():
    s, c = _cell(9, 0.0)
    for eps in R.UNIT:
        b, b_abs = R.rhs(c, eps)
        ratio = np.linalg.norm(b) / np.linalg.norm(b_abs)
        print(f"patch test: |b| / |b_abs| = {ratio:.2e}")
        assert ratio <= R.NOISE
        ut, status = R.solve_direct(c, eps)
        assert status == R.TRIVIAL and not ut.any()
        ut, it, status = R.pcg(c, eps)
        assert (it, status) == (0, R.TRIVIAL)
        f = R.fields(c, eps, ut)
        want = R.stiffness() @ eps
        assert np.abs(f.elem_stress - want).max() <= 1e-12 * np.abs(want).max()
        assert np.abs(f.stress - want).max() <= 1e-12 * np.abs(want).max()


def test_effective_stiffness_is_symmetric_consistent_and_below_voigt(cells):
    for (n, r), (s, c) in cells.items():
        ce = R.effective_stiffness(c)
        scale = np.abs(ce).max()
        assert np.abs(ce - ce.T).max() <= 1e-10 * scale
        eps = np.array([1e-3, -2e-3, 5e-4])
        f = R.fields(c, eps, R.solve_direct(c, eps)[0])
        assert np.abs(f.mean_stress - ce @ eps).max() <= 1e-10 * np.abs(ce @ eps).max()
        # Voigt: C_eff <= (material area / cell area) C in the Loewner order, strictly with a hole
        voigt = f.material_area / f.cell_area * R.stiffness()
        assert f.material_area < f.cell_area
        gap = np.linalg.eigvalsh(voigt - 0.5 * (ce + ce.T))
        assert gap.min() > 0.0, (n, r, gap)
        assert np.linalg.eigvalsh(0.5 * (ce + ce.T)).min() > 0.0


def test_direct_and_pcg_agree(cells):
    for (n, r), (s, c) in cells.items():
        for eps in R.UNIT:
            ud, sd = R.solve_direct(c, eps)
            up, it, st = R.pcg(c, eps, rtol=1e-10)
            assert sd == R.CONVERGED and st == R.CONVERGED
            assert R.residual(c, eps, up) <= 2e-10 and R.residual(c, eps, ud) <= 1e-10
            fd, fp = R.fields(c, eps, ud), R.fields(c, eps, up)
            err = np.abs(fd.stress - fp.stress).max() / np.abs(fd.stress).max()
            print(f"n={n} r={r}: pcg {it} iterations, stress difference to the direct solve {err:.2e}")
            assert err <= 1e-8           # rtol x the condition of the reduced operator (~ n^2)
            assert it <= 12 * n          # the prototype's 6.5 n, with slack
            assert np.abs(up[c.reps].mean(0)).max() <= 1e-12 * np.abs(up).max()


def test_pcg_stops_at_the_cap_and_nodal_weightings_differ(cells):
    s, c = cells[(9, 0.25)]
    up, it, st = R.pcg(c, R.UNIT[0], max_iter=5)
    assert (it, st) == (5, R.MAX_ITER) and np.isfinite(up).all()
    ud, _ = R.solve_direct(c, R.UNIT[0])
    fa, fc = R.fields(c, R.UNIT[0], ud, "area"), R.fields(c, R.UNIT[0], ud, "count")
    assert np.abs(fa.stress - fc.stress).max() > 1e-6 * np.abs(fa.stress).max()   # a jittered mesh: areas differ
    assert np.array_equal(fa.mean_stress, fc.mean_stress)
