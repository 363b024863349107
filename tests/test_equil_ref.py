"""The restatements of the equilibration (tests/equil_ref.py) against the identities that define it, on the five
meshes of the probe that fixed the mathematics: the dense fp64 projection removes the divergence defect, is
idempotent and W-self-adjoint, composes with the mean shift into the joint minimiser, and the fp32-vector
restatement of the kernel's iteration converges where the kernel is asked to."""
import numpy as np
import pytest

import equil_ref as R


@pytest.fixture(scope="module", params=sorted(R.MESHES))
def case(request):
    s = R.mesh(request.param)
    w, cell = R.areas(s)
    op = R.Operator.of(s)
    return request.param, s, op, R.Dense(op, w), w, cell, R.noisy_field(s)


def test_the_operator_restatements_agree(case):
    _, s, op, d, _, _, sigma = case
    flat = sigma.astype(np.float64).reshape(-1)
    assert np.allclose(op.apply(sigma).reshape(-1), d.C @ flat, rtol=0, atol=1e-12 * np.abs(flat).max())
    q = np.random.default_rng(0).standard_normal((op.n, 2))
    assert np.allclose(op.apply_t(q).reshape(-1), d.C.T @ q.reshape(-1), rtol=0, atol=1e-12)
    # the rows the training penalty keeps are the rows with node type 0, and constants are annihilated there
    assert set(np.unique(s.node_types)) <= {-1, 0, 1}
    # (the exact operator's interior row sums are zero; its entries are rounded to fp32 once: 2^-24 sum |a| a row)
    ones = np.ones(3 * op.n)
    assert np.all(np.abs(d.C @ ones) <= 2.0 ** -24 * (np.abs(d.C) @ ones) + 1e-14)


def test_projection_removes_the_defect(case):
    name, _, op, d, _, _, sigma = case
    star = d.project(sigma)
    before, after = op.defect(sigma), op.defect(star)
    print(f"{name}: n {op.n}, cond(S) {d.cond():.1f}, |C s| {before:.3e} -> {after:.3e}")
    assert d.rank_deficit() == 0
    assert before > 0 and after <= 1e-12 * before


def test_projection_is_idempotent_and_w_self_adjoint(case):
    name, _, _, d, _, _, _ = case
    P = d.matrix()
    scale = np.abs(P).max()
    idem = np.abs(P @ P - P).max() / scale
    WP = d.W[:, None] * P
    adj = np.abs(WP - WP.T).max() / np.abs(WP).max()
    print(f"{name}: |P P - P| {idem:.2e}, |W P - (W P)^T| {adj:.2e}")
    assert idem <= 1e-10 and adj <= 1e-10


def test_transpose_is_the_transpose(case):
    _, _, op, d, _, _, _ = case
    g = np.random.default_rng(1).standard_normal((op.n, 3))
    want = (d.matrix().T @ g.reshape(-1)).reshape(-1, 3)
    assert np.abs(d.project_t(g) - want).max() <= 1e-10 * np.abs(g).max()


def test_projection_then_mean_shift_is_the_joint_minimiser(case):
    """The target is what ``mean_stress`` is in the reference's datasets: the volume average of the field the
    network is asked to predict, here the noise-free ``local_stress``; ``sigma`` (that field plus 5 % noise) plays
    the prediction, so the shift is the noise's average.  The identity is exact only where C annihilates constants;
    the fp32 operator's interior row sums are ~1e-8, not 0, so the two-step result departs from the KKT solution in
    proportion to the shift.  With the generator's synthetic ``mean_stress`` as the target, which is not the
    average of its ``local_stress`` (a shift as large as the field), the departure measured on the CPU was
    3.0e-10 to 7.8e-9 over the five meshes (largest on quad17, cond(S) 673), against 3e-11 to 2.4e-10 with the
    dataset's target; that second figure is printed, not asserted."""
    name, s, op, d, _, cell, sigma = case
    far = s.mean_stress.astype(np.float64)
    far_err = (np.linalg.norm(d.mean_shift(d.project(sigma), far, cell) - d.joint(sigma, far, cell))
               / np.linalg.norm(d.joint(sigma, far, cell)))
    target = (d.W[0::3] @ s.local_stress.astype(np.float64)) / cell
    two_step = d.mean_shift(d.project(sigma), target, cell)
    joint = d.joint(sigma, target, cell)
    err = np.linalg.norm(two_step - joint) / np.linalg.norm(joint)
    mean = (d.W[0::3] @ two_step) / cell
    print(f"{name}: |two-step - KKT| / |KKT| {err:.2e} (synthetic far target: {far_err:.2e}), "
          f"mean miss {np.abs(mean - target).max():.2e}")
    assert err <= 1e-9
    assert np.abs(mean - target).max() <= 1e-10 * max(1.0, np.abs(target).max())


@pytest.mark.parametrize("weighted", [True, False])
def test_fp32_iteration_reaches_rtol(case, weighted):
    name, _, op, d, w, _, sigma = case
    out, (bnorm, tres, it, status) = R.cg32(op, sigma, w if weighted else None, rtol=1e-5, max_iter=1000)
    print(f"{name} weighted={weighted}: {it} iterations, true residual / |b| {tres / bnorm:.3e}, status {status}")
    assert status == 0 and 0 < it <= 1000
    assert abs(bnorm - op.defect(sigma)) <= 1e-12 * bnorm
    assert op.defect(out) <= 2e-5 * bnorm
    if weighted:   # and the result is the dense projection to the residual's bound (tests/test_gpu_equil.py)
        star = d.project(sigma)
        bound = np.sqrt(d.cond()) * (tres / bnorm) * R.wnorm(sigma - star, w) + 8 * 2.0 ** -24 * R.wnorm(sigma, w)
        assert R.wnorm(out - star, w) <= bound


def test_fp32_iteration_transpose_and_edge_cases(case):
    _, s, op, d, w, _, sigma = case
    g = np.random.default_rng(2).standard_normal((op.n, 3)).astype(np.float32)
    out, (bnorm, tres, it, status) = R.cg32(op, g, w, transpose=True, rtol=1e-5)
    assert status == 0 and it > 0
    want = d.project_t(g)
    iw = 1.0 / d.W.reshape(-1, 3)
    bound = (np.sqrt(d.cond()) * (tres / bnorm) * R.wnorm((g - want) * iw, w)
             + 8 * 2.0 ** -24 * R.wnorm(g * iw, w))
    assert R.wnorm((out - want) * iw, w) <= bound
    zero = np.zeros_like(sigma)
    out, info = R.cg32(op, zero, w)
    assert info == (0.0, 0.0, 0, 0) and np.array_equal(out, zero)
    out, info = R.cg32(R.Operator.of(s, np.ones_like(s.node_types)), sigma, w)
    assert info == (0.0, 0.0, 0, 0) and np.array_equal(out, sigma)
    out, info = R.cg32(op, sigma, w, max_iter=0)
    assert np.array_equal(out, sigma) and info[2] == 0 and info[3] & 1
