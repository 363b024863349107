"""The host restatement of the fused physics loss (tests/physloss_ref.py) against itself: its gradient against
central differences of its loss, and the identities the three terms satisfy.  What the GPU tests compare the kernels
with is checked here without a GPU."""
import numpy as np
import pytest

import physloss_ref as R


@pytest.fixture(scope="module")
def small():
    """The issue's plates without the large one (the differences below cost one forward per element), and the quad
    plate."""
    tri, quad = R.cases()
    return R.Inputs(tri[:3]), R.Inputs(quad)


@pytest.mark.parametrize("which", ["tri", "quad"])
@pytest.mark.parametrize("denom", [True, False])
def test_gradient_against_central_differences(small, which, denom):
    c = small[0] if which == "tri" else small[1]
    groups = c.groups(denom)
    scale = np.array([0.7, 1.3, 0.4]) / c.B
    y = c.y.astype(np.float64)
    table, loss = R.forward(c.ptr, y, c.affine, **groups)
    grad, mag = R.backward(c.ptr, y, c.affine, table, scale, **groups)
    assert np.isfinite(grad).all() and np.any(grad != 0)
    # every term is a quadratic in y: a central difference is exact up to rounding, so h only has to keep the
    # cancellation error f u / h small against the gradients' scale
    rng = np.random.default_rng(5)
    rows = np.unique(np.concatenate([rng.choice(c.N, 12, replace=False), np.flatnonzero(c.labels == -1)[:6],
                                     c.ei[1][c.ea == 0][:6].astype(np.int64)]))
    h = 1e-4
    f0 = abs(R.objective(c.ptr, y, c.affine, scale, **groups))
    worst = 0.0
    for i in rows:
        for k in range(3):
            yp, ym = y.copy(), y.copy()
            yp[i, k] += h
            ym[i, k] -= h
            fd = (R.objective(c.ptr, yp, c.affine, scale, **groups)
                  - R.objective(c.ptr, ym, c.affine, scale, **groups)) / (2 * h)
            tol = 64 * 2.0 ** -53 * f0 / h + 1e-9 * mag[i, k]
            worst = max(worst, abs(fd - grad[i, k]) / tol)
            assert abs(fd - grad[i, k]) <= tol, (i, k, fd, grad[i, k])
    print(f"{which} denom={denom}: worst |fd - grad| / tol {worst:.3e} over {len(rows)} rows")


def test_a_constant_field_has_no_periodic_loss(small):
    c = small[0]
    y = np.full((c.N, 3), 0.375, np.float32)
    table, loss = R.forward(c.ptr, y, c.affine, **c.groups())
    assert not loss[:, 1].any() and not table[:, 2].any()
    assert table[0, 3] > 0 and table[1, 3] == 0 and table[2, 3] > 0       # the second plate is not periodic
    grad, _ = R.backward(c.ptr, y, c.affine, table, np.array([0.0, 1.0, 0.0]), **c.groups())
    assert not grad.any()


@pytest.mark.parametrize("denom", [True, False])
def test_a_field_with_the_target_average_has_no_mean_loss(small, denom):
    c = small[0]
    groups = c.groups(denom)
    table, _ = R.forward(c.ptr, c.y, c.affine, **groups)
    # the targets the field already meets: std * S / D
    area, _, cell = groups["mean"]
    target = np.float64(c.affine[0]) * table[:, 5:8] / table[:, 8:9]
    groups["mean"] = (area, target, cell)
    t2, loss = R.forward(c.ptr, c.y, c.affine, **groups)
    scale = np.abs(table[:, 5:8] / table[:, 8:9]).max()
    assert np.all(loss[:, 2] <= (8 * 2.0 ** -53 * scale) ** 2)
    grad, _ = R.backward(c.ptr, c.y, c.affine, t2, np.array([0.0, 0.0, 1.0]), **groups)
    assert np.all(np.abs(grad) <= 1e-12)


def test_an_absent_term_is_exact_zeros(small):
    c = small[0]
    full = c.groups()
    table, loss = R.forward(c.ptr, c.y, c.affine, **full)
    assert loss[0].all() and loss[1, 0] > 0 and loss[2, 1] > 0 and loss[:, 2].all()
    assert loss[1, 1] == 0.0 and table[1, 3] == 0.0          # not periodic: no jump term
    assert loss[2, 0] == 0.0 and table[2, 0] == 0.0          # no hole: no traction term
    ones = np.ones(3)
    grad, mag = R.backward(c.ptr, c.y, c.affine, table, ones, **full)
    n0, n1, n2, n3 = c.ptr
    only_t = R.backward(c.ptr, c.y, c.affine, table, np.array([1.0, 0, 0]), **full)[0]
    only_p = R.backward(c.ptr, c.y, c.affine, table, np.array([0, 1.0, 0]), **full)[0]
    assert not only_t[n2:n3].any() and not only_p[n1:n2].any()
    assert not only_t[c.labels != -1].any()
    # a group that is not given is absent for every graph, and the others are what they were
    for drop, cols in (("boundary", [0, 1, 9]), ("edges", [2, 3, 10]), ("mean", [4, 5, 6, 7, 8, 11])):
        g = dict(full)
        g[drop] = None
        t, l = R.forward(c.ptr, c.y, c.affine, **g)
        keep = [k for k in range(12) if k not in cols]
        assert not t[:, cols].any() and np.array_equal(t[:, keep], table[:, keep])
        gr, _ = R.backward(c.ptr, c.y, c.affine, t, ones, **g)
        k = {"boundary": 0, "edges": 1, "mean": 2}[drop]
        w = ones.copy()
        w[k] = 0.0
        assert np.array_equal(gr, R.backward(c.ptr, c.y, c.affine, table, w, **full)[0])
    # no participating area, or a cell area that is not > 0: the mean term is absent, not NaN
    area = c.area.copy()
    area[n0:n1] = 0.0
    cell = c.cell.copy()
    cell[2] = 0.0
    g = dict(full, mean=(area, c.target, cell))
    t, l = R.forward(c.ptr, c.y, c.affine, **g)
    assert l[0, 2] == 0.0 and l[2, 2] == 0.0 and l[1, 2] > 0 and np.isfinite(t).all()
    gr, _ = R.backward(c.ptr, c.y, c.affine, t, np.array([0, 0, 1.0]), **g)
    assert not gr[n0:n1].any() and not gr[n2:n3].any() and gr[n1:n2].any()
    # a NaN in a participating input is not hidden
    y = c.y.copy()
    hole = int(np.flatnonzero(c.labels[n0:n1] == -1)[2])
    y[hole, 2] = np.nan
    assert np.isnan(R.forward(c.ptr, y, c.affine, **full)[1][0, 0])


def test_reduce_restatement():
    lp = np.array([[1.0, 2.0, np.nan], [3.0, 4.0, 5.0]], np.float32)
    out = R.reduce([0.5, 0.25], [2.0, 1.0], lp, 0.5, 0.25, [0.5, 2.0, 0.0])
    assert out.tolist() == [1.0, 0.375, 0.75, 0.375 + 0.75 + 2.0 + 12.0, 2.0, 12.0, 0.0]
    assert R.reduce([0.5, 0.25], None, None, 0.5, 0.0, None).tolist() == [1.0, 0.375, 0.0, 0.375, 0.0, 0.0, 0.0]
