"""The host restatement of the sampling operator (tests/sample_ref.py) checks itself, without a GPU: partition of
unity, the weights reproduce the query and a linear field, a vertex gives a unit weight, a point in the hole or
outside gives -1, the wrap is idempotent, and on a quad split into two triangles the quad restatement and the
triangle one agree for points on the splitting diagonal."""
from fractions import Fraction

import numpy as np
import pytest

import sample_ref as R


def _plates():
    from pdg import meshgen
    return {"tri": meshgen.hole_plate(13, 0.2), "quad": meshgen.quad_hole_plate(13, 0.2)}


@pytest.fixture(scope="module")
def plates():
    return _plates()


def _centroids(s, count, seed=0):
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(s.faces), size=count, replace=False)
    return pick, s.pos[s.faces[pick]].astype(np.float64).mean(1).astype(np.float32)


@pytest.mark.parametrize("kind", ["tri", "quad"])
def test_partition_of_unity_and_reproduction(plates, kind):
    """sum w = 1, sum w_k p_k = the query and a linear field is reproduced: exactly for triangles (rational
    arithmetic), to a few longdouble roundings for quads (the residual Newton stops at)."""
    s = plates[kind]
    pick, q = _centroids(s, 40)
    cell, w = R.locate(s.pos, s.faces, q)
    assert (cell == pick).all()
    lin = lambda x, y: 3 + 2 * x - 5 * y   # noqa: E731
    for i, c in enumerate(cell):
        p = [(Fraction(float(x)), Fraction(float(y))) for x, y in s.pos[s.faces[c]]]
        qx, qy = Fraction(float(q[i, 0])), Fraction(float(q[i, 1]))
        if kind == "tri":
            assert sum(w[i]) == 1
            assert sum(wk * x for wk, (x, _) in zip(w[i], p)) == qx
            assert sum(wk * y for wk, (_, y) in zip(w[i], p)) == qy
            assert sum(wk * lin(x, y) for wk, (x, y) in zip(w[i], p)) == lin(qx, qy)
        else:
            eps = float(np.finfo(np.longdouble).eps)
            assert abs(float(sum(w[i]) - 1)) <= 8 * eps
            assert abs(float(sum(wk * float(x) for wk, (x, _) in zip(w[i], p)) - float(qx))) <= 64 * eps * 100
            assert abs(float(sum(wk * float(y) for wk, (_, y) in zip(w[i], p)) - float(qy))) <= 64 * eps * 100
            got = sum(wk * float(lin(x, y)) for wk, (x, y) in zip(w[i], p))
            assert abs(float(got - float(lin(qx, qy)))) <= 64 * eps * 1000


@pytest.mark.parametrize("kind", ["tri", "quad"])
def test_a_vertex_gives_a_unit_weight(plates, kind):
    s = plates[kind]
    nodes = np.arange(0, s.num_nodes, 7)
    cell, w = R.locate(s.pos, s.faces, s.pos[nodes])
    assert (cell >= 0).all()
    for n, c, wq in zip(nodes, cell, w):
        k = list(s.faces[c]).index(n)
        for j, wk in enumerate(wq):
            want = 1.0 if j == k else 0.0
            assert abs(float(wk) - want) <= (0 if kind == "tri" else 1e-17), (n, c, j)


@pytest.mark.parametrize("kind", ["tri", "quad"])
def test_hole_and_outside_give_minus_one(plates, kind):
    s = plates[kind]
    q = np.array([[50, 50], [52, 47], [-1, 50], [50, 100.5], [101, 101], [np.nan, 3]], np.float32)
    cell, w = R.locate(s.pos, s.faces, q)
    assert (cell == -1).all() and all(float(x) == 0 for wq in w for x in wq)
    # with the wrap the points beyond the box come back into the material, the hole stays a hole
    cell, _ = R.locate(s.pos, s.faces, q, periodic=True)
    assert list(cell[:2]) == [-1, -1] and (cell[2:5] >= 0).all() and cell[5] == -1
    f = np.arange(s.num_nodes, dtype=np.float64)
    out = R.sample(f, s.faces, cell, R.clamp32(R.locate(s.pos, s.faces, q)[1]), fill=-7.0)
    assert (out[:2] == -7.0).all()


def test_wrap_is_idempotent_and_shifts_by_whole_periods():
    rng = np.random.default_rng(1)
    bb = np.array([0, 0, 100, 100], np.float32)
    q = rng.uniform(-350, 450, size=(500, 2)).astype(np.float32)
    once = R.wrap(q, bb)
    assert (once >= 0).all() and (once <= 100).all()
    assert np.array_equal(R.wrap64(once, bb), once)
    inside = rng.uniform(1, 99, size=(200, 2)).astype(np.float32)
    assert np.array_equal(R.wrap(inside, bb), inside.astype(np.float64))
    k = rng.integers(-3, 4, size=(200, 2))
    shifted = (inside.astype(np.float64) + 100.0 * k).astype(np.float32)   # fp32 rounding of the shifted point
    assert np.abs(R.wrap(shifted, bb) - inside) .max() <= 2.0 ** -24 * 400


def test_quad_restatement_meets_the_triangle_one_on_the_splitting_diagonal():
    """A parallelogram (a, b, c, d) split along a-c.  On that diagonal s = t = lam, so the quad's weights are
    ((1-lam)^2, lam(1-lam), lam^2, lam(1-lam)) and the triangle's (1-lam, 0, lam): both reproduce the point, and
    the bilinear interpolant is the linear one minus the twist term lam(1-lam)(f_a + f_c - f_b - f_d).  So the
    weights satisfy w_a + w_b = 1 - lam, w_c + w_d = lam, w_b = w_d, and the samples of a twist-free field agree."""
    pts = np.array([[1, 2], [5, 3], [7, 8], [3, 7]], np.float32)          # b - a = c - d: a parallelogram
    quad, tris = np.array([[0, 1, 2, 3]]), np.array([[0, 1, 2], [0, 2, 3]])
    lam = np.array([0.125, 0.25, 0.5, 0.75, 0.875])
    q = (pts[0] + lam[:, None] * (pts[2] - pts[0])).astype(np.float32)    # exact: dyadic lam
    cq, wq = R.locate(pts, quad, q)
    ct, wt = R.locate(pts, tris, q)
    assert (cq == 0).all() and (ct == 0).all()                            # the diagonal ties: the lowest id
    f = np.array([2.0, -1.0, 4.0, 7.0])                                   # f_a + f_c = f_b + f_d
    for i, lm in enumerate(lam):
        a, b, c, d = (float(x) for x in wq[i])
        ta, tb, tc = (float(x) for x in wt[i])
        assert (ta, tb, tc) == (1 - lm, 0.0, lm)
        assert abs(a + b - ta) <= 1e-17 and abs(c + d - tc) <= 1e-17 and abs(b - d) <= 1e-17
    vq = R.sample(f, quad, cq, wq)
    vt = R.sample(f, tris, ct, wt)
    assert np.abs(vq - vt).max() <= 1e-15


def test_csr_and_transpose_are_the_adjoint_of_sample():
    s = _plates()["tri"]
    rng = np.random.default_rng(2)
    q = rng.uniform(-5, 105, size=(60, 2)).astype(np.float32)
    cell, w = R.locate(s.pos, s.faces, q)
    w32 = R.clamp32(w)
    rowptr, entries = R.csr(s.faces, cell, s.num_nodes)
    assert rowptr[-1] == 3 * (cell >= 0).sum() and all(
        (np.diff(entries[rowptr[n]:rowptr[n + 1]]) > 0).all() for n in range(s.num_nodes))
    f, g = rng.normal(size=(s.num_nodes, 2)), rng.normal(size=(60, 2))
    g[cell < 0] = np.nan                                                  # outside queries add nothing
    sf = R.sample(f, s.faces, cell, w32, fill=0.0)
    stg, _, _ = R.sample_T(g, s.faces, cell, w32, s.num_nodes)
    lhs = float((sf * np.where(np.isnan(g), 0, g)).sum())
    assert abs(lhs - float((f * stg).sum())) <= 1e-12 * np.abs(f).sum()
