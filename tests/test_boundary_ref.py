"""The host restatements of the boundary residuals against what they must satisfy: pdg.meshgen.boundary_vectors
closes over every boundary component, and tests/boundary_ref.py (the yardstick of tests/test_gpu_boundary.py) gives
no net force for a constant field, no jump for a periodic one, the jump that was put in, and a gradient that
matches central finite differences.

Bounds, with u = 2^-53.  The boundary nodes of hole_plate lie on the grid (only interior nodes are jittered) and
the differences of two float32 coordinates are exact in fp64, so sum r_e over a closed boundary telescopes to 0
exactly; what is left is the one float32 rounding of each entry, 2^-24 |bvec[n]| <= 2^-24 blen[n] (1 + 2^-23),
summed over the component, plus the fp64 roundings of a node's sums, below 4 u per entry of size <= blen[n]:
closure <= (2^-24 (1 + 2^-22) + 4 u) L, L the component's sum of blen.  The same for sum blen against the
perimeter: along a side of the square the edges are collinear and their lengths telescope to the side, 100.
"""
import math

import numpy as np
import pytest

import boundary_ref as R

U = 2.0 ** -53
PLATES = {"plate9": (9, 0.0), "hole13": (13, 0.2), "plate35": (35, 0.0)}


def _closure_bound(L):
    return (2.0 ** -24 * (1.0 + 2.0 ** -22) + 4.0 * U) * L


@pytest.fixture(scope="module")
def plates():
    from pdg import meshgen
    out = {}
    for name, (n, hole) in PLATES.items():
        s = meshgen.hole_plate(n=n, hole_radius=hole, seed=3)
        out[name] = (s, *meshgen.boundary_vectors(s.pos, s.faces))
    return out


def _fsum_cols(x):
    return np.array([math.fsum(x[:, k].astype(np.float64)) for k in range(x.shape[1])])


@pytest.mark.parametrize("name", sorted(PLATES))
def test_boundary_vectors_close_over_each_boundary(plates, name):
    s, bvec, blen = plates[name]
    assert bvec.dtype == np.float32 and blen.dtype == np.float32 and bvec.shape == (s.num_nodes, 2)
    interior = s.node_types == 0
    assert not bvec[interior].any() and not blen[interior].any()      # exact zeros off the boundary
    assert np.all(blen[~interior] > 0)
    for label in (1, -1):
        on = s.node_types == label
        if label == -1:
            assert on.any() == (PLATES[name][1] > 0)
        L = math.fsum(blen[on].astype(np.float64))
        total = _fsum_cols(bvec[on]) if on.any() else np.zeros(2)
        print(f"{name} label {label}: nodes {int(on.sum())}, L {L}, |sum bvec| {np.abs(total).max():.3e}, "
              f"bound {_closure_bound(L):.3e}")
        assert np.all(np.abs(total) <= _closure_bound(L))
        if label == 1:
            assert abs(L - 400.0) <= _closure_bound(400.0)
    # the hole's vectors point into the hole, away from the material: towards the centre
    hole = s.node_types == -1
    if hole.any():
        centre = np.array([50.0, 50.0])
        assert np.all(np.sum(bvec[hole] * (centre - s.pos[hole]), 1) > 0)
    ext = s.node_types == 1
    assert np.all(np.sum(bvec[ext] * (s.pos[ext] - 50.0), 1) > 0)


def _edges(s):
    return s.edge_index, s.edge_attr


@pytest.mark.parametrize("name", sorted(PLATES))
def test_constant_field_has_no_net_force_and_no_jump(plates, name):
    s, bvec, blen = plates[name]
    sigma = np.tile(np.array([[37.5, -12.25, 8.0]], np.float32), (s.num_nodes, 1))
    ptr = np.array([0, s.num_nodes])
    table, argmax, mag = R.residuals(ptr, sigma, bvec, blen, s.node_types, _edges(s))
    n = s.num_nodes
    a = np.abs(sigma[0].astype(np.float64))
    for cols, L in ((slice(3, 5), table[0, 0]), (slice(5, 7), table[0, 1])):
        close = _closure_bound(L)
        bound = np.array([a[0] + a[2], a[2] + a[1]]) * close + (2.0 * n + 8.0) * U * mag[0, cols]
        print(f"{name}: F {table[0, cols]}, bound {bound}")
        assert np.all(np.abs(table[0, cols]) <= bound)
    assert table[0, 7] == 0.0 and table[0, 8] > 0
    if PLATES[name][1] > 0:
        assert table[0, 2] > 0 and table[0, 0] > 0 and argmax[0] >= 0      # the test is not vacuous
    else:
        assert table[0, 2] == 0 and table[0, 0] == 0 and argmax[0] == -1


def _periodic_field(s):
    """A field that is periodic by construction: a function of the coordinates with the far sides mapped onto
    the near ones, in multiples of 1/64 (so that adding a jump of the same kind is exact in float32)."""
    p = s.pos.astype(np.float64)
    x = np.where(p[:, 0] == p[:, 0].max(), p[:, 0].min(), p[:, 0])
    y = np.where(p[:, 1] == p[:, 1].max(), p[:, 1].min(), p[:, 1])
    f = np.stack([40 * np.sin(0.07 * x) + 3 * y, 25 * np.cos(0.05 * y) - x, 0.3 * x * np.sin(0.11 * y)], 1)
    return (np.round(f * 64) / 64).astype(np.float32)


@pytest.mark.parametrize("name", sorted(PLATES))
def test_periodic_field_has_no_jump_and_an_added_jump_is_counted(plates, name):
    s, bvec, blen = plates[name]
    ptr = np.array([0, s.num_nodes])
    sigma = _periodic_field(s)
    table, _, _ = R.residuals(ptr, sigma, bvec, blen, s.node_types, _edges(s))
    side = int(np.sum(s.pos[:, 0] == s.pos[:, 0].max()))
    # left-right, bottom-top (each side's nodes, corners included) and the two diagonal corner pairs
    assert table[0, 8] == 2 * side + 2 and table[0, 7] == 0.0
    delta = np.array([1.5, -2.25, 0.75], np.float32)
    right = s.pos[:, 0] == s.pos[:, 0].max()
    moved = sigma.copy()
    moved[right] += delta
    assert np.array_equal(moved[right].astype(np.float64), sigma[right].astype(np.float64) + delta)   # exact
    zero = s.edge_attr == 0
    src, dst = s.edge_index[0][zero], s.edge_index[1][zero]
    changed = int(np.sum(right[src] != right[dst])) // 2
    assert changed == side + 2          # the left-right pairs and the two diagonals; top-bottom pairs move together
    t2, _, _ = R.residuals(ptr, moved, bvec, blen, s.node_types, _edges(s))
    want = changed * float(np.sum(delta.astype(np.float64) ** 2))
    print(f"{name}: P2 {t2[0, 7]}, want {want}")
    assert abs(t2[0, 7] - want) <= 4.0 * changed * U * want and t2[0, 8] == table[0, 8]
    # without edges the periodic columns are 0
    t3, _, _ = R.residuals(ptr, moved, bvec, blen, s.node_types, None)
    assert t3[0, 7] == 0 and t3[0, 8] == 0 and np.array_equal(t3[0, :7], t2[0, :7])


def _batch(plates):
    """The three plates as one batch; graph 0 and graph 2 have no hole."""
    names = ("plate9", "hole13", "plate35")
    ss = [plates[k][0] for k in names]
    counts = [s.num_nodes for s in ss]
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ei = np.concatenate([s.edge_index + ptr[i] for i, s in enumerate(ss)], 1)
    ea = np.concatenate([s.edge_attr for s in ss])
    bvec = np.concatenate([plates[k][1] for k in names])
    blen = np.concatenate([plates[k][2] for k in names])
    labels = np.concatenate([s.node_types for s in ss])
    return ptr, (ei, ea), bvec, blen, labels


@pytest.mark.parametrize("term", ["traction", "periodic", "both"])
def test_gradient_matches_central_differences(plates, term):
    ptr, edges, bvec, blen, labels = _batch(plates)
    rng = np.random.default_rng(11)
    N, B = int(ptr[-1]), 3
    sigma = rng.normal(0.0, 50.0, (N, 3))
    gt = np.array([0.7, 1.3, -0.4]) if term != "periodic" else None
    gp = np.array([2.0, -0.5, 0.9]) if term != "traction" else None
    table, _, _ = R.residuals(ptr, sigma, bvec, blen, labels, edges)
    assert table[0, 0] == 0 and table[2, 0] == 0 and table[1, 0] > 0 and np.all(table[:, 8] > 0)
    grad, _ = R.residuals_grad(ptr, sigma, bvec, blen, labels, edges, table, gt, gp)
    assert np.isfinite(grad).all()
    # a graph without a hole has no participating row: its traction term is 0 / 0 and left out of the objective,
    # and only rows whose denominators are non-zero are perturbed
    gt_live = None if gt is None else np.where(table[:, 0] > 0, gt, 0.0)
    hole = np.flatnonzero(labels == -1)
    ext = np.flatnonzero(labels == 1)
    rows = np.concatenate([hole[:6], ext[::37], [int(ptr[1]) + 30, int(ptr[2]) + 700]])
    if term == "traction":
        assert not grad[labels != -1].any()
    h = 1e-3
    worst = 0.0
    for i in rows:
        for k in range(3):
            up, dn = sigma.copy(), sigma.copy()
            up[i, k] += h
            dn[i, k] -= h
            fd = (R.objective(ptr, up, bvec, blen, labels, edges, gt_live, gp)
                  - R.objective(ptr, dn, bvec, blen, labels, edges, gt_live, gp)) / (2 * h)
            scale = max(abs(grad[i, k]), np.abs(grad[i]).max())
            if scale == 0:
                assert fd == 0
                continue
            worst = max(worst, abs(fd - grad[i, k]) / scale)
            assert abs(fd - grad[i, k]) <= 1e-6 * scale, (i, k, fd, grad[i, k])
    print(f"{term}: worst relative difference {worst:.3e} over {len(rows)} rows")


def test_nan_rule_and_zero_weights_of_the_restated_gradient(plates):
    ptr, edges, bvec, blen, labels = _batch(plates)
    rng = np.random.default_rng(5)
    sigma = rng.normal(0.0, 50.0, (int(ptr[-1]), 3)).astype(np.float32)
    table, _, _ = R.residuals(ptr, sigma, bvec, blen, labels, edges)
    broken = table.copy()
    broken[1, 0] = 0.0      # the hole plate's L_int
    broken[2, 8] = 0.0      # the large plate's n_pairs
    g, _ = R.residuals_grad(ptr, sigma, bvec, blen, labels, edges, broken, np.ones(3), np.ones(3))
    n1, n2 = int(ptr[1]), int(ptr[2])
    hole = np.flatnonzero(labels == -1)
    assert np.isnan(g[hole]).all() and np.isfinite(g[:n1]).all()
    zero = (edges[1] == 0) & (edges[0][1] >= n2)
    paired = np.unique(edges[0][1][zero])
    assert np.isnan(g[paired]).all()
    rest = np.setdiff1d(np.arange(n2, int(ptr[3])), paired)
    assert not g[rest].any()
    g0, _ = R.residuals_grad(ptr, sigma, bvec, blen, labels, edges, broken, np.zeros(3), None)
    assert not g0.any()
