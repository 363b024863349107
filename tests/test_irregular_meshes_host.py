"""The irregular meshes of tests/irregular_meshes.py themselves, on the host: that each is the mesh its construction
says (counts, orientation, Euler characteristic, manifold edges, the hub's valence), and that pdg.meshgen's
restatements give on it what the construction knows without them -- the labels, the covered area (from the boundary
polygons alone) and a zero sum of the boundary vectors around every closed boundary.  tests/test_gpu_irregular_mesh.py
compares the device with those restatements on these meshes; this file keeps that yardstick honest without a GPU.

Bounds, with u = 2^-53 and D the bounding box's diagonal:

* total area.  meshgen.nodal_areas rounds each node's fp64 sum once to fp32 (<= 2^-24 area[n]); the fp64 work on both
  sides -- a det or a shoelace term is two products of coordinate differences (exact: float32 inputs) and their
  difference, <= 6 u D^2 off, and a few more roundings for the / 3 and the sums -- stays under 16 u D^2 per term,
  3 F + m terms for F faces and m boundary nodes:  |sum area - polygons| <= 2^-24 sum area + 16 u (3 F + m) D^2.
* closed-boundary sum.  An edge's r = (yb - ya, -(xb - xa)) is exact in fp64, so the exact nodal vectors 1/2 (r + r')
  of a closed curve telescope to exactly 0.  meshgen.boundary_vectors rounds r + r' once in fp64 (<= u), halves
  exactly, and rounds to fp32 (<= 2^-24):  |sum_n bvec[n]| <= (2^-24 + 2 u) sum_n |bvec[n]| per component, the sum
  taken exactly (math.fsum).  The same for the lengths is not an invariant (blen sums to the perimeter).
"""
import math

import numpy as np
import pytest

import irregular_meshes as M

U = 2.0 ** -53

CASES = {
    "disk11": lambda: M.fan_disk(11),
    "disk33_hub_last": lambda: M.fan_disk(33, hub_id=-1),
    "disk33_three_rings": lambda: M.fan_disk(33, rings=3),
    "disk700": lambda: M.fan_disk(700),
    "disk683_renumbered": lambda: M.fan_disk(683, renumber=5),
    "disk2049_hub_last": lambda: M.fan_disk(2049, hub_id=-1),
    "annulus33": lambda: M.fan_annulus(33, 2),
    "annulus700_renumbered": lambda: M.fan_annulus(700, 2, renumber=5),
    "annulus33_three_rings": lambda: M.fan_annulus(33, 3),
    "quad_fan2": lambda: M.quad_fan(2),
    "quad_fan3": lambda: M.quad_fan(3),
    "quad_fan129_renumbered": lambda: M.quad_fan(129, renumber=2),
    "quad_fan513": lambda: M.quad_fan(513),
    "refined13_periodic": lambda: M.refined_plate(13, 0.2, True),
    "refined24_open_renumbered": lambda: M.refined_plate(24, 0.3, False, splits=60, flips=50, renumber=7),
    "strip": lambda: M.two_column_strip(),
    "strip_renumbered": lambda: M.two_column_strip(renumber=3),
}


def _edge_uses(faces):
    nv = faces.shape[1]
    sides = np.sort(np.concatenate([faces[:, [j, (j + 1) % nv]] for j in range(nv)], 0), 1)
    return np.unique(sides, axis=0, return_counts=True)


def check_area_and_closed_boundaries(m, area, bvec, what):
    """The two invariants of the module docstring for the nodal areas and boundary vectors ``area`` / ``bvec`` of
    ``m`` (the host's here, the device's in tests/test_gpu_irregular_mesh.py)."""
    loops = M.boundary_loops(m.faces)
    p = m.pos.astype(np.float64)
    d2 = float(np.sum((p.max(0) - p.min(0)) ** 2))
    want = sum(M.polygon_area(m.pos, loop) for loop in loops)
    total = math.fsum(area.astype(np.float64))
    bound = 2.0 ** -24 * total + 16 * U * (m.faces.size + sum(map(len, loops))) * d2
    print(f"{what}: area {total!r} against the polygons' {want!r}: |diff| / bound {abs(total - want) / bound:.3e}")
    assert abs(total - want) <= bound
    on_loop = np.zeros(m.num_nodes, bool)
    for loop in loops:
        on_loop[loop] = True
        for c in range(2):
            v = bvec[loop, c].astype(np.float64)
            s, mag = math.fsum(v), math.fsum(np.abs(v))
            assert abs(s) <= (2.0 ** -24 + 2 * U) * mag, (what, len(loop), c, s, mag)
    assert not bvec[~on_loop].any()
    return loops


@pytest.mark.parametrize("name", CASES)
def test_the_mesh_is_what_its_construction_says(name):
    m = CASES[name]()
    n, nf = m.num_nodes, len(m.faces)
    assert m.pos.dtype == np.float32 and m.pos.shape == (n, 2) and m.faces.dtype == np.int64
    assert np.all(M.determinants(m.pos, m.faces) > 0)
    assert np.array_equal(np.unique(m.faces), np.arange(n))          # every node is used
    edges, uses = _edge_uses(m.faces)
    assert set(uses.tolist()) <= {1, 2}                               # an interior edge is in exactly two faces
    loops = M.boundary_loops(m.faces)
    assert int((uses == 1).sum()) == sum(map(len, loops))
    assert n - len(edges) + nf == 2 - len(loops)                      # Euler: 1 for a disk, 0 with one hole
    val = M.valences(m.faces, n)
    if name.startswith("disk"):
        k, rings = len(m.rings[0]), len(m.rings)
        assert (n, nf, len(loops)) == (1 + k * rings, k + 2 * k * (rings - 1), 1)
        assert val[m.hub] == k and val[m.rings[0]].tolist() == [5 if rings > 1 else 2] * k
        assert m.hub == (n - 1 if "last" in name else 0) or m.perm is not None
    elif name.startswith("annulus"):
        k, rings = len(m.rings[0]), len(m.rings)
        assert (n, nf, len(loops)) == (k * rings, 2 * k * (rings - 1), 2) and m.hub is None
        assert sorted(map(len, loops)) == [k, k]
    elif name.startswith("quad_fan"):
        k = len(m.rings[0]) // 2
        assert (n, nf, len(loops)) == (1 + 4 * k, 3 * k, 1) and m.faces.shape[1] == 4 and val[m.hub] == k
    elif name.startswith("refined"):
        assert val.min() < 5 and val.max() >= 12 and (val == 3).sum() >= 1 and len(loops) == 2
    else:
        assert (n, nf, len(loops)) == (14, 12, 1)


@pytest.mark.parametrize("name", CASES)
def test_the_restatements_reproduce_the_construction(name):
    from pdg import meshgen
    m = CASES[name]()
    labels, ncomp, next_ = meshgen.node_labels(m.pos, m.faces)
    assert np.array_equal(labels, m.labels)
    loops = M.boundary_loops(m.faces)
    assert (ncomp, next_) == (len(loops), 1)
    if name.startswith(("disk", "quad_fan")):
        assert set(np.where(labels == 1)[0].tolist()) == set(m.rings[-1].tolist()) and -1 not in labels
    if name.startswith("annulus"):
        assert set(np.where(labels == -1)[0].tolist()) == set(m.rings[0].tolist())
        assert set(np.where(labels == 1)[0].tolist()) == set(m.rings[-1].tolist())
    area, _ = meshgen.nodal_areas(m.pos, m.faces)
    bvec, blen = meshgen.boundary_vectors(m.pos, m.faces)
    check_area_and_closed_boundaries(m, area, bvec, name)
    assert np.array_equal(blen > 0, labels != 0)
    # the operator and the edges accept the mesh: one row per node, the hub's row with its valence + 1 column nodes
    rows, cols, vals = meshgen.cell_divergence_operator(m.pos, m.faces)
    assert np.array_equal(np.unique(rows), np.arange(m.num_nodes)) and np.isfinite(vals).all()
    ei, ea = M.host_graph(m.pos, m.faces, False)
    if m.hub is not None and not name.startswith("refined"):
        k = M.valences(m.faces, m.num_nodes)[m.hub]
        assert (ei[0] == m.hub).sum() == k and (rows == m.hub).sum() == 2 * ((2 if m.faces.shape[1] == 4 else 1) * k + 1)


@pytest.mark.parametrize("k,renumber", [(16, None), (17, 4), (1025, None)])
def test_pinwheel_is_one_pinched_boundary(k, renumber):
    """The one mesh here whose boundary is not a set of closed curves: 2 k boundary edges meet at the hub."""
    from pdg import meshgen
    m = M.pinwheel(k, renumber=renumber)
    assert (m.num_nodes, len(m.faces)) == (1 + 2 * k, k) and M.valences(m.faces, m.num_nodes)[m.hub] == k
    edges, uses = _edge_uses(m.faces)
    assert len(edges) == 3 * k and np.all(uses == 1) and (edges == m.hub).any(1).sum() == 2 * k
    labels, ncomp, next_ = meshgen.node_labels(m.pos, m.faces)
    assert np.array_equal(labels, m.labels) and (ncomp, next_) == (1, 1)
    area, _ = meshgen.nodal_areas(m.pos, m.faces)
    want = 0.5 * float(M.determinants(m.pos, m.faces).sum())
    assert abs(math.fsum(area.astype(np.float64)) - want) <= 2.0 ** -24 * want + 16 * U * 3 * k * 2 * (2 * M.RING_STEP) ** 2
    # every triangle is a closed curve of its own: each triangle's three edge vectors sum to 0, so the mesh's do
    bvec, _ = meshgen.boundary_vectors(m.pos, m.faces)
    for c in range(2):
        v = bvec[:, c].astype(np.float64)
        # as in the module docstring, but the hub's fp64 sum has 2 k terms, not 2: <= 2 k u (1/2 sum |r|), and its
        # 2 k edges have |r| = RING_STEP
        assert abs(math.fsum(v)) <= (2.0 ** -24 + 2 * U) * math.fsum(np.abs(v)) + 2 * k * U * k * M.RING_STEP


def test_refined_plate_keeps_the_sides_and_the_area():
    from pdg import meshgen
    m = M.refined_plate(13, 0.2, True)
    s = meshgen.hole_plate(n=13, hole_radius=0.2, periodic=True, seed=3)
    assert np.array_equal(m.pos[:s.num_nodes], s.pos) and np.array_equal(m.labels[:s.num_nodes], s.node_types)
    for a, b in zip(meshgen.periodic_pairs(m.pos), meshgen.periodic_pairs(s.pos)):
        assert np.array_equal(a, b)
    # a split and a flip keep the covered polygon: the same boundary curves as the plate's
    base = M.Irregular(s.pos, s.faces, s.node_types)
    assert [loop.tolist() for loop in M.boundary_loops(m.faces)] == [loop.tolist() for loop in M.boundary_loops(s.faces)]
    assert M.material_area(m) == M.material_area(base)
    val = M.valences(m.faces, m.num_nodes)
    print("valence histogram", np.bincount(val).tolist())
    assert val.max() >= 12 and (val == 3).sum() >= 1 and len(m.pos) == s.num_nodes + 40
    side = np.where(s.node_types != 0)[0]
    assert np.array_equal(val[side], M.valences(s.faces, s.num_nodes)[side])      # boundary nodes keep their faces


def test_every_left_right_pair_of_the_strip_is_a_mesh_edge():
    from pdg import meshgen
    m = M.two_column_strip()
    rows = m.num_nodes // 2
    pr, pc = meshgen.periodic_pairs(m.pos)
    mesh_ei, _ = M.host_graph(m.pos, m.faces, False)
    mesh = set(zip(*mesh_ei.tolist()))
    doubled = [(a, b) for a, b in zip(pr.tolist(), pc.tolist()) if (a, b) in mesh]
    assert sorted(doubled) == sorted([(j, rows + j) for j in range(rows)] + [(rows + j, j) for j in range(rows)])
    ei, ea = M.host_graph(m.pos, m.faces, True)
    width = np.float32(m.pos[:, 0].max())
    got = {(a, b): w for a, b, w in zip(*ei.tolist(), ea.tolist())}
    assert all(got[e] == width for e in doubled)                      # the length, not the pair's 0
    only_pairs = [(a, b) for a, b in zip(pr.tolist(), pc.tolist()) if (a, b) not in mesh]
    assert only_pairs and all(got[e] == 0.0 for e in only_pairs)
    assert ei.shape[1] == mesh_ei.shape[1] + len(only_pairs)


def operator_sum_noise(pos, faces):
    """For every entry of the divergence operator: |its terms added in face order in fp64 - their exact sum|, the
    largest over the entries, over the hub-sized rows' share of it, and max |entry|.  The terms are meshgen's:
    area (g / det) / wsum with g = y[v + 1] - y[v - 1] for Dx and x[v - 1] - x[v + 1] for Dy."""
    p = np.asarray(pos, np.float32).astype(np.float64)
    nv, n = faces.shape[1], len(pos)
    det = M.determinants(pos, faces)
    area = 0.5 * np.abs(det)
    wsum = np.zeros(n)
    np.add.at(wsum, faces.ravel(), np.repeat(area, nv))
    keys, vals = [], []
    for vi in range(nv):
        for vn in range(nv):
            nx, pv = faces[:, (vn + 1) % nv], faces[:, (vn - 1) % nv]
            for off, g in ((0, p[nx, 1] - p[pv, 1]), (n, p[pv, 0] - p[nx, 0])):
                keys.append(faces[:, vi] * (2 * n) + faces[:, vn] + off)
                vals.append(area * (g / det) / wsum[faces[:, vi]])
    keys, vals = np.concatenate(keys), np.concatenate(vals)
    face = np.tile(np.arange(len(faces)), 2 * nv * nv)
    order = np.lexsort((face, keys))
    keys, vals = keys[order], vals[order].tolist()
    starts = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1], [True]]))
    worst = biggest = 0.0
    for a, b in zip(starts[:-1].tolist(), starts[1:].tolist()):
        s = 0.0
        for t in vals[a:b]:
            s += t
        exact = math.fsum(vals[a:b])
        worst = max(worst, abs(s - exact))
        biggest = max(biggest, abs(exact))
    return worst, biggest


@pytest.mark.parametrize("name,mesh", [("disk2049", lambda: M.fan_disk(2049)), ("quad_fan513", lambda: M.quad_fan(513))])
def test_order_of_the_hub_sums_stays_under_the_operator_bound(name, mesh):
    """The device adds an entry's terms in face order, the host in (vi, vn, face) order; the operator tests allow
    1e-9 max|vals| for that.  A hub entry has up to 2049 terms: the distance of the face-order sum from the exact
    sum is the size of what a reordering can change.  Measured: 4.1e-8 of that allowance on the k = 2049 disk (2.2e-16
    absolute), 5.4e-8 on the k = 513 quad fan: the 1e-9 max|vals| term holds for the hub's row as for any other."""
    m = mesh()
    worst, biggest = operator_sum_noise(m.pos, m.faces)
    print(f"{name}: worst |face-order sum - exact sum| {worst:.3e} = {worst / (1e-9 * biggest):.3e} of 1e-9 max|vals|")
    assert 2 * worst <= 1e-3 * 1e-9 * biggest     # two orders, each this far from the exact sum at the most
