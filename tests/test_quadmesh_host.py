"""The host restatements of the quad mesh fields (pdg.meshgen: node_labels, boundary_vectors and nodal_areas given
(F, 4) faces, q1_divergence_operator, quad_hole_plate) against identities they must satisfy and against each other;
the device kernels are checked against these restatements in tests/test_gpu_quadmesh.py, which imports the meshes
built here.

Bounds, with u = 2^-53 and eps = 2^-24 (half an fp32 ulp, relative):
* a nodal area, a boundary vector and an operator value are each one fp32 rounding of an fp64 sum of a handful of
  terms: two evaluations that differ only in the order of the additions lie within one fp32 ulp, 2^-23 |value|;
* a sum of m such fp32 values misses the exact sum by at most eps sum |values| (the roundings) plus
  2 (m + 16) u sum |terms| (fp64 additions in some order and the few roundings inside a term);
* the operator on a linear field: the tolerance of the triangle test of the same identity
  (test_host.py::test_hole_plate_node_types_and_divergence_operator), 1e-4 absolute.
"""
from pathlib import Path

import numpy as np
import pytest

from test_meshfields_host import renumbered

U = 2.0 ** -53
PLATES = [(9, 0.25), (13, 0.2), (24, 0.3), (40, 0.2)]


def qplate(n, hole, jitter=True, periodic=True, seed=3):
    from pdg import meshgen
    return meshgen.quad_hole_plate(n=n, hole_radius=hole, jitter=0.15 if jitter else 0.0, periodic=periodic,
                                   seed=seed)


def split(quads):
    """Every quad (a, b, c, d) as the triangles (a, b, c), (a, c, d): the diagonal (a, c) is shared by the two, so it
    is never a boundary edge, and every side keeps its direction."""
    return np.concatenate([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], 0)


def two_hole_quad_plate(n=24, seed=5):
    """A jittered n x n quad plate without the quads around two centres: (pos, quads)."""
    s = qplate(n, 0.0, seed=seed)
    keep = np.ones(len(s.faces), bool)
    for cx, cy in ((30.0, 30.0), (70.0, 65.0)):
        inside = np.linalg.norm(s.pos - np.array([cx, cy]), axis=1) < 12.0
        keep &= ~inside[s.faces].any(1)
    faces = s.faces[keep]
    used = np.unique(faces.ravel())
    remap = -np.ones(len(s.pos), np.int64)
    remap[used] = np.arange(len(used))
    return s.pos[used], remap[faces]


def shoelace(pos, quads):
    """Signed areas of the quads in fp64: 1/2 sum_k (x_k y_k+1 - x_k+1 y_k)."""
    x, y = pos[quads, 0].astype(np.float64), pos[quads, 1].astype(np.float64)
    return 0.5 * sum(x[:, k] * y[:, (k + 1) % 4] - x[:, (k + 1) % 4] * y[:, k] for k in range(4))


def check_operator(got, want):
    """(rows, cols, vals) twice: the same keys, values to one fp32 ulp plus the fp64 noise of a structural zero
    (the criterion of test_gpu_meshfields.py::test_operator_is_the_host_operator)."""
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    g, w = got[2].astype(np.float64), want[2].astype(np.float64)
    assert np.all(np.abs(g - w) <= 2.0 ** -23 * np.abs(w) + 1e-9 * np.abs(w).max())


@pytest.mark.parametrize("n,hole", PLATES)
@pytest.mark.parametrize("jitter", [True, False])
@pytest.mark.parametrize("periodic", [True, False])
def test_restatement_equals_the_generator(n, hole, jitter, periodic):
    from pdg import meshgen
    s = qplate(n, hole, jitter, periodic)
    assert s.faces.shape[1] == 4 and s.faces.dtype == np.int64 and s.pos.dtype == np.float32
    labels, ncomp, next_ = meshgen.node_labels(s.pos, s.faces)
    assert labels.dtype == np.int64 and np.array_equal(labels, s.node_types)
    assert (ncomp, next_) == (2, 1) and set(np.unique(labels).tolist()) == {-1, 0, 1}
    # the graph is the four sides of every quad (+ the periodic pairs), lengths as for triangles
    ei = meshgen.quad_faces_to_edges(s.faces, s.num_nodes)
    if not periodic:
        assert np.array_equal(s.edge_index, ei) and np.array_equal(s.edge_attr, meshgen.edge_lengths(s.pos, ei))
    else:
        assert s.num_edges == ei.shape[1] + 4 * n + 4         # n pairs a side in both directions, 4 corner pairs


def test_plate_without_a_hole_has_one_external_boundary():
    from pdg import meshgen
    s = qplate(9, 0.0)
    assert len(s.faces) == 64 and s.num_nodes == 81
    labels, ncomp, next_ = meshgen.node_labels(s.pos, s.faces)
    assert (ncomp, next_) == (1, 1) and np.array_equal(labels, s.node_types) and -1 not in labels


def test_two_holes_are_two_internal_boundaries():
    from pdg import meshgen
    pos, quads = two_hole_quad_plate()
    labels, ncomp, next_ = meshgen.node_labels(pos, quads)
    assert (ncomp, next_) == (3, 1) and (labels == -1).sum() > 0


@pytest.mark.parametrize("n,hole", PLATES)
@pytest.mark.parametrize("jitter", [True, False])
def test_split_quads_have_the_same_boundary(n, hole, jitter):
    """Labels, bvec and blen are, bitwise, what the triangle functions give for the quads split along a diagonal:
    the same boundary edges in the same direction, the same side of the edge for the third vertex (the quads are
    convex), the same order of summation."""
    from pdg import meshgen
    s = qplate(n, hole, jitter)
    tri = split(s.faces)
    assert np.array_equal(meshgen.node_labels(s.pos, s.faces)[0], meshgen.node_labels(s.pos, tri)[0])
    qv, ql = meshgen.boundary_vectors(s.pos, s.faces)
    tv, tl = meshgen.boundary_vectors(s.pos, tri)
    assert qv.dtype == np.float32 and np.array_equal(qv.view(np.int32), tv.view(np.int32))
    assert np.array_equal(ql.view(np.int32), tl.view(np.int32))
    assert np.array_equal(ql > 0, s.node_types != 0)


@pytest.mark.parametrize("n,hole", PLATES)
@pytest.mark.parametrize("jitter", [True, False])
def test_nodal_areas_sum_to_the_area(n, hole, jitter):
    from pdg import meshgen
    s = qplate(n, hole, jitter)
    areas = shoelace(s.pos, s.faces)
    assert np.all(areas > 0)                                  # counter-clockwise, convex enough
    total = areas.sum()
    m = 4 * len(s.faces)
    acc = meshgen._quad_nodal_areas(s.pos.astype(np.float64), s.faces)     # the fp64 sums before their one rounding
    assert abs(acc.sum() - total) <= 2 * (m + 16) * U * total
    area, bbox = meshgen.nodal_areas(s.pos, s.faces)
    assert area.dtype == np.float32 and area.shape == (s.num_nodes,) and np.all(area > 0)
    assert np.array_equal(area, acc.astype(np.float32))
    assert abs(area.astype(np.float64).sum() - total) <= (2.0 ** -24 + 2 * (m + 16) * U) * total
    assert np.array_equal(bbox, np.array([0, 100, 0, 100], np.float32))
    # the P1 areas of the split mesh are another lumping of the same total
    tri_area = meshgen.nodal_areas(s.pos, split(s.faces))[0].astype(np.float64).sum()
    assert abs(tri_area - total) <= (2.0 ** -24 + 2 * (m + 16) * U) * total


@pytest.mark.parametrize("n,hole", [(9, 0.25), (41, 0.2)])
def test_a_corner_of_a_square_gets_a_quarter(n, hole):
    """area / 4 on a parallelogram, exactly: the grids of n = 9 and 41 have h = 12.5 and 2.5, so every coordinate,
    product and sum below is exact in fp64 and (2 m + m) / 12 is m / 4 without a rounding."""
    from pdg import meshgen
    s = qplate(n, hole, jitter=False)
    h = 100.0 / (n - 1)
    assert h == float(np.float32(h)) and np.array_equal(np.unique(np.diff(np.unique(s.pos[:, 0]))), [np.float32(h)])
    quarter = 0.5 * np.abs(2.0 * shoelace(s.pos, s.faces)) / 4.0
    assert np.all(quarter == h * h / 4)
    want = np.zeros(s.num_nodes)
    np.add.at(want, s.faces.ravel(), np.repeat(quarter, 4))
    got = meshgen.nodal_areas(s.pos, s.faces)[0]
    assert np.array_equal(got, want.astype(np.float32))
    assert np.all(got[s.node_types == 0] == np.float32(h * h))


@pytest.mark.parametrize("n", [13, 24])
def test_a_corner_of_a_rectangle_gets_a_quarter_to_rounding(n):
    """Where h is not a dyadic number the same identity holds to one fp32 ulp (the fp64 terms agree to a few u)."""
    from pdg import meshgen
    s = qplate(n, 0.3, jitter=False)
    want = np.zeros(s.num_nodes)
    np.add.at(want, s.faces.ravel(), np.repeat(np.abs(shoelace(s.pos, s.faces)) / 4.0, 4))
    got = meshgen.nodal_areas(s.pos, s.faces)[0].astype(np.float64)
    assert np.all(np.abs(got - want) <= 2.0 ** -23 * want)


def test_zero_area_quads_add_nothing():
    from pdg import meshgen
    s = qplate(9, 0.25)
    base = meshgen.nodal_areas(s.pos, s.faces)[0]
    flat = np.array([[0, 1, 1, 0], [2, 2, 2, 2]], np.int64)
    got = meshgen.nodal_areas(s.pos, np.concatenate([s.faces[:5], flat, s.faces[5:]]))[0]
    assert np.array_equal(got, base)


@pytest.mark.parametrize("n,hole", PLATES)
def test_boundary_vectors_of_a_closed_curve_sum_to_zero(n, hole):
    from pdg import meshgen
    s = qplate(n, hole)
    bvec, blen = meshgen.boundary_vectors(s.pos, s.faces)
    for label in (1, -1):
        part = bvec[s.node_types == label].astype(np.float64)
        m = len(part)
        assert m > 0
        for c in (0, 1):
            assert abs(part[:, c].sum()) <= (2.0 ** -24 + 2 * (m + 16) * U) * np.abs(part[:, c]).sum() \
                + 2.0 ** -24 * 2 * blen.astype(np.float64).sum()       # the edges' own roundings before they cancel
    assert not bvec[s.node_types == 0].any() and not blen[s.node_types == 0].any()
    # the outer boundary's length is the square's perimeter
    assert abs(blen[s.node_types == 1].astype(np.float64).sum() - 400.0) <= 400.0 * 2.0 ** -20


@pytest.mark.parametrize("n,hole,jitter", [(9, 0.25, True), (13, 0.2, True), (24, 0.3, True), (24, 0.3, False),
                                           (40, 0.2, True)])
def test_operator_is_exact_on_a_linear_field(n, hole, jitter):
    """(sxx, syy, sxy) = (x, y, 0) has the divergence (1, 1).  area g[vn] is the exact integral of grad N_vn over any
    quad, so the identity holds at every node; it is asserted on label 0 (all faces present) and everywhere."""
    from pdg import meshgen
    s = qplate(n, hole, jitter)
    rows, cols, vals = meshgen.q1_divergence_operator(s.pos, s.faces)
    assert np.array_equal(rows, s.op_div_rows) and np.array_equal(vals, s.op_div_vals)
    nn = s.num_nodes
    assert np.all(np.diff(rows * (2 * nn) + cols) > 0) and vals.dtype == np.float32
    A = np.zeros((nn, 2 * nn))
    np.add.at(A, (rows, cols), vals)
    x, y = s.pos[:, 0].astype(np.float64), s.pos[:, 1].astype(np.float64)
    zero = np.zeros(nn)
    div_x = A @ np.concatenate([x, zero])        # d sxx / dx + d sxy / dy
    div_y = A @ np.concatenate([zero, y])        # d sxy / dx + d syy / dy
    inner = s.node_types == 0
    assert inner.sum() > 0
    assert np.abs(div_x[inner] - 1).max() < 1e-4 and np.abs(div_y[inner] - 1).max() < 1e-4
    assert np.abs(div_x - 1).max() < 1e-4 and np.abs(div_y - 1).max() < 1e-4
    assert np.abs(A[:, nn:] @ x).max() < 1e-4 and np.abs(A[:, :nn] @ y).max() < 1e-4
    # a node's row sums to zero (a constant field has no divergence)
    assert np.abs(A[:, :nn].sum(1)).max() < 1e-6 and np.abs(A[:, nn:].sum(1)).max() < 1e-6
    assert meshgen.cell_divergence_operator(s.pos, s.faces)[2].tobytes() == vals.tobytes()


@pytest.mark.parametrize("n,hole", PLATES)
def test_clockwise_quads_give_the_same_fields(n, hole):
    from pdg import meshgen
    s = qplate(n, hole)
    cw = np.ascontiguousarray(s.faces[:, ::-1])
    assert np.all(shoelace(s.pos, cw) < 0)
    assert np.array_equal(meshgen.node_labels(s.pos, cw)[0], s.node_types)
    assert np.array_equal(meshgen.nodal_areas(s.pos, cw)[0], meshgen.nodal_areas(s.pos, s.faces)[0])
    for a, b in zip(meshgen.boundary_vectors(s.pos, cw), meshgen.boundary_vectors(s.pos, s.faces)):
        assert np.array_equal(a, b)
    check_operator(meshgen.q1_divergence_operator(s.pos, cw), meshgen.q1_divergence_operator(s.pos, s.faces))


@pytest.mark.parametrize("n,hole", PLATES)
def test_renumbering_permutes_the_fields(n, hole):
    from pdg import meshgen
    s = qplate(n, hole)
    pos2, faces2, perm = renumbered(s.pos, s.faces)
    nn = s.num_nodes
    a, ca, ea = meshgen.node_labels(s.pos, s.faces)
    b, cb, eb = meshgen.node_labels(pos2, faces2)
    assert np.array_equal(b[perm], a) and (ca, ea) == (cb, eb)
    # a boundary node has two edges: their sum does not depend on the order
    for x, y in zip(meshgen.boundary_vectors(pos2, faces2), meshgen.boundary_vectors(s.pos, s.faces)):
        assert np.array_equal(x[perm], y)
    # up to four faces a node, added in another order: one fp32 ulp
    w = meshgen.nodal_areas(s.pos, s.faces)[0].astype(np.float64)
    assert np.all(np.abs(meshgen.nodal_areas(pos2, faces2)[0][perm] - w) <= 2.0 ** -23 * w)
    r, c, v = meshgen.q1_divergence_operator(s.pos, s.faces)
    key = perm[r] * (2 * nn) + perm[c % nn] + nn * (c // nn)
    order = np.argsort(key)
    r2, c2, v2 = meshgen.q1_divergence_operator(pos2, faces2)
    check_operator((r2, c2, v2), (key[order] // (2 * nn), key[order] % (2 * nn), v[order]))


def test_quad_edges_against_the_reference_fixture():
    """quad_faces_to_edges against the reference's own _quad_face_to_edge on the two quad cases of
    tests/golden/mesh_to_graph.npz, read the way test_dataset_io.py reads them."""
    from pdg import meshgen
    g = np.load(Path(__file__).resolve().parent / "golden" / "mesh_to_graph.npz")
    names = sorted({k.rsplit("_", 1)[0] for k in g.files if k.endswith("_points")})
    quads = [k for k in names if k.startswith("quad_")]
    assert quads == ["quad_clockwise", "quad_scrambled"]
    for name in quads:
        cells = g[f"{name}_cells"]
        assert cells.shape[1] == 4
        ei = meshgen.quad_faces_to_edges(cells, len(g[f"{name}_points"]))
        assert ei.dtype == np.int64 and np.array_equal(ei, g[f"{name}_edge_index"]), name
