"""The host side of the homogenisation layer: pdg.meshgen.nodal_areas (the restatement of pdg_nodal_areas) and
tests/homog_ref.py (the restatement of pdg_graph_wmean / pdg_mean_correct) against identities that tie them to the
reference's averages (scripts/generate_dataset.py:73-82, :278-289: quadrature weights gathered to the nodes,
integrate_field(sigma) / bounding_box.volume and / integrate_field(1)).  The reference's own average needs fedoo,
so there is no golden file: the identities below are what a P1 Gauss quadrature satisfies."""
import numpy as np
import pytest

import homog_ref as R

U32 = 2.0 ** -24   # one fp32 rounding, relative


def _plate(n, hole=0.0, seed=3):
    from pdg import meshgen
    return meshgen.hole_plate(n=n, hole_radius=hole, seed=seed)


def _box_area(bbox):
    b = bbox.astype(np.float64)
    return (b[1] - b[0]) * (b[3] - b[2])


@pytest.mark.parametrize("n,hole", [(9, 0.0), (13, 0.2), (35, 0.0), (24, 0.3)])
def test_nodal_areas_sum_to_the_face_areas(n, hole):
    from pdg import meshgen
    s = _plate(n, hole)
    area, bbox = meshgen.nodal_areas(s.pos, s.faces)
    assert area.dtype == np.float32 and area.shape == (s.num_nodes,) and bbox.dtype == np.float32 and bbox.shape == (4,)
    assert np.all(area > 0)
    assert bbox.tolist() == [s.pos[:, 0].min(), s.pos[:, 0].max(), s.pos[:, 1].min(), s.pos[:, 1].max()]
    total, want = float(area.astype(np.float64).sum()), float(R.face_areas(s.pos, s.faces).sum())
    # every nodal area is one fp64 sum rounded once to fp32
    assert abs(total - want) <= U32 * want + 1e-12 * want
    # the same weights from the faces' side: a third of each face to each of its nodes
    by_node = np.zeros(s.num_nodes)
    for f, a in zip(s.faces, R.face_areas(s.pos, s.faces)):
        by_node[f] += a / 3.0
    assert np.all(np.abs(area - by_node) <= 2 * U32 * by_node)


@pytest.mark.parametrize("n", [9, 35])
def test_a_plate_without_a_hole_fills_its_bounding_box(n):
    from pdg import meshgen
    s = _plate(n)
    area, bbox = meshgen.nodal_areas(s.pos, s.faces)
    box = _box_area(bbox)
    assert abs(box - 1e4) <= 1e-2
    assert abs(float(area.astype(np.float64).sum()) - box) <= U32 * box + 1e-12 * box


def test_a_hole_lowers_the_material_area_by_about_its_polygon():
    from pdg import meshgen
    n, r = 25, 20.0
    s = _plate(n, r / 100.0)
    h = 100.0 / (n - 1)
    area, bbox = meshgen.nodal_areas(s.pos, s.faces)
    missing = _box_area(bbox) - float(area.astype(np.float64).sum())
    # the faces with a node inside the circle are removed: a polygon between the circles of radius r - h and r + 2 h
    assert np.pi * (r - h) ** 2 <= missing <= np.pi * (r + 2 * h) ** 2


def test_unreferenced_nodes_and_zero_area_faces_add_nothing():
    from pdg import meshgen
    s = _plate(9, 0.25)
    area, bbox = meshgen.nodal_areas(s.pos, s.faces)
    pos = np.concatenate([s.pos, np.array([[40.0, 60.0]], np.float32)])
    faces = np.concatenate([s.faces[:5], np.array([[0, 1, 1], [2, 2, 2]], np.int64), s.faces[5:]])
    a2, b2 = meshgen.nodal_areas(pos, faces)
    assert a2[-1] == 0.0 and np.array_equal(a2[:-1], area) and np.array_equal(b2, bbox)
    # only x and y are read
    pts3 = np.concatenate([s.pos, np.full((s.num_nodes, 1), 7.0, np.float32)], 1)
    a3, b3 = meshgen.nodal_areas(pts3, s.faces)
    assert np.array_equal(a3, area) and np.array_equal(b3, bbox)
    # no faces at all: zeros and the points' box
    a0, b0 = meshgen.nodal_areas(s.pos, np.zeros((0, 3), np.int64))
    assert not a0.any() and np.array_equal(b0, bbox)


@pytest.mark.parametrize("n,hole", [(9, 0.0), (13, 0.2), (35, 0.0)])
def test_a_linear_field_is_integrated_exactly(n, hole):
    """P1 exactness: sum_n area_n f(x_n) = sum_f area_f f(centroid_f) = the integral of a linear f over the
    triangulation, which is what makes the lumped weights equal to the reference's Gauss quadrature."""
    from pdg import meshgen
    s = _plate(n, hole)
    area, _ = meshgen.nodal_areas(s.pos, s.faces)
    p = s.pos.astype(np.float64)
    c0, cx, cy = 3.0, -0.7, 0.45
    f = c0 + cx * p[:, 0] + cy * p[:, 1]
    got = float((area.astype(np.float64) * f).sum())
    cen = p[s.faces].mean(1)
    fa = R.face_areas(s.pos, s.faces)
    want = float((fa * (c0 + cx * cen[:, 0] + cy * cen[:, 1])).sum())
    mag = float((area.astype(np.float64) * np.abs(f)).sum())
    assert abs(got - want) <= U32 * mag + 1e-12 * mag


def _batch_case(seed=0):
    rng = np.random.default_rng(seed)
    plates = [_plate(9), _plate(13, 0.2), _plate(12, 0.25)]
    from pdg import meshgen
    areas = [meshgen.nodal_areas(s.pos, s.faces) for s in plates]
    ptr = np.concatenate([[0], np.cumsum([s.num_nodes for s in plates])])
    w = np.concatenate([a for a, _ in areas])
    cell = np.array([_box_area(b) for _, b in areas])
    sigma = rng.normal(0.0, 50.0, (ptr[-1], 3)).astype(np.float32)
    target = rng.normal(0.0, 30.0, (len(plates), 3)).astype(np.float32)
    return ptr, w, cell, sigma, target


@pytest.mark.parametrize("convention", R.CONVENTIONS)
def test_the_corrected_field_has_the_target_average(convention):
    ptr, w, cell, sigma, target = _batch_case()
    w = w.copy()
    w[[3, 100, 200]] = [0.0, -1.0, np.nan]    # excluded rows are shifted too, and count in neither average
    out = R.enforce_mean(ptr, sigma, target, convention, w, cell)
    assert out.shape == sigma.shape
    # graph_wmean takes fp32 rows: average the unrounded field directly
    wk = np.where(w > 0, w, 0.0).astype(np.float64)
    for g in range(len(ptr) - 1):
        sl = slice(ptr[g], ptr[g + 1])
        S = (wk[sl, None] * out[sl]).sum(0)
        D = cell[g] if convention == "cell" else wk[sl].sum()
        scale = (wk[sl, None] * np.abs(out[sl])).sum(0) / D + np.abs(target[g])
        assert np.all(np.abs(S / D - target[g]) <= 1e-12 * scale)
    # the shift is one constant per graph and component
    d = out - sigma
    for g in range(len(ptr) - 1):
        sl = slice(ptr[g], ptr[g + 1])
        assert np.all(np.abs(d[sl] - d[ptr[g]]) <= 1e-12 * np.abs(d[ptr[g]]) + 1e-9)


def test_restatement_rules():
    ptr = np.array([0, 3, 3, 5])
    x = np.array([[1.0], [2.0], [4.0], [8.0], [16.0]], np.float32)
    w = np.array([1.0, 0.0, 2.0, np.nan, -3.0], np.float32)
    table, mag = R.graph_wmean(ptr, x, w)
    assert table.tolist() == [[3.0, 9.0], [0.0, 0.0], [0.0, 0.0]]
    assert R.graph_wmean(ptr, x)[0].tolist() == [[3.0, 7.0], [0.0, 0.0], [2.0, 24.0]]
    avg = R.graph_average(ptr, x, w, cell_area=[6.0, 1.0, 1.0])
    assert avg["mean_material"][0, 0] == 3.0 and avg["mean_cell"][0, 0] == 1.5 and avg["fraction"][0] == 0.5
    assert np.isnan(avg["mean_material"][1:]).all()
    s3 = np.arange(15, dtype=np.float32).reshape(5, 3)
    t3, _ = R.graph_wmean(ptr, s3, w)
    out, sh = R.mean_correct(ptr, s3, t3, np.ones((3, 3), np.float32))
    assert np.isnan(sh[1:]).all() and np.isnan(out[3:]).all() and np.isfinite(out[:3]).all()
    with pytest.raises(ValueError):
        R.enforce_mean(ptr, s3, np.ones((3, 3)), "cell", w, None)
    with pytest.raises(ValueError):
        R.enforce_mean(ptr, s3, np.ones((3, 3)), "box", w, [1.0, 1.0, 1.0])


def test_batch_carries_the_areas_when_every_graph_has_them():
    import torch
    from pdg import graph, meshgen
    plates = [_plate(5), _plate(9, 0.25)]
    datas = [graph.sample_to_data(s) for s in plates]
    for d, s in zip(datas, plates):
        a, b = meshgen.nodal_areas(s.pos, s.faces)
        d.node_area = torch.from_numpy(a)
        d.cell_area = torch.tensor([_box_area(b)], dtype=torch.float64)
    b = graph.Batch.from_data_list(datas)
    n = sum(s.num_nodes for s in plates)
    assert b.node_area.shape == (n,) and b.cell_area.shape == (2,) and b.cell_area.dtype == torch.float64
    assert torch.equal(b.node_area[:plates[0].num_nodes], datas[0].node_area)
    one = b[1]
    assert torch.equal(one.node_area, datas[1].node_area) and torch.equal(one.cell_area, datas[1].cell_area)
    del datas[0].node_area, datas[0].cell_area
    b = graph.Batch.from_data_list(datas)
    assert b.node_area is None and b.cell_area is None
