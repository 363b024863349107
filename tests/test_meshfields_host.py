"""The host restatement of compute_node_labels (pdg.meshgen.node_labels: boundary edges, union-find,
bounding-box test) against hole_plate's own labels (the square-plate rule of the synthetic
generator): two independent derivations of the same field.  pdg_node_labels on the device is checked
against the restatement in tests/test_gpu_meshfields.py, which imports the meshes built here."""
import numpy as np
import pytest

PLATES = [(9, 0.25), (24, 0.3), (71, 0.2)]


def plate(n, hole, jitter=True, periodic=True, seed=3):
    from pdg import meshgen
    return meshgen.hole_plate(n=n, hole_radius=hole, jitter=0.15 if jitter else 0.0, periodic=periodic, seed=seed)


def two_hole_plate(n=24, seed=5):
    """A jittered n x n plate without the faces around two centres: (pos, faces, rim node sets)."""
    from pdg import meshgen
    s = meshgen.hole_plate(n=n, hole_radius=0.0, seed=seed)
    holes = []
    keep = np.ones(len(s.faces), bool)
    for cx, cy in ((30.0, 30.0), (70.0, 65.0)):
        inside = np.linalg.norm(s.pos - np.array([cx, cy]), axis=1) < 12.0
        drop = inside[s.faces].any(1)
        keep &= ~drop
        holes.append((inside, drop))
    faces = s.faces[keep]
    used = np.unique(faces.ravel())
    remap = -np.ones(len(s.pos), np.int64)
    remap[used] = np.arange(len(used))
    rims = []
    for inside, drop in holes:
        touched = np.unique(s.faces[drop].ravel())
        rims.append(set(remap[touched[~inside[touched]]].tolist()))
    return s.pos[used], remap[faces], rims


def renumbered(pos, faces, seed=11):
    """The same mesh with its nodes renumbered and its faces shuffled: (pos', faces', perm) with
    node i of the original at perm[i]."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(pos))
    pos2 = np.empty_like(pos)
    pos2[perm] = pos
    faces2 = perm[faces][rng.permutation(len(faces))]
    return pos2, faces2, perm


@pytest.mark.parametrize("n,hole", PLATES)
@pytest.mark.parametrize("jitter", [True, False])
@pytest.mark.parametrize("periodic", [True, False])
def test_restatement_equals_the_generator(n, hole, jitter, periodic):
    from pdg import meshgen
    s = plate(n, hole, jitter, periodic)
    labels, ncomp, next_ = meshgen.node_labels(s.pos, s.faces)
    assert labels.dtype == np.int64 and labels.shape == (s.num_nodes,)
    assert np.array_equal(labels, s.node_types)
    assert (ncomp, next_) == (2, 1)
    assert set(np.unique(labels).tolist()) == {-1, 0, 1}


def test_plate_without_a_hole_has_one_external_boundary():
    from pdg import meshgen
    s = plate(9, 0.0)
    labels, ncomp, next_ = meshgen.node_labels(s.pos, s.faces)
    assert (ncomp, next_) == (1, 1)
    assert np.array_equal(labels, s.node_types) and -1 not in labels


def test_two_holes_are_two_internal_boundaries():
    from pdg import meshgen
    pos, faces, rims = two_hole_plate()
    labels, ncomp, next_ = meshgen.node_labels(pos, faces)
    # the construction is only a two-hole plate if the rims touch neither each other nor the outer side
    assert rims[0] and rims[1] and not (rims[0] & rims[1])
    outer = np.where(labels == 1)[0]
    on_box = ((pos[:, 0] == pos[:, 0].min()) | (pos[:, 0] == pos[:, 0].max())
              | (pos[:, 1] == pos[:, 1].min()) | (pos[:, 1] == pos[:, 1].max()))
    assert set(outer.tolist()) == set(np.where(on_box)[0].tolist())
    assert not (set(outer.tolist()) & (rims[0] | rims[1]))
    fe = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], 0), 1)
    assert not any((a in rims[0] and b in rims[1]) or (a in rims[1] and b in rims[0]) for a, b in fe.tolist())
    assert (ncomp, next_) == (3, 1)
    for rim in rims:
        assert np.all(labels[sorted(rim)] == -1)
    assert set(np.where(labels == -1)[0].tolist()) == rims[0] | rims[1]


@pytest.mark.parametrize("n,hole", PLATES)
def test_renumbering_permutes_the_labels(n, hole):
    from pdg import meshgen
    s = plate(n, hole)
    pos2, faces2, perm = renumbered(s.pos, s.faces)
    a, ca, ea = meshgen.node_labels(s.pos, s.faces)
    b, cb, eb = meshgen.node_labels(pos2, faces2)
    assert np.array_equal(b[perm], a) and (ca, ea) == (cb, eb)


def test_unused_nodes_and_third_coordinate():
    """A node of no face is 0 even on the bounding box; only x and y are read."""
    from pdg import meshgen
    s = plate(9, 0.25)
    pos = np.concatenate([s.pos, np.array([[200.0, 200.0]], np.float32)])
    labels, ncomp, next_ = meshgen.node_labels(pos, s.faces)
    assert labels[-1] == 0
    # the left and lower sides still lie on the box, so the outer boundary stays external
    assert (ncomp, next_) == (2, 1) and np.array_equal(labels[:-1], s.node_types)
    # with a second free node on the other corner no side lies on the box: both boundaries are internal
    pos = np.concatenate([pos, np.array([[-200.0, -200.0]], np.float32)])
    labels, ncomp, next_ = meshgen.node_labels(pos, s.faces)
    assert (ncomp, next_) == (2, 0) and set(np.unique(labels).tolist()) == {-1, 0}
    pts3 = np.concatenate([s.pos, np.full((s.num_nodes, 1), 7.0, np.float32)], 1)
    assert np.array_equal(meshgen.node_labels(pts3, s.faces)[0], s.node_types)
