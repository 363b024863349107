"""Small irregular meshes for the device geometry code: deterministic numpy generators, no GPU.

pdg.meshgen's plates are structured grids: a triangle node touches at most 8 faces, a quad node 4.  The meshes here
have what an unstructured mesh has and a grid has not: a hub node of any valence (fan_disk, quad_fan, pinwheel), a
hole rim whose node ids are scattered (fan_annulus renumbered), valences from 3 to 16 side by side (refined_plate)
and a periodic pair that is also a mesh edge (two_column_strip).  Every generator returns an ``Irregular`` with
float32 positions, int64 faces of positive determinant, and what its construction says about the result: the
labels, the hub, the rings in order.  ``renumber=seed`` gives the same mesh with random node ids and a shuffled face
order (tests/test_meshfields_host.py's ``renumbered``), the construction's facts renumbered with it.

Checked by tests/test_irregular_meshes_host.py against pdg.meshgen's restatements; fed to the device by
tests/test_gpu_irregular_mesh.py."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

CENTRE = (50.0, 50.0)
RING_STEP = 20.0       # ring j of a fan has radius j * RING_STEP


@dataclass
class Irregular:
    pos: np.ndarray                 # (N, 2) float32
    faces: np.ndarray               # (F, 3|4) int64, counter-clockwise
    labels: np.ndarray              # (N,) int64: what compute_node_labels must return, from the construction
    hub: int | None = None          # the high-valence node
    rings: list = field(default_factory=list)   # node ids of each ring, in counter-clockwise order, innermost first
    perm: np.ndarray | None = None  # renumber: node i of the orderly mesh is node perm[i]

    @property
    def num_nodes(self) -> int:
        return len(self.pos)


def determinants(pos, faces) -> np.ndarray:
    """meshgen's det of every face (2 x the signed area), fp64 from the float32 coordinates."""
    p = np.asarray(pos, np.float32).astype(np.float64)
    x, y = p[faces, 0], p[faces, 1]
    if faces.shape[1] == 4:
        return (x[:, 2] - x[:, 0]) * (y[:, 3] - y[:, 1]) - (x[:, 3] - x[:, 1]) * (y[:, 2] - y[:, 0])
    return (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])


def valences(faces, n) -> np.ndarray:
    """Faces per node."""
    return np.bincount(np.asarray(faces).ravel(), minlength=n)


def boundary_loops(faces) -> list:
    """The closed boundary curves of a manifold mesh as node-id arrays, each in the direction its faces give it
    (counter-clockwise faces: the outer boundary counter-clockwise, a hole's rim clockwise).  A side (a, b) is a
    boundary side when (b, a) is the side of no face."""
    nv = faces.shape[1]
    sides = np.concatenate([faces[:, [j, (j + 1) % nv]] for j in range(nv)], 0)
    have = set(map(tuple, sides.tolist()))
    nxt = {}
    for a, b in sides.tolist():
        if (b, a) not in have:
            assert a not in nxt, "non-manifold boundary"
            nxt[a] = b
    loops = []
    while nxt:
        start = min(nxt)
        loop, a = [], start
        while a in nxt:
            loop.append(a)
            a = nxt.pop(a)
        assert a == start, "open boundary"
        loops.append(np.array(loop, np.int64))
    return loops


def polygon_area(pos, loop) -> float:
    """The signed shoelace area of the closed curve ``loop``, fp64 from the float32 coordinates, taken about the
    curve's first point so that the products stay of the size of the polygon."""
    p = np.asarray(pos, np.float32).astype(np.float64)[loop, :2]
    q = p - p[0]
    x, y = q[:, 0], q[:, 1]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))


def material_area(m: Irregular) -> float:
    """The area the faces cover, from the boundary curves alone: outer polygon minus the holes."""
    return sum(polygon_area(m.pos, loop) for loop in boundary_loops(m.faces))


def _finish(pos, faces, labels, hub=None, rings=(), renumber=None) -> Irregular:
    pos = np.ascontiguousarray(pos, np.float32)
    faces = np.ascontiguousarray(faces, np.int64)
    labels = np.asarray(labels, np.int64)
    rings = [np.asarray(r, np.int64) for r in rings]
    perm = None
    if renumber is not None:
        from test_meshfields_host import renumbered
        pos, faces, perm = renumbered(pos, faces, seed=renumber)
        out = np.empty_like(labels)
        out[perm] = labels
        labels = out
        hub = None if hub is None else int(perm[hub])
        rings = [perm[r] for r in rings]
    assert np.all(determinants(pos, faces) > 0)
    return Irregular(pos, faces, labels, hub, rings, perm)


def _ring_points(k, radius, phase):
    a = 2.0 * np.pi * (np.arange(k) + phase) / k
    return np.stack([CENTRE[0] + radius * np.cos(a), CENTRE[1] + radius * np.sin(a)], 1)


def _fan(k, rings):
    """Hub 0, ring j = 1..rings at nodes 1 + (j - 1) k + i, alternate rings rotated by half a step."""
    assert k >= 3 and rings >= 1
    pos = [np.array([CENTRE])]
    ids = []
    for j in range(1, rings + 1):
        pos.append(_ring_points(k, j * RING_STEP, 0.5 * ((j - 1) % 2)))
        ids.append(1 + (j - 1) * k + np.arange(k))
    i = np.arange(k)
    nx = (i + 1) % k
    faces = [np.stack([np.zeros(k, np.int64), ids[0][i], ids[0][nx]], 1)]
    for j in range(1, rings):
        inner, outer = ids[j - 1], ids[j]
        # the outer node between inner[i] and inner[i + 1]: outer[i] when the outer ring is the rotated one
        o = i if j % 2 == 1 else nx
        faces.append(np.stack([inner[i], outer[o], inner[nx]], 1))
        faces.append(np.stack([outer[o], outer[(o + 1) % k], inner[nx]], 1))
    return np.concatenate(pos), np.concatenate(faces), ids


def _swap(pos, faces, labels, a, b):
    """Exchange node ids a and b."""
    m = np.arange(len(pos))
    m[[a, b]] = [b, a]
    pos2 = pos.copy()
    pos2[[a, b]] = pos[[b, a]]
    lab2 = labels.copy()
    lab2[[a, b]] = labels[[b, a]]
    return pos2, m[faces], lab2, m


def fan_disk(k, rings=2, hub_id=0, renumber=None) -> Irregular:
    """A hub at the centre and ``rings`` rings of k nodes: 1 + k rings nodes, k + 2 k (rings - 1) triangles.  The hub
    touches k faces.  ``hub_id``: 0, or N - 1 (also -1), the hub's node id, by a swap with that node."""
    pos, faces, ids = _fan(k, rings)
    n = len(pos)
    labels = np.zeros(n, np.int64)
    labels[ids[-1]] = 1
    hub = 0
    if hub_id in (-1, n - 1):
        pos, faces, labels, m = _swap(pos, faces, labels, 0, n - 1)
        ids = [m[r] for r in ids]
        hub = n - 1
    else:
        assert hub_id == 0
    return _finish(pos, faces, labels, hub, ids, renumber)


def fan_annulus(k, rings=2, renumber=None) -> Irregular:
    """fan_disk without the hub and its faces: the inner ring is a hole's rim of k nodes, the outer one external."""
    assert rings >= 2
    pos, faces, ids = _fan(k, rings)
    pos, faces, ids = pos[1:], faces[k:] - 1, [r - 1 for r in ids]
    labels = np.zeros(len(pos), np.int64)
    labels[ids[0]] = -1
    labels[ids[-1]] = 1
    return _finish(pos, faces, labels, None, ids, renumber)


def quad_fan(k, renumber=None) -> Irregular:
    """A hub, a ring of 2 k nodes, the k quads (hub, r[2i], r[2i+1], r[2i+2]) and an outer ring of 2 k quads:
    1 + 4 k nodes, 3 k quads.  The hub touches k quads (at k = 2 its two corners are straight angles: the quads are
    triangles in shape, with a non-zero det)."""
    assert k >= 2
    m = 2 * k
    pos = np.concatenate([np.array([CENTRE]), _ring_points(m, RING_STEP, 0.0), _ring_points(m, 2 * RING_STEP, 0.0)])
    r, o = 1 + np.arange(m), 1 + m + np.arange(m)
    i = 2 * np.arange(k)
    j = np.arange(m)
    faces = np.concatenate([np.stack([np.zeros(k, np.int64), r[i], r[i + 1], r[(i + 2) % m]], 1),
                            np.stack([r[j], o[j], o[(j + 1) % m], r[(j + 1) % m]], 1)])
    labels = np.zeros(len(pos), np.int64)
    labels[o] = 1
    return _finish(pos, faces, labels, 0, [r, o], renumber)


def pinwheel(k, renumber=None) -> Irregular:
    """Every other sector of a fan: a hub, a ring of 2 k nodes and the k triangles (hub, r[2i], r[2i+1]), which meet
    only at the hub.  The boundary is not a set of closed curves: the hub has 2 k boundary edges, so its row of the
    boundary edges' grouping by node is as long as one likes (on a manifold mesh such a row holds 2).  One external
    boundary component."""
    assert k >= 2
    m = 2 * k
    pos = np.concatenate([np.array([CENTRE]), _ring_points(m, RING_STEP, 0.0)])
    i = 2 * np.arange(k)
    faces = np.stack([np.zeros(k, np.int64), 1 + i, 2 + i], 1)
    return _finish(pos, faces, np.ones(len(pos), np.int64), 0, [1 + np.arange(m)], renumber)


def refined_plate(n, hole, periodic=True, splits=40, flips=30, seed=3, renumber=None) -> Irregular:
    """hole_plate(n, hole) made irregular.  ``splits`` interior faces get their centroid as a new node (1 -> 3): first
    every face around each of three interior vertices (valence 8 becomes 16, 6 becomes 12), then faces drawn at random.
    Then ``flips`` interior edges whose two triangles form a strictly convex quadrilateral are flipped.  Only faces and
    edges whose nodes are all interior are touched: the sides keep their nodes, so periodic_pairs still holds, and the
    labels are hole_plate's with 0 for the new nodes."""
    from pdg import meshgen
    s = meshgen.hole_plate(n=n, hole_radius=hole, periodic=periodic, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    pos = [p for p in s.pos.astype(np.float64)]
    faces = [tuple(f) for f in s.faces.tolist()]
    inner = s.node_types == 0
    inner_face = inner[s.faces].all(1)
    # vertices whose faces are all interior, the highest valence first
    val = valences(s.faces, s.num_nodes)
    full = np.bincount(s.faces[inner_face].ravel(), minlength=s.num_nodes) == val
    cand = np.where(inner & full)[0]
    cand = cand[np.argsort(-val[cand], kind="stable")]
    centres = []
    for v in cand.tolist():      # three of them, no two in one face
        if all(not np.any((s.faces == v).any(1) & (s.faces == c).any(1)) for c in centres):
            centres.append(v)
        if len(centres) == 3:
            break
    assert len(centres) == 3
    chosen = [f for c in centres for f in np.where((s.faces == c).any(1))[0].tolist()]
    rest = np.setdiff1d(np.where(inner_face)[0], chosen)
    assert len(chosen) <= splits <= len(chosen) + len(rest)
    chosen += rng.permutation(rest)[:splits - len(chosen)].tolist()
    for f in chosen:
        a, b, c = faces[f]
        m = len(pos)
        pos.append(np.float32((pos[a] + pos[b] + pos[c]) / 3.0).astype(np.float64))
        faces[f] = (a, b, m)
        faces += [(b, c, m), (c, a, m)]
    p = np.array(pos)
    ok_node = np.concatenate([inner, np.ones(len(p) - s.num_nodes, bool)])

    def det(a, b, c):
        return (p[b, 0] - p[a, 0]) * (p[c, 1] - p[a, 1]) - (p[c, 0] - p[a, 0]) * (p[b, 1] - p[a, 1])

    for _ in range(flips):
        across = {}      # directed side (a, b) -> (face, the vertex opposite to it)
        for f, (a, b, c) in enumerate(faces):
            across[(a, b)], across[(b, c)], across[(c, a)] = (f, c), (f, a), (f, b)
        edges = sorted(e for e in across if e[0] < e[1] and (e[1], e[0]) in across)
        for e in rng.permutation(len(edges)).tolist():
            a, b = edges[e]
            (f1, c), (f2, d) = across[(a, b)], across[(b, a)]
            if not ok_node[[a, b, c, d]].all():
                continue
            old = det(a, b, c) + det(b, a, d)
            if min(det(a, d, c), det(d, b, c)) > 0.05 * old:     # strictly convex, with a margin
                faces[f1], faces[f2] = (a, d, c), (d, b, c)
                break
        else:
            raise AssertionError("no edge left to flip")
    faces = np.array(faces, np.int64)
    labels = np.concatenate([s.node_types, np.zeros(len(p) - s.num_nodes, np.int64)])
    hist = valences(faces, len(p))
    assert hist.min() < 5 and hist.max() > 8, "the refinement left a regular mesh"
    return _finish(p, faces, labels, int(np.argmax(hist)), [], renumber)


def two_column_strip(rows=7, length=100.0, renumber=None) -> Irregular:
    """A periodic plate two nodes wide and ``rows`` high: every left-right periodic pair (L_j, R_j) is also a mesh
    edge, so its coalesced attribute is the sum of the length and of the pair's 0.  Every node is on a side."""
    assert rows >= 3
    h = length / (rows - 1)
    j = np.arange(rows)
    pos = np.concatenate([np.stack([np.zeros(rows), j * h], 1), np.stack([np.full(rows, h), j * h], 1)])
    lo, hi = j[:-1], j[:-1] + 1                # L_j = j, R_j = rows + j
    even = (lo % 2 == 0)[:, None]
    t1 = np.where(even, np.stack([lo, rows + lo, rows + hi], 1), np.stack([lo, rows + lo, hi], 1))
    t2 = np.where(even, np.stack([lo, rows + hi, hi], 1), np.stack([rows + lo, rows + hi, hi], 1))
    return _finish(pos, np.concatenate([t1, t2]), np.ones(2 * rows, np.int64), None, [], renumber)


def host_graph(pos, faces, periodic):
    """The reference's graph build restated on the host, as tests/test_gpu_devgraph.py does: FaceToEdge + coalesce,
    torch.linalg.vector_norm lengths, periodic pairs with attribute 0, coalesced with summed attributes."""
    import torch
    from pdg import meshgen
    n = len(pos)
    ei = meshgen.quad_faces_to_edges(faces, n) if faces.shape[1] == 4 else meshgen.faces_to_edges(faces, n)
    p = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float32))
    ea = torch.linalg.vector_norm(p[torch.from_numpy(ei[0])] - p[torch.from_numpy(ei[1])], dim=1).numpy()
    if periodic:
        pr, pc = meshgen.periodic_pairs(pos[:, :2])
        ei, ea = meshgen.coalesce(np.concatenate([ei, np.stack([pr, pc])], 1),
                                  np.concatenate([ea, np.zeros(len(pr), np.float32)]), n)
    return ei, ea
