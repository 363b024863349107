"""Mesh graph construction on the device.

The reference builds every sample's graph on the host before training or
inference (``scripts/benchmark_gnn_fem.py:388-415`` ``convert_mesh_to_graph``, the
"with preprocessing" series; ``datasets.py:247-263``): PyG ``FaceToEdge``
(``convert_utils.py:47-60``), Euclidean edge lengths (``datasets.py:182-188``) and
``compute_periodic_graph`` (``datasets.py:39-119``), then ``.to(device)``.  Here the
mesh goes to HBM as it is (points, triangles) and one ``pdg_mesh_graph`` call
builds the coalesced periodic graph there (csrc/pdg_graph.hip): bitwise the
host restatement's ``edge_index`` and ``edge_attr`` (``tests/test_gpu_devgraph.py``).

Quad meshes (``convert_utils.py:63-81``, the hyperelastic dataset's cells) are opt-in: every
function here takes ``cells``, ``"triangle"`` by default -- faces must be (F, 3), as they always
had to be, and a quad array is refused; ``"quad"`` takes (F, 4); ``"any"`` decides by
``faces.shape[1]``, which is what a VTK file's reader returns.  The default stays strict
because an (F, 4) array handed to code written for triangles is more often a mistake than a quad
mesh.  Quads run the ``*_cells`` entry points (the same kernels, templates on the vertices per
face); triangles run the entry points they always ran (``tests/test_gpu_quadmesh.py``).
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from .graph import Data
from .lib import lib, stream_handle

SIDE_MAX = 4096
CELLS = ("triangle", "quad", "any")


def _nv(fcs: torch.Tensor, cells: str) -> int:
    """Vertices per face (3 or 4) of ``fcs`` under ``cells``; ValueError when the array is not what ``cells``
    admits.  An array of no faces passes with any width."""
    if cells not in CELLS:
        raise ValueError(f"cells must be one of {CELLS}, got {cells!r}")
    width = fcs.shape[1] if fcs.dim() == 2 else -1
    if fcs.dim() == 2 and fcs.shape[0] == 0:
        return 4 if cells == "quad" or (cells == "any" and width == 4) else 3
    if cells == "triangle" and width != 3:
        raise ValueError("points must be (N, 2|3) and faces (F, 3): triangle meshes only"
                         + (" by default; pass cells='quad' (or cells='any') for a quad mesh" if width == 4 else ""))
    if cells == "quad" and width != 4:
        raise ValueError(f"cells='quad' takes faces of shape (F, 4), got {tuple(fcs.shape)}")
    if width not in (3, 4):
        raise ValueError(f"faces must be (F, 3) triangles or (F, 4) quads, got {tuple(fcs.shape)}")
    return width


def mesh_graph(points: torch.Tensor, faces: torch.Tensor, periodic: bool = True, cells: str = "triangle"):
    """Coalesced ``edge_index`` (2, E) int64 and ``edge_attr`` (E,) float32 of a triangle
    mesh on the device: FaceToEdge + lengths [+ periodic connections with zero length].
    ``points`` (N, 2|3) float32 and ``faces`` (F, 3) int64 on a HIP device.  Raises
    ValueError for geometry ``compute_periodic_graph`` cannot pair and for a face index outside the
    mesh (one host sync).  ``cells`` (module docstring): a quad mesh's (F, 4) faces give the four
    sides of every quad, never a diagonal (``_quad_face_to_edge``, ``pdg_mesh_graph_cells``)."""
    if points.device.type != "cuda" or faces.device.type != "cuda":
        raise RuntimeError("mesh_graph needs device tensors (the HIP path has no CPU fallback)")
    pts = points.contiguous().float()
    fcs = faces.contiguous().to(torch.int64)
    if pts.dim() != 2 or pts.shape[1] not in (2, 3):
        raise ValueError("points must be (N, 2|3) and faces (F, 3)")
    nv = _nv(fcs, cells)
    n, dim = pts.shape
    nf = fcs.shape[0]
    dev = pts.device
    nbytes = lib.pdg_mesh_graph_scratch_bytes(n, nf) if nv == 3 else lib.pdg_mesh_graph_cells_scratch_bytes(n, nf, nv)
    if nbytes < 0:
        raise ValueError("empty mesh")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    cap = 2 * nv * nf + (4 * SIDE_MAX + 4 if periodic else 0)
    ei = torch.empty(2, max(cap, 1), dtype=torch.int64, device=dev)
    ea = torch.empty(max(cap, 1), dtype=torch.float32, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    fptr = fcs.data_ptr() if nf else None
    if nv == 3:
        lib.pdg_mesh_graph(n, pts.data_ptr(), dim, nf, fptr, int(periodic), ei[0].data_ptr(), ei[1].data_ptr(),
                           ea.data_ptr(), cap, cnt.data_ptr(), scratch.data_ptr(), nbytes, stream_handle(dev))
    else:
        lib.pdg_mesh_graph_cells(n, pts.data_ptr(), dim, nf, nv, fptr, int(periodic), ei[0].data_ptr(),
                                 ei[1].data_ptr(), ea.data_ptr(), cap, cnt.data_ptr(), scratch.data_ptr(), nbytes,
                                 stream_handle(dev))
    e = int(cnt.item())
    if e == -2:
        raise ValueError(f"faces hold a node index outside [0, {n})")
    if e < 0:
        raise ValueError("periodic graph: opposite sides must hold the same number of nodes, each corner "
                         f"exactly one node, each side at most {SIDE_MAX} nodes (datasets.py:39-119)")
    return ei[:, :e].contiguous(), ea[:e].clone()


def _mesh_tensors(points: torch.Tensor, faces: torch.Tensor, what: str, cells: str = "triangle", bvec: bool = False):
    """(points, faces, nv, scratch, its size) for a mesh-field call; ``bvec``: the boundary vectors' scratch."""
    if points.device.type != "cuda" or faces.device.type != "cuda":
        raise RuntimeError(f"{what} needs device tensors (the HIP path has no CPU fallback)")
    pts = points.contiguous().float()
    fcs = faces.contiguous().to(torch.int64)
    if pts.dim() != 2 or pts.shape[1] not in (2, 3) or fcs.dim() != 2:
        raise ValueError("points must be (N, 2|3) and faces (F, 3): triangle meshes only")
    nv = _nv(fcs, cells)
    n, nf = pts.shape[0], fcs.shape[0]
    if nv == 3:
        nbytes = lib.pdg_boundary_vectors_scratch_bytes(n, nf) if bvec else lib.pdg_mesh_fields_scratch_bytes(n, nf)
    elif bvec:
        nbytes = lib.pdg_boundary_vectors_cells_scratch_bytes(n, nf, nv)
    else:
        nbytes = lib.pdg_mesh_fields_cells_scratch_bytes(n, nf, nv)
    if nbytes < 0:
        raise ValueError("empty mesh, or a mesh beyond int32 indexing")
    return pts, fcs, nv, torch.empty(nbytes, dtype=torch.uint8, device=pts.device), nbytes


def _call(name: str, nv: int, n: int, pts: torch.Tensor, dim: int, nf: int, fcs: torch.Tensor, *rest):
    """``pdg_<name>`` for triangles, ``pdg_<name>_cells`` (with nv after n_faces) otherwise; the P1 operator's
    triangle entry point keeps its own name."""
    fptr = fcs.data_ptr() if nf else None
    if nv == 3:
        getattr(lib, "pdg_p1_div_operator" if name == "div_operator" else f"pdg_{name}")(
            n, pts.data_ptr(), dim, nf, fptr, *rest)
    else:
        getattr(lib, f"pdg_{name}_cells")(n, pts.data_ptr(), dim, nf, nv, fptr, *rest)


def node_labels(points: torch.Tensor, faces: torch.Tensor, strict: bool = True,
                cells: str = "triangle") -> torch.Tensor:
    """``compute_node_labels`` (``datasets.py:122-179``) on the device (``pdg_node_labels``,
    csrc/pdg_meshfields.hip): (N,) int64 with +1 on the external boundary, -1 on an internal
    boundary (a hole's rim) and 0 elsewhere; bitwise ``pdg.meshgen.node_labels``.  One host
    read (the three status words).  Raises ValueError for a face index outside the mesh and for
    a boundary that is not a set of closed curves (a boundary node with other than two boundary
    edges); with ``strict`` also unless the mesh has exactly two boundaries, one of them
    external -- the reference's "Expected 2 regions" assertion.  ``strict=False`` labels a
    plate with any number of holes, none included.  ``cells`` (module docstring): a quad's edges are
    its four sides (``pdg_node_labels_cells``); everything else is as for triangles."""
    pts, fcs, nv, scratch, nbytes = _mesh_tensors(points, faces, "node_labels", cells)
    n, dim = pts.shape
    nf = fcs.shape[0]
    dev = pts.device
    labels = torch.empty(n, dtype=torch.int64, device=dev)
    info = torch.empty(3, dtype=torch.int32, device=dev)
    _call("node_labels", nv, n, pts, dim, nf, fcs, labels.data_ptr(), info.data_ptr(), scratch.data_ptr(), nbytes,
          stream_handle(dev))
    ncomp, next_, status = info.tolist()
    if status & 1:
        raise ValueError(f"faces hold a node index outside [0, {n})")
    if status & 2:
        raise ValueError("non-manifold boundary: a boundary node has other than two boundary edges")
    if status & 4:
        raise RuntimeError("pdg_node_labels: the boundary component search did not converge")
    if strict and (ncomp != 2 or next_ != 1):
        raise ValueError(f"Expected 2 regions (one external, one internal boundary), found {ncomp} "
                         f"({next_} external); strict=False labels any number of holes")
    return labels


_labels_of = node_labels   # convert_mesh_to_graph's `node_labels` argument shadows the function


def p1_divergence(points: torch.Tensor, faces: torch.Tensor, cells: str = "triangle") -> torch.Tensor:
    """The area-averaged P1 divergence operator A = [Dx | Dy] of a triangle mesh as a coalesced
    sparse COO (N, 2N) float32 tensor on the device (``pdg_p1_div_operator``): rows and columns
    bitwise ``pdg.meshgen.p1_divergence_operator``'s, values to one float32 rounding of the same
    fp64 sums.  One host read (entry count and status).  Raises ValueError for a face index
    outside the mesh or a face of zero area.  For a quad mesh (``cells``, module docstring) the same
    function returns the q1 operator: the same construction with the faces' mean Q1 gradients
    (``pdg_div_operator_cells``, ``pdg.meshgen.q1_divergence_operator``), up to 32 entries a face."""
    pts, fcs, nv, scratch, nbytes = _mesh_tensors(points, faces, "p1_divergence", cells)
    n, dim = pts.shape
    nf = fcs.shape[0]
    dev = pts.device
    cap = 2 * nv * nv * nf
    idx = torch.empty(2, max(cap, 1), dtype=torch.int64, device=dev)
    vals = torch.empty(max(cap, 1), dtype=torch.float32, device=dev)
    cnt = torch.empty(2, dtype=torch.int32, device=dev)
    _call("div_operator", nv, n, pts, dim, nf, fcs, idx[0].data_ptr(), idx[1].data_ptr(), vals.data_ptr(), cap,
          cnt.data_ptr(), cnt[1:].data_ptr(), scratch.data_ptr(), nbytes, stream_handle(dev))
    nnz, status = cnt.tolist()
    if status & 2:
        raise ValueError(f"faces hold a node index outside [0, {n})")
    if status & 1:
        raise ValueError("a face has zero area: the P1 / Q1 gradients are undefined there")
    return torch.sparse_coo_tensor(idx[:, :nnz], vals[:nnz], (n, 2 * n), is_coalesced=True)


cell_divergence = p1_divergence   # the name that fits both cell types


class NodalAreas(NamedTuple):
    """``area`` (N,) float32: the lumped nodal areas; ``cell_area`` (1,) float64: the bounding box's area,
    (xmax - xmin)(ymax - ymin) formed in fp64 from the float32 extremes.  Both on the device."""
    area: torch.Tensor
    cell_area: torch.Tensor


def nodal_areas(points: torch.Tensor, faces: torch.Tensor, cells: str = "triangle") -> NodalAreas:
    """The quadrature weights of the reference's volume averages on the device (``pdg_nodal_areas``,
    csrc/pdg_meshfields.hip): ``area[n]`` is the sum of area / 3 over the triangles that hold node n, to one
    float32 ulp of ``pdg.meshgen.nodal_areas`` (the same fp64 terms in the same order), and ``area / cell_area``
    is the reference's ``op_mean_stress`` (``scripts/generate_dataset.py:73-82``).  A node of no face gets 0, a
    face of zero area adds 0.  One host read (the status word).  Raises ValueError for a face index outside the
    mesh.  For a quad mesh (``cells``, module docstring) ``area[n]`` is the sum of the exact integrals of the
    bilinear N_n over the quads that hold n (``pdg_nodal_areas_cells``: area / 4 on a parallelogram, the 2 x 2
    Gauss weights gathered to the nodes)."""
    pts, fcs, nv, scratch, nbytes = _mesh_tensors(points, faces, "nodal_areas", cells)
    n, dim = pts.shape
    nf = fcs.shape[0]
    dev = pts.device
    area = torch.empty(n, dtype=torch.float32, device=dev)
    bbox = torch.empty(4, dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    _call("nodal_areas", nv, n, pts, dim, nf, fcs, area.data_ptr(), bbox.data_ptr(), status.data_ptr(),
          scratch.data_ptr(), nbytes, stream_handle(dev))
    if int(status.item()) & 1:
        raise ValueError(f"faces hold a node index outside [0, {n})")
    b = bbox.double()
    return NodalAreas(area, ((b[1] - b[0]) * (b[3] - b[2])).reshape(1))


class BoundaryVectors(NamedTuple):
    """``vec`` (N, 2) float32: the lumped outward boundary vectors, 1/2 sum length * n_outward over the boundary
    edges at a node; ``length`` (N,) float32: 1/2 sum length.  Both on the device, zero off the boundary."""
    vec: torch.Tensor
    length: torch.Tensor


def boundary_vectors(points: torch.Tensor, faces: torch.Tensor, cells: str = "triangle") -> BoundaryVectors:
    """The quadrature of the boundary tractions on the device (``pdg_boundary_vectors``,
    csrc/pdg_meshfields.hip): ``sigma(n) . vec[n]`` is the nodal boundary force, the lumped traction integral;
    to one float32 ulp of ``pdg.meshgen.boundary_vectors`` (the same fp64 terms in the same order).  One host
    read (the status word).  Raises ValueError for a face index outside the mesh and for a boundary node with
    other than two boundary edges; a boundary edge of a face of zero area is no error (it adds its length and no
    vector).  For a quad mesh (``cells``, module docstring) a boundary edge is a side of exactly one quad, oriented
    away from the vertex after it (``pdg_boundary_vectors_cells``)."""
    pts, fcs, nv, scratch, nbytes = _mesh_tensors(points, faces, "boundary_vectors", cells, bvec=True)
    n, dim = pts.shape
    nf = fcs.shape[0]
    dev = pts.device
    vec = torch.empty(n, 2, dtype=torch.float32, device=dev)
    length = torch.empty(n, dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    _call("boundary_vectors", nv, n, pts, dim, nf, fcs, vec.data_ptr(), length.data_ptr(), status.data_ptr(),
          scratch.data_ptr(), nbytes, stream_handle(dev))
    st = int(status.item())
    if st & 1:
        raise ValueError(f"faces hold a node index outside [0, {n})")
    if st & 2:
        raise ValueError("non-manifold boundary: a boundary node has other than two boundary edges")
    return BoundaryVectors(vec, length)


MESH_FIELDS = ("node_area", "cell_area", "boundary_vec", "boundary_len")


def attach_mesh_fields(data: Data, device, cells: str = "any") -> Data:
    """Set ``node_area`` (N,), ``cell_area`` (1,) fp64, ``boundary_vec`` (N, 2) and ``boundary_len`` (N,) on ``data``
    from its ``pos`` and ``face`` (the (3|4, F) layout of FaceToEdge), computed on the HIP ``device`` by
    ``nodal_areas`` and ``boundary_vectors`` and kept where ``data.pos`` lives: what ``Batch.from_data_list`` and
    ``DeviceGraphStore(..., mesh_fields=True)`` carry into a minibatch for the trainer's physics penalties
    (``pdg.trainer.PhysicsPenalty``).  Returns ``data``."""
    if device is None or torch.device(device).type != "cuda":
        raise RuntimeError("attach_mesh_fields computes on a HIP device (the HIP path has no CPU fallback)")
    pos, face = data.__dict__.get("pos"), data.__dict__.get("face")
    if pos is None or face is None:
        raise ValueError("attach_mesh_fields needs the mesh: data.pos (N, 2) and data.face (3|4, F)")
    pts = pos.to(device).float()
    fcs = face.to(device).T.contiguous()
    area = nodal_areas(pts, fcs, cells)
    bv = boundary_vectors(pts, fcs, cells)
    home = pos.device
    data.node_area, data.cell_area = area.area.to(home), area.cell_area.to(home)
    data.boundary_vec, data.boundary_len = bv.vec.to(home), bv.length.to(home)
    return data


def convert_mesh_to_graph(points: torch.Tensor, faces: torch.Tensor, mean_stress,
                          node_labels: torch.Tensor | None = None, periodic: bool = True,
                          divergence: bool = False, areas: bool = False, boundary: bool = False,
                          cells: str = "triangle") -> Data:
    """``benchmark_gnn_fem.py:388-415`` on the device: the graph of one FEM sample, ready for
    ``EncodeProcessDecode`` (pos reduced to (x, y) float32, mean stress broadcast to every
    node, node labels as both ``surfaces_nodes_for_div`` and ``nodes_types``).  Without
    ``node_labels`` they are computed from the mesh on the device (``node_labels`` above,
    strict); ``divergence`` also sets ``op_div_matrix`` (``p1_divergence``); ``areas`` also sets
    ``node_area`` (N,) and ``cell_area`` (1,) (``nodal_areas``), the weights and the cell of the volume
    averages of ``gnn_local_stress.homogenise``; ``boundary`` also sets ``boundary_vec`` (N, 2) and
    ``boundary_len`` (N,) (``boundary_vectors``), the quadrature of ``gnn_local_stress.boundary``.  ``cells``
    (module docstring) goes to every one of them: a quad mesh gets its own graph, labels, q1 operator, areas and
    boundary vectors; the model and everything after it see nodes and edges only."""
    edge_index, edge_attr = mesh_graph(points, faces, periodic, cells)
    n = points.shape[0]
    dev = points.device
    if node_labels is None:
        node_labels = _labels_of(points, faces, cells=cells)
    labels = node_labels.to(dev).reshape(-1, 1).to(torch.int64)
    ms = torch.as_tensor(mean_stress, dtype=torch.float32, device=dev).reshape(1, 3)
    out = Data(edge_index=edge_index, edge_attr=edge_attr, pos=points[:, :2].float().contiguous(),
               face=faces.T.contiguous(), mean_stress=torch.ones(n, 3, device=dev) * ms,
               surfaces_nodes_for_div=labels, nodes_types=labels.clone(), is_periodic=periodic)
    if divergence:
        out.op_div_matrix = p1_divergence(points, faces, cells)
    if areas:
        out.node_area, out.cell_area = nodal_areas(points, faces, cells)
    if boundary:
        out.boundary_vec, out.boundary_len = boundary_vectors(points, faces, cells)
    return out
