"""Mesh graph construction on the device.

The reference builds every sample's graph on the host before training or
inference (``scripts/benchmark_gnn_fem.py:388-415`` ``convert_mesh_to_graph``, the
"with preprocessing" series; ``datasets.py:247-263``): PyG ``FaceToEdge``
(``convert_utils.py:47-60``), Euclidean edge lengths (``datasets.py:182-188``) and
``compute_periodic_graph`` (``datasets.py:39-119``), then ``.to(device)``.  Here the
mesh goes to HBM as it is (points, triangles) and one ``pdg_mesh_graph`` call
builds the coalesced periodic graph there (csrc/pdg_graph.hip): bitwise the
host restatement's ``edge_index`` and ``edge_attr`` (``tests/test_gpu_devgraph.py``).
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from .graph import Data
from .lib import lib, stream_handle

SIDE_MAX = 4096


def mesh_graph(points: torch.Tensor, faces: torch.Tensor, periodic: bool = True):
    """Coalesced ``edge_index`` (2, E) int64 and ``edge_attr`` (E,) float32 of a triangle
    mesh on the device: FaceToEdge + lengths [+ periodic connections with zero length].
    ``points`` (N, 2|3) float32 and ``faces`` (F, 3) int64 on a HIP device.  Raises
    ValueError for geometry ``compute_periodic_graph`` cannot pair (one host sync)."""
    if points.device.type != "cuda" or faces.device.type != "cuda":
        raise RuntimeError("mesh_graph needs device tensors (the HIP path has no CPU fallback)")
    pts = points.contiguous().float()
    fcs = faces.contiguous().to(torch.int64)
    n, dim = pts.shape
    nf = fcs.shape[0]
    if dim not in (2, 3) or (nf and fcs.shape[1] != 3):
        raise ValueError("points must be (N, 2|3) and faces (F, 3)")
    dev = pts.device
    nbytes = lib.pdg_mesh_graph_scratch_bytes(n, nf)
    if nbytes < 0:
        raise ValueError("empty mesh")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    cap = 6 * nf + (4 * SIDE_MAX + 4 if periodic else 0)
    ei = torch.empty(2, max(cap, 1), dtype=torch.int64, device=dev)
    ea = torch.empty(max(cap, 1), dtype=torch.float32, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    lib.pdg_mesh_graph(n, pts.data_ptr(), dim, nf, fcs.data_ptr() if nf else None, int(periodic), ei[0].data_ptr(),
                       ei[1].data_ptr(), ea.data_ptr(), cap, cnt.data_ptr(), scratch.data_ptr(), nbytes,
                       stream_handle(dev))
    e = int(cnt.item())
    if e < 0:
        raise ValueError("periodic graph: opposite sides must hold the same number of nodes, each corner "
                         f"exactly one node, each side at most {SIDE_MAX} nodes (datasets.py:39-119)")
    return ei[:, :e].contiguous(), ea[:e].clone()


def _mesh_tensors(points: torch.Tensor, faces: torch.Tensor, what: str):
    if points.device.type != "cuda" or faces.device.type != "cuda":
        raise RuntimeError(f"{what} needs device tensors (the HIP path has no CPU fallback)")
    pts = points.contiguous().float()
    fcs = faces.contiguous().to(torch.int64)
    if pts.dim() != 2 or pts.shape[1] not in (2, 3) or fcs.dim() != 2 or (fcs.shape[0] and fcs.shape[1] != 3):
        raise ValueError("points must be (N, 2|3) and faces (F, 3): triangle meshes only")
    nbytes = lib.pdg_mesh_fields_scratch_bytes(pts.shape[0], fcs.shape[0])
    if nbytes < 0:
        raise ValueError("empty mesh, or a mesh beyond int32 indexing")
    return pts, fcs, torch.empty(nbytes, dtype=torch.uint8, device=pts.device), nbytes


def node_labels(points: torch.Tensor, faces: torch.Tensor, strict: bool = True) -> torch.Tensor:
    """``compute_node_labels`` (``datasets.py:122-179``) on the device (``pdg_node_labels``,
    csrc/pdg_meshfields.hip): (N,) int64 with +1 on the external boundary, -1 on an internal
    boundary (a hole's rim) and 0 elsewhere; bitwise ``pdg.meshgen.node_labels``.  One host
    read (the three status words).  Raises ValueError for a face index outside the mesh and for
    a boundary that is not a set of closed curves (a boundary node with other than two boundary
    edges); with ``strict`` also unless the mesh has exactly two boundaries, one of them
    external -- the reference's "Expected 2 regions" assertion.  ``strict=False`` labels a
    plate with any number of holes, none included."""
    pts, fcs, scratch, nbytes = _mesh_tensors(points, faces, "node_labels")
    n, dim = pts.shape
    nf = fcs.shape[0]
    dev = pts.device
    labels = torch.empty(n, dtype=torch.int64, device=dev)
    info = torch.empty(3, dtype=torch.int32, device=dev)
    lib.pdg_node_labels(n, pts.data_ptr(), dim, nf, fcs.data_ptr() if nf else None, labels.data_ptr(),
                        info.data_ptr(), scratch.data_ptr(), nbytes, stream_handle(dev))
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


def p1_divergence(points: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """The area-averaged P1 divergence operator A = [Dx | Dy] of a triangle mesh as a coalesced
    sparse COO (N, 2N) float32 tensor on the device (``pdg_p1_div_operator``): rows and columns
    bitwise ``pdg.meshgen.p1_divergence_operator``'s, values to one float32 rounding of the same
    fp64 sums.  One host read (entry count and status).  Raises ValueError for a face index
    outside the mesh or a face of zero area."""
    pts, fcs, scratch, nbytes = _mesh_tensors(points, faces, "p1_divergence")
    n, dim = pts.shape
    nf = fcs.shape[0]
    dev = pts.device
    cap = 18 * nf
    idx = torch.empty(2, max(cap, 1), dtype=torch.int64, device=dev)
    vals = torch.empty(max(cap, 1), dtype=torch.float32, device=dev)
    cnt = torch.empty(2, dtype=torch.int32, device=dev)
    lib.pdg_p1_div_operator(n, pts.data_ptr(), dim, nf, fcs.data_ptr() if nf else None, idx[0].data_ptr(),
                            idx[1].data_ptr(), vals.data_ptr(), cap, cnt.data_ptr(), cnt[1:].data_ptr(),
                            scratch.data_ptr(), nbytes, stream_handle(dev))
    nnz, status = cnt.tolist()
    if status & 2:
        raise ValueError(f"faces hold a node index outside [0, {n})")
    if status & 1:
        raise ValueError("a face has zero area: the P1 gradients are undefined there")
    return torch.sparse_coo_tensor(idx[:, :nnz], vals[:nnz], (n, 2 * n), is_coalesced=True)


class NodalAreas(NamedTuple):
    """``area`` (N,) float32: the lumped nodal areas; ``cell_area`` (1,) float64: the bounding box's area,
    (xmax - xmin)(ymax - ymin) formed in fp64 from the float32 extremes.  Both on the device."""
    area: torch.Tensor
    cell_area: torch.Tensor


def nodal_areas(points: torch.Tensor, faces: torch.Tensor) -> NodalAreas:
    """The quadrature weights of the reference's volume averages on the device (``pdg_nodal_areas``,
    csrc/pdg_meshfields.hip): ``area[n]`` is the sum of area / 3 over the triangles that hold node n, to one
    float32 ulp of ``pdg.meshgen.nodal_areas`` (the same fp64 terms in the same order), and ``area / cell_area``
    is the reference's ``op_mean_stress`` (``scripts/generate_dataset.py:73-82``).  A node of no face gets 0, a
    face of zero area adds 0.  One host read (the status word).  Raises ValueError for a face index outside the
    mesh.  Triangle meshes only."""
    pts, fcs, scratch, nbytes = _mesh_tensors(points, faces, "nodal_areas")
    n, dim = pts.shape
    nf = fcs.shape[0]
    dev = pts.device
    area = torch.empty(n, dtype=torch.float32, device=dev)
    bbox = torch.empty(4, dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    lib.pdg_nodal_areas(n, pts.data_ptr(), dim, nf, fcs.data_ptr() if nf else None, area.data_ptr(),
                        bbox.data_ptr(), status.data_ptr(), scratch.data_ptr(), nbytes, stream_handle(dev))
    if int(status.item()) & 1:
        raise ValueError(f"faces hold a node index outside [0, {n})")
    b = bbox.double()
    return NodalAreas(area, ((b[1] - b[0]) * (b[3] - b[2])).reshape(1))


class BoundaryVectors(NamedTuple):
    """``vec`` (N, 2) float32: the lumped outward boundary vectors, 1/2 sum length * n_outward over the boundary
    edges at a node; ``length`` (N,) float32: 1/2 sum length.  Both on the device, zero off the boundary."""
    vec: torch.Tensor
    length: torch.Tensor


def boundary_vectors(points: torch.Tensor, faces: torch.Tensor) -> BoundaryVectors:
    """The quadrature of the boundary tractions on the device (``pdg_boundary_vectors``,
    csrc/pdg_meshfields.hip): ``sigma(n) . vec[n]`` is the nodal boundary force, the lumped traction integral;
    to one float32 ulp of ``pdg.meshgen.boundary_vectors`` (the same fp64 terms in the same order).  One host
    read (the status word).  Raises ValueError for a face index outside the mesh and for a boundary node with
    other than two boundary edges; a boundary edge of a face of zero area is no error (it adds its length and no
    vector).  Triangle meshes only."""
    if points.device.type != "cuda" or faces.device.type != "cuda":
        raise RuntimeError("boundary_vectors needs device tensors (the HIP path has no CPU fallback)")
    pts = points.contiguous().float()
    fcs = faces.contiguous().to(torch.int64)
    if pts.dim() != 2 or pts.shape[1] not in (2, 3) or fcs.dim() != 2 or (fcs.shape[0] and fcs.shape[1] != 3):
        raise ValueError("points must be (N, 2|3) and faces (F, 3): triangle meshes only")
    n, dim = pts.shape
    nf = fcs.shape[0]
    dev = pts.device
    nbytes = lib.pdg_boundary_vectors_scratch_bytes(n, nf)
    if nbytes < 0:
        raise ValueError("empty mesh, or a mesh beyond int32 indexing")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    vec = torch.empty(n, 2, dtype=torch.float32, device=dev)
    length = torch.empty(n, dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    lib.pdg_boundary_vectors(n, pts.data_ptr(), dim, nf, fcs.data_ptr() if nf else None, vec.data_ptr(),
                             length.data_ptr(), status.data_ptr(), scratch.data_ptr(), nbytes, stream_handle(dev))
    st = int(status.item())
    if st & 1:
        raise ValueError(f"faces hold a node index outside [0, {n})")
    if st & 2:
        raise ValueError("non-manifold boundary: a boundary node has other than two boundary edges")
    return BoundaryVectors(vec, length)


def convert_mesh_to_graph(points: torch.Tensor, faces: torch.Tensor, mean_stress,
                          node_labels: torch.Tensor | None = None, periodic: bool = True,
                          divergence: bool = False, areas: bool = False, boundary: bool = False) -> Data:
    """``benchmark_gnn_fem.py:388-415`` on the device: the graph of one FEM sample, ready for
    ``EncodeProcessDecode`` (pos reduced to (x, y) float32, mean stress broadcast to every
    node, node labels as both ``surfaces_nodes_for_div`` and ``nodes_types``).  Without
    ``node_labels`` they are computed from the mesh on the device (``node_labels`` above,
    strict); ``divergence`` also sets ``op_div_matrix`` (``p1_divergence``); ``areas`` also sets
    ``node_area`` (N,) and ``cell_area`` (1,) (``nodal_areas``), the weights and the cell of the volume
    averages of ``gnn_local_stress.homogenise``; ``boundary`` also sets ``boundary_vec`` (N, 2) and
    ``boundary_len`` (N,) (``boundary_vectors``), the quadrature of ``gnn_local_stress.boundary``."""
    edge_index, edge_attr = mesh_graph(points, faces, periodic)
    n = points.shape[0]
    dev = points.device
    if node_labels is None:
        node_labels = _labels_of(points, faces)
    labels = node_labels.to(dev).reshape(-1, 1).to(torch.int64)
    ms = torch.as_tensor(mean_stress, dtype=torch.float32, device=dev).reshape(1, 3)
    out = Data(edge_index=edge_index, edge_attr=edge_attr, pos=points[:, :2].float().contiguous(),
               face=faces.T.contiguous(), mean_stress=torch.ones(n, 3, device=dev) * ms,
               surfaces_nodes_for_div=labels, nodes_types=labels.clone(), is_periodic=periodic)
    if divergence:
        out.op_div_matrix = p1_divergence(points, faces)
    if areas:
        out.node_area, out.cell_area = nodal_areas(points, faces)
    if boundary:
        out.boundary_vec, out.boundary_len = boundary_vectors(points, faces)
    return out
