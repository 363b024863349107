"""A nodal field at arbitrary points on the HIP kernels (csrc/pdg_sample.hip): locate, interpolate, transpose.

    loc = PointLocator(points, faces)                   # uniform bins over the mesh, built once per mesh
    plan = loc.locate(xy)                               # plan.cell (Q,), plan.weights (Q, nv), plan.inside (Q,)
    v = sample_field(sigma, plan)                       # (Q, C): S sigma, NaN where no cell holds the point
    g = sample_field_grad(gv, plan)                     # (N, C): S^T gv, the cotangent for input_gradients
    s, xy, v = line_profile(loc, sigma, p0, p1, n=200)  # a profile along a segment
    img = raster(loc, sigma, nx, ny)                    # (ny, nx, C) over the bounding box, NaN in holes
    v = transfer_field(points_a, faces_a, sigma_a, points_b)   # a field of mesh a at the nodes of mesh b

Everything the project computes lives on mesh nodes; S is what lets a result leave its own mesh: a profile along the
ligament, an image for a figure, the same plate at two resolutions compared on one of them, a virtual strain gauge
(``gnn_local_stress.sensitivity.sample_gradients`` gives its sensitivity to the load).  The interpolation is the
mesh's own: P1 on triangles (barycentric weights), Q1 on quads (the bilinear shape functions at the inverse-mapped
point), so a field that is linear in (x, y) is reproduced and the nodes' values are.

A cell contains a point iff every weight is >= -2^-40; a point on an edge shared by two cells belongs to the one
where its smallest weight is larger, the lower cell id among equals.  ``periodic=True`` first wraps a query into the
bounding box, x - floor((x - xmin) / Lx) Lx in fp64, which is how a periodic cell continues; otherwise a point
outside the box, like one in a hole, has cell -1, zero weights, ``fill`` as its sample and no part in the transpose.

Sums are fp64 on the fp32 inputs, rounded once, in a fixed order and without float atomics: two calls agree
bitwise.  Gradients with respect to the query or the node positions are not formed, and there is no autograd route
(a field that requires grad is refused, as the forward refuses inputs that do): the transpose is explicit.  CPU
tensors raise, as everywhere on the HIP path (the CPU restatement is test-only, tests/sample_ref.py).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field as _dc_field

import torch

from pdg.devgraph import _nv
from pdg.lib import lib, stream_handle

GRID_MAX = 1024


def _device_only(what: str, *tensors) -> None:
    for t in tensors:
        if t.device.type != "cuda":
            raise RuntimeError(f"{what} runs on the MI355X HIP path only; move the tensors to a HIP device (the CPU "
                               "restatement is test-only, tests/sample_ref.py)")


def grid_size(n_faces: int) -> int:
    """Bins per axis for a mesh of ``n_faces`` cells: about two cells a bin, 1 to 1024 a side."""
    return min(max(math.ceil(math.sqrt(n_faces / 2)), 1), GRID_MAX)


@dataclass
class SamplePlan:
    """Where a set of query points lies in a mesh: ``cell`` (Q,) int32, -1 where no cell contains the point;
    ``weights`` (Q, nv) fp32, zero rows for -1; ``inside`` (Q,) bool = ``cell >= 0``; ``n_outside`` (1,) int32, the
    number of -1; ``faces`` (F, nv) int64, the mesh's, and ``n_nodes`` its node count.  All on the device.
    ``csr()`` is the node-major CSR of S, built on first use and kept."""
    cell: torch.Tensor
    weights: torch.Tensor
    inside: torch.Tensor
    n_outside: torch.Tensor
    faces: torch.Tensor
    n_nodes: int
    xy: torch.Tensor
    _csr: tuple | None = _dc_field(default=None, repr=False)

    @property
    def n_queries(self) -> int:
        return int(self.cell.shape[0])

    @property
    def nv(self) -> int:
        return int(self.weights.shape[1])

    def csr(self) -> tuple[torch.Tensor, torch.Tensor]:
        """(rowptr (n_nodes + 1,), entries (rowptr[-1],)) int32: row n holds, ascending, the q nv + k with
        ``faces[cell[q], k] == n`` (``pdg_sample_csr``).  One host read, of the status word, when it is built."""
        if self._csr is None:
            dev, nq, nv, nf = self.cell.device, self.n_queries, self.nv, int(self.faces.shape[0])
            nbytes = lib.pdg_sample_csr_scratch_bytes(self.n_nodes, nq, nv)
            if nbytes < 0:
                raise ValueError("too many query points: nv * Q must stay below 2^31")
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            rowptr = torch.empty(self.n_nodes + 1, dtype=torch.int32, device=dev)
            entries = torch.empty(max(nq * nv, 1), dtype=torch.int32, device=dev)
            status = torch.empty(1, dtype=torch.int32, device=dev)
            lib.pdg_sample_csr(self.n_nodes, nf, nv, self.faces.data_ptr() if nf else None, nq,
                               self.cell.data_ptr() if nq else None, rowptr.data_ptr(),
                               entries.data_ptr() if nq else None, status.data_ptr(), scratch.data_ptr(), nbytes,
                               stream_handle(dev))
            if int(status.item()):
                raise ValueError("the plan holds a cell or a node index outside its mesh")
            self._csr = (rowptr, entries)
        return self._csr


class PointLocator:
    """Uniform bins over a mesh for point location (``pdg_cell_bins``): ``points`` (N, 2|3) fp32 and ``faces``
    (F, 3|4) int64 on a HIP device; ``cells`` as in ``pdg.devgraph`` (``"any"`` decides by the faces' width);
    ``periodic`` wraps the queries into the bounding box.  One host read here (the four info words), with one
    repeat of the call when the first guess of the bins' capacity was too small (``capacity`` sets that guess).
    Keeps ``points``, ``faces``, ``bin_ptr``, ``bin_cells``, ``bbox`` (min x, min y, max x, max y) on the device;
    ``degenerate`` counts the cells of zero area, which can contain no point.  Raises ValueError for a face index
    outside the mesh."""

    def __init__(self, points: torch.Tensor, faces: torch.Tensor, cells: str = "any", periodic: bool = False,
                 capacity: int | None = None):
        _device_only("PointLocator", points, faces)
        pts = points.detach().contiguous().float()
        fcs = faces.contiguous().to(torch.int64)
        if pts.dim() != 2 or pts.shape[1] not in (2, 3) or fcs.dim() != 2:
            raise ValueError("points must be (N, 2|3) and faces (F, 3|4)")
        self.nv = _nv(fcs, cells)
        self.points, self.faces, self.periodic = pts, fcs, bool(periodic)
        n, nf, dev = pts.shape[0], fcs.shape[0], pts.device
        self.gx = self.gy = grid_size(nf)
        nbytes = lib.pdg_cell_bins_scratch_bytes(self.gx, self.gy)
        if n < 1 or nbytes < 0:
            raise ValueError("empty mesh")
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.bin_ptr = torch.empty(self.gx * self.gy + 1, dtype=torch.int32, device=dev)
        self.bbox = torch.empty(4, dtype=torch.float32, device=dev)
        info = torch.empty(4, dtype=torch.int32, device=dev)
        cap = max(int(capacity) if capacity is not None else 6 * nf + 16, 1)
        self.retried = False
        while True:
            self.bin_cells = torch.empty(cap, dtype=torch.int32, device=dev)
            lib.pdg_cell_bins(n, pts.data_ptr(), pts.shape[1], nf, self.nv, fcs.data_ptr() if nf else None, self.gx,
                              self.gy, self.bin_ptr.data_ptr(), self.bin_cells.data_ptr(), cap, self.bbox.data_ptr(),
                              info.data_ptr(), scratch.data_ptr(), nbytes, stream_handle(dev))
            total, overflow, self.degenerate, bad = info.tolist()
            if bad:
                raise ValueError(f"faces hold a node index outside [0, {n})")
            if not overflow:
                break
            if self.retried or total >= 2 ** 31 - 1:
                raise ValueError("the mesh's cells overlap too many bins (2^31 entries or more)")
            cap, self.retried = total, True
        self.capacity, self.entries = cap, total

    def locate(self, xy: torch.Tensor) -> SamplePlan:
        """The plan of the query points ``xy`` (Q, 2|3; x and y are read): two launches, no host read
        (``pdg_locate_points``)."""
        _device_only("PointLocator.locate", xy)
        if xy.dim() != 2 or xy.shape[1] not in (2, 3):
            raise ValueError(f"query points must be (Q, 2|3), got {tuple(xy.shape)}")
        q = xy.detach()[:, :2].float().contiguous()
        nq, nf, dev = q.shape[0], self.faces.shape[0], self.points.device
        if nq * self.nv >= 2 ** 31:
            raise ValueError("too many query points: nv * Q must stay below 2^31")
        cell = torch.empty(nq, dtype=torch.int32, device=dev)
        weights = torch.empty(nq, self.nv, dtype=torch.float32, device=dev)
        nout = torch.empty(1, dtype=torch.int32, device=dev)
        lib.pdg_locate_points(self.points.shape[0], self.points.data_ptr(), self.points.shape[1], nf, self.nv,
                              self.faces.data_ptr() if nf else None, self.gx, self.gy, self.bin_ptr.data_ptr(),
                              self.bin_cells.data_ptr(), self.capacity, self.bbox.data_ptr(), int(self.periodic), nq,
                              q.data_ptr() if nq else None, cell.data_ptr() if nq else None,
                              weights.data_ptr() if nq else None, nout.data_ptr(), stream_handle(dev))
        return SamplePlan(cell=cell, weights=weights, inside=cell >= 0, n_outside=nout, faces=self.faces,
                          n_nodes=int(self.points.shape[0]), xy=q)


def _rows(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dim() not in (1, 2) or (t.dim() == 2 and t.shape[1] < 1):
        raise ValueError(f"{what} is (R,) or (R, C) with C >= 1, got {tuple(t.shape)}")
    return t.detach().float().reshape(t.shape[0], t.shape[1] if t.dim() == 2 else 1).contiguous()


def sample_field(field: torch.Tensor, plan: SamplePlan, fill: float = float("nan"),
                 node_offset: int = 0) -> torch.Tensor:
    """``field`` (N,) or (N, C) at the plan's points, (Q,) or (Q, C) fp32, in one launch (``pdg_sample_field``):
    ``sum_k weights[q, k] field[node_offset + faces[cell[q], k]]``; ``fill`` where ``cell`` is -1.  ``node_offset``
    addresses the plan's mesh inside a batched field (``batch.ptr[g]``)."""
    _device_only("sample_field", field, plan.cell)
    if field.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("sample_field has no autograd route: detach the field, and use sample_field_grad (S^T) "
                           "with gnn_local_stress.sensitivity.sample_gradients for gradients")
    rows = _rows(field, "a nodal field")
    n, c = rows.shape
    if node_offset < 0 or node_offset + plan.n_nodes > n:
        raise ValueError(f"the field has {n} rows: no room for the plan's {plan.n_nodes} nodes at offset {node_offset}")
    nq, nf = plan.n_queries, int(plan.faces.shape[0])
    out = torch.empty(nq, c, dtype=torch.float32, device=rows.device)
    lib.pdg_sample_field(nq, nf, plan.nv, plan.faces.data_ptr() if nf else None,
                         plan.cell.data_ptr() if nq else None, plan.weights.data_ptr() if nq else None,
                         rows.data_ptr(), n, c, int(node_offset), float(fill), out.data_ptr() if nq else None,
                         stream_handle(rows.device))
    return out if field.dim() == 2 else out.reshape(nq)


def sample_field_grad(grad_samples: torch.Tensor, plan: SamplePlan, n_nodes: int | None = None,
                      node_offset: int = 0) -> torch.Tensor:
    """S^T: the cotangent on the nodal field of the cotangent ``grad_samples`` (Q,) or (Q, C) on the samples, in one
    launch after the plan's CSR (``pdg_sample_field_bwd``): (n_nodes,) or (n_nodes, C) fp32 with the plan's mesh at
    rows ``node_offset ...`` and exact zeros elsewhere (``n_nodes`` defaults to ``node_offset`` + the mesh's node
    count).  Points outside the mesh add nothing, whatever their ``grad_samples`` holds."""
    _device_only("sample_field_grad", grad_samples, plan.cell)
    g = _rows(grad_samples, "the samples' cotangent")
    nq, c = g.shape
    if nq != plan.n_queries:
        raise ValueError(f"the plan holds {plan.n_queries} points, the cotangent {nq} rows")
    total = node_offset + plan.n_nodes if n_nodes is None else int(n_nodes)
    if node_offset < 0 or node_offset + plan.n_nodes > total:
        raise ValueError(f"{total} rows: no room for the plan's {plan.n_nodes} nodes at offset {node_offset}")
    rowptr, entries = plan.csr()
    whole = total == plan.n_nodes
    out = (torch.empty if whole else torch.zeros)(total, c, dtype=torch.float32, device=g.device)
    lib.pdg_sample_field_bwd(plan.n_nodes, nq, plan.nv, rowptr.data_ptr(), entries.data_ptr() if nq else None,
                             plan.weights.data_ptr() if nq else None, g.data_ptr() if nq else None, c,
                             out[node_offset:].data_ptr(), stream_handle(g.device))
    return out if grad_samples.dim() == 2 else out.reshape(total)


def line_profile(locator: PointLocator, field: torch.Tensor, p0, p1, n: int = 200, fill: float = float("nan"),
                 node_offset: int = 0):
    """``field`` along the segment p0 -> p1 at ``n`` equally spaced points: ``(s, xy, values)`` with ``s`` (n,) the
    distance from p0, ``xy`` (n, 2) the points (the first bitwise p0, the last bitwise p1) and ``values`` (n,) or
    (n, C)."""
    if n < 2:
        raise ValueError("a profile needs n >= 2 points")
    dev = locator.points.device
    a = torch.as_tensor(p0, dtype=torch.float32).reshape(2).to(dev)
    b = torch.as_tensor(p1, dtype=torch.float32).reshape(2).to(dev)
    t = torch.linspace(0.0, 1.0, n, dtype=torch.float64, device=dev)
    xy = (a.double()[None, :] * (1.0 - t)[:, None] + b.double()[None, :] * t[:, None]).float()
    s = (t * (b.double() - a.double()).norm()).float()
    return s, xy, sample_field(field, locator.locate(xy), fill, node_offset)


def raster_points(locator: PointLocator, nx: int, ny: int) -> torch.Tensor:
    """The (ny nx, 2) fp32 pixel centres of an nx x ny image over the locator's bounding box, row-major from
    (xmin, ymin): x_i = xmin + (i + 1/2) Lx / nx formed in fp64."""
    if nx < 1 or ny < 1:
        raise ValueError("an image needs nx, ny >= 1")
    bb = locator.bbox.double()
    dev = bb.device
    xs = bb[0] + (torch.arange(nx, dtype=torch.float64, device=dev) + 0.5) * ((bb[2] - bb[0]) / nx)
    ys = bb[1] + (torch.arange(ny, dtype=torch.float64, device=dev) + 0.5) * ((bb[3] - bb[1]) / ny)
    return torch.stack([xs[None, :].expand(ny, nx), ys[:, None].expand(ny, nx)], -1).reshape(-1, 2).float()


def raster(locator: PointLocator, field: torch.Tensor, nx: int, ny: int, fill: float = float("nan"),
           node_offset: int = 0) -> torch.Tensor:
    """``field`` as an image: (ny, nx, C) fp32 ((ny, nx) for an (N,) field) at the pixel centres of
    ``raster_points``, row 0 at ymin, ``fill`` in holes."""
    v = sample_field(field, locator.locate(raster_points(locator, nx, ny)), fill, node_offset)
    return v.reshape(ny, nx, -1) if field.dim() == 2 else v.reshape(ny, nx)


def transfer_field(src_points: torch.Tensor, src_faces: torch.Tensor, field: torch.Tensor,
                   dst_points: torch.Tensor, cells: str = "any", periodic: bool = False,
                   fill: float = float("nan"), return_plan: bool = False):
    """``field`` of the mesh (``src_points``, ``src_faces``) at ``dst_points`` (Q, 2|3), typically the nodes of
    another mesh of the same plate: a locator, a plan and a sample in one call.  ``fill`` where the source mesh has
    no material (the other mesh's hole is smaller, its boundary lies outside).  ``return_plan`` also returns the
    plan."""
    loc = PointLocator(src_points, src_faces, cells=cells, periodic=periodic)
    plan = loc.locate(dst_points)
    v = sample_field(field, plan, fill)
    return (v, plan) if return_plan else v
