"""FEM targets on the HIP kernels (csrc/pdg_fem.hip): the periodic elastic cell problem on P1 triangles, the fields
every prediction here is measured against, and the reference's dataset files.

    sol = solve_cell(points, faces, strain=(1e-3, 0.0, 0.0))     # or stress=(100.0, 0.0, 0.0): the imposed mean
    sol.stress, sol.mean_stress, sol.table                       # (N, 3) fp32, (3,) fp64, (L, 4) fp64
    C = effective_stiffness(points, faces)                       # (3, 3) fp64
    A = localisation_tensor(points, faces)                       # (N, 3, 3): the FEM field per unit mean stress
    data = fem_targets(points, faces, strain)                    # a Data with local_stress / mean_stress from FEM
    write_sample(folder, 0, points, faces, strain)               # .vtk + .npz + dataset.csv row

Plane-stress linear elasticity, one isotropic material (``young = 1e5``, ``poisson = 0.3``: the reference's
``compute_mechanical_fields_dirichlet``), ``u(x) = eps x + ut(x)`` with ``ut`` periodic and
``eps = [[exx, gxy / 2], [gxy / 2, eyy]]``.  Stress and strain are (xx, yy, xy) with the engineering shear ``gxy``, as
in the reference's dataset.  Triangles only: a quad mesh is refused.

``FemPlan.from_mesh`` is the plumbing, once per mesh, torch on the device: the periodic representative of every node
and the corner lists the kernels gather through.  ``solve_cells`` then runs three calls: ``pdg_fem_elements`` (the
element table, one host read of its status unless the table is passed in), ``pdg_fem_solve`` (one persistent
workgroup per graph and load case: Jacobi-preconditioned conjugate gradients, fp64) and ``pdg_fem_stress`` (nodal
fields and the volume sums).  ``table[g, l]`` = (iterations, ``|b|_2``, the true final relative residual, status),
``STATUS`` names the last column.  A right-hand side that is rounding noise -- a plate without a hole, whose exact
``b`` is 0 -- is detected in the kernel (``|b|_2 <= 1e-12 |b_abs|_2``) and returns ``ut = 0`` with ``TRIVIAL`` and no
iteration.  Nothing is read back after the solve: a caller who needs convergence checked reads ``table[..., 3]``.

The nodal fields average the incident elements' values over the node's own corners, weighted by the element's area
(``nodal="area"``, the weighting of the project's divergence operator) or unweighted (``nodal="count"``).  Which of
the two fedoo's Gauss-point-to-node map is cannot be pinned here.

CPU tensors raise, as everywhere on the HIP path (the CPU restatement is test-only, tests/fem_ref.py).
"""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path
from typing import Sequence

import numpy as np
import torch

from pdg.graph import Data
from pdg.lib import lib, stream_handle

COLUMNS = ("iterations", "rhs_norm", "residual", "status")
CONVERGED, TRIVIAL, MAX_ITER, BREAKDOWN = 0, 1, 2, 3
STATUS = ("CONVERGED", "TRIVIAL", "MAX_ITER", "BREAKDOWN")
NODAL = ("area", "count")
MAX_ITER_CAP = 100000
MAX_CASES = 64
YOUNG, POISSON = 1e5, 0.3


def _device_mesh(points, faces, what: str):
    if not isinstance(points, torch.Tensor) or not isinstance(faces, torch.Tensor) \
            or points.device.type != "cuda" or faces.device.type != "cuda":
        raise RuntimeError(f"{what} runs on the MI355X HIP path only; move the mesh to a HIP device (the CPU "
                           "restatement is test-only, tests/fem_ref.py)")
    if faces.dim() == 2 and faces.shape[1] == 4:
        raise ValueError("the FEM solver takes P1 triangles only: a quad mesh (cells='quad', faces (F, 4)) is out of "
                         "scope")
    if points.dim() != 2 or points.shape[1] not in (2, 3) or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"points must be (N, 2|3) and faces (F, 3), got {tuple(points.shape)} and "
                         f"{tuple(faces.shape)}")
    return points.contiguous().float(), faces.contiguous().to(torch.int64)


def _cells(cells: str) -> None:
    if cells != "triangle":
        raise ValueError(f"the FEM solver takes P1 triangles only (cells='triangle'), got cells={cells!r}: quads are "
                         "out of scope")


@dataclass
class FemPlan:
    """What the kernels read of a mesh, or of a batch of meshes, besides its points; int32 on the device, indices
    batch-wide.  ``rep`` (N): the periodic representative of every node.  ``item_rowptr`` (N + 1), ``item`` (3 F): a
    CSR keyed by representative, row v holding ``3 face + corner`` of every corner that is v or an image of v,
    ascending; rows of image nodes are empty.  ``verts`` (3 F): the node of every corner; ``rverts`` = ``rep[verts]``.
    ``ptr`` / ``fptr`` (B + 1): the node and face segments of the graphs."""
    rep: torch.Tensor
    item_rowptr: torch.Tensor
    item: torch.Tensor
    verts: torch.Tensor
    rverts: torch.Tensor
    ptr: torch.Tensor
    fptr: torch.Tensor
    n_nodes: int
    n_faces: int
    n_graphs: int
    sizes: tuple = ()        # (nodes, faces) of every graph

    @staticmethod
    def empty(device) -> "FemPlan":
        """A graph without nodes: an empty segment of a batch."""
        z = torch.zeros(0, dtype=torch.int32, device=device)
        z1 = torch.zeros(1, dtype=torch.int32, device=device)
        z2 = torch.zeros(2, dtype=torch.int32, device=device)
        return FemPlan(z, z1, z, z, z, z2, z2.clone(), 0, 0, 1, ((0, 0),))

    @staticmethod
    def from_mesh(points: torch.Tensor, faces: torch.Tensor, cells: str = "triangle") -> "FemPlan":
        """The plan of one periodic triangle mesh.  Nodes with ``x == xmax`` map to the node with ``x == xmin`` at
        the same y, nodes with ``y == ymax`` to the node with ``y == ymin`` at the same x, and the two maps are
        composed, so the four corners share one representative; equality is exact, in float32, as in
        ``pdg.meshgen.periodic_pairs``.  Raises ``ValueError("mesh is not periodic")`` when the side counts or the
        coordinates do not match, and for a face index outside the mesh."""
        _cells(cells)
        pts, fcs = _device_mesh(points, faces, "FemPlan.from_mesh")
        n, nf, dev = pts.shape[0], fcs.shape[0], pts.device
        if n == 0 or nf == 0:
            raise ValueError("empty mesh")
        if bool(((fcs < 0) | (fcs >= n)).any()):
            raise ValueError(f"faces hold a node index outside [0, {n})")
        ident = torch.arange(n, device=dev)

        def side_map(along: torch.Tensor, across: torch.Tensor) -> torch.Tensor:
            lo, hi = along.min(), along.max()
            src = torch.nonzero(along == hi).reshape(-1)
            dst = torch.nonzero(along == lo).reshape(-1)
            if src.numel() != dst.numel() or bool(lo == hi):
                raise ValueError("mesh is not periodic")
            src = src[torch.argsort(across[src], stable=True)]
            dst = dst[torch.argsort(across[dst], stable=True)]
            if not torch.equal(across[src], across[dst]):
                raise ValueError("mesh is not periodic")
            m = ident.clone()
            m[src] = dst
            return m

        x, y = pts[:, 0], pts[:, 1]
        rep = side_map(y, x)[side_map(x, y)]
        flat = fcs.reshape(-1)
        key = rep[flat]
        item = torch.argsort(key, stable=True)
        rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        rowptr[1:] = torch.cumsum(torch.bincount(key, minlength=n), 0)
        i32 = torch.int32
        return FemPlan(rep.to(i32), rowptr.to(i32), item.to(i32), flat.to(i32), key.to(i32),
                       torch.tensor([0, n], dtype=i32, device=dev), torch.tensor([0, nf], dtype=i32, device=dev),
                       n, nf, 1, ((n, nf),))

    @staticmethod
    def collate(plans: Sequence["FemPlan"]) -> "FemPlan":
        """The plans one after another, with node and face offsets: the plan of the batch whose points are the
        meshes' points concatenated in the same order."""
        plans = list(plans)
        if not plans:
            raise ValueError("no plan to collate")
        dev = plans[0].rep.device
        rep, rowptr, item, verts, rverts, sizes = [], [], [], [], [], []
        n0 = f0 = 0
        for p in plans:
            rep.append(p.rep + n0)
            rowptr.append(p.item_rowptr[:-1] + 3 * f0)
            item.append(p.item + 3 * f0)
            verts.append(p.verts + n0)
            rverts.append(p.rverts + n0)
            sizes.extend(p.sizes)
            n0 += p.n_nodes
            f0 += p.n_faces
        if n0 >= 2 ** 29 or f0 >= 2 ** 29:
            raise ValueError("a batch beyond int32 indexing")
        rowptr.append(torch.tensor([3 * f0], dtype=torch.int32, device=dev))
        nodes = torch.tensor([0] + [s[0] for s in sizes], dtype=torch.int64).cumsum(0)
        fcs = torch.tensor([0] + [s[1] for s in sizes], dtype=torch.int64).cumsum(0)
        i32 = torch.int32
        return FemPlan(torch.cat(rep).to(i32), torch.cat(rowptr).to(i32), torch.cat(item).to(i32),
                       torch.cat(verts).to(i32), torch.cat(rverts).to(i32), nodes.to(i32).to(dev),
                       fcs.to(i32).to(dev), n0, f0, len(sizes), tuple(sizes))


def _material(young: float, poisson: float) -> tuple[float, float]:
    young, poisson = float(young), float(poisson)
    if not (0.0 < young < float("inf")):
        raise ValueError(f"young must be finite and > 0, got {young}")
    if not (-1.0 < poisson < 0.5):
        raise ValueError(f"poisson must lie in (-1, 0.5), got {poisson}")
    return young, poisson


def stiffness(young: float = YOUNG, poisson: float = POISSON) -> torch.Tensor:
    """(3, 3) fp64 on the host: the plane-stress C on (xx, yy, gamma_xy)."""
    young, poisson = _material(young, poisson)
    c = young / (1.0 - poisson * poisson)
    return torch.tensor([[c, poisson * c, 0.0], [poisson * c, c, 0.0], [0.0, 0.0, c * (1.0 - poisson) / 2.0]],
                        dtype=torch.float64)


def _plan_points(plan: FemPlan, points: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(points, torch.Tensor) or points.device.type != "cuda":
        raise RuntimeError(f"{what} runs on the MI355X HIP path only; move the points to a HIP device (the CPU "
                           "restatement is test-only, tests/fem_ref.py)")
    if points.dim() != 2 or points.shape[1] not in (2, 3) or points.shape[0] != plan.n_nodes:
        raise ValueError(f"points must be ({plan.n_nodes}, 2|3), got {tuple(points.shape)}")
    if plan.rep.device != points.device:
        raise RuntimeError("the plan and the points must live on the same HIP device")
    return points.contiguous().float()


def element_table(plan: FemPlan, points: torch.Tensor) -> torch.Tensor:
    """(F, 8) fp64 on the device: det, area, gx[3], gy[3] of every face (``pdg_fem_elements``).  One host read (the
    status word); raises ValueError for a face of zero area."""
    pts = _plan_points(plan, points, "element_table")
    dev = pts.device
    elem = torch.empty(plan.n_faces, 8, dtype=torch.float64, device=dev)
    if plan.n_faces == 0:
        return elem
    status = torch.empty(1, dtype=torch.int32, device=dev)
    lib.pdg_fem_elements(plan.n_nodes, pts.data_ptr(), pts.shape[1], plan.n_faces, plan.verts.data_ptr(),
                         elem.data_ptr(), status.data_ptr(), stream_handle(dev))
    st = int(status.item())
    if st & 2:
        raise ValueError(f"faces hold a node index outside [0, {plan.n_nodes})")
    if st & 1:
        raise ValueError("a face has zero area (det == 0): the P1 gradients are undefined there, nothing is solved")
    return elem


@dataclass
class FemFields:
    """``solve_cells``' result, everything on the device.  ``stress`` / ``strain`` (L, N, 3) fp32 nodal fields;
    ``mean_stress`` (B, L, 3) fp64 in the cell convention (the reference's: over the bounding box),
    ``mean_stress_material`` and ``mean_strain_material`` over the material; ``ut`` (L, N, 2) fp64, the periodic part
    of the displacement; ``table`` (B, L, 4) fp64 (``COLUMNS``); ``material_area`` / ``cell_area`` (B,) fp64."""
    stress: torch.Tensor
    strain: torch.Tensor
    mean_stress: torch.Tensor
    mean_stress_material: torch.Tensor
    mean_strain_material: torch.Tensor
    ut: torch.Tensor
    table: torch.Tensor
    material_area: torch.Tensor
    cell_area: torch.Tensor


def _fields(plan: FemPlan, pts: torch.Tensor, elem: torch.Tensor, strains: torch.Tensor, ut: torch.Tensor,
            young: float, poisson: float, nodal: str):
    dev, n, cases = pts.device, plan.n_nodes, strains.shape[1]
    stress = torch.empty(cases, n, 3, dtype=torch.float32, device=dev)
    strain = torch.empty(cases, n, 3, dtype=torch.float32, device=dev)
    sums = torch.empty(plan.n_graphs, cases, 8, dtype=torch.float64, device=dev)
    lib.pdg_fem_stress(plan.n_graphs, cases, plan.ptr.data_ptr(), plan.fptr.data_ptr(), n, pts.data_ptr(),
                       pts.shape[1], plan.n_faces, plan.verts.data_ptr(), plan.rep.data_ptr(),
                       plan.item_rowptr.data_ptr(), plan.item.data_ptr(), elem.data_ptr(), strains.data_ptr(),
                       ut.data_ptr(), young, poisson, NODAL.index(nodal), stress.data_ptr(), strain.data_ptr(),
                       sums.data_ptr(), stream_handle(dev))
    return stress, strain, sums


def _result(stress, strain, sums, ut, table) -> FemFields:
    material, cell = sums[..., 6:7], sums[..., 7:8]
    return FemFields(stress, strain, sums[..., 0:3] / cell, sums[..., 0:3] / material, sums[..., 3:6] / material, ut,
                     table, sums[:, 0, 6], sums[:, 0, 7])


def solve_cells(plan: FemPlan, points: torch.Tensor, strains, young: float = YOUNG, poisson: float = POISSON,
                rtol: float = 1e-10, max_iter: int = 4000, nodal: str = "area",
                elements: torch.Tensor | None = None) -> FemFields:
    """The cell problem of every graph of ``plan`` under every load case: ``strains`` (B, L, 3) = (exx, eyy, gxy).
    ``points`` (N, 2|3): the meshes' points in the plan's order.  ``max_iter`` is clamped to [0, 100000].
    ``elements``: ``element_table(plan, points)`` built beforehand; the call then reads nothing back and can be
    captured into a HIP graph (while a stream is capturing the table must be passed, and the strains are not checked
    for finiteness: the kernel answers them with ``BREAKDOWN``)."""
    pts = _plan_points(plan, points, "solve_cells")
    young, poisson = _material(young, poisson)
    rtol = float(rtol)
    if not (0.0 < rtol < 1.0):
        raise ValueError(f"rtol must lie in (0, 1), got {rtol}")
    if nodal not in NODAL:
        raise ValueError(f"nodal is one of {NODAL}, got {nodal!r}")
    max_iter = min(max(int(max_iter), 0), MAX_ITER_CAP)
    dev = pts.device
    st = torch.as_tensor(strains, dtype=torch.float64, device=dev).contiguous()
    if st.dim() != 3 or st.shape[0] != plan.n_graphs or st.shape[2] != 3 or not (1 <= st.shape[1] <= MAX_CASES):
        raise ValueError(f"strains must be ({plan.n_graphs}, L, 3) with 1 <= L <= {MAX_CASES}, got {tuple(st.shape)}")
    capturing = torch.cuda.is_current_stream_capturing()
    if capturing and elements is None:
        raise RuntimeError("solve_cells under stream capture needs elements=element_table(plan, points), built "
                           "before the capture (its status is read on the host)")
    if not capturing and not bool(torch.isfinite(st).all()):
        raise ValueError("strains must be finite")
    b, cases, n = plan.n_graphs, st.shape[1], plan.n_nodes
    elem = element_table(plan, pts) if elements is None else elements
    if elem.shape != (plan.n_faces, 8) or elem.dtype != torch.float64 or elem.device != dev:
        raise ValueError(f"elements must be element_table's ({plan.n_faces}, 8) fp64 tensor on the points' device")
    elem = elem.contiguous()
    ut = torch.empty(cases, n, 2, dtype=torch.float64, device=dev)
    table = torch.empty(b, cases, 4, dtype=torch.float64, device=dev)
    if n == 0 or plan.n_faces == 0:
        nan = float("nan")
        return _result(torch.empty(cases, n, 3, device=dev), torch.empty(cases, n, 3, device=dev),
                       torch.full((b, cases, 8), nan, dtype=torch.float64, device=dev), ut, table.fill_(nan))
    nbytes = lib.pdg_fem_solve_scratch_bytes(n, cases)
    if nbytes < 0:
        raise ValueError(f"solve_cells: unsupported sizes (nodes {n}, load cases {cases})")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    lib.pdg_fem_solve(b, cases, plan.ptr.data_ptr(), n, pts.data_ptr(), pts.shape[1], plan.n_faces,
                      plan.verts.data_ptr(), plan.rverts.data_ptr(), plan.rep.data_ptr(), plan.item_rowptr.data_ptr(),
                      plan.item.data_ptr(), elem.data_ptr(), st.data_ptr(), young, poisson, rtol, max_iter,
                      ut.data_ptr(), table.data_ptr(), scratch.data_ptr(), nbytes, stream_handle(dev))
    stress, strain, sums = _fields(plan, pts, elem, st, ut, young, poisson, nodal)
    return _result(stress, strain, sums, ut, table)


@dataclass
class CellSolution:
    """``solve_cell``'s result for one mesh, on the device.  ``stress`` / ``strain`` (N, 3) fp32; ``mean_stress``
    (3,) fp64 (cell convention), ``mean_stress_material`` (3,); ``mean_strain`` (3,) fp64, the imposed eps;
    ``ut`` (N, 2) fp64; ``table`` (L, 4) fp64, one row per solve behind the result (1 with ``strain``, the 3 unit
    strains with ``stress``); ``material_area`` / ``cell_area`` () fp64."""
    stress: torch.Tensor
    strain: torch.Tensor
    mean_stress: torch.Tensor
    mean_stress_material: torch.Tensor
    mean_strain: torch.Tensor
    ut: torch.Tensor
    table: torch.Tensor
    material_area: torch.Tensor
    cell_area: torch.Tensor


def _vec3(v, what: str, dev) -> torch.Tensor:
    t = torch.as_tensor(v, dtype=torch.float64).reshape(-1).to(dev)
    if t.numel() != 3:
        raise ValueError(f"{what} holds 3 values (xx, yy, xy), got {t.numel()}")
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"{what} must be finite")
    return t


def _unit_solve(points, faces, cells, kw):
    _cells(cells)
    plan = FemPlan.from_mesh(points, faces)
    pts = points.contiguous().float()
    elem = element_table(plan, pts)
    unit = torch.eye(3, dtype=torch.float64, device=pts.device).reshape(1, 3, 3)
    return plan, pts, elem, solve_cells(plan, pts, unit, elements=elem, **kw)


def solve_cell(points: torch.Tensor, faces: torch.Tensor, strain=None, stress=None, young: float = YOUNG,
               poisson: float = POISSON, rtol: float = 1e-10, max_iter: int = 4000, nodal: str = "area",
               cells: str = "triangle") -> CellSolution:
    """One mesh under an imposed mean strain (``strain`` = exx, eyy, gxy) or an imposed mean stress (``stress``, cell
    convention).  With ``stress`` the three unit strains are solved in one launch, ``C_eff`` is formed from their
    cell means, ``eps = C_eff^-1 stress`` (3 x 3, fp64) and the three displacement fields are superposed, which is
    exact by linearity; the fields are then evaluated once."""
    if (strain is None) == (stress is None):
        raise ValueError("give exactly one of strain= and stress=")
    kw = dict(young=young, poisson=poisson, rtol=rtol, max_iter=max_iter, nodal=nodal)
    _cells(cells)
    _device_mesh(points, faces, "solve_cell")
    if strain is not None:
        plan = FemPlan.from_mesh(points, faces)
        eps = _vec3(strain, "strain", plan.rep.device)
        f = solve_cells(plan, points, eps.reshape(1, 1, 3), **kw)
        return CellSolution(f.stress[0], f.strain[0], f.mean_stress[0, 0], f.mean_stress_material[0, 0], eps, f.ut[0],
                            f.table[0], f.material_area[0], f.cell_area[0])
    target = _vec3(stress, "stress", points.device)
    plan, pts, elem, unit = _unit_solve(points, faces, cells, kw)
    c_eff = unit.mean_stress[0].T                                  # column j: the cell mean under unit strain j
    eps = torch.linalg.solve(c_eff, target)
    ut = torch.einsum("j,jnc->nc", eps, unit.ut).reshape(1, -1, 2).contiguous()
    young, poisson = _material(young, poisson)
    s, e, sums = _fields(plan, pts, elem, eps.reshape(1, 1, 3).contiguous(), ut, young, poisson, nodal)
    f = _result(s, e, sums, ut, unit.table)
    return CellSolution(f.stress[0], f.strain[0], f.mean_stress[0, 0], f.mean_stress_material[0, 0], eps, ut[0],
                        unit.table[0], f.material_area[0], f.cell_area[0])


def effective_stiffness(points: torch.Tensor, faces: torch.Tensor, cells: str = "triangle", **kw) -> torch.Tensor:
    """(3, 3) fp64 on the device: ``<sigma>_cell = C_eff eps``, column j the cell mean stress under the unit strain j
    (engineering shear).  Keywords as ``solve_cells``."""
    return _unit_solve(points, faces, cells, kw)[3].mean_stress[0].T.contiguous()


def localisation_tensor(points: torch.Tensor, faces: torch.Tensor, cells: str = "triangle", **kw) -> torch.Tensor:
    """(N, 3, 3) fp32: ``A[n, i, j]`` = the FEM ``local_stress[n, i]`` per unit imposed mean stress ``Sigma_j`` (cell
    convention), the counterpart of ``sensitivity.localisation_tensor(model, batch)``: the two can be subtracted.
    The three unit-strain fields times ``C_eff^-1``, formed in fp64 and rounded once."""
    unit = _unit_solve(points, faces, cells, kw)[3]
    inv = torch.linalg.inv(unit.mean_stress[0].T)                  # eps per unit mean stress: column j
    return torch.einsum("kni,kj->nij", unit.stress.double(), inv).float().contiguous()


def fem_targets(points: torch.Tensor, faces: torch.Tensor, strain, periodic: bool = True, cells: str = "triangle",
                **kw) -> Data:
    """The graph ``convert_mesh_to_graph(..., divergence=True)`` builds, with ``local_stress`` (N, 3) and
    ``mean_stress`` (cell convention, broadcast to every node) from the FEM solve under the mean ``strain``; the
    solution is kept as ``data.fem`` (``CellSolution``).  Node labels are computed without the two-boundary
    assertion, so a plate without a hole passes.  Keywords as ``solve_cell``."""
    from pdg import devgraph
    sol = solve_cell(points, faces, strain=strain, cells=cells, **kw)
    pts, fcs = _device_mesh(points, faces, "fem_targets")
    labels = devgraph.node_labels(pts, fcs, strict=False)
    data = devgraph.convert_mesh_to_graph(pts, fcs, sol.mean_stress.float(), labels, periodic, True)
    data.local_stress = sol.stress
    data.fem = sol
    return data


CSV_COLUMNS = ("mesh_filename", "data_filename", "mean_stress_x", "mean_stress_y", "mean_stress_xy", "mean_strain_x",
               "mean_strain_y", "mean_strain_xy", "mean_stress_x_material", "mean_stress_y_material",
               "mean_stress_xy_material", "hole_plate_center_x", "hole_plate_center_y", "hole_plate_radius",
               "plate_width", "plate_height", "global_mesh_refinement_size", "hole_mesh_refinement_factor", "n_nodes",
               "n_elements", "seed")


def write_sample(folder, index: int, points: torch.Tensor, faces: torch.Tensor, strain, meta: dict | None = None,
                 **kw) -> dict:
    """One sample of the reference's on-disk dataset (``scripts/generate_dataset.py``), which
    ``datasets.load_sample`` / ``MeshStressFieldDatasetInMemory`` read back: ``meshes/hole_plate_mesh_{index}.vtk``
    (``write_legacy_vtk``, single-precision points, so the round trip is exact), ``fields/hole_plate_mesh_{index}.npz``
    with the reference's keys (``stress_field``, ``mean_stress``, ``mean_strain``, ``mean_stress_material``,
    ``op_div_matrix_*``, ``op_mean_stress``, ``node_labels``) and a row of ``dataset.csv`` with its column names
    (``CSV_COLUMNS``; a row with the same mesh file is replaced).  ``meta`` fills the columns the solve does not know
    (hole centre and radius, refinement sizes, seed); they are NaN otherwise.  The divergence operator, the nodal
    areas behind ``op_mean_stress`` and the labels come from the device builders (``pdg.devgraph``).  Returns the
    row.  Keywords as ``solve_cell``."""
    import pandas as pd
    from pdg import devgraph
    from .vtk_io import write_legacy_vtk
    sol = solve_cell(points, faces, strain=strain, **kw)
    pts, fcs = _device_mesh(points, faces, "write_sample")
    op = devgraph.p1_divergence(pts, fcs)
    areas = devgraph.nodal_areas(pts, fcs)
    labels = devgraph.node_labels(pts, fcs, strict=False)
    folder = Path(folder)
    (folder / "meshes").mkdir(parents=True, exist_ok=True)
    (folder / "fields").mkdir(parents=True, exist_ok=True)
    name = f"hole_plate_mesh_{int(index)}"
    mesh_filename = (folder / "meshes" / f"{name}.vtk").as_posix()
    data_filename = (folder / "fields" / f"{name}.npz").as_posix()
    p = pts.cpu().numpy()
    write_legacy_vtk(mesh_filename, p, fcs.cpu().numpy(), point_type="float")
    idx = op.indices().cpu().numpy()
    ms, msm, eps = (t.cpu().numpy() for t in (sol.mean_stress, sol.mean_stress_material, sol.mean_strain))
    np.savez(data_filename, stress_field=sol.stress.cpu().numpy(), mean_stress=ms, mean_strain=eps,
             mean_stress_material=msm, op_div_matrix_data=op.values().cpu().numpy(),
             op_div_matrix_col_indices=idx[1].astype(np.int32), op_div_matrix_row_indices=idx[0].astype(np.int32),
             op_div_matrix_shape=np.array(op.shape), op_mean_stress=(areas.area.double() / areas.cell_area).cpu().numpy(),
             node_labels=labels.cpu().numpy())
    row = {c: float("nan") for c in CSV_COLUMNS}
    row.update(mesh_filename=mesh_filename, data_filename=data_filename, mean_stress_x=ms[0], mean_stress_y=ms[1],
               mean_stress_xy=ms[2], mean_strain_x=eps[0], mean_strain_y=eps[1], mean_strain_xy=eps[2],
               mean_stress_x_material=msm[0], mean_stress_y_material=msm[1], mean_stress_xy_material=msm[2],
               plate_width=float(p[:, 0].max() - p[:, 0].min()), plate_height=float(p[:, 1].max() - p[:, 1].min()),
               n_nodes=int(p.shape[0]), n_elements=int(fcs.shape[0]))
    for k, v in (meta or {}).items():
        if k not in CSV_COLUMNS or k in ("mesh_filename", "data_filename"):
            raise ValueError(f"meta: {k!r} is not a column write_sample leaves open")
        row[k] = v
    csv = folder / "dataset.csv"
    frame = pd.DataFrame([row], columns=list(CSV_COLUMNS))
    if csv.is_file():
        old = pd.read_csv(csv)
        frame = pd.concat([old[old["mesh_filename"] != mesh_filename], frame], ignore_index=True)
    frame.to_csv(csv.as_posix(), index=False)
    return row
