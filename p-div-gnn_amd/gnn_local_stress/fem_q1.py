"""FEM targets on quad meshes (csrc/pdg_femq1.hip): ``gnn_local_stress.fem``'s periodic elastic cell problem on
bilinear (Q1) quads, with the same fields, helpers and dataset files.

    sol = solve_cell(points, quads, strain=(1e-3, 0.0, 0.0))     # or stress=(100.0, 0.0, 0.0): the imposed mean
    C = effective_stiffness(points, quads)                       # (3, 3) fp64
    A = localisation_tensor(points, quads)                       # (N, 3, 3)
    data = fem_targets(points, quads, strain)                    # a Data of the quad graph with FEM targets
    write_sample(folder, 0, points, quads, strain)               # .vtk (quad cells) + .npz + dataset.csv row

The material, the load cases, the conventions of stress and strain, ``table``, ``STATUS`` and the noise rule are
``fem``'s (its module docstring); ``faces`` is (F, 4), the vertices of every quad running around it in either
orientation.  A triangle mesh is refused here as a quad mesh is there.  The integrals are the 2 x 2 Gauss rule's;
``element_table`` is (F, 36): det J, dN/dx[4], dN/dy[4] at each Gauss point, point g the one nearest corner g.  A face
whose four det J are not all strictly of one sign (a zero, a non-convex quad, a bow-tie) raises ``ValueError``.

The nodal fields average, over the node's own corners, the incident faces' values at the Gauss point nearest that
corner, weighted by that point's ``|det J|`` (``nodal="area"``) or unweighted (``nodal="count"``).  fedoo's
Gauss-point-to-node map for quads is not pinned here, as for triangles.

CPU tensors raise, as everywhere on the HIP path (the CPU restatement is test-only, tests/femq1_ref.py).
"""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path
from typing import Sequence

import numpy as np
import torch

from pdg.graph import Data
from pdg.lib import lib, stream_handle

from . import fem as _fem
from .fem import (BREAKDOWN, COLUMNS, CONVERGED, CSV_COLUMNS, MAX_CASES, MAX_ITER, MAX_ITER_CAP, NODAL, POISSON,  # noqa: F401
                  STATUS, TRIVIAL, YOUNG, CellSolution, FemFields, _material, _plan_points, _result, _vec3, stiffness)

ELEM = 36      # doubles per face of the element table


def _device_mesh(points, faces, what: str):
    if not isinstance(points, torch.Tensor) or not isinstance(faces, torch.Tensor) \
            or points.device.type != "cuda" or faces.device.type != "cuda":
        raise RuntimeError(f"{what} runs on the MI355X HIP path only; move the mesh to a HIP device (the CPU "
                           "restatement is test-only, tests/femq1_ref.py)")
    if faces.dim() == 2 and faces.shape[1] == 3:
        raise ValueError("the Q1 solver takes quads only: a triangle mesh (faces (F, 3)) goes to gnn_local_stress.fem")
    if points.dim() != 2 or points.shape[1] not in (2, 3) or faces.dim() != 2 or faces.shape[1] != 4:
        raise ValueError(f"points must be (N, 2|3) and faces (F, 4), got {tuple(points.shape)} and "
                         f"{tuple(faces.shape)}")
    return points.contiguous().float(), faces.contiguous().to(torch.int64)


@dataclass
class FemPlan(_fem.FemPlan):
    """``fem.FemPlan`` for quads, the same fields with four corners a face: ``item`` and ``verts`` / ``rverts`` hold
    4 F entries, an item is ``4 face + corner``."""

    @staticmethod
    def empty(device) -> "FemPlan":
        """A graph without nodes: an empty segment of a batch."""
        z = torch.zeros(0, dtype=torch.int32, device=device)
        z1 = torch.zeros(1, dtype=torch.int32, device=device)
        z2 = torch.zeros(2, dtype=torch.int32, device=device)
        return FemPlan(z, z1, z, z, z, z2, z2.clone(), 0, 0, 1, ((0, 0),))

    @staticmethod
    def from_mesh(points: torch.Tensor, faces: torch.Tensor) -> "FemPlan":
        """The plan of one periodic quad mesh; the periodic map and the refusals are ``fem.FemPlan.from_mesh``'s
        (``ValueError("mesh is not periodic")``, a face index outside the mesh)."""
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
        if not all(isinstance(p, FemPlan) for p in plans):
            raise ValueError("fem_q1.FemPlan.collate takes quad plans only")
        dev = plans[0].rep.device
        rep, rowptr, item, verts, rverts, sizes = [], [], [], [], [], []
        n0 = f0 = 0
        for p in plans:
            rep.append(p.rep + n0)
            rowptr.append(p.item_rowptr[:-1] + 4 * f0)
            item.append(p.item + 4 * f0)
            verts.append(p.verts + n0)
            rverts.append(p.rverts + n0)
            sizes.extend(p.sizes)
            n0 += p.n_nodes
            f0 += p.n_faces
        if n0 >= 2 ** 29 or f0 >= 2 ** 29:
            raise ValueError("a batch beyond int32 indexing")
        rowptr.append(torch.tensor([4 * f0], dtype=torch.int32, device=dev))
        nodes = torch.tensor([0] + [s[0] for s in sizes], dtype=torch.int64).cumsum(0)
        fcs = torch.tensor([0] + [s[1] for s in sizes], dtype=torch.int64).cumsum(0)
        i32 = torch.int32
        return FemPlan(torch.cat(rep).to(i32), torch.cat(rowptr).to(i32), torch.cat(item).to(i32),
                       torch.cat(verts).to(i32), torch.cat(rverts).to(i32), nodes.to(i32).to(dev),
                       fcs.to(i32).to(dev), n0, f0, len(sizes), tuple(sizes))


def _quad_plan(plan, what: str) -> None:
    if not isinstance(plan, FemPlan):
        raise ValueError(f"{what} takes a fem_q1.FemPlan (four corners a face), got {type(plan).__name__}")


def element_table(plan: FemPlan, points: torch.Tensor) -> torch.Tensor:
    """(F, 36) fp64 on the device: det J, dN/dx[4], dN/dy[4] at each of the four Gauss points of every face
    (``pdg_femq1_elements``).  One host read (the status word); raises ValueError for a face whose four det J are not
    all strictly of one sign."""
    _quad_plan(plan, "element_table")
    pts = _plan_points(plan, points, "element_table")
    dev = pts.device
    elem = torch.empty(plan.n_faces, ELEM, dtype=torch.float64, device=dev)
    if plan.n_faces == 0:
        return elem
    status = torch.empty(1, dtype=torch.int32, device=dev)
    lib.pdg_femq1_elements(plan.n_nodes, pts.data_ptr(), pts.shape[1], plan.n_faces, plan.verts.data_ptr(),
                           elem.data_ptr(), status.data_ptr(), stream_handle(dev))
    st = int(status.item())
    if st & 2:
        raise ValueError(f"faces hold a node index outside [0, {plan.n_nodes})")
    if st & 1:
        raise ValueError("a face is degenerate or not convex (its det J at the four Gauss points are not all strictly "
                         "of one sign: zero area, a re-entrant corner or a bow-tie): nothing is solved")
    return elem


def _fields(plan: FemPlan, pts: torch.Tensor, elem: torch.Tensor, strains: torch.Tensor, ut: torch.Tensor,
            young: float, poisson: float, nodal: str):
    dev, n, cases = pts.device, plan.n_nodes, strains.shape[1]
    stress = torch.empty(cases, n, 3, dtype=torch.float32, device=dev)
    strain = torch.empty(cases, n, 3, dtype=torch.float32, device=dev)
    sums = torch.empty(plan.n_graphs, cases, 8, dtype=torch.float64, device=dev)
    lib.pdg_femq1_stress(plan.n_graphs, cases, plan.ptr.data_ptr(), plan.fptr.data_ptr(), n, pts.data_ptr(),
                         pts.shape[1], plan.n_faces, plan.verts.data_ptr(), plan.rep.data_ptr(),
                         plan.item_rowptr.data_ptr(), plan.item.data_ptr(), elem.data_ptr(), strains.data_ptr(),
                         ut.data_ptr(), young, poisson, NODAL.index(nodal), stress.data_ptr(), strain.data_ptr(),
                         sums.data_ptr(), stream_handle(dev))
    return stress, strain, sums


def solve_cells(plan: FemPlan, points: torch.Tensor, strains, young: float = YOUNG, poisson: float = POISSON,
                rtol: float = 1e-10, max_iter: int = 4000, nodal: str = "area",
                elements: torch.Tensor | None = None) -> FemFields:
    """``fem.solve_cells`` on a quad plan: the cell problem of every graph of ``plan`` under every load case,
    ``strains`` (B, L, 3) = (exx, eyy, gxy).  ``elements``: ``element_table(plan, points)`` built beforehand; the
    call then reads nothing back and can be captured into a HIP graph (while a stream is capturing the table must be
    passed, and the strains are not checked for finiteness: the kernel answers them with ``BREAKDOWN``)."""
    _quad_plan(plan, "solve_cells")
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
    if elem.shape != (plan.n_faces, ELEM) or elem.dtype != torch.float64 or elem.device != dev:
        raise ValueError(f"elements must be element_table's ({plan.n_faces}, {ELEM}) fp64 tensor on the points' "
                         "device")
    elem = elem.contiguous()
    ut = torch.empty(cases, n, 2, dtype=torch.float64, device=dev)
    table = torch.empty(b, cases, 4, dtype=torch.float64, device=dev)
    if n == 0 or plan.n_faces == 0:
        nan = float("nan")
        return _result(torch.empty(cases, n, 3, device=dev), torch.empty(cases, n, 3, device=dev),
                       torch.full((b, cases, 8), nan, dtype=torch.float64, device=dev), ut, table.fill_(nan))
    nbytes = lib.pdg_femq1_solve_scratch_bytes(n, cases)
    if nbytes < 0:
        raise ValueError(f"solve_cells: unsupported sizes (nodes {n}, load cases {cases})")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    lib.pdg_femq1_solve(b, cases, plan.ptr.data_ptr(), n, pts.data_ptr(), pts.shape[1], plan.n_faces,
                        plan.verts.data_ptr(), plan.rverts.data_ptr(), plan.rep.data_ptr(),
                        plan.item_rowptr.data_ptr(), plan.item.data_ptr(), elem.data_ptr(), st.data_ptr(), young,
                        poisson, rtol, max_iter, ut.data_ptr(), table.data_ptr(), scratch.data_ptr(), nbytes,
                        stream_handle(dev))
    stress, strain, sums = _fields(plan, pts, elem, st, ut, young, poisson, nodal)
    return _result(stress, strain, sums, ut, table)


def _unit_solve(points, faces, kw):
    plan = FemPlan.from_mesh(points, faces)
    pts = points.contiguous().float()
    elem = element_table(plan, pts)
    unit = torch.eye(3, dtype=torch.float64, device=pts.device).reshape(1, 3, 3)
    return plan, pts, elem, solve_cells(plan, pts, unit, elements=elem, **kw)


def solve_cell(points: torch.Tensor, faces: torch.Tensor, strain=None, stress=None, young: float = YOUNG,
               poisson: float = POISSON, rtol: float = 1e-10, max_iter: int = 4000,
               nodal: str = "area") -> CellSolution:
    """``fem.solve_cell`` on a quad mesh: an imposed mean strain (``strain`` = exx, eyy, gxy) or an imposed mean
    stress (``stress``, cell convention; the three unit strains in one launch, ``eps = C_eff^-1 stress`` and the
    displacement fields superposed, the fields then evaluated once)."""
    if (strain is None) == (stress is None):
        raise ValueError("give exactly one of strain= and stress=")
    kw = dict(young=young, poisson=poisson, rtol=rtol, max_iter=max_iter, nodal=nodal)
    _device_mesh(points, faces, "solve_cell")
    if strain is not None:
        plan = FemPlan.from_mesh(points, faces)
        eps = _vec3(strain, "strain", plan.rep.device)
        f = solve_cells(plan, points, eps.reshape(1, 1, 3), **kw)
        return CellSolution(f.stress[0], f.strain[0], f.mean_stress[0, 0], f.mean_stress_material[0, 0], eps, f.ut[0],
                            f.table[0], f.material_area[0], f.cell_area[0])
    target = _vec3(stress, "stress", points.device)
    plan, pts, elem, unit = _unit_solve(points, faces, kw)
    c_eff = unit.mean_stress[0].T                                  # column j: the cell mean under unit strain j
    eps = torch.linalg.solve(c_eff, target)
    ut = torch.einsum("j,jnc->nc", eps, unit.ut).reshape(1, -1, 2).contiguous()
    young, poisson = _material(young, poisson)
    s, e, sums = _fields(plan, pts, elem, eps.reshape(1, 1, 3).contiguous(), ut, young, poisson, nodal)
    f = _result(s, e, sums, ut, unit.table)
    return CellSolution(f.stress[0], f.strain[0], f.mean_stress[0, 0], f.mean_stress_material[0, 0], eps, ut[0],
                        unit.table[0], f.material_area[0], f.cell_area[0])


def effective_stiffness(points: torch.Tensor, faces: torch.Tensor, **kw) -> torch.Tensor:
    """(3, 3) fp64 on the device: ``<sigma>_cell = C_eff eps``, column j the cell mean stress under the unit strain j
    (engineering shear).  Keywords as ``solve_cells``."""
    return _unit_solve(points, faces, kw)[3].mean_stress[0].T.contiguous()


def localisation_tensor(points: torch.Tensor, faces: torch.Tensor, **kw) -> torch.Tensor:
    """(N, 3, 3) fp32: ``A[n, i, j]`` = the FEM ``local_stress[n, i]`` per unit imposed mean stress ``Sigma_j`` (cell
    convention), as ``fem.localisation_tensor``."""
    unit = _unit_solve(points, faces, kw)[3]
    inv = torch.linalg.inv(unit.mean_stress[0].T)                  # eps per unit mean stress: column j
    return torch.einsum("kni,kj->nij", unit.stress.double(), inv).float().contiguous()


def fem_targets(points: torch.Tensor, faces: torch.Tensor, strain, periodic: bool = True, **kw) -> Data:
    """The graph ``convert_mesh_to_graph(..., divergence=True, cells="quad")`` builds, with ``local_stress`` (N, 3)
    and ``mean_stress`` (cell convention, broadcast to every node) from the Q1 solve under the mean ``strain``; the
    solution is kept as ``data.fem``.  Node labels are computed without the two-boundary assertion, so a plate
    without a hole passes.  Keywords as ``solve_cell``."""
    from pdg import devgraph
    sol = solve_cell(points, faces, strain=strain, **kw)
    pts, fcs = _device_mesh(points, faces, "fem_targets")
    labels = devgraph.node_labels(pts, fcs, strict=False, cells="quad")
    data = devgraph.convert_mesh_to_graph(pts, fcs, sol.mean_stress.float(), labels, periodic, True, cells="quad")
    data.local_stress = sol.stress
    data.fem = sol
    return data


def write_sample(folder, index: int, points: torch.Tensor, faces: torch.Tensor, strain, meta: dict | None = None,
                 **kw) -> dict:
    """``fem.write_sample`` for a quad mesh: the same three files with the same keys and columns, the mesh written
    as an unstructured grid of VTK quad cells (cell type 9), the divergence operator (Q1), the nodal areas behind ``op_mean_stress`` and the labels from
    the device builders' quad variants.  ``datasets.load_sample`` reads it back.  Returns the row."""
    import pandas as pd
    from pdg import devgraph
    from .vtk_io import write_legacy_vtk
    sol = solve_cell(points, faces, strain=strain, **kw)
    pts, fcs = _device_mesh(points, faces, "write_sample")
    op = devgraph.p1_divergence(pts, fcs, cells="quad")
    areas = devgraph.nodal_areas(pts, fcs, cells="quad")
    labels = devgraph.node_labels(pts, fcs, strict=False, cells="quad")
    folder = Path(folder)
    (folder / "meshes").mkdir(parents=True, exist_ok=True)
    (folder / "fields").mkdir(parents=True, exist_ok=True)
    name = f"hole_plate_mesh_{int(index)}"
    mesh_filename = (folder / "meshes" / f"{name}.vtk").as_posix()
    data_filename = (folder / "fields" / f"{name}.npz").as_posix()
    p = pts.cpu().numpy()
    write_legacy_vtk(mesh_filename, p, fcs.cpu().numpy(), dataset="UNSTRUCTURED_GRID", point_type="float")
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
