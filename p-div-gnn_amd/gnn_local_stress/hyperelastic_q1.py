"""Hyperelastic FEM targets on quad meshes (csrc/pdg_hyperq1.hip): ``gnn_local_stress.hyperelastic``'s periodic
neo-Hookean cell problem on bilinear (Q1) quads, with the same fields, helpers and dataset files; the counterpart of
the reference's ``scripts/generate_dataset_hyperelast.py`` run on its ``hole_plate_mesh_quad``.

    sol = solve_cell(points, quads, strain=(0.15, -0.10, 0.08))   # the logarithmic strain, or F=[[..], [..]]
    sol.stress, sol.mean_stress, sol.deformed, sol.table          # (N, 3) fp32 Cauchy, (3,) fp64, (N, 2), (1, 6)
    data = hyper_targets(points, quads, strain)                   # a Data; op_div_matrix (Q1) on the deformed mesh
    write_sample(folder, 0, points, quads, strain)                # .vtk (quad cells) + .npz + dataset.csv row

The law, the load, the conventions of stress and strain, the solver, ``table``, ``COLUMNS`` and ``STATUS`` are
``hyperelastic``'s (its module docstring); ``faces`` is (F, 4), the vertices of every quad running around it in either
orientation, and the plan and the element table are ``fem_q1``'s: ``fem_q1.FemPlan`` and ``fem_q1.element_table``,
(F, 36).  A triangle mesh or a triangle plan is refused here as a quad mesh is there.

What differs from triangles: the law is evaluated at the four points of the 2 x 2 Gauss rule, ``F_g = Fbar + sum_k
ut_k (x) grad N_k(g)`` with the weight ``|det J_g|``; a face counts as inverted when any of its four ``J_g`` is
``<= 0`` or not finite; the nodal fields average, over the node's own corners, the incident faces' values at the Gauss
point nearest that corner, weighted by that point's deformed weight ``|det J_g| J_g`` (``nodal="area"``) or unweighted
(``nodal="count"``); the solve's scratch holds 56 doubles a face and load case.  fedoo's Gauss-point-to-node map for
quads is not pinned here.

CPU tensors raise, as everywhere on the HIP path (the CPU restatement is test-only, tests/hyperq1_ref.py).
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from pdg.graph import Data
from pdg.lib import lib, stream_handle

from . import fem as _fem
from . import fem_q1 as _q1
from . import hyperelastic as _hy
from .fem_q1 import FemPlan, element_table  # noqa: F401
from .hyperelastic import (ARMIJO, BREAKDOWN, COLUMNS, CONVERGED, HALVINGS, KAPPA, MAX_CASES, MAX_ITER,  # noqa: F401
                           MAX_NEWTON_CAP, MAX_PCG_CAP, MAX_STEPS, MU, NODAL, PHI_NOISE, STATUS, TRIVIAL, VOLUMETRIC,
                           HyperFields, HyperSolution, deformation_gradient)

ELEM = _q1.ELEM      # doubles per face of the element table


def _device_mesh(points, faces, what: str):
    if not isinstance(points, torch.Tensor) or not isinstance(faces, torch.Tensor) \
            or points.device.type != "cuda" or faces.device.type != "cuda":
        raise RuntimeError(f"{what} runs on the MI355X HIP path only; move the mesh to a HIP device (the CPU "
                           "restatement is test-only, tests/hyperq1_ref.py)")
    if faces.dim() == 2 and faces.shape[1] == 3:
        raise ValueError("the Q1 hyperelastic solver takes quads only: a triangle mesh (faces (F, 3)) goes to "
                         "gnn_local_stress.hyperelastic")
    if points.dim() != 2 or points.shape[1] not in (2, 3) or faces.dim() != 2 or faces.shape[1] != 4:
        raise ValueError(f"points must be (N, 2|3) and faces (F, 4), got {tuple(points.shape)} and "
                         f"{tuple(faces.shape)}")
    return points.contiguous().float(), faces.contiguous().to(torch.int64)


def _quad_plan(plan, what: str) -> None:
    if not isinstance(plan, FemPlan):
        raise ValueError(f"{what} takes a fem_q1.FemPlan (four corners a face), got {type(plan).__name__}: a triangle "
                         "plan goes to gnn_local_stress.hyperelastic")


def solve_cells(plan: FemPlan, points: torch.Tensor, F, mu: float = MU, kappa: float = KAPPA,
                volumetric: str = "log", rtol: float = 1e-10, n_steps: int = 10, max_newton: int = 25,
                eta: float = 1e-4, max_pcg: int = 4000, nodal: str = "area",
                elements: torch.Tensor | None = None) -> HyperFields:
    """``hyperelastic.solve_cells`` on a quad plan: the cell problem of every graph of ``plan`` under every load case,
    ``F`` (B, L, 2, 2) (or (B, L, 4), row-major) the mean deformation gradients.  Keywords, clamps and results are
    ``hyperelastic.solve_cells``'s.  ``elements``: ``fem_q1.element_table(plan, points)`` built beforehand; the call
    then reads nothing back and can be captured into a HIP graph (while a stream is capturing the table must be
    passed, and ``F`` is not checked: the kernel answers a value that is not finite with ``BREAKDOWN`` and NaN
    rows)."""
    _quad_plan(plan, "hyperelastic_q1.solve_cells")
    pts = _fem._plan_points(plan, points, "hyperelastic_q1.solve_cells")
    mu, kappa, vol = _hy._law(mu, kappa, volumetric)
    rtol, eta = float(rtol), float(eta)
    if not (0.0 < rtol < 1.0):
        raise ValueError(f"rtol must lie in (0, 1), got {rtol}")
    if not (0.0 < eta < 1.0):
        raise ValueError(f"eta must lie in (0, 1), got {eta}")
    if nodal not in NODAL:
        raise ValueError(f"nodal is one of {NODAL}, got {nodal!r}")
    n_steps = int(n_steps)
    if not (1 <= n_steps <= MAX_STEPS):
        raise ValueError(f"n_steps must lie in [1, {MAX_STEPS}], got {n_steps}")
    max_newton = min(max(int(max_newton), 0), MAX_NEWTON_CAP)
    max_pcg = min(max(int(max_pcg), 1), MAX_PCG_CAP)
    dev = pts.device
    fb = torch.as_tensor(F, dtype=torch.float64, device=dev)
    if fb.dim() == 4 and fb.shape[2:] == (2, 2):
        fb = fb.reshape(fb.shape[0], fb.shape[1], 4)
    fb = fb.contiguous()
    if fb.dim() != 3 or fb.shape[0] != plan.n_graphs or fb.shape[2] != 4 or not (1 <= fb.shape[1] <= MAX_CASES):
        raise ValueError(f"F must be ({plan.n_graphs}, L, 2, 2) with 1 <= L <= {MAX_CASES}, got {tuple(fb.shape)}")
    capturing = torch.cuda.is_current_stream_capturing()
    if capturing and elements is None:
        raise RuntimeError("solve_cells under stream capture needs elements=fem_q1.element_table(plan, points), built "
                           "before the capture (its status is read on the host)")
    det = fb[..., 0] * fb[..., 3] - fb[..., 1] * fb[..., 2]
    if not capturing:
        if not bool(torch.isfinite(fb).all()):
            raise ValueError("F must be finite")
        if not bool((det > 0).all()):
            raise ValueError("det F must be > 0 for every load case")
    b, cases, n, nf = plan.n_graphs, fb.shape[1], plan.n_nodes, plan.n_faces
    elem = element_table(plan, pts) if elements is None else elements
    if elem.shape != (nf, ELEM) or elem.dtype != torch.float64 or elem.device != dev:
        raise ValueError(f"elements must be fem_q1.element_table's ({nf}, {ELEM}) fp64 tensor on the points' device")
    elem = elem.contiguous()
    ut = torch.empty(cases, n, 2, dtype=torch.float64, device=dev)
    table = torch.empty(b, cases, 6, dtype=torch.float64, device=dev)
    stress = torch.empty(cases, n, 3, dtype=torch.float32, device=dev)
    strain = torch.empty(cases, n, 3, dtype=torch.float32, device=dev)
    sums = torch.empty(b, cases, 10, dtype=torch.float64, device=dev)
    if n == 0 or nf == 0:
        table.fill_(float("nan"))
        sums.fill_(float("nan"))
    else:
        nbytes = lib.pdg_hyperq1_solve_scratch_bytes(n, nf, cases)
        if nbytes < 0:
            raise ValueError(f"solve_cells: unsupported sizes (nodes {n}, faces {nf}, load cases {cases})")
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        s = stream_handle(dev)
        lib.pdg_hyperq1_solve(b, cases, plan.ptr.data_ptr(), plan.fptr.data_ptr(), n, nf, plan.rverts.data_ptr(),
                              plan.rep.data_ptr(), plan.item_rowptr.data_ptr(), plan.item.data_ptr(), elem.data_ptr(),
                              fb.data_ptr(), mu, kappa, vol, rtol, n_steps, max_newton, eta, max_pcg, ut.data_ptr(),
                              table.data_ptr(), scratch.data_ptr(), nbytes, s)
        lib.pdg_hyperq1_stress(b, cases, plan.ptr.data_ptr(), plan.fptr.data_ptr(), n, pts.data_ptr(), pts.shape[1],
                               nf, plan.verts.data_ptr(), plan.rep.data_ptr(), plan.item_rowptr.data_ptr(),
                               plan.item.data_ptr(), elem.data_ptr(), fb.data_ptr(), ut.data_ptr(), mu, kappa, vol,
                               NODAL.index(nodal), stress.data_ptr(), strain.data_ptr(), sums.data_ptr(), s)
    # Fbar X + ut in fp64, rounded once; the graph of a node from the segments, on the device
    gid = torch.searchsorted(plan.ptr[1:].to(torch.int64), torch.arange(n, device=dev), right=True)
    gid = gid.clamp_(max=b - 1)
    deformed = (torch.einsum("nlij,nj->lni", fb.reshape(b, cases, 2, 2)[gid], pts[:, :2].double()) + ut).float()
    cell = sums[..., 9:10]
    return HyperFields(stress, strain, sums[..., 0:3] / (det.unsqueeze(-1) * cell), sums[..., 0:3] / sums[..., 7:8],
                       (sums[..., 3:7] / cell).reshape(b, cases, 2, 2), ut, deformed, table, sums[:, 0, 8],
                       sums[:, 0, 9])


def solve_cell(points: torch.Tensor, faces: torch.Tensor, strain=None, F=None, **kw) -> HyperSolution:
    """``hyperelastic.solve_cell`` on a quad mesh: ``strain`` = the logarithmic (exx, eyy, gxy), with
    ``Fbar = matrix_exp([[exx, gxy / 2], [gxy / 2, eyy]])`` in fp64, or ``F`` (2, 2) itself.  Keywords as
    ``solve_cells``."""
    if (strain is None) == (F is None):
        raise ValueError("give exactly one of strain= and F=")
    _device_mesh(points, faces, "hyperelastic_q1.solve_cell")
    if strain is not None:
        fbar = deformation_gradient(strain)
        eps = torch.as_tensor(strain, dtype=torch.float64).reshape(3).cpu()
    else:
        fbar = torch.as_tensor(F, dtype=torch.float64).reshape(2, 2).cpu()
        if not bool(torch.isfinite(fbar).all()):
            raise ValueError("F must be finite")
        if not float(torch.linalg.det(fbar)) > 0.0:
            raise ValueError("det F must be > 0")
        eps = _hy._log_strain_of(fbar)
    plan = FemPlan.from_mesh(points, faces)
    dev = plan.rep.device
    f = solve_cells(plan, points, fbar.reshape(1, 1, 4).to(dev), **kw)
    return HyperSolution(f.stress[0], f.log_strain[0], f.mean_stress[0, 0], f.mean_stress_material[0, 0],
                         f.mean_pk1[0, 0], fbar.to(dev), eps.to(dev), f.ut[0], f.deformed[0], f.table[0],
                         f.material_area[0], f.cell_area[0])


def hyper_targets(points: torch.Tensor, faces: torch.Tensor, strain, periodic: bool = True, **kw) -> Data:
    """``hyperelastic.hyper_targets`` for a quad mesh: the graph ``convert_mesh_to_graph(..., cells="quad")`` builds
    from the undeformed points, with ``local_stress`` (N, 3) and ``mean_stress`` (broadcast to every node) from the
    solve under the logarithmic mean ``strain``, and ``op_div_matrix`` the Q1 operator on the deformed mesh
    (``devgraph.p1_divergence(sol.deformed, faces, cells="quad")``).  The solution is kept as ``data.fem``
    (``HyperSolution``).  Keywords as ``solve_cell``."""
    from pdg import devgraph
    sol = solve_cell(points, faces, strain=strain, **kw)
    pts, fcs = _device_mesh(points, faces, "hyper_targets")
    labels = devgraph.node_labels(pts, fcs, strict=False, cells="quad")
    data = devgraph.convert_mesh_to_graph(pts, fcs, sol.mean_stress.float(), labels, periodic, False, cells="quad")
    data.op_div_matrix = devgraph.p1_divergence(sol.deformed, fcs, cells="quad")
    data.local_stress = sol.stress
    data.fem = sol
    return data


def write_sample(folder, index: int, points: torch.Tensor, faces: torch.Tensor, strain, meta: dict | None = None,
                 **kw) -> dict:
    """``hyperelastic.write_sample`` for a quad mesh: the same three files with the same keys and columns, the mesh
    written as an unstructured grid of VTK quad cells (cell type 9) as ``fem_q1.write_sample`` writes it, the
    divergence operator (Q1, on the deformed mesh), the nodal areas behind ``mean_stress_reference_mesh`` and the
    labels from the device builders' quad variants.  ``datasets.load_sample`` reads it back.  Returns the row.
    Keywords as ``solve_cell``."""
    import pandas as pd
    from pdg import devgraph
    from .vtk_io import write_legacy_vtk
    sol = solve_cell(points, faces, strain=strain, **kw)
    pts, fcs = _device_mesh(points, faces, "write_sample")
    op = devgraph.p1_divergence(sol.deformed, fcs, cells="quad")
    areas = devgraph.nodal_areas(pts, fcs, cells="quad")
    labels = devgraph.node_labels(pts, fcs, strict=False, cells="quad")
    ref_mean = (areas.area.double().unsqueeze(1) * sol.stress.double()).sum(0)
    ref_mean = ref_mean / (torch.linalg.det(sol.F) * areas.cell_area)
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
             mean_stress_reference_mesh=ref_mean.cpu().numpy(), op_div_matrix_data=op.values().cpu().numpy(),
             op_div_matrix_col_indices=idx[1].astype(np.int32), op_div_matrix_row_indices=idx[0].astype(np.int32),
             op_div_matrix_shape=np.array(op.shape), node_labels=labels.cpu().numpy())
    row = {c: float("nan") for c in _fem.CSV_COLUMNS}
    row.update(mesh_filename=mesh_filename, data_filename=data_filename, mean_stress_x=ms[0], mean_stress_y=ms[1],
               mean_stress_xy=ms[2], mean_strain_x=eps[0], mean_strain_y=eps[1], mean_strain_xy=eps[2],
               mean_stress_x_material=msm[0], mean_stress_y_material=msm[1], mean_stress_xy_material=msm[2],
               plate_width=float(p[:, 0].max() - p[:, 0].min()), plate_height=float(p[:, 1].max() - p[:, 1].min()),
               n_nodes=int(p.shape[0]), n_elements=int(fcs.shape[0]))
    for k, v in (meta or {}).items():
        if k not in _fem.CSV_COLUMNS or k in ("mesh_filename", "data_filename"):
            raise ValueError(f"meta: {k!r} is not a column write_sample leaves open")
        row[k] = v
    csv = folder / "dataset.csv"
    frame = pd.DataFrame([row], columns=list(_fem.CSV_COLUMNS))
    if csv.is_file():
        old = pd.read_csv(csv)
        frame = pd.concat([old[old["mesh_filename"] != mesh_filename], frame], ignore_index=True)
    frame.to_csv(csv.as_posix(), index=False)
    return row
