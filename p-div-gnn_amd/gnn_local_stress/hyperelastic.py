"""Hyperelastic FEM targets on the HIP kernels (csrc/pdg_hyper.hip): the periodic cell problem of a compressible
neo-Hookean material in plane strain under a finite mean deformation, the counterpart of the reference's
``scripts/generate_dataset_hyperelast.py`` (fedoo ``"2Dplane"``, simcoon ``"NEOHC"`` with ``mu = 2 C10 = 3``,
``kappa = 10``, ``nlgeom=True``, periodicity imposed on ``F - I``, the load applied in increments).

    sol = solve_cell(points, faces, strain=(0.15, -0.10, 0.08))   # the logarithmic strain, or F=[[..], [..]]
    sol.stress, sol.mean_stress, sol.deformed, sol.table          # (N, 3) fp32 Cauchy, (3,) fp64, (N, 2), (1, 6)
    data = hyper_targets(points, faces, strain)                   # a Data; op_div_matrix on the deformed mesh
    write_sample(folder, 0, points, faces, strain)                # .vtk + .npz + dataset.csv row

``u(X) = (Fbar - I) X + ut(X)`` with ``ut`` periodic; per element ``F = Fbar + grad ut``, ``F3 = diag(F, 1)``,
``I1 = tr(F^T F) + 1``, ``J = det F`` and

    W = mu / 2 (J^(-2/3) I1 - 3) + U(J),   U = kappa (J ln J - J + 1)  (volumetric="log", the default)
                                           U = kappa / 2 (J - 1)^2     (volumetric="quadratic")

Which of the two simcoon's NEOHC uses cannot be pinned here.  ``Fbar = exp(eps)`` of the logarithmic
strain ``eps = [[exx, gxy / 2], [gxy / 2, eyy]]``, as ``simcoon.eR_to_F`` with no rotation.  Stress is the Cauchy
stress (xx, yy, xy), strain the logarithmic strain ``1/2 ln(F F^T)`` as (xx, yy, 2 xy).

``solve_cells`` reuses ``fem.FemPlan`` and ``fem.element_table`` and runs ``pdg_hyper_solve`` (one persistent
workgroup per graph and load case: load steps, Newton with a backtracking line search on the energy, matrix-free
Jacobi-preconditioned conjugate gradients inside) and ``pdg_hyper_stress`` (nodal fields, volume sums).
``table[g, l]`` = ``COLUMNS``; ``STATUS`` names the last column (the linear solver's codes; ``TRIVIAL`` is not used: a
plate without a hole is ``CONVERGED`` with no iteration and ``ut = 0``).  Nothing is read back after the solve: a
caller who needs convergence checked reads ``table[..., 5]``.

Triangles only (quad meshes go to ``gnn_local_stress.hyperelastic_q1``); CPU tensors raise (the CPU restatement is test-only, tests/hyper_ref.py).
"""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path

import numpy as np
import torch

from pdg.graph import Data
from pdg.lib import lib, stream_handle

from . import fem
from .fem import FemPlan, element_table

COLUMNS = ("load_steps", "newton_iterations", "pcg_iterations", "force_norm", "residual", "status")
CONVERGED, TRIVIAL, MAX_ITER, BREAKDOWN = fem.CONVERGED, fem.TRIVIAL, fem.MAX_ITER, fem.BREAKDOWN
STATUS = fem.STATUS
NODAL = fem.NODAL
VOLUMETRIC = ("log", "quadratic")
MU, KAPPA = 3.0, 10.0
MAX_CASES = fem.MAX_CASES
MAX_STEPS, MAX_NEWTON_CAP, MAX_PCG_CAP = 10000, 1000, 100000
# the kernel's line search (csrc/pdg_hyper.hip): Phi(x + alpha d) <= Phi(x) - ARMIJO alpha r.d + PHI_NOISE |Phi|, alpha
# halved at most HALVINGS times; |Phi| is the sum of the energy terms' magnitudes before they cancel
ARMIJO, HALVINGS, PHI_NOISE = 1e-4, 10, 32.0 * 2.0 ** -52


def _law(mu: float, kappa: float, volumetric: str) -> tuple[float, float, int]:
    mu, kappa = float(mu), float(kappa)
    if not (0.0 < mu < float("inf")):
        raise ValueError(f"mu must be finite and > 0, got {mu}")
    if not (0.0 < kappa < float("inf")):
        raise ValueError(f"kappa must be finite and > 0, got {kappa}")
    if volumetric not in VOLUMETRIC:
        raise ValueError(f"volumetric is one of {VOLUMETRIC}, got {volumetric!r}")
    return mu, kappa, VOLUMETRIC.index(volumetric)


def deformation_gradient(strain) -> torch.Tensor:
    """(2, 2) fp64 on the host: ``Fbar = exp([[exx, gxy / 2], [gxy / 2, eyy]])`` of the logarithmic strain
    (exx, eyy, gxy)."""
    e = torch.as_tensor(strain, dtype=torch.float64).reshape(-1).cpu()
    if e.numel() != 3:
        raise ValueError(f"strain holds 3 values (xx, yy, xy), got {e.numel()}")
    if not bool(torch.isfinite(e).all()):
        raise ValueError("strain must be finite")
    return torch.linalg.matrix_exp(torch.stack([torch.stack([e[0], e[2] / 2]), torch.stack([e[2] / 2, e[1]])]))


@dataclass
class HyperFields:
    """``solve_cells``' result, everything on the device.  ``stress`` (L, N, 3) fp32: the nodal Cauchy stress;
    ``log_strain`` (L, N, 3) fp32; ``mean_stress`` (B, L, 3) fp64: the Cauchy mean over the deformed cell,
    ``sum area J sigma / (det Fbar cell_area)``; ``mean_stress_material`` the same sum over the deformed material
    area; ``mean_pk1`` (B, L, 2, 2) fp64: ``sum area P / cell_area``; ``ut`` (L, N, 2) fp64; ``deformed`` (L, N, 2)
    fp32: ``Fbar X + ut``; ``table`` (B, L, 6) fp64 (``COLUMNS``); ``material_area`` / ``cell_area`` (B,) fp64, both
    undeformed."""
    stress: torch.Tensor
    log_strain: torch.Tensor
    mean_stress: torch.Tensor
    mean_stress_material: torch.Tensor
    mean_pk1: torch.Tensor
    ut: torch.Tensor
    deformed: torch.Tensor
    table: torch.Tensor
    material_area: torch.Tensor
    cell_area: torch.Tensor


def solve_cells(plan: FemPlan, points: torch.Tensor, F, mu: float = MU, kappa: float = KAPPA,
                volumetric: str = "log", rtol: float = 1e-10, n_steps: int = 10, max_newton: int = 25,
                eta: float = 1e-4, max_pcg: int = 4000, nodal: str = "area",
                elements: torch.Tensor | None = None) -> HyperFields:
    """The cell problem of every graph of ``plan`` under every load case: ``F`` (B, L, 2, 2) (or (B, L, 4), row-major)
    the mean deformation gradients.  The load is applied in ``n_steps`` equal increments of ``F - I``; ``max_newton``
    caps the Newton iterations of one increment (clamped to [0, 1000]), ``max_pcg`` the inner iterations of one
    Newton iteration (clamped to [1, 100000]), which stop at ``|r_k| <= eta |r_0|``; an increment has converged at
    ``|r|_2 <= rtol |f_abs|_2``.  ``elements``: ``fem.element_table(plan, points)`` built beforehand; the call then
    reads nothing back and can be captured into a HIP graph (while a stream is capturing the table must be passed,
    and ``F`` is not checked: the kernel answers a value that is not finite with ``BREAKDOWN`` and NaN rows)."""
    pts = fem._plan_points(plan, points, "hyperelastic.solve_cells")
    mu, kappa, vol = _law(mu, kappa, volumetric)
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
        raise RuntimeError("solve_cells under stream capture needs elements=fem.element_table(plan, points), built "
                           "before the capture (its status is read on the host)")
    det = fb[..., 0] * fb[..., 3] - fb[..., 1] * fb[..., 2]
    if not capturing:
        if not bool(torch.isfinite(fb).all()):
            raise ValueError("F must be finite")
        if not bool((det > 0).all()):
            raise ValueError("det F must be > 0 for every load case")
    b, cases, n, nf = plan.n_graphs, fb.shape[1], plan.n_nodes, plan.n_faces
    elem = element_table(plan, pts) if elements is None else elements
    if elem.shape != (nf, 8) or elem.dtype != torch.float64 or elem.device != dev:
        raise ValueError(f"elements must be element_table's ({nf}, 8) fp64 tensor on the points' device")
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
        nbytes = lib.pdg_hyper_solve_scratch_bytes(n, nf, cases)
        if nbytes < 0:
            raise ValueError(f"solve_cells: unsupported sizes (nodes {n}, faces {nf}, load cases {cases})")
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        s = stream_handle(dev)
        lib.pdg_hyper_solve(b, cases, plan.ptr.data_ptr(), plan.fptr.data_ptr(), n, nf, plan.rverts.data_ptr(),
                            plan.rep.data_ptr(), plan.item_rowptr.data_ptr(), plan.item.data_ptr(), elem.data_ptr(),
                            fb.data_ptr(), mu, kappa, vol, rtol, n_steps, max_newton, eta, max_pcg, ut.data_ptr(),
                            table.data_ptr(), scratch.data_ptr(), nbytes, s)
        lib.pdg_hyper_stress(b, cases, plan.ptr.data_ptr(), plan.fptr.data_ptr(), n, pts.data_ptr(), pts.shape[1], nf,
                             plan.verts.data_ptr(), plan.rep.data_ptr(), plan.item_rowptr.data_ptr(),
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


@dataclass
class HyperSolution:
    """``solve_cell``'s result for one mesh, on the device.  ``stress`` / ``log_strain`` (N, 3) fp32; ``mean_stress``
    (3,) fp64, the Cauchy mean over the deformed cell; ``mean_stress_material`` (3,); ``mean_pk1`` (2, 2) fp64;
    ``F`` (2, 2) fp64, the imposed mean deformation gradient; ``mean_strain`` (3,) fp64, its logarithmic strain
    (exx, eyy, gxy); ``ut`` (N, 2) fp64; ``deformed`` (N, 2) fp32; ``table`` (1, 6) fp64; ``material_area`` /
    ``cell_area`` () fp64 (undeformed)."""
    stress: torch.Tensor
    log_strain: torch.Tensor
    mean_stress: torch.Tensor
    mean_stress_material: torch.Tensor
    mean_pk1: torch.Tensor
    F: torch.Tensor
    mean_strain: torch.Tensor
    ut: torch.Tensor
    deformed: torch.Tensor
    table: torch.Tensor
    material_area: torch.Tensor
    cell_area: torch.Tensor


def _log_strain_of(f: torch.Tensor) -> torch.Tensor:
    """(3,) the logarithmic strain (xx, yy, 2 xy) of a (2, 2) fp64 F on the host: 1/2 ln(F F^T)."""
    lam, vec = torch.linalg.eigh(f @ f.T)
    e = (vec * (0.5 * torch.log(lam))) @ vec.T
    return torch.stack([e[0, 0], e[1, 1], 2 * e[0, 1]])


def solve_cell(points: torch.Tensor, faces: torch.Tensor, strain=None, F=None, cells: str = "triangle",
               **kw) -> HyperSolution:
    """One mesh under an imposed mean deformation: ``strain`` = the logarithmic (exx, eyy, gxy), with
    ``Fbar = matrix_exp([[exx, gxy / 2], [gxy / 2, eyy]])`` in fp64, or ``F`` (2, 2) itself.  Keywords as
    ``solve_cells``."""
    if (strain is None) == (F is None):
        raise ValueError("give exactly one of strain= and F=")
    fem._cells(cells)
    fem._device_mesh(points, faces, "hyperelastic.solve_cell")
    if strain is not None:
        fbar = deformation_gradient(strain)
        eps = torch.as_tensor(strain, dtype=torch.float64).reshape(3).cpu()
    else:
        fbar = torch.as_tensor(F, dtype=torch.float64).reshape(2, 2).cpu()
        if not bool(torch.isfinite(fbar).all()):
            raise ValueError("F must be finite")
        if not float(torch.linalg.det(fbar)) > 0.0:
            raise ValueError("det F must be > 0")
        eps = _log_strain_of(fbar)
    plan = FemPlan.from_mesh(points, faces)
    dev = plan.rep.device
    f = solve_cells(plan, points, fbar.reshape(1, 1, 4).to(dev), **kw)
    return HyperSolution(f.stress[0], f.log_strain[0], f.mean_stress[0, 0], f.mean_stress_material[0, 0],
                         f.mean_pk1[0, 0], fbar.to(dev), eps.to(dev), f.ut[0], f.deformed[0], f.table[0],
                         f.material_area[0], f.cell_area[0])


def hyper_targets(points: torch.Tensor, faces: torch.Tensor, strain, periodic: bool = True, cells: str = "triangle",
                  **kw) -> Data:
    """The graph ``convert_mesh_to_graph`` builds from the undeformed points, with ``local_stress`` (N, 3) and
    ``mean_stress`` (broadcast to every node) from the hyperelastic solve under the logarithmic mean ``strain``, and
    ``op_div_matrix`` built on the deformed mesh (``devgraph.p1_divergence(sol.deformed, faces)``), as the reference
    takes it from ``assemb.current.mesh``.  The solution is kept as ``data.fem`` (``HyperSolution``).  Keywords as
    ``solve_cell``."""
    from pdg import devgraph
    sol = solve_cell(points, faces, strain=strain, cells=cells, **kw)
    pts, fcs = fem._device_mesh(points, faces, "hyper_targets")
    labels = devgraph.node_labels(pts, fcs, strict=False)
    data = devgraph.convert_mesh_to_graph(pts, fcs, sol.mean_stress.float(), labels, periodic, False)
    data.op_div_matrix = devgraph.p1_divergence(sol.deformed, fcs)
    data.local_stress = sol.stress
    data.fem = sol
    return data


def write_sample(folder, index: int, points: torch.Tensor, faces: torch.Tensor, strain, meta: dict | None = None,
                 **kw) -> dict:
    """One sample of the reference's hyperelastic dataset (``scripts/generate_dataset_hyperelast.py``), which
    ``datasets.load_sample`` reads back: ``meshes/hole_plate_mesh_{index}.vtk`` (the undeformed mesh),
    ``fields/hole_plate_mesh_{index}.npz`` with the reference's keys (``stress_field``, ``mean_stress``,
    ``mean_strain``, ``op_div_matrix_*`` on the deformed mesh, ``node_labels``) plus ``mean_stress_reference_mesh``,
    and a row of ``dataset.csv`` with ``fem.CSV_COLUMNS`` (the ``*_material`` columns hold the Cauchy mean over the
    deformed material).  ``mean_stress`` is the Cauchy mean over the deformed cell;
    ``mean_stress_reference_mesh`` is the reference's own formula, the nodal stress integrated with the undeformed
    nodal areas over the deformed cell area (the two differ on purpose).  ``meta`` as
    ``fem.write_sample``.  Returns the row.  Keywords as ``solve_cell``."""
    import pandas as pd
    from pdg import devgraph
    from .vtk_io import write_legacy_vtk
    sol = solve_cell(points, faces, strain=strain, **kw)
    pts, fcs = fem._device_mesh(points, faces, "write_sample")
    op = devgraph.p1_divergence(sol.deformed, fcs)
    areas = devgraph.nodal_areas(pts, fcs)
    labels = devgraph.node_labels(pts, fcs, strict=False)
    ref_mean = (areas.area.double().unsqueeze(1) * sol.stress.double()).sum(0)
    ref_mean = ref_mean / (torch.linalg.det(sol.F) * areas.cell_area)
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
             mean_stress_reference_mesh=ref_mean.cpu().numpy(), op_div_matrix_data=op.values().cpu().numpy(),
             op_div_matrix_col_indices=idx[1].astype(np.int32), op_div_matrix_row_indices=idx[0].astype(np.int32),
             op_div_matrix_shape=np.array(op.shape), node_labels=labels.cpu().numpy())
    row = {c: float("nan") for c in fem.CSV_COLUMNS}
    row.update(mesh_filename=mesh_filename, data_filename=data_filename, mean_stress_x=ms[0], mean_stress_y=ms[1],
               mean_stress_xy=ms[2], mean_strain_x=eps[0], mean_strain_y=eps[1], mean_strain_xy=eps[2],
               mean_stress_x_material=msm[0], mean_stress_y_material=msm[1], mean_stress_xy_material=msm[2],
               plate_width=float(p[:, 0].max() - p[:, 0].min()), plate_height=float(p[:, 1].max() - p[:, 1].min()),
               n_nodes=int(p.shape[0]), n_elements=int(fcs.shape[0]))
    for k, v in (meta or {}).items():
        if k not in fem.CSV_COLUMNS or k in ("mesh_filename", "data_filename"):
            raise ValueError(f"meta: {k!r} is not a column write_sample leaves open")
        row[k] = v
    csv = folder / "dataset.csv"
    frame = pd.DataFrame([row], columns=list(fem.CSV_COLUMNS))
    if csv.is_file():
        old = pd.read_csv(csv)
        frame = pd.concat([old[old["mesh_filename"] != mesh_filename], frame], ignore_index=True)
    frame.to_csv(csv.as_posix(), index=False)
    return row
