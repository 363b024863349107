"""Volume averages of a nodal field and mean consistency on the HIP kernels (csrc/pdg_homog.hip).

    g = convert_mesh_to_graph(points, faces, load, areas=True)     # g.node_area (N,), g.cell_area (1,)
    a = graph_average(sigma, batch)                                # a.integral, a.mean_cell, a.mean_material, ...
    d = mean_defect(sigma, batch)                                  # (B, 3): <sigma> - Sigma
    s = enforce_mean(sigma, batch)                                 # (N, 3): sigma + the shift that makes d zero

The model's input ``mean_stress`` is, in the reference's datasets, the volume average of the field it is asked to
predict (``scripts/generate_dataset.py:278-289``), so a correct prediction satisfies <sigma> = Sigma.  With the
lumped nodal areas w (``pdg.devgraph.nodal_areas``; for P1 triangles exactly the reference's quadrature weights
gathered to the nodes, ``:73-82``), S = sum w sigma is its ``integrate_field(sigma)`` and W = sum w its
``integrate_field(1)``.  Two conventions:

* ``"cell"``: <sigma> = S / D with D the cell's area, the bounding box (the reference's ``mean_stress``; a hole
  counts as material of zero stress);
* ``"material"``: <sigma> = S / W (the reference's ``mean_stress_material``).

A node takes part if and only if its weight is > 0 (the criteria's rule: 0, negative and NaN weights exclude it);
``weights=None`` without areas on the batch is 1 everywhere, the plain nodal mean.  ``enforce_mean`` adds the
constant (Sigma D - S) / W to every node of the graph, participating or not: a constant c moves S / D by c W / D.
A graph without a participating node has W = 0: its averages are 0 / 0 = NaN and its corrected rows NaN, since a
plain result would hide that it has no average.

Sums are fp64 per graph (fp64 arithmetic on the fp32 field, one workgroup per graph in a fixed order: a graph gets
bitwise the same sums alone and inside any batch), the corrected field fp32 rounded once.  CPU tensors raise, as
everywhere on the HIP path.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from pdg.lib import lib, ptr as _p, stream_handle

from .criteria import _id, _ptr_of, _weights_of

CONVENTIONS = ("cell", "material")
MAX_COLS = 9


@dataclass
class Average:
    """``total_weight`` (B,) = W, ``integral`` (B, C) = S, ``mean_material`` (B, C) = S / W, ``mean_cell`` (B, C) =
    S / D and ``fraction`` (B,) = W / D (the material's share of the cell), both None without a cell area.  All
    fp64."""
    total_weight: torch.Tensor
    integral: torch.Tensor
    mean_material: torch.Tensor
    mean_cell: torch.Tensor | None
    fraction: torch.Tensor | None


def _rows_of(field: torch.Tensor, what: str, cols: int | None = None) -> torch.Tensor:
    if field.dim() not in (1, 2) or (field.dim() == 2 and not 1 <= field.shape[1] <= MAX_COLS):
        raise ValueError(f"{what} is (N,) or (N, C) with 1 <= C <= {MAX_COLS}, got {tuple(field.shape)}")
    if cols is not None and (field.dim() != 2 or field.shape[1] != cols):
        raise ValueError(f"{what} is (N, {cols}) in xx, yy, xy order, got {tuple(field.shape)}")
    if field.device.type != "cuda":
        raise RuntimeError("volume averages run on the MI355X HIP path only; move the field to a HIP device (the "
                           "CPU restatement is test-only, tests/homog_ref.py)")
    return field.detach().float().reshape(field.shape[0], field.shape[1] if field.dim() == 2 else 1).contiguous()


def _of_batch(batch, key: str):
    return None if batch is None or isinstance(batch, torch.Tensor) else batch.__dict__.get(key)


def _cell_area_of(cell_area, batch, b: int, dev):
    if cell_area is None:
        cell_area = _of_batch(batch, "cell_area")
    if cell_area is None:
        return None
    d = torch.as_tensor(cell_area).detach().reshape(-1).to(device=dev, dtype=torch.float64).contiguous()
    if d.numel() != b:
        raise ValueError(f"cell_area must hold one value per graph ({b}), got {d.numel()}")
    return d


def _setup(field, batch, weights, cell_area, what: str, cols: int | None = None):
    """(rows (N, C), ptr (B + 1,), weights or None, cell area (B,) fp64 or None), all on the field's device."""
    rows = _rows_of(field, what, cols)
    n, dev = rows.shape[0], rows.device
    ptr = _ptr_of(batch, n, dev)
    if weights is None:
        weights = _of_batch(batch, "node_area")
    return rows, ptr, _weights_of(weights, n, dev), _cell_area_of(cell_area, batch, ptr.numel() - 1, dev)


def _wmean(ptr, rows, weights) -> torch.Tensor:
    b, c = ptr.numel() - 1, rows.shape[1]
    table = torch.empty(b, c + 1, dtype=torch.float64, device=rows.device)
    lib.pdg_graph_wmean(b, ptr.data_ptr(), rows.data_ptr(), c, _p(weights), table.data_ptr(),
                        stream_handle(rows.device))
    return table


def _average(table: torch.Tensor, cell) -> Average:
    W, S = table[:, 0], table[:, 1:]
    return Average(total_weight=W, integral=S, mean_material=S / W[:, None],
                   mean_cell=None if cell is None else S / cell[:, None],
                   fraction=None if cell is None else W / cell)


def graph_average(field: torch.Tensor, batch, weights=None, cell_area=None) -> Average:
    """The per-graph integral and averages of ``field`` (N,) or (N, C), C <= 9, in one launch
    (``pdg_graph_wmean``).  ``batch``: a ``Batch``, a single ``Data`` or a ``ptr`` tensor of node offsets.
    ``weights`` (N,) and ``cell_area`` (B,) default to the batch's ``node_area`` and ``cell_area`` when it has
    them (``convert_mesh_to_graph(..., areas=True)``); without weights every node counts 1."""
    rows, ptr, w, cell = _setup(field, batch, weights, cell_area, "a nodal field")
    return _average(_wmean(ptr, rows, w), cell)


def _convention(convention: str, cell) -> bool:
    """True for the cell convention."""
    cid = _id(convention, CONVENTIONS, "convention")
    if cid == 0 and cell is None:
        raise ValueError("convention='cell' needs the cell's area: pass cell_area, build the graph with "
                         "areas=True, or use convention='material'")
    return cid == 0


def _target_of(mean_stress, batch, ptr, n: int, dev) -> torch.Tensor:
    """(B, 3) fp32: the imposed mean stress of each graph; by default the first node's row of the batch's
    ``mean_stress``, the load broadcast to every node."""
    b = ptr.numel() - 1
    if mean_stress is None:
        ms = _of_batch(batch, "mean_stress")
        if ms is None:
            raise ValueError("mean_stress is needed: the batch holds none")
        if ms.device.type != "cuda":
            raise RuntimeError("volume averages run on the MI355X HIP path only; move the batch to a HIP device")
        if ms.dim() != 2 or tuple(ms.shape) != (n, 3):
            raise ValueError(f"the batch's mean_stress must be ({n}, 3), got {tuple(ms.shape)}")
        return ms.detach().float()[ptr[:-1].long().clamp(max=max(n - 1, 0))].contiguous()
    t = torch.as_tensor(mean_stress)
    if t.numel() != 3 * b:
        raise ValueError(f"mean_stress must hold 3 values per graph ({b}), got {tuple(t.shape)}")
    return t.detach().reshape(b, 3).to(device=dev, dtype=torch.float32).contiguous()


def mean_defect(sigma: torch.Tensor, batch, mean_stress=None, convention: str = "cell", weights=None,
                cell_area=None) -> torch.Tensor:
    """(B, 3) fp64: <sigma> - Sigma_g, the defect between a field's volume average and the imposed mean stress
    (zero for a mean-consistent prediction).  ``mean_stress`` (B, 3) defaults to row ``ptr[g]`` of the batch's
    ``mean_stress``; ``convention``, ``weights`` and ``cell_area`` as in the module docstring."""
    _id(convention, CONVENTIONS, "convention")
    rows, ptr, w, cell = _setup(sigma, batch, weights, cell_area, "a stress field", 3)
    cellwise = _convention(convention, cell)
    target = _target_of(mean_stress, batch, ptr, rows.shape[0], rows.device)
    avg = _average(_wmean(ptr, rows, w), cell)
    return (avg.mean_cell if cellwise else avg.mean_material) - target.double()


def enforce_mean(sigma: torch.Tensor, batch, mean_stress=None, convention: str = "cell", weights=None,
                 cell_area=None) -> torch.Tensor:
    """(N, 3) fp32: ``sigma`` plus the per-graph constant that makes its volume average equal the imposed mean
    stress, in two launches (``pdg_graph_wmean``, ``pdg_mean_correct``).  Arguments as ``mean_defect``.  The
    rows of a graph without a participating node are NaN."""
    _id(convention, CONVENTIONS, "convention")
    rows, ptr, w, cell = _setup(sigma, batch, weights, cell_area, "a stress field", 3)
    cellwise = _convention(convention, cell)
    target = _target_of(mean_stress, batch, ptr, rows.shape[0], rows.device)
    table = _wmean(ptr, rows, w)
    out = torch.empty_like(rows)
    lib.pdg_mean_correct(ptr.numel() - 1, ptr.data_ptr(), rows.data_ptr(), table.data_ptr(), target.data_ptr(),
                         _p(cell if cellwise else None), out.data_ptr(), stream_handle(rows.device))
    return out
