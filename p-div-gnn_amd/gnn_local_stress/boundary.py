"""Boundary residuals of a predicted stress field on the HIP kernels (csrc/pdg_boundary.hip): how hard the field
pushes on the traction-free hole, the net forces on the hole and on the cell, and the jump across the periodic
connections; and the gradient of the two mean squares with respect to the field.

    g = convert_mesh_to_graph(points, faces, load, boundary=True)      # g.boundary_vec (N, 2), g.boundary_len (N,)
    r = boundary_residuals(sigma, batch)                               # r.traction_rms, r.hole_force, r.periodic_rms
    d = boundary_residuals_grad(sigma, batch, traction=1.0, periodic=0.5)     # (N, 3)

The divergence check excludes the boundary rows (``losses.compute_divergence``), so nothing else looks at the
field where the physics is set.  With the lumped outward boundary vectors m (``pdg.devgraph.boundary_vectors``:
1/2 sum length * n_outward over the boundary edges at a node, and l, 1/2 sum length), the nodal boundary force is
f(n) = sigma(n) . m(n), that is fx = sxx mx + sxy my and fy = sxy mx + syy my: the lumped traction integral.

* The hole's edge (``nodes_types`` -1) is traction free: ``T2`` = sum |f|^2 / l is the integral of the squared
  traction over it, ``L_int`` = sum l its length, ``traction_rms`` = sqrt(T2 / L_int); ``traction_max`` is the
  largest |f| / l and ``argmax`` / ``node`` the first node that attains it; ``hole_force`` = sum f is the net force
  on the hole, 0 for a traction-free one.
* ``cell_force`` = sum f over the external boundary (+1, length ``L_ext``) is 0 for any periodic field in
  equilibrium.
* The cell is periodic: sigma takes the same value at the two ends of every periodic connection (the zero-length
  edges of ``compute_periodic_graph`` / ``pdg_mesh_graph``).  ``P2`` = 1/2 sum over nodes n and the periodic edges
  into n of |sigma(n) - sigma(src)|^2, ``n_pairs`` = 1/2 the number of those edges, ``periodic_rms`` =
  sqrt(P2 / n_pairs).

A node takes part in the traction sums if and only if its label is +1 or -1 and its boundary length is > 0 (the
criteria's rule: 0, negative and NaN lengths exclude it).  0 / 0 is NaN and stays NaN: a plate without a hole has no
hole traction and a non-periodic graph no jump.  A NaN traction at a participating node gives NaN sums and
``argmax`` -1.  The gradient of the periodic term is the full gradient when the periodic connections appear in
both directions, as ``compute_periodic_graph`` and ``pdg_mesh_graph`` build them and ``coalesce`` keeps them.  A
graph whose denominator is 0 under a non-zero weight has no mean square; its gradient rows are zero where no node
takes part and NaN where one does.

Values are fp64 per graph (fp64 arithmetic on the fp32 field, one workgroup per graph in a fixed order: a graph gets
bitwise the same values alone and inside any batch), gradients fp32 rounded once.  CPU tensors raise, as everywhere
on the HIP path.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from pdg.lib import lib, ptr as _p, stream_handle
from pdg.plan import plan_for

from .criteria import _field3, _ptr_of


@dataclass
class BoundaryResiduals:
    """``L_int``, ``L_ext``, ``T2``, ``P2``, ``n_pairs`` (B,) and ``F_int``, ``F_ext`` (B, 2) fp64: the table of
    ``pdg_boundary_residuals``.  ``traction_rms`` = sqrt(T2 / L_int), ``traction_max`` = max |f| / l over the hole's
    edge (NaN without one), ``periodic_rms`` = sqrt(P2 / n_pairs), all (B,) fp64; ``hole_force`` and ``cell_force``
    are ``F_int`` and ``F_ext``; ``argmax`` (B,) int64, the graph-local index of the first participating -1 node
    that attains ``traction_max`` (-1 without one or for a NaN graph) and ``node`` the same as an index into the
    batch's nodes."""
    L_int: torch.Tensor
    L_ext: torch.Tensor
    T2: torch.Tensor
    F_int: torch.Tensor
    F_ext: torch.Tensor
    P2: torch.Tensor
    n_pairs: torch.Tensor
    traction_rms: torch.Tensor
    traction_max: torch.Tensor
    hole_force: torch.Tensor
    cell_force: torch.Tensor
    periodic_rms: torch.Tensor
    argmax: torch.Tensor
    node: torch.Tensor


@dataclass
class _Inputs:
    sigma: torch.Tensor
    ptr: torch.Tensor
    vec: torch.Tensor
    length: torch.Tensor
    labels: torch.Tensor
    edges: tuple   # (rowptr_dst, src, perm, edge_attr) or four Nones


def _of_batch(batch, key: str):
    return None if batch is None or isinstance(batch, torch.Tensor) else batch.__dict__.get(key)


def _node_tensor(t, n: int, cols: int | None, dtype, dev, what: str) -> torch.Tensor:
    if t.device.type != "cuda":
        raise RuntimeError(f"boundary residuals run on the MI355X HIP path only; move {what} to a HIP device")
    shape = (n,) if cols is None else (n, cols)
    if t.numel() != n * (cols or 1) or (cols is not None and tuple(t.shape) != shape):
        raise ValueError(f"{what} must be {shape}, got {tuple(t.shape)}")
    return t.detach().reshape(shape).to(device=dev, dtype=dtype).contiguous()


def _setup(sigma, batch, boundary_vec, boundary_len, periodic: bool, labels=None) -> _Inputs:
    s = _field3(sigma)
    n, dev = s.shape[0], s.device
    ptr = _ptr_of(batch, n, dev)
    vec = boundary_vec if boundary_vec is not None else _of_batch(batch, "boundary_vec")
    length = boundary_len if boundary_len is not None else _of_batch(batch, "boundary_len")
    if vec is None or length is None:
        raise ValueError("boundary vectors are needed: pass boundary_vec and boundary_len "
                         "(pdg.devgraph.boundary_vectors) or build the graph with "
                         "convert_mesh_to_graph(..., boundary=True)")
    if labels is None:
        labels = _of_batch(batch, "nodes_types")
    if labels is None:
        raise ValueError("node labels are needed: the batch holds no nodes_types")
    edges = (None, None, None, None)
    if periodic:
        if batch is None or isinstance(batch, torch.Tensor) or batch.__dict__.get("edge_index") is None \
                or batch.__dict__.get("edge_attr") is None:
            raise ValueError("periodic=True needs the batch's edge_index and edge_attr; pass periodic=False for the "
                             "traction columns alone")
        if batch.edge_index.device.type != "cuda":
            raise RuntimeError("boundary residuals run on the MI355X HIP path only; move the batch to a HIP device")
        plan = plan_for(batch)
        plan.validate()
        ea = batch.edge_attr
        if ea.numel() != plan.n_edges or plan.n_nodes != n:
            raise ValueError(f"the batch's graph ({plan.n_nodes} nodes, {plan.n_edges} edges, {ea.numel()} edge "
                             f"lengths) does not match the field's {n} rows")
        if plan.n_edges:
            edges = (plan.rowptr_dst, plan.src, plan.perm,
                     ea.detach().reshape(-1).to(device=dev, dtype=torch.float32).contiguous())
    return _Inputs(s, ptr, _node_tensor(vec, n, 2, torch.float32, dev, "boundary_vec"),
                   _node_tensor(length, n, None, torch.float32, dev, "boundary_len"),
                   _node_tensor(labels, n, None, torch.int64, dev, "nodes_types"), edges)


def _forward(a: _Inputs):
    dev, b = a.sigma.device, a.ptr.numel() - 1
    table = torch.empty(b, 9, dtype=torch.float64, device=dev)
    argmax = torch.empty(b, dtype=torch.int32, device=dev)
    lib.pdg_boundary_residuals(b, a.ptr.data_ptr(), a.sigma.data_ptr(), a.vec.data_ptr(), a.length.data_ptr(),
                               a.labels.data_ptr(), *(_p(e) for e in a.edges), table.data_ptr(), argmax.data_ptr(),
                               stream_handle(dev))
    return table, argmax


def _weight(w, b: int, dev, what: str) -> torch.Tensor:
    if isinstance(w, torch.Tensor):
        if w.numel() != b and w.numel() != 1:
            raise ValueError(f"{what} must be a scalar or hold one value per graph ({b}), got {tuple(w.shape)}")
        if w.numel() == b and w.device.type != "cuda":
            raise RuntimeError(f"boundary residuals run on the MI355X HIP path only; move {what} to a HIP device")
        w = w.detach().reshape(-1).to(device=dev, dtype=torch.float64)
        return (w.expand(b) if w.numel() != b else w).contiguous()
    return torch.full((b,), float(w), dtype=torch.float64, device=dev)


def _grad(a: _Inputs, traction, periodic):
    """(table, argmax, g_sigma): the two launches on one field."""
    dev, b = a.sigma.device, a.ptr.numel() - 1
    gt, gp = _weight(traction, b, dev, "traction"), _weight(periodic, b, dev, "periodic")
    table, argmax = _forward(a)
    out = torch.empty_like(a.sigma)
    lib.pdg_boundary_residuals_bwd(b, a.ptr.data_ptr(), a.sigma.data_ptr(), a.vec.data_ptr(), a.length.data_ptr(),
                                   a.labels.data_ptr(), *(_p(e) for e in a.edges), table.data_ptr(), gt.data_ptr(),
                                   gp.data_ptr(), out.data_ptr(), stream_handle(dev))
    return table, argmax, out


def _result(a: _Inputs, table: torch.Tensor, argmax: torch.Tensor) -> BoundaryResiduals:
    am = argmax.long()
    node = torch.where(am >= 0, am + a.ptr[:-1].long(), am)
    # |f| / l at the maximum's node, formed from the same fp32 rows (NaN where there is none)
    at = node.clamp(min=0)
    s, m, l = a.sigma.double()[at], a.vec.double()[at], a.length.double()[at]
    fx, fy = s[:, 0] * m[:, 0] + s[:, 2] * m[:, 1], s[:, 2] * m[:, 0] + s[:, 1] * m[:, 1]
    tmax = torch.where(am >= 0, torch.sqrt(fx * fx + fy * fy) / l, torch.full_like(l, float("nan")))
    return BoundaryResiduals(L_int=table[:, 0], L_ext=table[:, 1], T2=table[:, 2], F_int=table[:, 3:5],
                             F_ext=table[:, 5:7], P2=table[:, 7], n_pairs=table[:, 8],
                             traction_rms=torch.sqrt(table[:, 2] / table[:, 0]), traction_max=tmax,
                             hole_force=table[:, 3:5], cell_force=table[:, 5:7],
                             periodic_rms=torch.sqrt(table[:, 7] / table[:, 8]), argmax=am, node=node)


def boundary_residuals(sigma: torch.Tensor, batch, boundary_vec=None, boundary_len=None,
                       periodic: bool = True) -> BoundaryResiduals:
    """The per-graph boundary residuals of ``sigma`` (N, 3), in one launch (``pdg_boundary_residuals``).  ``batch``:
    a ``Batch`` or a single ``Data`` (its ``nodes_types``, and with ``periodic`` its ``edge_index`` and
    ``edge_attr``).  ``boundary_vec`` (N, 2) and ``boundary_len`` (N,) default to the batch's
    (``convert_mesh_to_graph(..., boundary=True)``).  ``periodic=True`` builds or reuses ``plan_for(batch)`` and
    passes its arrays; ``periodic=False`` leaves the periodic columns 0 (``periodic_rms`` NaN)."""
    a = _setup(sigma, batch, boundary_vec, boundary_len, bool(periodic))
    if a.sigma.shape[0] == 0:
        raise ValueError("an empty field has no boundary")
    return _result(a, *_forward(a))


def boundary_residuals_grad(sigma: torch.Tensor, batch, traction=1.0, periodic=0.0, boundary_vec=None,
                            boundary_len=None) -> torch.Tensor:
    """(N, 3) fp32: the gradient with respect to ``sigma`` of sum_g traction[g] T2_g / L_int,g + periodic[g] P2_g /
    n_pairs,g, the mean-square hole traction and the mean-square periodic jump, in two launches
    (``pdg_boundary_residuals``, ``pdg_boundary_residuals_bwd``).  The two weights are scalars or (B,) tensors.
    Rows that take no part get exact zeros; see the module docstring for the NaN rule and the precondition of the
    periodic term.  The graph plan is built (or reused) whenever the batch has edges; a batch without edges takes
    the traction term alone (``periodic`` must then be 0)."""
    has_edges = _of_batch(batch, "edge_index") is not None and _of_batch(batch, "edge_attr") is not None
    if not has_edges and not (isinstance(periodic, (int, float)) and periodic == 0):
        raise ValueError("a periodic weight needs the batch's edge_index and edge_attr")
    a = _setup(sigma, batch, boundary_vec, boundary_len, has_edges)
    if a.sigma.shape[0] == 0:
        raise ValueError("an empty field has no boundary")
    return _grad(a, traction, periodic)[2]
