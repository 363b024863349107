"""Equilibration of a predicted stress field on the HIP kernel (csrc/pdg_equil.hip): the hard correction for the
network's defining property, div sigma = 0 at the interior nodes.

    b = store.batch(idx)                                 # DeviceGraphStore(..., mesh_fields=True): b.node_area
    s = equilibrate(sigma, b)                            # (N, 3): the closest field with C s = 0
    s, info = equilibrate(sigma, b, return_info=True)    # info (B, 4) fp64 on the device, never read back here
    g = equilibrate_grad(g_out, b)                       # P^T g_out, the vector-Jacobian product of sigma -> s
    d = divergence_defect(sigma, b)                      # (B,) fp64: |C sigma|_2

``C`` is the batch's divergence operator exactly as the training penalty reads it (``pdg_div_fwd``), restricted to
the rows with ``node_types == 0``; "closest" is in the weighted Frobenius norm of the tensor field,
``|t|^2_W = sum_v w_v (t_xx^2 + t_yy^2 + 2 t_xy^2)``, with ``w`` the nodal areas (``weights="area"``), ones
(``None``) or a tensor of positive weights.  With ``S = C W^-1 C^T``:

    S lam = C sigma,   sigma' = sigma - W^-1 C^T lam            (equilibrate)
    S mu  = C W^-1 g,  P^T g  = g - C^T mu                      (equilibrate_grad)

solved per graph by conjugate gradients on ``S`` in one launch (``pdg_equilibrate``), fp32 vectors and fp64 sums in
a fixed order: a graph's rows are bitwise the same alone and inside any batch.  The iteration stops at a recurrence
residual of ``rtol |C sigma|_2`` or after ``max_iter`` steps.  ``info[g]`` = (``|C sigma|_2``, the true final
residual ``|C sigma'|_2`` recomputed in fp64 from the stored field, the iterations run, status bits: 1 not converged,
2 true residual above ``2 rtol |C sigma|_2``, 4 a weight of the graph <= 0 or not finite, the graph's rows then
returned unchanged).  A graph with nothing to remove (no interior node, no operator, a zero field) runs no
iteration and returns its rows bitwise.

The field is unstandardised, (N, 3) in xx, yy, xy order, and must not require grad: the projection has no autograd
route, ``equilibrate_grad`` is its transpose.  CPU tensors raise, as everywhere on the HIP path (the CPU
restatement is test-only, tests/equil_ref.py).
"""
from __future__ import annotations

import torch

from pdg.lib import lib, ptr as _p, stream_handle
from pdg.plan import GraphPlan, plan_for

from . import homogenise
from .criteria import _weights_of

COLUMNS = ("defect", "residual", "iterations", "status")
NOT_CONVERGED, ABOVE_TWICE_RTOL, BAD_WEIGHT = 1, 2, 4


def _field(x: torch.Tensor, what: str) -> torch.Tensor:
    if x.device.type != "cuda":
        raise RuntimeError("equilibration runs on the MI355X HIP path only; move the field to a HIP device (the "
                           "CPU restatement is test-only, tests/equil_ref.py)")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{what} is (N, 3) in xx, yy, xy order, got {tuple(x.shape)}")
    if x.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("equilibrate has no autograd route: detach the field, and use equilibrate_grad (P^T) for "
                           "gradients")
    return x.detach().float().contiguous()


def _plan_of(batch, n: int, dev) -> GraphPlan:
    """The batch's plan with its divergence operator: ``plan_for`` for a ``Batch``, a divergence-only plan for a
    single ``Data`` that carries ``op_div_matrix`` (kept on it)."""
    d = None if isinstance(batch, torch.Tensor) else getattr(batch, "__dict__", None)
    if d is None:
        raise ValueError("equilibration needs the batch's divergence operator: pass a Batch or a Data, not offsets")
    if d.get("op_div_rows") is not None:
        plan = plan_for(batch)
    else:
        op = d.get("op_div_matrix")
        if op is None:
            raise ValueError("the batch has no divergence operator (op_div_matrix): build the graph with "
                             "divergence=True")
        cached = d.get("_equil_plan_cache")
        if cached is not None and cached[0] is op and cached[1].ptr.device == dev:
            plan = cached[1]
        else:
            from .losses import _SinglePlan
            plan = _SinglePlan.get(n, dev, op)
            d["_equil_plan_cache"] = (op, plan)
    if not plan.has_div:
        raise ValueError("the batch has no divergence operator")
    if plan.n_nodes != n:
        raise ValueError(f"the field has {n} rows, the batch {plan.n_nodes} nodes")
    if plan.ptr.device != dev:
        raise RuntimeError("the batch and the field must live on the same HIP device")
    return plan


def _types_of(batch, n: int, dev) -> torch.Tensor:
    t = batch.surfaces_nodes_for_div if batch.surfaces_nodes_for_div is not None else batch.nodes_types
    if t is None:
        raise ValueError("the batch has no node types (nodes_types)")
    t = t.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    if t.numel() != n:
        raise ValueError(f"{t.numel()} node types for {n} nodes")
    return t


def _metric(weights, batch, n: int, dev):
    if isinstance(weights, str):
        if weights != "area":
            raise ValueError(f"weights is 'area', None or a tensor, got {weights!r}")
        area = homogenise._of_batch(batch, "node_area")
        if area is None:
            raise ValueError("weights='area' needs the batch's nodal areas (node_area): build the store with "
                             "DeviceGraphStore(..., mesh_fields=True) or the graph with areas=True, or pass weights")
        weights = area
    return _weights_of(weights, n, dev)


def _solve(x: torch.Tensor, batch, weights, rtol: float, max_iter: int, transpose: bool):
    dev, n = x.device, x.shape[0]
    rtol, max_iter = float(rtol), int(max_iter)
    if not (0.0 < rtol < float("inf")):
        raise ValueError(f"rtol must be finite and > 0, got {rtol}")
    if max_iter < 0:
        raise ValueError(f"max_iter must be >= 0, got {max_iter}")
    plan = _plan_of(batch, n, dev)
    types = _types_of(batch, n, dev)
    w = _metric(weights, batch, n, dev)
    b = plan.n_graphs
    out = torch.empty_like(x)
    table = torch.empty(b, 4, dtype=torch.float64, device=dev)
    if n == 0:
        return out, table.fill_(float("nan"))
    nbytes = lib.pdg_equilibrate_scratch_bytes(n, b)
    if nbytes < 0:
        raise ValueError(f"equilibrate: unsupported sizes (nodes {n}, graphs {b})")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    # an operator without entries has empty (NULL) entry arrays; the kernel reads none of them
    a_col, a_val, at_row, at_comp, at_val = (
        t if t.numel() else plan.a_rowptr for t in (plan.a_col, plan.a_val, plan.at_row, plan.at_comp, plan.at_val))
    lib.pdg_equilibrate(b, plan.ptr.data_ptr(), n, plan.a_rowptr.data_ptr(), a_col.data_ptr(), a_val.data_ptr(),
                        plan.at_rowptr.data_ptr(), at_row.data_ptr(), at_comp.data_ptr(), at_val.data_ptr(),
                        types.data_ptr(), _p(w), x.data_ptr(), int(transpose), rtol, max_iter, out.data_ptr(),
                        table.data_ptr(), scratch.data_ptr(), nbytes, stream_handle(dev))
    return out, table


def equilibrate(sigma: torch.Tensor, batch, weights="area", rtol: float = 1e-5, max_iter: int = 1000,
                mean: str | None = None, return_info: bool = False):
    """(N, 3) fp32: the field closest to ``sigma`` in the ``weights`` norm whose divergence vanishes at the interior
    nodes of every graph of ``batch`` (module docstring).  ``batch``: a ``Batch`` or a single ``Data`` with its
    divergence operator and node types.  ``weights``: ``"area"`` for the nodal areas the batch carries (the source
    ``homogenise.graph_average`` uses; a batch without them is refused), ``None`` for ones, or an (N,) tensor of
    positive weights.  ``return_info`` also returns the (B, 4) fp64 table on the device (``COLUMNS``); nothing is
    read back here, so a caller who needs convergence checked reads ``info[:, 3]``.

    ``mean`` = ``"cell"`` or ``"material"`` applies ``homogenise.enforce_mean`` with that convention (and the
    batch's ``mean_stress``, areas and cell area) after the projection.  The constant shift leaves the divergence
    at zero because the device-built operators annihilate constants on the interior rows (row sums of Dx and Dy
    below 1e-8), and projection then shift is exactly the minimiser of the joint problem (C s = 0 and <s> =
    Sigma) when the weights of the volume average are proportional to the weights of the projection: that is
    ``weights="area"`` with the batch's areas.  The multipliers of the projection are then unchanged by the extra
    constraint.  With other weights the result still satisfies both constraints but is not the closest such
    field."""
    if mean is not None:
        homogenise._id(mean, homogenise.CONVENTIONS, "convention")
    out, table = _solve(_field(sigma, "a stress field"), batch, weights, rtol, max_iter, False)
    if mean is not None:
        out = homogenise.enforce_mean(out, batch, convention=mean)
    return (out, table) if return_info else out


def equilibrate_grad(g: torch.Tensor, batch, weights="area", rtol: float = 1e-5, max_iter: int = 1000,
                     return_info: bool = False):
    """(N, 3) fp32: ``P^T g``, the vector-Jacobian product of ``sigma -> equilibrate(sigma)`` (without ``mean``):
    the same solve with the ``W^-1`` on the other side (``pdg_equilibrate`` with ``transpose=1``).  The table's
    first two columns are then ``|C W^-1 g|_2`` and ``|C W^-1 out|_2``.  Arguments as :func:`equilibrate`."""
    out, table = _solve(_field(g, "a gradient field"), batch, weights, rtol, max_iter, True)
    return (out, table) if return_info else out


def divergence_defect(sigma: torch.Tensor, batch) -> torch.Tensor:
    """(B,) fp64 on the device: ``|C sigma|_2`` of every graph, the quantity :func:`equilibrate` removes (column 0
    of a ``max_iter=0`` call; NaN for a graph without nodes)."""
    return _solve(_field(sigma, "a stress field"), batch, None, 1.0, 0, False)[1][:, 0]
