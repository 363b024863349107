"""Failure criteria of a predicted stress field on the HIP kernels (csrc/pdg_criteria.hip): per-node fields,
per-graph peaks and smooth aggregates, and the aggregates' gradients with respect to the field.

    f = stress_fields(sigma)                                   # von_mises, sigma1, sigma2, max_shear, angle, criterion
    c = graph_criterion(sigma, batch, "tresca", weights=w)     # c.max, c.mean, c.pnorm, c.ks, c.argmax, c.node
    g = graph_criterion_grad(sigma, batch, "tresca", "pnorm", weights=w)     # (N, 3): d pnorm / d sigma

Conventions (plane stress, as the reference's ``von_mises_stress``, datasets.py:82).  ``sigma`` is (N, 3) in
xx, yy, xy order, unstandardised.  With m = (sx + sy) / 2, d = (sx - sy) / 2, r = sqrt(d^2 + sxy^2), s1 = m + r,
s2 = m - r:

* ``von_mises`` = sqrt(0.5 ((sx - sy)^2 + sx^2 + sy^2 + 6 sxy^2)); its gradient is 0 where it is 0;
* ``tresca`` = max(2 r, |s1|, |s2|), the out-of-plane principal stress being 0.  The branch is chosen in that
  order and the first wins an exact tie (``s2 == 0`` gives the 2 r branch); the gradient is the chosen branch's,
  with d r = 0 where r == 0 and sign(0) = 0;
* ``rankine`` = max(s1, 0); the gradient is d s1 where s1 > 0, else 0.

``weights`` (N,) decides which nodes count: a node takes part in its graph's aggregates if and only if its weight
is > 0, so a weight of 0 (or a negative or NaN one) masks the node, boundary nodes for instance; None is 1
everywhere.  With W the sum of the participating weights and M the maximum: ``mean`` = sum w c / W, ``pnorm`` =
M (sum w (c / M)^p / W)^(1/p), ``ks`` = M + log(sum w exp(rho (c - M)) / W) / rho.  ``max`` is differentiated
as a subgradient: all of it goes to ``argmax``, the first node that attains it.  A graph without a
participating node, or with a NaN criterion at one, gets NaN values and ``argmax`` -1.

``rho`` has the unit of 1 / stress and no default scale is guessed: ``rho=None`` computes ``ks`` with rho = 1
(``GraphCriterion.rho`` says which value was used) and asking for the gradient of ``ks`` with ``rho=None``
raises.

Values are fp64 per graph (fp64 arithmetic on the fp32 field), fields and gradients fp32 rounded once.  CPU
tensors raise, as everywhere on the HIP path.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from pdg.lib import lib, ptr as _p, stream_handle

CRITERIA = ("von_mises", "tresca", "rankine")
AGGREGATES = ("max", "mean", "pnorm", "ks")
FIELDS = ("von_mises", "sigma1", "sigma2", "max_shear", "angle", "criterion")


@dataclass
class GraphCriterion:
    """``max``, ``mean``, ``pnorm``, ``ks`` (B,) fp64; ``argmax`` (B,) int64, the graph-local index of the first
    participating node that attains ``max`` (-1 for a NaN graph); ``node`` (B,) int64, the same as an index into
    the batch's nodes (-1 likewise); ``p`` and ``rho`` the values the aggregates were computed with; ``fields``
    the dict of :func:`stress_fields`, or None."""
    max: torch.Tensor
    mean: torch.Tensor
    pnorm: torch.Tensor
    ks: torch.Tensor
    argmax: torch.Tensor
    node: torch.Tensor
    p: float
    rho: float
    fields: dict | None = None


def _id(name, names, what: str) -> int:
    if name not in names:
        raise ValueError(f"unknown {what} {name!r}: one of {', '.join(names)}")
    return names.index(name)


def _field3(sigma: torch.Tensor) -> torch.Tensor:
    if sigma.device.type != "cuda":
        raise RuntimeError("stress criteria run on the MI355X HIP path only; move the field to a HIP device (the "
                           "CPU restatement is test-only, tests/criteria_ref.py)")
    if sigma.dim() != 2 or sigma.shape[1] != 3:
        raise ValueError(f"a stress field is (N, 3) in xx, yy, xy order, got {tuple(sigma.shape)}")
    return sigma.detach().float().contiguous()


def _ptr_of(batch, n: int, dev) -> torch.Tensor:
    """The node offsets of a ``Batch`` (its ``ptr``), of a single ``Data`` ([0, N]) or a ``ptr`` tensor, int32 on
    the device, checked against the field's N rows on the host (the kernels trust them)."""
    if batch is None:
        host = torch.tensor([0, n], dtype=torch.int64)
    elif isinstance(batch, torch.Tensor):
        host = batch.detach().reshape(-1).to("cpu", torch.int64)
    elif "ptr" in batch:
        host = batch.ptr.detach().reshape(-1).to("cpu", torch.int64)
    else:
        host = torch.tensor([0, int(batch.num_nodes)], dtype=torch.int64)
    if host.numel() < 2 or int(host[0]) != 0 or int(host[-1]) != n or bool((host[1:] < host[:-1]).any()):
        raise ValueError(f"ptr must rise from 0 to the field's {n} rows, got {host.tolist()[:8]}"
                         f"{'...' if host.numel() > 8 else ''}")
    return host.to(dev, torch.int32)


def _weights_of(weights, n: int, dev):
    if weights is None:
        return None
    if weights.device.type != "cuda":
        raise RuntimeError("stress criteria run on the MI355X HIP path only; move the weights to a HIP device")
    if weights.numel() != n:
        raise ValueError(f"{weights.numel()} weights for {n} nodes")
    return weights.detach().reshape(-1).to(device=dev, dtype=torch.float32).contiguous()


def _check_p_rho(p, rho):
    p = float(p)
    if not (p >= 1.0 and p != float("inf")):
        raise ValueError(f"p must be finite and >= 1, got {p}")
    if rho is not None and not (0.0 < float(rho) < float("inf")):
        raise ValueError(f"rho must be finite and > 0, got {rho}")
    return p, (1.0 if rho is None else float(rho))


def _forward(ptr, sigma, weights, cid: int, p: float, rho: float, want_fields: bool):
    dev, n, b = sigma.device, sigma.shape[0], ptr.numel() - 1
    table = torch.empty(b, 4, dtype=torch.float64, device=dev)
    argmax = torch.empty(b, dtype=torch.int32, device=dev)
    fields = torch.empty(n, 6, dtype=torch.float32, device=dev) if want_fields else None
    lib.pdg_stress_criteria(b, ptr.data_ptr(), sigma.data_ptr(), _p(weights), cid, p, rho, table.data_ptr(),
                            argmax.data_ptr(), _p(fields), stream_handle(dev))
    return table, argmax, fields


def _fields_dict(fields: torch.Tensor) -> dict:
    return {k: fields[:, i] for i, k in enumerate(FIELDS)}


def stress_fields(sigma: torch.Tensor, criterion: str = "von_mises") -> dict:
    """The six (N,) fp32 fields of a stress field (N, 3): ``von_mises``, ``sigma1``, ``sigma2`` (the principal
    stresses), ``max_shear`` (r, the in-plane maximum shear), ``angle`` (the principal angle atan2(sxy, d) / 2)
    and ``criterion`` (the chosen one).  Needs no batch."""
    cid = _id(criterion, CRITERIA, "criterion")
    s = _field3(sigma)
    n = s.shape[0]
    if n == 0:
        return _fields_dict(torch.empty(0, 6, dtype=torch.float32, device=s.device))
    return _fields_dict(_forward(_ptr_of(None, n, s.device), s, None, cid, 1.0, 1.0, True)[2])


def graph_criterion(sigma: torch.Tensor, batch, criterion: str = "von_mises", weights=None, p: float = 8.0,
                    rho: float | None = None, fields: bool = False) -> GraphCriterion:
    """The per-graph peak and aggregates of ``criterion`` over ``sigma`` (N, 3).  ``batch``: a ``Batch``, a single
    ``Data`` or a ``ptr`` tensor of node offsets.  ``rho=None``: ``ks`` is computed with rho = 1 and the result's
    ``rho`` is 1.0 (see the module docstring).  ``fields=True`` adds the per-node fields, defined for every node
    of a non-empty graph, participating or not."""
    cid = _id(criterion, CRITERIA, "criterion")
    s = _field3(sigma)
    p, rho = _check_p_rho(p, rho)
    ptr = _ptr_of(batch, s.shape[0], s.device)
    table, argmax, f = _forward(ptr, s, _weights_of(weights, s.shape[0], s.device), cid, p, rho, bool(fields))
    am = argmax.long()
    node = torch.where(am >= 0, am + ptr[:-1].long(), am)
    return GraphCriterion(max=table[:, 0], mean=table[:, 1], pnorm=table[:, 2], ks=table[:, 3], argmax=am, node=node,
                          p=p, rho=rho, fields=_fields_dict(f) if fields else None)


def _grad(ptr, sigma, weights, cid: int, aid: int, p: float, rho: float, g_value):
    """(table, argmax, g_sigma): the two launches on one field."""
    dev, b = sigma.device, ptr.numel() - 1
    if g_value is not None:
        if g_value.device.type != "cuda":
            raise RuntimeError("stress criteria run on the MI355X HIP path only; move g_value to a HIP device")
        if g_value.numel() != b:
            raise ValueError(f"g_value must hold one value per graph ({b}), got {tuple(g_value.shape)}")
        g_value = g_value.detach().reshape(-1).to(device=dev, dtype=torch.float32).contiguous()
    table, argmax, _ = _forward(ptr, sigma, weights, cid, p, rho, False)
    g_sigma = torch.empty_like(sigma)
    lib.pdg_stress_criteria_bwd(b, ptr.data_ptr(), sigma.data_ptr(), _p(weights), cid, aid, p, rho, table.data_ptr(),
                                argmax.data_ptr(), _p(g_value), g_sigma.data_ptr(), stream_handle(dev))
    return table, argmax, g_sigma


def _aggregate_id(aggregate: str, rho) -> int:
    aid = _id(aggregate, AGGREGATES, "aggregate")
    if aid == 3 and rho is None:
        raise ValueError("aggregate='ks' needs rho (the unit of 1 / stress): no default scale is guessed")
    return aid


def graph_criterion_grad(sigma: torch.Tensor, batch, criterion: str = "von_mises", aggregate: str = "pnorm",
                         weights=None, p: float = 8.0, rho: float | None = None, g_value=None) -> torch.Tensor:
    """(N, 3) fp32: ``g_value[g]`` (ones when None) times the gradient of graph g's ``aggregate`` (``max``,
    ``mean``, ``pnorm`` or ``ks``) of ``criterion`` with respect to ``sigma``.  Nodes that take no part get exact
    zero rows; the participating nodes of a NaN graph NaN rows.  ``aggregate='ks'`` needs ``rho``."""
    cid = _id(criterion, CRITERIA, "criterion")
    aid = _aggregate_id(aggregate, rho)
    s = _field3(sigma)
    p, rho = _check_p_rho(p, rho)
    ptr = _ptr_of(batch, s.shape[0], s.device)
    return _grad(ptr, s, _weights_of(weights, s.shape[0], s.device), cid, aid, p, rho, g_value)[2]
