"""Training losses of scripts/gnn_train.py:41-92 on the HIP kernels.

* ``normalized_mse_loss_single`` / ``compute_divergence``: the reference's
  per-graph functions, same signatures and error behaviour;
* ``batch_loss``: the whole per-graph loop of gnn_train.py:168-197 fused into
  two segmented kernels over the batch's ``ptr`` (no Python loop, no dense
  operator), returning (total, nmse, div) with nmse/div already / batch_size.
  All three are differentiable: total = nmse + div, and back-propagating nmse
  and div separately (or their sum) gives the reference's gradients.

All three run through the ``torch.ops.pdivgnn.batch_loss`` custom op (pdg.ops).
"""
from __future__ import annotations

import torch

from pdg import ops  # noqa: F401  (registers torch.ops.pdivgnn.*)
from pdg.plan import GraphPlan, plan_for


def _check_dev(t: torch.Tensor) -> None:
    if t.device.type != "cuda":
        raise RuntimeError("HIP losses need tensors on a HIP device (the CPU restatement is test-only, oracle/)")


def _loss(pred, gt, plan: GraphPlan, types, with_nmse: bool, divergence: bool, penalty: float,
          reduce_abs: bool):
    """(total, nmse / B, penalty * div / B) through the torch.ops.pdivgnn.batch_loss custom op (pdg.ops)."""
    _check_dev(pred)
    if divergence and not plan.has_div:
        raise ValueError("batch has no divergence operator")
    d = plan.has_div and divergence
    total, nmse, div, _den, _divf = torch.ops.pdivgnn.batch_loss(
        pred, gt if with_nmse else None, plan.ptr, types if divergence else None,
        plan.a_rowptr if d else None, plan.a_col if d else None, plan.a_val if d else None,
        plan.at_rowptr if d else None, plan.at_row if d else None, plan.at_comp if d else None,
        plan.at_val if d else None, bool(with_nmse), bool(divergence), float(penalty), bool(reduce_abs))
    return total, nmse, div


class _PhysicsTerms(torch.autograd.Function):
    """(traction, periodic, mean) of a standardised prediction, each weight / B times its sum over the graphs:
    pdg_phys_loss_fwd, and pdg_phys_loss_bwd with the upstream gradients folded into its three weights on the
    device (csrc/pdg_physloss.hip; no host read either way)."""

    @staticmethod
    def forward(ctx, pred, affine, weights, ptr, bvec, blen, labels, rowptr, src, perm, ea, area, cell, target):
        from pdg.lib import lib, ptr as p_, stream_handle
        B, N = ptr.numel() - 1, pred.shape[0]
        y = pred.detach().float().contiguous()
        table = torch.empty(B, 12, dtype=torch.float64, device=y.device)
        loss = torch.empty(B, 3, dtype=torch.float32, device=y.device)
        args = (y, affine, bvec, blen, labels, rowptr, src, perm, ea, area, cell, target)
        lib.pdg_phys_loss_fwd(B, ptr.data_ptr(), *(p_(a) for a in args), table.data_ptr(), loss.data_ptr(),
                              stream_handle(y.device))
        ctx.saved = (args, ptr, table, weights, B, N)
        out = loss.sum(0) * weights
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g_t, g_p, g_m):
        from pdg.lib import lib, ptr as p_, stream_handle
        args, ptr, table, weights, B, N = ctx.saved
        scale = (torch.stack([g_t, g_p, g_m]).float() * weights).contiguous()
        g = torch.empty(N, 3, dtype=torch.float32, device=table.device)
        lib.pdg_phys_loss_bwd(B, ptr.data_ptr(), N, *(p_(a) for a in args), table.data_ptr(), scale.data_ptr(), 0,
                              g.data_ptr(), stream_handle(g.device))
        return (g,) + (None,) * 13


def _physics_terms(pred, batch, plan: GraphPlan, physics, mean_local_stress, std_local_stress):
    _check_dev(pred)
    if mean_local_stress is None or std_local_stress is None:
        raise ValueError("physics penalties need mean_local_stress and std_local_stress (the terms are evaluated on "
                         "pred + mean / std)")
    need = ("boundary_vec", "boundary_len", "node_area") + (("cell_area",) if physics.convention == "cell" else ())
    missing = [k for k in need if batch.__dict__.get(k) is None]
    if missing:
        raise ValueError(f"physics penalties need the batch's {', '.join(missing)}: build the store with "
                         "DeviceGraphStore(..., mesh_fields=True) (pdg.devgraph.attach_mesh_fields sets them)")
    dev, f32 = pred.device, torch.float32
    B = plan.n_graphs
    affine = torch.stack([torch.as_tensor(std_local_stress, dtype=f32, device=dev).reshape(()),
                          torch.as_tensor(mean_local_stress, dtype=f32, device=dev).reshape(())])
    weights = torch.tensor([physics.traction / B, physics.periodic / B, physics.mean / B], dtype=f32, device=dev)
    cell = batch.cell_area.to(dev, torch.float64).reshape(-1).contiguous() if physics.convention == "cell" else None
    target = batch.mean_stress.index_select(0, plan.ptr[:-1].long()).float().contiguous()
    return _PhysicsTerms.apply(
        pred, affine, weights, plan.ptr, batch.boundary_vec.to(dev, f32).contiguous(),
        batch.boundary_len.to(dev, f32).reshape(-1).contiguous(),
        batch.nodes_types.reshape(-1).to(torch.int64).contiguous(), plan.rowptr_dst, plan.src, plan.perm,
        batch.edge_attr.reshape(-1).float().contiguous(), batch.node_area.to(dev, f32).reshape(-1).contiguous(), cell,
        target)


def batch_loss(pred: torch.Tensor, batch, gt_std: torch.Tensor, divergence: bool = False,
               divergence_penalty: float = 1.0, reduce_strategy: str = "square", physics=None,
               mean_local_stress=None, std_local_stress=None):
    """Fused gnn_train.py:168-197: returns (total, nmse/B, lambda*div/B).  With ``physics`` (a
    ``pdg.trainer.PhysicsPenalty``) and the local stress's ``mean_local_stress`` / ``std_local_stress`` it returns
    (total, nmse/B, lambda*div/B, traction, periodic, mean): the boundary and mean-consistency penalties of
    ``pred`` (standardised) on a batch that carries the mesh fields, each mu / B times its sum over the graphs,
    and total includes them.  Without ``physics`` the result is what it always was."""
    if reduce_strategy not in ("abs", "square"):
        raise AttributeError("reduce_strategy must be 'abs' or 'square'")
    plan = plan_for(batch)
    types = batch.surfaces_nodes_for_div if batch.surfaces_nodes_for_div is not None else batch.nodes_types
    base = _loss(pred, gt_std, plan, types, True, bool(divergence), float(divergence_penalty),
                 reduce_strategy == "abs")
    if physics is None:
        return base
    t, p, m = _physics_terms(pred, batch, plan, physics, mean_local_stress, std_local_stress)
    return base[0] + t + p + m, base[1], base[2], t, p, m


def normalized_mse_loss_single(ground_truth_local_stress: torch.Tensor,
                               predicted_local_stress: torch.Tensor) -> torch.Tensor:
    """gnn_train.py:41-57 on one graph."""
    n = predicted_local_stress.shape[0]
    plan = _SinglePlan.get(n, predicted_local_stress.device)
    total, _, _ = _loss(predicted_local_stress, ground_truth_local_stress, plan, None, True, False, 1.0, False)
    return total


class _SinglePlan:
    """Minimal plan for single-graph loss calls (ptr = [0, n], optional operator)."""

    _cache: dict = {}

    @classmethod
    def get(cls, n: int, device, op=None) -> GraphPlan:
        p = GraphPlan.__new__(GraphPlan)
        p.n_nodes, p.n_edges, p.n_graphs = n, 0, 1
        p.ptr = torch.tensor([0, n], dtype=torch.int32, device=device)
        p.has_div = False
        if op is not None:
            op = op.coalesce()
            idx = op.indices().to(device)
            p.has_div = True
            if torch.device(device).type == "cuda":   # the device planner (clamped; the status word is not read)
                p._build_div_device(idx[0], idx[1], op.values())
            else:
                GraphPlan._build_div(p, idx[0], idx[1], op.values().to(device).float())
        return p


def compute_divergence(local_stress_field: torch.Tensor, op_div_matrix: torch.Tensor,
                       surface_nodes_ids: torch.Tensor, reduce_strategy: str = "square") -> torch.Tensor:
    """gnn_train.py:60-92 on one graph: mean over rows of |A[:, :2N] S|^2 (boundary rows
    zeroed), summed over the 2 components.  Sparse CSR instead of ``to_dense``."""
    if reduce_strategy not in ("abs", "square"):
        raise AttributeError("reduce_strategy must be 'abs' or 'square'")
    n = local_stress_field.shape[0]
    plan = _SinglePlan.get(n, local_stress_field.device, op_div_matrix)
    total, _, _ = _loss(local_stress_field, None, plan, surface_nodes_ids, False, True, 1.0,
                        reduce_strategy == "abs")
    return total
