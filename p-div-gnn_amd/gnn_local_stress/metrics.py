"""Evaluation of predictions against the FEM solution on the HIP kernels: the numbers of the
reference's ``scripts/compare_results.py`` (the numeric part of ``main``, lines 1098-1245, and the
helpers at 122-141, 333-364, 647-673, 713-726) without its plotting.

* :func:`batch_metrics`: every per-sample number of the script for a whole batch with three
  launches (``pdg_eval_nmse`` once, ``pdg_eval_div`` on the prediction and on the ground truth)
  over the batch's plan: per-component and mean NMSE, the von Mises NMSE, R2, the divergence scalar
  of the raw and of the standardised field for the model and for FEM and, with ``fields=True``, the
  element-wise NMSE, von Mises and divergence-norm fields;
* ``normalized_mse_loss_single`` / ``normalized_mse_loss_element_wise`` / ``von_mises_stress`` /
  ``compute_divergence_norm_field``: the script's single-graph functions, same names and argument
  orders, on the same two calls;
* :func:`evaluate_inference`: scores the folder ``gnn_local_stress.inference`` writes against the
  ground-truth dataset and writes ``metrics.csv`` and ``summary.json``.

    python -m gnn_local_stress.metrics config_metrics.yml

with the YAML holding :func:`evaluate_inference`'s keywords.

Values are fp64 per graph (fp64 sums of the fp32 inputs), fields fp32 rounded once.  ``r2`` is
``1 - nmse``, which is sklearn's ``r2_score`` with uniform averaging whenever the denominators are
non-zero; sklearn's special case for a constant ground-truth column is not reproduced (the IEEE
quotient is returned, as numpy gives for the NMSE).

Deliberate deviation from the script: its ``main`` passes the prediction and the ground truth in
swapped roles to ``normalized_mse_loss_single`` and ``r2_score`` (lines 1166-1202: the ``zip``
yields ``(gt, pred)`` under the names ``pred, gt``), so its NMSE and R2 are normalised by the
prediction's variance.  Here the ground truth is the ground truth by default;
``evaluate_inference(..., swap_like_reference=True)`` swaps the two pointers of the NMSE call and
reproduces the script's numbers (the divergences are not affected: the script does not swap them).
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import torch

from pdg.lib import lib, ptr, stream_handle
from pdg.plan import GraphPlan, plan_for

NMSE_COLUMNS = ("nmse_xx", "nmse_yy", "nmse_xy", "nmse", "nmse_vm", "r2")
DIV_COLUMNS = ("div", "div_standard", "div_fem", "div_fem_standard")


def _check_dev(t: torch.Tensor) -> None:
    if t.device.type != "cuda":
        raise RuntimeError("HIP metrics need tensors on a HIP device (the CPU restatement is test-only, "
                           "tests/metrics_ref.py)")


def _field3(t: torch.Tensor, n: int | None = None) -> torch.Tensor:
    _check_dev(t)
    if t.dim() != 2 or t.shape[1] != 3 or (n is not None and t.shape[0] != n):
        raise ValueError(f"a stress field is (N, 3) in xx, yy, xy order, got {tuple(t.shape)}")
    return t.detach().float().contiguous()


def _reduce_abs(reduce_strategy: str) -> bool:
    if reduce_strategy not in ("abs", "square"):
        raise AttributeError("reduce_strategy must be 'abs' or 'square'")
    return reduce_strategy == "abs"


def _eval_nmse(plan: GraphPlan, gt: torch.Tensor, pred: torch.Tensor, fields: bool):
    """(table (B, 6), err_field (N, 4), vm_gt (N), vm_pred (N)); the fields None without ``fields``."""
    dev, n = gt.device, gt.shape[0]
    table = torch.empty(plan.n_graphs, 6, dtype=torch.float64, device=dev)
    err = torch.empty(n, 4, dtype=torch.float32, device=dev) if fields else None
    vm_gt = torch.empty(n, dtype=torch.float32, device=dev) if fields else None
    vm_pred = torch.empty(n, dtype=torch.float32, device=dev) if fields else None
    lib.pdg_eval_nmse(plan.n_graphs, plan.ptr.data_ptr(), gt.data_ptr(), pred.data_ptr(), table.data_ptr(),
                      ptr(err), ptr(vm_gt), ptr(vm_pred), stream_handle(dev))
    return table, err, vm_gt, vm_pred


def _eval_div(plan: GraphPlan, types: torch.Tensor, sigma: torch.Tensor, mean: float, std: float,
              reduce_abs: bool, fields: bool):
    """(table (B, 2), norm (N), norm_std (N)); the fields None without ``fields``."""
    dev, n = sigma.device, sigma.shape[0]
    types = types.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    if types.numel() != n:
        raise ValueError(f"{types.numel()} node types for {n} nodes")
    table = torch.empty(plan.n_graphs, 2, dtype=torch.float64, device=dev)
    norm = torch.empty(n, dtype=torch.float32, device=dev) if fields else None
    norm_std = torch.empty(n, dtype=torch.float32, device=dev) if fields else None
    # an operator without entries has empty (NULL) column / value arrays; the kernel reads none of them
    a_col = plan.a_col if plan.a_col.numel() else plan.a_rowptr
    a_val = plan.a_val if plan.a_val.numel() else plan.a_rowptr
    lib.pdg_eval_div(plan.n_graphs, plan.ptr.data_ptr(), plan.a_rowptr.data_ptr(), a_col.data_ptr(),
                     a_val.data_ptr(), types.data_ptr(), sigma.data_ptr(), float(mean), float(std),
                     int(reduce_abs), table.data_ptr(), ptr(norm), ptr(norm_std), stream_handle(dev))
    return table, norm, norm_std


def _score(pred, gt, batch, mean_local_stress, std_local_stress, reduce_strategy, fields, swap_nmse) -> dict:
    rabs = _reduce_abs(reduce_strategy)
    plan = plan_for(batch)
    pred = _field3(pred, plan.n_nodes)
    gt = _field3(gt, plan.n_nodes)
    a, b = (pred, gt) if swap_nmse else (gt, pred)
    table, err, vm_a, vm_b = _eval_nmse(plan, a, b, fields)
    out = {k: table[:, i] for i, k in enumerate(NMSE_COLUMNS)}
    if fields:
        out["nmse_field"] = err
        out["von_mises_gt"], out["von_mises_pred"] = (vm_b, vm_a) if swap_nmse else (vm_a, vm_b)
    if not plan.has_div:
        return out
    types = batch.surfaces_nodes_for_div if batch.surfaces_nodes_for_div is not None else batch.nodes_types
    if types is None:
        raise ValueError("batch has a divergence operator but no node types")
    mean, std = float(mean_local_stress), float(std_local_stress)
    for sigma, tag in ((pred, ""), (gt, "_fem")):
        t, norm, norm_std = _eval_div(plan, types, sigma, mean, std, rabs, fields)
        out["div" + tag], out["div" + tag + "_standard"] = t[:, 0], t[:, 1]
        if fields:
            out["div_norm" + tag], out["div_norm" + tag + "_standard"] = norm, norm_std
    return out


def batch_metrics(pred: torch.Tensor, gt: torch.Tensor, batch, mean_local_stress, std_local_stress,
                  reduce_strategy: str = "square", fields: bool = False) -> dict:
    """Scores of every graph of ``batch``: per-graph fp64 tensors ``nmse_xx``, ``nmse_yy``, ``nmse_xy``,
    ``nmse``, ``nmse_vm``, ``r2`` and, when the batch carries a divergence operator, ``div``,
    ``div_standard`` (the prediction) and ``div_fem``, ``div_fem_standard`` (the ground truth); a batch
    without an operator gives the first six only.  ``pred`` and ``gt`` are (N, 3) unstandardised
    stress fields on the HIP device; ``mean_local_stress`` / ``std_local_stress`` the scalars of
    ``normalize_params.json``.  ``fields=True`` adds the per-node fp32 tensors ``nmse_field`` (N, 4:
    xx, yy, xy, von Mises), ``von_mises_gt``, ``von_mises_pred`` and ``div_norm``,
    ``div_norm_standard``, ``div_norm_fem``, ``div_norm_fem_standard`` (N)."""
    return _score(pred, gt, batch, mean_local_stress, std_local_stress, reduce_strategy, bool(fields), False)


# ------------------------------------------------------------------------------ single-graph functions
def _single(n: int, device, op=None) -> GraphPlan:
    from .losses import _SinglePlan
    return _SinglePlan.get(n, device, op)


def normalized_mse_loss_single(ground_truth_local_stress: torch.Tensor, predicted_local_stress: torch.Tensor,
                               reduce: bool = True) -> torch.Tensor:
    """compare_results.py:333-348 on one (N, 3) graph: the fp64 mean NMSE, or the three
    per-component values with ``reduce=False``."""
    gt, pred = _field3(ground_truth_local_stress), _field3(predicted_local_stress, ground_truth_local_stress.shape[0])
    table = _eval_nmse(_single(gt.shape[0], gt.device), gt, pred, False)[0]
    return table[0, 3] if reduce else table[0, :3]


def normalized_mse_loss_element_wise(ground_truth_local_stress: torch.Tensor,
                                     predicted_local_stress: torch.Tensor, reduce: bool = True) -> torch.Tensor:
    """compare_results.py:351-364 on one (N, 3) graph: (gt - pred)^2 / sum (gt - mean gt)^2, (N, 3)
    fp32 (``reduce`` is unused there too).  ``batch_metrics(fields=True)`` also gives the von Mises
    column the script appends."""
    gt, pred = _field3(ground_truth_local_stress), _field3(predicted_local_stress, ground_truth_local_stress.shape[0])
    return _eval_nmse(_single(gt.shape[0], gt.device), gt, pred, True)[1][:, :3]


def von_mises_stress(mean_stress_x: torch.Tensor, mean_stress_y: torch.Tensor,
                     mean_stress_xy: torch.Tensor) -> torch.Tensor:
    """compare_results.py:713-726 on three (N,) component tensors: (N,) fp32."""
    s = torch.stack([torch.as_tensor(mean_stress_x).reshape(-1), torch.as_tensor(mean_stress_y).reshape(-1),
                     torch.as_tensor(mean_stress_xy).reshape(-1)], 1)
    s = _field3(s)
    return _eval_nmse(_single(s.shape[0], s.device), s, s, True)[2]


def compute_divergence_norm_field(local_stress_field: torch.Tensor, op_div_matrix: torch.Tensor,
                                  surface_nodes_ids: torch.Tensor) -> torch.Tensor:
    """compare_results.py:122-141 on one graph: |div sigma| per node, external-boundary rows zeroed."""
    s = _field3(local_stress_field)
    plan = _single(s.shape[0], s.device, op_div_matrix)
    return _eval_div(plan, surface_nodes_ids, s, 0.0, 1.0, False, True)[1]


# ------------------------------------------------------------------------------ a whole inference folder
def evaluate_inference(ground_truth_csv, inference_folder, device, batch_size: int = 64,
                       reduce_strategy: str = "square", swap_like_reference: bool = False) -> dict:
    """Score the folder ``run_inference`` wrote (``dataset.csv``, ``normalize_params.json``, one
    ``.npz`` per sample whose ``stress_field`` is the prediction) against the ground-truth
    ``dataset.csv``, samples paired by index.  Writes into the folder ``metrics.csv`` (one row per
    sample, the columns of :func:`batch_metrics`) and ``summary.json`` (the means of ``nmse``,
    ``div_standard`` and ``div_fem_standard``, the count of samples with ``div_standard <
    div_fem_standard`` and the indices of the 10 best and 10 worst samples by ``nmse``, as the script's
    ``topk_indices``); returns the summary.  ``swap_like_reference``: see the module docstring."""
    import pandas as pd

    from pdg.collate import DeviceGraphStore
    from pdg.graph import index_loader

    from . import datasets
    _reduce_abs(reduce_strategy)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("HIP metrics need a HIP device")
    folder = Path(inference_folder)
    gt_frame = pd.read_csv(ground_truth_csv)
    pred_frame = pd.read_csv(folder / "dataset.csv")
    if len(gt_frame) != len(pred_frame):
        raise ValueError(f"{len(gt_frame)} ground-truth samples but {len(pred_frame)} predictions")
    with open(folder / "normalize_params.json") as f:
        params = json.load(f)
    mean, std = float(params["mean_local_stress"]), float(params["std_local_stress"])
    # the graphs' edges play no part in the scores: the cheaper non-periodic graph is read
    dataset = datasets.MeshStressFieldDatasetInMemory(gt_frame, periodic_graph=False, device=device)
    preds = []
    for i, name in enumerate(pred_frame["data_filename"]):
        with np.load(name, allow_pickle=False) as f:
            p = torch.from_numpy(np.asarray(f["stress_field"], np.float32))
        if tuple(p.shape) != tuple(dataset.graphs[i].local_stress.shape):
            raise ValueError(f"sample {i}: prediction {tuple(p.shape)} against ground truth "
                             f"{tuple(dataset.graphs[i].local_stress.shape)}")
        preds.append(p)
    store = DeviceGraphStore(dataset.graphs, device)
    columns: dict[str, list] = {}
    for idx in index_loader(len(dataset), int(batch_size), shuffle=False):
        batch = store.batch(idx)
        pred = torch.cat([preds[i] for i in idx]).to(device)
        m = _score(pred, batch.local_stress, batch, mean, std, reduce_strategy, False, bool(swap_like_reference))
        for k, v in m.items():
            columns.setdefault(k, []).append(v.cpu())
    table = pd.DataFrame({k: torch.cat(v).numpy() for k, v in columns.items()})
    table.index.name = "sample"
    table.to_csv(folder / "metrics.csv")
    nmse = table["nmse"].to_numpy()
    order = np.argsort(nmse)
    k = min(10, len(order))
    summary = {"samples": int(len(table)), "reduce_strategy": reduce_strategy,
               "swap_like_reference": bool(swap_like_reference), "mean_nmse": float(nmse.mean()),
               "best_nmse_indices": [int(i) for i in order[:k]],
               "worst_nmse_indices": [int(i) for i in order[-k:][::-1]]}
    if "div_standard" in table:
        summary["mean_div_standard"] = float(table["div_standard"].mean())
        summary["mean_div_fem_standard"] = float(table["div_fem_standard"].mean())
        summary["div_standard_below_fem"] = int((table["div_standard"] < table["div_fem_standard"]).sum())
    with open(folder / "summary.json", "w") as f:
        json.dump(summary, f, indent=1)
    return summary


def main(config_path: str) -> None:
    import yaml
    with open(config_path) as f:
        params = yaml.safe_load(f)
    print(json.dumps(evaluate_inference(**params)))


if __name__ == "__main__":
    import sys
    main(sys.argv[1])
