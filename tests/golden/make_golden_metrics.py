"""Generate tests/golden/eval_metrics.npz from the REFERENCE's evaluation functions
(``scripts/compare_results.py``: ``normalized_mse_loss_single``, ``normalized_mse_loss_element_wise``,
``von_mises_stress``, ``compute_divergence``, ``compute_divergence_norm_field``; sklearn's
``r2_score`` as its ``main`` calls it; ``gnn_local_stress/data_utils.py``: ``standardize``).

Run in the build container only (needs the reference tree, scipy, scikit-learn and pandas; never
shipped):

    python tests/golden/make_golden_metrics.py

The script imports fedoo, fitz, pyvista, fire and matplotlib at module level for its plotting;
make_golden.py's stand-ins are registered and extended with what that import touches (``fitz``,
``pyvista.global_theme.font``, and ``matplotlib.pyplot`` where it is not installed).  None of them
is reached by the functions recorded here, which run unchanged.

Three small cases from pdg.meshgen.hole_plate (one with an internal boundary), each with the P1
operator of ``meshgen.p1_divergence_operator``, the labels of ``meshgen.node_labels``, a seeded
ground truth and ``pred = gt + noise``.  Every input is generated as fp32 (the standardisation
constants too) and widened to fp64 for the reference, so the fixture's inputs are exactly what the
kernels see.  The roles are the true ones (ground truth as ground truth): the swapped call of the
script's ``main`` is the same function with the arguments exchanged.

Per case ``<name>_`` + : the inputs ``gt``, ``pred`` (N, 3) f32, ``op_rows``, ``op_cols`` i32, ``op_vals``
f32, ``labels`` i8, ``mean``, ``std`` f32; and in fp64 ``nmse_c`` / ``nmse`` (reduce=False / True),
``nmse_c_std`` / ``nmse_std`` (on the standardised fields), ``r2`` / ``r2_std``, ``vm_gt`` / ``vm_pred``,
``nmse_vm``, ``err_field`` (N, 4: element-wise NMSE of [stress, von Mises]), ``div`` / ``div_fem`` (2, 2:
[strategy square, abs] x [raw, standardised]) and ``norm`` / ``norm_fem`` (2, N: raw, standardised).
"""
from __future__ import annotations

import importlib
import os
import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_golden as mg  # noqa: E402  (stand-ins and paths)

CASES = (("plate8", 8, 0.0, 11), ("hole12", 12, 0.25, 12), ("plate17", 17, 0.0, 13))


def install():
    mg.install_stubs()
    pv = sys.modules["pyvista"]
    pv.global_theme = types.SimpleNamespace(font=types.SimpleNamespace())
    mg._module("fitz")
    try:
        import matplotlib.pyplot  # noqa: F401
    except ImportError:
        mg._module("matplotlib").pyplot = mg._module("matplotlib.pyplot")


def inputs(n: int, hole: float, seed: int):
    from pdg import meshgen
    s = meshgen.hole_plate(n, hole_radius=hole, seed=seed)
    rows, cols, vals = meshgen.p1_divergence_operator(s.pos, s.faces)
    labels = meshgen.node_labels(s.pos, s.faces)[0]
    rng = np.random.default_rng(seed)
    N = s.num_nodes
    gt = (rng.normal(size=(N, 3)) * np.array([40.0, 25.0, 10.0]) + np.array([60.0, -35.0, 8.0])).astype(np.float32)
    pred = (gt + rng.normal(size=(N, 3)) * np.array([6.0, 4.0, 3.0])).astype(np.float32)
    mean = np.float32(gt.mean())
    std = np.float32(gt.std())
    return gt, pred, rows, cols, vals.astype(np.float32), labels, mean, std


def main():
    install()
    os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(mg.REF / "scripts"))
    sys.path.insert(0, str(mg.REF))
    import scipy.sparse
    from sklearn.metrics import r2_score
    cr = importlib.import_module("compare_results")          # reference script
    from gnn_local_stress import data_utils                   # reference module
    assert Path(cr.__file__).is_relative_to(mg.REF) and Path(data_utils.__file__).is_relative_to(mg.REF)
    rec = {}
    for name, n, hole, seed in CASES:
        gt32, pred32, rows, cols, vals, labels, mean, std = inputs(n, hole, seed)
        N = len(gt32)
        gt, pred = gt32.astype(np.float64), pred32.astype(np.float64)
        op = scipy.sparse.coo_matrix((vals.astype(np.float64), (rows, cols)), shape=(N, 2 * N)).tocsr()
        gt_s = data_utils.standardize(gt, float(mean), float(std))
        pred_s = data_utils.standardize(pred, float(mean), float(std))
        vm_gt, vm_pred = cr.von_mises_stress(*gt.T), cr.von_mises_stress(*pred.T)
        out = {
            "gt": gt32, "pred": pred32, "op_rows": rows.astype(np.int32), "op_cols": cols.astype(np.int32),
            "op_vals": vals, "labels": labels.astype(np.int8), "mean": mean, "std": std,
            "nmse_c": cr.normalized_mse_loss_single(gt, pred, reduce=False),
            "nmse": cr.normalized_mse_loss_single(gt, pred, reduce=True),
            "nmse_c_std": cr.normalized_mse_loss_single(gt_s, pred_s, reduce=False),
            "nmse_std": cr.normalized_mse_loss_single(gt_s, pred_s, reduce=True),
            "r2": r2_score(y_true=gt, y_pred=pred), "r2_std": r2_score(y_true=gt_s, y_pred=pred_s),
            "vm_gt": vm_gt, "vm_pred": vm_pred,
            "nmse_vm": cr.normalized_mse_loss_single(vm_gt, vm_pred),
            "err_field": cr.normalized_mse_loss_element_wise(
                ground_truth_local_stress=np.concatenate((gt, vm_gt[:, None]), 1),
                predicted_local_stress=np.concatenate((pred, vm_pred[:, None]), 1)),
        }
        for tag, raw, sd in (("", pred, pred_s), ("_fem", gt, gt_s)):
            out["div" + tag] = np.array([[cr.compute_divergence(f, op, labels, strategy) for f in (raw, sd)]
                                         for strategy in ("square", "abs")])
            out["norm" + tag] = np.stack([cr.compute_divergence_norm_field(f, op, labels) for f in (raw, sd)])
        for k, v in out.items():
            rec[f"{name}_{k}"] = np.asarray(v)
        print(name, N, "internal-boundary nodes", int((labels == -1).sum()), "nmse", out["nmse"], "div", out["div"][0])
    np.savez_compressed(HERE / "eval_metrics.npz", **rec)
    print((HERE / "eval_metrics.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
