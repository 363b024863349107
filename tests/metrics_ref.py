"""fp64 numpy restatement of the evaluation metrics (include/pdivgnn.h: pdg_eval_nmse, pdg_eval_div),
numpy only: the yardstick of tests/test_gpu_metrics.py for arbitrary shapes.  tests/test_metrics_ref.py
pins it against the reference's own functions through tests/golden/eval_metrics.npz.

Inputs are widened to fp64 first; a zero denominator gives numpy's IEEE result (inf or NaN)."""
from __future__ import annotations

import numpy as np


def _f64(a) -> np.ndarray:
    return np.asarray(a, dtype=np.float64)


def von_mises(x, y, xy) -> np.ndarray:
    x, y, xy = _f64(x), _f64(y), _f64(xy)
    return np.sqrt(0.5 * ((x - y) ** 2 + x ** 2 + y ** 2 + 6 * xy ** 2))


def with_von_mises(field) -> np.ndarray:
    """(N, 3) -> (N, 4): the von Mises column appended."""
    f = _f64(field)
    return np.concatenate([f, von_mises(*f.T)[:, None]], 1)


def nmse_element_wise(gt, pred) -> np.ndarray:
    """(gt - pred)^2 / sum (gt - mean gt)^2 per column."""
    gt, pred = _f64(gt), _f64(pred)
    with np.errstate(all="ignore"):
        den = ((gt - gt.mean(axis=0)) ** 2).sum(axis=0)
        return (gt - pred) ** 2 / den


def nmse(gt, pred, reduce: bool = True):
    gt, pred = _f64(gt), _f64(pred)
    with np.errstate(all="ignore"):
        loss = ((gt - pred) ** 2).sum(axis=0) / ((gt - gt.mean(axis=0)) ** 2).sum(axis=0)
        return loss.mean() if reduce else loss


def r2(gt, pred) -> float:
    """r2_score with uniform averaging over the columns (denominators non-zero)."""
    gt, pred = _f64(gt), _f64(pred)
    with np.errstate(all="ignore"):
        return float(np.mean(1.0 - ((gt - pred) ** 2).sum(axis=0) / ((gt - gt.mean(axis=0)) ** 2).sum(axis=0)))


def standardize(field, mean, std) -> np.ndarray:
    return (_f64(field) - float(mean)) / float(std)


def coo_to_csr(n: int, rows, cols, vals):
    """(rowptr, cols, vals) of a COO operator, entries of a row in their given order."""
    rows = np.asarray(rows, np.int64)
    order = np.argsort(rows, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return rowptr, np.asarray(cols, np.int64)[order], np.asarray(vals)[order]


def div_sigma(field, rowptr, cols, vals) -> np.ndarray:
    """A[:, :2n] @ [[sxx; sxy], [sxy; syy]]: (n, 2).  CSR rows of one graph, graph-local columns;
    entries at or beyond column 2n are ignored; a row's entries are added in their order."""
    f = _f64(field)
    n = len(f)
    rowptr, cols, vals = np.asarray(rowptr, np.int64), np.asarray(cols, np.int64), _f64(vals)
    x = np.stack([np.concatenate([f[:, 0], f[:, 2]]), np.concatenate([f[:, 2], f[:, 1]])], 1)   # (2n, 2)
    row = np.repeat(np.arange(n), np.diff(rowptr))
    keep = cols < 2 * n
    out = np.zeros((n, 2))
    np.add.at(out, row[keep], vals[keep, None] * x[cols[keep]])
    return out


def divergence(div, labels, reduce_strategy: str = "square") -> float:
    """The divergence scalar: rows labelled +-1 zeroed, |.| or square, mean over the rows, summed over x, y."""
    if reduce_strategy not in ("abs", "square"):
        raise AttributeError("reduce_strategy must be 'abs' or 'square'")
    labels = np.asarray(labels).reshape(-1)
    d = np.array(div, dtype=np.float64)
    d[(labels == 1) | (labels == -1)] = 0
    d = np.abs(d) if reduce_strategy == "abs" else d ** 2
    with np.errstate(all="ignore"):
        return float(np.sum(np.mean(d, axis=0))) if len(d) else float("nan")


def divergence_norm(div, labels) -> np.ndarray:
    """sqrt(dx^2 + dy^2) per row, only the rows labelled +1 zeroed."""
    d = np.array(div, dtype=np.float64)
    d[np.asarray(labels).reshape(-1) == 1] = 0
    return np.sqrt((d ** 2).sum(axis=1))


def graph_metrics(gt, pred, csr=None, labels=None, mean=0.0, std=1.0, reduce_strategy: str = "square") -> dict:
    """Everything the two kernels give for one graph: ``nmse_table`` (6), ``err_field`` (n, 4), ``vm_gt``,
    ``vm_pred`` and, with ``csr`` = (rowptr, cols, vals) and ``labels``, ``div_table`` / ``div_table_fem``
    (2: raw, standardised) and ``norm``, ``norm_std``, ``norm_fem``, ``norm_fem_std`` (n).  An empty
    graph has NaN tables and empty fields."""
    gt, pred = _f64(gt).reshape(-1, 3), _f64(pred).reshape(-1, 3)
    n = len(gt)
    out = {}
    if n == 0:
        out["nmse_table"] = np.full(6, np.nan)
        out["err_field"], out["vm_gt"], out["vm_pred"] = np.zeros((0, 4)), np.zeros(0), np.zeros(0)
    else:
        g4, p4 = with_von_mises(gt), with_von_mises(pred)
        c = nmse(g4, p4, reduce=False)
        with np.errstate(all="ignore"):
            m = (c[0] + c[1] + c[2]) / 3.0
            out["nmse_table"] = np.array([c[0], c[1], c[2], m, c[3], 1.0 - m])
        out["err_field"], out["vm_gt"], out["vm_pred"] = nmse_element_wise(g4, p4), g4[:, 3], p4[:, 3]
    if csr is None:
        return out
    for tag, f in (("", pred), ("_fem", gt)):
        if n == 0:
            out["div_table" + tag] = np.full(2, np.nan)
            out["norm" + tag] = out["norm" + tag + "_std"] = np.zeros(0)
            continue
        d, ds = div_sigma(f, *csr), div_sigma(standardize(f, mean, std), *csr)
        out["div_table" + tag] = np.array([divergence(d, labels, reduce_strategy),
                                           divergence(ds, labels, reduce_strategy)])
        out["norm" + tag], out["norm" + tag + "_std"] = divergence_norm(d, labels), divergence_norm(ds, labels)
    return out
