"""Numpy-only fp64 restatement of pdg_graph_wmean / pdg_mean_correct (csrc/pdg_homog.hip) and of the Python layer
built on them (gnn_local_stress/homogenise.py): what the GPU tests compare against, with the magnitudes their
bounds need.  The sums are math.fsum's, exact to one rounding, so a difference from the device is the device's."""
import math

import numpy as np

CONVENTIONS = ("cell", "material")


def graph_wmean(ptr, rows, weights=None):
    """(table (B, C + 1) fp64 = W then S_c, mag (B, C + 1) fp64 = sum |w| then sum |w x_c|) over the rows whose
    weight is > 0 (0, negative and NaN weights take no part); zeros for a graph without such a row."""
    ptr = np.asarray(ptr, np.int64)
    x = np.asarray(rows, np.float32).astype(np.float64)
    x = x.reshape(len(x), -1)
    w = np.ones(len(x)) if weights is None else np.asarray(weights, np.float32).astype(np.float64)
    b, c = len(ptr) - 1, x.shape[1]
    table, mag = np.zeros((b, c + 1)), np.zeros((b, c + 1))
    for g in range(b):
        sl = slice(int(ptr[g]), int(ptr[g + 1]))
        wg, xg = w[sl], x[sl]
        with np.errstate(invalid="ignore"):
            keep = wg > 0
        wg, xg = wg[keep], xg[keep]
        table[g, 0] = mag[g, 0] = math.fsum(wg)
        for k in range(c):
            prod = wg * xg[:, k]          # exact: two 24-bit significands
            table[g, 1 + k] = math.fsum(prod)
            mag[g, 1 + k] = math.fsum(np.abs(prod))
    return table, mag


def shifts(table, target, denom=None):
    """(B, 3) fp64: (target D - S) / W with D = denom or W; NaN where W is not > 0."""
    table = np.asarray(table, np.float64)
    W = table[:, 0]
    D = W if denom is None else np.asarray(denom, np.float64).reshape(-1)
    t = np.asarray(target, np.float32).astype(np.float64).reshape(-1, 3)
    out = np.full((len(W), 3), np.nan)
    ok = W > 0
    out[ok] = (t[ok] * D[ok, None] - table[ok, 1:4]) / W[ok, None]
    return out


def mean_correct(ptr, sigma, table, target, denom=None):
    """(out (N, 3) fp64 = sigma + shift_g, unrounded; shift (B, 3) fp64).  Every row of a graph is shifted."""
    ptr = np.asarray(ptr, np.int64)
    s = np.asarray(sigma, np.float32).astype(np.float64)
    sh = shifts(table, target, denom)
    out = s + np.repeat(sh, np.diff(ptr), axis=0)
    return out, sh


def graph_average(ptr, field, weights=None, cell_area=None):
    """dict of total_weight, integral, mean_material, mean_cell, fraction (the last two None without a cell area)."""
    table, _ = graph_wmean(ptr, field, weights)
    W, S = table[:, 0], table[:, 1:]
    with np.errstate(invalid="ignore", divide="ignore"):
        out = {"total_weight": W, "integral": S, "mean_material": S / W[:, None], "mean_cell": None, "fraction": None}
        if cell_area is not None:
            D = np.asarray(cell_area, np.float64).reshape(-1)
            out["mean_cell"], out["fraction"] = S / D[:, None], W / D
    return out


def enforce_mean(ptr, sigma, target, convention="cell", weights=None, cell_area=None):
    """(N, 3) fp64, unrounded: sigma plus the shift that makes its average in `convention` equal `target`."""
    if convention not in CONVENTIONS:
        raise ValueError(convention)
    if convention == "cell" and cell_area is None:
        raise ValueError("cell convention without a cell area")
    table, _ = graph_wmean(ptr, sigma, weights)
    return mean_correct(ptr, sigma, table, target, cell_area if convention == "cell" else None)[0]


def face_areas(pos, faces):
    """fp64 area of every triangle from the float32 coordinates (the shoelace formula, written independently of
    pdg.meshgen's det expression)."""
    p = np.asarray(pos, np.float32).astype(np.float64)[:, :2]
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    return 0.5 * np.abs(a[:, 0] * (b[:, 1] - c[:, 1]) + b[:, 0] * (c[:, 1] - a[:, 1]) + c[:, 0] * (a[:, 1] - b[:, 1]))
