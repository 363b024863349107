"""fp64 restatement of pdg_boundary_residuals and pdg_boundary_residuals_bwd (csrc/pdg_boundary.hip) in numpy: the
same fp64 terms, formed from the inputs as given (fp32 arrays are widened first; fp64 arrays serve the finite
differences), every sum taken with math.fsum (exact to one rounding), as homog_ref.py does.

Edges are given as the batch holds them: ``edge_index`` (2, E) and ``edge_attr`` (E,) in any order; a periodic
connection is an edge into n whose ``edge_attr`` is exactly 0 and whose source lies in n's graph.
"""
import math

import numpy as np

COLS = ("L_int", "L_ext", "T2", "F_int_x", "F_int_y", "F_ext_x", "F_ext_y", "P2", "n_pairs")


def forces(sigma, bvec):
    """(fx, fy, ax, ay): f = sigma . m and the same expressions on the absolute values (the terms' magnitudes)."""
    s, m = np.asarray(sigma, np.float64), np.asarray(bvec, np.float64)
    fx = s[:, 0] * m[:, 0] + s[:, 2] * m[:, 1]
    fy = s[:, 2] * m[:, 0] + s[:, 1] * m[:, 1]
    a, b = np.abs(s), np.abs(m)
    return fx, fy, a[:, 0] * b[:, 0] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 1] * b[:, 1]


def takes_part(labels, blen):
    labels = np.asarray(labels).reshape(-1)
    with np.errstate(invalid="ignore"):
        return ((labels == 1) | (labels == -1)) & (np.asarray(blen) > 0)


def periodic_edges(ptr, edges, n):
    """(dst, src) of the periodic connections that are read."""
    if edges is None:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    ei, ea = np.asarray(edges[0], np.int64), np.asarray(edges[1]).reshape(-1)
    src, dst = ei[0], ei[1]
    graph = np.searchsorted(np.asarray(ptr), np.arange(n), side="right") - 1
    keep = (ea == 0) & (graph[src] == graph[dst])
    return dst[keep], src[keep]


def residuals(ptr, sigma, bvec, blen, labels, edges=None):
    """(table (B, 9) fp64, argmax (B,) int64, mag (B, 9): the sum of the absolute values of each column's terms,
    the forces' taken on absolute values)."""
    ptr = np.asarray(ptr, np.int64)
    s = np.asarray(sigma, np.float64)
    n, B = len(s), len(ptr) - 1
    bl = np.asarray(blen, np.float64)
    labels = np.asarray(labels).reshape(-1)
    part = takes_part(labels, blen)
    fx, fy, ax, ay = forces(s, bvec)
    with np.errstate(invalid="ignore", divide="ignore"):
        f2 = fx * fx + fy * fy
        t2 = f2 / bl
        q = np.sqrt(f2) / bl
        a2 = (ax * ax + ay * ay) / bl
    dst, src = periodic_edges(ptr, edges, n)
    d = s[dst] - s[src]
    jump = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    table, mag = np.zeros((B, 9)), np.zeros((B, 9))
    argmax = np.full(B, -1, np.int64)

    def fsum(x):
        x = np.asarray(x, np.float64)
        return math.fsum(x) if np.isfinite(x).all() else float(np.sum(x))

    for g in range(B):
        n0, n1 = int(ptr[g]), int(ptr[g + 1])
        idx = np.arange(n0, n1)
        hole = idx[part[idx] & (labels[idx] == -1)]
        ext = idx[part[idx] & (labels[idx] == 1)]
        e = (dst >= n0) & (dst < n1)
        cols = [bl[hole], bl[ext], t2[hole], fx[hole], fy[hole], fx[ext], fy[ext], 0.5 * jump[e]]
        mags = [bl[hole], bl[ext], a2[hole], ax[hole], ay[hole], ax[ext], ay[ext], 0.5 * jump[e]]
        for c, (terms, m) in enumerate(zip(cols, mags)):
            table[g, c] = fsum(terms)
            mag[g, c] = fsum(np.abs(m)) if np.isfinite(m).all() else np.inf
        table[g, 8] = mag[g, 8] = 0.5 * int(e.sum())
        both = np.concatenate([hole, ext])
        if len(hole) and not np.isnan(f2[both]).any():
            argmax[g] = int(hole[np.argmax(q[hole])] - n0)    # np.argmax: the first of equal values
    return table, argmax, mag


def residuals_grad(ptr, sigma, bvec, blen, labels, edges, table, g_traction=None, g_periodic=None):
    """(grad (N, 3) fp64, mag (N, 3): the sum of the absolute values of each element's terms) of
    sum_g g_traction[g] T2_g / L_int,g + g_periodic[g] P2_g / n_pairs,g, with the kernel's rules: a zero weight
    switches its term off, a denominator that is not > 0 under a non-zero weight gives NaN where a row takes part,
    rows that take no part get zeros."""
    ptr = np.asarray(ptr, np.int64)
    s = np.asarray(sigma, np.float64)
    m = np.asarray(bvec, np.float64)
    bl = np.asarray(blen, np.float64)
    n, B = len(s), len(ptr) - 1
    labels = np.asarray(labels).reshape(-1)
    part = takes_part(labels, blen) & (labels == -1)
    gt = np.zeros(B) if g_traction is None else np.asarray(g_traction, np.float64)
    gp = np.zeros(B) if g_periodic is None else np.asarray(g_periodic, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ct = np.where(gt == 0, 0.0, np.where(table[:, 0] > 0, gt / table[:, 0], np.nan))
        cp = np.where(gp == 0, 0.0, np.where(table[:, 8] > 0, gp / table[:, 8], np.nan))
    graph = np.searchsorted(ptr, np.arange(n), side="right") - 1
    fx, fy, ax, ay = forces(s, m)
    grad, mag = np.zeros((n, 3)), np.zeros((n, 3))
    dst, src = periodic_edges(ptr, edges, n)
    incoming = [[] for _ in range(n)]
    for a, b in zip(dst.tolist(), src.tolist()):
        incoming[a].append(b)
    am = np.abs(m)
    for i in range(n):
        g = graph[i]
        terms = [[], [], []]
        if ct[g] != 0 and part[i]:
            c = 2.0 / bl[i]
            terms[0].append((ct[g] * (c * (fx[i] * m[i, 0])), abs(ct[g]) * c * ax[i] * am[i, 0]))
            terms[1].append((ct[g] * (c * (fy[i] * m[i, 1])), abs(ct[g]) * c * ay[i] * am[i, 1]))
            terms[2].append((ct[g] * (c * (fx[i] * m[i, 1] + fy[i] * m[i, 0])),
                             abs(ct[g]) * c * (ax[i] * am[i, 1] + ay[i] * am[i, 0])))
        if cp[g] != 0:
            for j in incoming[i]:
                for k in range(3):
                    terms[k].append((cp[g] * (2.0 * (s[i, k] - s[j, k])), abs(cp[g]) * 2.0 * (abs(s[i, k]) + abs(s[j, k]))))
        for k in range(3):
            vals = [t[0] for t in terms[k]]
            grad[i, k] = math.fsum(vals) if np.isfinite(vals).all() else float(np.sum(vals))
            mag[i, k] = float(np.sum([t[1] for t in terms[k]])) if terms[k] else 0.0
    return grad, mag


def objective(ptr, sigma, bvec, blen, labels, edges, g_traction=None, g_periodic=None):
    """sum_g g_traction[g] T2_g / L_int,g + g_periodic[g] P2_g / n_pairs,g over the terms whose weight is not 0."""
    table, _, _ = residuals(ptr, sigma, bvec, blen, labels, edges)
    B = len(table)
    gt = np.zeros(B) if g_traction is None else np.asarray(g_traction, np.float64)
    gp = np.zeros(B) if g_periodic is None else np.asarray(g_periodic, np.float64)
    total = 0.0
    for g in range(B):
        if gt[g] != 0:
            total += gt[g] * table[g, 2] / table[g, 0]
        if gp[g] != 0:
            total += gp[g] * table[g, 7] / table[g, 8]
    return total
