"""Host restatement of the sampling operator (csrc/pdg_sample.hip), imported by the tests only.

Triangles: barycentric coordinates with ``fractions.Fraction`` from the fp32 inputs, so they are exact.  Quads: the
inverse of the bilinear map by Newton from the centre in ``numpy.longdouble`` (or another dtype, for the
discrepancy the quad bound quotes), iterated until the iterate is stationary (it moves by no more than 8 ulp).
Location is brute force over all cells (a vectorised bounding-box pass with a margin of 1e-9 of the cell's extents, far above the 3 * 2^-40 that
containment allows, only spares the exact arithmetic on cells that cannot contain the point) with the kernel's
containment rule and tie-break and the same fp64 wrap formula.  sample, sample_T and the CSR are plain loops, sums
by ``math.fsum``."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

TOL = 2.0 ** -40
U = 2.0 ** -53
NEWTON_MAX = 100


def bbox_of(points) -> np.ndarray:
    """(min x, min y, max x, max y) as fp32, the kernel's bounding box."""
    p = np.asarray(points, np.float32)
    return np.array([p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max()], np.float32)


def wrap(xy, bbox) -> np.ndarray:
    """x - floor((x - xmin) / Lx) Lx and the same for y, in fp64 from the fp32 inputs, one rounding per operation."""
    return wrap64(np.asarray(xy, np.float32)[:, :2].astype(np.float64), bbox)


def wrap64(q, bbox) -> np.ndarray:
    """``wrap`` of fp64 points."""
    q = np.asarray(q, np.float64)
    b = np.asarray(bbox, np.float32).astype(np.float64)
    lx, ly = b[2] - b[0], b[3] - b[1]
    out = np.empty_like(q)
    out[:, 0] = q[:, 0] - np.floor((q[:, 0] - b[0]) / lx) * lx
    out[:, 1] = q[:, 1] - np.floor((q[:, 1] - b[1]) / ly) * ly
    return out


def _fr(v) -> Fraction:
    return Fraction(float(v))


def det_exact(pts) -> Fraction:
    """2 x the signed area, exactly: pdg_meshfields' det of a triangle, the diagonals' cross product of a quad."""
    p = [(_fr(x), _fr(y)) for x, y in pts]
    if len(p) == 4:
        (xa, ya), (xb, yb), (xc, yc), (xd, yd) = p
        return (xc - xa) * (yd - yb) - (xd - xb) * (yc - ya)
    (xa, ya), (xb, yb), (xc, yc) = p
    return (xb - xa) * (yc - ya) - (xc - xa) * (yb - ya)


def tri_weights(p, pts) -> list[Fraction] | None:
    """Exact barycentric coordinates of ``p`` in the triangle ``pts`` (3, 2), signed sub-area over signed area;
    None for a triangle of zero area."""
    det = det_exact(pts)
    if det == 0:
        return None
    px, py = _fr(p[0]), _fr(p[1])
    v = [(_fr(x), _fr(y)) for x, y in pts]
    w = []
    for k in range(3):
        (x1, y1), (x2, y2) = v[(k + 1) % 3], v[(k + 2) % 3]
        w.append(((x1 - px) * (y2 - py) - (x2 - px) * (y1 - py)) / det)
    return w


def quad_st(p, pts, dtype=np.longdouble):
    """(s, t) with a + (b - a) s + (d - a) t + (a - b + c - d) s t = p by Newton from the centre in ``dtype``,
    until the iterate is stationary; None when the Jacobian is singular on the way or nothing is stationary after
    NEWTON_MAX steps (a point far outside a distorted quad)."""
    T = dtype
    (xa, ya), (xb, yb), (xc, yc), (xd, yd) = ((T(float(x)), T(float(y))) for x, y in pts)
    ex, ey, fx, fy = xb - xa, yb - ya, xd - xa, yd - ya
    gx, gy = (xa - xb) + (xc - xd), (ya - yb) + (yc - yd)
    hx, hy = T(float(p[0])) - xa, T(float(p[1])) - ya
    s = t = T(0.5)
    tiny = 8 * np.finfo(T).eps
    for _ in range(NEWTON_MAX):
        rx = ex * s + fx * t + gx * s * t - hx
        ry = ey * s + fy * t + gy * s * t - hy
        j11, j12, j21, j22 = ex + gx * t, fx + gx * s, ey + gy * t, fy + gy * s
        dj = j11 * j22 - j12 * j21
        if dj == 0 or not np.isfinite(dj):
            return None
        s2 = s - (j22 * rx - j12 * ry) / dj
        t2 = t - (j11 * ry - j21 * rx) / dj
        # stationary: the iterate repeats, or only wanders among neighbouring numbers (the residual's own rounding)
        if abs(s2 - s) <= tiny * max(1, abs(s)) and abs(t2 - t) <= tiny * max(1, abs(t)):
            return s2, t2
        s, t = s2, t2
    return None


def quad_weights(p, pts, dtype=np.longdouble):
    """The bilinear weights ((1-s)(1-t), s(1-t), st, (1-s)t) of ``p`` in the quad ``pts`` (4, 2) as ``dtype``; None
    for a quad of zero area (det == 0, exactly) and where ``quad_st`` gives nothing."""
    if det_exact(pts) == 0:
        return None
    st = quad_st(p, pts, dtype)
    if st is None:
        return None
    s, t = st
    one = dtype(1)
    return [(one - s) * (one - t), s * (one - t), s * t, (one - s) * t]


def cell_weights(p, pts, dtype=np.longdouble):
    return tri_weights(p, pts) if len(pts) == 3 else quad_weights(p, pts, dtype)


def locate(points, faces, xy, periodic=False, dtype=np.longdouble):
    """(cell (Q,) int64 with -1 for no cell, weights: Q lists of nv numbers (Fraction / dtype; zeros for -1), not
    clamped).  A cell contains the point iff every weight >= -TOL; the largest smallest weight wins, the lowest cell
    id among equals."""
    pts = np.asarray(points, np.float32)[:, :2].astype(np.float64)
    faces = np.asarray(faces, np.int64)
    nv = faces.shape[1]
    bb = bbox_of(points)
    q = np.asarray(xy, np.float32)[:, :2].astype(np.float64)
    if periodic:
        q = wrap(xy, bb)
    valid = ((faces >= 0) & (faces < len(pts))).all(1)
    cx, cy = pts[np.where(valid[:, None], faces, 0), 0], pts[np.where(valid[:, None], faces, 0), 1]
    mnx, mxx, mny, mxy = cx.min(1), cx.max(1), cy.min(1), cy.max(1)
    ex, ey = 1e-9 * (mxx - mnx), 1e-9 * (mxy - mny)
    cell = -np.ones(len(q), np.int64)
    weights = []
    b64 = bb.astype(np.float64)
    for i, (x, y) in enumerate(q):
        best, bmin, bw = -1, None, [0] * nv
        inbox = np.isfinite(x) and np.isfinite(y) and (periodic or (b64[0] <= x <= b64[2] and b64[1] <= y <= b64[3]))
        if inbox:
            cand = np.nonzero(valid & (mnx - ex <= x) & (x <= mxx + ex) & (mny - ey <= y) & (y <= mxy + ey))[0]
            for f in cand:
                w = cell_weights((x, y), pts[faces[f]], dtype)
                if w is None or not all(wk >= -TOL for wk in w):
                    continue
                mn = min(w)
                if best < 0 or mn > bmin:       # candidates ascend, so an equal smallest weight keeps the lower id
                    best, bmin, bw = int(f), mn, w
        cell[i] = best
        weights.append(bw)
    return cell, weights


def clamp32(weights) -> np.ndarray:
    """What the kernel stores: negative weights set to 0, rounded to fp32 once."""
    return np.array([[np.float32(float(max(wk, 0))) for wk in w] for w in weights], np.float32)


def sample(field, faces, cell, weights, fill=float("nan"), node_offset=0) -> np.ndarray:
    """out[q, c] = fsum_k float(w[q, k]) * field[node_offset + faces[cell[q], k], c] as fp64 (not rounded to fp32);
    ``fill`` for cell -1."""
    f = np.asarray(field, np.float64)
    f = f.reshape(len(f), -1)
    out = np.full((len(cell), f.shape[1]), float(fill), np.float64)
    for q, c in enumerate(cell):
        if c >= 0:
            for j in range(f.shape[1]):
                out[q, j] = math.fsum(float(w) * f[node_offset + v, j] for w, v in zip(weights[q], faces[c]))
    return out


def sample_abs(field, faces, cell, weights, node_offset=0) -> np.ndarray:
    """sum_k |w f|, the scale of ``sample``'s rounding bound (0 for cell -1)."""
    f = np.abs(np.asarray(field, np.float64))
    f = f.reshape(len(f), -1)
    out = np.zeros((len(cell), f.shape[1]))
    for q, c in enumerate(cell):
        if c >= 0:
            for j in range(f.shape[1]):
                out[q, j] = math.fsum(abs(float(w)) * f[node_offset + v, j] for w, v in zip(weights[q], faces[c]))
    return out


def csr(faces, cell, n_nodes):
    """(rowptr (n_nodes + 1,), entries) of the node-major CSR of S: row n holds, ascending, the q nv + k with
    faces[cell[q], k] == n."""
    nv = np.asarray(faces).shape[1]
    rows = [[] for _ in range(n_nodes)]
    for q, c in enumerate(cell):
        if c >= 0:
            for k in range(nv):
                rows[int(faces[c][k])].append(q * nv + k)
    rowptr = np.zeros(n_nodes + 1, np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    return rowptr, np.array([e for r in rows for e in r], np.int64)


def sample_T(gout, faces, cell, weights, n_nodes):
    """(S^T gout (n_nodes, C) fp64 by fsum, sum |w g| (n_nodes, C), the entries per node (n_nodes,))."""
    g = np.asarray(gout, np.float64)
    g = g.reshape(len(g), -1)
    nv = np.asarray(faces).shape[1]
    rowptr, entries = csr(faces, cell, n_nodes)
    out, mag = np.zeros((n_nodes, g.shape[1])), np.zeros((n_nodes, g.shape[1]))
    for n in range(n_nodes):
        ent = entries[rowptr[n]:rowptr[n + 1]]
        for j in range(g.shape[1]):
            terms = [float(weights[e // nv][e % nv]) * g[e // nv, j] for e in ent]
            out[n, j] = math.fsum(terms)
            mag[n, j] = math.fsum(abs(t) for t in terms)
    return out, mag, np.diff(rowptr)
