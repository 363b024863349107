"""Numpy-only fp64 restatement of pdg_stress_criteria / pdg_stress_criteria_bwd (csrc/pdg_criteria.hip): the
failure criteria of a plane-stress field, their per-graph aggregates and the aggregates' gradients, with the
kernels' tie and participation rules.  Test-only; pinned by tests/test_criteria_ref.py.

Per node, columns xx, yy, xy: m = (sx + sy) / 2, d = (sx - sy) / 2, r = sqrt(d^2 + sxy^2), s1 = m + r,
s2 = m - r.  Criteria 0 von Mises, 1 Tresca = max(2 r, |s1|, |s2|) (branch in that order, the first wins an exact
tie), 2 Rankine = max(s1, 0).  Aggregates 0 max, 1 mean, 2 pnorm, 3 ks.  A node takes part iff its weight > 0."""
import numpy as np

CRITERIA = ("von_mises", "tresca", "rankine")
AGGREGATES = ("max", "mean", "pnorm", "ks")
FIELDS = ("von_mises", "sigma1", "sigma2", "max_shear", "angle", "criterion")


def _cid(criterion):
    return CRITERIA.index(criterion) if isinstance(criterion, str) else int(criterion)


def _aid(aggregate):
    return AGGREGATES.index(aggregate) if isinstance(aggregate, str) else int(aggregate)


def _parts(sigma):
    s = np.asarray(sigma, np.float64).reshape(-1, 3)
    x, y, xy = s[:, 0], s[:, 1], s[:, 2]
    m, d = (x + y) / 2.0, (x - y) / 2.0
    r = np.sqrt(d * d + xy * xy)
    return x, y, xy, m, d, r


def von_mises(sigma):
    x, y, xy, _, _, _ = _parts(sigma)
    return np.sqrt(0.5 * ((x - y) * (x - y) + x * x + y * y + 6.0 * (xy * xy)))


def _tresca_branch(r, s1, s2):
    """0: 2 r, 1: |s1|, 2: |s2|; NaN rows fall to branch 2, as comparisons with a NaN are false."""
    t2, a1, a2 = 2.0 * r, np.abs(s1), np.abs(s2)
    with np.errstate(invalid="ignore"):
        return np.where((t2 >= a1) & (t2 >= a2), 0, np.where(a1 >= a2, 1, 2))


def criterion_values(sigma, criterion):
    """(n,) fp64 criterion values; a NaN row gives NaN."""
    cid = _cid(criterion)
    x, y, xy, m, d, r = _parts(sigma)
    if cid == 0:
        return von_mises(sigma)
    s1, s2 = m + r, m - r
    if cid == 1:
        b = _tresca_branch(r, s1, s2)
        return np.where(b == 0, 2.0 * r, np.where(b == 1, np.abs(s1), np.abs(s2)))
    with np.errstate(invalid="ignore"):
        return np.where(s1 <= 0.0, 0.0, s1)   # max(s1, 0) that keeps a NaN


def fields(sigma, criterion="von_mises"):
    """The six per-node fields in fp64, keyed by FIELDS."""
    x, y, xy, m, d, r = _parts(sigma)
    return {"von_mises": von_mises(sigma), "sigma1": m + r, "sigma2": m - r, "max_shear": r,
            "angle": 0.5 * np.arctan2(xy, d), "criterion": criterion_values(sigma, criterion)}


def criterion_grad(sigma, criterion):
    """(n, 3) fp64: d criterion / d (sx, sy, sxy), the gradient of the chosen branch; 0 at vm == 0 and r == 0."""
    cid = _cid(criterion)
    x, y, xy, m, d, r = _parts(sigma)
    with np.errstate(invalid="ignore", divide="ignore"):
        if cid == 0:
            vm = von_mises(sigma)
            h = 2.0 * vm
            g = np.stack([(2.0 * x - y) / h, (2.0 * y - x) / h, (6.0 * xy) / h], 1)
            g[vm == 0.0] = 0.0
            return g
        a = d / (2.0 * r)
        dr = np.stack([a, -a, xy / r], 1)
        dr[r == 0.0] = 0.0
        half = np.array([0.5, 0.5, 0.0])
        s1, s2 = m + r, m - r
        if cid == 2:
            return np.where((s1 > 0.0)[:, None], half + dr, 0.0)
        b = _tresca_branch(r, s1, s2)
        g1 = np.sign(s1)[:, None] * (half + dr)
        g2 = np.sign(s2)[:, None] * (half - dr)
        return np.where((b == 0)[:, None], 2.0 * dr, np.where((b == 1)[:, None], g1, g2))


def _weights(n, weights):
    w = np.ones(n) if weights is None else np.asarray(weights, np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        part = w > 0.0
    return np.where(part, w, 0.0), part


def graph_criteria(sigma, weights=None, criterion="von_mises", p=8.0, rho=1.0):
    """One graph: ((max, mean, pnorm, ks), argmax).  No node, no participating node or a NaN criterion at a
    participating node: four NaNs and argmax -1."""
    c = criterion_values(sigma, criterion)
    w, part = _weights(len(c), weights)
    nan4 = (np.nan,) * 4
    if not part.any() or np.isnan(c[part]).any():
        return nan4, -1
    idx = np.flatnonzero(part)
    c, w = c[idx], w[idx]
    M = c.max()
    am = int(idx[np.argmax(c)])   # numpy's argmax: the first of equal maxima
    W = w.sum()
    mean = (w * c).sum() / W
    pn = M * ((w * (c / M) ** p).sum() / W) ** (1.0 / p) if M > 0.0 else 0.0
    ks = M + np.log((w * np.exp(rho * (c - M))).sum() / W) / rho
    return (M, mean, pn, ks), am


def graph_criteria_grad(sigma, weights=None, criterion="von_mises", aggregate="pnorm", p=8.0, rho=1.0,
                        g_value=1.0):
    """One graph: (n, 3) fp64 = g_value d J / d sigma.  Exact zero rows at nodes that take no part; NaN rows at
    the participating nodes of a NaN graph."""
    aid = _aid(aggregate)
    s = np.asarray(sigma, np.float64).reshape(-1, 3)
    out = np.zeros_like(s)
    c = criterion_values(s, criterion)
    w, part = _weights(len(c), weights)
    if not part.any():
        return out
    (M, mean, pn, ks), am = graph_criteria(s, weights, criterion, p, rho)
    if am < 0:
        out[part] = np.nan
        return out
    dc = criterion_grad(s, criterion)
    W = w.sum()
    if aid == 0:
        wn = np.zeros(len(c))
        wn[am] = 1.0
    elif aid == 1:
        wn = w / W
    elif aid == 2:
        wn = (w / W) * (c / pn) ** (p - 1.0) if pn != 0.0 else np.zeros(len(c))
    else:
        e = w * np.exp(rho * (c - M))
        wn = e / e[part].sum()
    out[part] = g_value * (wn[part, None] * dc[part])
    return out


def batch_criteria(ptr, sigma, weights=None, criterion="von_mises", p=8.0, rho=1.0):
    """(table (B, 4), argmax (B,)) over the node segments ptr[0..B]."""
    ptr = np.asarray(ptr, np.int64)
    B = len(ptr) - 1
    table, am = np.full((B, 4), np.nan), np.full(B, -1, np.int64)
    s = np.asarray(sigma, np.float64).reshape(-1, 3)
    for g in range(B):
        n0, n1 = int(ptr[g]), int(ptr[g + 1])
        if n1 > n0:
            table[g], am[g] = graph_criteria(s[n0:n1], None if weights is None else weights[n0:n1], criterion, p, rho)
    return table, am


def batch_criteria_grad(ptr, sigma, weights=None, criterion="von_mises", aggregate="pnorm", p=8.0, rho=1.0,
                        g_value=None):
    ptr = np.asarray(ptr, np.int64)
    s = np.asarray(sigma, np.float64).reshape(-1, 3)
    out = np.zeros_like(s)
    for g in range(len(ptr) - 1):
        n0, n1 = int(ptr[g]), int(ptr[g + 1])
        if n1 > n0:
            out[n0:n1] = graph_criteria_grad(s[n0:n1], None if weights is None else weights[n0:n1], criterion,
                                             aggregate, p, rho, 1.0 if g_value is None else float(g_value[g]))
    return out
