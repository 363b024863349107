"""fp64 restatement of pdg_phys_loss_fwd / pdg_phys_loss_bwd / pdg_loss_reduce_phys (csrc/pdg_physloss.hip) in numpy,
built on boundary_ref.py (the traction and periodic sums) and homog_ref.py (the weighted sums): the same fp64 terms,
formed from the inputs as given (fp32 arrays are widened first; fp64 arrays serve the finite differences), every sum
taken with math.fsum.

Every term is evaluated on z = y + mean / std, the standardised prediction moved back to sigma / std.  The training
rule differs from the diagnostics': a term whose denominator is not > 0 is absent for that graph (loss exactly 0,
gradient rows exactly 0), never NaN.  A group passed as None is absent for every graph.
"""
import math

import numpy as np

import boundary_ref as BR

COLS = ("L_int", "T2", "P2", "n_pairs", "W", "S_xx", "S_yy", "S_xy", "D", "traction", "periodic", "mean")


def cases():
    """The issue's inputs: a batch of four triangle plates (periodic with a hole; not periodic; no hole; more rows
    than the per-graph workgroup has threads) and one quad plate."""
    from pdg import meshgen
    tri = [meshgen.hole_plate(13, hole_radius=0.2), meshgen.hole_plate(9, hole_radius=0.2, periodic=False),
           meshgen.hole_plate(7, hole_radius=0.0), meshgen.hole_plate(37, hole_radius=0.2)]
    return tri, [meshgen.quad_hole_plate(13, hole_radius=0.2)]


def box_area(bbox):
    b = np.asarray(bbox, np.float32).astype(np.float64)
    return (b[1] - b[0]) * (b[3] - b[2])


class Inputs:
    """The kernels' host-side inputs for a list of samples: ptr, edges, the mesh fields of pdg.meshgen, a random
    standardised field y, the affine pair and the targets."""

    def __init__(self, samples, seed=11, std=37.5, mean=12.25):
        from pdg import meshgen
        counts = [s.num_nodes for s in samples]
        self.samples = samples
        self.ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.B, self.N = len(samples), int(self.ptr[-1])
        self.ei = np.concatenate([s.edge_index + self.ptr[i] for i, s in enumerate(samples)], 1)
        self.ea = np.concatenate([s.edge_attr for s in samples])
        vecs = [meshgen.boundary_vectors(s.pos, s.faces) for s in samples]
        areas = [meshgen.nodal_areas(s.pos, s.faces) for s in samples]
        self.bvec = np.concatenate([v[0] for v in vecs])
        self.blen = np.concatenate([v[1] for v in vecs])
        self.labels = np.concatenate([s.node_types for s in samples])
        self.area = np.concatenate([a[0] for a in areas])
        self.cell = np.array([box_area(a[1]) for a in areas])
        rng = np.random.default_rng(seed)
        self.y = rng.normal(0.0, 1.0, (self.N, 3)).astype(np.float32)
        self.affine = np.array([std, mean], np.float32)
        self.target = np.stack([s.mean_stress for s in samples]).astype(np.float32)

    def groups(self, denom=True):
        return dict(boundary=(self.bvec, self.blen, self.labels), edges=(self.ei, self.ea),
                    mean=(self.area, self.target, self.cell if denom else None))


def shifted(y, affine):
    """z = y + mean / std in fp64 (std and mean widened from what is given)."""
    a = np.asarray(affine, np.float64)
    return np.asarray(y, np.float64) + a[1] / a[0]


def _fsum(x):
    x = np.asarray(x, np.float64)
    return math.fsum(x) if np.isfinite(x).all() else float(np.sum(x))


def forward(ptr, y, affine, boundary=None, edges=None, mean=None):
    """(table (B, 12) fp64, loss (B, 3) fp64 = the last three columns)."""
    ptr = np.asarray(ptr, np.int64)
    z = shifted(y, affine)
    n, B = len(z), len(ptr) - 1
    sd = float(np.asarray(affine, np.float64)[0])
    table = np.zeros((B, 12))
    if boundary is not None or edges is not None:
        if boundary is None:
            bvec, blen, labels = np.zeros((n, 2)), np.zeros(n), np.zeros(n, np.int64)
        else:
            bvec, blen, labels = boundary
        bt, _, _ = BR.residuals(ptr, z, bvec, blen, labels, edges)
        table[:, 0], table[:, 1], table[:, 2], table[:, 3] = bt[:, 0], bt[:, 2], bt[:, 7], bt[:, 8]
    if mean is not None:
        area, target, denom = mean
        w = np.asarray(area, np.float64)
        with np.errstate(invalid="ignore"):
            keep = w > 0
        for g in range(B):
            idx = np.arange(ptr[g], ptr[g + 1])
            idx = idx[keep[idx]]
            table[g, 4] = _fsum(w[idx])
            for c in range(3):
                table[g, 5 + c] = _fsum(w[idx] * z[idx, c])
        table[:, 8] = table[:, 4] if denom is None else np.asarray(denom, np.float64).reshape(-1)
        t = np.asarray(target, np.float64).reshape(B, 3) / sd
    for g in range(B):
        L, T2, P2, npairs, W, D = table[g, 0], table[g, 1], table[g, 2], table[g, 3], table[g, 4], table[g, 8]
        table[g, 9] = T2 / L if L > 0 else 0.0
        table[g, 10] = P2 / npairs if npairs > 0 else 0.0
        if mean is not None and D > 0 and W > 0:
            d = table[g, 5:8] / D - t[g]
            table[g, 11] = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    return table, table[:, 9:12].copy()


def objective(ptr, y, affine, scale, boundary=None, edges=None, mean=None):
    """sum_g scale . loss_g over the terms whose weight is not 0."""
    _, loss = forward(ptr, y, affine, boundary, edges, mean)
    total = 0.0
    for k in range(3):
        if scale[k] != 0:
            total += float(scale[k]) * _fsum(loss[:, k])
    return total


def backward(ptr, y, affine, table, scale, boundary=None, edges=None, mean=None):
    """(grad (N, 3) fp64, mag (N, 3): the sum of the absolute values of each element's terms) of `objective` with
    respect to y, with the kernel's rules: a zero weight or a denominator that is not > 0 switches a term off."""
    ptr = np.asarray(ptr, np.int64)
    z = shifted(y, affine)
    n, B = len(z), len(ptr) - 1
    sd = float(np.asarray(affine, np.float64)[0])
    table = np.asarray(table, np.float64)
    scale = np.asarray(scale, np.float64)
    grad, mag = np.zeros((n, 3)), np.zeros((n, 3))
    with np.errstate(invalid="ignore"):
        on_t = (scale[0] != 0) & (table[:, 0] > 0) & (boundary is not None)
        on_p = (scale[1] != 0) & (table[:, 3] > 0) & (edges is not None)
        on_m = (scale[2] != 0) & (table[:, 8] > 0) & (table[:, 4] > 0) & (mean is not None)
    if on_t.any() or on_p.any():
        if boundary is None:
            bvec, blen, labels = np.zeros((n, 2)), np.zeros(n), np.zeros(n, np.int64)
        else:
            bvec, blen, labels = boundary
        # boundary_ref's columns: L_int at 0, n_pairs at 8; its NaN rule never applies (weights are zeroed here)
        bt = np.zeros((B, 9))
        bt[:, 0], bt[:, 8] = table[:, 0], table[:, 3]
        g, m = BR.residuals_grad(ptr, z, bvec, blen, labels, edges, bt, np.where(on_t, scale[0], 0.0),
                                 np.where(on_p, scale[1], 0.0))
        grad += g
        mag += m
    if on_m.any():
        area, target, _ = mean
        w = np.asarray(area, np.float64)
        t = np.asarray(target, np.float64).reshape(B, 3) / sd
        graph = np.searchsorted(ptr, np.arange(n), side="right") - 1
        for i in range(n):
            g = graph[i]
            if on_m[g] and w[i] > 0:
                D = table[g, 8]
                c = scale[2] * (2.0 * w[i] / D)
                grad[i] += c * (table[g, 5:8] / D - t[g])
                mag[i] += abs(c) * (np.abs(table[g, 5:8]) / D + np.abs(t[g]))
    return grad, mag


def reduce(loss_nmse, loss_div, loss_phys, scale_nmse, scale_div, scale_phys, flag=1.0):
    """pdg_loss_reduce_phys's seven values in fp32 arithmetic (out[1] + out[2] is the kernel's fused multiply-add:
    the exact fp64 product plus out[2], rounded to fp64 and then to fp32)."""
    f = np.float32
    sn = f(_fsum(np.asarray(loss_nmse, np.float64)))
    fn = sn * f(scale_nmse)
    fd = f(0) if loss_div is None else f(_fsum(np.asarray(loss_div, np.float64))) * f(scale_div)
    out = [f(flag), fn, fd, f(np.float64(sn) * np.float64(f(scale_nmse)) + np.float64(fd))]
    for k in range(3):
        w = f(0) if loss_phys is None else f(scale_phys[k])
        v = f(0) if w == 0 else f(_fsum(np.asarray(loss_phys, np.float64)[:, k])) * w
        out.append(f(v))
        out[3] = f(out[3] + v)
    return np.array(out, np.float32)
