"""Numpy-only restatements of the equilibration (csrc/pdg_equil.hip, gnn_local_stress/equilibrate.py) for one graph:
a dense fp64 one (the constraint operator C, S = C W^-1 C^T, the multipliers by numpy.linalg.lstsq, the projection
P, its transpose and cond(S) over the non-zero spectrum) and an fp32-vector / fp64-sum restatement of the kernel's
conjugate-gradient iteration on the operator's COO entries.  Not a test.

Layouts: a field is (n, 3) in xx, yy, xy order and flattens to index 3 c + k; a constraint vector is (n, 2) and
flattens to 2 v + k.  The operator is A = [Dx | Dy]: COO rows, cols (col < n: Dx, else Dy, col >= 2 n ignored),
vals fp32.  m_v = 1 where node_types[v] == 0.  W = diag(w, w, 2 w)."""
from functools import lru_cache

import numpy as np

# name -> (quad, n, hole radius as a fraction of the side): the five meshes of the issue's probe
MESHES = {"tri9": (False, 9, 0.25), "tri17": (False, 17, 0.2), "tri25": (False, 25, 0.2),
          "tri17_full": (False, 17, 0.0), "quad17": (True, 17, 0.2)}


@lru_cache(maxsize=None)
def mesh(name):
    from pdg import meshgen
    quad, n, hole = MESHES[name]
    return (meshgen.quad_hole_plate if quad else meshgen.hole_plate)(n=n, hole_radius=hole, seed=3)


def noisy_field(sample, seed=11, level=0.05):
    """local_stress plus `level` x its rms of seeded normal noise, fp32."""
    s = sample.local_stress.astype(np.float64)
    rng = np.random.default_rng(seed)
    return (s + level * np.sqrt(np.mean(s * s)) * rng.standard_normal(s.shape)).astype(np.float32)


def areas(sample):
    from pdg import meshgen
    w, box = meshgen.nodal_areas(sample.pos, sample.faces)
    b = box.astype(np.float64)
    return w.astype(np.float32), float((b[1] - b[0]) * (b[3] - b[2]))


class Operator:
    """The kept COO entries of one graph's operator and its mask."""

    def __init__(self, rows, cols, vals, node_types):
        n = len(node_types)
        rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
        keep = cols < 2 * n
        self.n = n
        self.rows, self.vals = rows[keep], np.asarray(vals, np.float32)[keep].astype(np.float64)
        self.x = cols[keep] < n
        self.node = np.where(self.x, cols[keep], cols[keep] - n)
        self.mask = (np.asarray(node_types).reshape(-1) == 0).astype(np.float64)

    @classmethod
    def of(cls, sample, node_types=None):
        return cls(sample.op_div_rows, sample.op_div_cols, sample.op_div_vals,
                   sample.node_types if node_types is None else node_types)

    def apply(self, f):
        """C f, (n, 2) fp64, from a field (n, 3)."""
        f = np.asarray(f, np.float64)
        u0 = np.where(self.x, f[self.node, 0], f[self.node, 2])
        u1 = np.where(self.x, f[self.node, 2], f[self.node, 1])
        d = np.stack([np.bincount(self.rows, self.vals * u0, self.n), np.bincount(self.rows, self.vals * u1, self.n)], 1)
        return d * self.mask[:, None]

    def apply_t(self, q):
        """C^T q, (n, 3) fp64, from a constraint vector (n, 2)."""
        q = np.asarray(q, np.float64) * self.mask[:, None]
        qx, qy = self.vals * q[self.rows, 0], self.vals * q[self.rows, 1]
        return np.stack([np.bincount(self.node, np.where(self.x, qx, 0.0), self.n),
                         np.bincount(self.node, np.where(self.x, 0.0, qy), self.n),
                         np.bincount(self.node, np.where(self.x, qy, qx), self.n)], 1)

    def dense(self):
        """C as a (2 n, 3 n) fp64 matrix."""
        n = self.n
        C = np.zeros((2 * n, 3 * n))
        # x block: (sxx, sxy); y block: (sxy, syy)
        np.add.at(C, (2 * self.rows, 3 * self.node + np.where(self.x, 0, 2)), self.vals)
        np.add.at(C, (2 * self.rows + 1, 3 * self.node + np.where(self.x, 2, 1)), self.vals)
        return C * np.repeat(self.mask, 2)[:, None]

    def defect(self, f):
        """|C f|_2 in fp64."""
        return float(np.linalg.norm(self.apply(f)))


def metric(w, n):
    """diag(W) over the flat field, (3 n,) fp64; w None is ones."""
    w = np.ones(n) if w is None else np.asarray(w, np.float64)
    return (w[:, None] * np.array([1.0, 1.0, 2.0])).reshape(-1)


def wnorm(t, w=None):
    t = np.asarray(t, np.float64)
    return float(np.sqrt(np.sum(metric(w, len(t)) * t.reshape(-1) ** 2)))


class Dense:
    """The dense fp64 projection of one graph."""

    def __init__(self, op, w=None):
        self.op, self.n = op, op.n
        self.W = metric(w, op.n)
        self.C = op.dense()
        self.S = (self.C / self.W) @ self.C.T

    def multipliers(self, rhs):
        return np.linalg.lstsq(self.S, rhs, rcond=None)[0]

    def project(self, sigma):
        """sigma* = sigma - W^-1 C^T lam with S lam = C sigma."""
        s = np.asarray(sigma, np.float64).reshape(-1)
        return (s - (self.C.T @ self.multipliers(self.C @ s)) / self.W).reshape(-1, 3)

    def project_t(self, g):
        """P^T g = g - C^T mu with S mu = C W^-1 g."""
        g = np.asarray(g, np.float64).reshape(-1)
        return (g - self.C.T @ self.multipliers(self.C @ (g / self.W))).reshape(-1, 3)

    def matrix(self):
        """P = I - W^-1 C^T S^+ C, (3 n, 3 n)."""
        return np.eye(3 * self.n) - (self.C.T / self.W[:, None]) @ np.linalg.lstsq(self.S, self.C, rcond=None)[0]

    def cond(self):
        """lambda_max / lambda_min of S over its non-zero spectrum (the masked rows are zero rows of S)."""
        ev = np.linalg.eigvalsh(self.S)
        ev = ev[ev > 1e-12 * ev[-1]]
        return float(ev[-1] / ev[0])

    def rank_deficit(self):
        """Interior constraint rows minus rank(S): 0 when S has full rank on the interior rows."""
        ev = np.linalg.eigvalsh(self.S)
        return int(2 * self.op.mask.sum()) - int((ev > 1e-12 * ev[-1]).sum())

    def joint(self, sigma, target, denom):
        """The minimiser of |s - sigma|_W subject to C s = 0 and sum_v w_v s[v] / denom = target, by the dense KKT
        system (the constraint rows of C that are identically zero dropped)."""
        n = self.n
        s = np.asarray(sigma, np.float64).reshape(-1)
        live = np.repeat(self.op.mask, 2) > 0
        M = np.zeros((3, 3 * n))
        for k in range(3):
            M[k, k::3] = self.W[0::3] / denom
        G = np.concatenate([self.C[live], M])
        K = np.block([[np.diag(self.W), G.T], [G, np.zeros((len(G), len(G)))]])
        rhs = np.concatenate([self.W * s, np.zeros(int(live.sum())), np.asarray(target, np.float64)])
        return np.linalg.lstsq(K, rhs, rcond=None)[0][:3 * n].reshape(-1, 3)

    def mean_shift(self, sigma, target, denom):
        """homogenise.enforce_mean in fp64: sigma + (target denom - sum w sigma) / sum w."""
        s = np.asarray(sigma, np.float64)
        w = self.W[0::3]
        return s + (np.asarray(target, np.float64) * denom - w @ s) / w.sum()


def cg32(op, x, w=None, transpose=False, rtol=1e-5, max_iter=1000):
    """The kernel's iteration: fp32 vectors, each product row accumulated in fp64 and rounded once, fp64 inner
    products.  Returns (out fp32 (n, 3), (|b|, true residual, iterations, status))."""
    f32, f64 = np.float32, np.float64
    x = np.asarray(x, f32)
    n = op.n
    iw = (1.0 / metric(w, n)).reshape(n, 3)
    pre = iw if transpose else 1.0
    b = op.apply(x.astype(f64) * pre)
    bnorm = float(np.sqrt(np.sum(b * b)))
    if bnorm == 0.0:
        return x.copy(), (0.0, 0.0, 0, 0)
    lam = np.zeros((n, 2), f32)
    r = b.astype(f32)
    p = r.copy()
    rr, tol, it = bnorm * bnorm, float(f32(rtol)) * bnorm, 0
    res = bnorm
    while it < max_iter and not res <= tol:
        work = (op.apply_t(p) * iw).astype(f32)
        sp = op.apply(work).astype(f32)
        psp = float(np.sum(p.astype(f64) * sp.astype(f64)))
        if not psp > 0.0:
            break
        alpha = rr / psp
        lam = (lam.astype(f64) + alpha * p.astype(f64)).astype(f32)
        r = (r.astype(f64) - alpha * sp.astype(f64)).astype(f32)
        rrn = float(np.sum(r.astype(f64) ** 2))
        p = (r.astype(f64) + (rrn / rr) * p.astype(f64)).astype(f32)
        rr, res = rrn, float(np.sqrt(rrn))
        it += 1
    if it == 0:
        out = x.copy()
    else:
        out = (x.astype(f64) - op.apply_t(lam) * (1.0 if transpose else iw)).astype(f32)
    tres = float(np.linalg.norm(op.apply(out.astype(f64) * pre)))
    return out, (bnorm, tres, it, (0 if res <= tol else 1) | (0 if tres <= 2.0 * tol else 2))
