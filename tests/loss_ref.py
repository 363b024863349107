"""Plain torch float64 restatements of the kernels that end a training step (include/pdivgnn.h: pdg_div_fwd,
pdg_div_bwd, pdg_nmse_*, pdg_loss_reduce, pdg_nonfinite2, pdg_format_inputs), a host builder of the divergence
operator's CSR / CSR^T arrays in the layout pdg_div_plan documents, and the seeded inputs the op tests feed the
kernels.  Nothing here imports pdg.lib.

tests/test_loss_ref.py anchors these to the oracle (oracle.epd_oracle.compute_divergence, the dense form tied to
the upstream golden vectors, and autograd through it) and to the plan's CPU path; tests/test_gpu_loss_ops.py
holds the kernels to them."""
from __future__ import annotations

from types import SimpleNamespace

import torch

from oracle import epd_oracle as O

U = 2.0 ** -24    # unit roundoff of fp32
F64 = torch.float64


def _cpu(t, dtype=None):
    t = torch.as_tensor(t).detach().cpu()
    return t if dtype is None else t.to(dtype)


def _segments(ptr, idx):
    """(graph, first node, node count) of each global node index in idx; ptr may hold empty graphs."""
    g = torch.searchsorted(ptr, idx, right=True) - 1
    return g, ptr[g], ptr[g + 1] - ptr[g]


def _rows_of(rowptr):
    n = rowptr.numel() - 1
    return torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])


# ---------------------------------------------------------------------------------------------- divergence
def div_fwd_ref(ptr, a_rowptr, a_col, a_val, types, sigma, reduce_abs):
    """pdg_div_fwd in fp64.  Columns are graph-local: col < n_g reads [sxx, sxy] of node col, n_g <= col < 2 n_g
    reads [sxy, syy] of node col - n_g, any other column is ignored; rows of type +-1 are zeroed; loss_g is the
    mean over all n_g rows of |div| (reduce_abs) or div^2, summed over the two components (NaN for an empty
    graph, as torch.mean of an empty tensor).  sigma may require grad.

    Returns (div (N, 2), loss (B,), bound (N, 2)): bound[v] = (nnz_v + 1) 2^-24 sum_j |a_j| |s_j| over the nnz_v
    entries the row uses, the standard bound of a length-nnz_v fp32 fma chain (nnz_v roundings,
    gamma_n = n u / (1 - n u) <= (n + 1) u while n^2 u <= 1); 0 on the zeroed rows."""
    ptr, a_rowptr, a_col = _cpu(ptr, torch.int64), _cpu(a_rowptr, torch.int64), _cpu(a_col, torch.int64)
    a_val, types = _cpu(a_val, F64), _cpu(types, torch.int64).reshape(-1)
    sig = sigma.double() if sigma.requires_grad else _cpu(sigma, F64)
    N = int(ptr[-1])
    row = _rows_of(a_rowptr)
    _, off, ng = _segments(ptr, row)
    xb = (a_col >= 0) & (a_col < ng)
    yb = (a_col >= ng) & (a_col < 2 * ng)
    used = xb | yb
    node = torch.where(used, off + torch.where(xb, a_col, a_col - ng), torch.zeros_like(off))
    a = a_val * used
    s0 = torch.where(xb, sig[node, 0], sig[node, 2])
    s1 = torch.where(xb, sig[node, 2], sig[node, 1])
    live = ~((types == 1) | (types == -1))
    terms = torch.stack([a * s0, a * s1], 1)
    div = torch.zeros(N, 2, dtype=F64).index_add(0, row, terms) * live[:, None]
    nnz = torch.bincount(row[used], minlength=N)
    bound = torch.zeros(N, 2, dtype=F64).index_add(0, row, terms.detach().abs())
    bound = bound * ((nnz + 1) * U)[:, None] * live[:, None]
    red = div.abs() if reduce_abs else div.square()
    loss = torch.stack([torch.mean(red[int(ptr[g]):int(ptr[g + 1])], 0).sum() for g in range(ptr.numel() - 1)])
    return div, loss, bound


def div_bwd_ref(ptr, at_rowptr, at_row, at_comp, at_val, div, scale, reduce_abs):
    """pdg_div_bwd in fp64, from the div it is handed: g_div[v] = scale * 2 div[v] / n_g ("square") or
    scale * sign(div[v]) / n_g ("abs"); node m collects its A^T entries j (source row v_j, value a_j): component
    block 0 (x) adds a g_div[v][0] to xx and a g_div[v][1] to xy, block 1 (y) adds a g_div[v][0] to xy and
    a g_div[v][1] to yy.

    Returns (g_sigma (N, 3), bound (N, 3)), columns [xx, yy, xy] as the kernel writes them.
    bound[m] = (nnz_m + 3) 2^-24 sum_j |a_j g_j|: the fp32 kernel forms f = c scale / n_g with one rounding
    (c = 2 or 1 is exact) and g_j = f d_j with another, so every term enters the fma chain with a relative
    error of at most 2 u + u^2, and the chain of at most nnz_m fmas adds gamma_nnz:
    (1 + u)^(nnz + 2) - 1 <= (nnz + 3) u while (nnz + 3)^2 u <= 1."""
    ptr, at_rowptr, at_row = _cpu(ptr, torch.int64), _cpu(at_rowptr, torch.int64), _cpu(at_row, torch.int64)
    at_comp, at_val, div = _cpu(at_comp, torch.int64), _cpu(at_val, F64), _cpu(div, F64)
    N = int(ptr[-1])
    m = _rows_of(at_rowptr)
    _, _, ng = _segments(ptr, m)
    f = (1.0 if reduce_abs else 2.0) * float(scale) / ng.double()
    d = div[at_row]
    gd = f[:, None] * (torch.sign(d) if reduce_abs else d)
    t0, t1 = at_val * gd[:, 0], at_val * gd[:, 1]
    x = at_comp == 0
    zero = torch.zeros_like(t0)
    terms = torch.stack([torch.where(x, t0, zero), torch.where(x, zero, t1), torch.where(x, t1, t0)], 1)
    gs = torch.zeros(N, 3, dtype=F64).index_add(0, m, terms)
    nnz = at_rowptr[1:] - at_rowptr[:-1]
    bound = torch.zeros(N, 3, dtype=F64).index_add(0, m, terms.abs()) * ((nnz + 3) * U)[:, None]
    return gs, bound


def loss_ref(ptr, a_rowptr, a_col, a_val, types, sigma, scale, reduce_abs):
    """The composed pass in fp64: (div, g_sigma) with g_sigma = d/d sigma of scale * sum_g loss_g by autograd
    (empty graphs, whose loss is NaN and which own no row, left out of the sum)."""
    sig = _cpu(sigma, F64).requires_grad_(True)
    div, loss, _ = div_fwd_ref(ptr, a_rowptr, a_col, a_val, types, sig, reduce_abs)
    (g,) = torch.autograd.grad(float(scale) * loss[~loss.isnan()].sum(), sig)
    return div.detach(), g


def abs_rows_left_out(op, div64, rel=1e-4):
    """Rows of g_sigma fed (through A^T) by a div entry with 0 < |div64| < rel * rms(div64): there the fp32 sign
    may legitimately differ from the fp64 one.  An exact zero (a zeroed or empty row) is zero in fp32 too."""
    near = ((div64.abs() > 0) & (div64.abs() < rel * div64.square().mean().sqrt())).any(1)
    m = _rows_of(op.at_rowptr.long())
    out = torch.zeros(div64.shape[0], dtype=torch.bool)
    out[m[near[op.at_row.long()]]] = True
    return out


# ---------------------------------------------------------------------------------------------- operator
def build_div_csr(ptr, rows, cols, vals, keep_beyond=False):
    """The arrays pdg_div_plan documents, from a COO operator (global rows, graph-local columns) on the host:
    an entry of row r belongs to the graph g with ptr[g] <= r < ptr[g + 1] and is kept when col < 2 n_g.
    a_rowptr / a_col / a_val: the kept entries by row in entry order; at_rowptr / at_row / at_comp / at_val: the
    same entries by global node ptr[g] + (col mod n_g), in entry order, at_comp = col >= n_g.
    keep_beyond: the A arrays also keep the entries with col >= 2 n_g (pdg_div_fwd must ignore them); the A^T
    arrays never hold them.  int32 / fp32 on the CPU."""
    ptr, rows, cols = _cpu(ptr, torch.int64), _cpu(rows, torch.int64), _cpu(cols, torch.int64)
    vals = _cpu(vals, torch.float32)
    N = int(ptr[-1])
    _, off, ng = _segments(ptr, rows)
    kept = cols < 2 * ng

    def csr(keys, sel):
        order = torch.sort(keys[sel], stable=True).indices
        rp = torch.zeros(N + 1, dtype=torch.int64)
        rp[1:] = torch.cumsum(torch.bincount(keys[sel], minlength=N), 0)
        return rp.int(), order

    sel = torch.ones_like(kept) if keep_beyond else kept
    a_rowptr, oa = csr(rows, sel)
    node = off + torch.where(cols < ng, cols, cols - ng)
    at_rowptr, ot = csr(node, kept)
    return SimpleNamespace(
        a_rowptr=a_rowptr, a_col=cols[sel][oa].int().contiguous(), a_val=vals[sel][oa].contiguous(),
        at_rowptr=at_rowptr, at_row=rows[kept][ot].int().contiguous(),
        at_comp=(cols >= ng)[kept][ot].int().contiguous(), at_val=vals[kept][ot].contiguous())


DIV_SIZES = (1, 2, 63, 64, 65, 0, 1023, 1024, 1025, 2500)   # both sides of the 1024-thread stride, an empty graph
DIV_SEED = 5


def random_div_case(sizes=DIV_SIZES, seed=DIV_SEED):
    """A seeded ragged batch for the divergence kernels: 0..20 entries per row with a tenth of the rows emptied,
    columns over both blocks, ~15 % of the entries repeating the column before them in their row, ~5 % with a
    column in [2 n_g, 2 n_g + 8), the COO entries in random order (so unsorted within a row); int64 types from
    {-1, 0, 1, 2}; fp32 Gaussian values and sigma."""
    g = torch.Generator().manual_seed(seed)
    ptr = torch.tensor([0] + list(torch.tensor(sizes).cumsum(0)), dtype=torch.int64)
    N = int(ptr[-1])
    k = torch.randint(0, 21, (N,), generator=g)
    k[torch.rand(N, generator=g) < 0.1] = 0
    rows = torch.repeat_interleave(torch.arange(N), k)
    _, _, ng = _segments(ptr, rows)
    nnz = rows.numel()
    cols = (torch.rand(nnz, generator=g, dtype=F64) * (2 * ng)).long().clamp(max=2 * ng - 1)
    beyond = torch.rand(nnz, generator=g) < 0.05
    cols = torch.where(beyond, 2 * ng + torch.randint(0, 8, (nnz,), generator=g), cols)
    rep = (torch.rand(nnz, generator=g) < 0.15)
    rep[0] = False
    rep[1:] &= rows[1:] == rows[:-1]
    for i in torch.nonzero(rep).reshape(-1).tolist():    # ascending, so runs of repeats chain
        cols[i] = cols[i - 1]
    vals = torch.randn(nnz, generator=g, dtype=F64).float()
    shuffle = torch.randperm(nnz, generator=g)
    types = torch.randint(-1, 3, (N,), generator=g)
    sigma = torch.randn(N, 3, generator=g, dtype=F64).float()
    return SimpleNamespace(sizes=tuple(sizes), ptr=ptr, N=N, B=len(sizes), rows=rows[shuffle], cols=cols[shuffle],
                           vals=vals[shuffle], types=types, sigma=sigma)


# ---------------------------------------------------------------------------------------------- NMSE
def nmse_ref(ptr, gt, pred, scale):
    """pdg_nmse_fwd / pdg_nmse_bwd in fp64: loss (B,) = oracle.epd_oracle.normalized_mse_loss_single per graph,
    den (B, 3) = sum_n (gt - mean gt)^2, grad (N, 3) = scale * d loss_g / d pred by autograd."""
    ptr, gt = _cpu(ptr, torch.int64), _cpu(gt, F64)
    pred = _cpu(pred, F64).requires_grad_(True)
    loss, den = [], []
    for g in range(ptr.numel() - 1):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        loss.append(O.normalized_mse_loss_single(gt[lo:hi], pred[lo:hi]))
        den.append((gt[lo:hi] - gt[lo:hi].mean(0)).square().sum(0))
    loss = torch.stack(loss)
    (grad,) = torch.autograd.grad(loss.sum(), pred)
    return loss.detach(), torch.stack(den), float(scale) * grad


# ---------------------------------------------------------------------------------------------- one-liners
def loss_reduce_ref(loss_nmse, loss_div, scale_nmse, scale_div, zero_flag):
    """pdg_loss_reduce in fp64: [flag (1 without one), scale_nmse sum nmse, scale_div sum div (0 without), total]."""
    a = scale_nmse * float(_cpu(loss_nmse, F64).sum())
    b = scale_div * float(_cpu(loss_div, F64).sum()) if loss_div is not None else 0.0
    return [1.0 if zero_flag is None else float(zero_flag), a, b, a + b]


def nonfinite_ref(x, zero_flag):
    """pdg_nonfinite2's flag: any non-finite x[i], or a zero_flag of (either) zero."""
    return int(bool((~torch.isfinite(_cpu(x))).any()) or (zero_flag is not None and float(zero_flag) == 0.0))


def format_ref(stats, pos, mean_stress, types, edge_attr, perm, scale_input, dtype=F64):
    """pdg_format_inputs: oracle.epd_oracle.format_inputs in `dtype`, the edge rows gathered by perm."""
    c = lambda t: _cpu(t, dtype)
    x, e = O.format_inputs({k: c(v) for k, v in stats.items()}, c(pos), c(mean_stress), c(types).reshape(-1, 1),
                           c(edge_attr), scale_input)
    return x, e.reshape(-1)[_cpu(perm, torch.int64)]
