"""Plain torch restatement of one message-passing step's edge backward (what pdg_edge_bwd and
pdg_edge_bwd_w2 compute, include/pdivgnn.h), and the inputs the op tests feed both kernels.

edge_bwd_ref is the closed form in the dtype of its choice (float64: the reference; float32: the
yardstick of the per-row check).  tests/test_edge_bwd_ref.py anchors it to torch autograd through
oracle.epd_oracle.graph_layer_norm; tests/test_gpu_edge_bwd.py holds the kernels to it."""
from __future__ import annotations

from types import SimpleNamespace

import torch

LN_EPS = 1e-5   # oracle.epd_oracle.LN_EPS (the CPU test checks they agree)
L = 128


def ln_bwd(gy, a2, ln_g, eps=LN_EPS):
    """Backward of y = (a2 - mean) / (std + eps) * ln_g + b with the mean and the population std over ALL
    elements of a2 (graph mode).  Returns (ga2, info): info holds the statistics, the column sums
    sum gy and sum gy * xhat (the LayerNorm bias / weight gradients) and S1 = sum_c g_c sum gy_c,
    S2 = sum_c g_c sum (gy xhat)_c  (include/pdivgnn.h above pdg_ln_colsum)."""
    M = a2.numel()
    mean = a2.mean()
    xc = a2 - mean
    std = xc.pow(2).mean().sqrt()
    den = std + eps
    xhat = xc / den
    col_gy = gy.sum(0)
    col_gyx = (gy * xhat).sum(0)
    S1 = (ln_g * col_gy).sum()
    S2 = (ln_g * col_gyx).sum()
    ga2 = (ln_g * gy - S1 / M) / den - xhat * (S2 / (M * std))
    return ga2, SimpleNamespace(mean=mean, std=std, den=den, count=M, col_gy=col_gy, col_gyx=col_gyx, S1=S1, S2=S2)


def edge_bwd_ref(dst, gaggr, ge_next, a2m, a1m, a2e, a1e, ln_g, W2, Wc, dtype=torch.float64):
    """One step's edge backward on the CPU in `dtype`.  ge_next None: no edge update (a2e / a1e unused).
    The relu masks come from the a1 / a2 arrays as given (the fp32 arrays the kernels read: converting
    them changes no sign).  Returns ga2m, gz2m, gz1m, [ga2e, gz2e, gz1e,] gC, ge_out, dW2, db2, ln_m[, ln_e]."""
    c = lambda t: t.detach().to("cpu", dtype)
    dst = dst.detach().cpu().long()
    gaggr, a2m, a1m, ln_g, W2, Wc = map(c, (gaggr, a2m, a1m, ln_g, W2, Wc))
    r = SimpleNamespace(eu=ge_next is not None)
    r.ga2m, r.ln_m = ln_bwd(gaggr[dst], a2m, ln_g)
    r.gz2m = r.ga2m * (a2m > 0)
    r.gz1m = (r.gz2m @ W2) * (a1m > 0)
    r.dW2 = r.gz2m.T @ a1m
    r.db2 = r.gz2m.sum(0)
    r.gC = r.gz1m
    if r.eu:
        ge_next, a2e, a1e = map(c, (ge_next, a2e, a1e))
        r.ga2e, r.ln_e = ln_bwd(ge_next, a2e, ln_g)
        r.gz2e = r.ga2e * (a2e > 0)
        r.gz1e = (r.gz2e @ W2) * (a1e > 0)
        r.dW2 = r.dW2 + r.gz2e.T @ a1e
        r.db2 = r.db2 + r.gz2e.sum(0)
        r.gC = r.gz1m + r.gz1e
    r.ge_out = r.gC @ Wc
    if r.eu:
        r.ge_out = ge_next + r.ge_out
    return r


def hub_graph(E, seed=0):
    """A dst-sorted edge list as the plan delivers it, with the shapes a regular mesh never has: one hub
    node owning a run of at least min(E, max(40, E // 9)) consecutive rows, every 5th node without an incoming
    edge, 3 trailing nodes without any edge, N << E for large E.  Returns (N, src, dst, rowptr_dst,
    rowptr_src, perm_src) (int64, CPU), the row pointers and the src permutation as
    test_gpu_ops.test_pq_scatter_bwd builds them."""
    g = torch.Generator().manual_seed(1000 + 7 * E + seed)
    isolated = 3
    n_live = max(4, min(E, 6 + E // 12))
    N = n_live + isolated
    hub = n_live // 2 + (1 if (n_live // 2) % 5 == 0 else 0)   # not one of the edge-free nodes
    run = min(E, max(40, E // 9))
    live = torch.tensor([v for v in range(n_live) if v % 5 != 0])
    dst = live[torch.randint(0, live.numel(), (E,), generator=g)]
    dst[:run] = hub
    src = torch.randint(0, n_live, (E,), generator=g)  # the trailing nodes have no edge at all
    order = torch.sort(dst * N + src, stable=True).indices
    src, dst = src[order], dst[order]
    rp = torch.zeros(N + 1, dtype=torch.int64)
    rp[1:] = torch.cumsum(torch.bincount(dst, minlength=N), 0)
    perm_src = torch.sort(src * N + dst, stable=True).indices
    rps = torch.zeros(N + 1, dtype=torch.int64)
    rps[1:] = torch.cumsum(torch.bincount(src, minlength=N), 0)
    return N, src, dst, rp, rps, perm_src


def worst_row(x, ref):
    """max over rows r of |x_r - ref_r| / rms over rows of |ref_r|: one bad row shows, however many good
    ones a global L2 would average it with, and a row of tiny norm does not inflate the figure."""
    x, ref = x.detach().double().cpu(), ref.detach().double().cpu()
    scale = ref.pow(2).sum(1).mean().sqrt()
    return float((x - ref).pow(2).sum(1).sqrt().max() / max(float(scale), 1e-300))
