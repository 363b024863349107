"""Plain torch restatement of one message-passing step's node backward and of the backward's two ends (what
pdg_node_bwd_coop, pdg_gemm_sum2_coop, pdg_decoder_bwd_coop, pdg_mlp2_bwd_coop and pdg_ln_colsum_nodes compute,
include/pdivgnn.h), in the dtype of the caller's choice (float64: the reference; float32: the yardstick of the
per-row check).  tests/test_node_bwd_ref.py anchors every closed form to torch autograd through
oracle.epd_oracle.graph_layer_norm; tests/test_gpu_node_bwd.py holds the kernels to them.

The weight arguments named ...T are the arrays the kernels take (pdg/engine.py `transposed`): XT = X.T stored
row-major, so that "X^T g" over rows is g @ XT.T.  The relu masks come from the a1 / a2 arrays as given (the fp32
arrays the kernels read: converting them changes no sign)."""
from __future__ import annotations

from types import SimpleNamespace

import torch

from edge_bwd_ref import L, LN_EPS, ln_bwd


def _c(dtype, *ts):
    return [None if t is None else t.detach().to("cpu", dtype) for t in ts]


def node_bwd_ref(gy, a2n, a1n, ln_g, Wn2T, Wn1aT, Wn1bT, dtype=torch.float64, eps=LN_EPS):
    """node_net backward of one step: ga2 = LN_bwd(gy); gz2 = ga2 [a2n > 0]; gz1 = (Wn2^T gz2) [a1n > 0];
    gaggr = Wn1a^T gz1; gx_part = Wn1b^T gz1 + gy.  r.ln: ln_bwd's statistics, column sums, S1 and S2."""
    gy, a2n, a1n, ln_g, Wn2T, Wn1aT, Wn1bT = _c(dtype, gy, a2n, a1n, ln_g, Wn2T, Wn1aT, Wn1bT)
    r = SimpleNamespace()
    r.ga2, r.ln = ln_bwd(gy, a2n, ln_g, eps)
    r.gz2 = r.ga2 * (a2n > 0)
    r.gz1 = (r.gz2 @ Wn2T.T) * (a1n > 0)
    r.gaggr = r.gz1 @ Wn1aT.T
    r.gx_part = r.gz1 @ Wn1bT.T + gy
    return r


def gemm_sum2_ref(in0, in1, W0T, W1T, res=None, dtype=torch.float64):
    """out = W0^T in0 + W1^T in1 [+ res]."""
    in0, in1, W0T, W1T, res = _c(dtype, in0, in1, W0T, W1T, res)
    out = in0 @ W0T.T + in1 @ W1T.T
    return out if res is None else out + res


def decoder_bwd_ref(gy3, a1d, Wd2, Wd1T, dtype=torch.float64):
    """gz1d = (Wd2^T gy) [a1d > 0] (Wd2: 3 x 128, gy: rows x 3); gx = Wd1^T gz1d; node_decoder.2's weight / bias
    gradient dWd2 = gy^T a1d (3 x 128), dbd2 = sum gy."""
    gy3, a1d, Wd2, Wd1T = _c(dtype, gy3, a1d, Wd2, Wd1T)
    r = SimpleNamespace()
    r.gz1d = (gy3 @ Wd2) * (a1d > 0)
    r.gx = r.gz1d @ Wd1T.T
    r.dWd2 = gy3.T @ a1d
    r.dbd2 = gy3.sum(0)
    return r


def mlp2_bwd_ref(gy, a2, a1, ln_g, W2T, x_narrow=None, dtype=torch.float64, eps=LN_EPS):
    """An MLP tail backwards (LN -> relu -> Linear2 -> relu): gz2 = LN_bwd(gy) [a2 > 0]; gz1 = (W2^T gz2) [a1 > 0];
    with x_narrow (rows x k, the first layer's input) the first layer's gradients dW0 = gz1^T x_narrow (128 x k)
    and db0 = sum gz1."""
    gy, a2, a1, ln_g, W2T, x_narrow = _c(dtype, gy, a2, a1, ln_g, W2T, x_narrow)
    r = SimpleNamespace()
    r.ga2, r.ln = ln_bwd(gy, a2, ln_g, eps)
    r.gz2 = r.ga2 * (a2 > 0)
    r.gz1 = (r.gz2 @ W2T.T) * (a1 > 0)
    if x_narrow is not None:
        r.dW0 = r.gz1.T @ x_narrow
        r.db0 = r.gz1.sum(0)
    return r


def colsums(gy, a2, ln_g, dtype=torch.float64, eps=LN_EPS):
    """What a column-sum producer emits for the LayerNorm over a2 with upstream gradient gy, summed over its
    blocks: (cols, S1, S2) with cols = [sum gy (128) | sum gy xhat (128)], S1 = sum_c g_c cols_c,
    S2 = sum_c g_c cols_{128 + c}."""
    gy, a2, ln_g = _c(dtype, gy, a2, ln_g)
    _, info = ln_bwd(gy, a2, ln_g, eps)
    return torch.cat([info.col_gy, info.col_gyx]), info.S1, info.S2


def colsums_nodes(gaggr, dst, a2m, ln_g, xs=None, dtype=torch.float64, eps=LN_EPS):
    """colsums for the message LayerNorm, whose upstream gradient is gy_k = gaggr[dst_k], in the node-level form
    pdg_ln_colsum_nodes evaluates: sum_k gy_k = sum_v deg_v gaggr_v, sum_k gy_k xhat_k = sum_v gaggr_v xs_v with
    xs_v the sum of xhat over the edges into v -- formed here from a2m, or the array the kernel is given (the
    forward's pdg_segment_sum output), which makes this the exact value of what the kernel is asked for."""
    gaggr, a2m, ln_g, xs = _c(dtype, gaggr, a2m, ln_g, xs)
    dst = dst.detach().cpu().long()
    N = gaggr.shape[0]
    deg = torch.bincount(dst, minlength=N).to(dtype).unsqueeze(1)
    if xs is None:
        mean = a2m.mean()
        xc = a2m - mean
        xhat = xc / (xc.pow(2).mean().sqrt() + eps)
        xs = torch.zeros(N, L, dtype=dtype).index_add_(0, dst, xhat)
    cols = torch.cat([(deg * gaggr).sum(0), (gaggr * xs).sum(0)])
    return cols, (ln_g * cols[:L]).sum(), (ln_g * cols[L:]).sum()
