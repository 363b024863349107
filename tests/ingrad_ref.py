"""Plain torch closed form of the two encoders' input gradients (what pdg_node_enc_gin / pdg_edge_enc_gin
compute, include/pdivgnn.h):  LN backward -> relu -> W2^T -> relu -> W0, then the unformat step (/ std, edges
back to the caller's order).

enc_gin_ref is the per-encoder chain in the dtype of its inputs' choice (float64: the reference of the op
tests); encoder_input_grads applies it to a whole model from the upstream gradients of the encoder outputs.
tests/test_ingrad_ref.py anchors both to torch autograd through oracle.epd_oracle and to finite differences."""
from __future__ import annotations

import torch

from edge_bwd_ref import ln_bwd


def enc_gin_ref(gy, a2, a1_mask, ln_g, W2, W0, dtype=torch.float64):
    """g_in (rows, in_features) = ((LN_bwd(gy) [a2 > 0]) W2 [a1 > 0]) W0 for an encoder
    Lin(W0) relu Lin(W2) relu LN: gy the gradient of its output, a2 its second relu's output, a1_mask the
    first relu's mask (bool, as the caller formed it: converting a2 changes no sign)."""
    c = lambda t: t.detach().to("cpu", dtype)
    gy, a2, ln_g, W2, W0 = map(c, (gy, a2, ln_g, W2, W0))
    ga2, _ = ln_bwd(gy, a2, ln_g)
    gz2 = ga2 * (a2 > 0)
    gz1 = (gz2 @ W2) * a1_mask.detach().cpu().to(dtype)
    return gz1 @ W0


def edge_a1_mask(e_in, w0, b0):
    """[w0 e + b0 > 0] (E, 128) in the dtype of the inputs; in float32 the product and the sum are each
    rounded once, as the kernels' fma(w0, e, 0) + b0."""
    return (e_in.reshape(-1, 1) * w0.reshape(1, -1) + b0.reshape(1, -1)) > 0


def edge_enc_gin_ref(gy, a2, e_in, w0, b0, ln_g, W2, perm, std_edge=None, dtype=torch.float64):
    """g_edge_attr (E,) in the caller's order: row k of the plan order is edge perm[k]."""
    g = enc_gin_ref(gy, a2, edge_a1_mask(e_in, w0, b0), ln_g, W2, w0.reshape(-1, 1), dtype)[:, 0]
    out = torch.empty_like(g)
    out[perm.detach().cpu().long()] = g
    return out if std_edge is None else out / float(std_edge)


def node_enc_gin_ref(gy, a2, a1, W0, ln_g, W2, std_ms=None, std_pos=None, dtype=torch.float64):
    """(g_mean_stress (N, 3), g_pos (N, 2)): columns 0-2 and 3-4 of g_in; column 5 (the node type) dropped."""
    g = enc_gin_ref(gy, a2, a1.detach().cpu() > 0, ln_g, W2, W0, dtype)
    gm, gp = g[:, :3], g[:, 3:5]
    if std_ms is not None:
        gm, gp = gm / float(std_ms), gp / float(std_pos)
    return gm, gp


def encoder_input_grads(P, stats, pos, mean_stress, nodes_types, edge_attr, gx0, ge0, scale_input=True):
    """(g_mean_stress, g_pos, g_edge_attr) of a model with parameters P (float64) from gx0 / ge0, the
    gradients of the encoder outputs x_0 (N, 128) / e_0 (E, 128, the caller's edge order): the encoders'
    forward (models.py:260-274 on format_node_features / format_edge_features, :140-162) restated, then
    enc_gin_ref.  Edges stay in the caller's order (identity permutation)."""
    from oracle.epd_oracle import format_inputs
    x, e = format_inputs(stats, pos, mean_stress, nodes_types, edge_attr, scale_input)
    out = []
    for name, inp, g in (("node_encoder", x, gx0), ("edge_encoder", e, ge0)):
        W0, b0, W2, b2 = (P[f"{name}.{k}"] for k in ("0.weight", "0.bias", "2.weight", "2.bias"))
        h1 = inp.to(W0.dtype) @ W0.T + b0
        a2 = torch.relu(torch.relu(h1) @ W2.T + b2)
        out.append(enc_gin_ref(g, a2, h1 > 0, P[f"{name}.4.weight"], W2, W0, W0.dtype))
    gn, ge = out
    gm, gp, gea = gn[:, :3], gn[:, 3:5], ge[:, 0]
    if scale_input:
        gm, gp = gm / stats["std_mean_stress"], gp / stats["std_pos"]
        gea = gea / stats["std_edge_weight"]
    return gm, gp, gea
