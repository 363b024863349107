"""float64 torch restatements of the tangent-pass entry points (csrc/pdg_tangent.hip), one function per entry
point with its operands, and their composition `epd_tangent`, which tests/test_tangent_ref.py anchors to
torch.func.jvp through the oracle.  The GPU op tests hold each kernel to its function here.

Tangents of a forward linearised at stored activations: relu -> mask [a > 0], biases drop out, the graph
LayerNorm y = g (a - mu) / (sigma + eps) + b over all n elements of `a` becomes
  dLN = g ((da - T1 / n) / (sigma + eps) - (a - mu) T2 / (n sigma (sigma + eps)^2)),  T1 = sum da, T2 = sum (a - mu) da.
Weights are nn.Linear (out x in) arrays."""
import torch

LN_EPS = 1e-5
D = torch.float64


def _d(t):
    return torch.as_tensor(t).detach().cpu().to(D)


def ln_tan(da, a, g=None):
    """dLN of the whole tensor (g None: without the weight)."""
    da, a = _d(da), _d(a)
    n = a.numel()
    mu, sd = a.mean(), a.std(unbiased=False)
    den = sd + LN_EPS
    xc = a - mu
    t1, t2 = da.sum(), (xc * da).sum()
    c2 = t2 / (n * sd * den * den) if float(sd) > 0 else 0.0
    out = (da - t1 / n) / den - xc * c2
    return out if g is None else out * _d(g)


def pairs_ref(da, a):
    """(T1, T2) of a pre-LayerNorm tangent."""
    da, a = _d(da), _d(a)
    return da.sum(), ((a - a.mean()) * da).sum()


def node_enc_tan_ref(dx_in, a1, W0, W2, a2):
    da1 = (_d(dx_in) @ _d(W0).T) * (_d(a1) > 0)
    return (da1 @ _d(W2).T) * (_d(a2) > 0)


def edge_enc_tan_ref(de_in, e_in, w0, b0, W2, a2):
    """The first layer's sign as the kernels recompute it in fp32: fma(w0, e, 0) + b0 > 0."""
    e32, w32, b32 = (torch.as_tensor(t).detach().cpu().float().reshape(-1) for t in (e_in, w0, b0))
    m1 = (e32[:, None] * w32[None, :] + b32[None, :]) > 0
    da1 = (_d(de_in).reshape(-1, 1) * _d(w0).reshape(1, -1)) * m1
    return (da1 @ _d(W2).T) * (_d(a2) > 0)


def node_pre_tan_ref(da2_prev, a2_prev, g, dx_res, W1):
    """(dx_t, dP, dQ); W1 = edge_net.0's 128 x 384 weight."""
    dx = ln_tan(da2_prev, a2_prev, g)
    if dx_res is not None:
        dx = dx + _d(dx_res)
    W1 = _d(W1)
    return dx, dx @ W1[:, :128].T, dx @ W1[:, 128:256].T


def edge_tan_ref(da2_prev, a2_prev, g, de_res, src, dst, dP, dQ, W1, W2, a1m, a2m, a1e=None, a2e=None):
    """(de_t, da2m, da2e or None)."""
    de = ln_tan(da2_prev, a2_prev, g)
    if de_res is not None:
        de = de + _d(de_res)
    src, dst = torch.as_tensor(src).cpu().long(), torch.as_tensor(dst).cpu().long()
    W1, W2, dP, dQ = _d(W1), _d(W2), _d(dP), _d(dQ)
    C = de @ W1[:, 256:].T
    da2m = (((C + dP[dst] + dQ[src]) * (_d(a1m) > 0)) @ W2.T) * (_d(a2m) > 0)
    da2e = None
    if a1e is not None:
        da2e = (((C + dP[src] + dQ[dst]) * (_d(a1e) > 0)) @ W2.T) * (_d(a2e) > 0)
    return de, da2m, da2e


def segment_sum_tan_ref(rowptr, da2m, a2m, g):
    t = ln_tan(da2m, a2m, g)
    rp = torch.as_tensor(rowptr).cpu().long()
    n = rp.numel() - 1
    idx = torch.repeat_interleave(torch.arange(n), rp[1:] - rp[:-1])
    out = torch.zeros(n, t.shape[1], dtype=D)
    out.index_add_(0, idx, t)
    return out


def node_net_tan_ref(daggr, dx, W1, W2, a1n, a2n):
    """W1 = node_net.0's 128 x 256 weight ([aggr, x] order)."""
    W1 = _d(W1)
    da1 = (_d(daggr) @ W1[:, :128].T + _d(dx) @ W1[:, 128:].T) * (_d(a1n) > 0)
    return (da1 @ _d(W2).T) * (_d(a2n) > 0)


def decoder_tan_ref(da2_prev, a2_prev, g, dx_res, Wd1, a1d, Wd2, std_out=None):
    dx = ln_tan(da2_prev, a2_prev, g)
    if dx_res is not None:
        dx = dx + _d(dx_res)
    dy = ((dx @ _d(Wd1).T) * (_d(a1d) > 0)) @ _d(Wd2).T
    return dy if std_out is None else dy * float(std_out)


def edge_len_tan_ref(src, dst, pos, dpos, edge_attr):
    src, dst = torch.as_tensor(src).cpu().long(), torch.as_tensor(dst).cpu().long()
    pos, dpos, ln = _d(pos), _d(dpos), _d(edge_attr).reshape(-1)
    dot = ((pos[src] - pos[dst]) * (dpos[src] - dpos[dst])).sum(1)
    return torch.where(ln > 0, dot / torch.where(ln > 0, ln, torch.ones_like(ln)), torch.zeros_like(ln))


def epd_tangent(P, stats, pos, mean_stress, nodes_types, edge_index, edge_attr, steps, d_mean_stress, d_pos,
                d_edge_attr, scale_output=True, scale_input=True):
    """(y, dy): the oracle's forward in float64 with every activation kept, then the entry points above composed
    as pdg.engine.EPDEngine.tangent composes the kernels (edges in the caller's order: a permutation of the
    rows changes no sum but the aggregation's order)."""
    from oracle import epd_oracle as O
    P = {k: _d(v) for k, v in P.items()}
    st = {k: _d(v) for k, v in stats.items()}
    pos, ms, ea = _d(pos), _d(mean_stress), _d(edge_attr)
    src, dst = edge_index[0].long(), edge_index[1].long()
    N = pos.shape[0]
    relu = torch.relu
    lin = torch.nn.functional.linear
    x_in, e_in = O.format_inputs(st, pos, ms, nodes_types.to(D), ea, scale_input)

    def mlp(x, name):
        a1 = relu(lin(x, P[f"{name}.0.weight"], P[f"{name}.0.bias"]))
        a2 = relu(lin(a1, P[f"{name}.2.weight"], P[f"{name}.2.bias"]))
        return a1, a2, O.graph_layer_norm(a2, P[f"{name}.4.weight"], P[f"{name}.4.bias"])

    # tangents of the formatted inputs
    dx_in = torch.zeros(N, 6, dtype=D)
    dx_in[:, 0:3] = _d(d_mean_stress) / (st["std_mean_stress"] if scale_input else 1.0)
    dx_in[:, 3:5] = _d(d_pos) / (st["std_pos"] if scale_input else 1.0)
    de_in = _d(d_edge_attr).reshape(-1) / (st["std_edge_weight"] if scale_input else 1.0)

    a1n_, a2n_, x = mlp(x_in, "node_encoder")
    a1e_, a2e_, e = mlp(e_in, "edge_encoder")
    da2n = node_enc_tan_ref(dx_in, a1n_, P["node_encoder.0.weight"], P["node_encoder.2.weight"], a2n_)
    da1e = (de_in.reshape(-1, 1) * P["edge_encoder.0.weight"].reshape(1, -1)) * (a1e_ > 0)
    da2e = (da1e @ P["edge_encoder.2.weight"].T) * (a2e_ > 0)
    ln_n = (a2n_, P["node_encoder.4.weight"])
    ln_e = (a2e_, P["edge_encoder.4.weight"])
    W1e, W2e = P["processor.edge_net.0.weight"], P["processor.edge_net.2.weight"]
    ge, gn = P["processor.edge_net.4.weight"], P["processor.node_net.4.weight"]
    dx_prev = de_prev = None
    rowptr = torch.zeros(N + 1, dtype=torch.long)
    order = torch.argsort(dst, stable=True)
    rowptr[1:] = torch.cumsum(torch.bincount(dst, minlength=N), 0)
    for t in range(steps):
        dx, dP, dQ = node_pre_tan_ref(da2n, ln_n[0], ln_n[1], dx_prev, W1e)
        eu = t < steps - 1
        a1m, a2m, msg = mlp(torch.cat([x[dst], x[src], e], -1), "processor.edge_net")
        a1u = a2u = None
        if eu:
            a1u, a2u, new_e = mlp(torch.cat([x[src], x[dst], e], -1), "processor.edge_net")
        de, da2m, da2e_new = edge_tan_ref(da2e, ln_e[0], ln_e[1], de_prev, src, dst, dP, dQ, W1e, W2e, a1m, a2m,
                                          a1u, a2u)
        aggr = torch.zeros(N, 128, dtype=D).index_add_(0, dst, msg)
        # the kernel's rows are dst-sorted: the same sum in that order
        daggr = segment_sum_tan_ref(rowptr, da2m[order], a2m[order], ge)
        a1n, a2n, upd = mlp(torch.cat([aggr, x], -1), "processor.node_net")
        da2n = node_net_tan_ref(daggr, dx, P["processor.node_net.0.weight"], P["processor.node_net.2.weight"],
                                a1n, a2n)
        ln_n = (a2n, gn)
        if eu:
            ln_e, da2e, e = (a2u, ge), da2e_new, new_e + e
        x = upd + x
        dx_prev, de_prev = dx, de
    a1d = relu(lin(x, P["node_decoder.0.weight"], P["node_decoder.0.bias"]))
    y = lin(a1d, P["node_decoder.2.weight"], P["node_decoder.2.bias"])
    if scale_output:
        y = y * st["std_local_stress"] + st["mean_local_stress"]
    dy = decoder_tan_ref(da2n, ln_n[0], ln_n[1], dx_prev, P["node_decoder.0.weight"], a1d,
                         P["node_decoder.2.weight"], st["std_local_stress"] if scale_output else None)
    return y, dy
