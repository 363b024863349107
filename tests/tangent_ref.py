"""float64 torch restatements of the tangent-pass entry points (csrc/pdg_tangent.hip), one function per entry
point with its operands, and their composition `epd_tangent`, which tests/test_tangent_ref.py anchors to
torch.func.jvp through the oracle.  The GPU op tests hold each kernel to its function here.

Tangents of a forward linearised at stored activations: relu -> mask [a > 0], biases drop out, the graph
LayerNorm y = g (a - mu) / (sigma + eps) + b over all n elements of `a` becomes
  dLN = g ((da - T1 / n) / (sigma + eps) - (a - mu) T2 / (n sigma (sigma + eps)^2)),  T1 = sum da, T2 = sum (a - mu) da.
Weights are nn.Linear (out x in) arrays.

Every entry-point function takes `dtype` (float64: the reference; float32: the plain evaluation of the same closed
form, the yardstick of the per-row checks) and, where it holds a LayerNorm tangent, `totals` = (T1, T2) and `stat`
(a namespace as fwd_ref.ln_stat_ref returns: mean_d, std_d, count and the fp32 fields mean, den): what a consumer
kernel was handed instead of what the arrays themselves give.  Left at None, both come from the arrays in fp64 and
the functions are the ones tests/test_tangent_ref.py anchors to the JVP.  The scalars c1 = T1 / n and c2 are formed
in fp64 in either dtype, as tan_resolve forms them; a float32 evaluation normalises with the fp32 fields.

tan_inputs / seg_tan_inputs / exact_pairs: the inputs of tests/test_gpu_tangent_ops.py, made on the CPU so that
tests/test_tangent_ref.py can show on the same inputs that wrong restatements are far outside the GPU bounds."""
from types import SimpleNamespace

import torch

LN_EPS = 1e-5
D = torch.float64
L = 128


def _d(t, dtype=D):
    return torch.as_tensor(t).detach().cpu().to(dtype)


def _idx(t):
    return torch.as_tensor(t).detach().cpu().long()


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


def stat_of(a):
    """The statistics of the array itself (two-pass, fp64) and the fp32 fields of pdg_ln_stat derived from them."""
    a = _d(a)
    mean_d = float(a.mean())
    std_d = float((a - mean_d).pow(2).mean().sqrt())
    mean, std_ = torch.tensor(mean_d, dtype=D).float(), torch.tensor(std_d, dtype=D).float()
    den = std_ + torch.tensor(LN_EPS, dtype=torch.float32)
    return SimpleNamespace(mean_d=mean_d, std_d=std_d, den_d=std_d + LN_EPS, mean=float(mean), std_=float(std_),
                           den=float(den), rstd=float(torch.tensor(1.0) / den), count=float(a.numel()))


def ln_tan_given(da, a, g=None, totals=None, stat=None, dtype=D):
    """ln_tan with explicit totals (T1, T2) and explicit statistics (mean, std, count): a consumer kernel held to
    exactly what it was handed.  c2 = 0 where std_d is 0 (the kernels' choice for a constant tensor)."""
    if stat is None:
        stat = stat_of(a)
    if totals is None:
        totals = pairs_ref(da, a, stat.mean_d)
    n, sd = float(stat.count), float(stat.std_d)
    c1 = float(totals[0]) / n
    c2 = float(totals[1]) / (n * sd * (sd + LN_EPS) ** 2) if sd > 0 else 0.0
    da, a = _d(da, dtype), _d(a, dtype)
    if dtype == D:
        out = (da - c1) / getattr(stat, "den_d", sd + LN_EPS) - (a - stat.mean_d) * c2
    else:
        t = lambda v: torch.tensor(v, dtype=D).to(dtype)
        out = (da - t(c1)) / t(stat.den) - (a - t(stat.mean)) * t(c2)
    return out if g is None else out * _d(g, dtype)


def pairs_ref(da, a, mean=None):
    """(T1, T2) of a pre-LayerNorm tangent (mean None: the array's own)."""
    da, a = _d(da), _d(a)
    return da.sum(), ((a - (a.mean() if mean is None else mean)) * da).sum()


def _ln_res(da, a, g, res, totals, stat, dtype):
    x = ln_tan_given(da, a, g, totals, stat, dtype)
    return x if res is None else x + _d(res, dtype)


def node_enc_tan_ref(dx_in, a1, W0, W2, a2, dtype=D):
    da1 = (_d(dx_in, dtype) @ _d(W0, dtype).T) * (_d(a1) > 0)
    return (da1 @ _d(W2, dtype).T) * (_d(a2) > 0)


def edge_enc_tan_ref(de_in, e_in, w0, b0, W2, a2, dtype=D):
    """The first layer's sign as the kernels recompute it in fp32: fma(w0, e, 0) + b0 > 0."""
    e32, w32, b32 = (torch.as_tensor(t).detach().cpu().float().reshape(-1) for t in (e_in, w0, b0))
    m1 = (e32[:, None] * w32[None, :] + b32[None, :]) > 0
    da1 = (_d(de_in, dtype).reshape(-1, 1) * _d(w0, dtype).reshape(1, -1)) * m1
    return (da1 @ _d(W2, dtype).T) * (_d(a2) > 0)


def node_pre_tan_ref(da2_prev, a2_prev, g, dx_res, W1, dtype=D, totals=None, stat=None):
    """(dx_t, dP, dQ); W1 = edge_net.0's 128 x 384 weight."""
    dx = _ln_res(da2_prev, a2_prev, g, dx_res, totals, stat, dtype)
    W1 = _d(W1, dtype)
    return dx, dx @ W1[:, :128].T, dx @ W1[:, 128:256].T


def edge_tan_ref(da2_prev, a2_prev, g, de_res, src, dst, dP, dQ, W1, W2, a1m, a2m, a1e=None, a2e=None, dtype=D,
                 totals=None, stat=None):
    """(de_t, da2m, da2e or None)."""
    de = _ln_res(da2_prev, a2_prev, g, de_res, totals, stat, dtype)
    src, dst = _idx(src), _idx(dst)
    W1, W2, dP, dQ = _d(W1, dtype), _d(W2, dtype), _d(dP, dtype), _d(dQ, dtype)
    C = de @ W1[:, 256:].T
    da2m = (((C + dP[dst] + dQ[src]) * (_d(a1m) > 0)) @ W2.T) * (_d(a2m) > 0)
    da2e = None
    if a1e is not None:
        da2e = (((C + dP[src] + dQ[dst]) * (_d(a1e) > 0)) @ W2.T) * (_d(a2e) > 0)
    return de, da2m, da2e


def segment_sum_tan_ref(rowptr, da2m, a2m, g, dtype=D, totals=None, stat=None):
    """g x the sum over a node's rows of dLN without the weight, row after row in edge order in `dtype` (the
    kernel's order: in float32 the yardstick of a long row)."""
    t = ln_tan_given(da2m, a2m, None, totals, stat, dtype)
    rp = _idx(rowptr)
    n, deg = rp.numel() - 1, rp[1:] - rp[:-1]
    out = torch.zeros(n, t.shape[1], dtype=dtype)
    for j in range(int(deg.max()) if n else 0):
        live = deg > j
        out[live] = out[live] + t[rp[:-1][live] + j]
    return out * _d(g, dtype)


def node_net_tan_ref(daggr, dx, W1, W2, a1n, a2n, dtype=D):
    """W1 = node_net.0's 128 x 256 weight ([aggr, x] order)."""
    W1 = _d(W1, dtype)
    da1 = (_d(daggr, dtype) @ W1[:, :128].T + _d(dx, dtype) @ W1[:, 128:].T) * (_d(a1n) > 0)
    return (da1 @ _d(W2, dtype).T) * (_d(a2n) > 0)


def decoder_tan_ref(da2_prev, a2_prev, g, dx_res, Wd1, a1d, Wd2, std_out=None, dtype=D, totals=None, stat=None):
    dx = _ln_res(da2_prev, a2_prev, g, dx_res, totals, stat, dtype)
    dy = ((dx @ _d(Wd1, dtype).T) * (_d(a1d) > 0)) @ _d(Wd2, dtype).T
    return dy if std_out is None else dy * _d(std_out, dtype).reshape(())


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


# ---------------------------------------------------------------- the inputs of the GPU op tests (CPU, fp32 / int64)

TOL = 3e-6        # relative L2 of a tangent kernel's output against fp64 at sigma ~ 0.6 (the bf16x6 op tests' order)
TOL_LN = 1e-5     # the forward tier's bound downstream of a small-std LayerNorm: the fp32 restatement stays below it
ROW_FACTOR = 4    # kernel <= ROW_FACTOR x the fp32 restatement, both against fp64 (the other tiers' margin)
CONDS = {"p": 1.0, "c": 2e-4}   # scale of the producer's second layer: sigma ~ 0.6 / sigma ~ 5e-5 (eps counts in den)
NN = 53           # nodes of the edge cases
EXACT_K = 2       # the integer-exact family's c1


def _rn(g):
    return lambda *s, shift=0.0: (torch.randn(*s, generator=g, dtype=D) + shift).float()


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _sparse_rows(g, rows, cols, nnz, lo, hi):
    W = torch.zeros(rows, cols)
    for r in range(rows):
        W[r, torch.randperm(cols, generator=g)[:nnz]] = _ints(g, lo, hi, nnz)
    return W


def _produce(g, rows, cond, const=None):
    """The real producer's inputs (a1p, W2p, b2p) and its fp64 output rounded to fp32: a2 = relu(W2p a1p + b2p).
    const: W2p = 0 and b2p = const, a constant tensor."""
    a1p = torch.relu(_rn(g)(rows, L))
    if const is not None:
        W2p, b2p = torch.zeros(L, L), torch.full((L,), float(const))
    else:
        W2p = ((torch.rand(L, L, generator=g) * 2 - 1) / L ** 0.5 * CONDS[cond]).contiguous()
        b2p = (((torch.rand(L, generator=g) * 2 - 1) / L ** 0.5 + 0.1) * CONDS[cond]).contiguous()
    a2 = torch.relu(a1p.double() @ W2p.double().T + b2p.double()).float()
    return SimpleNamespace(a1p=a1p, W2p=W2p, b2p=b2p, a2=a2)


def ends_edges(g, M, nn=NN):
    """M dst-sorted edges over nn nodes, the last three nodes without an incoming edge but for the last edge; node 0
    and node nn - 1 each occur as a src and as a dst (M >= 2)."""
    dst = torch.sort(torch.randint(0, nn - 3, (M,), generator=g)).values
    src = torch.randint(0, nn, (M,), generator=g)
    if M >= 2:
        dst[0], dst[-1], src[0], src[-1] = 0, nn - 1, nn - 1, 0
    return src, dst


def tan_inputs(M, cond):
    """The operands of the six row kernels at M rows.  cond "p" / "c": the randn family; the LayerNorm inputs a_prev
    (consumers), a2 and a2b (producers: masks and T2) are the producer's outputs (`prod_*`: its inputs); the tangent
    da_prev has a mean of 0.7 and a component 0.5 (a - mu) / sigma, so both LayerNorm terms matter at either sigma;
    in "c" everything added to a LayerNorm tangent (residual, dP, dQ) is scaled by 1 / sigma as well, so that it
    still counts.  cond "x": the integer-exact family, operands and tangents in -4 .. 4, weights in -2 .. 2 (W2 with
    8 entries of -1 .. 1 per row), g in {-1, 1, 2}, to go with unit statistics and the totals (n EXACT_K, 0): |dx| <=
    6 x 2 + 4 = 16, |dP| <= 128 x 16 x 2 = 4096, |da1| <= 4096 + 8, |da2| <= 8 x 4104, |dy| <= 128 x 4096 x 2 = 2^20,
    a row pair sum of T2 <= 4 x 4 x 32832 < 2^20: every fp32 sum is an integer below 2^24."""
    g = torch.Generator().manual_seed(9300 + 3 * M + {"p": 0, "c": 1, "x": 2}[cond])
    r = SimpleNamespace(M=M, cond=cond, NN=NN)
    r.src, r.dst = ends_edges(g, M)
    if cond == "x":
        it = lambda lo, hi, *s: _ints(g, lo, hi, *s)
        r.W0n, r.w0e, r.b0e = it(-2, 2, L, 6), it(-2, 2, L), it(-2, 2, L)
        r.W2, r.We1, r.Wn1 = _sparse_rows(g, L, L, 8, -1, 1), it(-2, 2, L, 3 * L), it(-2, 2, L, 2 * L)
        r.Wd1, r.Wd2 = it(-2, 2, L, L), it(-2, 2, 3, L)
        r.g = torch.tensor([-1.0, 1.0, 2.0])[torch.randint(0, 3, (L,), generator=g)]
        for k in ("a1", "a2", "a1b", "a2b", "a_prev", "da_prev", "res", "rows2"):
            setattr(r, k, it(-4, 4, M, L))
        r.dx_in, r.de_in, r.e_in = it(-4, 4, M, 6), it(-4, 4, M), it(-4, 4, M)
        r.dP, r.dQ = it(-4, 4, NN, L), it(-4, 4, NN, L)
        r.std_out = 2.0
        return r
    rn = _rn(g)
    lin = lambda o, i: (rn(o, i) / i ** 0.5).contiguous()
    r.W0n, r.w0e, r.b0e = lin(L, 6), rn(L), rn(L) * 0.5
    r.W2, r.We1, r.Wn1, r.Wd1, r.Wd2 = lin(L, L), lin(L, 3 * L), lin(L, 2 * L), lin(L, L), lin(3, L)
    r.g = rn(L) * 0.3 + 1.0
    r.a1, r.a1b = torch.relu(rn(M, L, shift=0.3)), torch.relu(rn(M, L, shift=0.3))
    r.prod_prev, r.prod_a2, r.prod_a2b = (_produce(g, M, cond) for _ in range(3))
    r.a_prev, r.a2, r.a2b = r.prod_prev.a2, r.prod_a2.a2, r.prod_a2b.a2
    st = stat_of(r.a_prev)
    xc = r.a_prev.double() - st.mean_d
    up = 1.0 / st.std_d if cond == "c" else 1.0
    r.da_prev = (rn(M, L, shift=0.7).double() + 0.5 * xc / max(st.std_d, 1e-300)).float()
    r.res, r.rows2 = (rn(M, L).double() * up).float(), rn(M, L)
    r.dx_in, r.de_in, r.e_in = rn(M, 6), rn(M), rn(M)
    r.dP, r.dQ = (rn(NN, L).double() * up).float(), (rn(NN, L).double() * up).float()
    r.std_out = 2.75
    return r


def seg_degrees(N):
    """In-degrees 0, 1, 7, 8, 9, 16, 17 and a hub of 300, then a filler pattern; the first and the last node empty."""
    return [0, 1, 7, 8, 9, 16, 17, 300] + [(3 * v) % 11 for v in range(N - 9)] + [0]


def seg_tan_inputs(N, cond):
    """The hand-built CSR of seg_degrees(N) and the rows to sum (as tan_inputs' a_prev / da_prev)."""
    deg = torch.tensor(seg_degrees(N))
    r = SimpleNamespace(N=N, E=int(deg.sum()), deg=deg, cond=cond)
    r.rowptr = torch.zeros(N + 1, dtype=torch.int64)
    r.rowptr[1:] = torch.cumsum(deg, 0)
    g = torch.Generator().manual_seed(9400 + 3 * N + {"p": 0, "c": 1, "x": 2}[cond])
    if cond == "x":
        r.a_prev, r.da_prev = _ints(g, -4, 4, r.E, L), _ints(g, -4, 4, r.E, L)
        r.g = torch.tensor([-1.0, 1.0, 2.0])[torch.randint(0, 3, (L,), generator=g)]
        return r
    rn = _rn(g)
    r.prod_prev = _produce(g, r.E, cond)
    r.a_prev = r.prod_prev.a2
    st = stat_of(r.a_prev)
    r.da_prev = (rn(r.E, L, shift=0.7).double() + 0.5 * (r.a_prev.double() - st.mean_d) / st.std_d).float()
    r.g = rn(L) * 0.3 + 1.0
    return r


def split_totals(t1, t2, npairs, seed=0):
    """(T1, T2) split unevenly over npairs pairs, interleaved (2 npairs doubles)."""
    g = torch.Generator().manual_seed(9500 + npairs + seed)
    w = torch.rand(npairs, dtype=D, generator=g) + 0.1
    w = w / w.sum()
    return torch.stack([float(t1) * w, float(t2) * w], 1).reshape(-1)


def exact_pairs(n, npairs, k=EXACT_K):
    """Integer pairs: T1 pieces that total n k, T2 pieces that cancel to exactly 0; every piece non-zero where
    npairs > 1, so a pair that is left out or counted twice changes c1 or c2."""
    g = torch.Generator().manual_seed(9600 + npairs)
    p1 = torch.randint(1, 50, (npairs,), generator=g).double()
    p2 = torch.randint(1, 50, (npairs,), generator=g).double()
    p1[-1] += n * k - p1.sum()
    p2[-1] -= p2.sum()
    if npairs > 1:
        assert float(p1[-1]) != 0 and float(p2[-1]) != 0
    assert float(p1.sum()) == n * k and float(p2.sum()) == 0.0
    return torch.stack([p1, p2], 1).reshape(-1)


def unit_stat(n):
    """mean 0, den = 1.0f, rstd = 1, count = n: the hand-packed statistics of the integer-exact family (std_d = 1:
    c2 is 0 through T2 = 0, not through the constant-tensor branch)."""
    return SimpleNamespace(mean=0.0, den=1.0, rstd=1.0, std_=1.0, mean_d=0.0, std_d=1.0, den_d=1.0, count=float(n))


def chain_inputs(E=600):
    """Two message-passing steps on edge_bwd_ref.hub_graph(E) (a hub run, edge-free nodes, dst-sorted): the
    parameters, the formatted inputs, their tangents and every activation the tangent pass reads, from the fp64
    forward of tests/fwd_ref.py rounded to fp32 (the kernels and the references linearise at the same arrays)."""
    import fwd_ref as F
    from edge_bwd_ref import hub_graph
    from oracle import epd_oracle as O
    N, src, dst, rp = hub_graph(E)[:4]
    g = torch.Generator().manual_seed(9700 + E)
    prm = {k: v.float() for k, v in O.init_params(seed=11).items()}
    for k in prm:
        if k.endswith(".4.weight") or k.endswith(".4.bias"):
            prm[k] = prm[k] + 0.2 * torch.randn(L, generator=g)
    c = SimpleNamespace(N=N, E=E, src=src, dst=dst, rowptr=rp, prm=prm, std_out=3.5)
    c.x_in, c.e_in = torch.randn(N, 6, generator=g), torch.randn(E, 1, generator=g)
    c.dx_in, c.de_in = torch.randn(N, 6, generator=g), torch.randn(E, generator=g)
    f = lambda t: t.float().contiguous()
    c.a1ne, c.a2ne = map(f, F.mlp_ref(c.x_in, *(prm[f"node_encoder.{i}"] for i in ("0.weight", "0.bias", "2.weight", "2.bias"))))
    c.a1ee, c.a2ee = map(f, F.mlp_ref(c.e_in, *(prm[f"edge_encoder.{i}"] for i in ("0.weight", "0.bias", "2.weight", "2.bias"))))
    _, steps, dec = F.forward_ref(prm, c.x_in, c.e_in, src, dst, 2)
    c.steps = [SimpleNamespace(**{k: f(getattr(s, k)) for k in ("a1m", "a2m", "a1n", "a2n") + (("a1e", "a2e") if s.eu else ())},
                               eu=s.eu) for s in steps]
    c.a1d = f(dec.a1d)
    return c


def chain_ref(c, dtype=D):
    """The entry points composed in the engine's order (pdg.engine.EPDEngine.tangent) on chain_inputs, every
    LayerNorm's statistics and totals from its own arrays."""
    p = c.prm
    da2n = node_enc_tan_ref(c.dx_in, c.a1ne, p["node_encoder.0.weight"], p["node_encoder.2.weight"], c.a2ne, dtype)
    da2e = edge_enc_tan_ref(c.de_in, c.e_in, p["edge_encoder.0.weight"], p["edge_encoder.0.bias"],
                            p["edge_encoder.2.weight"], c.a2ee, dtype)
    W1e, W2e = p["processor.edge_net.0.weight"], p["processor.edge_net.2.weight"]
    g_e, g_n = p["processor.edge_net.4.weight"], p["processor.node_net.4.weight"]
    ln_n, ln_e = (c.a2ne, p["node_encoder.4.weight"]), (c.a2ee, p["edge_encoder.4.weight"])
    dx_prev = de_prev = None
    for s in c.steps:
        dx, dP, dQ = node_pre_tan_ref(da2n, ln_n[0], ln_n[1], dx_prev, W1e, dtype)
        de, da2m, da2e_new = edge_tan_ref(da2e, ln_e[0], ln_e[1], de_prev, c.src, c.dst, dP, dQ, W1e, W2e, s.a1m, s.a2m,
                                          s.a1e if s.eu else None, s.a2e if s.eu else None, dtype)
        daggr = segment_sum_tan_ref(c.rowptr, da2m, s.a2m, g_e, dtype)
        da2n = node_net_tan_ref(daggr, dx, p["processor.node_net.0.weight"], p["processor.node_net.2.weight"], s.a1n,
                                s.a2n, dtype)
        ln_n = (s.a2n, g_n)
        if s.eu:
            ln_e, da2e = (s.a2e, g_e), da2e_new
        dx_prev, de_prev = dx, de
    return decoder_tan_ref(da2n, ln_n[0], ln_n[1], dx_prev, p["node_decoder.0.weight"], c.a1d,
                           p["node_decoder.2.weight"], c.std_out, dtype)
