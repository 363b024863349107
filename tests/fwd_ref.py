"""Plain torch restatement of the per-step forward (what pdg_node_pq_rw[_fin], pdg_edge_fwd_coop, pdg_edge_fwd_infer,
pdg_segment_sum[_fin], pdg_node_net, pdg_decoder_fwd_coop and pdg_ln_finalize[2] compute, include/pdivgnn.h), on the
CPU in the dtype of the caller's choice (float64: the reference; float32: the yardstick of the per-row check).
tests/test_fwd_ref.py anchors the closed forms to oracle.epd_oracle (_mlp, processor_step, graph_layer_norm);
tests/test_gpu_fwd.py holds the kernels to them.

A LayerNorm's statistics travel as the namespace ln_stat_ref returns: the fp64 pair (mean_d, std_d), den_d = std_d +
eps, and the four fp32 fields of pdg_ln_stat as the header defines them.  A float64 form normalises with (mean_d,
den_d), a float32 form with the fp32 fields (mean, den).  UNIT (mean 0, den = rstd = 1) is the hand-packed statistic
of the integer-exact inputs.  Weights are the model's arrays (out x in, row-major): W1 = processor.edge_net.0.weight
(128 x 384) = [Wa | Wb | Wc], Wn1 = processor.node_net.0.weight (128 x 256) = [Wn1a | Wn1b]."""
from __future__ import annotations

from types import SimpleNamespace

import torch

from edge_bwd_ref import L, LN_EPS

EPS32 = torch.tensor(LN_EPS, dtype=torch.float32)   # 1e-5f


def _c(dtype, *ts):
    return [None if t is None else t.detach().to("cpu", dtype) for t in ts]


def fp32_fields(mean_d: float, std_d: float):
    """The fp32 fields of pdg_ln_stat from its fp64 pair: mean = fp32(mean_d), std_ = fp32(std_d), den = std_ +
    1e-5f and rstd = 1 / den, both in fp32 arithmetic.  Python floats holding the fp32 values."""
    mean = torch.tensor(mean_d, dtype=torch.float64).float()
    std_ = torch.tensor(std_d, dtype=torch.float64).float()
    den = std_ + EPS32
    rstd = torch.tensor(1.0, dtype=torch.float32) / den
    return float(mean), float(std_), float(den), float(rstd)


def ln_stat_ref(a, eps=LN_EPS):
    """Graph-LayerNorm statistics of the array itself: mean and population std over all elements, two-pass in
    fp64, and the fp32 fields derived from them."""
    a = a.detach().to("cpu", torch.float64)
    mean_d = float(a.mean())
    std_d = float((a - mean_d).pow(2).mean().sqrt())
    mean, std_, den, rstd = fp32_fields(mean_d, std_d)
    return SimpleNamespace(mean_d=mean_d, std_d=std_d, den_d=std_d + eps, mean=mean, std_=std_, den=den, rstd=rstd,
                           count=float(a.numel()))


UNIT = SimpleNamespace(mean_d=0.0, std_d=1.0, den_d=1.0, mean=0.0, std_=1.0, den=1.0, rstd=1.0, count=0.0)


def _norm(a2, stat, dtype):
    if dtype == torch.float64:
        return (a2 - stat.mean_d) / stat.den_d
    return (a2 - torch.tensor(stat.mean, dtype=dtype)) / torch.tensor(stat.den, dtype=dtype)


def ln_res_ref(a2, stat, g, b, res=None, dtype=torch.float64):
    """(a2 - mean) / den * g + b [+ res]."""
    a2, g, b, res = _c(dtype, a2, g, b, res)
    y = _norm(a2, stat, dtype) * g + b
    return y if res is None else y + res


def mlp_ref(x, W0, b0, W2, b2, dtype=torch.float64):
    """An encoder's two layers: a1 = relu(W0 x + b0), a2 = relu(W2 a1 + b2)."""
    x, W0, b0, W2, b2 = _c(dtype, x, W0, b0, W2, b2)
    a1 = torch.relu(x @ W0.T + b0)
    return a1, torch.relu(a1 @ W2.T + b2)


def node_pq_ref(a2n, stat, g, b, x_res, W1, dtype=torch.float64):
    """x_t = LN(a2n) [+ x_res]; P = x_t Wa^T, Q = x_t Wb^T (Wa, Wb: the first two column blocks of W1)."""
    W1, = _c(dtype, W1)
    r = SimpleNamespace(x_t=ln_res_ref(a2n, stat, g, b, x_res, dtype))
    r.P = r.x_t @ W1[:, :L].T
    r.Q = r.x_t @ W1[:, L:2 * L].T
    return r


def edge_step_ref(a2_prev, stat, g, b, e_res, src, dst, P, Q, W1, b1, W2, b2, eu=True, dtype=torch.float64):
    """e_t = LN(a2_prev) [+ e_res]; C = e_t Wc^T + b1; message a1m = relu(C + P[dst] + Q[src]), edge update a1e =
    relu(C + P[src] + Q[dst]); a2* = relu(a1* W2^T + b2); sums_* = (sum, sum of squares) of a2*."""
    P, Q, W1, b1, W2, b2 = _c(dtype, P, Q, W1, b1, W2, b2)
    src, dst = src.detach().cpu().long(), dst.detach().cpu().long()
    r = SimpleNamespace(eu=bool(eu), e_t=ln_res_ref(a2_prev, stat, g, b, e_res, dtype))
    C = r.e_t @ W1[:, 2 * L:].T + b1
    r.a1m = torch.relu(C + P[dst] + Q[src])
    r.a2m = torch.relu(r.a1m @ W2.T + b2)
    r.sums_m = (r.a2m.sum(), r.a2m.pow(2).sum())
    if eu:
        r.a1e = torch.relu(C + P[src] + Q[dst])
        r.a2e = torch.relu(r.a1e @ W2.T + b2)
        r.sums_e = (r.a2e.sum(), r.a2e.pow(2).sum())
    return r


def segment_sum_ref(dst, rows, stat, g, b, N, dtype=torch.float64):
    """aggr[v] = sum over the rows k with dst[k] = v of LN(rows[k]) (stat None: of rows[k]) and xhat_sum[v], the
    same sum of (rows[k] - mean) / den; rows in CSR (dst-sorted) order.  Returns (aggr, xhat_sum or None)."""
    rows, g, b = _c(dtype, rows, g, b)
    dst = dst.detach().cpu().long()
    zero = torch.zeros(N, rows.shape[1], dtype=dtype)
    if stat is None:
        return zero.index_add_(0, dst, rows), None
    xhat = _norm(rows, stat, dtype)
    return zero.clone().index_add_(0, dst, xhat * g + b), zero.index_add_(0, dst, xhat)


def node_net_ref(aggr, x, Wn1, bn1, Wn2, bn2, dtype=torch.float64):
    """a1n = relu(Wn1 [aggr | x] + bn1); a2n = relu(Wn2 a1n + bn2)."""
    aggr, x, Wn1, bn1, Wn2, bn2 = _c(dtype, aggr, x, Wn1, bn1, Wn2, bn2)
    a1n = torch.relu(torch.cat([aggr, x], 1) @ Wn1.T + bn1)
    return a1n, torch.relu(a1n @ Wn2.T + bn2)


def decoder_ref(a2n, stat, g, b, x_res, Wd1, bd1, Wd2, bd2, stats8=None, scale_output=False, dtype=torch.float64):
    """x_S = LN(a2n) + x_res; a1d = relu(Wd1 x_S + bd1); y = Wd2 a1d + bd2; scale_output: y = y std_local_stress +
    mean_local_stress (stats8[5], stats8[4])."""
    Wd1, bd1, Wd2, bd2, stats8 = _c(dtype, Wd1, bd1, Wd2, bd2, stats8)
    r = SimpleNamespace(x_S=ln_res_ref(a2n, stat, g, b, x_res, dtype))
    r.a1d = torch.relu(r.x_S @ Wd1.T + bd1)
    r.y = r.a1d @ Wd2.T + bd2
    if scale_output:
        r.y = r.y * stats8[5] + stats8[4]
    return r


def step_ref(p, a2n_prev, ln_n, x_res, a2e_prev, ln_e, e_res, src, dst, eu=True, dtype=torch.float64):
    """One message-passing step as the engine splits it, from the previous node / edge second-layer outputs:
    ln_n / ln_e are the (weight, bias) of the LayerNorms that normalise a2n_prev / a2e_prev (the encoders' at step
    0, with x_res = e_res = None; node_net's / edge_net's later); every statistic is taken from the array itself.
    p: the model's parameters by name.  The step's x (= r.x_t) and e (= r.e_t) are what oracle.epd_oracle's
    processor_step takes; its outputs are the next step's x_t / e_t."""
    N = a2n_prev.shape[0]
    ge, be = p["processor.edge_net.4.weight"], p["processor.edge_net.4.bias"]
    st_n_prev = ln_stat_ref(a2n_prev)
    r = node_pq_ref(a2n_prev, st_n_prev, *ln_n, x_res, p["processor.edge_net.0.weight"], dtype)
    r.st_n_prev, r.st_e_prev = st_n_prev, ln_stat_ref(a2e_prev)
    ed = edge_step_ref(a2e_prev, r.st_e_prev, *ln_e, e_res, src, dst, r.P, r.Q, p["processor.edge_net.0.weight"],
                       p["processor.edge_net.0.bias"], p["processor.edge_net.2.weight"],
                       p["processor.edge_net.2.bias"], eu, dtype)
    r.__dict__.update(ed.__dict__)
    r.st_m = ln_stat_ref(r.a2m)
    r.st_e = ln_stat_ref(r.a2e) if eu else None
    r.aggr, r.xs = segment_sum_ref(dst, r.a2m, r.st_m, ge, be, N, dtype)
    r.a1n, r.a2n = node_net_ref(r.aggr, r.x_t, p["processor.node_net.0.weight"], p["processor.node_net.0.bias"],
                                p["processor.node_net.2.weight"], p["processor.node_net.2.bias"], dtype)
    r.st_n = ln_stat_ref(r.a2n)
    return r


def forward_ref(p, x_in, e_in, src, dst, steps, stats8=None, scale_output=False, dtype=torch.float64):
    """The encoders, `steps` message-passing steps (the last without the edge update) and the decoder, from the
    formatted inputs x_in (N x 6) and e_in (E x 1).  Returns (the encoders' a2 pair, the steps' namespaces, the
    decoder's)."""
    _, a2n = mlp_ref(x_in, p["node_encoder.0.weight"], p["node_encoder.0.bias"], p["node_encoder.2.weight"],
                     p["node_encoder.2.bias"], dtype)
    _, a2e = mlp_ref(e_in, p["edge_encoder.0.weight"], p["edge_encoder.0.bias"], p["edge_encoder.2.weight"],
                     p["edge_encoder.2.bias"], dtype)
    enc = SimpleNamespace(a2n=a2n, a2e=a2e)
    ln_n = (p["node_encoder.4.weight"], p["node_encoder.4.bias"])
    ln_e = (p["edge_encoder.4.weight"], p["edge_encoder.4.bias"])
    x_res = e_res = None
    out = []
    for t in range(steps):
        r = step_ref(p, a2n, ln_n, x_res, a2e, ln_e, e_res, src, dst, t < steps - 1, dtype)
        out.append(r)
        x_res, e_res, a2n = r.x_t, r.e_t, r.a2n
        a2e = r.a2e if r.eu else None
        ln_n = (p["processor.node_net.4.weight"], p["processor.node_net.4.bias"])
        ln_e = (p["processor.edge_net.4.weight"], p["processor.edge_net.4.bias"])
    dec = decoder_ref(a2n, ln_stat_ref(a2n), *ln_n, x_res, p["node_decoder.0.weight"], p["node_decoder.0.bias"],
                      p["node_decoder.2.weight"], p["node_decoder.2.bias"], stats8, scale_output, dtype)
    dec.st_n = ln_stat_ref(a2n)
    return enc, out, dec


# ---------------------------------------------------------------- the inputs of the op tests (CPU, fp32 / int64)

# the bounds tests/test_gpu_fwd.py applies (tests/test_fwd_ref.py shows that its inputs tell the closed forms from
# wrong ones at 1000 x these)
TOL = 2e-6        # relative L2 of one fp32 / bf16x6 product of given inputs against fp64 (tests/test_gpu_ops.py)
TOL_LN = 1e-5     # the same downstream of a small-std LayerNorm (tests/test_gpu_node_bwd.py)
TOL_STAT = 1e-9   # mean_d (relative to the rms) and std_d (relative) from exact fp64 partials
CONDS = {"p": 1.0, "c": 2e-4}   # scale of the producer's second layer: std ~ 0.6 / std ~ 5e-5 (eps counts in den)


def ends_graph(E, seed=0):
    """A dst-sorted edge list in which node 0 and node N - 1 each occur as a src and as a dst (an off-by-one in a
    gathered row index then reads the row before P / Q or the one after).  Returns (N, src, dst), int64."""
    if E == 1:
        return 1, torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64)
    g = torch.Generator().manual_seed(2000 + 11 * E + seed)
    N = 2 + E // 6
    dst = torch.sort(torch.randint(0, N, (E,), generator=g)).values
    src = torch.randint(0, N, (E,), generator=g)
    dst[0], dst[-1], src[0], src[-1] = 0, N - 1, N - 1, 0
    return N, src, dst


def graph_of(kind, E):
    """(N, src, dst) of the hub graph (edge_bwd_ref.hub_graph) or the ends graph."""
    from edge_bwd_ref import hub_graph
    if kind == "ends":
        return ends_graph(E)
    N, src, dst = hub_graph(E)[:3]
    return N, src, dst


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _sparse_rows(g, rows, cols, nnz, lo, hi):
    """rows x cols integers in lo .. hi with exactly nnz entries per row drawn (some of them zero)."""
    W = torch.zeros(rows, cols)
    for r in range(rows):
        W[r, torch.randperm(cols, generator=g)[:nnz]] = _ints(g, lo, hi, nnz)
    return W


def exact_edge_inputs(E, N, seed=0):
    """The integer-exact family of the edge kernels: a2_prev, e_res, P, Q in -4 .. 4, Wc in -2 .. 2 and W2 in -1 ..
    1 with 8 entries per row, biases in -2 .. 2, to go with UNIT statistics, g = 1, b = 0.  Then |e_t| <= 8, |C| <=
    8 * 2 * 8 + 2 = 130, a1 <= 138, a2 <= 8 * 138 + 2 = 1106 < 2^11: every operand is an integer of one to three
    bf16 terms, every weight one bf16 term, every fp32 partial sum an integer below 2^24, and the LayerNorm
    partials' fp32 sums of four squares stay below 2^23: the kernels' results are exact."""
    g = torch.Generator().manual_seed(3000 + E + seed)
    W1 = torch.cat([_ints(g, -2, 2, L, 2 * L), _sparse_rows(g, L, L, 8, -2, 2)], 1)
    return SimpleNamespace(a2_prev=_ints(g, -4, 4, E, L), e_res=_ints(g, -4, 4, E, L), P=_ints(g, -4, 4, N, L),
                           Q=_ints(g, -4, 4, N, L), W1=W1, b1=_ints(g, -2, 2, L),
                           W2=_sparse_rows(g, L, L, 8, -1, 1), b2=_ints(g, -2, 2, L), g=torch.ones(L), b=torch.zeros(L))


def randn_edge_inputs(E, N, cond, seed=0):
    """The randn family: a2_prev = relu(W2p a1p + b2p) with the producer's weights scaled by CONDS[cond] (the GPU
    test takes a2_prev and its statistics from the real producer on a1p, W2p, b2p; `a2_prev` here is the fp64
    product rounded to fp32), the residual, P, Q randn, the step's weights as torch.nn.Linear draws them."""
    g = torch.Generator().manual_seed(4000 + E + seed + (7 if cond == "c" else 0))
    rn, lin = _rn(g), lambda o, i: _lin(g, o, i)
    r = SimpleNamespace(a1p=torch.relu(rn(E, L)))
    W2p, b2p = lin(L, L)
    r.W2p, r.b2p = (W2p * CONDS[cond]).contiguous(), (b2p * CONDS[cond]).contiguous()
    r.a2_prev = torch.relu(r.a1p.double() @ r.W2p.double().T + r.b2p.double()).float()
    r.e_res, r.P, r.Q = rn(E, L), rn(N, L), rn(N, L)
    r.W1, r.b1 = lin(L, 3 * L)
    r.W2, r.b2 = lin(L, L)
    r.g, r.b = rn(L) * 0.3 + 1.0, rn(L) * 0.1
    return r


# ---------------------------------------------------------------- the node, segment-sum and statistics inputs

STATS8 = torch.tensor([0.1, 1.2, -0.3, 2.0, 0.25, 3.5, 0.05, 0.7])


def _lin(g, o, i):
    """Weight and bias as torch.nn.Linear draws them (the bias moved off zero mean)."""
    return (torch.rand(o, i, generator=g) * 2 - 1) / i ** 0.5, (torch.rand(o, generator=g) * 2 - 1) / i ** 0.5 + 0.1


def _rn(g):
    return lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float()


def _produce(r, cond, g, rows):
    """The real producer's inputs a1p, W2p, b2p (scaled by CONDS[cond]) and its fp64 output rounded to fp32."""
    r.a1p = torch.relu(_rn(g)(rows, L))
    W2p, b2p = _lin(g, L, L)
    r.W2p, r.b2p = (W2p * CONDS[cond]).contiguous(), (b2p * CONDS[cond]).contiguous()
    return torch.relu(r.a1p.double() @ r.W2p.double().T + r.b2p.double()).float()


def node_inputs(N, cond):
    """The inputs of the node pre-pass and the decoder.  cond "x": the integer-exact family, a2n, x_res in -4 .. 4,
    weights and biases in -2 .. 2, g = 1, b = 0 (|x| <= 8, |P| <= 128 * 8 * 2, a1d <= 128 * 8 * 2 + 2 = 2050, |y| <= 128 *
    2050 * 2 + 2 < 2^24: all exact).  "p" / "c": a2n from the producer (as randn_edge_inputs), the rest randn / Linear."""
    g = torch.Generator().manual_seed(7000 + N + (3 if cond == "c" else 0))
    r = SimpleNamespace(N=N, stats8=STATS8)
    if cond == "x":
        it = lambda lo, hi, *s: _ints(g, lo, hi, *s)
        r.a2n, r.x_res, r.g, r.b = it(-4, 4, N, L), it(-4, 4, N, L), torch.ones(L), torch.zeros(L)
        r.W1 = it(-2, 2, L, 3 * L)
        r.Wd1, r.bd1, r.Wd2, r.bd2 = it(-2, 2, L, L), it(-2, 2, L), it(-2, 2, 3, L), it(-2, 2, 3)
        return r
    rn = _rn(g)
    r.a2n = _produce(r, cond, g, N)
    r.x_res, r.g, r.b = rn(N, L), rn(L) * 0.3 + 1.0, rn(L) * 0.1
    r.W1 = _lin(g, L, 3 * L)[0]
    (r.Wd1, r.bd1), (r.Wd2, r.bd2) = _lin(g, L, L), _lin(g, 3, L)
    return r


def seg_degrees(N):
    """In-degrees around SEG_U = 8 (0, 1, 7, 8, 9, 16, 17), a hub of 300, the first and the last node without an edge.
    N > 77: in-degrees 1 - 2 (the grid-stride case)."""
    if N == 1:
        return [0]
    if N == 8:
        return [0, 1, 7, 8, 9, 17, 300, 0]
    head = [0, 1, 7, 8, 9, 16, 17, 300]
    if N <= 77:
        return head + [(3 * v) % 11 for v in range(N - 9)] + [0]
    return [0] + [1 + v % 2 for v in range(N - 2)] + [0]


def seg_inputs(N, cond):
    """The hand-built CSR of seg_degrees(N) (deg, dst, rowptr, E) and the rows to sum.  cond "x": rows in 0 .. 8, g in
    {-1, 1, 2}, b in -1 .. 1 (sums below 300 * (8 * 2 + 1), exact); "p" / "c": rows from the producer."""
    deg = torch.tensor(seg_degrees(N))
    r = SimpleNamespace(N=N, E=int(deg.sum()), deg=deg, dst=torch.repeat_interleave(torch.arange(N), deg))
    r.rowptr = torch.zeros(N + 1, dtype=torch.int64)
    r.rowptr[1:] = torch.cumsum(deg, 0)
    g = torch.Generator().manual_seed(9000 + N + (cond == "c"))
    if cond == "x":
        r.rows = _ints(g, 0, 8, r.E, L)
        r.g = torch.tensor([-1.0, 1.0, 2.0])[torch.randint(0, 3, (L,), generator=g)]
        r.b = _ints(g, -1, 1, L)
        return r
    r.rows = _produce(r, cond, g, r.E)
    rn = _rn(g)
    r.g, r.b = rn(L) * 0.3 + 1.0, rn(L) * 0.1
    return r


STAT_ROWS = 3001                              # rows of the statistics tests' arrays
NPARTS = [1, 255, 256, 257, 700, 2048]        # around one 256-thread reduction round, up to pdg_max_blocks()
_stat_arrays = {}


def stat_array(cond):
    """The array whose row-slice sums the statistics tests reduce, and its two-pass statistics."""
    if cond not in _stat_arrays:
        g = torch.Generator().manual_seed(8000 + (cond == "c"))
        a = torch.relu(torch.randn(STAT_ROWS, L, generator=g, dtype=torch.float64)).float() * CONDS[cond]
        _stat_arrays[cond] = (a, ln_stat_ref(a))
    return _stat_arrays[cond]


def stat_bound(n, nparts, ref):
    """(K u, K u (1 + mean^2 / var)): the bounds on the relative errors of mean_d and std_d formed from exact fp64
    partials of an array of n non-negative elements.  The partials are fp64 sums of at most n terms, good to log2(n) u
    each (pairwise; u = 2^-53); the kernel adds nparts of them, at most ceil(nparts / 256) + 8 + 4 additions deep; the
    division, mean^2, the subtraction and the square root add a few u: K = log2(n) + nparts / 256 + 16 roundings.
    var = sumsq / n - mean^2 cancels: a relative error K u of either term is K u (1 + 2 mean^2 / var) of var, half of
    that of std."""
    import math
    K = math.log2(n) + nparts / 256 + 16
    return K * 2.0 ** -53, K * 2.0 ** -53 * (1 + ref.mean_d ** 2 / ref.std_d ** 2)
