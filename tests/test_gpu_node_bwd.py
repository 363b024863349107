"""The per-step node backward kernels and the backward's two ends at the op level, against the float64
restatements of tests/node_bwd_ref.py (anchored to autograd through the model's LayerNorm by
tests/test_node_bwd_ref.py):

  pdg_node_bwd_coop      gz2 / gz1 / gaggr / gx_part from the inputs (not from the kernel's own intermediate), with
                         lb = NULL and exact host-made pairs;
  pdg_gemm_sum2_coop     with and without the residual and the LayerNorm columns: out, column partials, pairs;
  pdg_decoder_bwd_coop   gz1d, gx, column partials, pairs, node_decoder.2's gradients through the finalize;
  pdg_mlp2_bwd_coop      both forms (gz1 stored; x_narrow with gz1 = NULL) and the 128 x 6 gradient;
  pdg_ln_colsum_nodes    the engine's form (ln_g, pairs, accumulate) on the hub graph;
  accumulate = 1         two calls into one accumulator, then pdg_ln_param_grads onto non-zero gradients;
  the engine's chains    producer -> consumer with lb = NULL, npairs = nblocks and the pairs straight from the
                         producer's NaN-prefilled buffer, against the fp64 reference of the whole chain.

Inputs (one set per case, shared by all tests; references computed once per case): a1 = relu(randn); the a2 arrays
and their pdg_ln_stat from the real producer (pdg_mlp2_fwd + pdg_ln_finalize) on different inputs -- LayerNorm "c",
the one the consumers invert, from second-layer weights scaled by 2e-4, so that its std (~5e-5) makes eps = 1e-5
count in den = std + eps and a kernel that mixes den and std up fails (Wn2T is scaled by 1e-4 in turn, so that
the products stay of the size of the residual); LayerNorm "p", the one the stand-alone
producers write sums for, from unscaled weights (statistics four orders of magnitude apart).  The upstream
gradients carry a multiple of xhat and a constant, so that S1 / M and S2 / M are of order one and the two scalar
terms of the LayerNorm backward carry weight.  Every output buffer has three NaN rows past N that must stay NaN;
every pairs buffer, and every partials buffer of an accumulate = 0 call, is NaN-filled: the engine hands the
kernels torch.empty, so a block without rows has to write its zeros.
"""
import ctypes
import math
import struct
from types import SimpleNamespace

import pytest
import torch

from edge_bwd_ref import hub_graph, worst_row
from node_bwd_ref import colsums, colsums_nodes, decoder_bwd_ref, gemm_sum2_ref, mlp2_bwd_ref, node_bwd_ref

pytestmark = pytest.mark.gpu

L = 128
# (N, nblocks): the smallest shapes that reach each path of the row schedule (block_rows, pdg_coop.hpp: per-block
# ranges of ceil(N / nblocks) rows rounded up to 32-row units; pdg_gemm_sum2_coop runs two 16-row rounds per unit
# and a trailing epilogue, the other three kernels walk 32-row units).
#   (1, 1) (15, 1)  fewer rows than a round            (16, 1)  exactly one round: the second round of the unit
#   (17, 1)         one row past a round                        is all padding
#   (31, 1)         one row short of a unit            (32, 1)  exactly one unit
#   (33, 2)         per = 32: block 0 a full unit, block 1 one row (one row past a unit)
#   (77, 37)        per = 32: blocks 0 - 2 hold 32, 32, 13 rows, 34 blocks are empty (more blocks than units)
#   (456, 256)      the published mesh size on the engine's grid: per = 32, 14 full blocks, one of 8 rows, 241 empty
#   (4099, 37)      per = 128: four units per block, block 32 holds 3 rows (ragged last round), blocks 33 - 36 empty
#   (8209, 256)     per = 64: two units per block, block 128 holds 17 rows, blocks 129 - 255 empty
CASES = [(1, 1), (15, 1), (16, 1), (17, 1), (31, 1), (32, 1), (33, 2), (77, 37), (456, 256), (4099, 37), (8209, 256)]
ACC_CASES = [(17, 1), (456, 256), (4099, 37)]
TOL = 2e-6      # a single bf16x6 / fp32 product from given inputs against fp64 (TOL of test_gpu_ops.py)
TOL_LN = 1e-5   # anything downstream of a LayerNorm backward (TOL of test_gpu_edge_bwd.py)
TOL_SUM = 1e-6  # fp64-accumulated column sums and narrow gradients (test_gpu_ops.py)
# the per-row bound: worst-row error of a kernel <= ROW_FACTOR x the worst-row error of the plain fp32 torch
# restatement of the same chain, both against fp64 (the edge suite's rule and its factor).  Measured on the MI355X
# for every case, kernel and output (profiles/node_bwd_op_errors.txt): ratios 0.49 - 1.66, the largest ones at N = 1
# (pdg_node_bwd_coop / pdg_mlp2_bwd_coop gz1 1.66, the chains 1.58 / 1.65, pdg_decoder_bwd_coop gx 1.53,
# pdg_gemm_sum2_coop 1.33), 0.49 - 1.43 from N = 15 on; none above 2.  The factor is the smallest power of two that
# is at least twice the largest of them (2 x 1.66 = 3.32 -> 4)
ROW_FACTOR = 4


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pdg.lib import lib, stream_handle
    from pdg import engine
    torch.manual_seed(0)
    return lib, stream_handle, engine


def rel(a, b):
    a = a.double().cpu()
    b = b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def rnd(*shape, scale=1.0):
    return (torch.randn(*shape, dtype=torch.float64) * scale).float().cuda()


def lin(out, inp):
    m = torch.nn.Linear(inp, out)
    return m.weight.detach().float().cuda().contiguous(), (m.bias.detach().float().cuda() + 0.1).contiguous()


def stat_from(buf):
    raw = buf.cpu().numpy().tobytes()
    mean, den, rstd, sd, mean_d, std_d, count = struct.unpack("ffffddd", raw[:40])
    return dict(mean=mean, den=den, rstd=rstd, std=sd, mean_d=mean_d, std_d=std_d, count=count)


def p(t):
    return None if t is None else t.data_ptr()


def nan_rows(N, width=L):
    return torch.full((N + 3, width), float("nan"), device="cuda")


def nan64(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def tails_are_nan(N, *outs):
    return all(bool(o[N:].isnan().all()) and o.shape[0] == N + 3 for o in outs)


def mlp2_fwd_stats(lib, s, x, W2, b2):
    """a2 = relu(W2 x + b2) and its LayerNorm statistics from the real producer."""
    M = x.shape[0]
    a2 = torch.empty(M, L, device="cuda")
    part = torch.empty(4096, dtype=torch.float64, device="cuda")
    n = ctypes.c_int(0)
    assert lib.pdg_mlp2_fwd(M, p(x), p(W2), p(b2), p(a2), p(part), ctypes.byref(n), s) == 0
    st = torch.zeros(40, dtype=torch.uint8, device="cuda")
    assert lib.pdg_ln_finalize(p(part), n.value, float(M * L), p(st), s) == 0
    return a2, st


def correlated(a2):
    """randn + xhat / 2 + 0.3: an upstream gradient for which S1 / M and S2 / M are of order one."""
    a = a2.double()
    xh = ((a - a.mean()) / a.std(unbiased=False)).float()
    return (rnd(*a2.shape) + 0.5 * xh + 0.3).contiguous()


def exact_pairs(S1, S2, nb):
    """(S1, S2), rounded to 40 significant bits (1e-12 relative), split over nb pairs as multiples k_i / 1024 with
    integers k_i in {-1 .. 3} (zero and negative pieces included) and a last piece that makes them sum to 1024:
    every partial sum, in any order, is a multiple of S 2^-10 below 2^12 S 2^-10 and therefore exact."""
    k = torch.tensor([(7 * i) % 5 - 1 for i in range(nb)], dtype=torch.float64)
    k[-1] += 1024 - k.sum()
    assert float(k.abs().sum()) < 4096

    def r40(x):
        m, e = math.frexp(float(x))
        return math.ldexp(round(m * 2 ** 40), e - 40)

    out = torch.stack([r40(S1) * k / 1024, r40(S2) * k / 1024], 1).contiguous()
    assert float(out[:, 0].sum()) == r40(S1) and float(out[:, 1].sum()) == r40(S2)
    return out.cuda()


class Case:
    """The inputs of one (N, nblocks) case on the device and its references (each made once)."""

    def __init__(self, env, N, nb):
        lib, sh, _ = env
        s = sh()
        torch.manual_seed(5000 + N)
        self.N, self.nb = N, nb
        self.a1 = torch.relu(rnd(N, L))
        W2, b2 = lin(L, L)
        self.a2, self.st = {}, {}
        self.a2["c"], self.st["c"] = mlp2_fwd_stats(lib, s, self.a1, (W2 * 2e-4).contiguous(), (b2 * 2e-4).contiguous())
        self.a2["p"], self.st["p"] = mlp2_fwd_stats(lib, s, torch.relu(rnd(N, L, scale=2.0)), W2, b2)
        torch.cuda.synchronize()
        sc, sp_ = stat_from(self.st["c"]), stat_from(self.st["p"])
        assert abs(sp_["mean_d"] - sc["mean_d"]) > 0.1 * sc["mean_d"] and abs(sp_["std_d"] - sc["std_d"]) > 0.1 * sc["std_d"]
        assert sc["count"] == N * L and 0.02 < 1e-5 / sc["std_d"] < 1.0   # eps counts in den
        self.ln_g = rnd(L) * 0.3 + 1.0
        self.gy = correlated(self.a2["c"])           # the consumers' upstream gradient; the chains' residual
        self.res_p = correlated(self.a2["p"])        # the stand-alone producer's residual
        self.Wn2T, self.Wn1aT, self.Wn1bT, self.W0T, self.W1T, self.Wd1T = (lin(L, L)[0] for _ in range(6))
        # 1 / den ~ 2e4 makes gz2 that large: Wn2T scaled back, so that Wn1b^T gz1 is of the size of the residual gy
        # in gx_part and a dropped residual shows (tests/test_node_bwd_ref.py measures it)
        self.Wn2T = (self.Wn2T * 1e-4).contiguous()
        # the products' operands carry a constant, so that the column sums of `out` / gx do not cancel: a bound on
        # the relative error of a sum is the per-element error x sum |o| / |sum o|, which for zero-mean rows is
        # 0.8 sqrt(N) (72 at N = 8209) and lets the bf16x6 chain's mean bias (-1.1e-9 of the product scale,
        # test_register_weight_kernels_match_lds_kernels) alone reach 1e-6 of a sum
        self.in0, self.in1 = rnd(N, L) + 0.5, rnd(N, L) - 0.25
        self.gy3, self.a1d, self.Wd2 = rnd(N, 3) + 0.5, torch.relu(rnd(N, L)), rnd(3, L)
        self.xn = rnd(N, 6)
        self._ref, self._runs = {}, {}

    def ref(self, name, dtype=torch.float64):
        """The restatements, in fp64 (the reference) or fp32 (the per-row yardstick), made once."""
        key = (name, dtype)
        if key in self._ref:
            return self._ref[key]
        d = dict(dtype=dtype)
        nw = (self.ln_g, self.Wn2T, self.Wn1aT, self.Wn1bT)
        if name == "node":            # pdg_node_bwd_coop alone
            r = node_bwd_ref(self.gy, self.a2["c"], self.a1, *nw, **d)
        elif name == "mlp2":          # pdg_mlp2_bwd_coop alone
            r = mlp2_bwd_ref(self.gy, self.a2["c"], self.a1, self.ln_g, self.Wn2T, self.xn, **d)
        elif name == "dec":
            r = decoder_bwd_ref(self.gy3, self.a1d, self.Wd2, self.Wd1T, **d)
        elif name in ("sum2_res", "sum2"):
            r = gemm_sum2_ref(self.in0, self.in1, self.W0T, self.W1T, self.res_p if name == "sum2_res" else None, **d)
        elif name == "sum2_chain":    # the chains' producer: residual gy, LayerNorm "c"
            r = gemm_sum2_ref(self.in0, self.in1, self.W0T, self.W1T, self.gy, **d)
        elif name == "dec->node":
            r = node_bwd_ref(self.ref("dec", dtype).gx, self.a2["c"], self.a1, *nw, **d)
        elif name == "sum2->node":
            r = node_bwd_ref(self.ref("sum2_chain", dtype), self.a2["c"], self.a1, *nw, **d)
        elif name == "sum2->mlp2":
            r = mlp2_bwd_ref(self.ref("sum2_chain", dtype), self.a2["c"], self.a1, self.ln_g, self.Wn2T, self.xn, **d)
        self._ref[key] = r
        return r

    # ---- kernel runs

    def node_bwd(self, env, gy, pairs, npairs):
        lib, sh, _ = env
        N = self.N
        o = SimpleNamespace(**{k: nan_rows(N) for k in ("gz2", "gz1", "gaggr", "gx_part")})
        assert lib.pdg_node_bwd_coop(N, p(gy), p(self.a2["c"]), p(self.a1), p(self.st["c"]), None, p(self.ln_g),
                                     p(self.Wn2T), p(self.Wn1aT), p(self.Wn1bT), p(o.gz2), p(o.gz1), p(o.gaggr),
                                     p(o.gx_part), p(pairs), npairs, self.nb, sh()) == 0
        torch.cuda.synchronize()
        return o

    def mlp2_bwd(self, env, gy, pairs, npairs, narrow):
        lib, sh, _ = env
        N, nb = self.N, self.nb
        o = SimpleNamespace(gz2=nan_rows(N), gz1=None if narrow else nan_rows(N),
                            npart=nan64(nb * (6 * L + L + 6)) if narrow else None)
        assert lib.pdg_mlp2_bwd_coop(N, p(gy), p(self.a2["c"]), p(self.a1), p(self.st["c"]), None, p(self.ln_g),
                                     p(self.Wn2T), p(o.gz2), p(o.gz1), p(pairs), npairs, p(self.xn) if narrow else None,
                                     p(o.npart), nb, sh()) == 0
        torch.cuda.synchronize()
        return o

    def gemm_sum2(self, env, res, ln, cols=True, acc=None, in0=None, in1=None):
        """pdg_gemm_sum2_coop; acc None: accumulate = 0 into a NaN-filled partials buffer, else accumulate = 1
        into `acc`.  The pairs buffer is always NaN-filled."""
        lib, sh, _ = env
        N, nb = self.N, self.nb
        o = SimpleNamespace(out=nan_rows(N), part=(nan64(nb, 256) if acc is None else acc) if cols else None,
                            pairs=nan64(nb, 2) if cols else None)
        in0, in1 = self.in0 if in0 is None else in0, self.in1 if in1 is None else in1
        assert lib.pdg_gemm_sum2_coop(N, p(in0), p(in1), p(self.W0T), p(self.W1T), p(res), p(o.out),
                                      p(self.a2[ln]) if cols else None, p(self.st[ln]) if cols else None, p(o.part),
                                      p(self.ln_g) if cols else None, p(o.pairs), int(acc is not None), nb, sh()) == 0
        torch.cuda.synchronize()
        return o

    def decoder(self, env, ln, acc=None, gy3=None):
        lib, sh, _ = env
        N, nb = self.N, self.nb
        o = SimpleNamespace(gz1d=nan_rows(N), gx=nan_rows(N), part=nan64(nb, 256) if acc is None else acc,
                            pairs=nan64(nb, 2), npart=nan64(nb * (3 * L + L + 3)))
        assert lib.pdg_decoder_bwd_coop(N, p(self.gy3 if gy3 is None else gy3), p(self.a1d), p(self.Wd2), p(self.Wd1T),
                                        p(o.gz1d), p(o.gx), p(self.a2[ln]), p(self.st[ln]), p(o.part), p(self.ln_g),
                                        p(o.pairs), int(acc is not None), p(o.npart), nb, sh()) == 0
        torch.cuda.synchronize()
        return o

    def chain_producer(self, env, which):
        """The producers of the engine's chains (LayerNorm "c", accumulate = 0, NaN-prefilled buffers), run once."""
        if which not in self._runs:
            self._runs[which] = self.decoder(env, "c") if which == "dec" else self.gemm_sum2(env, self.gy, "c")
        return self._runs[which]


_cases = {}


def case(env, N, nb):
    if (N, nb) not in _cases:
        _cases[(N, nb)] = Case(env, N, nb)
    return _cases[(N, nb)]


def check_rows(kernel, c, got, r64, r32, keys):
    """The per-row bound for the outputs `keys` (attributes of got / r64 / r32, or the tensors themselves when
    keys is None); prints the figures profiles/node_bwd_op_errors.txt records."""
    items = [("out", got, r64, r32)] if keys is None else [(k, getattr(got, k), getattr(r64, k), getattr(r32, k))
                                                           for k in keys]
    bad = []
    for k, g, a, b in items:
        mine, plain = worst_row(g[:c.N], a), worst_row(b, a)
        ratio = mine / plain if plain > 0 else (0.0 if mine == 0 else float("inf"))
        print(f"ROWS {kernel} N={c.N} nb={c.nb} {k}: rel {rel(g[:c.N], a):.2e} worst row {mine:.2e} / fp32 {plain:.2e} "
              f"= {ratio:.2f}")
        if not mine <= ROW_FACTOR * plain:
            bad.append((k, mine, plain, ratio))
    assert not bad, (kernel, bad)


def check_sums(c, part, pairs, cols64, S1, S2, tol=TOL_SUM):
    """A producer's accumulate = 0 output: all nblocks rows and pairs written (finite: an empty block wrote its
    zeros), the rows summed within `tol` of the fp64 column sums of the fp64 upstream gradient, the pairs summed
    equal to g . (the kernel's own summed rows) and within tol x sum_c |g_c cols_c| of the fp64 (S1, S2) -- the
    error that a relative error `tol` of every column sum can give a g-weighted sum of them."""
    assert part.shape == (c.nb, 256) and bool(part.isfinite().all()), "a block left its partial row unwritten"
    assert pairs.shape == (c.nb, 2) and bool(pairs.isfinite().all()), "a block left its pair unwritten"
    got = part.sum(0).cpu()
    print(f"SUMS N={c.N} nb={c.nb}: {rel(got, cols64):.2e} (sum gy {rel(got[:L], cols64[:L]):.2e}, sum gy xhat "
          f"{rel(got[L:], cols64[L:]):.2e})")
    assert rel(got, cols64) < tol, rel(got, cols64)
    gd = c.ln_g.double().cpu()
    sp = pairs.sum(0).cpu()
    assert rel(sp, torch.stack([(gd * got[:L]).sum(), (gd * got[L:]).sum()])) < 1e-9
    for k, (S, half) in enumerate(((S1, cols64[:L]), (S2, cols64[L:]))):
        assert abs(float(sp[k]) - float(S)) <= tol * float((gd * half).abs().sum()), (k, float(sp[k]), float(S))


# ------------------------------------------------------------------------------------------ the kernels alone

@pytest.mark.parametrize("N,nb", CASES)
def test_node_bwd_coop_vs_fp64(env, N, nb):
    """pdg_node_bwd_coop with lb = NULL and the fp64 (S1, S2) as nblocks exact pairs: gz2, gz1, gaggr and gx_part
    within 1e-5 of the fp64 restatement formed from the inputs, the worst row within ROW_FACTOR of the fp32
    restatement's, no row written at or past N."""
    c = case(env, N, nb)
    r64, r32 = c.ref("node"), c.ref("node", torch.float32)
    o = c.node_bwd(env, c.gy, exact_pairs(r64.ln.S1, r64.ln.S2, nb), nb)
    keys = ("gz2", "gz1", "gaggr", "gx_part")
    errs = {k: rel(getattr(o, k)[:N], getattr(r64, k)) for k in keys}
    assert tails_are_nan(N, o.gz2, o.gz1, o.gaggr, o.gx_part)
    assert max(errs.values()) < TOL_LN, errs
    check_rows("node_bwd_coop", c, o, r64, r32, keys)


@pytest.mark.parametrize("res", [True, False])
@pytest.mark.parametrize("N,nb", CASES)
def test_gemm_sum2_coop_vs_fp64(env, N, nb, res):
    """pdg_gemm_sum2_coop with and without the residual, with and without the LayerNorm columns: out within 2e-6 of
    fp64 and bitwise the same with and without the columns; the column partials summed over the blocks against the
    column sums of the fp64 out (not of the kernel's output); the pairs summed over all nblocks entries against the
    fp64 (S1, S2), NaN if an empty block wrote nothing."""
    c = case(env, N, nb)
    name = "sum2_res" if res else "sum2"
    r64, r32 = c.ref(name), c.ref(name, torch.float32)
    plain = c.gemm_sum2(env, c.res_p if res else None, "p", cols=False)
    o = c.gemm_sum2(env, c.res_p if res else None, "p")
    assert tails_are_nan(N, plain.out, o.out)
    assert torch.equal(plain.out[:N], o.out[:N])
    assert rel(o.out[:N], r64) < TOL, rel(o.out[:N], r64)
    check_rows(f"gemm_sum2_coop res={int(res)}", c, o.out, r64, r32, None)
    check_sums(c, o.part, o.pairs, *colsums(r64, c.a2["p"], c.ln_g))


@pytest.mark.parametrize("N,nb", CASES)
def test_decoder_bwd_coop_vs_fp64(env, N, nb):
    """pdg_decoder_bwd_coop with columns, pairs and narrow partials: gz1d and gx within 2e-6 of fp64 (products of
    given inputs), the column partials / pairs against the sums of the fp64 gx, and node_decoder.2's weight / bias
    gradient through pdg_wgrad_narrow_finalize added onto a non-zero start."""
    lib, sh, _ = env
    c = case(env, N, nb)
    r64, r32 = c.ref("dec"), c.ref("dec", torch.float32)
    o = c.decoder(env, "p")
    assert tails_are_nan(N, o.gz1d, o.gx)
    errs = {k: rel(getattr(o, k)[:N], getattr(r64, k)) for k in ("gz1d", "gx")}
    assert max(errs.values()) < TOL, errs
    check_rows("decoder_bwd_coop", c, o, r64, r32, ("gz1d", "gx"))
    check_sums(c, o.part, o.pairs, *colsums(r64.gx, c.a2["p"], c.ln_g))
    assert bool(o.npart.isfinite().all()), "a block left its narrow partial unwritten"
    gW, gb = torch.full((3, L), 0.5, device="cuda"), torch.full((3,), -0.25, device="cuda")
    assert lib.pdg_wgrad_narrow_finalize(p(o.npart), nb, 3, 1, p(gW), None, p(gb), sh()) == 0
    assert rel(gW.double() - 0.5, r64.dWd2) < TOL_SUM and rel(gb.double() + 0.25, r64.dbd2) < TOL_SUM


@pytest.mark.parametrize("N,nb", CASES)
def test_mlp2_bwd_coop_vs_fp64(env, N, nb):
    """pdg_mlp2_bwd_coop in both forms -- gz1 stored; x_narrow with gz1 = NULL -- with exact pairs: gz2 / gz1 within
    1e-5 of the fp64 restatement formed from the inputs and within the per-row bound, gz2 bitwise the same in both
    forms; the finalized 128 x 6 weight gradient and the bias gradient, added onto a non-zero start, within 1e-6 of
    the fp64 sums over the stored gz1 and within 1e-5 (downstream of a LayerNorm backward) of fp64 from the inputs."""
    lib, sh, _ = env
    c = case(env, N, nb)
    r64, r32 = c.ref("mlp2"), c.ref("mlp2", torch.float32)
    pairs = exact_pairs(r64.ln.S1, r64.ln.S2, nb)
    a, b = c.mlp2_bwd(env, c.gy, pairs, nb, narrow=False), c.mlp2_bwd(env, c.gy, pairs, nb, narrow=True)
    assert tails_are_nan(N, a.gz2, a.gz1, b.gz2)
    errs = {k: rel(getattr(a, k)[:N], getattr(r64, k)) for k in ("gz2", "gz1")}
    assert max(errs.values()) < TOL_LN, errs
    assert torch.equal(a.gz2[:N], b.gz2[:N])
    check_rows("mlp2_bwd_coop", c, a, r64, r32, ("gz2", "gz1"))
    assert bool(b.npart.isfinite().all()), "a block left its narrow partial unwritten"
    gW, gb = torch.full((L, 6), 0.5, device="cuda"), torch.full((L,), -0.25, device="cuda")
    assert lib.pdg_wgrad_narrow_finalize(p(b.npart), nb, 6, 0, p(gW), p(gb), None, sh()) == 0
    z1 = a.gz1[:N].double()
    assert rel(gW.double() - 0.5, z1.T @ c.xn.double()) < TOL_SUM and rel(gb.double() + 0.25, z1.sum(0)) < TOL_SUM
    assert rel(gW.double() - 0.5, r64.dW0) < TOL_LN and rel(gb.double() + 0.25, r64.db0) < TOL_LN


# ------------------------------------------------------------------------------------------ pdg_ln_colsum_nodes

class Graph:
    """hub_graph(E) on the device with the message LayerNorm's a2m / statistics from the real producer and the
    per-node sums of xhat from pdg_segment_sum, as the engine has them."""

    def __init__(self, env, E):
        lib, sh, _ = env
        s = sh()
        torch.manual_seed(6000 + E)
        self.E = E
        self.N, _, self.dst64, rp, _, _ = hub_graph(E)
        self.rp = rp.int().cuda()
        W2, b2 = lin(L, L)
        self.a2m, self.st = mlp2_fwd_stats(lib, s, torch.relu(rnd(E, L)), W2, b2)
        self.ln_g, ln_b = rnd(L) * 0.3 + 1.0, rnd(L) * 0.1
        self.xs, out = torch.empty(self.N, L, device="cuda"), torch.empty(self.N, L, device="cuda")
        assert lib.pdg_segment_sum(self.N, p(self.rp), p(self.a2m), p(self.st), p(self.ln_g), p(ln_b), p(out),
                                   p(self.xs), s) == 0
        self.gaggr = rnd(self.N, L) + 0.3
        self.rows = lib.pdg_max_blocks() + 1
        torch.cuda.synchronize()

    def colsum_nodes(self, env, part, pairs, accumulate, gaggr=None):
        lib, sh, _ = env
        n = ctypes.c_int(-1)
        assert lib.pdg_ln_colsum_nodes(self.N, p(self.gaggr if gaggr is None else gaggr), p(self.rp), p(self.xs),
                                       p(part), ctypes.byref(n), p(self.ln_g), p(pairs), accumulate, sh()) == 0
        torch.cuda.synchronize()
        return n.value


_graphs = {}


def graph(env, E):
    if E not in _graphs:
        _graphs[E] = Graph(env, E)
    return _graphs[E]


@pytest.mark.parametrize("E", [1, 77, 4099, 60000])
def test_ln_colsum_nodes_engine_form(env, E):
    """pdg_ln_colsum_nodes as the engine calls it (ln_g, pairs, accumulate) on the hub graph (a hub run, nodes
    without an incoming edge, trailing isolated nodes; E = 60000: more nodes than 8 x the grid's cap).  accumulate
    = 0 into NaN-filled buffers: *nparts <= 2 x the CU count, rows and pairs below *nparts finite, those at and
    after it still NaN; the summed rows within 1e-6 of the node-level fp64 form over the xhat_sum array the kernel is
    given, and against the fp64 sums over the edges with gy = gaggr[dst] (sum gy within 1e-6; sum gy xhat within the
    fp32 rounding of xhat_sum, pdg_segment_sum's output, bounded per column from the number format), the pairs
    against g . rows and the fp64 (S1, S2).  accumulate = 1 onto a non-zero accumulator adds the same rows
    and leaves a sentinel in the rows at and after *nparts."""
    g = graph(env, E)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    part, pairs = nan64(g.rows, 256), nan64(g.rows, 2)
    n = g.colsum_nodes(env, part, pairs, 0)
    assert 1 <= n <= 2 * cus and n == min((g.N + 7) // 8, 2 * cus)
    assert bool(part[:n].isfinite().all()) and bool(pairs[:n].isfinite().all())
    assert bool(part[n:].isnan().all()) and bool(pairs[n:].isnan().all())
    got, sp = part[:n].sum(0).cpu(), pairs[:n].sum(0).cpu()
    gd = g.ln_g.double().cpu()
    assert rel(sp, torch.stack([(gd * got[:L]).sum(), (gd * got[L:]).sum()])) < 1e-9
    # what the kernel is asked for: the node-level sums over the xhat_sum array it is given
    cols, S1, S2 = colsums_nodes(g.gaggr, g.dst64, g.a2m, g.ln_g, xs=g.xs)
    e_gy, e_gyx = rel(got[:L], cols[:L]), rel(got[L:], cols[L:])
    assert e_gy < TOL_SUM and e_gyx < TOL_SUM, (e_gy, e_gyx)
    assert abs(float(sp[0] - S1)) <= TOL_SUM * float((gd * cols[:L]).abs().sum())
    assert abs(float(sp[1] - S2)) <= TOL_SUM * float((gd * cols[L:]).abs().sum())
    # and the fp64 sums over the edges, gy_k = gaggr[dst_k] with xhat from a2m: the difference is the fp32 rounding
    # of xhat_sum.  Per node and column: each fp32 xhat_k is within 2^-24 (5 |xhat_k| + |mean| / den) of the fp64
    # one (the subtraction, the fp32 mean, den = std + eps twice rounded, a division good to 1 ulp), and an fp32 sum
    # of deg_v terms in any order adds at most deg_v 2^-24 sum_k |xhat_k|; weighted by |gaggr_v|, plus the 1e-6 of
    # the kernel's own sums
    true, _, _ = colsums_nodes(g.gaggr, g.dst64, g.a2m, g.ln_g)
    a2 = g.a2m.double().cpu()
    den = a2.std(unbiased=False) + 1e-5
    xhat = (a2 - a2.mean()) / den
    A = torch.zeros(g.N, L, dtype=torch.float64).index_add_(0, g.dst64, xhat.abs())
    deg = torch.bincount(g.dst64, minlength=g.N).double().unsqueeze(1)
    ga = g.gaggr.double().cpu().abs()
    bound = (2.0 ** -24 * (ga * ((deg + 5) * A + deg * a2.mean().abs() / den)).sum(0)
             + TOL_SUM * (ga * g.xs.double().cpu().abs()).sum(0))
    t_gy, t_gyx = rel(got[:L], true[:L]), rel(got[L:], true[L:])
    print(f"ln_colsum_nodes E={E} N={g.N} nparts={n}: given xhat_sum: sum gy {e_gy:.2e} sum gy xhat {e_gyx:.2e}; "
          f"from a2m: sum gy {t_gy:.2e} sum gy xhat {t_gyx:.2e}, largest error / bound "
          f"{float(((got[L:] - true[L:]).abs() / bound).max()):.3f}")
    assert t_gy < TOL_SUM
    assert bool(((got[L:] - true[L:]).abs() <= bound).all())
    acc = torch.full((g.rows, 256), 3.25, dtype=torch.float64, device="cuda")
    pairs1 = nan64(g.rows, 2)
    assert g.colsum_nodes(env, acc, pairs1, 1) == n
    assert torch.equal(acc[:n], part[:n] + 3.25) and bool((acc[n:] == 3.25).all())
    assert torch.equal(pairs1[:n], pairs[:n]) and bool(pairs1[n:].isnan().all())


# ------------------------------------------------------------------------------------------ accumulate = 1

def param_grads(env, acc, rows, start_g=0.5, start_b=-0.25):
    """pdg_ln_param_grads of one accumulator group onto non-zero gradient arrays; returns what it added."""
    lib, sh, _ = env
    gg, gb = torch.full((L,), start_g, device="cuda"), torch.full((L,), start_b, device="cuda")
    P = ctypes.c_void_p
    assert lib.pdg_ln_param_grads(1, (P * 1)(acc.data_ptr()), (ctypes.c_int * 1)(rows), (P * 1)(gg.data_ptr()),
                                  (P * 1)(gb.data_ptr()), sh()) == 0
    torch.cuda.synchronize()
    return torch.cat([gb.double() - start_b, gg.double() - start_g]).cpu()   # [sum gy | sum gy xhat]


@pytest.mark.parametrize("producer", ["gemm_sum2_coop", "decoder_bwd_coop", "edge_gout_wc", "ln_colsum_nodes"])
@pytest.mark.parametrize("N,nb", ACC_CASES)
def test_accumulate_two_calls_then_param_grads(env, N, nb, producer):
    """The engine's accumulate = 1: two calls on different inputs, for two LayerNorms of one group, into one
    zeroed accumulator; pdg_ln_param_grads then adds onto non-zero gradient arrays start + the fp64 sum of both
    calls' column sums.  The cooperative column-sum producers of the backward (pdg_gemm_sum2_coop,
    pdg_decoder_bwd_coop and, sharing their emit code, pdg_edge_gout_wc run over the same rows) and
    pdg_ln_colsum_nodes (on hub_graph(N)).  The pairs, NaN-prefilled, are those of each call alone.  With
    accumulate = 0 the first nblocks rows of a NaN-filled buffer come out finite in all 256 columns."""
    lib, sh, _ = env
    c = case(env, N, nb)
    if producer == "ln_colsum_nodes":
        g = graph(env, N)
        acc = torch.zeros(g.rows, 256, dtype=torch.float64, device="cuda")
        g2 = g.gaggr.flip(1).contiguous() * 0.5
        n = g.colsum_nodes(env, acc, nan64(g.rows, 2), 1)
        assert g.colsum_nodes(env, acc, nan64(g.rows, 2), 1, gaggr=g2) == n
        want = (colsums_nodes(g.gaggr, g.dst64, g.a2m, g.ln_g, xs=g.xs)[0]
                + colsums_nodes(g2, g.dst64, g.a2m, g.ln_g, xs=g.xs)[0])
        got = param_grads(env, acc, n)
        assert rel(got[:L], want[:L]) < TOL_SUM and rel(got[L:], want[L:]) < TOL_SUM
        return
    acc = torch.zeros(nb, 256, dtype=torch.float64, device="cuda")
    if producer == "gemm_sum2_coop":
        in0b, in1b = c.in1.flip(0).contiguous(), (c.in0 * 0.5).contiguous()
        o1 = c.gemm_sum2(env, c.res_p, "p", acc=acc)
        o2 = c.gemm_sum2(env, c.gy, "c", acc=acc, in0=in0b, in1=in1b)
        o0 = c.gemm_sum2(env, c.res_p, "p")
        gy1, gy2 = c.ref("sum2_res"), gemm_sum2_ref(in0b, in1b, c.W0T, c.W1T, c.gy)
    elif producer == "decoder_bwd_coop":
        gy3b = (c.gy3.flip(0) * 0.5).contiguous()
        o1 = c.decoder(env, "p", acc=acc)
        o2 = c.decoder(env, "c", acc=acc, gy3=gy3b)
        o0 = c.decoder(env, "p")
        gy1, gy2 = c.ref("dec").gx, decoder_bwd_ref(gy3b, c.a1d, c.Wd2, c.Wd1T).gx
    else:   # pdg_edge_gout_wc over N rows: ge_out = ge_next + Wc^T gC, the same sums for the LayerNorm of ge_out
        def gout(gC, ge_next, ln, part, accumulate):
            o = SimpleNamespace(out=nan_rows(N), part=part, pairs=nan64(nb, 2))
            slabs = torch.empty(nb, L * L + L, device="cuda")
            assert lib.pdg_edge_gout_wc(N, p(gC), p(c.in1), p(ge_next), p(c.W0T), p(o.out), p(slabs), nb, p(c.a2[ln]),
                                        p(c.st[ln]), p(part), p(c.ln_g), p(o.pairs), accumulate, 1, sh()) == 0
            torch.cuda.synchronize()
            return o
        zero = torch.zeros(N, L)
        in0b = c.in1.flip(0).contiguous()
        o1, o2 = gout(c.in0, c.res_p, "p", acc, 1), gout(in0b, c.gy, "c", acc, 1)
        o0 = gout(c.in0, c.res_p, "p", nan64(nb, 256), 0)
        gy1 = gemm_sum2_ref(c.in0, zero, c.W0T, c.W1T, c.res_p)
        gy2 = gemm_sum2_ref(in0b, zero, c.W0T, c.W1T, c.gy)
        assert rel(o1.out[:N], gy1) < TOL and rel(o2.out[:N], gy2) < TOL and tails_are_nan(N, o1.out, o2.out)
    c1, c2 = colsums(gy1, c.a2["p"], c.ln_g), colsums(gy2, c.a2["c"], c.ln_g)
    got = param_grads(env, acc, nb)
    err = rel(got, c1[0] + c2[0])
    print(f"accumulate {producer} N={N} nb={nb}: {err:.2e}")
    assert err < TOL_SUM, err
    # accumulate = 0: every row and pair written; the pairs of an accumulating call are its own, not accumulated
    check_sums(c, o0.part, o0.pairs, *c1)
    assert torch.equal(o1.pairs, o0.pairs) and bool(o2.pairs.isfinite().all())
    gd = c.ln_g.double().cpu()
    sp2 = o2.pairs.sum(0).cpu()
    for k, (S, half) in enumerate(((c2[1], c2[0][:L]), (c2[2], c2[0][L:]))):
        assert abs(float(sp2[k]) - float(S)) <= TOL_SUM * float((gd * half).abs().sum())


# ------------------------------------------------------------------------------------------ the engine's chains

@pytest.mark.parametrize("chain", ["dec->node", "sum2->node", "sum2->mlp2"])
@pytest.mark.parametrize("N,nb", CASES)
def test_engine_chain_producer_pairs_to_consumer(env, N, nb, chain):
    """Producer -> consumer as the engine runs them: the producer writes the sums of the LayerNorm the consumer
    inverts into NaN-prefilled buffers (accumulate = 0), the consumer takes lb = NULL, the producer's pairs buffer
    as it is and npairs = nblocks, and its upstream gradient is the producer's output.  The consumer's outputs
    against the fp64 reference of the whole chain: that a producer's pair layout and a consumer's reduction agree.
      pdg_decoder_bwd_coop -> pdg_node_bwd_coop   (_bwd_decoder -> _bwd_step(S - 1))
      pdg_gemm_sum2_coop   -> pdg_node_bwd_coop   (_bwd_step(t) -> _bwd_step(t - 1))
      pdg_gemm_sum2_coop   -> pdg_mlp2_bwd_coop   (_bwd_step(0) -> _bwd_encoders, x_narrow, gz1 = NULL)"""
    lib, sh, _ = env
    c = case(env, N, nb)
    r64, r32 = c.ref(chain), c.ref(chain, torch.float32)
    prod = c.chain_producer(env, "dec" if chain.startswith("dec") else "sum2")
    gy = (prod.gx if chain.startswith("dec") else prod.out)[:N]
    assert bool(prod.pairs.isfinite().all()), "a block left its pair unwritten"
    if chain.endswith("node"):
        o = c.node_bwd(env, gy, prod.pairs, nb)
        keys = ("gz2", "gz1", "gaggr", "gx_part")
        assert tails_are_nan(N, *(getattr(o, k) for k in keys))
    else:
        o = c.mlp2_bwd(env, gy, prod.pairs, nb, narrow=True)
        keys = ("gz2",)
        assert tails_are_nan(N, o.gz2) and o.gz1 is None
    errs = {k: rel(getattr(o, k)[:N], getattr(r64, k)) for k in keys}
    if not chain.endswith("node"):
        gW, gb = torch.full((L, 6), 0.5, device="cuda"), torch.full((L,), -0.25, device="cuda")
        assert lib.pdg_wgrad_narrow_finalize(p(o.npart), nb, 6, 0, p(gW), p(gb), None, sh()) == 0
        errs["dW0"], errs["db0"] = rel(gW.double() - 0.5, r64.dW0), rel(gb.double() + 0.25, r64.db0)
    print(f"chain {chain} N={N} nb={nb} " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < TOL_LN, errs
    check_rows(f"chain {chain}", c, o, r64, r32, keys)
