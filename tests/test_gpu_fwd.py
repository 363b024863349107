"""The per-step forward kernels at the op level, against the float64 restatements of tests/fwd_ref.py (anchored to
oracle.epd_oracle by tests/test_fwd_ref.py) formed from the inputs, never from another kernel:

  pdg_edge_fwd_coop        e_t, a1m / a1e (and their NULL, inference form), a2m / a2e, both LayerNorm partials;
  pdg_edge_fwd_infer       e_t, a2m / a2e, partials;
  pdg_node_pq_rw[_fin]     x_t, P, Q in the library's P / Q layout, the stored statistics;
  pdg_segment_sum[_fin]    aggr, xhat_sum (also NULL), without LayerNorm, the stored statistics;
  pdg_decoder_fwd_coop     x_S, a1d, y, the stored statistics;
  pdg_ln_finalize[2]       and the three in-kernel reducers, against the statistics of the array itself;
  the engine's chain       two steps in the engine's order and buffer hand-over, against the oracle.

Two input families per case (fwd_ref.exact_edge_inputs / randn_edge_inputs, node_inputs, seg_inputs).  Integer-
exact: unit statistics, small integer operands and one-term integer weights, for which every product, sum and
LayerNorm partial of the kernels is exact, so the outputs must EQUAL the fp64 (integer) reference: a wrong, missing
or doubled row at any block layout shows without a tolerance.  randn: a2_prev and its pdg_ln_stat from the real
producer (pdg_mlp2_fwd + pdg_ln_finalize) in two conditionings, "p" (unscaled weights, std ~ 0.6, on the hub graph)
and "c" (second-layer weights x 2e-4, std ~ 5e-5, on the ends graph), so that eps = 1e-5 counts in den and a kernel
that mixes den and std up fails.  Bounds of the randn family: relative L2 against fp64 below TOL in conditioning
"p" and below TOL_LN in "c" (every output there is downstream of the small-std LayerNorm), for every output: e_t,
x_t, x_S, a1*, a2*, P, Q, aggr, xhat_sum, a1d, y; per row, the worst-row error at most ROW_FACTOR x that of the plain
fp32 torch restatement, both against fp64; LayerNorm partial totals within 1e-6 sum |ref| (sum) and 1e-6 relative
(sum of squares), the bounds of test_gpu_ops.test_edge_enc_fwd_vs_fp64.

Every output buffer has three NaN rows past its rows that must stay NaN; the P / Q buffer has one NaN row after node
N - 1 (an off-by-one gather poisons the output); every partials buffer is NaN-filled: the engine hands the kernels
torch.empty, so a block without rows has to write its zeros."""
import ctypes
import struct
from types import SimpleNamespace

import pytest
import torch

import fwd_ref as F
from edge_bwd_ref import hub_graph, worst_row
from oracle import epd_oracle as O

pytestmark = pytest.mark.gpu

L = 128
TOL, TOL_LN, TOL_STAT = F.TOL, F.TOL_LN, F.TOL_STAT
# (E, nblocks): the smallest shapes that reach each path of row_schedule (pdg_coop.hpp).  nblocks != 256: block_rows,
# per-block ranges of ceil(E / nblocks) rows rounded up to 32-row units, walked unit by unit (pdg_edge_fwd_coop) or
# as two 16-row rounds per unit (pdg_edge_fwd_infer).  nblocks == 256 = XCD_GRID: the interleaved form, units =
# ceil(E / 32), perx = ceil(units / 8) units per XCD x = block & 7, block j = block >> 3 starts at unit j of its XCD's
# range [32 x perx, 32 (x + 1) perx) and strides 32 units = 1024 rows.
#   (1, 1) (15, 1)  fewer rows than a round            (16, 1)  exactly one round
#   (17, 1)         one row past a round               (31, 1)  one row short of a unit     (32, 1)  one unit
#   (33, 2)         per = 32: block 1 holds one row
#   (77, 37)        per = 32: blocks 0 - 2 hold 32, 32, 13 rows, 34 blocks are empty (more blocks than units)
#   (4099, 37)      per = 128: four units per block, block 32 holds 3 rows (ragged last round), blocks 33 - 36 empty
#   (33, 256)       units = 2, perx = 1: XCD 0 one unit, XCD 1 one row (r0 = 32, r1 = 33), XCDs 2 - 7 r0 = r1 = 33,
#                   every block j >= 1 empty (first = min(E, r0 + 32 j) >= r1)
#   (257, 256)      units = 9, perx = 2: XCDs 0 - 3 two units (j = 0, 1), XCD 4 the 1-row unit [256, 257), XCDs 5 - 7
#                   r0 = r1 = 257
#   (8193, 256)     units = 257, perx = 33: XCDs 0 - 6 hold 33 units each, so block j = 0 walks units 0 and 32 of its
#                   XCD (a second round one stride of 1024 rows on: the deferred a2 store across a stride; the
#                   smallest E with perx > 32); XCD 7 holds units 231 - 256, the last a 1-row unit at j = 25, its
#                   blocks j >= 26 are empty with first = E
CASES = [(1, 1), (15, 1), (16, 1), (17, 1), (31, 1), (32, 1), (33, 2), (77, 37), (4099, 37), (33, 256), (257, 256),
         (8193, 256)]
FLAGS = [(1, 1), (0, 1), (1, 0), (0, 0)]   # (eu, res)
# node kernels (N, nblocks of pdg_decoder_fwd_coop): pdg_node_pq_rw walks 16-row tiles on min(tiles, CUs) blocks (N =
# 4099: 257 tiles, block 0 takes a second one); the decoder walks block_rows as above
NODE_CASES = [(1, 1), (15, 1), (16, 1), (17, 1), (33, 2), (77, 37), (4099, 37), (257, 256)]
NPARTS, STAT_ROWS = F.NPARTS, F.STAT_ROWS   # nparts up to pdg_max_blocks(); ln_stat_from_partials strides 256 threads
VARIANTS = [("hub", "p"), ("ends", "c")]
# the per-row bound: worst-row error of a kernel <= ROW_FACTOR x the worst-row error of the plain fp32 torch
# restatement of the same chain, both against fp64 (the rule of the backward suites).  Measured on the MI355X for
# every case, kernel and output (profiles/fwd_op_errors.txt): ratios 0.27 - 1.78, the largest ones
# pdg_decoder_fwd_coop's y at N = 17 (1.78), the edge kernels' a2m at E = 1 (1.57), pdg_node_pq_rw's x_t at N = 15
# (1.18), pdg_segment_sum 1.01, the chain's y 0.96; none above 2.  The factor is the smallest power of two that is at
# least twice the largest of them (2 x 1.78 = 3.56 -> 4)
ROW_FACTOR = 4


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pdg.lib import lib, stream_handle
    torch.manual_seed(0)
    return lib, stream_handle


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def p(t):
    return None if t is None else t.data_ptr()


def cu(t):
    return t.float().contiguous().cuda()


def nan_rows(n, width=L):
    return torch.full((n + 3, width), float("nan"), device="cuda")


def nan64(n):
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def tail_ok(n, t):
    return t.shape[0] == n + 3 and bool(t[n:].isnan().all())


def pack_stat(s):
    raw = struct.pack("ffffddd", s.mean, s.den, s.rstd, s.std_, s.mean_d, s.std_d, s.count)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()


def stat_from(buf):
    mean, den, rstd, sd, mean_d, std_d, count = struct.unpack("ffffddd", buf.cpu().numpy().tobytes()[:40])
    return SimpleNamespace(mean=mean, den=den, rstd=rstd, std_=sd, mean_d=mean_d, std_d=std_d, count=count)


def sentinel():
    return torch.full((40,), 0xAB, dtype=torch.uint8, device="cuda")


def unit_partials(nparts, count):
    """(sum, sumsq) pairs that pdg_ln_finalize turns into the unit statistics: sum 0 in pieces that cancel, sumsq =
    count s^2 with s the fp32 nearest 1 - 1e-5f, spread evenly: std_ = s, den = s + 1e-5f = 1.0f, rstd = 1."""
    s = float(torch.tensor(1.0) - F.EPS32)
    part = torch.zeros(nparts, 2, dtype=torch.float64)
    part[:, 1] = count * s * s / nparts
    if nparts > 1:
        part[0, 0], part[-1, 0] = 3.0, -3.0
    return part.reshape(-1).cuda()


def unit_stats(env, nparts, count):
    """unit_partials and what pdg_ln_finalize makes of them, checked field by field: the statistics an in-kernel
    reducer must store for the integer-exact family (compared bitwise)."""
    lib, sh = env
    part, st = unit_partials(nparts, count), sentinel()
    assert lib.pdg_ln_finalize(p(part), nparts, float(count), p(st), sh()) == 0
    torch.cuda.synchronize()
    s = stat_from(st)
    assert (s.mean, s.den, s.rstd, s.mean_d, s.count) == (0.0, 1.0, 1.0, 0.0, float(count))
    assert s.std_ == float(torch.tensor(1.0) - F.EPS32) and abs(s.std_d - s.std_) < 1e-15
    return part, st


class PQ:
    """P / Q in the library's layout (pdg_pq_layout: two N x 128 arrays, or one N x 256 array of interleaved
    16-feature blocks with Q 16 floats after P), NaN-filled, with one extra NaN row after node N - 1."""

    def __init__(self, lib, N, P=None, Q=None):
        self.N, self.blocked = N, bool(lib.pdg_pq_layout())
        if self.blocked:
            self.buf = torch.full((N + 1, 2 * L), float("nan"), device="cuda")
            self.p, self.q = self.buf.data_ptr(), self.buf.data_ptr() + 16 * 4
        else:
            self.P, self.Q = (torch.full((N + 1, L), float("nan"), device="cuda") for _ in range(2))
            self.p, self.q = self.P.data_ptr(), self.Q.data_ptr()
        if P is not None:
            if self.blocked:
                v = self.buf[:N].view(N, 8, 2, 16)
                v[:, :, 0], v[:, :, 1] = P.view(N, 8, 16), Q.view(N, 8, 16)
            else:
                self.P[:N], self.Q[:N] = P, Q

    def unpack(self):
        N = self.N
        if not self.blocked:
            assert bool(self.P[N:].isnan().all()) and bool(self.Q[N:].isnan().all())
            return self.P[:N], self.Q[:N]
        assert bool(self.buf[N:].isnan().all())
        v = self.buf[:N].view(N, 8, 2, 16)
        return v[:, :, 0].reshape(N, L).contiguous(), v[:, :, 1].reshape(N, L).contiguous()


def producer(env, a1, W2, b2):
    """a2 = relu(W2 a1 + b2), its partials in a NaN-prefilled buffer as pdg_mlp2_fwd leaves them, *nparts and the
    finalized pdg_ln_stat: the real producer of the randn family."""
    lib, sh = env
    M = a1.shape[0]
    a2 = torch.empty(M, L, device="cuda")
    part = nan64(2 * lib.pdg_max_blocks())
    n = ctypes.c_int(0)
    assert lib.pdg_mlp2_fwd(M, p(a1), p(W2), p(b2), p(a2), p(part), ctypes.byref(n), sh()) == 0
    st = sentinel()
    assert lib.pdg_ln_finalize(p(part), n.value, float(M * L), p(st), sh()) == 0
    torch.cuda.synchronize()
    return a2, st, part, n.value


def check_rows(tag, n, got, r64, r32, keys, tol):
    """Relative L2 below tol and the per-row bound for the outputs `keys`; prints the figures
    profiles/fwd_op_errors.txt records."""
    bad = []
    for k in keys:
        g, a, b = getattr(got, k)[:n], getattr(r64, k), getattr(r32, k)
        mine, plain, e = worst_row(g, a), worst_row(b, a), rel(g, a)
        ratio = mine / plain if plain > 0 else (0.0 if mine == 0 else float("inf"))
        print(f"FWD {tag} {k}: rel {e:.2e} (bound {tol:.0e}) worst row {mine:.2e} / fp32 {plain:.2e} = {ratio:.2f}")
        if not (e < tol and mine <= ROW_FACTOR * plain):
            bad.append((k, e, mine, plain, ratio))
    assert not bad, (tag, bad)


def check_partials(tag, nb, part, sums, exact):
    assert bool(part.isfinite().all()), f"{tag}: a block left its partial unwritten"
    got = part.view(nb, 2).sum(0).cpu()
    s1, s2 = float(sums[0]), float(sums[1])
    if exact:
        assert float(got[0]) == s1 and float(got[1]) == s2, (tag, got.tolist(), s1, s2)
    else:   # a2 >= 0: sum |ref| = sum ref
        assert abs(float(got[0]) - s1) <= 1e-6 * abs(s1) and abs(float(got[1]) - s2) <= 1e-6 * s2, (tag, got.tolist(), s1, s2)


# ------------------------------------------------------------------------------------------ the edge kernels

class EdgeCase:
    """The inputs of one (E, family variant) on the device and its references per `res` (each made once, with the
    edge update: the message half is the eu = 0 reference)."""

    def __init__(self, env, E, variant):
        lib, sh = env
        kind, cond = variant
        self.E, self.exact = E, cond == "x"
        self.N, src, dst = F.graph_of(kind, E)
        self.src64, self.dst64 = src, dst
        self.src, self.dst = src.int().cuda(), dst.int().cuda()
        i = F.exact_edge_inputs(E, self.N) if self.exact else F.randn_edge_inputs(E, self.N, cond)
        self.i = i
        self.d = SimpleNamespace(**{k: cu(getattr(i, k)) for k in ("e_res", "W1", "b1", "W2", "b2", "g", "b")})
        self.pq = PQ(lib, self.N, cu(i.P), cu(i.Q))
        if self.exact:
            self.stat, self.a2p = F.UNIT, cu(i.a2_prev)
            self.st = pack_stat(F.UNIT)
        else:
            self.a2p, self.st, _, _ = producer(env, cu(i.a1p), cu(i.W2p), cu(i.b2p))
            self.stat = F.ln_stat_ref(self.a2p)
            assert rel(self.a2p, i.a2_prev) < TOL
            if cond == "c":
                assert 0.02 < 1e-5 / self.stat.std_d < 1.0   # eps counts in den
        self._ref = {}

    def ref(self, res, dtype):
        if (res, dtype) not in self._ref:
            i = self.i
            self._ref[(res, dtype)] = F.edge_step_ref(self.a2p, self.stat, i.g, i.b, i.e_res if res else None, self.src64,
                                                      self.dst64, i.P, i.Q, i.W1, i.b1, i.W2, i.b2, True, dtype)
        return self._ref[(res, dtype)]

    def run(self, env, kernel, nb, eu, res):
        """kernel: "coop" (a1m / a1e stored), "coop_inf" (a1m = a1e = NULL) or "infer"."""
        lib, sh = env
        E, d = self.E, self.d
        o = SimpleNamespace(e_t=nan_rows(E), a2m=nan_rows(E), a2e=nan_rows(E) if eu else None,
                            a1m=nan_rows(E) if kernel == "coop" else None,
                            a1e=nan_rows(E) if kernel == "coop" and eu else None,
                            part_m=nan64(2 * nb), part_e=nan64(2 * nb) if eu else None)
        head = (E, p(self.a2p), p(self.st), p(d.g), p(d.b), p(d.e_res) if res else None, p(o.e_t), p(self.src),
                p(self.dst), self.pq.p, self.pq.q, p(d.W1), p(d.b1), p(d.W2), p(d.b2))
        if kernel == "infer":
            assert lib.pdg_edge_fwd_infer(*head, p(o.a2m), p(o.a2e), p(o.part_m), p(o.part_e), eu, nb, sh()) == 0
        else:
            assert lib.pdg_edge_fwd_coop(*head, p(o.a1m), p(o.a2m), p(o.a1e), p(o.a2e), p(o.part_m), p(o.part_e), eu,
                                         nb, sh()) == 0
        torch.cuda.synchronize()
        return o


_edge = {}


def edge_case(env, E, variant):
    if (E, variant) not in _edge:
        _edge[(E, variant)] = EdgeCase(env, E, variant)
    return _edge[(E, variant)]


def edge_keys(kernel, eu):
    return ["e_t", "a2m"] + (["a2e"] if eu else []) + ((["a1m"] + (["a1e"] if eu else [])) if kernel == "coop" else [])


@pytest.mark.parametrize("kernel", ["coop", "coop_inf", "infer"])
@pytest.mark.parametrize("eu,res", FLAGS)
@pytest.mark.parametrize("E,nb", CASES)
def test_edge_fwd_integer_exact(env, E, nb, eu, res, kernel):
    """The integer-exact family on both graphs: every stored row equals the reference bit for bit, the rows past E
    stay NaN, every block's partial pair is written and the pairs sum to the integer totals exactly."""
    for kind in ("hub", "ends"):
        c = edge_case(env, E, (kind, "x"))
        r = c.ref(res, torch.float64)
        o = c.run(env, kernel, nb, eu, res)
        tag = f"{kernel} exact {kind} E={E} nb={nb} eu={eu} res={res}"
        for k in edge_keys(kernel, eu):
            got = getattr(o, k)
            assert tail_ok(E, got), (tag, k)
            want = getattr(r, k).float()
            assert torch.equal(got[:E].cpu(), want), (tag, k, int((got[:E].cpu() != want).any(1).sum()), "rows differ")
        check_partials(tag, nb, o.part_m, r.sums_m, True)
        if eu:
            check_partials(tag, nb, o.part_e, r.sums_e, True)


@pytest.mark.parametrize("kernel", ["coop", "coop_inf", "infer"])
@pytest.mark.parametrize("eu,res", FLAGS)
@pytest.mark.parametrize("E,nb", CASES)
def test_edge_fwd_vs_fp64(env, E, nb, eu, res, kernel):
    """The randn family in both conditionings against fp64 from the inputs: relative L2 (TOL in "p", TOL_LN in "c"),
    the per-row bound, the partial totals, the NaN rows past E."""
    for variant in VARIANTS:
        c = edge_case(env, E, variant)
        r64, r32 = c.ref(res, torch.float64), c.ref(res, torch.float32)
        o = c.run(env, kernel, nb, eu, res)
        tag = f"{kernel} {variant[1]} E={E} nb={nb} eu={eu} res={res}"
        keys = edge_keys(kernel, eu)
        assert all(tail_ok(E, getattr(o, k)) for k in keys), tag
        check_rows(tag, E, o, r64, r32, keys, TOL if variant[1] == "p" else TOL_LN)
        check_partials(tag, nb, o.part_m, r64.sums_m, False)
        if eu:
            check_partials(tag, nb, o.part_e, r64.sums_e, False)


# ------------------------------------------------------------------------------------------ the node kernels

class NodeCase:
    """fwd_ref.node_inputs on the device; a2n, its partials, *nparts and pdg_ln_stat from the real producer (randn) or
    integers with unit statistics (st: hand-packed; part / st_fin: unit partials and their pdg_ln_finalize)."""

    def __init__(self, env, N, cond):
        i = F.node_inputs(N, cond)
        self.__dict__.update(i.__dict__)
        self.exact = cond == "x"
        if self.exact:
            self.a2n, self.stat, self.st, self.nparts = cu(i.a2n), F.UNIT, pack_stat(F.UNIT), 37
            self.part, self.st_fin = unit_stats(env, 37, N * L)
        else:
            self.a2n, self.st, self.part, self.nparts = producer(env, cu(i.a1p), cu(i.W2p), cu(i.b2p))
            assert rel(self.a2n, i.a2n) < TOL
            self.stat, self.st_fin = F.ln_stat_ref(self.a2n), self.st
        self.d = SimpleNamespace(**{k: cu(getattr(self, k)) for k in ("x_res", "g", "b", "W1", "Wd1", "bd1", "Wd2", "bd2",
                                                                       "stats8")})


_node = {}


def node_case(env, N, cond):
    if (N, cond) not in _node:
        _node[(N, cond)] = NodeCase(env, N, cond)
    return _node[(N, cond)]


def run_node_pq(env, c, res, fin):
    lib, sh = env
    N, d = c.N, c.d
    o = SimpleNamespace(x_t=nan_rows(N), pq=PQ(lib, N), st=sentinel())
    tail = (p(d.g), p(d.b), p(d.x_res) if res else None, p(o.x_t), p(d.W1), o.pq.p, o.pq.q, sh())
    if fin:
        assert lib.pdg_node_pq_rw_fin(N, p(c.a2n), p(c.part), c.nparts, float(N * L), p(o.st), *tail) == 0
    else:
        assert lib.pdg_node_pq_rw(N, p(c.a2n), p(c.st), *tail) == 0
    torch.cuda.synchronize()
    o.P, o.Q = o.pq.unpack()
    return o


@pytest.mark.parametrize("res", [True, False])
@pytest.mark.parametrize("N,_nb", NODE_CASES)
def test_node_pq_rw_vs_fp64(env, N, _nb, res):
    """pdg_node_pq_rw and pdg_node_pq_rw_fin (partials and *nparts straight from the producer): integer-exact x_t, P,
    Q equal to the reference; randn in both conditionings within the bounds; the NaN row after node N - 1 of the
    P / Q buffer and the rows past N of x_t untouched; the statistics _fin stores equal to pdg_ln_finalize's."""
    for cond in ("x", "p", "c"):
        c = node_case(env, N, cond)
        xr = c.x_res if res else None
        r64 = F.node_pq_ref(c.a2n, c.stat, c.g, c.b, xr, c.W1)
        r32 = F.node_pq_ref(c.a2n, c.stat, c.g, c.b, xr, c.W1, torch.float32)
        for fin in (False, True):
            o = run_node_pq(env, c, res, fin)
            tag = f"node_pq_rw{'_fin' if fin else ''} {cond} N={N} res={int(res)}"
            assert tail_ok(N, o.x_t), tag
            if fin:
                assert torch.equal(o.st, c.st_fin), tag
            if cond == "x":
                for k in ("x_t", "P", "Q"):
                    assert torch.equal(getattr(o, k)[:N].cpu(), getattr(r64, k).float()), (tag, k)
            else:
                check_rows(tag, N, o, r64, r32, ("x_t", "P", "Q"), TOL if cond == "p" else TOL_LN)


@pytest.mark.parametrize("N,nb", NODE_CASES)
def test_decoder_fwd_coop_vs_fp64(env, N, nb):
    """pdg_decoder_fwd_coop with the statistics given and with pending partials (the engine's form): integer-exact
    x_S, a1d and y (scale_output = 0) equal to the reference; randn (scale_output = 1) within the bounds."""
    lib, sh = env
    for cond in ("x", "p", "c"):
        c = node_case(env, N, cond)
        d, scale = c.d, int(cond != "x")
        args = (c.a2n, c.stat, c.g, c.b, c.x_res, c.Wd1, c.bd1, c.Wd2, c.bd2, c.stats8, bool(scale))
        r64, r32 = F.decoder_ref(*args), F.decoder_ref(*args, torch.float32)
        for pend in (False, True):
            o = SimpleNamespace(x_S=nan_rows(N), a1d=nan_rows(N), y=nan_rows(N, 3), st=sentinel())
            assert lib.pdg_decoder_fwd_coop(N, p(c.a2n), None if pend else p(c.st), p(c.part) if pend else None,
                                            c.nparts if pend else 0, float(N * L), p(o.st) if pend else None, p(d.g),
                                            p(d.b), p(d.x_res), p(o.x_S), p(d.Wd1), p(d.bd1), p(o.a1d), p(d.Wd2),
                                            p(d.bd2), p(d.stats8), scale, p(o.y), nb, sh()) == 0
            torch.cuda.synchronize()
            tag = f"decoder_fwd_coop {cond} N={N} nb={nb} pend={int(pend)}"
            assert tail_ok(N, o.x_S) and tail_ok(N, o.a1d) and tail_ok(N, o.y), tag
            if pend:
                assert torch.equal(o.st, c.st_fin), tag
            if cond == "x":
                for k in ("x_S", "a1d", "y"):
                    assert torch.equal(getattr(o, k)[:N].cpu(), getattr(r64, k).float()), (tag, k)
            else:
                check_rows(tag, N, o, r64, r32, ("x_S", "a1d", "y"), TOL if cond == "p" else TOL_LN)


# ------------------------------------------------------------------------------------------ the statistics

@pytest.mark.parametrize("cond", ["p", "c"])
@pytest.mark.parametrize("nparts", NPARTS)
def test_ln_statistics_vs_the_array(env, nparts, cond):
    """pdg_ln_finalize, pdg_ln_finalize2 and the in-kernel reducers of pdg_node_pq_rw_fin, pdg_segment_sum_fin and
    pdg_decoder_fwd_coop on the fp64 row-slice sums of an array: mean_d / std_d against the two-pass statistics of
    the array itself, the fp32 fields bitwise from the stored fp64 pair (rstd within 1 ulp of 1 / den), count exact,
    the reducers bitwise pdg_ln_finalize.
    The bounds (fwd_ref.stat_bound, derived there from the one-pass formula's cancellation): K u on mean_d, K u (1 +
    mean^2 / var) on std_d, relative, with K = log2(n) + nparts / 256 + 16 roundings; both below TOL_STAT = 1e-9 for
    these arrays (tests/test_fwd_ref.py checks that without a device; asserted here too)."""
    lib, sh = env
    assert max(NPARTS) == lib.pdg_max_blocks()
    a, ref = F.stat_array(cond)
    n = a.numel()
    b_mean, bound = F.stat_bound(n, nparts, ref)
    assert b_mean <= bound < TOL_STAT
    edges = torch.linspace(0, STAT_ROWS, nparts + 1).round().long().tolist()
    a64 = a.double()

    def partials(x):
        return torch.stack([torch.stack([x[i:j].sum(), x[i:j].square().sum()])
                            for i, j in zip(edges[:-1], edges[1:])]).reshape(-1).cuda()
    pa, pb = partials(a64), partials(a64.flip(0) * 0.5)
    refb = F.ln_stat_ref(a64 * 0.5)
    st = sentinel()
    assert lib.pdg_ln_finalize(p(pa), nparts, float(n), p(st), sh()) == 0
    sa, sb = sentinel(), sentinel()
    assert lib.pdg_ln_finalize2(p(pa), p(pb), nparts, float(n), p(sa), p(sb), sh()) == 0
    torch.cuda.synchronize()
    assert torch.equal(sa, st)
    for which, buf, r in (("a", st, ref), ("b", sb, refb)):
        s = stat_from(buf)
        e_mean, e_std = abs(s.mean_d - r.mean_d) / abs(r.mean_d), abs(s.std_d - r.std_d) / r.std_d
        print(f"FWD ln_finalize {cond} nparts={nparts} part_{which}: mean_d {e_mean:.2e} std_d {e_std:.2e} (bound {bound:.2e})")
        assert e_mean <= b_mean and e_std <= bound, (e_mean, e_std, bound)
        mean, std_, den, rstd = F.fp32_fields(s.mean_d, s.std_d)
        assert (s.mean, s.std_, s.den) == (mean, std_, den) and s.count == float(n)
        ulp = float(torch.nextafter(torch.tensor(rstd), torch.tensor(float("inf"))) - torch.tensor(rstd))
        assert abs(s.rstd - rstd) <= ulp, (s.rstd, rstd)
    # the in-kernel reducers: 7 rows of work, the statistics' own count
    c = node_case(env, 7, "p")
    d = c.d
    o = SimpleNamespace(x=nan_rows(7), pq=PQ(lib, 7), st=sentinel())
    assert lib.pdg_node_pq_rw_fin(7, p(c.a2n), p(pa), nparts, float(n), p(o.st), p(d.g), p(d.b), p(d.x_res), p(o.x), p(d.W1),
                                  o.pq.p, o.pq.q, sh()) == 0
    dst = torch.zeros(7, L, device="cuda"), torch.zeros(7, L, device="cuda"), torch.zeros(7, 3, device="cuda")
    s_dec = sentinel()
    assert lib.pdg_decoder_fwd_coop(7, p(c.a2n), None, p(pa), nparts, float(n), p(s_dec), p(d.g), p(d.b), p(d.x_res),
                                    p(dst[0]), p(d.Wd1), p(d.bd1), p(dst[1]), p(d.Wd2), p(d.bd2), p(d.stats8), 0,
                                    p(dst[2]), 37, sh()) == 0
    rp = torch.tensor([0, 1, 1, 3, 4, 5, 6, 7], dtype=torch.int32, device="cuda")
    s_a, s_b = sentinel(), sentinel()
    assert lib.pdg_segment_sum_fin(7, p(rp), p(c.a2n), p(pa), p(pb), nparts, float(n), p(s_a), p(s_b), p(d.g), p(d.b),
                                   p(dst[0]), p(dst[1]), sh()) == 0
    torch.cuda.synchronize()
    assert torch.equal(o.st, st) and torch.equal(s_dec, st) and torch.equal(s_a, st) and torch.equal(s_b, sb)


# ------------------------------------------------------------------------------------------ pdg_segment_sum(_fin)

class SegCase:
    """fwd_ref.seg_inputs on the device, three NaN rows after the rows; statistics as NodeCase's."""

    def __init__(self, env, N, cond):
        i = F.seg_inputs(N, cond)
        self.N, self.E, self.exact, self.dst64, self.g, self.b = N, i.E, cond == "x", i.dst, i.g, i.b
        self.rp, self.deg0 = i.rowptr.int().cuda(), i.deg == 0
        E = self.E
        self.rows = nan_rows(E)
        if self.exact:
            self.rows[:E] = cu(i.rows)
            self.stat, self.st, self.nparts = F.UNIT, pack_stat(F.UNIT), 37
            self.part, self.st_fin = unit_stats(env, 37, max(E, 1) * L)
        else:
            a2, self.st, self.part, self.nparts = producer(env, cu(i.a1p), cu(i.W2p), cu(i.b2p))
            assert rel(a2, i.rows) < TOL
            self.rows[:E] = a2
            self.stat, self.st_fin = F.ln_stat_ref(a2), self.st
        self.gd, self.bd = cu(self.g), cu(self.b)

    def run(self, env, form, fin=None):
        """form: "ln_xs", "ln" (xhat_sum = NULL) or "raw" (no LayerNorm); fin: None, "a" or "ab"."""
        lib, sh = env
        N = self.N
        o = SimpleNamespace(aggr=nan_rows(N), xs=nan_rows(N) if form == "ln_xs" else None, st_a=sentinel(), st_b=sentinel())
        if fin:
            assert lib.pdg_segment_sum_fin(N, p(self.rp), p(self.rows), p(self.part), p(self.part) if fin == "ab" else None,
                                           self.nparts, float(max(self.E, 1) * L), p(o.st_a), p(o.st_b) if fin == "ab" else None,
                                           p(self.gd), p(self.bd), p(o.aggr), p(o.xs), sh()) == 0
        else:
            ln = form != "raw"
            assert lib.pdg_segment_sum(N, p(self.rp), p(self.rows), p(self.st) if ln else None, p(self.gd) if ln else None,
                                       p(self.bd) if ln else None, p(o.aggr), p(o.xs), sh()) == 0
        torch.cuda.synchronize()
        return o


def seg_sizes():
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    return 64 * cus + 9


@pytest.mark.parametrize("N", [1, 8, 9, 77, "grid"])
def test_segment_sum_vs_fp64(env, N):
    """pdg_segment_sum and pdg_segment_sum_fin on the hand-built CSR (N = "grid": 64 x CUs + 9 nodes, the smallest N
    at which a half-wave takes a second grid-stride pass), in the three forms, _fin with and without part_b:
    integer-exact equal to the reference; randn within the bounds (TOL, the bound of test_gpu_ops.py's segment-sum
    test, also for the 300-row hub: its row-by-row fp32 sum comes to 0.57 of TOL, as the fp32 restatement's does);
    nodes without an edge exactly 0; the rows past N untouched; sentinel-filled st_a / st_b afterwards hold pdg_ln_finalize's statistics of the producer's partials."""
    N = seg_sizes() if N == "grid" else N
    for cond in ("x", "p", "c"):
        if N == 1 and cond != "x":
            continue   # no rows: nothing for the producer to make
        c = SegCase(env, N, cond)
        ref = {}
        for dtype in (torch.float64, torch.float32):
            aggr, xs = F.segment_sum_ref(c.dst64, c.rows[:c.E], c.stat, c.g, c.b, N, dtype)
            raw, _ = F.segment_sum_ref(c.dst64, c.rows[:c.E], None, None, None, N, dtype)
            ref[dtype] = SimpleNamespace(aggr=aggr, xs=xs, raw=raw)
        runs = [("ln_xs", None), ("ln", None), ("raw", None)] + ([("ln_xs", "a"), ("ln_xs", "ab"), ("ln", "ab")] if c.E else [])
        for form, fin in runs:
            o = c.run(env, form, fin)
            tag = f"segment_sum{'_fin' if fin else ''} {cond} N={N} {form} fin={fin}"
            keys = ["aggr"] + (["xs"] if form == "ln_xs" else [])
            if form == "raw":
                o.raw, keys = o.aggr, ["raw"]
            for k in keys:
                got = getattr(o, k)
                assert tail_ok(N, got), (tag, k)
                assert float(got[:N].cpu()[c.deg0].abs().max()) == 0.0, (tag, k)
            if cond == "x":
                for k in keys:
                    assert torch.equal(getattr(o, k)[:N].cpu(), getattr(ref[torch.float64], k).float()), (tag, k)
            else:
                check_rows(tag, N, o, ref[torch.float64], ref[torch.float32], keys, TOL if cond == "p" else TOL_LN)
            if fin:
                for buf in (o.st_a,) + ((o.st_b,) if fin == "ab" else ()):
                    assert torch.equal(buf, c.st_fin), tag
                if fin == "a":
                    assert torch.equal(o.st_b, sentinel()), tag


# ------------------------------------------------------------------------------------------ the engine's chain

@pytest.mark.parametrize("edge_kernel", ["coop", "infer"])
@pytest.mark.parametrize("E", [77, 4099])
def test_engine_order_chain_vs_oracle(env, E, edge_kernel):
    """Two message-passing steps in the engine's order and buffer hand-over on hub_graph(E): pdg_node_enc_fwd (partials
    -> part_b), pdg_edge_enc_fwd (-> part_a) + pdg_ln_finalize, then per step pdg_node_pq_rw_fin (pending partials),
    the edge forward on 256 blocks (-> part_a / part_b), pdg_segment_sum_fin, pdg_node_net (-> part_a, *nparts as
    returned), and pdg_decoder_fwd_coop with pending partials; part_a / part_b NaN-filled before the first use.  y
    against oracle.epd_oracle in fp64 on the same parameters and every stored statistic against the fp64 chain's:
    y's worst row within ROW_FACTOR x the fp32 fwd_ref chain's; a statistic of an array A within ROW_FACTOR x the
    rms error of the fp32 chain's A (an rms change delta of an array moves its mean and its std by at most delta)."""
    lib, sh = env
    s, NB = sh(), 256
    N, src, dst, rp = hub_graph(E)[:4]
    gen = torch.Generator().manual_seed(E)
    prm = {k: v.float() for k, v in O.init_params(seed=11).items()}
    for k in prm:
        if k.endswith(".4.weight") or k.endswith(".4.bias"):
            prm[k] = prm[k] + 0.2 * torch.randn(L, generator=gen)
    x_in, e_in = torch.randn(N, 6, generator=gen), torch.randn(E, 1, generator=gen)
    stats8 = torch.tensor([0.1, 1.2, -0.3, 2.0, 0.25, 3.5, 0.05, 0.7])
    P = {k: v.contiguous().cuda() for k, v in prm.items()}
    w = lambda k: p(P[k])
    src_d, dst_d, rp_d = src.int().cuda(), dst.int().cuda(), rp.int().cuda()
    part_a, part_b = nan64(2 * lib.pdg_max_blocks()), nan64(2 * lib.pdg_max_blocks())
    st = {k: sentinel() for k in ("ne", "ee", "m0", "e0", "n0", "m1", "n1")}
    emp = lambda *sh_: torch.empty(*sh_, device="cuda")
    a2n, a2e = emp(N, L), emp(E, L)
    x_d, e_d, st8 = x_in.cuda(), e_in.reshape(-1).contiguous().cuda(), stats8.cuda()
    assert lib.pdg_node_enc_fwd(N, p(x_d), w("node_encoder.0.weight"), w("node_encoder.0.bias"), w("node_encoder.2.weight"),
                                w("node_encoder.2.bias"), None, p(a2n), p(part_b), NB, s) == 0
    pend_buf, pend_n = part_b, NB
    assert lib.pdg_edge_enc_fwd(E, p(e_d), w("edge_encoder.0.weight"), w("edge_encoder.0.bias"), w("edge_encoder.2.weight"),
                                w("edge_encoder.2.bias"), p(a2e), p(part_a), NB, s) == 0
    assert lib.pdg_ln_finalize(p(part_a), NB, float(E * L), p(st["ee"]), s) == 0
    ln_n, ln_e, st_n, st_e = "node_encoder.4", "edge_encoder.4", st["ne"], st["ee"]
    x_res = e_res = None
    n = ctypes.c_int(0)
    for t in range(2):
        eu = int(t == 0)
        x_t, pq, e_t = emp(N, L), PQ(lib, N), emp(E, L)
        assert lib.pdg_node_pq_rw_fin(N, p(a2n), p(pend_buf), pend_n, float(N * L), p(st_n), w(ln_n + ".weight"),
                                      w(ln_n + ".bias"), p(x_res), p(x_t), w("processor.edge_net.0.weight"), pq.p, pq.q, s) == 0
        a2m, a2e_new = emp(E, L), emp(E, L) if eu else None
        head = (E, p(a2e), p(st_e), w(ln_e + ".weight"), w(ln_e + ".bias"), p(e_res), p(e_t), p(src_d), p(dst_d), pq.p,
                pq.q, w("processor.edge_net.0.weight"), w("processor.edge_net.0.bias"), w("processor.edge_net.2.weight"),
                w("processor.edge_net.2.bias"))
        if edge_kernel == "infer":
            assert lib.pdg_edge_fwd_infer(*head, p(a2m), p(a2e_new), p(part_a), p(part_b), eu, NB, s) == 0
        else:
            a1m, a1e = emp(E, L), emp(E, L) if eu else None
            assert lib.pdg_edge_fwd_coop(*head, p(a1m), p(a2m), p(a1e), p(a2e_new), p(part_a), p(part_b), eu, NB, s) == 0
        aggr, xs = emp(N, L), emp(N, L)
        assert lib.pdg_segment_sum_fin(N, p(rp_d), p(a2m), p(part_a), p(part_b) if eu else None, NB, float(E * L),
                                       p(st[f"m{t}"]), p(st["e0"]) if eu else None, w("processor.edge_net.4.weight"),
                                       w("processor.edge_net.4.bias"), p(aggr), p(xs), s) == 0
        a2n = emp(N, L)
        assert lib.pdg_node_net(N, p(aggr), p(x_t), w("processor.node_net.0.weight"), w("processor.node_net.0.bias"),
                                w("processor.node_net.2.weight"), w("processor.node_net.2.bias"), None, p(a2n), p(part_a),
                                ctypes.byref(n), s) == 0
        pend_buf, pend_n = part_a, n.value
        x_res, e_res, a2e = x_t, e_t, a2e_new
        ln_n, ln_e, st_n, st_e = "processor.node_net.4", "processor.edge_net.4", st[f"n{t}"], st["e0"]
    y, x_S, a1d = nan_rows(N, 3), emp(N, L), emp(N, L)
    assert lib.pdg_decoder_fwd_coop(N, p(a2n), None, p(pend_buf), pend_n, float(N * L), p(st_n), w(ln_n + ".weight"),
                                    w(ln_n + ".bias"), p(x_res), p(x_S), w("node_decoder.0.weight"), w("node_decoder.0.bias"),
                                    p(a1d), w("node_decoder.2.weight"), w("node_decoder.2.bias"), p(st8), 1, p(y), NB, s) == 0
    torch.cuda.synchronize()
    assert tail_ok(N, y)
    # fp64: the oracle's own pieces for y, the fwd_ref chain (equal to them, tests/test_fwd_ref.py) for the statistics
    p64 = {k: v.double() for k, v in prm.items()}
    ei = torch.stack([src, dst])
    xo, eo = O._mlp(x_in.double(), p64, "node_encoder"), O._mlp(e_in.double(), p64, "edge_encoder")
    for _ in range(2):
        xo, eo = O.processor_step(p64, xo, eo, ei)
    y64 = O._mlp(xo, p64, "node_decoder", layer_norm=False) * float(stats8[5]) + float(stats8[4])
    enc64, r64, d64 = F.forward_ref(prm, x_in, e_in, src, dst, 2, stats8, True)
    enc32, r32, d32 = F.forward_ref(prm, x_in, e_in, src, dst, 2, stats8, True, torch.float32)
    assert rel(d64.y, y64) < 1e-12
    mine, plain = worst_row(y[:N], y64), worst_row(d32.y, y64)
    print(f"FWD chain {edge_kernel} E={E} N={N} y: rel {rel(y[:N], y64):.2e} worst row {mine:.2e} / fp32 {plain:.2e} = "
          f"{mine / plain:.2f}")
    assert mine <= ROW_FACTOR * plain, (mine, plain)
    arrays = {"ne": (enc64.a2n, enc32.a2n), "ee": (enc64.a2e, enc32.a2e), "m0": (r64[0].a2m, r32[0].a2m),
              "e0": (r64[0].a2e, r32[0].a2e), "n0": (r64[0].a2n, r32[0].a2n), "m1": (r64[1].a2m, r32[1].a2m),
              "n1": (r64[1].a2n, r32[1].a2n)}
    for k, (a64, a32) in arrays.items():
        got, want = stat_from(st[k]), F.ln_stat_ref(a64)
        delta = float((a32.double() - a64).pow(2).mean().sqrt())
        e_mean, e_std = abs(got.mean_d - want.mean_d), abs(got.std_d - want.std_d)
        print(f"FWD chain {edge_kernel} E={E} stat {k}: mean_d {e_mean:.2e} std_d {e_std:.2e} / fp32 rms {delta:.2e} = "
              f"{max(e_mean, e_std) / delta:.2f}")
        assert got.count == float(a64.numel())
        assert e_mean <= ROW_FACTOR * delta and e_std <= ROW_FACTOR * delta, (k, e_mean, e_std, delta)
        assert (got.mean, got.std_, got.den) == F.fp32_fields(got.mean_d, got.std_d)[:3]
