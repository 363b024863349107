"""The tangent-pass kernels at the op level (csrc/pdg_tangent.hip) against the float64 restatements of
tests/tangent_ref.py (anchored to torch.func.jvp by tests/test_tangent_ref.py).

Shapes: (rows 200, nblocks 3): several 32-row rounds per block with a ragged last one; (rows 37, nblocks 256):
mostly empty blocks, which read the last row and must store nothing.  Every output array has NaN guard rows
past its end, every pair buffer NaN past its count.  The pre-LayerNorm tangents are drawn with a non-zero mean
and a component along (a - mu), so both LayerNorm terms matter (asserted).  The consumers take pairs split
unevenly over 5 blocks; the producers' partials are compared with the fp64 sums.

Bound: 3e-6 relative L2 per output, the order of the bf16x6 op tests against fp64.  The (T1, T2) partials: each
da is within 3e-6 in L2, so |dT1| <= sqrt(n) |d da|_2 and |dT2| <= |a - mu|_2 |d da|_2 (Cauchy-Schwarz).

The second half of the file pins the same kernels at the row schedule's edges, in three input families, at every
pair count, on a hand-built CSR and in the engine's chain; its shapes and bounds are stated where it starts."""
import pytest
import torch

import tangent_ref as R

pytestmark = pytest.mark.gpu

L = 128
SHAPES = [(200, 3), (37, 256)]
TOL = 3e-6
NPAIRS = 5
NN = 53   # nodes of the edge / aggregation cases


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pdg.lib import lib, stream_handle
    return lib, stream_handle


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def rnd(gen, *shape, shift=0.0):
    return (torch.randn(*shape, dtype=torch.float64, generator=gen) + shift).float().cuda()


def guarded(rows, cols=L):
    return torch.full((rows + 3, cols), float("nan"), device="cuda")


def ln_stat(env, a):
    """pdg_ln_stat of the tensor `a` through pdg_ln_finalize from its fp64 (sum, sum of squares)."""
    lib, sh = env
    ad = a.double()
    part = torch.stack([ad.sum(), (ad * ad).sum()]).cuda()
    st = torch.zeros(40, dtype=torch.uint8, device="cuda")
    lib.pdg_ln_finalize(part.data_ptr(), 1, float(a.numel()), st.data_ptr(), sh())
    torch.cuda.synchronize()
    return st


def split_pairs(env, da, a, gen):
    """(T1, T2) of (da, a) in fp64 split unevenly over NPAIRS blocks, NaN past them."""
    lib, _ = env
    t1, t2 = R.pairs_ref(da, a)
    w = torch.rand(NPAIRS, dtype=torch.float64, generator=gen) + 0.1
    w = w / w.sum()
    buf = torch.full((2 * lib.pdg_max_blocks(),), float("nan"), dtype=torch.float64)
    buf[0:2 * NPAIRS:2] = t1 * w
    buf[1:2 * NPAIRS:2] = t2 * w
    return buf.cuda()


def part_buf(env):
    lib, _ = env
    return torch.full((2 * lib.pdg_max_blocks(),), float("nan"), dtype=torch.float64, device="cuda")


def check_partials(name, part, nblocks, da_ref, a):
    p = part.cpu()
    assert torch.isfinite(p[:2 * nblocks]).all() and torch.isnan(p[2 * nblocks:]).all(), name
    t1, t2 = R.pairs_ref(da_ref, a)
    n2 = float(da_ref.norm())
    xc = a.double().cpu() - a.double().cpu().mean()
    e1, e2 = abs(float(p[0:2 * nblocks:2].sum() - t1)), abs(float(p[1:2 * nblocks:2].sum() - t2))
    b1, b2 = TOL * a.numel() ** 0.5 * n2, TOL * float(xc.norm()) * n2
    print(f"{name}: T1 err {e1:.2e} (bound {b1:.2e}), T2 err {e2:.2e} (bound {b2:.2e})")
    assert e1 <= b1 and e2 <= b2, (name, e1, b1, e2, b2)


def check(name, got, ref, rows):
    assert torch.isnan(got[rows:]).all(), f"{name}: wrote past the end"
    e = rel(got[:rows], ref)
    print(f"{name}: {e:.2e} (bound {TOL:.0e})")
    assert e <= TOL, (name, e)


class Case:
    """Operands of one (rows, nblocks) shape, shared by the tests."""

    def __init__(self, env, M, nblocks):
        gen = torch.Generator().manual_seed(9100 + M)
        self.M, self.nblocks, self.gen = M, nblocks, gen
        lin = lambda o, i: (rnd(gen, o, i) / i ** 0.5).contiguous()
        self.W0n, self.w0e, self.b0e = lin(L, 6), rnd(gen, L), rnd(gen, L) * 0.5
        self.W2, self.We1, self.Wn1, self.Wd1, self.Wd2 = lin(L, L), lin(L, 3 * L), lin(L, 2 * L), lin(L, L), lin(3, L)
        self.g = rnd(gen, L) * 0.3 + 1.0
        act = lambda: torch.relu(rnd(gen, M, L, shift=0.3))
        self.a1, self.a2, self.a1b, self.a2b = act(), act(), act(), act()
        self.a_prev = act() * 1.7                    # the LayerNorm input of the consumers
        self.st2, self.st2b, self.st_prev = ln_stat(env, self.a2), ln_stat(env, self.a2b), ln_stat(env, self.a_prev)
        xc = self.a_prev - self.a_prev.mean()
        self.da_prev = rnd(gen, M, L, shift=0.7) + 0.5 * xc
        t1, t2 = R.pairs_ref(self.da_prev, self.a_prev)
        # both LayerNorm terms matter: T1 / n of the order of da, T2 well away from zero
        assert abs(float(t1)) / self.da_prev.numel() > 0.3
        assert abs(float(t2)) > 0.2 * float(self.da_prev.double().norm() * xc.double().norm())
        self.pairs = split_pairs(env, self.da_prev, self.a_prev, gen)
        self.res = rnd(gen, M, L)
        self.rows2 = rnd(gen, M, L)                  # a second tangent operand (daggr)
        self.dx_in, self.de_in, self.e_in = rnd(gen, M, 6), rnd(gen, M), rnd(gen, M)
        # the edge case: M edges over NN nodes, dst-sorted with empty nodes
        dst = torch.sort(torch.randint(0, NN - 3, (M,), generator=gen)).values
        self.src = torch.randint(0, NN, (M,), generator=gen).int().cuda()
        self.dst = dst.int().cuda()
        rp = torch.zeros(NN + 1, dtype=torch.long)
        rp[1:] = torch.cumsum(torch.bincount(dst, minlength=NN), 0)
        self.rowptr = rp.int().cuda()
        self.dP, self.dQ = rnd(gen, NN, L), rnd(gen, NN, L)


_cases = {}


def case(env, M, nblocks):
    if (M, nblocks) not in _cases:
        _cases[(M, nblocks)] = Case(env, M, nblocks)
    return _cases[(M, nblocks)]


def p(t):
    return None if t is None else t.data_ptr()


@pytest.mark.parametrize("M,nblocks", SHAPES)
def test_node_enc_tan(env, M, nblocks):
    lib, sh = env
    c = case(env, M, nblocks)
    out, part = guarded(M), part_buf(env)
    lib.pdg_node_enc_tan(M, p(c.dx_in), p(c.a1), p(c.W0n), p(c.W2), p(c.a2), p(c.st2), p(out), p(part), nblocks, sh())
    torch.cuda.synchronize()
    ref = R.node_enc_tan_ref(c.dx_in, c.a1, c.W0n, c.W2, c.a2)
    check(f"node_enc_tan M={M} blocks={nblocks}", out, ref, M)
    check_partials("node_enc_tan partials", part, nblocks, ref, c.a2)


@pytest.mark.parametrize("M,nblocks", SHAPES)
def test_edge_enc_tan(env, M, nblocks):
    lib, sh = env
    c = case(env, M, nblocks)
    out, part = guarded(M), part_buf(env)
    lib.pdg_edge_enc_tan(M, p(c.de_in), p(c.e_in), p(c.w0e), p(c.b0e), p(c.W2), p(c.a2), p(c.st2), p(out), p(part),
                         nblocks, sh())
    torch.cuda.synchronize()
    ref = R.edge_enc_tan_ref(c.de_in, c.e_in, c.w0e, c.b0e, c.W2, c.a2)
    check(f"edge_enc_tan M={M} blocks={nblocks}", out, ref, M)
    check_partials("edge_enc_tan partials", part, nblocks, ref, c.a2)


@pytest.mark.parametrize("res", [True, False])
@pytest.mark.parametrize("M,nblocks", SHAPES)
def test_node_pre_tan(env, M, nblocks, res):
    lib, sh = env
    c = case(env, M, nblocks)
    dx, dP, dQ = guarded(M), guarded(M), guarded(M)
    r = c.res if res else None
    lib.pdg_node_pre_tan(M, p(c.da_prev), p(c.a_prev), p(c.st_prev), p(c.pairs), NPAIRS, p(c.g), p(r), p(dx),
                         p(c.We1), p(dP), p(dQ), nblocks, sh())
    torch.cuda.synchronize()
    rx, rP, rQ = R.node_pre_tan_ref(c.da_prev, c.a_prev, c.g, r, c.We1)
    for nm, got, ref in (("dx", dx, rx), ("dP", dP, rP), ("dQ", dQ, rQ)):
        check(f"node_pre_tan {nm} M={M} blocks={nblocks} res={res}", got, ref, M)


@pytest.mark.parametrize("res", [True, False])
@pytest.mark.parametrize("eu", [True, False])
@pytest.mark.parametrize("M,nblocks", SHAPES)
def test_edge_tan(env, M, nblocks, eu, res):
    lib, sh = env
    c = case(env, M, nblocks)
    outs = []
    for _ in range(2):   # twice: bitwise the same
        de, da2m, da2e = guarded(M), guarded(M), guarded(M)
        pm, pe = part_buf(env), part_buf(env)
        r = c.res if res else None
        lib.pdg_edge_tan(M, NN, p(c.da_prev), p(c.a_prev), p(c.st_prev), p(c.pairs), NPAIRS, p(c.g), p(r), p(de),
                         p(c.src), p(c.dst), p(c.dP), p(c.dQ), p(c.We1), p(c.W2), p(c.a1), p(c.a2), p(c.st2),
                         p(c.a1b) if eu else None, p(c.a2b) if eu else None, p(c.st2b) if eu else None, p(da2m),
                         p(da2e) if eu else None, p(pm), p(pe) if eu else None, int(eu), nblocks, sh())
        torch.cuda.synchronize()
        outs.append((de, da2m, da2e, pm, pe))
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int64),
                           b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int64))
    de, da2m, da2e, pm, pe = outs[0]
    rde, rm, re_ = R.edge_tan_ref(c.da_prev, c.a_prev, c.g, r, c.src, c.dst, c.dP, c.dQ, c.We1, c.W2, c.a1, c.a2,
                                  c.a1b if eu else None, c.a2b if eu else None)
    tag = f"M={M} blocks={nblocks} eu={eu} res={res}"
    check(f"edge_tan de {tag}", de, rde, M)
    check(f"edge_tan da2m {tag}", da2m, rm, M)
    check_partials("edge_tan part_m", pm, nblocks, rm, c.a2)
    if eu:
        check(f"edge_tan da2e {tag}", da2e, re_, M)
        check_partials("edge_tan part_e", pe, nblocks, re_, c.a2b)
    else:   # no edge update: its outputs untouched
        assert torch.isnan(da2e).all() and torch.isnan(pe).all()


@pytest.mark.parametrize("M,nblocks", SHAPES)
def test_segment_sum_tan(env, M, nblocks):
    lib, sh = env
    c = case(env, M, nblocks)
    out = guarded(NN)
    lib.pdg_segment_sum_tan(NN, M, p(c.rowptr), p(c.da_prev), p(c.a_prev), p(c.st_prev), p(c.pairs), NPAIRS, p(c.g),
                            p(out), nblocks, sh())
    torch.cuda.synchronize()
    ref = R.segment_sum_tan_ref(c.rowptr, c.da_prev, c.a_prev, c.g)
    check(f"segment_sum_tan M={M} blocks={nblocks}", out, ref, NN)
    empty = (c.rowptr[1:] == c.rowptr[:-1]).cpu()
    assert empty.any() and float(out[:NN][empty].abs().max()) == 0.0


@pytest.mark.parametrize("M,nblocks", SHAPES)
def test_node_net_tan(env, M, nblocks):
    lib, sh = env
    c = case(env, M, nblocks)
    out, part = guarded(M), part_buf(env)
    lib.pdg_node_net_tan(M, p(c.rows2), p(c.res), p(c.Wn1), p(c.W2), p(c.a1), p(c.a2), p(c.st2), p(out), p(part),
                         nblocks, sh())
    torch.cuda.synchronize()
    ref = R.node_net_tan_ref(c.rows2, c.res, c.Wn1, c.W2, c.a1, c.a2)
    check(f"node_net_tan M={M} blocks={nblocks}", out, ref, M)
    check_partials("node_net_tan partials", part, nblocks, ref, c.a2)


@pytest.mark.parametrize("scale", [1, 0])
@pytest.mark.parametrize("res", [True, False])
@pytest.mark.parametrize("M,nblocks", SHAPES)
def test_decoder_tan(env, M, nblocks, res, scale):
    lib, sh = env
    c = case(env, M, nblocks)
    out = guarded(M, 3)
    std = torch.tensor([2.75], device="cuda")
    r = c.res if res else None
    lib.pdg_decoder_tan(M, p(c.da_prev), p(c.a_prev), p(c.st_prev), p(c.pairs), NPAIRS, p(c.g), p(r), p(c.Wd1),
                        p(c.a1), p(c.Wd2), p(std) if scale else None, scale, p(out), nblocks, sh())
    torch.cuda.synchronize()
    ref = R.decoder_tan_ref(c.da_prev, c.a_prev, c.g, r, c.Wd1, c.a1, c.Wd2, 2.75 if scale else None)
    check(f"decoder_tan M={M} blocks={nblocks} res={res} scale={scale}", out, ref, M)


def test_edge_len_tan_within_4_ulp(env):
    """fp32 rounding of the closed form: <= 4 ulp of the fp64 value per element, exact zeros on zero lengths
    (coincident endpoints and periodic pairs of distinct nodes)."""
    lib, sh = env
    gen = torch.Generator().manual_seed(9200)
    N, E = 61, 777
    pos, dpos = rnd(gen, N, 2) * 10, rnd(gen, N, 2)
    src, dst = torch.randint(0, N, (E,), generator=gen), torch.randint(0, N, (E,), generator=gen)
    src[:9] = dst[:9]
    ln = (pos.cpu().double()[src] - pos.cpu().double()[dst]).norm(dim=1).float()
    ln[9:20] = 0.0
    out = torch.full((E + 3,), float("nan"), device="cuda")
    sd, dd, lnd = src.cuda(), dst.cuda(), ln.cuda()
    lib.pdg_edge_len_tan(E, N, p(sd), p(dd), p(pos), p(dpos), p(lnd), p(out), sh())
    torch.cuda.synchronize()
    ref = R.edge_len_tan_ref(src, dst, pos, dpos, ln)
    got = out[:E].double().cpu()
    assert torch.isnan(out[E:]).all()
    assert float(got[:20].abs().max()) == 0.0 and int((ln == 0).sum()) >= 20
    ulp = 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(1e-300))) - 23)
    worst = float(((got - ref).abs() / ulp)[ln > 0].max())
    print(f"edge_len_tan: worst {worst:.2f} ulp (bound 4)")
    assert worst <= 4.0


# =====================================================================================================================
# The row schedule's edges, three input families, npairs, the hand-built CSR and the engine's chain.
#
# Shapes (rows, nblocks) of the six row kernels.  block_rows gives a block ceil(rows / nblocks) rows rounded up to the
# 32-row round, walked as two 16-row halves (rows rg and rg + 16 of the round):
#   (1, 1) (15, 1) (16, 1) (17, 1)   a half round short by one, exact, one past
#   (31, 1) (32, 1) (33, 1)          the same for the round: (33, 1) is a second round of one row
#   (33, 2) (64, 2) (65, 2)          per = 32: a one-row block after a full one, two full ones; per = 64: two rounds and
#                                    a one-row block
#   (77, 37)                         per = 32: 32, 32, 13 rows and 34 empty blocks
#   (4099, 37)                       per = 128: block 32 holds 3 rows, blocks 33 - 36 are empty
#   (37, 256)                        per = 32: 32 and 5 rows, 254 empty blocks
#   (8193, 256) (8209, 256)          per = 64: 128 full two-round blocks, block 128 with 1 / 17 rows, 127 empty blocks
# Families (tangent_ref.tan_inputs): "x" integer-exact with hand-packed unit statistics and the hand-made pairs of
# tangent_ref.exact_pairs (c1 = EXACT_K, c2 = 0): outputs and partial totals EQUAL the fp64 reference; "p" / "c" randn
# with a_prev, a2, a2b and their pdg_ln_stat from the real producer (pdg_mlp2_fwd + pdg_ln_finalize) at sigma ~ 0.6 /
# ~ 5e-5.  Every reference is evaluated with the pairs' totals and the stored statistics the kernel was handed.
# Bounds: "p" TOL = 3e-6; "c", for what lies downstream of the small-sigma LayerNorm, ROW_FACTOR x the distance of
# the fp32 restatement of the same output from fp64 (itself asserted below TOL_LN = 1e-5), TOL for the rest; per row
# in both, the worst row within ROW_FACTOR x the fp32 restatement's.  Measured (profiles/tangent_op_errors.txt): worst-
# row ratios 0.24 - 1.14, and 1.85 / 2.11 for pdg_decoder_tan's three values at one row; kernel / bound at most 0.53.
import ctypes
import struct
from types import SimpleNamespace

from edge_bwd_ref import worst_row

EDGE_SHAPES = [(1, 1), (15, 1), (16, 1), (17, 1), (31, 1), (32, 1), (33, 1), (33, 2), (64, 2), (65, 2), (77, 37),
               (4099, 37), (37, 256), (8193, 256), (8209, 256)]
ROW_FACTOR, TOL_LN = R.ROW_FACTOR, R.TOL_LN
NPAIRS_LIST = [1, 5, 63, 64, 65, 256, "max"]
F32 = torch.float32


def cu(t):
    return t.float().contiguous().cuda()


def pack_stat(s):
    raw = struct.pack("ffffddd", s.mean, s.den, s.rstd, s.std_, s.mean_d, s.std_d, s.count)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()


def stat_from(buf):
    mean, den, rstd, sd, mean_d, std_d, count = struct.unpack("ffffddd", buf.cpu().numpy().tobytes()[:40])
    return SimpleNamespace(mean=mean, den=den, rstd=rstd, std_=sd, mean_d=mean_d, std_d=std_d, den_d=std_d + R.LN_EPS,
                           count=count)


def producer(env, prod):
    """a2 = relu(W2p a1p + b2p) and its pdg_ln_stat from the real producer: pdg_mlp2_fwd into a NaN-filled partials
    buffer, pdg_ln_finalize over the count it returns.  (a2, the packed statistics, the statistics read back)."""
    lib, sh = env
    M = prod.a1p.shape[0]
    a1, W2, b2 = cu(prod.a1p), cu(prod.W2p), cu(prod.b2p)
    a2, part, n = torch.empty(M, L, device="cuda"), part_buf(env), ctypes.c_int(0)
    assert lib.pdg_mlp2_fwd(M, p(a1), p(W2), p(b2), p(a2), p(part), ctypes.byref(n), sh()) == 0
    st = torch.full((40,), 0xAB, dtype=torch.uint8, device="cuda")
    assert lib.pdg_ln_finalize(p(part), n.value, float(M * L), p(st), sh()) == 0
    torch.cuda.synchronize()
    assert rel(a2, prod.a2) < TOL
    return a2, st, stat_from(st)


def pairs_buf(env, pairs):
    """The pairs at the start of a NaN-filled buffer of pdg_max_blocks() pairs."""
    buf = part_buf(env)
    buf[:pairs.numel()] = pairs.cuda()
    return buf


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64)


def same_bits(a, b):
    return all((x is None and y is None) or torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def twice(launch):
    """Two launches into fresh NaN-filled buffers: bitwise the same.  Returns the first one's buffers."""
    a, b = launch(), launch()
    torch.cuda.synchronize()
    assert same_bits(a, b), "two runs differ"
    return a


def bound_of(tag, r32, r64, small):
    """The relative-L2 bound of one output: TOL, or downstream of the small-sigma LayerNorm ROW_FACTOR x the fp32
    restatement's distance (below TOL_LN)."""
    if not small:
        return TOL
    d = rel(r32, r64)
    assert d < TOL_LN, (tag, d)
    return ROW_FACTOR * d


def check_out(tag, got, rows, r64, r32, exact, small=False):
    """One row output: NaN guard rows intact; integer-exact: EQUAL; randn: relative L2 and the per-row bound."""
    assert got.shape[0] == rows + 3 and torch.isnan(got[rows:]).all(), f"{tag}: wrote past the end"
    if exact:
        diff = got[:rows].cpu() != r64.float()
        assert not diff.any(), (tag, int(diff.any(1).sum()), "rows differ")
        return
    tol = bound_of(tag, r32, r64, small)
    e, e32, mine, plain = rel(got[:rows], r64), rel(r32, r64), worst_row(got[:rows], r64), worst_row(r32, r64)
    ratio = mine / plain if plain > 0 else (0.0 if mine == 0 else float("inf"))
    print(f"TAN {tag}: rel {e:.2e} (bound {tol:.1e}, fp32 {e32:.2e}) worst row {mine:.2e} / fp32 {plain:.2e} = {ratio:.2f}")
    assert e <= tol and mine <= ROW_FACTOR * plain, (tag, e, tol, mine, plain)
    return tol


def check_part(tag, part, nblocks, da_ref, a, mean, exact, tol=TOL):
    """A producer's partials: finite in [0, 2 nblocks), NaN past; totals EQUAL the integer sums, or within the
    Cauchy-Schwarz bounds of an output that is within tol in L2 (module docstring)."""
    q = part.cpu()
    assert torch.isfinite(q[:2 * nblocks]).all() and torch.isnan(q[2 * nblocks:]).all(), tag
    t1, t2 = R.pairs_ref(da_ref, a, mean)
    g1, g2 = float(q[0:2 * nblocks:2].sum()), float(q[1:2 * nblocks:2].sum())
    if exact:
        assert g1 == float(t1) and g2 == float(t2), (tag, g1, float(t1), g2, float(t2))
        return
    n2 = float(da_ref.double().norm())
    xc = a.double().cpu() - mean
    b1, b2 = tol * a.numel() ** 0.5 * n2, tol * float(xc.norm()) * n2
    print(f"TAN {tag}: T1 err {abs(g1 - float(t1)):.2e} (bound {b1:.2e}) T2 err {abs(g2 - float(t2)):.2e} (bound {b2:.2e})")
    assert abs(g1 - float(t1)) <= b1 and abs(g2 - float(t2)) <= b2, (tag, g1, float(t1), b1, g2, float(t2), b2)


class RowCase:
    """tangent_ref.tan_inputs(M, cond) on the device with the statistics the kernels are handed, the host copies the
    references are formed from (the arrays as the device holds them) and the references, made once."""

    def __init__(self, env, M, cond):
        lib, _ = env
        i = R.tan_inputs(M, cond)
        self.M, self.cond, self.exact, self.n, self.i = M, cond, cond == "x", M * L, i
        self.d = SimpleNamespace(**{k: cu(getattr(i, k)) for k in (
            "W0n", "w0e", "b0e", "W2", "We1", "Wn1", "Wd1", "Wd2", "g", "a1", "a1b", "da_prev", "res", "rows2", "dx_in",
            "de_in", "e_in", "dP", "dQ")})
        d = self.d
        d.src, d.dst = i.src.int().cuda(), i.dst.int().cuda()
        rp = torch.zeros(R.NN + 1, dtype=torch.long)
        rp[1:] = torch.cumsum(torch.bincount(i.dst, minlength=R.NN), 0)
        self.rowptr, d.rowptr = rp, rp.int().cuda()
        d.std = torch.tensor([i.std_out], device="cuda")
        if self.exact:
            d.a_prev, d.a2, d.a2b = cu(i.a_prev), cu(i.a2), cu(i.a2b)
            self.stat = self.stat2 = self.stat2b = R.unit_stat(self.n)
            d.st_prev = d.st2 = d.st2b = pack_stat(self.stat)
            self.totals = (float(self.n * R.EXACT_K), 0.0)
        else:
            d.a_prev, d.st_prev, self.stat = producer(env, i.prod_prev)
            d.a2, d.st2, self.stat2 = producer(env, i.prod_a2)
            d.a2b, d.st2b, self.stat2b = producer(env, i.prod_a2b)
            if cond == "c":
                assert 0.02 < R.LN_EPS / self.stat.std_d < 1.0   # eps counts in den
            t1, t2 = R.pairs_ref(i.da_prev, d.a_prev, self.stat.mean_d)
            xc = d.a_prev.double().cpu() - self.stat.mean_d
            # both LayerNorm terms matter: T1 / n of the order of da, T2 well away from zero
            assert abs(float(t1)) / self.n > 0.3
            assert abs(float(t2)) > 0.2 * float(i.da_prev.double().norm() * xc.norm())
            self.totals = (float(t1), float(t2))
        self.h = SimpleNamespace(a_prev=d.a_prev.cpu(), a2=d.a2.cpu(), a2b=d.a2b.cpu())
        self._pairs, self._ref = {}, {}
        self.max_blocks = lib.pdg_max_blocks()

    def pairs(self, env, npairs):
        """The totals over npairs pairs, NaN beyond."""
        if npairs not in self._pairs:
            pr = R.exact_pairs(self.n, npairs) if self.exact else R.split_totals(*self.totals, npairs)
            if not self.exact:   # the totals the kernel is handed: those of the split
                assert abs(float(pr[0::2].sum()) - self.totals[0]) <= 1e-12 * abs(self.totals[0])
            self._pairs[npairs] = pairs_buf(env, pr)
        return self._pairs[npairs]

    def ref(self, key, fn):
        """fn(dtype) in fp64 and fp32, made once per key."""
        if key not in self._ref:
            self._ref[key] = (fn(torch.float64), None if self.exact else fn(F32))
        return self._ref[key]

    @property
    def ln(self):
        return dict(totals=self.totals, stat=self.stat)


_rows = {}


def row_case(env, M, cond):
    if (M, cond) not in _rows:
        _rows[(M, cond)] = RowCase(env, M, cond)
    return _rows[(M, cond)]


def run_enc(env, c, nb, edge):
    lib, sh = env
    d, M = c.d, c.M

    def launch():
        out, part = guarded(M), part_buf(env)
        if edge:
            assert lib.pdg_edge_enc_tan(M, p(d.de_in), p(d.e_in), p(d.w0e), p(d.b0e), p(d.W2), p(d.a2), p(d.st2), p(out),
                                        p(part), nb, sh()) == 0
        else:
            assert lib.pdg_node_enc_tan(M, p(d.dx_in), p(d.a1), p(d.W0n), p(d.W2), p(d.a2), p(d.st2), p(out), p(part), nb,
                                        sh()) == 0
        return out, part
    return twice(launch)


def ref_enc(c, edge):
    i, h = c.i, c.h
    if edge:
        return c.ref("edge_enc", lambda dt: R.edge_enc_tan_ref(i.de_in, i.e_in, i.w0e, i.b0e, i.W2, h.a2, dt))
    return c.ref("node_enc", lambda dt: R.node_enc_tan_ref(i.dx_in, i.a1, i.W0n, i.W2, h.a2, dt))


def run_node_pre(env, c, nb, res, pairs, npairs):
    lib, sh = env
    d, M = c.d, c.M

    def launch():
        dx, dP, dQ = guarded(M), guarded(M), guarded(M)
        assert lib.pdg_node_pre_tan(M, p(d.da_prev), p(d.a_prev), p(d.st_prev), p(pairs), npairs, p(d.g),
                                    p(d.res) if res else None, p(dx), p(d.We1), p(dP), p(dQ), nb, sh()) == 0
        return dx, dP, dQ
    return twice(launch)


def ref_node_pre(c, res):
    i, h = c.i, c.h
    return c.ref(("node_pre", res), lambda dt: R.node_pre_tan_ref(i.da_prev, h.a_prev, i.g, i.res if res else None,
                                                                  i.We1, dt, **c.ln))


def run_edge(env, c, nb, eu, res, pairs, npairs):
    lib, sh = env
    d, M = c.d, c.M

    def launch():
        de, da2m, da2e, pm, pe = guarded(M), guarded(M), guarded(M), part_buf(env), part_buf(env)
        assert lib.pdg_edge_tan(M, R.NN, p(d.da_prev), p(d.a_prev), p(d.st_prev), p(pairs), npairs, p(d.g),
                                p(d.res) if res else None, p(de), p(d.src), p(d.dst), p(d.dP), p(d.dQ), p(d.We1), p(d.W2),
                                p(d.a1), p(d.a2), p(d.st2), p(d.a1b) if eu else None, p(d.a2b) if eu else None,
                                p(d.st2b) if eu else None, p(da2m), p(da2e) if eu else None, p(pm), p(pe) if eu else None,
                                int(eu), nb, sh()) == 0
        return de, da2m, da2e, pm, pe
    return twice(launch)


def ref_edge(c, res):
    i, h = c.i, c.h
    return c.ref(("edge", res), lambda dt: R.edge_tan_ref(i.da_prev, h.a_prev, i.g, i.res if res else None, i.src, i.dst,
                                                          i.dP, i.dQ, i.We1, i.W2, i.a1, h.a2, i.a1b, h.a2b, dt, **c.ln))


def run_node_net(env, c, nb):
    lib, sh = env
    d, M = c.d, c.M

    def launch():
        out, part = guarded(M), part_buf(env)
        assert lib.pdg_node_net_tan(M, p(d.rows2), p(d.res), p(d.Wn1), p(d.W2), p(d.a1), p(d.a2), p(d.st2), p(out), p(part),
                                    nb, sh()) == 0
        return out, part
    return twice(launch)


def ref_node_net(c):
    i, h = c.i, c.h
    return c.ref("node_net", lambda dt: R.node_net_tan_ref(i.rows2, i.res, i.Wn1, i.W2, i.a1, h.a2, dt))


def run_decoder(env, c, nb, res, scale, pairs, npairs):
    lib, sh = env
    d, M = c.d, c.M

    def launch():
        out = guarded(M, 3)
        assert lib.pdg_decoder_tan(M, p(d.da_prev), p(d.a_prev), p(d.st_prev), p(pairs), npairs, p(d.g),
                                   p(d.res) if res else None, p(d.Wd1), p(d.a1), p(d.Wd2), p(d.std) if scale else None,
                                   scale, p(out), nb, sh()) == 0
        return (out,)
    return twice(launch)[0]


def ref_decoder(c, res, scale):
    i, h = c.i, c.h
    return c.ref(("decoder", res, scale), lambda dt: R.decoder_tan_ref(
        i.da_prev, h.a_prev, i.g, i.res if res else None, i.Wd1, i.a1, i.Wd2, i.std_out if scale else None, dt, **c.ln))


def run_segsum(env, N, E, rowptr, da, a, st, pairs, npairs, g, nb):
    lib, sh = env

    def launch():
        out = guarded(N)
        assert lib.pdg_segment_sum_tan(N, E, p(rowptr), p(da), p(a), p(st), p(pairs), npairs, p(g), p(out), nb, sh()) == 0
        return (out,)
    return twice(launch)[0]


CONDS3 = ["x", "p", "c"]


@pytest.mark.parametrize("M,nblocks", EDGE_SHAPES)
def test_enc_tan_at_the_schedule_edges(env, M, nblocks):
    """pdg_node_enc_tan and pdg_edge_enc_tan: no LayerNorm tangent upstream, TOL in either conditioning (a2 and its
    mean, which enter the mask and T2, come from the small-sigma producer in "c")."""
    for cond in CONDS3:
        c = row_case(env, M, cond)
        for edge in (False, True):
            tag = f"{'edge' if edge else 'node'}_enc_tan {cond} M={M} nb={nblocks}"
            out, part = run_enc(env, c, nblocks, edge)
            r64, r32 = ref_enc(c, edge)
            check_out(tag, out, M, r64, r32, c.exact)
            check_part(tag + " partials", part, nblocks, r64, c.h.a2, c.stat2.mean_d, c.exact)


@pytest.mark.parametrize("M,nblocks", EDGE_SHAPES)
def test_node_pre_tan_at_the_schedule_edges(env, M, nblocks):
    for cond in CONDS3:
        c = row_case(env, M, cond)
        pairs = c.pairs(env, NPAIRS)
        for res in (True, False):
            got = run_node_pre(env, c, nblocks, res, pairs, NPAIRS)
            r64, r32 = ref_node_pre(c, res)
            for k, nm in enumerate(("dx", "dP", "dQ")):
                check_out(f"node_pre_tan {nm} {cond} M={M} nb={nblocks} res={int(res)}", got[k], M, r64[k],
                          r32 and r32[k], c.exact, cond == "c")


@pytest.mark.parametrize("M,nblocks", EDGE_SHAPES)
def test_edge_tan_at_the_schedule_edges(env, M, nblocks):
    for cond in CONDS3:
        c = row_case(env, M, cond)
        pairs = c.pairs(env, NPAIRS)
        for eu in (True, False):
            for res in (True, False):
                de, da2m, da2e, pm, pe = run_edge(env, c, nblocks, eu, res, pairs, NPAIRS)
                r64, r32 = ref_edge(c, res)
                r32 = r32 or (None, None, None)
                tag = f"{cond} M={M} nb={nblocks} eu={int(eu)} res={int(res)}"
                small = cond == "c"
                check_out(f"edge_tan de {tag}", de, M, r64[0], r32[0], c.exact, small)
                tm = check_out(f"edge_tan da2m {tag}", da2m, M, r64[1], r32[1], c.exact, small)
                check_part(f"edge_tan part_m {tag}", pm, nblocks, r64[1], c.h.a2, c.stat2.mean_d, c.exact, tm)
                if eu:
                    te = check_out(f"edge_tan da2e {tag}", da2e, M, r64[2], r32[2], c.exact, small)
                    check_part(f"edge_tan part_e {tag}", pe, nblocks, r64[2], c.h.a2b, c.stat2b.mean_d, c.exact, te)
                else:   # no edge update: its outputs untouched
                    assert torch.isnan(da2e).all() and torch.isnan(pe).all(), tag


@pytest.mark.parametrize("M,nblocks", EDGE_SHAPES)
def test_node_net_tan_at_the_schedule_edges(env, M, nblocks):
    for cond in CONDS3:
        c = row_case(env, M, cond)
        tag = f"node_net_tan {cond} M={M} nb={nblocks}"
        out, part = run_node_net(env, c, nblocks)
        r64, r32 = ref_node_net(c)
        check_out(tag, out, M, r64, r32, c.exact)
        check_part(tag + " partials", part, nblocks, r64, c.h.a2, c.stat2.mean_d, c.exact)


@pytest.mark.parametrize("M,nblocks", EDGE_SHAPES)
def test_decoder_tan_at_the_schedule_edges(env, M, nblocks):
    """scale_output 1 multiplies by 2.75 (randn) or by 2 (integer-exact: still exact)."""
    for cond in CONDS3:
        c = row_case(env, M, cond)
        pairs = c.pairs(env, NPAIRS)
        for res in (True, False):
            for scale in (1, 0):
                out = run_decoder(env, c, nblocks, res, scale, pairs, NPAIRS)
                r64, r32 = ref_decoder(c, res, scale)
                check_out(f"decoder_tan {cond} M={M} nb={nblocks} res={int(res)} scale={scale}", out, M, r64, r32, c.exact,
                          cond == "c")


@pytest.mark.parametrize("cond", ["x", "p"])
@pytest.mark.parametrize("M", [33, 77, 4099])
def test_row_outputs_do_not_depend_on_the_block_layout(env, M, cond):
    """The same pairs and statistics at nblocks 1, 37 and 256: every row output bitwise the same (a block's r0 is a
    multiple of 32, so every row sits at the same image position in any layout).  Partials are not compared."""
    c = row_case(env, M, cond)
    pairs = c.pairs(env, NPAIRS)

    def rows(nb):
        return (run_enc(env, c, nb, False)[0], run_enc(env, c, nb, True)[0], *run_node_pre(env, c, nb, True, pairs, NPAIRS),
                *run_edge(env, c, nb, True, True, pairs, NPAIRS)[:3], run_node_net(env, c, nb)[0],
                run_decoder(env, c, nb, True, 1, pairs, NPAIRS))
    one = rows(1)
    for nb in (37, 256):
        other = rows(nb)
        for k, (a, b) in enumerate(zip(one, other)):
            assert torch.equal(bits(a), bits(b)), (M, cond, nb, k)


@pytest.mark.parametrize("npairs", NPAIRS_LIST)
def test_consumers_at_every_pair_count(env, npairs):
    """pdg_node_pre_tan, pdg_edge_tan, pdg_segment_sum_tan and pdg_decoder_tan at (77, 37) with the same totals split
    unevenly over npairs pairs (tan_resolve's lane-strided loop takes a second trip past 64 and 32 at
    pdg_max_blocks()); NaN from entry 2 npairs on.  randn within TOL, integer-exact EQUAL for every split."""
    lib, _ = env
    M, nb = 77, 37
    npairs = lib.pdg_max_blocks() if npairs == "max" else npairs
    for cond in ("x", "p"):
        c = row_case(env, M, cond)
        pairs = c.pairs(env, npairs)
        assert torch.isfinite(pairs[:2 * npairs]).all() and torch.isnan(pairs[2 * npairs:]).all()
        assert (pairs.numel() == 2 * npairs) == (npairs == lib.pdg_max_blocks())
        tag = f"{cond} npairs={npairs}"
        got = run_node_pre(env, c, nb, True, pairs, npairs)
        r64, r32 = ref_node_pre(c, True)
        for k, nm in enumerate(("dx", "dP", "dQ")):
            check_out(f"node_pre_tan {nm} {tag}", got[k], M, r64[k], r32 and r32[k], c.exact)
        de, da2m, da2e, _, _ = run_edge(env, c, nb, True, True, pairs, npairs)
        r64, r32 = ref_edge(c, True)
        for k, (nm, o) in enumerate((("de", de), ("da2m", da2m), ("da2e", da2e))):
            check_out(f"edge_tan {nm} {tag}", o, M, r64[k], r32 and r32[k], c.exact)
        out = run_decoder(env, c, nb, True, 1, pairs, npairs)
        r64, r32 = ref_decoder(c, True, 1)
        check_out(f"decoder_tan {tag}", out, M, r64, r32, c.exact)
        i, d = c.i, c.d
        out = run_segsum(env, R.NN, M, d.rowptr, d.da_prev, d.a_prev, d.st_prev, pairs, npairs, d.g, nb)
        r64, r32 = c.ref("segsum", lambda dt: R.segment_sum_tan_ref(c.rowptr, i.da_prev, c.h.a_prev, i.g, dt, **c.ln))
        check_out(f"segment_sum_tan {tag}", out, R.NN, r64, r32, c.exact)


@pytest.mark.parametrize("M,nblocks", [(33, 2), (77, 37)])
def test_constant_tensor_takes_the_c2_zero_branch(env, M, nblocks):
    """a_prev one positive value, its statistics from the real producer (W2p = 0, b2p = 0.75): the stored std_d is 0
    (hand-packed if the one-pass statistic leaves a residue), tan_resolve takes its `sd > 0 ? ... : 0` branch and the
    outputs follow the reference's c2 = 0 at TOL, whatever T2 the pairs carry (here 1: without the branch c2 is inf
    and (a - mean) c2 = 0 x inf a NaN)."""
    c = row_case(env, M, "p")
    i, d = c.i, c.d
    prod = R._produce(torch.Generator().manual_seed(9800 + M), M, "p", const=0.75)
    a, st, stat = producer(env, prod)
    assert float(a.min()) == 0.75 == float(a.max())
    if stat.std_d != 0.0:
        eps32 = torch.tensor(R.LN_EPS, dtype=F32)
        stat = SimpleNamespace(mean=0.75, den=float(eps32), rstd=float(1 / eps32), std_=0.0, mean_d=0.75, std_d=0.0,
                               den_d=R.LN_EPS, count=float(M * L))
        st = pack_stat(stat)
    assert stat.std_d == 0.0 and stat.mean_d == 0.75 and stat.count == float(M * L)
    t1 = float(i.da_prev.double().sum())
    pairs = pairs_buf(env, R.split_totals(t1, 1.0, NPAIRS))
    ln = dict(totals=(t1, 1.0), stat=stat)
    ha = a.cpu()
    lib, sh = env
    tag = f"const M={M} nb={nblocks}"
    dx, dP, dQ = guarded(M), guarded(M), guarded(M)
    assert lib.pdg_node_pre_tan(M, p(d.da_prev), p(a), p(st), p(pairs), NPAIRS, p(d.g), p(d.res), p(dx), p(d.We1), p(dP),
                                p(dQ), nblocks, sh()) == 0
    de, da2m, pm = guarded(M), guarded(M), part_buf(env)
    assert lib.pdg_edge_tan(M, R.NN, p(d.da_prev), p(a), p(st), p(pairs), NPAIRS, p(d.g), p(d.res), p(de), p(d.src),
                            p(d.dst), p(d.dP), p(d.dQ), p(d.We1), p(d.W2), p(d.a1), p(d.a2), p(d.st2), None, None, None,
                            p(da2m), None, p(pm), None, 0, nblocks, sh()) == 0
    dy = guarded(M, 3)
    assert lib.pdg_decoder_tan(M, p(d.da_prev), p(a), p(st), p(pairs), NPAIRS, p(d.g), p(d.res), p(d.Wd1), p(d.a1),
                               p(d.Wd2), p(d.std), 1, p(dy), nblocks, sh()) == 0
    dag = guarded(R.NN)
    assert lib.pdg_segment_sum_tan(R.NN, M, p(d.rowptr), p(d.da_prev), p(a), p(st), p(pairs), NPAIRS, p(d.g), p(dag),
                                   nblocks, sh()) == 0
    torch.cuda.synchronize()
    both = lambda fn: (fn(torch.float64), fn(F32))
    r = both(lambda dt: R.node_pre_tan_ref(i.da_prev, ha, i.g, i.res, i.We1, dt, **ln))
    for k, (nm, o) in enumerate((("dx", dx), ("dP", dP), ("dQ", dQ))):
        check_out(f"node_pre_tan {nm} {tag}", o, M, r[0][k], r[1][k], False)
    r = both(lambda dt: R.edge_tan_ref(i.da_prev, ha, i.g, i.res, i.src, i.dst, i.dP, i.dQ, i.We1, i.W2, i.a1, c.h.a2,
                                       None, None, dt, **ln))
    check_out(f"edge_tan de {tag}", de, M, r[0][0], r[1][0], False)
    check_out(f"edge_tan da2m {tag}", da2m, M, r[0][1], r[1][1], False)
    r = both(lambda dt: R.decoder_tan_ref(i.da_prev, ha, i.g, i.res, i.Wd1, i.a1, i.Wd2, i.std_out, dt, **ln))
    check_out(f"decoder_tan {tag}", dy, M, r[0], r[1], False)
    r = both(lambda dt: R.segment_sum_tan_ref(c.rowptr, i.da_prev, ha, i.g, dt, **ln))
    check_out(f"segment_sum_tan {tag}", dag, R.NN, r[0], r[1], False)


@pytest.mark.parametrize("N,nblocks", [(25, 1), (57, 3), (40, 256)])
def test_segment_sum_tan_on_the_hand_built_csr(env, N, nblocks):
    """In-degrees 0, 1, 7, 8, 9, 16, 17 and a hub of 300, the first and the last node empty.  N = 16 nblocks + 9 at 1
    and 3 blocks: a second sweep with a ragged tail; N = 40 at 256 blocks: most blocks without a node.  Empty nodes
    exactly 0, guard rows NaN, the bounds of the row kernels; the hub row, a 300-term fp32 sum in edge order, also
    within ROW_FACTOR x the fp32 restatement summed in the same order."""
    HUB = 7
    for cond in CONDS3:
        s = R.seg_tan_inputs(N, cond)
        assert s.deg[HUB] == 300 and s.deg[0] == 0 and s.deg[-1] == 0 and s.E < 2 ** 22
        n = s.E * L
        if cond == "x":
            a, stat = cu(s.a_prev), R.unit_stat(n)
            st, totals = pack_stat(stat), (float(n * R.EXACT_K), 0.0)
            pr = R.exact_pairs(n, NPAIRS)
        else:
            a, st, stat = producer(env, s.prod_prev)
            if cond == "c":
                assert 0.02 < R.LN_EPS / stat.std_d < 1.0
            t1, t2 = R.pairs_ref(s.da_prev, a, stat.mean_d)
            totals = (float(t1), float(t2))
            pr = R.split_totals(*totals, NPAIRS)
        out = run_segsum(env, N, s.E, s.rowptr.int().cuda(), cu(s.da_prev), a, st, pairs_buf(env, pr), NPAIRS, cu(s.g),
                         nblocks)
        ha = a.cpu()
        fn = lambda dt: R.segment_sum_tan_ref(s.rowptr, s.da_prev, ha, s.g, dt, totals=totals, stat=stat)
        r64, r32 = fn(torch.float64), None if cond == "x" else fn(F32)
        tag = f"segment_sum_tan csr {cond} N={N} nb={nblocks}"
        check_out(tag, out, N, r64, r32, cond == "x", cond == "c")
        assert float(out[:N].cpu()[s.deg == 0].abs().max()) == 0.0, tag
        if cond != "x":
            mine, plain = rel(out[HUB], r64[HUB]), rel(r32[HUB], r64[HUB])
            print(f"TAN {tag} hub row: {mine:.2e} / fp32 in edge order {plain:.2e} = {mine / plain:.2f}")
            assert mine <= ROW_FACTOR * plain, (tag, mine, plain)


@pytest.mark.parametrize("nb", [37, 256])
def test_engine_order_chain_vs_fp64(env, nb):
    """Two steps in EPDEngine.tangent's order and buffer hand-over on tangent_ref.chain_inputs (hub_graph(600): 59
    nodes, a hub run, edge-free nodes): the encoders' tangents, then node_pre, edge (with the edge update, then
    without), segment sum, node_net per step, and the decoder.  Every consumer reads its producer's own partials
    buffer (NaN-filled before the first use) with npairs = nblocks; the tangent, pair and residual buffers roll as the
    engine rolls them.  dy against the fp64 composition of the reference functions: ROW_FACTOR x the fp32
    composition's distance, never above the model tier's 3e-5, in L2 and for the worst row."""
    lib, sh = env
    s = sh()
    c = R.chain_inputs()
    N, E = c.N, c.E
    P = {k: cu(v) for k, v in c.prm.items()}
    w = lambda k: p(P[k])
    act = SimpleNamespace(a1ne=cu(c.a1ne), a2ne=cu(c.a2ne), a2ee=cu(c.a2ee), a1d=cu(c.a1d))
    steps = [SimpleNamespace(eu=t.eu, **{k: cu(v) for k, v in vars(t).items() if k != "eu"}) for t in c.steps]
    st_ne, st_ee = ln_stat(env, act.a2ne), ln_stat(env, act.a2ee)
    for t in steps:
        t.st_m, t.st_n = ln_stat(env, t.a2m), ln_stat(env, t.a2n)
        t.st_e = ln_stat(env, t.a2e) if t.eu else None
    src, dst, rp = c.src.int().cuda(), c.dst.int().cuda(), c.rowptr.int().cuda()
    dx_in, de_in, e_in = cu(c.dx_in), cu(c.de_in), cu(c.e_in.reshape(-1))
    pr_n, pr_m, pr_e0, pr_e1 = (part_buf(env) for _ in range(4))
    emp = lambda rows: torch.empty(rows, L, device="cuda")
    da2n, dx_a, dx_b, dP, dQ, daggr = (emp(N) for _ in range(6))
    da2e_a, da2e_b, de_a, de_b, da2m = (emp(E) for _ in range(5))
    assert lib.pdg_node_enc_tan(N, p(dx_in), p(act.a1ne), w("node_encoder.0.weight"), w("node_encoder.2.weight"),
                                p(act.a2ne), p(st_ne), p(da2n), p(pr_n), nb, s) == 0
    assert lib.pdg_edge_enc_tan(E, p(de_in), p(e_in), w("edge_encoder.0.weight"), w("edge_encoder.0.bias"),
                                w("edge_encoder.2.weight"), p(act.a2ee), p(st_ee), p(da2e_a), p(pr_e0), nb, s) == 0
    W1e, W2e = w("processor.edge_net.0.weight"), w("processor.edge_net.2.weight")
    g_e, g_n = w("processor.edge_net.4.weight"), w("processor.node_net.4.weight")
    ln_n, ln_e = (act.a2ne, st_ne, w("node_encoder.4.weight")), (act.a2ee, st_ee, w("edge_encoder.4.weight"))
    dx_prev = de_prev = None
    for t in steps:
        eu = t.eu
        assert lib.pdg_node_pre_tan(N, p(da2n), p(ln_n[0]), p(ln_n[1]), p(pr_n), nb, ln_n[2], p(dx_prev), p(dx_a), W1e,
                                    p(dP), p(dQ), nb, s) == 0
        assert lib.pdg_edge_tan(E, N, p(da2e_a), p(ln_e[0]), p(ln_e[1]), p(pr_e0), nb, ln_e[2], p(de_prev), p(de_a),
                                p(src), p(dst), p(dP), p(dQ), W1e, W2e, p(t.a1m), p(t.a2m), p(t.st_m),
                                p(t.a1e) if eu else None, p(t.a2e) if eu else None, p(t.st_e) if eu else None, p(da2m),
                                p(da2e_b) if eu else None, p(pr_m), p(pr_e1) if eu else None, int(eu), nb, s) == 0
        assert lib.pdg_segment_sum_tan(N, E, p(rp), p(da2m), p(t.a2m), p(t.st_m), p(pr_m), nb, g_e, p(daggr), nb, s) == 0
        if eu:
            ln_e = (t.a2e, t.st_e, g_e)
        da2e_a, da2e_b, pr_e0, pr_e1 = da2e_b, da2e_a, pr_e1, pr_e0
        de_prev, de_a, de_b = de_a, de_b, de_a
        assert lib.pdg_node_net_tan(N, p(daggr), p(dx_a), w("processor.node_net.0.weight"),
                                    w("processor.node_net.2.weight"), p(t.a1n), p(t.a2n), p(t.st_n), p(da2n), p(pr_n), nb,
                                    s) == 0
        ln_n = (t.a2n, t.st_n, g_n)
        dx_prev, dx_a, dx_b = dx_a, dx_b, dx_a
    dy, std = guarded(N, 3), torch.tensor([c.std_out], device="cuda")
    assert lib.pdg_decoder_tan(N, p(da2n), p(ln_n[0]), p(ln_n[1]), p(pr_n), nb, ln_n[2], p(dx_prev),
                               w("node_decoder.0.weight"), p(act.a1d), w("node_decoder.2.weight"), p(std), 1, p(dy), nb,
                               s) == 0
    torch.cuda.synchronize()
    for buf in (pr_n, pr_m, pr_e0, pr_e1):
        assert torch.isfinite(buf[:2 * nb]).all() and torch.isnan(buf[2 * nb:]).all()
    assert torch.isnan(dy[N:]).all()
    d64, d32 = R.chain_ref(c), R.chain_ref(c, F32)
    e, e32 = rel(dy[:N], d64), rel(d32, d64)
    mine, plain = worst_row(dy[:N], d64), worst_row(d32, d64)
    bound = min(ROW_FACTOR * e32, 3e-5)
    print(f"TAN chain nb={nb} N={N} E={E} dy: rel {e:.2e} (bound {bound:.1e}, fp32 {e32:.2e}) worst row {mine:.2e} / "
          f"fp32 {plain:.2e} = {mine / plain:.2f}")
    assert e <= bound and mine <= min(ROW_FACTOR * plain, 3e-5), (e, bound, mine, plain)
