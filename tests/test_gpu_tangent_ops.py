"""The tangent-pass kernels at the op level (csrc/pdg_tangent.hip) against the float64 restatements of
tests/tangent_ref.py (anchored to torch.func.jvp by tests/test_tangent_ref.py).

Shapes: (rows 200, nblocks 3): several 32-row rounds per block with a ragged last one; (rows 37, nblocks 256):
mostly empty blocks, which read the last row and must store nothing.  Every output array has NaN guard rows
past its end, every pair buffer NaN past its count.  The pre-LayerNorm tangents are drawn with a non-zero mean
and a component along (a - mu), so both LayerNorm terms matter (asserted).  The consumers take pairs split
unevenly over 5 blocks; the producers' partials are compared with the fp64 sums.

Bound: 3e-6 relative L2 per output, the order of the bf16x6 op tests against fp64.  The (T1, T2) partials: each
da is within 3e-6 in L2, so |dT1| <= sqrt(n) |d da|_2 and |dT2| <= |a - mu|_2 |d da|_2 (Cauchy-Schwarz)."""
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
