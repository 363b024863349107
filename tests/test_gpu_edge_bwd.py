"""The per-step edge backward kernels at the op level, against the float64 restatement of
tests/edge_bwd_ref.py (anchored to autograd through the model's LayerNorm by tests/test_edge_bwd_ref.py):

  pdg_edge_bwd_w2                  the shipped kernel (pdg_ebw.hip): both templates, blocks with fewer rows than a
                                   16-row round, ragged last rounds, empty blocks, slabs written then accumulated;
  pdg_edge_bwd                     the unfused kernel the `fused_edge_wgrad=False` variant and every
                                   "fused vs separate" model test use as the baseline;
  pdg_edge_bwd_w2 -> pdg_pq_scatter_bwd(e_is_sum=1)   the chain the engine runs, with a gz1e that is never stored.

Inputs (one set per case, shared by all tests; the fp64 / fp32 references are computed once per case): a1 =
relu(randn); a2m / a2e from pdg_mlp2_fwd on different inputs, so the two LayerNorms' statistics differ by a factor
~2 and a kernel that swaps them fails; dst sorted with a hub node owning >= 40 consecutive rows (E permitting) and
nodes without an edge; gaggr with N << E rows; the LayerNorm pairs from the real producer, pdg_ln_colsum.
"""
import ctypes
import struct
from types import SimpleNamespace

import pytest
import torch

from edge_bwd_ref import edge_bwd_ref, hub_graph, worst_row

pytestmark = pytest.mark.gpu

L = 128
# (E, nslabs): the smallest shapes that reach each path of the row schedule (32-row units, two 16-row rounds each,
# one contiguous range of units per block).  (1..17, 1) and (31 / 33, 2): a block with fewer rows than a round,
# exactly one round, one row past a round, one row short of / past a unit, only one register set ever real;
# (77, 37): more blocks than units, the empty ones read row E - 1 and must store nothing; (4099, 37): several
# units per block, a ragged last round in the last block; (30011, 256): the engine's grid, the one large case.
CASES = [(1, 1), (15, 1), (16, 1), (17, 1), (31, 2), (33, 2), (77, 37), (4099, 37), (30011, 256)]
MID = (4099, 37)
TOL = 1e-5      # this LayerNorm-backward -> W2^T chain against fp64 (test_ln_colsum_and_mlp2_bwd_vs_autograd's bound)
# the per-row bound: worst-row error of a kernel <= ROW_FACTOR x the worst-row error of the plain fp32 torch
# restatement of the chain.  Measured on the MI355X over every case (profiles/edge_bwd_op_errors.txt): ratios
# 0.79 - 1.27 for pdg_edge_bwd_w2 and 0.71 - 1.17 for pdg_edge_bwd; the factor is the smallest power of two that
# is at least twice the largest of them (2 x 1.27 = 2.54 -> 4)
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


def finalize(lib, s, part, nparts, count):
    st = torch.zeros(40, dtype=torch.uint8, device="cuda")
    lib.pdg_ln_finalize(part.data_ptr(), nparts, float(count), st.data_ptr(), s)
    return st


def p(t):
    return None if t is None else t.data_ptr()


def nan_rows(E):
    return torch.full((E + 3, L), float("nan"), device="cuda")


class Case:
    """The inputs of one (E, nslabs) case on the device, its references and the kernels' runs (each made once)."""

    def __init__(self, env, E, nslabs):
        lib, sh, _ = env
        s = sh()
        torch.manual_seed(4000 + E)
        self.E, self.nslabs = E, nslabs
        self.N, src, dst, rp, rps, perm_src = hub_graph(E)
        self.src64, self.dst64 = src, dst
        self.dst = dst.int().cuda()
        self.rp, self.rps, self.perm_src = rp.int().cuda(), rps.int().cuda(), perm_src.int().cuda()
        self.a1m, self.a1e = torch.relu(rnd(E, L)), torch.relu(rnd(E, L))
        xe = torch.relu(rnd(E, L, scale=2.0))      # the edge-update LayerNorm's input: other statistics
        self.W2, b2 = lin(L, L)
        self.Wc, _ = lin(L, L)
        self.W2T, self.WcT = self.W2.T.contiguous(), self.Wc.T.contiguous()
        self.ln_g = rnd(L) * 0.3 + 1.0
        self.gaggr, self.ge_next = rnd(self.N, L), rnd(E, L)
        self.slab_fill = rnd(nslabs, L * L + L)
        part = torch.empty(4096, dtype=torch.float64, device="cuda")
        n = ctypes.c_int(0)
        self.a2m, self.a2e = torch.empty(E, L, device="cuda"), torch.empty(E, L, device="cuda")
        self.st = {}
        for k, x, a2 in (("m", self.a1m, self.a2m), ("e", xe, self.a2e)):
            lib.pdg_mlp2_fwd(E, x.data_ptr(), self.W2.data_ptr(), b2.data_ptr(), a2.data_ptr(), part.data_ptr(),
                             ctypes.byref(n), s)
            self.st[k] = finalize(lib, s, part, n.value, E * L)
        sm, se = stat_from(self.st["m"]), stat_from(self.st["e"])
        assert abs(se["mean_d"] - sm["mean_d"]) > 0.1 * sm["mean_d"] and abs(se["std_d"] - sm["std_d"]) > 0.1 * sm["std_d"]
        # the LayerNorm pairs from the real producer, as the engine calls it (pdg_ln_colsum; lb = None downstream)
        mb = lib.pdg_max_blocks()
        self.part, self.pairs, self.npairs = {}, {}, {}
        for k, gy, gidx, a2 in (("m", self.gaggr, self.dst, self.a2m), ("e", self.ge_next, None, self.a2e)):
            self.part[k] = torch.zeros((mb + 1) * 256, dtype=torch.float64, device="cuda")
            self.pairs[k] = torch.zeros(2 * mb, dtype=torch.float64, device="cuda")
            lib.pdg_ln_colsum(E, gy.data_ptr(), p(gidx), a2.data_ptr(), self.st[k].data_ptr(), self.part[k].data_ptr(),
                              ctypes.byref(n), self.ln_g.data_ptr(), self.pairs[k].data_ptr(), 0, s)
            self.npairs[k] = n.value
        torch.cuda.synchronize()
        self._ref, self._runs = {}, {}

    def ref(self, eu, dtype=torch.float64):
        key = (eu, dtype)
        if key not in self._ref:
            self._ref[key] = edge_bwd_ref(self.dst64, self.gaggr, self.ge_next if eu else None, self.a2m, self.a1m,
                                          self.a2e, self.a1e, self.ln_g, self.W2, self.Wc, dtype=dtype)
        return self._ref[key]

    def ln_args(self, eu, lb=None, pairs=None):
        """(lb_m, lb_e, pairs_m, npairs_m, pairs_e, npairs_e) of a call: the producer's pairs unless given."""
        if lb is not None:
            return p(lb["m"]), p(lb["e"]) if eu else None, None, 0, None, 0
        pm, nm, pe, ne = pairs or (self.pairs["m"], self.npairs["m"], self.pairs["e"], self.npairs["e"])
        return None, None, p(pm), nm, p(pe) if eu else None, ne if eu else 0

    def w2(self, env, eu, store_gz1e=True, alias=False, lb=None, pairs=None, keep=None):
        """pdg_edge_bwd_w2 twice on garbage-filled slabs: slab_init = 1, then 0.  Outputs with 3 NaN rows past E."""
        key = ("w2", eu, keep)
        if keep is not None and key in self._runs:
            return self._runs[key]
        lib, sh, _ = env
        s = sh()
        E = self.E
        gz1m = nan_rows(E)
        gC = gz1m if alias else nan_rows(E)
        gz1e = nan_rows(E) if eu and store_gz1e else None
        slabs = self.slab_fill.clone()
        lbm, lbe, pm, nm, pe, ne = self.ln_args(eu, lb, pairs)
        for init in (1, 0):
            assert lib.pdg_edge_bwd_w2(E, p(self.dst), p(self.gaggr), p(self.ge_next) if eu else None, p(self.a2m),
                                       p(self.a1m), p(self.a2e) if eu else None, p(self.a1e) if eu else None,
                                       p(self.st["m"]), p(self.st["e"]) if eu else None, lbm, lbe, p(self.ln_g),
                                       p(self.W2T), p(gz1m), p(gz1e), p(gC), p(slabs), self.nslabs, pm, nm, pe, ne,
                                       init, s) == 0
        torch.cuda.synchronize()
        r = SimpleNamespace(gz1m=gz1m, gz1e=gz1e, gC=gC, slabs=slabs)
        if keep is not None:
            self._runs[key] = r
        return r

    def unfused(self, env, eu, lb=None, keep=None):
        key = ("unfused", eu, keep)
        if keep is not None and key in self._runs:
            return self._runs[key]
        lib, sh, _ = env
        s = sh()
        E = self.E
        o = SimpleNamespace(**{k: nan_rows(E) for k in ("gz2m", "gz1m", "gz2e", "gz1e", "gC", "ge_out")})
        lbm, lbe, pm, nm, pe, ne = self.ln_args(eu, lb)
        assert lib.pdg_edge_bwd(E, p(self.dst), p(self.gaggr), p(self.ge_next) if eu else None, p(self.a2m), p(self.a1m),
                                p(self.a2e) if eu else None, p(self.a1e) if eu else None, p(self.st["m"]),
                                p(self.st["e"]) if eu else None, lbm, lbe, p(self.ln_g), p(self.W2T), p(self.WcT),
                                p(o.gz2m), p(o.gz1m), p(o.gz2e), p(o.gz1e), p(o.gC), p(o.ge_out), pm, nm, pe, ne, s) == 0
        torch.cuda.synchronize()
        if keep is not None:
            self._runs[key] = o
        return o

    def finalized_lb(self, env):
        """The finalised pdg_ln_bwd blocks of both LayerNorms from the producer's partials."""
        lib, sh, _ = env
        s = sh()
        lb = {}
        for k in ("m", "e"):
            lb[k] = torch.zeros(24, dtype=torch.uint8, device="cuda")
            gg, gb = torch.zeros(L, device="cuda"), torch.zeros(L, device="cuda")
            lib.pdg_ln_colsum_finalize(self.part[k].data_ptr(), self.npairs[k], self.ln_g.data_ptr(),
                                       self.st[k].data_ptr(), gg.data_ptr(), gb.data_ptr(), lb[k].data_ptr(), s)
        torch.cuda.synchronize()
        return lb


_cases = {}


def case(env, E, nslabs):
    if (E, nslabs) not in _cases:
        _cases[(E, nslabs)] = Case(env, E, nslabs)
    return _cases[(E, nslabs)]


def reduce_slabs(env, slabs, nslabs):
    """The engine's own contract for the slabs (pdg_wgrad_reduce into zeroed gradients): no slab layout here."""
    lib, sh, _ = env
    gW, gb = torch.zeros(L, L, device="cuda"), torch.zeros(L, device="cuda")
    scratch = slabs.clone()   # the reduction overwrites its slabs
    lib.pdg_wgrad_reduce(scratch.data_ptr(), nslabs, gW.data_ptr(), L, 0, gb.data_ptr(), sh())
    torch.cuda.synchronize()
    return gW, gb


def tails_are_nan(E, *outs):
    return all(bool(o[E:].isnan().all()) and o.shape[0] == E + 3 for o in outs)


def row_ratios(c, eu, got):
    """Worst-row error of gz1m and gC over the worst-row error of the fp32 restatement (both against fp64)."""
    r64, r32 = c.ref(eu), c.ref(eu, torch.float32)
    out = {}
    for k in ("gz1m", "gC"):
        mine, plain = worst_row(getattr(got, k)[:c.E], getattr(r64, k)), worst_row(getattr(r32, k), getattr(r64, k))
        out[k] = (mine, plain, mine / plain)
    return out


@pytest.mark.parametrize("eu", [1, 0])
@pytest.mark.parametrize("E,nslabs", CASES)
def test_edge_bwd_w2_vs_fp64(env, E, nslabs, eu):
    """pdg_edge_bwd_w2 against fp64: gz1m / gz1e / gC within 1e-5, no row written at or past E, and the slabs
    through pdg_wgrad_reduce equal to 2 dW2 / 2 db2 after a slab_init = 1 call and a slab_init = 0 call on
    randn-filled slabs (the first overwrote the garbage, the second accumulated).  Per row: the worst row of gz1m
    and of gC is within ROW_FACTOR of the worst row of the plain fp32 torch restatement of the chain (a global
    L2 hides one bad row among 30011).

    Measured on the MI355X (profiles/edge_bwd_op_errors.txt): gz1m / gz1e / gC 1.4e-7 - 2.0e-7 and dW2 / db2
    0.5e-7 - 1.9e-7 from fp64 over all cases; worst row of gz1m / gC 1.5e-7 - 4.2e-7 against 1.6e-7 - 4.1e-7 for
    the fp32 restatement, ratios 0.79 - 1.27 (largest at E = 4099), hence ROW_FACTOR = 4."""
    c = case(env, E, nslabs)
    r = c.w2(env, eu, keep="main")
    ref = c.ref(eu)
    gW, gb = reduce_slabs(env, r.slabs, nslabs)
    errs = {k: rel(getattr(r, k)[:E], getattr(ref, k)) for k in ("gz1m", "gC") + (("gz1e",) if eu else ())}
    errs["dW2"], errs["db2"] = rel(gW, 2 * ref.dW2), rel(gb, 2 * ref.db2)
    rows = row_ratios(c, eu, r)
    print(f"edge_bwd_w2 E={E} nslabs={nslabs} eu={eu} " + " ".join(f"{k}={v:.2e}" for k, v in sorted(errs.items()))
          + " | worst row " + " ".join(f"{k}: {m:.2e} / fp32 {q:.2e} = {t:.2f}" for k, (m, q, t) in rows.items()))
    assert max(errs.values()) < TOL, errs
    assert tails_are_nan(E, r.gz1m, r.gC, *((r.gz1e,) if eu else ()))
    if not eu:
        assert r.gz1e is None and torch.equal(r.gC[:E], r.gz1m[:E])
    for k, (mine, plain, ratio) in rows.items():
        assert mine <= ROW_FACTOR * plain, (k, mine, plain, ratio)


@pytest.mark.parametrize("E,nslabs", CASES)
def test_edge_bwd_w2_without_gz1e_is_bitwise(env, E, nslabs):
    """'gz1e may be NULL with the edge update: it is then not stored': gz1m, gC and the slabs bitwise those of the
    run that stores gz1e."""
    c = case(env, E, nslabs)
    a, b = c.w2(env, 1, keep="main"), c.w2(env, 1, store_gz1e=False)
    assert torch.equal(a.gz1m[:E], b.gz1m[:E]) and torch.equal(a.gC[:E], b.gC[:E]) and torch.equal(a.slabs, b.slabs)
    assert tails_are_nan(E, b.gz1m, b.gC)


@pytest.mark.parametrize("E,nslabs", CASES)
def test_edge_bwd_w2_gc_may_be_gz1m_without_edge_update(env, E, nslabs):
    """'gC may then be the gz1m pointer itself: written once': bitwise the run with a separate gC; with the edge
    update the aliased call is refused on the host and nothing runs (outputs and slabs untouched)."""
    lib, sh, _ = env
    from pdg.lib import PdgError
    c = case(env, E, nslabs)
    a, b = c.w2(env, 0, keep="main"), c.w2(env, 0, alias=True)
    assert b.gC is b.gz1m
    assert torch.equal(a.gz1m[:E], b.gz1m[:E]) and torch.equal(a.gC[:E], b.gz1m[:E]) and torch.equal(a.slabs, b.slabs)
    assert tails_are_nan(E, b.gz1m)
    out, slabs = nan_rows(E), c.slab_fill.clone()
    with pytest.raises(PdgError):
        lib.pdg_edge_bwd_w2(E, p(c.dst), p(c.gaggr), p(c.ge_next), p(c.a2m), p(c.a1m), p(c.a2e), p(c.a1e), p(c.st["m"]),
                            p(c.st["e"]), None, None, p(c.ln_g), p(c.W2T), p(out), None, p(out), p(slabs), nslabs,
                            p(c.pairs["m"]), c.npairs["m"], p(c.pairs["e"]), c.npairs["e"], 1, sh())
    torch.cuda.synchronize()
    assert bool(out.isnan().all()) and torch.equal(slabs, c.slab_fill)


def test_edge_bwd_w2_finalized_lb_and_host_pairs(env):
    """The other two ways to hand over the LayerNorm scalars, both within 1e-6 of the producer-pairs run: the
    finalised pdg_ln_bwd blocks of pdg_ln_colsum_finalize (pairs = NULL), and host-made pairs, the restatement's
    fp64 (S1, S2) split unevenly into 3 parts for the message and 41 for the edge-update branch (npairs_m !=
    npairs_e: each branch must reduce its own count)."""
    E, nslabs = MID
    c = case(env, E, nslabs)
    base = c.w2(env, 1, keep="main")
    gW0, gb0 = reduce_slabs(env, base.slabs, nslabs)
    ref = c.ref(1)
    host = []
    for ln, n in ((ref.ln_m, 3), (ref.ln_e, 41)):
        w = torch.linspace(-1.0, 2.0, n, dtype=torch.float64).pow(3)
        w = w / w.sum()
        host += [(torch.stack([ln.S1 * w, ln.S2 * w], 1).reshape(-1).contiguous().cuda()), n]
    for name, kw in (("lb", dict(lb=c.finalized_lb(env))), ("host pairs", dict(pairs=tuple(host)))):
        r = c.w2(env, 1, **kw)
        gW, gb = reduce_slabs(env, r.slabs, nslabs)
        d = {k: rel(getattr(r, k)[:E], getattr(base, k)[:E]) for k in ("gz1m", "gz1e", "gC")}
        d["dW2"], d["db2"] = rel(gW, gW0), rel(gb, gb0)
        print(f"edge_bwd_w2 E={E} {name} vs producer pairs: " + " ".join(f"{k}={v:.2e}" for k, v in d.items()))
        assert max(d.values()) < 1e-6, (name, d)
        assert max(rel(r.gz1m[:E], ref.gz1m), rel(r.gz1e[:E], ref.gz1e), rel(r.gC[:E], ref.gC)) < TOL


@pytest.mark.parametrize("eu", [1, 0])
@pytest.mark.parametrize("E,nslabs", CASES)
def test_edge_bwd_vs_fp64_and_fused_is_no_worse(env, E, nslabs, eu):
    """pdg_edge_bwd (pairs; a finalised lb for the 4099-row case) against fp64 on the same inputs: all six outputs
    within 1e-5, the NaN rows past E kept; without the edge update gz2e / gz1e keep their fill, gC = gz1m and
    ge_out = gC Wc.  Its gz2 rows through the unfused path's weight-gradient pass (pdg_wgrad_segments +
    pdg_wgrad_reduce) give dW2 / db2 within 1e-5 as well.  And the header's 'gz1m/gz1e/gC as pdg_edge_bwd': the
    fused kernel no further from fp64 than 1.5 x the unfused one (test_edge_fwd_coop_matches_edge_fwd's idiom).
    The per-row bound holds for this kernel too."""
    lib, sh, _ = env
    c = case(env, E, nslabs)
    o = c.unfused(env, eu, lb=c.finalized_lb(env) if (E, nslabs) == MID else None)
    f = c.w2(env, eu, keep="main")
    ref = c.ref(eu)
    keys = ("gz2m", "gz1m", "gC", "ge_out") + (("gz2e", "gz1e") if eu else ())
    errs = {k: rel(getattr(o, k)[:E], getattr(ref, k)) for k in keys}
    # dW2 / db2 of the unfused path: its gz2 rows through pdg_wgrad_segments (written, not accumulated)
    segs = [(o.gz2m, c.a1m)] + ([(o.gz2e, c.a1e)] if eu else [])
    ns = 61
    slabs = torch.empty(ns, L * L + L, device="cuda")
    gp = (ctypes.c_void_p * len(segs))(*[g.data_ptr() for g, _ in segs])
    xp = (ctypes.c_void_p * len(segs))(*[x.data_ptr() for _, x in segs])
    rw = (ctypes.c_int * len(segs))(*[E] * len(segs))
    lib.pdg_wgrad_segments(len(segs), gp, xp, rw, slabs.data_ptr(), ns, sh())
    gW, gb = reduce_slabs(env, slabs, ns)
    errs["dW2"], errs["db2"] = rel(gW, ref.dW2), rel(gb, ref.db2)
    rows = row_ratios(c, eu, o)
    print(f"edge_bwd E={E} eu={eu} " + " ".join(f"{k}={v:.2e}" for k, v in sorted(errs.items()))
          + " | worst row " + " ".join(f"{k}: {m:.2e} / fp32 {q:.2e} = {t:.2f}" for k, (m, q, t) in rows.items()))
    assert max(errs.values()) < TOL, errs
    assert tails_are_nan(E, o.gz2m, o.gz1m, o.gC, o.ge_out, o.gz2e, o.gz1e)
    if not eu:
        assert bool(o.gz2e.isnan().all()) and bool(o.gz1e.isnan().all())
        assert torch.equal(o.gC[:E], o.gz1m[:E])
        assert rel(o.ge_out[:E], o.gC[:E].double() @ c.Wc.double()) < 2e-6
    for k in ("gz1m", "gC") + (("gz1e",) if eu else ()):
        ef, eo = rel(getattr(f, k)[:E], getattr(ref, k)), errs[k]
        assert ef <= 1.5 * eo + 1e-9, (k, ef, eo)
    for k, (mine, plain, ratio) in rows.items():
        assert mine <= ROW_FACTOR * plain, (k, mine, plain, ratio)


@pytest.mark.parametrize("E,nslabs", [MID, (77, 37)])
def test_edge_bwd_w2_then_pq_scatter_bwd(env, E, nslabs):
    """The combination the engine runs: pdg_edge_bwd_w2 with the edge update and no gz1e array, then
    pdg_pq_scatter_bwd(gz1m, gC, e_is_sum = 1) over the hub graph (isolated trailing nodes included).  gP / gQ
    within 1e-5 of fp64 formed from the restatement's exact gz1m and gz1e, and within 1e-6 of the chain that stores
    gz1e and passes e_is_sum = 0 (the figure test_gz1e_from_gc_matches_stored_gz1e holds the model to)."""
    lib, sh, _ = env
    c = case(env, E, nslabs)
    N = c.N
    ref = c.ref(1)
    out = {}
    for e_is_sum in (1, 0):
        r = c.w2(env, 1, store_gz1e=not e_is_sum)
        gP, gQ = torch.full((N, L), float("nan"), device="cuda"), torch.full((N, L), float("nan"), device="cuda")
        lib.pdg_pq_scatter_bwd(N, p(c.rp), p(c.rps), p(c.perm_src), p(r.gz1m), p(r.gC if e_is_sum else r.gz1e),
                               e_is_sum, p(gP), p(gQ), sh())
        torch.cuda.synchronize()
        out[e_is_sum] = (gP, gQ)
    z = lambda: torch.zeros(N, L, dtype=torch.float64)
    refP = z().index_add_(0, c.dst64, ref.gz1m).index_add_(0, c.src64, ref.gz1e)
    refQ = z().index_add_(0, c.src64, ref.gz1m).index_add_(0, c.dst64, ref.gz1e)
    eP, eQ = rel(out[1][0], refP), rel(out[1][1], refQ)
    dP, dQ = rel(out[1][0], out[0][0]), rel(out[1][1], out[0][1])
    print(f"edge_bwd_w2 -> pq_scatter_bwd E={E} N={N}: gP={eP:.2e} gQ={eQ:.2e} vs fp64; e_is_sum vs stored gz1e "
          f"gP={dP:.2e} gQ={dQ:.2e}")
    assert eP < TOL and eQ < TOL
    assert dP < 1e-6 and dQ < 1e-6
    # a node without an edge gets zeros, not the fill
    assert float(out[1][0][-3:].abs().max()) == 0 and float(out[1][1][-3:].abs().max()) == 0
