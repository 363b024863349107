"""The input-gradient kernels at the op level (csrc/pdg_ingrad.hip) against the float64 closed form of
tests/ingrad_ref.py (anchored to autograd and finite differences by tests/test_ingrad_ref.py):

  pdg_node_enc_gin, pdg_edge_enc_gin   blocks with fewer rows than a 32-row round, exactly / one past half a
                                       round, one short of / past a round, more blocks than rounds (empty
                                       blocks read the last row and must store nothing), several rounds per
                                       block with a ragged last one; a non-identity permutation; scale on and
                                       off; NaN guard elements past the end; two LayerNorms whose statistics
                                       are a factor ~2 apart, so a kernel that mixed them up fails;
  pdg_graph_colsum3                    ragged ptr with an empty graph.

Inputs as tests/test_gpu_edge_bwd.py builds them: a2 from pdg_mlp2_fwd, its statistics from pdg_ln_finalize,
the LayerNorm pairs from the real producer pdg_ln_colsum."""
import ctypes

import pytest
import torch

from ingrad_ref import edge_enc_gin_ref, node_enc_gin_ref

pytestmark = pytest.mark.gpu

L = 128
CASES = [(1, 1), (15, 1), (16, 1), (17, 1), (31, 2), (33, 2), (77, 37), (4099, 37)]
TOL = 1e-5   # the LayerNorm-backward -> W2^T -> W0 chain against fp64: the edge-backward op gate


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pdg.lib import lib, stream_handle
    return lib, stream_handle


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def rnd(*shape, scale=1.0):
    return (torch.randn(*shape, dtype=torch.float64) * scale).float().cuda()


def lin(out, inp):
    m = torch.nn.Linear(inp, out)
    return m.weight.detach().float().cuda().contiguous(), (m.bias.detach().float().cuda() + 0.1).contiguous()


class Case:
    """One (rows, blocks) case: two operand sets (LayerNorm inputs a factor 2 apart) shared by both kernels."""

    def __init__(self, env, M, nblocks):
        lib, sh = env
        s = sh()
        torch.manual_seed(7000 + M)
        self.M, self.nblocks = M, nblocks
        self.W2, b2 = lin(L, L)
        self.W2T = self.W2.T.contiguous()
        self.W0n, _ = lin(L, 6)
        self.w0e, self.b0e = lin(L, 1)
        self.ln_g = rnd(L) * 0.3 + 1.0
        self.stats8 = (torch.rand(8, dtype=torch.float64) * 3 + 0.5).float().cuda()
        self.perm = torch.randperm(M).int().cuda()
        assert M < 3 or not torch.equal(self.perm.cpu(), torch.arange(M, dtype=torch.int32))
        self.sets = []
        part = torch.empty(4096, dtype=torch.float64, device="cuda")
        n = ctypes.c_int(0)
        mb = lib.pdg_max_blocks()
        for scale in (1.0, 2.0):
            o = {"a1": torch.relu(rnd(M, L, scale=scale)), "gy": rnd(M, L), "e_in": rnd(M),
                 "a2": torch.empty(M, L, device="cuda"), "st": torch.zeros(40, dtype=torch.uint8, device="cuda"),
                 "pairs": torch.zeros(2 * mb, dtype=torch.float64, device="cuda")}
            lib.pdg_mlp2_fwd(M, o["a1"].data_ptr(), self.W2.data_ptr(), b2.data_ptr(), o["a2"].data_ptr(),
                             part.data_ptr(), ctypes.byref(n), s)
            lib.pdg_ln_finalize(part.data_ptr(), n.value, float(M * L), o["st"].data_ptr(), s)
            cpart = torch.zeros((mb + 1) * 256, dtype=torch.float64, device="cuda")
            lib.pdg_ln_colsum(M, o["gy"].data_ptr(), None, o["a2"].data_ptr(), o["st"].data_ptr(), cpart.data_ptr(),
                              ctypes.byref(n), self.ln_g.data_ptr(), o["pairs"].data_ptr(), 0, s)
            o["npairs"] = n.value
            self.sets.append(o)
        torch.cuda.synchronize()
        m0, m1 = (float(o["a2"].double().std()) for o in self.sets)
        assert m1 > 1.5 * m0


_cases = {}


def case(env, M, nblocks):
    if (M, nblocks) not in _cases:
        _cases[(M, nblocks)] = Case(env, M, nblocks)
    return _cases[(M, nblocks)]


@pytest.mark.parametrize("scale", [1, 0])
@pytest.mark.parametrize("M,nblocks", CASES)
def test_node_enc_gin_matches_fp64(env, M, nblocks, scale):
    lib, sh = env
    c = case(env, M, nblocks)
    for o in c.sets:
        gm = torch.full((M + 3, 3), float("nan"), device="cuda")
        gp = torch.full((M + 3, 2), float("nan"), device="cuda")
        assert lib.pdg_node_enc_gin(M, o["gy"].data_ptr(), o["a2"].data_ptr(), o["a1"].data_ptr(), c.W0n.data_ptr(),
                                    o["st"].data_ptr(), None, o["pairs"].data_ptr(), o["npairs"], c.ln_g.data_ptr(),
                                    c.W2T.data_ptr(), c.stats8.data_ptr(), scale, gm.data_ptr(), gp.data_ptr(),
                                    nblocks, sh()) == 0
        torch.cuda.synchronize()
        std = (float(c.stats8[3]), float(c.stats8[1])) if scale else (None, None)
        rm, rp = node_enc_gin_ref(o["gy"], o["a2"], o["a1"], c.W0n, c.ln_g, c.W2, *std)
        assert torch.isnan(gm[M:]).all() and torch.isnan(gp[M:]).all()
        em, ep = rel(gm[:M], rm), rel(gp[:M], rp)
        print(f"node_enc_gin M={M} blocks={nblocks} scale={scale}: {em:.2e} {ep:.2e}")
        assert em <= TOL and ep <= TOL, (em, ep)


@pytest.mark.parametrize("scale", [1, 0])
@pytest.mark.parametrize("M,nblocks", CASES)
def test_edge_enc_gin_matches_fp64(env, M, nblocks, scale):
    lib, sh = env
    c = case(env, M, nblocks)
    for o in c.sets:
        ge = torch.full((M + 3,), float("nan"), device="cuda")
        assert lib.pdg_edge_enc_gin(M, o["gy"].data_ptr(), o["a2"].data_ptr(), o["e_in"].data_ptr(),
                                    c.w0e.data_ptr(), c.b0e.data_ptr(), o["st"].data_ptr(), None,
                                    o["pairs"].data_ptr(), o["npairs"], c.ln_g.data_ptr(), c.W2T.data_ptr(),
                                    c.perm.data_ptr(), c.stats8.data_ptr(), scale, ge.data_ptr(), nblocks, sh()) == 0
        torch.cuda.synchronize()
        ref = edge_enc_gin_ref(o["gy"], o["a2"], o["e_in"].cpu(), c.w0e.cpu(), c.b0e.cpu(), c.ln_g, c.W2, c.perm,
                               float(c.stats8[7]) if scale else None)
        assert torch.isnan(ge[M:]).all()
        e = rel(ge[:M], ref)
        print(f"edge_enc_gin M={M} blocks={nblocks} scale={scale}: {e:.2e}")
        assert e <= TOL, e


def test_kernels_are_deterministic(env):
    lib, sh = env
    c = case(env, 4099, 37)
    o = c.sets[0]
    outs = []
    for _ in range(2):
        ge = torch.empty(c.M, device="cuda")
        gm, gp = torch.empty(c.M, 3, device="cuda"), torch.empty(c.M, 2, device="cuda")
        lib.pdg_edge_enc_gin(c.M, o["gy"].data_ptr(), o["a2"].data_ptr(), o["e_in"].data_ptr(), c.w0e.data_ptr(),
                             c.b0e.data_ptr(), o["st"].data_ptr(), None, o["pairs"].data_ptr(), o["npairs"],
                             c.ln_g.data_ptr(), c.W2T.data_ptr(), c.perm.data_ptr(), c.stats8.data_ptr(), 1,
                             ge.data_ptr(), c.nblocks, sh())
        lib.pdg_node_enc_gin(c.M, o["gy"].data_ptr(), o["a2"].data_ptr(), o["a1"].data_ptr(), c.W0n.data_ptr(),
                             o["st"].data_ptr(), None, o["pairs"].data_ptr(), o["npairs"], c.ln_g.data_ptr(),
                             c.W2T.data_ptr(), c.stats8.data_ptr(), 1, gm.data_ptr(), gp.data_ptr(), c.nblocks, sh())
        torch.cuda.synchronize()
        outs.append((ge, gm, gp))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_graph_colsum3_ragged_with_empty_graph(env):
    """Within one fp32 rounding of the fp64 sums: 2^-24 |sum| for the single rounding, plus the fp64
    accumulation's own 2^-53 n sum |x| (the order differs from torch's)."""
    lib, sh = env
    torch.manual_seed(5)
    ptr = torch.tensor([0, 5, 5, 1200, 1201, 3333], dtype=torch.int32)
    N, B = int(ptr[-1]), ptr.numel() - 1
    x = torch.full((N + 2, 3), float("nan"), device="cuda")
    x[:N] = rnd(N, 3, scale=10.0) + 3.0
    out = torch.full((B + 1, 3), float("nan"), device="cuda")
    ptr_d = ptr.cuda()
    assert lib.pdg_graph_colsum3(B, ptr_d.data_ptr(), x.data_ptr(), out.data_ptr(), sh()) == 0
    torch.cuda.synchronize()
    xd = x[:N].double().cpu()
    assert torch.isnan(out[B]).all()
    for g in range(B):
        a, b = int(ptr[g]), int(ptr[g + 1])
        ref = xd[a:b].sum(0)
        bound = 2.0 ** -24 * ref.abs() + 2.0 ** -53 * (b - a) * xd[a:b].abs().sum(0)
        assert ((out[g].double().cpu() - ref).abs() <= bound).all(), (g, out[g], ref)
    assert float(out[1].abs().max()) == 0.0
