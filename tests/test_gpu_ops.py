"""Op-level parity of the HIP kernels (SURVEY §4 tier T1).  Inputs are seeded; sizes include ragged tails
(rows not a multiple of the 32-row wave tile), zero in-degree nodes and repeated indices.

Two kinds of test live here.  Against a float64 torch restatement of the same op, stated inline: the tests named
*_vs_fp64 / *_vs_autograd, test_mlp2_fwd_and_ln_stats, test_encoder_fwd, test_segment_sum_with_layernorm, the
weight-gradient and loss tests.  Kernel against kernel (bitwise, or to fp32 rounding, with fp64 only as the yardstick
of which of the two is closer): the tests named *_matches_*, *_equals_* and *_vs_<another kernel>, among them every
test of the LayerNorm + residual outputs (e_t, x_t, x_S), of pdg_edge_fwd_infer and of the in-kernel statistics;
they show that two kernels agree, not that either is right.  The reference suites that hold those kernels to fp64
from their inputs are tests/test_gpu_fwd.py (the per-step forward), tests/test_gpu_edge_bwd.py and
tests/test_gpu_node_bwd.py (the per-step backward); tests/test_gpu_wgrad.py and tests/test_gpu_loss_ops.py do the
same for the weight gradients and the kernels that end a step."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

L = 128
TOL = 2e-6   # relative L2 vs float64 for a single fp32 op


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
    import struct
    mean, den, rstd, sd, mean_d, std_d, count = struct.unpack("ffffddd", raw[:40])
    return dict(mean=mean, den=den, rstd=rstd, std=sd, mean_d=mean_d, std_d=std_d, count=count)


def finalize(lib, s, part, nparts, count):
    st = torch.zeros(40, dtype=torch.uint8, device="cuda")
    lib.pdg_ln_finalize(part.data_ptr(), nparts, float(count), st.data_ptr(), s)
    return st


class PQ:
    """P / Q of the node pre-pass in the library's layout (pdg_pq_layout: two N x 128 arrays, or one
    N x 256 array of interleaved 16-feature blocks with Q 16 floats after P): `p`, `q` are the pointers
    the kernels take, `unpack()` returns (P, Q) as N x 128 tensors; `PQ.of(lib, P, Q)` packs inputs."""

    def __init__(self, lib, N):
        self.N, self.blocked = N, bool(lib.pdg_pq_layout())
        if self.blocked:
            self.buf = torch.empty(N, 2 * L, device="cuda")
            self.p, self.q = self.buf.data_ptr(), self.buf.data_ptr() + 16 * 4
        else:
            self.P, self.Q = torch.empty(N, L, device="cuda"), torch.empty(N, L, device="cuda")
            self.p, self.q = self.P.data_ptr(), self.Q.data_ptr()

    def unpack(self):
        if not self.blocked:
            return self.P, self.Q
        v = self.buf.view(self.N, 8, 2, 16)
        return v[:, :, 0].reshape(self.N, L).contiguous(), v[:, :, 1].reshape(self.N, L).contiguous()

    @classmethod
    def of(cls, lib, P, Q):
        pq = cls(lib, P.shape[0])
        if pq.blocked:
            v = pq.buf.view(pq.N, 8, 2, 16)
            v[:, :, 0] = P.view(pq.N, 8, 16)
            v[:, :, 1] = Q.view(pq.N, 8, 16)
        else:
            pq.P.copy_(P)
            pq.Q.copy_(Q)
        return pq


def ln_ref(a, g, b, eps=1e-5):
    a = a.double()
    x = a - a.mean()
    return x / (x.std(unbiased=False) + eps) * g.double() + b.double()


@pytest.mark.parametrize("M", [1, 33, 1000, 4099])
def test_mlp2_fwd_and_ln_stats(env, M):
    lib, sh, _ = env
    s = sh()
    a1 = torch.relu(rnd(M, L))
    W, b = lin(L, L)
    a2 = torch.empty(M, L, device="cuda")
    part = torch.empty(4096, dtype=torch.float64, device="cuda")
    n = ctypes.c_int(0)
    lib.pdg_mlp2_fwd(M, a1.data_ptr(), W.data_ptr(), b.data_ptr(), a2.data_ptr(), part.data_ptr(), ctypes.byref(n), s)
    ref = torch.relu(a1.double() @ W.double().T + b.double())
    assert rel(a2, ref) < TOL
    st = stat_from(finalize(lib, s, part, n.value, M * L))
    assert abs(st["mean_d"] - float(ref.mean())) <= 1e-6 * abs(float(ref.mean())) + 1e-9
    assert abs(st["std_d"] - float(ref.std(unbiased=False))) <= 1e-6 * float(ref.std(unbiased=False))


@pytest.mark.parametrize("M,IN", [(77, 6), (1025, 1)])
def test_encoder_fwd(env, M, IN):
    lib, sh, _ = env
    s = sh()
    x = rnd(M, IN)
    W0, b0 = lin(L, IN)
    W2, b2 = lin(L, L)
    a1, a2 = torch.empty(M, L, device="cuda"), torch.empty(M, L, device="cuda")
    part = torch.empty(4096, dtype=torch.float64, device="cuda")
    n = ctypes.c_int(0)
    lib.pdg_encoder_fwd(M, IN, x.data_ptr(), W0.data_ptr(), b0.data_ptr(), W2.data_ptr(), b2.data_ptr(),
                        a1.data_ptr(), a2.data_ptr(), part.data_ptr(), ctypes.byref(n), s)
    r1 = torch.relu(x.double() @ W0.double().T + b0.double())
    r2 = torch.relu(r1 @ W2.double().T + b2.double())
    assert rel(a1, r1) < TOL and rel(a2, r2) < TOL


def _csr(N, E, seed=1):
    g = torch.Generator().manual_seed(seed)
    dst = torch.randint(0, N, (E,), generator=g)
    dst[: N // 7] = 0            # one heavy node
    src = torch.randint(0, N, (E,), generator=g)
    key = dst * N + src
    order = torch.sort(key, stable=True).indices
    src, dst = src[order], dst[order]
    rp = torch.zeros(N + 1, dtype=torch.int64)
    rp[1:] = torch.cumsum(torch.bincount(dst, minlength=N), 0)
    return src, dst, rp


@pytest.mark.parametrize("N,E", [(50, 300), (1031, 6000)])
def test_segment_sum_with_layernorm(env, N, E):
    lib, sh, _ = env
    s = sh()
    src, dst, rp = _csr(N, E)
    rows = torch.relu(rnd(E, L))
    g, b = rnd(L) + 1.0, rnd(L)
    part = torch.empty(4096, dtype=torch.float64, device="cuda")
    # stats via the library (pdg_mlp2_fwd path is tested above); use torch values packed as a struct
    st = torch.zeros(40, dtype=torch.uint8, device="cuda")
    import struct
    r64 = rows.double()
    mean, sd = float(r64.mean()), float(r64.std(unbiased=False))
    den = float(torch.tensor(sd, dtype=torch.float32) + 1e-5)
    st.copy_(torch.frombuffer(bytearray(struct.pack("ffffddd", mean, den, 1.0 / den, sd, mean, sd, E * L)),
                              dtype=torch.uint8).cuda())
    out = torch.empty(N, L, device="cuda")
    rp_d = rp.int().cuda()
    xs = torch.empty(N, L, device="cuda")
    lib.pdg_segment_sum(N, rp_d.data_ptr(), rows.data_ptr(), st.data_ptr(), g.data_ptr(), b.data_ptr(),
                        out.data_ptr(), xs.data_ptr(), s)
    xhat = (r64.cpu() - mean) / den
    normed = xhat * g.double().cpu() + b.double().cpu()
    ref = torch.zeros(N, L, dtype=torch.float64).index_add_(0, dst, normed)
    assert rel(out, ref) < TOL
    assert rel(xs, torch.zeros(N, L, dtype=torch.float64).index_add_(0, dst, xhat)) < TOL
    # node-level LayerNorm-backward sums of the gathered gradient gy_k = gaggr[dst_k]
    gaggr = rnd(N, L)
    part = torch.empty(4096 * 256, dtype=torch.float64, device="cuda")
    n = ctypes.c_int(0)
    lib.pdg_ln_colsum_nodes(N, gaggr.data_ptr(), rp_d.data_ptr(), xs.data_ptr(), part.data_ptr(), ctypes.byref(n),
                            None, None, 0, s)
    tot = part[: n.value * 256].view(n.value, 256).sum(0).cpu()
    gy = gaggr.double().cpu()[dst]
    assert rel(tot[:L], gy.sum(0)) < 1e-6
    assert rel(tot[L:], (gy * xhat).sum(0)) < 1e-5
    # zero in-degree nodes are exactly zero
    deg0 = (rp[1:] - rp[:-1]) == 0
    if deg0.any():
        assert float(out.cpu()[deg0].abs().max()) == 0.0
    raw = torch.empty(N, L, device="cuda")
    lib.pdg_segment_sum(N, rp_d.data_ptr(), rows.data_ptr(), None, None, None, raw.data_ptr(), None, s)
    assert rel(raw, torch.zeros(N, L, dtype=torch.float64).index_add_(0, dst, r64.cpu())) < TOL


@pytest.mark.parametrize("M", [64, 1000, 3001])
def test_wgrad_accum_reduce(env, M):
    lib, sh, _ = env
    s = sh()
    G, X, G2, X2 = rnd(M, L), rnd(M, L), rnd(M, L), rnd(M, L)
    ns = 37
    slabs = torch.zeros(ns, L * L + L, device="cuda")
    lib.pdg_wgrad_accum(M, G.data_ptr(), X.data_ptr(), G2.data_ptr(), X2.data_ptr(), slabs.data_ptr(), ns, s)
    lib.pdg_wgrad_accum(M, G.data_ptr(), X.data_ptr(), None, None, slabs.data_ptr(), ns, s)   # accumulates
    gW = torch.zeros(L, 3 * L, device="cuda")
    gb = torch.zeros(L, device="cuda")
    lib.pdg_wgrad_reduce(slabs.data_ptr(), ns, gW.data_ptr(), 3 * L, L, gb.data_ptr(), s)
    ref = 2 * G.double().T @ X.double() + G2.double().T @ X2.double()
    assert rel(gW[:, L:2 * L], ref) < 1e-5
    assert float(gW[:, :L].abs().max()) == 0 and float(gW[:, 2 * L:].abs().max()) == 0
    assert rel(gb, 2 * G.double().sum(0) + G2.double().sum(0)) < 1e-5


@pytest.mark.parametrize("K,transpose", [(1, 0), (3, 1), (6, 0)])
def test_wgrad_narrow(env, K, transpose):
    lib, sh, _ = env
    s = sh()
    M = 2049
    wide, narrow = rnd(M, L), rnd(M, K)
    part = torch.empty(4096 * (L * 6 + L + 6), dtype=torch.float64, device="cuda")
    gW = torch.zeros(L * K, device="cuda")
    gbw, gbn = torch.zeros(L, device="cuda"), torch.zeros(K, device="cuda")
    lib.pdg_wgrad_narrow(M, wide.data_ptr(), narrow.data_ptr(), K, transpose, part.data_ptr(), gW.data_ptr(),
                         gbw.data_ptr(), gbn.data_ptr(), s)
    T = wide.double().T @ narrow.double()   # (128, K)
    ref = T.T.reshape(-1) if transpose else T.reshape(-1)
    assert rel(gW, ref) < 1e-6
    assert rel(gbw, wide.double().sum(0)) < 1e-6 and rel(gbn, narrow.double().sum(0)) < 1e-6


def test_transpose_strided(env):
    lib, sh, _ = env
    W = rnd(L, 3 * L)
    out = torch.empty(L, L, device="cuda")
    lib.pdg_transpose(L, L, 3 * L, W.data_ptr() + 4 * 2 * L, out.data_ptr(), sh())
    assert torch.equal(out.cpu(), W[:, 2 * L:].T.contiguous().cpu())


@pytest.mark.parametrize("e_is_sum", [0, 1])
@pytest.mark.parametrize("N,E,isolated", [(300, 2500, 0), (300, 2500, 7), (5000, 30000, 3)])
def test_pq_scatter_bwd(env, N, E, isolated, e_is_sum):
    """Heavy node (in-degree N/7 > the 8 rows kept in flight), random degrees, and `isolated`
    trailing nodes with no edge at all (their row pointers equal E: nothing may be read there).
    e_is_sum: the second array is gC = gz1m + gz1e (fp32, as the edge backward writes it) and the
    kernel forms gz1e = gC - gz1m per row; checked against the exact gz1e in fp64."""
    lib, sh, _ = env
    s = sh()
    src, dst, rp = _csr(N - isolated, E, seed=3)
    rp = torch.cat([rp, rp[-1:].expand(isolated)])
    key2 = src * N + dst
    perm_src = torch.sort(key2, stable=True).indices
    rps = torch.zeros(N + 1, dtype=torch.int64)
    rps[1:] = torch.cumsum(torch.bincount(src, minlength=N), 0)
    gm, ge = rnd(E, L), rnd(E, L)
    gP, gQ = torch.empty(N, L, device="cuda"), torch.empty(N, L, device="cuda")
    # keep every device array referenced until the kernel has run (no temporaries)
    rp_d, rps_d, perm_d = rp.int().cuda(), rps.int().cuda(), perm_src.int().cuda()
    g2 = gm + ge if e_is_sum else ge
    lib.pdg_pq_scatter_bwd(N, rp_d.data_ptr(), rps_d.data_ptr(), perm_d.data_ptr(), gm.data_ptr(), g2.data_ptr(),
                           e_is_sum, gP.data_ptr(), gQ.data_ptr(), s)
    z = lambda: torch.zeros(N, L, dtype=torch.float64)
    refP = z().index_add_(0, dst, gm.double().cpu()).index_add_(0, src, ge.double().cpu())
    refQ = z().index_add_(0, src, gm.double().cpu()).index_add_(0, dst, ge.double().cpu())
    assert rel(gP, refP) < TOL and rel(gQ, refQ) < TOL


def test_pq_scatter_bwd_gz1e_from_gc_under_cancellation(env):
    """e_is_sum with |gz1e| = 1e-4 |gz1m| (gC dominated by gz1m): the formed row gz1e = gC - gz1m is
    exact up to the one rounding of gC (Sterbenz: gC and gz1m within a factor 2), so its absolute
    error is <= 2^-24 |gC| (~6e-4 of |gz1e| here) and gP / gQ, whose own magnitude is |gz1m|'s, stay at
    fp32 accuracy against the exact sums (pdg_pq_scatter_bwd)."""
    lib, sh, _ = env
    s = sh()
    N, E = 5000, 30000
    src, dst, rp = _csr(N, E, seed=4)
    perm_src = torch.sort(src * N + dst, stable=True).indices
    rps = torch.zeros(N + 1, dtype=torch.int64)
    rps[1:] = torch.cumsum(torch.bincount(src, minlength=N), 0)
    gm, ge = rnd(E, L), rnd(E, L, scale=1e-4)
    gC = gm + ge
    out = {}
    rp_d, rps_d, perm_d = rp.int().cuda(), rps.int().cuda(), perm_src.int().cuda()
    for e_is_sum, g2 in ((1, gC), (0, ge)):
        gP, gQ = torch.empty(N, L, device="cuda"), torch.empty(N, L, device="cuda")
        lib.pdg_pq_scatter_bwd(N, rp_d.data_ptr(), rps_d.data_ptr(), perm_d.data_ptr(), gm.data_ptr(), g2.data_ptr(),
                               e_is_sum, gP.data_ptr(), gQ.data_ptr(), s)
        out[e_is_sum] = (gP, gQ)
    z = lambda: torch.zeros(N, L, dtype=torch.float64)
    ge_x = gC.double().cpu() - gm.double().cpu()     # the exact gz1e the fp32 gC encodes
    refP = z().index_add_(0, dst, gm.double().cpu()).index_add_(0, src, ge_x)
    refQ = z().index_add_(0, src, gm.double().cpu()).index_add_(0, dst, ge_x)
    gP, gQ = out[1]
    assert rel(gP, refP) < TOL and rel(gQ, refQ) < TOL
    # against the stored-gz1e form: the difference is the gz1e rows' rounding, <= 2^-24 |gC| per row
    # (+ the two fp32 accumulations' own rounding, the recursive-summation bound deg * 2^-24 * sum|terms| each)
    aC = gC.double().abs().cpu()
    bP = z().index_add_(0, src, aC) * 2.0 ** -24
    A = z().index_add_(0, dst, gm.double().abs().cpu()).index_add_(0, src, aC)
    deg = (torch.bincount(dst, minlength=N) + torch.bincount(src, minlength=N)).double().unsqueeze(1)
    dP = (out[1][0].double() - out[0][0].double()).abs().cpu()
    assert float((dP - bP - 2.0 ** -23 * deg * A).max()) <= 0.0


def test_ln_colsum_and_mlp2_bwd_vs_autograd(env):
    """LayerNorm(graph) -> relu -> Linear backward of one MLP tail, against torch autograd in fp64."""
    lib, sh, _ = env
    s = sh()
    M = 1500
    a1 = torch.relu(rnd(M, L))
    W, b = lin(L, L)
    g, beta = (rnd(L) * 0.3 + 1.0), rnd(L) * 0.1
    a2 = torch.empty(M, L, device="cuda")
    part = torch.empty(4096 * 256, dtype=torch.float64, device="cuda")
    n = ctypes.c_int(0)
    lib.pdg_mlp2_fwd(M, a1.data_ptr(), W.data_ptr(), b.data_ptr(), a2.data_ptr(), part.data_ptr(), ctypes.byref(n), s)
    st = finalize(lib, s, part, n.value, M * L)
    gy = rnd(M, L)
    lib.pdg_ln_colsum(M, gy.data_ptr(), None, a2.data_ptr(), st.data_ptr(), part.data_ptr(), ctypes.byref(n), None,
                      None, 0, s)
    gg, gb = torch.zeros(L, device="cuda"), torch.zeros(L, device="cuda")
    lb = torch.zeros(24, dtype=torch.uint8, device="cuda")
    lib.pdg_ln_colsum_finalize(part.data_ptr(), n.value, g.data_ptr(), st.data_ptr(), gg.data_ptr(), gb.data_ptr(),
                               lb.data_ptr(), s)
    WT = W.T.contiguous()
    gz2, gz1 = torch.empty(M, L, device="cuda"), torch.empty(M, L, device="cuda")
    lib.pdg_mlp2_bwd(M, gy.data_ptr(), None, a2.data_ptr(), a1.data_ptr(), st.data_ptr(), lb.data_ptr(),
                     g.data_ptr(), WT.data_ptr(), gz2.data_ptr(), gz1.data_ptr(), None, 0, s)
    # the launch-free form: the producer accumulates column rows and writes (S1, S2) pairs, the
    # consumer reduces the pairs, pdg_ln_param_grads turns the accumulator into g / b gradients
    acc = torch.zeros(4096 * 256, dtype=torch.float64, device="cuda")
    pairs = torch.zeros(4096 * 2, dtype=torch.float64, device="cuda")
    for rep in range(2):      # accumulate twice: the accumulator holds 2x the sums
        lib.pdg_ln_colsum(M, gy.data_ptr(), None, a2.data_ptr(), st.data_ptr(), acc.data_ptr(), ctypes.byref(n),
                          g.data_ptr(), pairs.data_ptr(), 1, s)
    gz2p, gz1p = torch.empty(M, L, device="cuda"), torch.empty(M, L, device="cuda")
    lib.pdg_mlp2_bwd(M, gy.data_ptr(), None, a2.data_ptr(), a1.data_ptr(), st.data_ptr(), None,
                     g.data_ptr(), WT.data_ptr(), gz2p.data_ptr(), gz1p.data_ptr(), pairs.data_ptr(), n.value, s)
    assert rel(gz2p, gz2) < 1e-6 and rel(gz1p, gz1) < 1e-6
    gg2, gb2 = torch.zeros(L, device="cuda"), torch.zeros(L, device="cuda")
    P = ctypes.c_void_p
    lib.pdg_ln_param_grads(1, (P * 1)(acc.data_ptr()), (ctypes.c_int * 1)(n.value), (P * 1)(gg2.data_ptr()),
                           (P * 1)(gb2.data_ptr()), s)
    assert rel(gg2, 2 * gg.double().cpu()) < 1e-6 and rel(gb2, 2 * gb.double().cpu()) < 1e-6
    # reference
    a1d = a1.double().cpu().requires_grad_(True)
    Wd, bd = W.double().cpu(), b.double().cpu()
    gd, betad = g.double().cpu().requires_grad_(True), beta.double().cpu().requires_grad_(True)
    z2 = (a1d @ Wd.T + bd)
    z2.retain_grad()
    out = ln_ref(torch.relu(z2), gd, betad)
    out.backward(gy.double().cpu())
    assert rel(gg, gd.grad) < 1e-5 and rel(gb, betad.grad) < 1e-5
    assert rel(gz2, z2.grad) < 1e-5
    assert rel(gz1, (z2.grad @ Wd) * (a1d.detach() > 0)) < 1e-5


def test_wgrad_segments_reduce(env):
    """Segmented weight gradient: ragged segments (not multiples of the 32-row tile), one pass."""
    lib, sh, _ = env
    s = sh()
    rows = [1, 33, 2000, 777, 4096, 5]
    Gs = [rnd(r, L) for r in rows]
    Xs = [rnd(r, L) for r in rows]
    ns = 61
    slabs = torch.empty(ns, L * L + L, device="cuda")
    gp = (ctypes.c_void_p * len(rows))(*[g.data_ptr() for g in Gs])
    xp = (ctypes.c_void_p * len(rows))(*[x.data_ptr() for x in Xs])
    rw = (ctypes.c_int * len(rows))(*rows)
    lib.pdg_wgrad_segments(len(rows), gp, xp, rw, slabs.data_ptr(), ns, s)
    gW = torch.zeros(L, 2 * L, device="cuda")
    gb = torch.zeros(L, device="cuda")
    lib.pdg_wgrad_reduce(slabs.data_ptr(), ns, gW.data_ptr(), 2 * L, L, gb.data_ptr(), s)
    ref = sum(g.double().T @ x.double() for g, x in zip(Gs, Xs))
    err = rel(gW[:, L:], ref)
    print(f"wgrad_segments rel err {err:.3e}")
    assert err < 2e-6
    assert float(gW[:, :L].abs().max()) == 0
    assert rel(gb, sum(g.double().sum(0) for g in Gs)) < 1e-6


def test_wgrad_segments_dynamic_range(env):
    """Operands spanning 30 decades (the three-term bf16 split must stay exact across exponents):
    elementwise error of each weight-gradient entry against its fp64 value, relative to the
    sum of |G||X| products behind it (the scale of fp32 rounding)."""
    lib, sh, _ = env
    s = sh()
    rows = [3000, 517]
    gen = torch.Generator(device="cuda").manual_seed(5)
    def wild(r):
        mag = 10.0 ** (torch.rand(r, L, device="cuda", generator=gen) * 30 - 15)
        return (torch.randn(r, L, device="cuda", generator=gen) * mag).float()
    Gs = [wild(r) * 1e-3 for r in rows]
    Xs = [wild(r) for r in rows]
    ns = 37
    slabs = torch.empty(ns, L * L + L, device="cuda")
    gp = (ctypes.c_void_p * len(rows))(*[g.data_ptr() for g in Gs])
    xp = (ctypes.c_void_p * len(rows))(*[x.data_ptr() for x in Xs])
    rw = (ctypes.c_int * len(rows))(*rows)
    lib.pdg_wgrad_segments(len(rows), gp, xp, rw, slabs.data_ptr(), ns, s)
    gW = torch.zeros(L, L, device="cuda")
    lib.pdg_wgrad_reduce(slabs.data_ptr(), ns, gW.data_ptr(), L, 0, None, s)
    ref = sum(g.double().T @ x.double() for g, x in zip(Gs, Xs))
    scale = sum(g.double().abs().T @ x.double().abs() for g, x in zip(Gs, Xs))
    worst = float(((gW.double() - ref).abs() / scale).max())
    print(f"wgrad_segments dynamic-range worst |err|/sum|GX| {worst:.3e}")
    assert worst < 1e-6


@pytest.mark.parametrize("N", [5, 1031, 4099, 8209, 40328, 100489])
def test_node_net_matches_separate_kernels(env, N):
    """Fused node_net (register-stationary weights, unbiased bf16x6 products) against pdg_node_mlp1 +
    pdg_mlp2_fwd (fp32 MFMA) and float64 torch: each layer's product (fed the fused kernel's own a1 for
    layer 2) within 1e-6 of fp64, no less accurate than the fp32 kernels and without a mean bias; the
    LayerNorm partial totals equal to the fused a2's to fp32 rounding; the inference form (a1n not
    stored) bitwise the training form."""
    lib, sh, _ = env
    s = sh()
    aggr = rnd(N, L) * 3.0
    x = rnd(N, L)
    W1, b1 = lin(L, 2 * L)
    W2, b2 = lin(L, L)
    n = ctypes.c_int(0)
    a10, a20 = torch.empty(N, L, device="cuda"), torch.empty(N, L, device="cuda")
    part0 = torch.zeros(4096, dtype=torch.float64, device="cuda")
    lib.pdg_node_mlp1(N, aggr.data_ptr(), x.data_ptr(), W1.data_ptr(), b1.data_ptr(), a10.data_ptr(), s)
    lib.pdg_mlp2_fwd(N, a10.data_ptr(), W2.data_ptr(), b2.data_ptr(), a20.data_ptr(), part0.data_ptr(),
                     ctypes.byref(n), s)
    a11, a21 = torch.empty(N, L, device="cuda"), torch.empty(N, L, device="cuda")
    part1 = torch.zeros(4096, dtype=torch.float64, device="cuda")
    assert lib.pdg_node_net(N, aggr.data_ptr(), x.data_ptr(), W1.data_ptr(), b1.data_ptr(), W2.data_ptr(),
                            b2.data_ptr(), a11.data_ptr(), a21.data_ptr(), part1.data_ptr(), ctypes.byref(n), s) == 0
    n1 = n.value
    # layer 1 (pre-activation compared where both relu outputs are positive) and layer 2 on the fused a1
    z1 = torch.cat([aggr, x], 1).double() @ W1.double().T + b1.double()
    h1 = torch.relu(z1)
    assert rel(a11, h1) < 1e-6 and rel(a11, h1) <= rel(a10, h1) * 1.05 + 1e-9, (rel(a11, h1), rel(a10, h1))
    h2 = torch.relu(a11.double() @ W2.double().T + b2.double())
    h2_0 = torch.relu(a10.double() @ W2.double().T + b2.double())
    assert rel(a21, h2) < 1e-6 and rel(a21, h2) <= rel(a20, h2_0) * 1.05 + 1e-9, (rel(a21, h2), rel(a20, h2_0))
    if N >= 1000:   # mean signed error of layer 1 relative to the product scale (one bf16x6 chain: ~ -1e-9)
        scale = torch.cat([aggr, x], 1).double().abs() @ W1.double().abs().T
        pos = (a11 > 0) & (z1 > 0)
        bias = float(((a11.double() - z1) / scale.clamp_min(1e-30))[pos].mean())
        assert abs(bias) < 3e-10, bias
    t1 = part1[: 2 * n1].view(n1, 2).sum(0)
    a2d = a21.double()
    assert rel(t1, torch.stack([a2d.sum(), a2d.square().sum()])) < 1e-7
    a2i = torch.empty(N, L, device="cuda")   # inference form: a1n not stored
    lib.pdg_node_net(N, aggr.data_ptr(), x.data_ptr(), W1.data_ptr(), b1.data_ptr(), W2.data_ptr(), b2.data_ptr(),
                     None, a2i.data_ptr(), part1.data_ptr(), ctypes.byref(n), s)
    assert torch.equal(a2i, a21)
    h2f = torch.relu(h1 @ W2.double().T + b2.double())
    assert rel(a21, h2f) < TOL


@pytest.mark.parametrize("N", [7, 1031, 40328])
def test_node_bwd_matches_separate_kernels(env, N):
    """Fused node_net backward == pdg_mlp2_bwd + pdg_gemm_dual (res1 = gy) bitwise."""
    import struct
    lib, sh, _ = env
    s = sh()
    gy = rnd(N, L)
    a1 = torch.relu(rnd(N, L))
    a2 = torch.relu(rnd(N, L))
    g = rnd(L) * 0.3 + 1.0
    W2T, _ = lin(L, L)
    WaT, _ = lin(L, L)
    WbT, _ = lin(L, L)
    r64 = a2.double()
    mean, sd = float(r64.mean()), float(r64.std(unbiased=False))
    den = float(torch.tensor(sd, dtype=torch.float32) + 1e-5)
    st = torch.frombuffer(bytearray(struct.pack("ffffddd", mean, den, 1.0 / den, sd, mean, sd, N * L)),
                          dtype=torch.uint8).cuda()
    lb = torch.frombuffer(bytearray(struct.pack("ffdd", 0.013, -0.021, 1.0, 2.0)), dtype=torch.uint8).cuda()
    outs0 = [torch.empty(N, L, device="cuda") for _ in range(4)]
    lib.pdg_mlp2_bwd(N, gy.data_ptr(), None, a2.data_ptr(), a1.data_ptr(), st.data_ptr(), lb.data_ptr(),
                     g.data_ptr(), W2T.data_ptr(), outs0[0].data_ptr(), outs0[1].data_ptr(), None, 0, s)
    lib.pdg_gemm_dual(N, outs0[1].data_ptr(), WaT.data_ptr(), WbT.data_ptr(), None, gy.data_ptr(),
                      outs0[2].data_ptr(), outs0[3].data_ptr(), s)
    outs1 = [torch.empty(N, L, device="cuda") for _ in range(4)]
    assert lib.pdg_node_bwd(N, gy.data_ptr(), a2.data_ptr(), a1.data_ptr(), st.data_ptr(), lb.data_ptr(),
                            g.data_ptr(), W2T.data_ptr(), WaT.data_ptr(), WbT.data_ptr(), *[o.data_ptr() for o in outs1],
                            None, 0, s) == 0
    for a, b in zip(outs0, outs1):
        assert torch.equal(a, b)
    # the backward scalars from producer pairs instead of a finalized pdg_ln_bwd: dyadic pieces of
    # (S1, S2) sum exactly, so c1 / c2 and therefore every output are bitwise those of lb
    S1, S2 = 37.25, -12.5
    M, sdv = float(N * L), sd
    lb2 = torch.frombuffer(bytearray(struct.pack("ffdd", S1 / M, S2 / (M * sdv), S1, S2)), dtype=torch.uint8).cuda()
    pairs = torch.tensor([[S1 / 2, S2 / 4], [S1 / 4, S2 / 2], [S1 / 4, S2 / 4]], dtype=torch.float64).cuda()
    outs2, outs3 = ([torch.empty(N, L, device="cuda") for _ in range(4)] for _ in range(2))
    assert lib.pdg_node_bwd(N, gy.data_ptr(), a2.data_ptr(), a1.data_ptr(), st.data_ptr(), lb2.data_ptr(),
                            g.data_ptr(), W2T.data_ptr(), WaT.data_ptr(), WbT.data_ptr(), *[o.data_ptr() for o in outs2],
                            None, 0, s) == 0
    assert lib.pdg_node_bwd(N, gy.data_ptr(), a2.data_ptr(), a1.data_ptr(), st.data_ptr(), None,
                            g.data_ptr(), W2T.data_ptr(), WaT.data_ptr(), WbT.data_ptr(), *[o.data_ptr() for o in outs3],
                            pairs.data_ptr(), 3, s) == 0
    for a, b in zip(outs2, outs3):
        assert torch.equal(a, b)


@pytest.mark.parametrize("N,res", [(7, True), (1031, False), (4099, True), (8209, False), (40328, True),
                                   (100489, False)])
def test_register_weight_kernels_match_lds_kernels(env, N, res):
    """pdg_node_pq_rw / pdg_gemm_sum2_rw (weights in registers) against pdg_node_pq / pdg_gemm_sum2
    (weights in LDS): x_t and the gemm_sum2 outputs bitwise; P / Q (bf16x6 products with the unbiased
    accumulation, gemm_x6f) against the fp64 products of the same x_t: relative L2 error below 1e-6,
    no larger than the fp32-MFMA kernel's, and no mean bias beyond 3e-10 of the product scale."""
    import struct
    lib, sh, _ = env
    s = sh()
    a2 = torch.relu(rnd(N, L))
    xr = rnd(N, L) if res else None
    g, b = rnd(L) * 0.3 + 1.0, rnd(L) * 0.1
    W1, _ = lin(L, 3 * L)
    r64 = a2.double()
    mean, sd = float(r64.mean()), float(r64.std(unbiased=False))
    den = float(torch.tensor(sd, dtype=torch.float32) + 1e-5)
    st = torch.frombuffer(bytearray(struct.pack("ffffddd", mean, den, 1.0 / den, sd, mean, sd, N * L)),
                          dtype=torch.uint8).cuda()
    outs = []
    # pdg_node_pq (LDS weights) writes two N x 128 arrays; pdg_node_pq_rw the library's P / Q layout
    x, P, Q = (torch.empty(N, L, device="cuda") for _ in range(3))
    assert lib.pdg_node_pq(N, a2.data_ptr(), st.data_ptr(), g.data_ptr(), b.data_ptr(),
                           xr.data_ptr() if res else None, x.data_ptr(), W1.data_ptr(), P.data_ptr(), Q.data_ptr(),
                           s) == 0
    outs.append((x, P, Q))
    x, pq = torch.empty(N, L, device="cuda"), PQ(lib, N)
    assert lib.pdg_node_pq_rw(N, a2.data_ptr(), st.data_ptr(), g.data_ptr(), b.data_ptr(),
                              xr.data_ptr() if res else None, x.data_ptr(), W1.data_ptr(), pq.p, pq.q, s) == 0
    outs.append((x, *pq.unpack()))
    assert torch.equal(outs[0][0], outs[1][0])
    x64 = outs[1][0].double()
    for k, Wk in ((1, W1[:, :L]), (2, W1[:, L:2 * L])):
        ref = x64 @ Wk.double().t()
        scale = x64.abs() @ Wk.double().abs().t()
        e_rw, e_lds = rel(outs[1][k], ref), rel(outs[0][k], ref)
        assert e_rw < 1e-6 and e_rw <= e_lds * 1.05 + 1e-9, (k, e_rw, e_lds)
        if N >= 1000:   # noise floor ~ 1e-8 / sqrt(N * 128); one bf16x6 MFMA chain measured -1.1e-9
            bias = float(((outs[1][k].double() - ref) / scale.clamp_min(1e-30)).mean())
            assert abs(bias) < 3e-10, (k, bias)
    i0, i1 = rnd(N, L), rnd(N, L)
    W0T, _ = lin(L, L)
    W1T, _ = lin(L, L)
    rr = rnd(N, L) if res else None
    o = []
    out = torch.empty(N, L, device="cuda")
    assert lib.pdg_gemm_sum2(N, i0.data_ptr(), i1.data_ptr(), W0T.data_ptr(), W1T.data_ptr(),
                             rr.data_ptr() if res else None, out.data_ptr(), s) == 0
    o.append(out)
    part = torch.full((lib.pdg_max_blocks() * 256,), float("nan"), dtype=torch.float64, device="cuda")
    pairs = torch.full((lib.pdg_max_blocks() * 2,), float("nan"), dtype=torch.float64, device="cuda")
    npart = ctypes.c_int(0)
    for cols in (False, True):
        out = torch.empty(N, L, device="cuda")
        assert lib.pdg_gemm_sum2_rw(N, i0.data_ptr(), i1.data_ptr(), W0T.data_ptr(), W1T.data_ptr(),
                                    rr.data_ptr() if res else None, out.data_ptr(), a2.data_ptr() if cols else None,
                                    st.data_ptr() if cols else None, part.data_ptr() if cols else None,
                                    ctypes.byref(npart), g.data_ptr() if cols else None,
                                    pairs.data_ptr() if cols else None, 0, s) == 0
        o.append(out)
    assert torch.equal(o[0], o[1]) and torch.equal(o[0], o[2])
    # the LayerNorm column partials folded into the _rw kernel (pdg_ln_colsum formulas)
    got = part[:npart.value * 256].view(-1, 256).sum(0).cpu()
    gyv = o[0].double().cpu()
    xhat = ((a2.double() - mean) / den).cpu()
    ref = torch.cat([gyv.sum(0), (gyv * xhat).sum(0)])
    assert rel(got, ref) < 1e-6
    sp = pairs[:2 * npart.value].view(-1, 2).sum(0).cpu()
    gd = g.double().cpu()
    assert rel(sp, torch.stack([(gd * got[:L]).sum(), (gd * got[L:]).sum()])) < 1e-9


@pytest.mark.parametrize("N,E,nparts,both", [(7, 30, 1, True), (1031, 6000, 37, False), (40328, 239744, 256, True)])
def test_segment_sum_fin_equals_finalize2_then_segment_sum(env, N, E, nparts, both):
    """pdg_segment_sum_fin (the edge LayerNorms' statistics reduced inside the segment sum) is bitwise
    pdg_ln_finalize2 (or pdg_ln_finalize) + pdg_segment_sum: the sums, the x-hat sums and both 40-byte
    statistics it stores."""
    lib, sh, _ = env
    s = sh()
    src, dst, rp = _csr(N, E)
    rows = torch.relu(rnd(E, L))
    other = torch.relu(rnd(E, L)) * 0.5
    g, b = rnd(L) + 1.0, rnd(L)
    rp_d = rp.int().cuda()
    edges = torch.linspace(0, E, nparts + 1).round().long().tolist()

    def partials(a):
        a64 = a.double()
        return torch.stack([torch.stack([a64[i:j].sum(), a64[i:j].square().sum()])
                            for i, j in zip(edges[:-1], edges[1:])]).reshape(-1).cuda()
    pa, pb = partials(rows), partials(other)
    outs = []
    for fin in (False, True):
        st_a = torch.full((40,), 0xAB, dtype=torch.uint8, device="cuda")
        st_b = torch.full((40,), 0xCD, dtype=torch.uint8, device="cuda")
        out, xs = torch.empty(N, L, device="cuda"), torch.empty(N, L, device="cuda")
        if fin:
            assert lib.pdg_segment_sum_fin(N, rp_d.data_ptr(), rows.data_ptr(), pa.data_ptr(),
                                           pb.data_ptr() if both else None, nparts, float(E * L), st_a.data_ptr(),
                                           st_b.data_ptr() if both else None, g.data_ptr(), b.data_ptr(),
                                           out.data_ptr(), xs.data_ptr(), s) == 0
        else:
            if both:
                lib.pdg_ln_finalize2(pa.data_ptr(), pb.data_ptr(), nparts, float(E * L), st_a.data_ptr(),
                                     st_b.data_ptr(), s)
            else:
                lib.pdg_ln_finalize(pa.data_ptr(), nparts, float(E * L), st_a.data_ptr(), s)
            lib.pdg_segment_sum(N, rp_d.data_ptr(), rows.data_ptr(), st_a.data_ptr(), g.data_ptr(), b.data_ptr(),
                                out.data_ptr(), xs.data_ptr(), s)
        torch.cuda.synchronize()
        outs.append((st_a, st_b if both else None, out, xs))
    for u, v in zip(*outs):
        assert (u is None and v is None) or torch.equal(u, v)


@pytest.mark.parametrize("N,nparts,res", [(7, 1, True), (1031, 37, False), (40328, 256, True), (5000, 700, False)])
def test_node_pq_rw_fin_equals_finalize_then_pq_rw(env, N, nparts, res):
    """pdg_node_pq_rw_fin (node LayerNorm statistics reduced inside the consumer) is bitwise
    pdg_ln_finalize + pdg_node_pq_rw: x_out, P, Q and the 40-byte pdg_ln_stat it stores, for
    nparts below, at and above one 256-thread reduction round (advisor round 1)."""
    lib, sh, _ = env
    s = sh()
    a2 = torch.relu(rnd(N, L))
    xr = rnd(N, L) if res else None
    g, b = rnd(L) * 0.3 + 1.0, rnd(L) * 0.1
    W1, _ = lin(L, 3 * L)
    # partials as pdg_node_net writes them: (sum, sumsq) per block, here of row slices of a2
    edges = torch.linspace(0, N, nparts + 1).round().long().tolist()
    a64 = a2.double()
    part = torch.stack([torch.stack([a64[i:j].sum(), a64[i:j].square().sum()])
                        for i, j in zip(edges[:-1], edges[1:])]).reshape(-1).cuda()
    st_ref = finalize(lib, s, part, nparts, N * L)
    outs = []
    x, pq = torch.empty(N, L, device="cuda"), PQ(lib, N)
    assert lib.pdg_node_pq_rw(N, a2.data_ptr(), st_ref.data_ptr(), g.data_ptr(), b.data_ptr(),
                              xr.data_ptr() if res else None, x.data_ptr(), W1.data_ptr(), pq.p, pq.q, s) == 0
    outs.append((x, *pq.unpack()))
    st_fin = torch.full((40,), 0xAB, dtype=torch.uint8, device="cuda")
    x, pq = torch.empty(N, L, device="cuda"), PQ(lib, N)
    assert lib.pdg_node_pq_rw_fin(N, a2.data_ptr(), part.data_ptr(), nparts, float(N * L), st_fin.data_ptr(),
                                  g.data_ptr(), b.data_ptr(), xr.data_ptr() if res else None, x.data_ptr(),
                                  W1.data_ptr(), pq.p, pq.q, s) == 0
    outs.append((x, *pq.unpack()))
    torch.cuda.synchronize()
    assert torch.equal(st_ref, st_fin)
    for u, v in zip(*outs):
        assert torch.equal(u, v)


@pytest.mark.parametrize("N,nparts,scale", [(7, 1, 1), (1031, 37, 0), (40328, 256, 1), (5000, 700, 0)])
def test_decoder_fwd_fin_equals_finalize_then_decoder(env, N, nparts, scale):
    """pdg_decoder_fwd_fin (the last node LayerNorm's statistics reduced inside the decoder) is bitwise
    pdg_ln_finalize + pdg_decoder_fwd: x_S, a1d, y and the stored pdg_ln_stat."""
    lib, sh, _ = env
    s = sh()
    a2 = torch.relu(rnd(N, L))
    xr = rnd(N, L)
    g, b = rnd(L) * 0.3 + 1.0, rnd(L) * 0.1
    Wd1, bd1 = lin(L, L)
    Wd2, bd2 = lin(3, L)
    st8 = torch.tensor([0.1, 1.2, -0.3, 2.0, 0.25, 3.5, 0.05, 0.7], device="cuda")
    edges = torch.linspace(0, N, nparts + 1).round().long().tolist()
    a64 = a2.double()
    part = torch.stack([torch.stack([a64[i:j].sum(), a64[i:j].square().sum()])
                        for i, j in zip(edges[:-1], edges[1:])]).reshape(-1).cuda()
    st_ref = finalize(lib, s, part, nparts, N * L)
    outs = []
    xs, a1, y = torch.empty(N, L, device="cuda"), torch.empty(N, L, device="cuda"), torch.empty(N, 3, device="cuda")
    assert lib.pdg_decoder_fwd(N, a2.data_ptr(), st_ref.data_ptr(), g.data_ptr(), b.data_ptr(), xr.data_ptr(),
                               xs.data_ptr(), Wd1.data_ptr(), bd1.data_ptr(), a1.data_ptr(), Wd2.data_ptr(),
                               bd2.data_ptr(), st8.data_ptr(), scale, y.data_ptr(), s) == 0
    outs.append((xs, a1, y))
    st_fin = torch.full((40,), 0xAB, dtype=torch.uint8, device="cuda")
    xs, a1, y = torch.empty(N, L, device="cuda"), torch.empty(N, L, device="cuda"), torch.empty(N, 3, device="cuda")
    assert lib.pdg_decoder_fwd_fin(N, a2.data_ptr(), part.data_ptr(), nparts, float(N * L), st_fin.data_ptr(),
                                   g.data_ptr(), b.data_ptr(), xr.data_ptr(), xs.data_ptr(), Wd1.data_ptr(),
                                   bd1.data_ptr(), a1.data_ptr(), Wd2.data_ptr(), bd2.data_ptr(), st8.data_ptr(),
                                   scale, y.data_ptr(), s) == 0
    outs.append((xs, a1, y))
    torch.cuda.synchronize()
    assert torch.equal(st_ref, st_fin)
    for u, v in zip(*outs):
        assert torch.equal(u, v)


@pytest.mark.parametrize("N,nparts,scale,nb", [(7, 1, 1, 37), (1031, 37, 0, 37), (40328, 256, 1, 256),
                                                (5000, 700, 0, 256)])
def test_decoder_fwd_coop_vs_decoder_fwd(env, N, nparts, scale, nb):
    """pdg_decoder_fwd_coop against pdg_decoder_fwd_fin on the same inputs: x_S and the stored statistics
    bitwise (with the statistics reduced in-kernel, and given as st); a1d within 1e-6 of fp64 on x_S, no less
    accurate than the fp32-MFMA kernel, no mean bias beyond 3e-10 of the product scale; y within 1e-6 of the
    fp64 decoder on the kernel's own a1d and of the fp32 kernel's y; rows past N untouched."""
    lib, sh, _ = env
    s = sh()
    a2 = torch.relu(rnd(N, L))
    xr = rnd(N, L)
    g, b = rnd(L) * 0.3 + 1.0, rnd(L) * 0.1
    Wd1, bd1 = lin(L, L)
    Wd2, bd2 = lin(3, L)
    st8 = torch.tensor([0.1, 1.2, -0.3, 2.0, 0.25, 3.5, 0.05, 0.7], device="cuda")
    edges = torch.linspace(0, N, nparts + 1).round().long().tolist()
    a64 = a2.double()
    part = torch.stack([torch.stack([a64[i:j].sum(), a64[i:j].square().sum()])
                        for i, j in zip(edges[:-1], edges[1:])]).reshape(-1).cuda()
    st_ref = torch.full((40,), 0xAB, dtype=torch.uint8, device="cuda")
    xs0, a10, y0 = torch.empty(N, L, device="cuda"), torch.empty(N, L, device="cuda"), torch.empty(N, 3, device="cuda")
    assert lib.pdg_decoder_fwd_fin(N, a2.data_ptr(), part.data_ptr(), nparts, float(N * L), st_ref.data_ptr(),
                                   g.data_ptr(), b.data_ptr(), xr.data_ptr(), xs0.data_ptr(), Wd1.data_ptr(),
                                   bd1.data_ptr(), a10.data_ptr(), Wd2.data_ptr(), bd2.data_ptr(), st8.data_ptr(),
                                   scale, y0.data_ptr(), s) == 0
    for fin in (True, False):
        st_c = torch.full((40,), 0xCD, dtype=torch.uint8, device="cuda")
        xs, a1, y = (torch.full((N + 40, c), float("nan"), device="cuda") for c in (L, L, 3))
        assert lib.pdg_decoder_fwd_coop(N, a2.data_ptr(), None if fin else st_ref.data_ptr(),
                                        part.data_ptr() if fin else None, nparts if fin else 0, float(N * L),
                                        st_c.data_ptr() if fin else None, g.data_ptr(), b.data_ptr(), xr.data_ptr(),
                                        xs.data_ptr(), Wd1.data_ptr(), bd1.data_ptr(), a1.data_ptr(), Wd2.data_ptr(),
                                        bd2.data_ptr(), st8.data_ptr(), scale, y.data_ptr(), nb, s) == 0
        torch.cuda.synchronize()
        for t in (xs, a1, y):
            assert torch.isnan(t[N:]).all()
        xs, a1, y = xs[:N], a1[:N], y[:N]
        if fin:
            assert torch.equal(st_c, st_ref)
        assert torch.equal(xs, xs0)
        z = xs.double() @ Wd1.double().T + bd1.double()
        h = torch.relu(z)
        assert rel(a1, h) < 1e-6 and rel(a1, h) <= 1.05 * rel(a10, h) + 1e-9, (rel(a1, h), rel(a10, h))
        if N >= 1000:
            scale_ = xs.double().abs() @ Wd1.double().abs().T + bd1.double().abs()
            pos = (a1 > 0) & (z > 0)
            bias = float(((a1.double() - z) / scale_.clamp_min(1e-30))[pos].mean())
            assert abs(bias) < 3e-10, bias
        yr = a1.double() @ Wd2.double().T + bd2.double()
        if scale:
            yr = yr * float(st8[5]) + float(st8[4])
        assert rel(y, yr) < 1e-6 and rel(y, y0) < 1e-5, (rel(y, yr), rel(y, y0))


@pytest.mark.parametrize("slab_init", [0, 1])
@pytest.mark.parametrize("E", [77, 5000])
def test_edge_enc_bwd_vs_autograd(env, E, slab_init):
    """pdg_edge_enc_bwd (edge encoder backward in one pass, layer-1 output recomputed from the scalar
    input) against torch autograd of Lin(1->128) ReLU Lin(128->128) ReLU LN in fp64: all four
    weight / bias gradients; the encoder forward is run with a1 == NULL (not stored)."""
    lib, sh, _ = env
    s = sh()
    e_in = rnd(E)
    W0, b0 = lin(L, 1)
    W2, b2 = lin(L, L)
    g = rnd(L) * 0.3 + 1.0
    beta = rnd(L) * 0.1
    a2 = torch.empty(E, L, device="cuda")
    part = torch.empty(4096 * 256, dtype=torch.float64, device="cuda")
    n = ctypes.c_int(0)
    lib.pdg_encoder_fwd(E, 1, e_in.data_ptr(), W0.data_ptr(), b0.data_ptr(), W2.data_ptr(), b2.data_ptr(), None,
                        a2.data_ptr(), part.data_ptr(), ctypes.byref(n), s)
    st = finalize(lib, s, part, n.value, E * L)
    gy = rnd(E, L)
    acc = torch.zeros(4096 * 256, dtype=torch.float64, device="cuda")
    pairs = torch.zeros(4096 * 2, dtype=torch.float64, device="cuda")
    lib.pdg_ln_colsum(E, gy.data_ptr(), None, a2.data_ptr(), st.data_ptr(), acc.data_ptr(), ctypes.byref(n),
                      g.data_ptr(), pairs.data_ptr(), 1, s)
    ns = 37
    # slab_init: the slabs are written, not accumulated (their NaN contents must not leak)
    slabs = torch.full((ns, L * L + L), float("nan"), device="cuda") if slab_init else torch.zeros(ns, L * L + L, device="cuda")
    nsum = torch.empty(ns, 2 * L, dtype=torch.float64, device="cuda")
    WT = W2.T.contiguous()
    lib.pdg_edge_enc_bwd(E, gy.data_ptr(), a2.data_ptr(), e_in.data_ptr(), W0.data_ptr(), b0.data_ptr(),
                         st.data_ptr(), None, pairs.data_ptr(), n.value, g.data_ptr(), WT.data_ptr(),
                         slabs.data_ptr(), nsum.data_ptr(), ns, slab_init, s)
    gW2, gb2 = torch.zeros(L, L, device="cuda"), torch.zeros(L, device="cuda")
    gW0, gb0 = torch.zeros(L, 1, device="cuda"), torch.zeros(L, device="cuda")
    lib.pdg_wgrad_reduce(slabs.data_ptr(), ns, gW2.data_ptr(), L, 0, gb2.data_ptr(), s)
    lib.pdg_enc_narrow_reduce(nsum.data_ptr(), ns, gW0.data_ptr(), gb0.data_ptr(), s)
    # reference (fp64 autograd)
    W0d, b0d = W0.double().cpu().requires_grad_(True), b0.double().cpu().requires_grad_(True)
    W2d, b2d = W2.double().cpu().requires_grad_(True), b2.double().cpu().requires_grad_(True)
    a1 = torch.relu(e_in.double().cpu()[:, None] @ W0d.T + b0d)
    out = ln_ref(torch.relu(a1 @ W2d.T + b2d), g.double().cpu(), beta.double().cpu())
    out.backward(gy.double().cpu())
    assert rel(gW2, W2d.grad) < 1e-5 and rel(gb2, b2d.grad) < 1e-5
    assert rel(gW0, W0d.grad) < 1e-5 and rel(gb0, b0d.grad) < 1e-5


@pytest.mark.parametrize("shared_x", [1, 0])
def test_wgrad_pairs_vs_fp64(env, shared_x):
    """pdg_wgrad_pairs: two weight gradients sharing an operand over ragged segments (rows not
    multiples of the 32-row rounds, an empty segment), bias rows = column sums of the G operand(s)."""
    lib, sh, _ = env
    s = sh()
    rows = [1000, 0, 77, 4099]
    A = [[rnd(r, L) for r in rows] for _ in range(3)]
    ns = 41
    slabs = torch.empty(2, ns, L * L + L, device="cuda")
    n = len(rows)
    P = ctypes.c_void_p
    arr = [(P * n)(*[t.data_ptr() for t in A[k]]) for k in range(3)]
    lib.pdg_wgrad_pairs(n, arr[0], arr[1], arr[2], (ctypes.c_int * n)(*rows), shared_x, slabs[0].data_ptr(),
                        slabs[1].data_ptr(), ns, s)
    cat = [torch.cat([t.double().cpu() for t in A[k]]) for k in range(3)]
    if shared_x:
        refs = [(cat[0].T @ cat[2], cat[0].sum(0)), (cat[1].T @ cat[2], cat[1].sum(0))]
    else:
        refs = [(cat[0].T @ cat[1], cat[0].sum(0)), (cat[0].T @ cat[2], cat[0].sum(0))]
    for k in range(2):
        gW = torch.zeros(L, 2 * L, device="cuda")
        gb = torch.zeros(L, device="cuda")
        lib.pdg_wgrad_reduce(slabs[k].data_ptr(), ns, gW.data_ptr(), 2 * L, L * k, gb.data_ptr(), s)
        assert rel(gW[:, L * k:L * (k + 1)], refs[k][0]) < 1e-6, k
        assert float(gW[:, L * (1 - k):L * (2 - k)].abs().max()) == 0.0
        assert rel(gb, refs[k][1]) < 1e-6


def test_transpose128_batch(env):
    """The backward's W^T copies in one launch (strided sources: blocks of edge_net.0's 128 x 384)."""
    lib, sh, _ = env
    W = rnd(L, 3 * L)
    V = rnd(L, L)
    outs = [torch.empty(L, L, device="cuda") for _ in range(4)]
    srcs = [W.data_ptr(), W.data_ptr() + 4 * L, W.data_ptr() + 4 * 2 * L, V.data_ptr()]
    lds = [3 * L, 3 * L, 3 * L, L]
    P = ctypes.c_void_p
    lib.pdg_transpose128_batch(4, (P * 4)(*srcs), (ctypes.c_int * 4)(*lds), (P * 4)(*[o.data_ptr() for o in outs]),
                               sh())
    refs = [W[:, :L], W[:, L:2 * L], W[:, 2 * L:], V]
    for o, r in zip(outs, refs):
        assert torch.equal(o.cpu(), r.T.contiguous().cpu())


@pytest.mark.parametrize("E,eu,res", [(1000, 1, 1), (4099, 0, 1), (77, 1, 0), (1, 1, 1), (33, 0, 0)])
def test_edge_fwd_coop_matches_edge_fwd(env, E, eu, res):
    """pdg_edge_fwd_coop (block-cooperative layout) against pdg_edge_fwd on the same inputs: e_t bitwise;
    the layer-1 outputs (C = Wc e an unbiased bf16x6 product in the coop kernel, fp32 MFMAs in pdg_edge_fwd)
    against fp64 within 1e-6, no less accurate than the fp32 kernel's, and with no sign bias (mean signed
    error below 3e-10 of the product scale); the W2 outputs and the LayerNorm partials to fp32 rounding."""
    lib, sh, _ = env
    s = sh()
    N = 300
    g = torch.Generator().manual_seed(E)
    src = torch.randint(0, N, (E,), generator=g).int().cuda()
    dst = torch.sort(torch.randint(0, N, (E,), generator=g)).values.int().cuda()
    a2p, eres = torch.relu(rnd(E, L)), rnd(E, L)
    Pn, Qn = rnd(N, L), rnd(N, L)
    W1, b1 = lin(L, 3 * L)
    W2, b2 = lin(L, L)
    lg, lbv = rnd(L) * 0.3 + 1.0, rnd(L) * 0.1
    part = torch.empty(4096, dtype=torch.float64, device="cuda")
    n = ctypes.c_int(0)
    tmp = torch.empty(E, L, device="cuda")
    lib.pdg_mlp2_fwd(E, a2p.data_ptr(), W2.data_ptr(), b2.data_ptr(), tmp.data_ptr(), part.data_ptr(),
                     ctypes.byref(n), s)
    st = finalize(lib, s, part, n.value, E * L)
    outs = {}
    for name in ("ref", "coop"):
        o = {k: torch.full((E, L), float("nan"), device="cuda") for k in ("e", "a1m", "a2m", "a1e", "a2e")}
        pm = torch.zeros(4096, dtype=torch.float64, device="cuda")
        pe = torch.zeros(4096, dtype=torch.float64, device="cuda")
        args = (E, a2p.data_ptr(), st.data_ptr(), lg.data_ptr(), lbv.data_ptr(), eres.data_ptr() if res else None,
                o["e"].data_ptr(), src.data_ptr(), dst.data_ptr(), Pn.data_ptr(), Qn.data_ptr(), W1.data_ptr(),
                b1.data_ptr(), W2.data_ptr(), b2.data_ptr(), o["a1m"].data_ptr(), o["a2m"].data_ptr(),
                o["a1e"].data_ptr() if eu else None, o["a2e"].data_ptr() if eu else None)
        if name == "ref":
            lib.pdg_edge_fwd(*args, pm.data_ptr(), pe.data_ptr() if eu else None, eu, ctypes.byref(n), s)
            np_ = n.value
        else:   # P / Q in the layout the library's node pre-pass writes (pdg_pq_layout)
            np_ = 37
            pq = PQ.of(lib, Pn, Qn)
            args = args[:9] + (pq.p, pq.q) + args[11:]
            lib.pdg_edge_fwd_coop(*args, pm.data_ptr(), pe.data_ptr() if eu else None, eu, np_, s)
        outs[name] = (o, pm[: 2 * np_].view(np_, 2).sum(0), pe[: 2 * np_].view(np_, 2).sum(0))
    (o0, pm0, pe0), (o1, pm1, pe1) = outs["ref"], outs["coop"]
    assert torch.equal(o0["e"], o1["e"])
    e64, Wc64 = o1["e"].double(), W1[:, 2 * L:].double()
    c64 = e64 @ Wc64.T + b1.double()
    cscale = e64.abs() @ Wc64.abs().T + b1.double().abs()
    P64, Q64, sl, dl = Pn.double(), Qn.double(), src.long(), dst.long()
    pairs = [("a1m", P64[dl], Q64[sl])] + ([("a1e", P64[sl], Q64[dl])] if eu else [])
    for k, pg, qg in pairs:
        z = c64 + pg + qg
        h = torch.relu(z)
        assert rel(o1[k], h) < 1e-6 and rel(o1[k], h) <= 1.5 * rel(o0[k], h) + 1e-9, (k, rel(o1[k], h), rel(o0[k], h))
        if E >= 1000:
            pos = (o1[k] > 0) & (z > 0)
            scale = (cscale + pg.abs() + qg.abs()).clamp_min(1e-30)
            bias = float(((o1[k].double() - z) / scale)[pos].mean())
            assert abs(bias) < 3e-10, (k, bias)
    for k in ("a2m",) + (("a2e",) if eu else ()):
        assert rel(o1[k], o0[k]) < 1e-6, k
    assert rel(pm1, pm0) < 1e-6
    if eu:
        assert rel(pe1, pe0) < 1e-6


def test_wgrad_reduce_batch_matches_single(env):
    """pdg_wgrad_reduce_batch (every deferred slab reduction of a backward in one launch) against one
    pdg_wgrad_reduce per job and an fp64 sum: column offsets, accumulation into the existing gradient
    and the optional bias honoured, distinct slab counts per job."""
    lib, sh, _ = env
    s = sh()
    SL = L * L + L
    jobs = [(256, 3 * L, 2 * L, True), (512, 2 * L, L, False), (37, L, 0, True)]
    slabs = [rnd(n, SL) for n, _, _, _ in jobs]
    gW0 = [rnd(L, ld) for _, ld, _, _ in jobs]      # pre-existing gradients (accumulated into)
    gb0 = [rnd(L) if hb else None for _, _, _, hb in jobs]
    outs = {}
    for mode in ("single", "batch"):
        gW = [w.clone() for w in gW0]
        gb = [b.clone() if b is not None else None for b in gb0]
        if mode == "single":
            for (n, ld, c0, hb), sl, w, b in zip(jobs, [t.clone() for t in slabs], gW, gb):   # reduces in place
                lib.pdg_wgrad_reduce(sl.data_ptr(), n, w.data_ptr(), ld, c0, b.data_ptr() if hb else None, s)
        else:
            k = len(jobs)
            VP, IA = ctypes.c_void_p * k, ctypes.c_int * k
            lib.pdg_wgrad_reduce_batch(k, VP(*[t.data_ptr() for t in slabs]), IA(*[j[0] for j in jobs]),
                                       VP(*[w.data_ptr() for w in gW]), IA(*[j[1] for j in jobs]),
                                       IA(*[j[2] for j in jobs]),
                                       VP(*[b.data_ptr() if b is not None else None for b in gb]), s)
        outs[mode] = (gW, gb)
    for i, (n, ld, c0, hb) in enumerate(jobs):
        ref = slabs[i].double().sum(0).cpu()
        w0, w1 = outs["single"][0][i], outs["batch"][0][i]
        assert rel(w1, w0) < 1e-6, i
        assert torch.equal(w1[:, :c0], gW0[i][:, :c0]) and torch.equal(w1[:, c0 + L:], gW0[i][:, c0 + L:])
        assert rel(w1[:, c0:c0 + L].double().cpu() - gW0[i][:, c0:c0 + L].double().cpu(), ref[:L * L].view(L, L)) < 1e-5
        if hb:
            assert rel(outs["batch"][1][i].double().cpu() - gb0[i].double().cpu(), ref[L * L:]) < 1e-5


@pytest.mark.parametrize("E,nb", [(77, 37), (4099, 37), (20000, 512)])
def test_edge_enc_fwd_vs_fp64(env, E, nb):
    """pdg_edge_enc_fwd (W2 product in bf16x6, register-stationary) against an fp64 restatement: a2 to fp32
    rounding, the LayerNorm partials' (sum, sum of squares) to 1e-6.  Rows past the edges are not written (the
    NaN fill survives nowhere)."""
    lib, sh, _ = env
    s = sh()
    e_in = rnd(E)
    w0, b0 = lin(L, 1)
    W2, b2 = lin(L, L)
    a2 = torch.full((E + 5, L), float("nan"), device="cuda")
    part = torch.zeros(2 * nb, dtype=torch.float64, device="cuda")
    lib.pdg_edge_enc_fwd(E, e_in.data_ptr(), w0.data_ptr(), b0.data_ptr(), W2.data_ptr(), b2.data_ptr(),
                         a2.data_ptr(), part.data_ptr(), nb, s)
    assert bool(a2[E:].isnan().all())
    a2 = a2[:E]
    a1 = torch.relu(e_in.double()[:, None] * w0.double()[:, 0][None, :] + b0.double())
    ref = torch.relu(a1 @ W2.double().T + b2.double())
    assert rel(a2, ref) < TOL
    p = part.view(nb, 2).sum(0).cpu()
    assert abs(float(p[0]) - float(ref.sum())) <= 1e-6 * float(ref.abs().sum())
    assert abs(float(p[1]) - float((ref * ref).sum())) <= 1e-6 * float((ref * ref).sum())


@pytest.mark.parametrize("N,nb", [(7, 37), (1031, 37), (40328, 256), (100489, 256)])
def test_node_enc_fwd_vs_encoder_fwd(env, N, nb):
    """pdg_node_enc_fwd (node encoder, cooperative layout, unbiased bf16x6 W2 product) against pdg_encoder_fwd
    (LDS weights, fp32 MFMAs) and fp64: a1 bitwise (the same fma order), a2 within 1e-6 of fp64, no less
    accurate than the fp32 kernel, no mean bias beyond 3e-10 of the product scale; the LayerNorm partials'
    totals to 1e-7.  Rows past a block's range (empty blocks when nb exceeds the 32-row rounds) write nothing."""
    lib, sh, _ = env
    s = sh()
    x = rnd(N, 6)
    w0, b0 = lin(L, 6)
    W2, b2 = lin(L, L)
    a1r, a2r = torch.empty(N, L, device="cuda"), torch.empty(N, L, device="cuda")
    pr = torch.zeros(lib.pdg_max_blocks() * 2, dtype=torch.float64, device="cuda")
    n = ctypes.c_int(0)
    assert lib.pdg_encoder_fwd(N, 6, x.data_ptr(), w0.data_ptr(), b0.data_ptr(), W2.data_ptr(), b2.data_ptr(),
                               a1r.data_ptr(), a2r.data_ptr(), pr.data_ptr(), ctypes.byref(n), s) == 0
    a1, a2 = (torch.full((N + 64, L), float("nan"), device="cuda") for _ in range(2))
    part = torch.zeros(2 * nb, dtype=torch.float64, device="cuda")
    assert lib.pdg_node_enc_fwd(N, x.data_ptr(), w0.data_ptr(), b0.data_ptr(), W2.data_ptr(), b2.data_ptr(),
                                a1.data_ptr(), a2.data_ptr(), part.data_ptr(), nb, s) == 0
    assert torch.isnan(a1[N:]).all() and torch.isnan(a2[N:]).all()
    a1, a2 = a1[:N], a2[:N]
    assert torch.equal(a1, a1r)
    z = a1.double() @ W2.double().T + b2.double()
    ref = torch.relu(z)
    assert rel(a2, ref) < 1e-6 and rel(a2, ref) <= 1.05 * rel(a2r, ref) + 1e-9, (rel(a2, ref), rel(a2r, ref))
    if N >= 1000:
        scale = a1.double().abs() @ W2.double().abs().T + b2.double().abs()
        pos = (a2 > 0) & (z > 0)
        bias = float(((a2.double() - z) / scale.clamp_min(1e-30))[pos].mean())
        assert abs(bias) < 3e-10, bias
    p = part.view(nb, 2).sum(0).cpu()
    a2d = a2.double().cpu()
    assert rel(p, torch.stack([a2d.sum(), a2d.square().sum()])) < 1e-7


@pytest.mark.parametrize("N,nb,res", [(7, 37, True), (1031, 37, False), (40328, 256, True)])
def test_gemm_sum2_coop_vs_fp64(env, N, nb, res):
    """pdg_gemm_sum2_coop (bf16x6, register-stationary, cooperative layout) against an fp64
    restatement of W0T in0 + W1T in1 + res, and its LayerNorm column partials / pairs against the
    pdg_ln_colsum formulas on the fp64 output."""
    import struct
    lib, sh, _ = env
    s = sh()
    i0, i1 = rnd(N, L), rnd(N, L)
    W0T, _ = lin(L, L)
    W1T, _ = lin(L, L)
    rr = rnd(N, L) if res else None
    a2 = torch.relu(rnd(N, L))
    g = rnd(L) * 0.3 + 1.0
    r64 = a2.double()
    mean, sd = float(r64.mean()), float(r64.std(unbiased=False))
    den = float(torch.tensor(sd, dtype=torch.float32) + 1e-5)
    st = torch.frombuffer(bytearray(struct.pack("ffffddd", mean, den, 1.0 / den, sd, mean, sd, N * L)),
                          dtype=torch.uint8).cuda()
    ref = i0.double() @ W0T.double().T + i1.double() @ W1T.double().T
    if res:
        ref = ref + rr.double()
    for cols in (False, True):
        out = torch.full((N, L), float("nan"), device="cuda")
        part = torch.full((nb * 256,), float("nan"), dtype=torch.float64, device="cuda")
        pairs = torch.full((nb * 2,), float("nan"), dtype=torch.float64, device="cuda")
        lib.pdg_gemm_sum2_coop(N, i0.data_ptr(), i1.data_ptr(), W0T.data_ptr(), W1T.data_ptr(),
                               rr.data_ptr() if res else None, out.data_ptr(), a2.data_ptr() if cols else None,
                               st.data_ptr() if cols else None, part.data_ptr() if cols else None,
                               g.data_ptr() if cols else None, pairs.data_ptr() if cols else None, 0, nb, s)
        assert rel(out, ref) < TOL
        if cols:
            got = part.view(nb, 256).sum(0).cpu()
            gyv = out.double().cpu()   # the sums of the kernel's own output (the output is checked above)
            xhat = ((a2.double() - mean) / den).cpu()
            want = torch.cat([gyv.sum(0), (gyv * xhat).sum(0)])
            assert rel(got, want) < 1e-6
            sp = pairs.view(nb, 2).sum(0).cpu()
            gd = g.double().cpu()
            assert rel(sp, torch.stack([(gd * got[:L]).sum(), (gd * got[L:]).sum()])) < 1e-9


@pytest.mark.parametrize("N,nb", [(7, 37), (1031, 37), (40328, 256)])
def test_node_bwd_coop_vs_node_bwd(env, N, nb):
    """pdg_node_bwd_coop (bf16x6 W^T products, cooperative layout) against pdg_node_bwd (fp32 MFMA):
    gz2 bitwise (the same elementwise LayerNorm backward), gz1 / gaggr / gx_part to fp32 rounding
    against an fp64 restatement, with the backward scalars from producer pairs."""
    import struct
    lib, sh, _ = env
    s = sh()
    gy = rnd(N, L)
    a1 = torch.relu(rnd(N, L))
    a2 = torch.relu(rnd(N, L))
    g = rnd(L) * 0.3 + 1.0
    W2T, _ = lin(L, L)
    WaT, _ = lin(L, L)
    WbT, _ = lin(L, L)
    r64 = a2.double()
    mean, sd = float(r64.mean()), float(r64.std(unbiased=False))
    den = float(torch.tensor(sd, dtype=torch.float32) + 1e-5)
    st = torch.frombuffer(bytearray(struct.pack("ffffddd", mean, den, 1.0 / den, sd, mean, sd, N * L)),
                          dtype=torch.uint8).cuda()
    S1, S2 = 37.25, -12.5
    pairs = torch.tensor([[S1 / 2, S2 / 4], [S1 / 4, S2 / 2], [S1 / 4, S2 / 4]], dtype=torch.float64).cuda()
    o0 = [torch.empty(N, L, device="cuda") for _ in range(4)]
    o1 = [torch.full((N, L), float("nan"), device="cuda") for _ in range(4)]
    assert lib.pdg_node_bwd(N, gy.data_ptr(), a2.data_ptr(), a1.data_ptr(), st.data_ptr(), None, g.data_ptr(),
                            W2T.data_ptr(), WaT.data_ptr(), WbT.data_ptr(), *[o.data_ptr() for o in o0],
                            pairs.data_ptr(), 3, s) == 0
    lib.pdg_node_bwd_coop(N, gy.data_ptr(), a2.data_ptr(), a1.data_ptr(), st.data_ptr(), None, g.data_ptr(),
                          W2T.data_ptr(), WaT.data_ptr(), WbT.data_ptr(), *[o.data_ptr() for o in o1],
                          pairs.data_ptr(), 3, nb, s)
    assert torch.equal(o0[0], o1[0])                       # gz2
    z2 = o0[0].double()
    z1 = torch.where(a1 > 0, z2 @ W2T.double().T, torch.zeros_like(z2))
    assert rel(o1[1], z1) < TOL and rel(o0[1], z1) < TOL
    z1c = o1[1].double()                                    # the next products from the kernel's own gz1
    assert rel(o1[2], z1c @ WaT.double().T) < TOL
    assert rel(o1[3], z1c @ WbT.double().T + gy.double()) < TOL


@pytest.mark.parametrize("N,nb", [(1, 1), (33, 2), (5000, 7), (70000, 256)])
def test_mlp2_bwd_coop_vs_mlp2_bwd(env, N, nb):
    """pdg_mlp2_bwd_coop (the node encoder's backward, bf16x6 W2^T product) against pdg_mlp2_bwd:
    gz2 bitwise (the same elementwise LayerNorm backward), gz1 to fp32 rounding against fp64."""
    import struct
    lib, sh, _ = env
    s = sh()
    gy = rnd(N, L)
    a1 = torch.relu(rnd(N, L))
    a2 = torch.relu(rnd(N, L))
    g = rnd(L) * 0.3 + 1.0
    W2T, _ = lin(L, L)
    r64 = a2.double()
    mean, sd = float(r64.mean()), float(r64.std(unbiased=False))
    den = float(torch.tensor(sd, dtype=torch.float32) + 1e-5)
    st = torch.frombuffer(bytearray(struct.pack("ffffddd", mean, den, 1.0 / den, sd, mean, sd, N * L)),
                          dtype=torch.uint8).cuda()
    pairs = torch.tensor([[3.5, -1.25], [1.0, 0.5]], dtype=torch.float64).cuda()
    o0 = [torch.empty(N, L, device="cuda") for _ in range(2)]
    o1 = [torch.full((N, L), float("nan"), device="cuda") for _ in range(2)]
    assert lib.pdg_mlp2_bwd(N, gy.data_ptr(), None, a2.data_ptr(), a1.data_ptr(), st.data_ptr(), None, g.data_ptr(),
                            W2T.data_ptr(), o0[0].data_ptr(), o0[1].data_ptr(), pairs.data_ptr(), 2, s) == 0
    assert lib.pdg_mlp2_bwd_coop(N, gy.data_ptr(), a2.data_ptr(), a1.data_ptr(), st.data_ptr(), None, g.data_ptr(),
                                 W2T.data_ptr(), o1[0].data_ptr(), o1[1].data_ptr(), pairs.data_ptr(), 2, None, None,
                                 nb, s) == 0
    assert torch.equal(o0[0], o1[0])                       # gz2
    z1 = torch.where(a1 > 0, o0[0].double() @ W2T.double().T, torch.zeros(N, L, dtype=torch.float64, device="cuda"))
    assert rel(o1[1], z1) < TOL and rel(o0[1], z1) < TOL
    # + the encoder's first-layer gradient (wide = gz1, narrow = the 6-wide input), gz1 not stored: the same
    # gz2, and the finalized dW0 (128 x 6) / db0 against fp64 sums over the kernel's own gz1
    xn = rnd(N, 6)
    npart = torch.full((nb * (6 * L + L + 6),), float("nan"), dtype=torch.float64, device="cuda")
    gz2b = torch.full((N, L), float("nan"), device="cuda")
    assert lib.pdg_mlp2_bwd_coop(N, gy.data_ptr(), a2.data_ptr(), a1.data_ptr(), st.data_ptr(), None, g.data_ptr(),
                                 W2T.data_ptr(), gz2b.data_ptr(), None, pairs.data_ptr(), 2, xn.data_ptr(),
                                 npart.data_ptr(), nb, s) == 0
    assert torch.equal(o0[0], gz2b)
    gW, gb = torch.full((L, 6), 0.5, device="cuda"), torch.full((L,), -0.25, device="cuda")   # += semantics
    assert lib.pdg_wgrad_narrow_finalize(npart.data_ptr(), nb, 6, 0, gW.data_ptr(), gb.data_ptr(), None, s) == 0
    z1k = o1[1].double()
    assert rel(gW.double() - 0.5, z1k.T @ xn.double()) < 1e-6
    assert rel(gb.double() + 0.25, z1k.sum(0)) < 1e-6


@pytest.mark.parametrize("N,nb", [(1, 1), (7, 37), (1031, 37), (40328, 256)])
def test_decoder_bwd_coop_vs_decoder_bwd(env, N, nb):
    """pdg_decoder_bwd_coop against pdg_decoder_bwd: gz1d bitwise (the same 3-wide FMA chain), gx to
    fp32 rounding against fp64; its LayerNorm column partials / pairs against the pdg_ln_colsum
    formulas on the kernel's own gx."""
    import struct
    lib, sh, _ = env
    s = sh()
    gy = rnd(N, 3)
    a1 = torch.relu(rnd(N, L))
    Wd2 = rnd(3, L)
    W1T, _ = lin(L, L)
    a2 = torch.relu(rnd(N, L))
    g = rnd(L) * 0.3 + 1.0
    r64 = a2.double()
    mean, sd = float(r64.mean()), float(r64.std(unbiased=False))
    den = float(torch.tensor(sd, dtype=torch.float32) + 1e-5)
    st = torch.frombuffer(bytearray(struct.pack("ffffddd", mean, den, 1.0 / den, sd, mean, sd, N * L)),
                          dtype=torch.uint8).cuda()
    z0, x0 = torch.empty(N, L, device="cuda"), torch.empty(N, L, device="cuda")
    assert lib.pdg_decoder_bwd(N, gy.data_ptr(), a1.data_ptr(), Wd2.data_ptr(), W1T.data_ptr(), z0.data_ptr(),
                               x0.data_ptr(), s) == 0
    ref = z0.double() @ W1T.double().T
    npart = torch.full((nb * (3 * L + L + 3),), float("nan"), dtype=torch.float64, device="cuda")
    for cols in (False, True):
        z1, x1 = (torch.full((N, L), float("nan"), device="cuda") for _ in range(2))
        part = torch.full((nb * 256,), float("nan"), dtype=torch.float64, device="cuda")
        pairs = torch.full((nb * 2,), float("nan"), dtype=torch.float64, device="cuda")
        assert lib.pdg_decoder_bwd_coop(N, gy.data_ptr(), a1.data_ptr(), Wd2.data_ptr(), W1T.data_ptr(),
                                        z1.data_ptr(), x1.data_ptr(), a2.data_ptr() if cols else None,
                                        st.data_ptr() if cols else None, part.data_ptr() if cols else None,
                                        g.data_ptr() if cols else None, pairs.data_ptr() if cols else None, 0,
                                        npart.data_ptr() if cols else None, nb, s) == 0
        assert torch.equal(z0, z1)
        assert rel(x1, ref) < TOL and rel(x0, ref) < TOL
        if cols:   # node_decoder.2's weight / bias gradient (wide = a1d, narrow = gy, stored transposed 3 x 128)
            gW, gb = torch.full((3, L), 0.5, device="cuda"), torch.full((3,), -0.25, device="cuda")
            assert lib.pdg_wgrad_narrow_finalize(npart.data_ptr(), nb, 3, 1, gW.data_ptr(), None, gb.data_ptr(),
                                                 s) == 0
            assert rel(gW.double() - 0.5, gy.double().T @ a1.double()) < 1e-6
            assert rel(gb.double() + 0.25, gy.double().sum(0)) < 1e-6
        if cols:
            got = part.view(nb, 256).sum(0).cpu()
            gyv = x1.double().cpu()
            xhat = ((a2.double() - mean) / den).cpu()
            want = torch.cat([gyv.sum(0), (gyv * xhat).sum(0)])
            assert rel(got, want) < 1e-6
            sp = pairs.view(nb, 2).sum(0).cpu()
            gd = g.double().cpu()
            assert rel(sp, torch.stack([(gd * got[:L]).sum(), (gd * got[L:]).sum()])) < 1e-9


def test_wgrad_segments_batch_matches_single(env):
    """pdg_wgrad_segments_batch (three weights' segment passes in one launch) == one
    pdg_wgrad_segments per weight, slab for slab (the same kernel body per job)."""
    lib, sh, _ = env
    s = sh()
    SL = L * L + L
    ns = 37
    jobs = [[(rnd(1000, L), rnd(1000, L), 1000), (rnd(77, L), rnd(77, L), 77)], [(rnd(4099, L), rnd(4099, L), 4099)],
            [(rnd(31, L), rnd(31, L), 31), (rnd(500, L), rnd(500, L), 500), (rnd(64, L), rnd(64, L), 64)]]
    single = []
    for sl in jobs:
        out = torch.full((ns, SL), float("nan"), device="cuda")
        n = len(sl)
        lib.pdg_wgrad_segments(n, (ctypes.c_void_p * n)(*[g.data_ptr() for g, _, _ in sl]),
                               (ctypes.c_void_p * n)(*[x.data_ptr() for _, x, _ in sl]),
                               (ctypes.c_int * n)(*[r for _, _, r in sl]), out.data_ptr(), ns, s)
        single.append(out)
    batch = [torch.full((ns, SL), float("nan"), device="cuda") for _ in jobs]
    flat = [t for sl in jobs for t in sl]
    n = len(flat)
    lib.pdg_wgrad_segments_batch(len(jobs), (ctypes.c_int * 3)(*[len(sl) for sl in jobs]),
                                 (ctypes.c_void_p * n)(*[g.data_ptr() for g, _, _ in flat]),
                                 (ctypes.c_void_p * n)(*[x.data_ptr() for _, x, _ in flat]),
                                 (ctypes.c_int * n)(*[r for _, _, r in flat]),
                                 (ctypes.c_void_p * 3)(*[b.data_ptr() for b in batch]), ns, s)
    for a, b in zip(single, batch):
        torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)


def test_fence_free_timing_events_agree_with_torch_events(env):
    """pdg/hiptimer.py's events (hipEventDisableSystemFence, used by the bench's per-kernel timing)
    time a long stream of launches like torch.cuda.Event does, and nest in order."""
    from pdg import hiptimer
    x = torch.randn(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    a, b = hiptimer.Event(), hiptimer.Event()
    ta, tb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ta.record()
    a.record()
    for _ in range(20):
        x = x @ x.T * 1e-3
    b.record()
    tb.record()
    torch.cuda.synchronize()
    ours, ref = a.elapsed_time(b), ta.elapsed_time(tb)
    assert ours > 0 and ref > 0
    assert ours <= ref * 1.02 + 0.05, (ours, ref)
    assert abs(ours - ref) / ref < 0.1, (ours, ref)


def test_bwd_epilogue_matches_separate_launches(env):
    """pdg_bwd_epilogue (every end-of-backward reduction in one launch) against pdg_wgrad_reduce_batch +
    pdg_ln_param_grads + pdg_wgrad_narrow_finalize x2 + pdg_enc_narrow_reduce on the same partials: the
    slab, LayerNorm and narrow gradients bitwise (the same per-block order), the edge encoder's first
    layer to fp64 rounding (its rows are added in another order); gradients accumulate (+=)."""
    lib, sh, _ = env
    s = sh()
    VP, IA = ctypes.c_void_p, ctypes.c_int
    f64 = dict(dtype=torch.float64, device="cuda")
    nj, ns = 3, 37
    slabs = [torch.randn(ns, L * L + L, device="cuda") for _ in range(nj)]
    ld, col0 = [L, 3 * L, 3 * L], [0, 2 * L, 0]
    acc = [torch.randn(51 * 256, **f64) for _ in range(4)]
    rows = [51, 40, 51, 13]
    npart = [torch.randn(29 * (3 * L + L + 3), **f64), torch.randn(17 * (6 * L + L + 6), **f64)]
    nk = [(29, 3, 1), (17, 6, 0)]
    enc = torch.randn(ns, 2 * L, **f64)

    def grads():
        return {"W": [torch.full((L, w), 0.25, device="cuda") for w in ld], "b": [torch.full((L,), -0.5, device="cuda") if j != 2 else None for j in range(nj)],
                "lg": [torch.full((L,), 1.0, device="cuda") for _ in range(4)], "lb": [torch.full((L,), 2.0, device="cuda") for _ in range(4)],
                "nW": [torch.full((3, L), 0.5, device="cuda"), torch.full((L, 6), 0.5, device="cuda")],
                "nbw": [None, torch.full((L,), 0.1, device="cuda")], "nbn": [torch.full((3,), 0.2, device="cuda"), None],
                "w0": torch.full((L,), 0.3, device="cuda"), "b0": torch.full((L,), 0.4, device="cuda")}

    a, b = grads(), grads()
    p = lambda t: None if t is None else t.data_ptr()
    assert lib.pdg_wgrad_reduce_batch(nj, (VP * nj)(*[p(x) for x in slabs]), (IA * nj)(*[ns] * nj),
                                      (VP * nj)(*[p(x) for x in a["W"]]), (IA * nj)(*ld), (IA * nj)(*col0),
                                      (VP * nj)(*[p(x) for x in a["b"]]), s) == 0
    assert lib.pdg_ln_param_grads(4, (VP * 4)(*[p(x) for x in acc]), (IA * 4)(*rows), (VP * 4)(*[p(x) for x in a["lg"]]),
                                  (VP * 4)(*[p(x) for x in a["lb"]]), s) == 0
    for q in range(2):
        assert lib.pdg_wgrad_narrow_finalize(p(npart[q]), nk[q][0], nk[q][1], nk[q][2], p(a["nW"][q]), p(a["nbw"][q]),
                                             p(a["nbn"][q]), s) == 0
    assert lib.pdg_enc_narrow_reduce(p(enc), ns, p(a["w0"]), p(a["b0"]), s) == 0
    assert lib.pdg_bwd_epilogue(nj, (VP * nj)(*[p(x) for x in slabs]), (IA * nj)(*[ns] * nj),
                                (VP * nj)(*[p(x) for x in b["W"]]), (IA * nj)(*ld), (IA * nj)(*col0),
                                (VP * nj)(*[p(x) for x in b["b"]]), 4, (VP * 4)(*[p(x) for x in acc]), (IA * 4)(*rows),
                                (VP * 4)(*[p(x) for x in b["lg"]]), (VP * 4)(*[p(x) for x in b["lb"]]), 2,
                                (VP * 2)(*[p(x) for x in npart]), (IA * 2)(*[t[0] for t in nk]),
                                (IA * 2)(*[t[1] for t in nk]), (IA * 2)(*[t[2] for t in nk]),
                                (VP * 2)(*[p(x) for x in b["nW"]]), (VP * 2)(*[p(x) for x in b["nbw"]]),
                                (VP * 2)(*[p(x) for x in b["nbn"]]), p(enc), ns, p(b["w0"]), p(b["b0"]), s) == 0
    torch.cuda.synchronize()
    for k in ("W", "b", "lg", "lb", "nW", "nbw", "nbn"):
        for x, y in zip(a[k], b[k]):
            assert (x is None and y is None) or torch.equal(x, y), k
    for k in ("w0", "b0"):
        assert rel(b[k], a[k]) < 1e-6, k
    assert not torch.equal(a["W"][0], torch.full((L, L), 0.25, device="cuda"))   # something was added


@pytest.mark.parametrize("sizes,accumulate", [((5041,) * 8, 0), ((17, 2, 3000, 250), 1), ((9000, 20000, 8192), 0),
                                              ((1025, 1, 4096, 4097, 2), 0), ((1025, 1, 4096, 4097, 2), 1)])
def test_nmse_fwd_bwd_equals_fwd_then_bwd(env, sizes, accumulate):
    """pdg_nmse_fwd_bwd (per-graph NMSE and its gradient in one launch) is bitwise pdg_nmse_fwd + pdg_nmse_bwd:
    losses, denominators and the gradient (written or accumulated); ragged graphs, and graphs past the
    8,192 nodes whose values the kernel keeps in registers (the rest re-read).  Against fp64 (loss_ref.nmse_ref,
    autograd of the oracle's loss): losses and denominators within 1e-5 relative, the gradient rows within relative
    L2 TOL (accumulated: after removing the base).  A 1-node graph (den = 0, between graphs on both sides of the
    1024-thread stride and of the 4,096 nodes of one cached iteration) gets the IEEE quotients torch gives in fp32 on
    the same input, inf or NaN, and leaves the other graphs' values alone."""
    from loss_ref import nmse_ref
    from oracle import epd_oracle as O
    lib, sh, _ = env
    s = sh()
    B, N = len(sizes), sum(sizes)
    ptr = torch.tensor([0] + list(torch.tensor(sizes).cumsum(0)), dtype=torch.int32, device="cuda")
    gt, pred = rnd(N, 3), rnd(N, 3)
    scale = torch.tensor([0.125], device="cuda")
    base = rnd(N, 3)
    l0, d0, g0 = torch.empty(B, device="cuda"), torch.empty(B, 3, device="cuda"), base.clone()
    assert lib.pdg_nmse_fwd(B, ptr.data_ptr(), gt.data_ptr(), pred.data_ptr(), l0.data_ptr(), d0.data_ptr(), s) == 0
    assert lib.pdg_nmse_bwd(B, ptr.data_ptr(), N, gt.data_ptr(), pred.data_ptr(), d0.data_ptr(), scale.data_ptr(),
                            accumulate, g0.data_ptr(), s) == 0
    l1, d1, g1 = torch.empty(B, device="cuda"), torch.empty(B, 3, device="cuda"), base.clone()
    assert lib.pdg_nmse_fwd_bwd(B, ptr.data_ptr(), gt.data_ptr(), pred.data_ptr(), l1.data_ptr(), d1.data_ptr(),
                                scale.data_ptr(), accumulate, g1.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert torch.equal(l0, l1) and torch.equal(d0, d1) and torch.equal(g0, g1)
    gt64, pr64 = gt.double().cpu(), pred.double().cpu()
    for b in range(B):
        lo, hi = int(ptr[b]), int(ptr[b + 1])
        t, p = gt64[lo:hi], pr64[lo:hi]
        if hi - lo == 1:
            continue    # den = 0: below
        ref = (((t - p) ** 2).sum(0) / ((t - t.mean(0)) ** 2).sum(0)).mean()
        assert abs(float(l1[b]) - float(ref)) <= 1e-5 * abs(float(ref)), (b, float(l1[b]), float(ref))
    loss64, den64, grad64 = nmse_ref(ptr, gt, pred, float(scale))
    ok = torch.tensor([n > 1 for n in sizes])
    rows_ok = torch.repeat_interleave(ok, torch.tensor(sizes))
    dc, gc, bc = d1.cpu(), g1.cpu(), base.cpu()
    assert bool(((l1.cpu().double() - loss64).abs() <= 1e-5 * loss64)[ok].all())
    assert bool(((dc.double() - den64).abs() <= 1e-5 * den64)[ok].all()), (dc, den64)
    # written: g1 is the gradient.  Accumulated: g1 = fl(base + v) carries the final addition's rounding, at most
    # 2^-24 |g1| per element whatever v is, so ||(g1 - base) - grad|| <= ||v - grad|| + 2^-24 ||g1||: the kernel's
    # own v is held to TOL, the addition to the format's bound (base is O(1), v as small as 1e-5 of it)
    gv = gc.double() - (bc.double() if accumulate else 0)
    slack = 2.0 ** -24 * float(gc[rows_ok].double().norm()) if accumulate else 0.0
    err = float((gv[rows_ok] - grad64[rows_ok]).norm())
    assert err <= TOL * float(grad64[rows_ok].norm()) + slack, (err, float(grad64[rows_ok].norm()), slack)
    for b in (i for i, n in enumerate(sizes) if n == 1):
        lo = int(ptr[b])
        t, q = gt[lo:lo + 1].cpu(), pred[lo:lo + 1].cpu()
        want = O.normalized_mse_loss_single(t, q)                       # fp32 on the CPU: x / 0
        den32 = (t - t.mean(0)).square().sum(0)
        wg = scale.cpu() * ((-2.0 * (t - q)) / den32) / 3.0
        wg = bc[lo:lo + 1] + wg if accumulate else wg
        assert float(den32.abs().max()) == 0 and float(dc[b].abs().max()) == 0
        assert not bool(torch.isfinite(want)) and not bool(torch.isfinite(wg).any())
        for got, exp in ((l1[b].cpu().reshape(1), want.reshape(1)), (gc[lo], wg[0])):
            assert torch.equal(got.isnan(), exp.isnan()) and torch.equal(got[~got.isnan()], exp[~exp.isnan()]), (got, exp)


@pytest.mark.parametrize("E,nb", [(77, 37), (4099, 37), (30011, 256), (100000, 256)])
@pytest.mark.parametrize("res,ln,acc", [(1, 1, 0), (0, 1, 1), (1, 0, 0), (0, 0, 0)])
def test_edge_gout_wc_vs_fp64(env, E, nb, res, ln, acc):
    """pdg_edge_gout_wc (16-row rounds, two rounds of loads in flight, one barrier per round, a round's
    output rows stored after the next round's barrier) against fp64: ge_out = [ge_next +] gC Wc, the dWc
    slabs (sum over blocks = gC^T e, b1 sums = column sums of gC; written by the first call, accumulated by
    the second), the LayerNorm column partials (sum of ge_out and of ge_out * xhat per column, written or
    accumulated) and the pairs; no row written past E (the NaN fill survives); grids of 37 blocks (ragged
    tails, empty blocks) and 256.  (Round 6 replaced the 32-row two-barrier kernel; the two were bitwise
    equal on these cases, EXPERIMENTS §5.)"""
    lib, sh, _ = env
    s = sh()
    g = torch.Generator().manual_seed(E + 5 * res + 3 * ln)
    gC, e, gen = (torch.randn(E, L, generator=g).cuda() for _ in range(3))
    a2 = torch.relu(torch.randn(E, L, generator=g)).cuda()
    WcT = (torch.randn(L, L, generator=g) * 0.08).cuda()
    lg = (torch.randn(L, generator=g) * 0.3 + 1.0).cuda()
    part = torch.empty(4096, dtype=torch.float64, device="cuda")
    n = ctypes.c_int(0)
    tmp = torch.empty(E, L, device="cuda")
    W2, b2 = lin(L, L)
    lib.pdg_mlp2_fwd(E, a2.data_ptr(), W2.data_ptr(), b2.data_ptr(), tmp.data_ptr(), part.data_ptr(),
                     ctypes.byref(n), s)
    st = finalize(lib, s, part, n.value, E * L)
    slabs = torch.randn(nb, L * L + L, generator=g).cuda()
    lnp0 = torch.randn(nb + 1, 256, generator=g).double().cuda()
    lnp = lnp0.clone()
    pairs = torch.zeros(2 * nb, dtype=torch.float64, device="cuda")
    go = torch.full((E + 3, L), float("nan"), device="cuda")
    for init in (1, 0):   # the first call writes the slabs, the second accumulates
        assert lib.pdg_edge_gout_wc(E, gC.data_ptr(), e.data_ptr(), gen.data_ptr() if res else None, WcT.data_ptr(),
                                    go.data_ptr(), slabs.data_ptr(), nb, a2.data_ptr() if ln else None,
                                    st.data_ptr() if ln else None, lnp.data_ptr() if ln else None,
                                    lg.data_ptr() if ln else None, pairs.data_ptr() if ln else None, acc, init, s) == 0
    torch.cuda.synchronize()
    G, X = gC.double(), e.double()
    ref = G @ WcT.double().T + (gen.double() if res else 0)
    assert rel(go[:E].double(), ref) < 1e-6, rel(go[:E].double(), ref)
    assert bool(go[E:].isnan().all())
    tot = slabs.double().sum(0)
    assert rel(tot[:L * L].view(L, L), 2 * G.T @ X) < 1e-6
    assert rel(tot[L * L:], 2 * G.sum(0)) < 1e-6
    if ln:
        sd = stat_from(st)
        mean, den = sd["mean"], sd["den"]
        xhat = (a2.double() - mean) / den
        cols = torch.cat([ref.sum(0), (ref * xhat).sum(0)])
        got = lnp[:nb].sum(0) - (lnp0[:nb].sum(0) if acc else 0)
        assert rel(got, (2 if acc else 1) * cols) < 1e-5, rel(got, (2 if acc else 1) * cols)
        # the pairs are the last call's (of its own block rows, accumulated or not): against the written rows
        # to rounding, and against fp64 at 5e-5 (the g-weighted column sums cancel: the products' accumulated
        # rounding over 1e5 rows is ~1e-5 of the pair at E = 100,000)
        pr = pairs.view(nb, 2).sum(0)
        w = lg.double()
        if not acc:
            rows = lnp[:nb]
            assert rel(pr, torch.stack([(rows[:, :L] * w).sum(), (rows[:, L:] * w).sum()])) < 1e-12
        assert rel(pr, torch.stack([(cols[:L] * w).sum(), (cols[L:] * w).sum()])) < 5e-5




@pytest.mark.parametrize("E,nb", [(77, 37), (4099, 37), (30011, 256), (100000, 256), (1, 1), (33, 2), (33, 256)])
@pytest.mark.parametrize("eu,res", [(1, 1), (0, 1), (1, 0), (0, 0)])
def test_edge_fwd_infer_matches_coop(env, E, nb, eu, res):
    """pdg_edge_fwd_infer (inference: 16-row rounds, one barrier per round, the C product of round k beside the
    W2 products of round k - 1) against pdg_edge_fwd_coop without layer-1 outputs on the same inputs: e_t, a2m /
    a2e bitwise (the same MFMA chain per element), no row written past E (the NaN fill survives), the
    LayerNorm partials' totals to 1e-12 (the same fp64 terms in another order); grids of 37 blocks (contiguous
    ranges, ragged tails, empty blocks) and 256 (XCD-interleaved units)."""
    lib, sh, _ = env
    s = sh()
    N = max(E // 6, 40)
    g = torch.Generator().manual_seed(E + 7 * eu + 3 * res)
    src = torch.randint(0, N, (E,), generator=g).int().cuda()
    dst = torch.sort(torch.randint(0, N, (E,), generator=g)).values.int().cuda()
    a2p, eres = torch.relu(rnd(E, L)), rnd(E, L)
    Pn, Qn = rnd(N, L), rnd(N, L)
    W1, b1 = lin(L, 3 * L)
    W2, b2 = lin(L, L)
    lg, lbv = rnd(L) * 0.3 + 1.0, rnd(L) * 0.1
    part = torch.empty(4096, dtype=torch.float64, device="cuda")
    n = ctypes.c_int(0)
    tmp = torch.empty(E, L, device="cuda")
    lib.pdg_mlp2_fwd(E, a2p.data_ptr(), W2.data_ptr(), b2.data_ptr(), tmp.data_ptr(), part.data_ptr(),
                     ctypes.byref(n), s)
    st = finalize(lib, s, part, n.value, E * L)
    pq = PQ.of(lib, Pn, Qn)
    outs = {}
    for infer in (False, True):
        o = {k: torch.full((E + 3, L), float("nan"), device="cuda") for k in ("e", "a2m", "a2e")}
        pm = torch.zeros(2 * nb, dtype=torch.float64, device="cuda")
        pe = torch.zeros(2 * nb, dtype=torch.float64, device="cuda")
        head = (E, a2p.data_ptr(), st.data_ptr(), lg.data_ptr(), lbv.data_ptr(), eres.data_ptr() if res else None,
                o["e"].data_ptr(), src.data_ptr(), dst.data_ptr(), pq.p, pq.q, W1.data_ptr(), b1.data_ptr(),
                W2.data_ptr(), b2.data_ptr())
        tail = (pm.data_ptr(), pe.data_ptr() if eu else None, eu, nb, s)
        a2e = o["a2e"].data_ptr() if eu else None
        if infer:
            assert lib.pdg_edge_fwd_infer(*head, o["a2m"].data_ptr(), a2e, *tail) == 0
        else:
            assert lib.pdg_edge_fwd_coop(*head, None, o["a2m"].data_ptr(), None, a2e, *tail) == 0
        torch.cuda.synchronize()
        outs[infer] = (o, pm.view(nb, 2).sum(0), pe.view(nb, 2).sum(0))
    (o0, pm0, pe0), (o1, pm1, pe1) = outs[False], outs[True]
    for k in ["e", "a2m"] + (["a2e"] if eu else []):
        assert torch.equal(o0[k][:E], o1[k][:E]), (k, rel(o1[k][:E], o0[k][:E]))
        assert bool(o1[k][E:].isnan().all()), k
    assert float((pm1 - pm0).abs().max()) <= 1e-12 * float(pm0.abs().max())
    if eu:
        assert float((pe1 - pe0).abs().max()) <= 1e-12 * float(pe0.abs().max())
