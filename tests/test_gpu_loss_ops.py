"""The kernels that end a training step at the op level, driven through pdg.lib, against the float64
restatements of tests/loss_ref.py (anchored to the oracle by tests/test_loss_ref.py):

  pdg_div_fwd / pdg_div_bwd        one ragged batch (graphs of 1 and 2 nodes, both sides of 64 and of the 1024-thread
                                   block stride, an empty graph in the middle), an operator with empty rows, unsorted
                                   and repeated columns and entries at or beyond 2 n_g, both reductions, g_sigma
                                   written and accumulated, the two composed, and the device planner's arrays;
  pdg_loss_reduce, pdg_nonfinite2  around the 256-thread block and the 1024 x 256 grid, every flag value, both parities;
  pdg_any_nonzero, pdg_zero_unless, pdg_format_inputs, pdg_ln_partials_sum.

The operator comes from the host builder (loss_ref.build_div_csr), not from pdg_div_plan, except where the two are
compared.  Every bound is the reference's own (derived in loss_ref) or the number format's.  With
PDG_LOSS_OP_ERRORS=<file> the measured figures are written there (profiles/loss_op_errors.txt)."""
import math
import os

import pytest
import torch

from loss_ref import (DIV_SIZES, U, abs_rows_left_out, build_div_csr, div_bwd_ref, div_fwd_ref, format_ref, loss_ref,
                      loss_reduce_ref, nonfinite_ref, random_div_case)

pytestmark = pytest.mark.gpu

TOL = 2e-6            # relative L2 vs float64 for a single fp32 op (the file-level constant of test_gpu_ops.py)
GUARD = 64
# 262144 = 1024 blocks x 256 threads (the flag kernels' largest grid): 262145 starts the second grid-stride sweep
NS = [0, 1, 255, 256, 257, 262144, 262145, 1000003]
NAN, INF = float("nan"), float("inf")
_lines = []

HEADER = """Op-level errors of the loss and step-guard kernels against the float64 restatements of tests/loss_ref.py
(tests/test_gpu_loss_ops.py, one MI355X; reproduce with `PDG_LOSS_OP_ERRORS=<file> pytest tests/test_gpu_loss_ops.py`).

"worst err/bound": max over elements of |x - ref| / bound with the reference's elementwise bound (loss_ref:
(nnz + 1) 2^-24 sum |a s| for div, (nnz + 3) 2^-24 sum |a g| for g_sigma, plus 2^-24 |result| when accumulated, plus
the forward's bound carried through |A^T| when composed); must be <= 1.  "rel" figures are relative L2 (bound 2e-6)
or the largest relative error over the graphs (bound 1e-5).  The flag kernels are exact: their lines count the cases.
"""


def note(line):
    print(line)
    _lines.append(line)


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pdg.lib import lib, stream_handle
    torch.manual_seed(0)
    yield lib, stream_handle
    path = os.environ.get("PDG_LOSS_OP_ERRORS")
    if path:
        with open(path, "w") as f:
            f.write(HEADER + "\n" + "\n".join(_lines) + "\n")


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def p(t):
    return None if t is None else t.data_ptr()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def guarded(n, fill=NAN, dtype=torch.float32):
    """n elements and GUARD more, all `fill`; the kernels get the base pointer."""
    return torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")


def guard_ok(buf, n):
    return bool(buf[n:].isnan().all()) and buf.numel() == n + GUARD


def worst_ratio(err, bound):
    """max err / bound; where the bound is 0 (nothing summed) the error must be 0 too."""
    pos = bound > 0
    assert not bool((err[~pos] != 0).any())
    return float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0


# ================================================================================================ divergence
class DivCase:
    """The ragged batch of loss_ref.random_div_case on the device, its fp64 references and the kernels' runs (each
    made once and kept)."""

    def __init__(self, env):
        self.c = c = random_div_case()
        self.N, self.B = c.N, c.B
        self.host = build_div_csr(c.ptr, c.rows, c.cols, c.vals, keep_beyond=True)
        self.op = self.to_dev(self.host)
        self.ptr = c.ptr.int().cuda()
        self.types, self.sigma = c.types.cuda(), c.sigma.cuda()
        self.scale = torch.tensor([0.125 * 10 / c.B], device="cuda")
        self.base = torch.randn(c.N * 3, generator=torch.Generator().manual_seed(77)).cuda()
        self._fwd, self._bwd, self._ref = {}, {}, {}

    @staticmethod
    def to_dev(op):
        return {k: v.cuda() for k, v in vars(op).items()}

    def fwd(self, env, ra, op=None):
        key = ra if op is None else None
        if key in self._fwd:
            return self._fwd[key]
        lib, sh = env
        op = op or self.op
        div, loss = guarded(self.N * 2), guarded(self.B)
        assert lib.pdg_div_fwd(self.B, p(self.ptr), p(op["a_rowptr"]), p(op["a_col"]), p(op["a_val"]), p(self.types),
                               p(self.sigma), ra, p(div), p(loss), sh()) == 0
        torch.cuda.synchronize()
        if key is not None:
            self._fwd[key] = (div, loss)
        return div, loss

    def bwd(self, env, ra, acc, op=None):
        key = (ra, acc) if op is None else None
        if key in self._bwd:
            return self._bwd[key]
        lib, sh = env
        op = op or self.op
        div = self.fwd(env, ra)[0][:self.N * 2].clone()      # the GPU's own div, without the guard
        gs = guarded(self.N * 3)
        if acc:
            gs[:self.N * 3] = self.base
        assert lib.pdg_div_bwd(self.B, p(self.ptr), self.N, p(op["at_rowptr"]), p(op["at_row"]), p(op["at_comp"]),
                               p(op["at_val"]), p(div), p(self.scale), ra, acc, p(gs), sh()) == 0
        torch.cuda.synchronize()
        if key is not None:
            self._bwd[key] = gs
        return gs

    def ref_fwd(self, ra):
        if ("f", ra) not in self._ref:
            h = self.host
            self._ref[("f", ra)] = div_fwd_ref(self.c.ptr, h.a_rowptr, h.a_col, h.a_val, self.c.types, self.c.sigma, ra)
        return self._ref[("f", ra)]


_div = []


@pytest.fixture(scope="module")
def dc(env):
    if not _div:
        _div.append(DivCase(env))
    return _div[0]


@pytest.mark.parametrize("ra", [0, 1])
def test_div_fwd_vs_fp64(env, dc, ra):
    """pdg_div_fwd: every div entry within the fma chain's bound of fp64, the per-graph loss within 1e-5 relative,
    NaN for the empty graph, rows of type +-1 exactly 0 (type 2 is not masked), nothing written past row N."""
    div_buf, loss_buf = dc.fwd(env, ra)
    div, loss = div_buf[:dc.N * 2].reshape(dc.N, 2).cpu(), loss_buf[:dc.B].cpu()
    div64, loss64, bound = dc.ref_fwd(ra)
    ratio = worst_ratio((div.double() - div64).abs(), bound)
    empty = torch.tensor([s == 0 for s in DIV_SIZES])
    lrel = ((loss.double() - loss64).abs() / loss64.abs().clamp(min=1e-300))[~empty]
    note(f"div_fwd reduce_abs={ra} N={dc.N} B={dc.B}: div worst err/bound={ratio:.3f} rel={rel(div, div64):.2e} "
         f"loss worst rel={float(lrel.max()):.2e}")
    assert not bool(div.isnan().any()) and ratio <= 1
    assert bool(loss[empty].isnan().all()) and bool(loss64[empty].isnan().all()) and int(empty.sum()) == 1
    assert bool(((loss.double() - loss64).abs() <= 1e-5 * loss64.abs())[~empty].all()), (loss, loss64)
    masked = (dc.c.types == 1) | (dc.c.types == -1)
    assert float(div[masked].abs().max()) == 0 and float(div[dc.c.types == 2].abs().max()) > 0
    assert guard_ok(div_buf, dc.N * 2) and guard_ok(loss_buf, dc.B)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("ra", [0, 1])
def test_div_bwd_vs_fp64(env, dc, ra, acc):
    """pdg_div_bwd on the GPU's own div (the same fp32 values on both sides: nothing is near a sign threshold):
    every g_sigma entry within the reference's bound (+ 2^-24 |result| for the final addition when accumulating)
    and relative L2 below TOL; accumulate = 0 overwrites a NaN fill everywhere, nodes with an empty A^T row get
    exact zeros; nothing written past row N."""
    gs_buf = dc.bwd(env, ra, acc)
    gs = gs_buf[:dc.N * 3].reshape(dc.N, 3).cpu()
    div = dc.fwd(env, ra)[0][:dc.N * 2].reshape(dc.N, 2).cpu()
    h = dc.host
    g64, bound = div_bwd_ref(dc.c.ptr, h.at_rowptr, h.at_row, h.at_comp, h.at_val, div, float(dc.scale), ra)
    assert not bool(gs.isnan().any())
    if acc:
        g64 = g64 + dc.base.cpu().double().reshape(dc.N, 3)
        bound = bound + U * gs.double().abs()
    ratio, r = worst_ratio((gs.double() - g64).abs(), bound), rel(gs, g64)
    note(f"div_bwd reduce_abs={ra} accumulate={acc}: g_sigma worst err/bound={ratio:.3f} rel={r:.2e}")
    assert ratio <= 1 and r < TOL
    unfed = (h.at_rowptr[1:] == h.at_rowptr[:-1])
    assert int(unfed.sum()) > 0
    if acc:
        assert torch.equal(gs[unfed], dc.base.cpu().reshape(dc.N, 3)[unfed])
    else:
        assert float(gs[unfed].abs().max()) == 0
    assert guard_ok(gs_buf, dc.N * 3)


@pytest.mark.parametrize("ra", [0, 1])
def test_div_fwd_then_bwd_vs_fp64_autograd(env, dc, ra):
    """The two composed, against the fp64 autograd gradient of scale * sum_g loss_g (loss_ref).  Elementwise bound:
    the backward's own bound plus, for "square", the forward's bound carried through |A^T| (g_div is linear in div:
    |delta g_sigma| <= sum_j |a_j| f |delta div_j|; second-order terms dropped); relative L2 below TOL.  For "abs" the
    rows fed by a div entry with 0 < |div64| < 1e-4 rms(div64) are left out (the fp32 sign may differ there) and
    must be at most 0.1 % of the rows; on the rows kept the signs agree, so the forward's error does not carry."""
    h = dc.host
    gs = dc.bwd(env, ra, 0)[:dc.N * 3].reshape(dc.N, 3).cpu()
    sc = float(dc.scale)
    div64, g64 = loss_ref(dc.c.ptr, h.a_rowptr, h.a_col, h.a_val, dc.c.types, dc.c.sigma, sc, ra)
    _, bound = div_bwd_ref(dc.c.ptr, h.at_rowptr, h.at_row, h.at_comp, h.at_val, div64, sc, ra)
    out = abs_rows_left_out(h, div64) if ra else torch.zeros(dc.N, dtype=torch.bool)
    if not ra:
        carried, _ = div_bwd_ref(dc.c.ptr, h.at_rowptr, h.at_row, h.at_comp, h.at_val.abs(), dc.ref_fwd(ra)[2], sc, 0)
        bound = bound + carried
    keep = ~out
    ratio = worst_ratio((gs.double() - g64).abs()[keep], bound[keep])
    r = rel(gs[keep], g64[keep])
    share = float(out.double().mean())
    note(f"div_fwd -> div_bwd reduce_abs={ra}: g_sigma vs fp64 autograd worst err/bound={ratio:.3f} rel={r:.2e} "
         f"rows left out={int(out.sum())} of {dc.N} ({share:.2e})")
    assert share <= 1e-3
    assert ratio <= 1 and r < TOL


def test_div_kernels_take_the_planners_arrays(env, dc):
    """pdg_div_plan's arrays (GraphPlan._build_div_device) and the host builder's are interchangeable: the A^T arrays
    are equal, the A arrays equal the builder's without the entries at or beyond 2 n_g, and both kernels' outputs
    are bitwise those of the runs fed by the host arrays (which keep such entries in A: the forward ignores them)."""
    from pdg.plan import GraphPlan
    c = dc.c
    plan = GraphPlan.__new__(GraphPlan)
    plan.n_nodes, plan.ptr, plan.n_graphs = c.N, dc.ptr, c.B
    plan._build_div_device(c.rows.cuda(), c.cols.cuda(), c.vals.cuda())
    assert int(plan.status.item()) == 0
    names = ("a_rowptr", "a_col", "a_val", "at_rowptr", "at_row", "at_comp", "at_val")
    dev = {k: getattr(plan, k) for k in names}
    slim = build_div_csr(c.ptr, c.rows, c.cols, c.vals)
    for k in names:
        assert torch.equal(dev[k].cpu(), getattr(slim, k)), k
    assert dev["a_col"].numel() < dc.host.a_col.numel()
    for ra in (0, 1):
        a, b = dc.fwd(env, ra), dc.fwd(env, ra, op=dev)
        assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))
        for acc in (0, 1):
            assert torch.equal(bits(dc.bwd(env, ra, acc)), bits(dc.bwd(env, ra, acc, op=dev)))
    note("div_fwd / div_bwd fed by pdg_div_plan's arrays: bitwise the host builder's (2 x fwd, 4 x bwd)")


# ================================================================================================ loss scalars
@pytest.mark.parametrize("B", [1, 255, 256, 257, 1000])
def test_loss_reduce(env, B):
    """pdg_loss_reduce: out[1] / out[2] within 3 x 2^-24 relative of fp64 (non-negative inputs; the kernel rounds the
    fp64 sum to fp32 and the product with the scale once more), out[3] bitwise the fp32 sum of the GPU's own out[1]
    and out[2], out[0] the flag or 1; loss_div NULL gives out[2] = 0 exactly."""
    lib, sh = env
    g = torch.Generator().manual_seed(B)
    ln, ld = torch.rand(B, generator=g) * 3, torch.rand(B, generator=g) * 50
    sn, sd = float(torch.tensor(1.0 / B).float()), float(torch.tensor(10.0 / B).float())
    lnd, ldd = ln.cuda(), ld.cuda()
    worst = 0.0
    for with_div in (True, False):
        for zf in (None, 1.0, 0.0):
            flag = None if zf is None else torch.tensor([zf], device="cuda")
            out = guarded(4)
            assert lib.pdg_loss_reduce(B, p(lnd), p(ldd) if with_div else None, sn, sd, p(flag), p(out), sh()) == 0
            torch.cuda.synchronize()
            o = out[:4].cpu()
            ref = loss_reduce_ref(ln, ld if with_div else None, sn, sd, zf)
            assert float(o[0]) == ref[0]
            for k in (1, 2) if with_div else (1,):
                e = abs(float(o[k]) - ref[k]) / ref[k]
                worst = max(worst, e)
                assert e <= 3 * U, (k, float(o[k]), ref[k])
            if not with_div:
                assert float(o[2]) == 0
            assert torch.equal(bits(o[3]), bits(o[1] + o[2]))
            assert guard_ok(out, 4)
    note(f"loss_reduce B={B}: worst rel of out[1] / out[2] = {worst / U:.2f} x 2^-24 (bound 3), 6 cases")


def poison_cases(n):
    """(value, index) pairs: every non-finite kind at the first, middle and last element and at index 262144."""
    at = sorted({i for i in (0, n // 2, n - 1, 262144) if 0 <= i < n})
    return [None] + [(v, i) for v in (NAN, INF, -INF) for i in at]


def benign(n, seed):
    """n finite floats with 3e38 and a denormal among them, and one element more (a NaN) that no kernel may read."""
    x = torch.rand(n + 1, generator=torch.Generator().manual_seed(seed)) - 0.5
    if n:
        x[n // 3], x[(2 * n) // 3] = 3e38, 1e-45
        assert float(x[(2 * n) // 3]) > 0
    x[n] = NAN
    return x.cuda()


@pytest.mark.parametrize("n", NS)
def test_nonfinite2(env, n):
    """pdg_nonfinite2: flags[parity] = any non-finite x[i < n] or a zero_flag of +-0, flags[parity ^ 1] cleared, for
    both parities from flags prefilled [parity] = 0, [parity ^ 1] = 7; 3e38, a denormal and a NaN at x[n] do not flag."""
    lib, sh = env
    x = benign(n, n)
    flags = torch.zeros(2 + GUARD, dtype=torch.int32, device="cuda")
    ncases = 0
    for zf in (None, 1.0, 0.0, -0.0):
        flag = None if zf is None else torch.tensor([zf], device="cuda")
        for parity in (0, 1):
            for poison in poison_cases(n):
                if poison:
                    keep = float(x[poison[1]])
                    x[poison[1]] = poison[0]
                fill = torch.full((2 + GUARD,), 99, dtype=torch.int32)
                fill[parity], fill[parity ^ 1] = 0, 7
                flags.copy_(fill)
                assert lib.pdg_nonfinite2(p(x), n, p(flag), p(flags), parity, sh()) == 0
                got = flags.cpu()
                want = nonfinite_ref(x[:n], zf)
                assert want == int(poison is not None or (zf is not None and zf == 0))
                assert int(got[parity]) == want and int(got[parity ^ 1]) == 0, (zf, parity, poison, got[:2])
                assert bool((got[2:] == 99).all())
                if poison:
                    x[poison[1]] = keep
                ncases += 1
    note(f"nonfinite2 n={n}: {ncases} cases exact")


def test_nonfinite2_back_to_back(env):
    """The trainer's use: four calls on one stream with alternating parity and [bad, ok, bad, ok] inputs, the flag
    read after each, no host memset in between (each call clears the slot the next one ORs into)."""
    lib, sh = env
    n = 262145
    ok = benign(n, 1)
    bad = ok.clone()
    bad[n - 1] = INF
    flags = torch.tensor([0, 7], dtype=torch.int32, device="cuda")
    seen = []
    for k, x in enumerate((bad, ok, bad, ok)):
        assert lib.pdg_nonfinite2(p(x), n, None, p(flags), k % 2, sh()) == 0
        seen.append(int(flags.cpu()[k % 2]))
    assert seen == [1, 0, 1, 0], seen
    note("nonfinite2 back to back, parity 0 1 0 1, [bad, ok, bad, ok]: flags " + str(seen))


@pytest.mark.parametrize("n", NS)
def test_any_nonzero(env, n):
    """pdg_any_nonzero = torch.any on the CPU, from a flag prefilled with 0x7c7c7c7c: all zero and all -0.0 give 0
    (a nonzero at x[n] is not read); one nonzero at the first / last element or at index 262144, one NaN, one
    1e-45 denormal give 1."""
    lib, sh = env
    cases = [("zero", 0.0, None), ("-zero", -0.0, None)]
    if n:
        at = sorted({i for i in (0, n - 1, 262144) if i < n})
        cases += [("one", 0.0, (1.0, i)) for i in at] + [("nan", 0.0, (NAN, n // 2)), ("denormal", -0.0, (1e-45, n - 1))]
    for name, fill, spot in cases:
        x = torch.full((n + 1,), fill)
        x[n] = 1.0
        if spot:
            x[spot[1]] = spot[0]
        want = int(bool(torch.any(x[:n])))
        assert want == int(spot is not None)
        flag = torch.full((1 + GUARD,), 0x7c7c7c7c, dtype=torch.int32, device="cuda")
        xd = x.cuda()
        assert lib.pdg_any_nonzero(p(xd), n, p(flag), sh()) == 0
        got = flag.cpu()
        assert int(got[0]) == want, (name, spot, int(got[0]))
        assert bool((got[1:] == 0x7c7c7c7c).all())
    note(f"any_nonzero n={n}: {len(cases)} cases exact")


@pytest.mark.parametrize("n", NS)
def test_zero_unless(env, n):
    """pdg_zero_unless: flag 0 zeroes exactly n elements (the sentinel at element n survives); flag 1 and flag 0x100
    leave the buffer bitwise untouched, NaN payloads included."""
    lib, sh = env
    y0 = torch.randn(n + GUARD, generator=torch.Generator().manual_seed(n + 5))
    raw = y0.view(torch.int32)
    raw[::7] = 0x7fc12345          # NaNs with a payload
    raw[n] = 0x7fc54321            # the sentinel
    for f in (0, 1, 0x100):
        flag = torch.tensor([f], dtype=torch.int32, device="cuda")
        y = y0.cuda()
        assert lib.pdg_zero_unless(p(flag), p(y), n, sh()) == 0
        got = bits(y)
        if f:
            assert torch.equal(got, raw), f
        else:
            assert bool((got[:n] == 0).all()) and torch.equal(got[n:], raw[n:])
    note(f"zero_unless n={n}: flags 0, 1, 0x100 exact")


# ================================================================================================ inputs, LayerNorm sums
@pytest.mark.parametrize("scale_input", [1, 0])
@pytest.mark.parametrize("N,E", [(1, 0), (257, 255), (255, 1031), (5041, 30000)])
def test_format_inputs(env, N, E, scale_input):
    """pdg_format_inputs against format_ref in fp64 (relative L2 below TOL) and bitwise against the fp32 restatement
    (v - m) / s in torch on the CPU (one IEEE subtraction, one correctly rounded division; no fast-math, nothing
    to contract); o[5] = float(type) exactly; E = 0 with NULL edge arrays; nothing written past the outputs."""
    lib, sh = env
    g = torch.Generator().manual_seed(N + E)
    pos, ms = torch.rand(N, 2, generator=g) * 3 - 1, torch.randn(N, 3, generator=g) * 2 + 0.4
    types = torch.randint(-1, 2, (N,), generator=g)
    ea, perm = torch.rand(E, generator=g) * 0.2 + 0.01, torch.randperm(E, generator=g).int()
    st = torch.tensor([0.3, 1.7, -0.2, 2.3, 9.0, 9.0, 0.05, 0.4])
    stats = dict(mean_pos=st[0], std_pos=st[1], mean_mean_stress=st[2], std_mean_stress=st[3],
                 mean_edge_weight=st[6], std_edge_weight=st[7])
    x_in, e_in = guarded(N * 6), guarded(E) if E else None
    d = [t.cuda() for t in (pos, ms, types, ea, perm, st)]
    assert lib.pdg_format_inputs(N, E, p(d[0]), p(d[1]), p(d[2]), p(d[3]) if E else None, p(d[4]) if E else None,
                                 p(d[5]), scale_input, p(x_in), p(e_in), sh()) == 0
    torch.cuda.synchronize()
    x = x_in[:N * 6].reshape(N, 6).cpu()
    e = e_in[:E].cpu() if E else torch.empty(0)
    x64, e64 = format_ref(stats, pos, ms, types, ea, perm.long(), bool(scale_input))
    f32 = lambda v, m, s: (v - torch.full_like(v, float(m))) / torch.full_like(v, float(s)) if scale_input else v
    x32 = torch.cat([f32(ms, st[2], st[3]), f32(pos, st[0], st[1]), types.float().reshape(-1, 1)], 1)
    e32 = f32(ea, st[6], st[7])[perm.long()]
    rx, re = rel(x, x64), rel(e, e64) if E else 0.0
    nx, ne = int((bits(x) != bits(x32)).sum()), int((bits(e) != bits(e32)).sum())
    note(f"format_inputs N={N} E={E} scale_input={scale_input}: x_in rel={rx:.2e} e_in rel={re:.2e}; "
         f"elements not bitwise the fp32 restatement: x_in {nx} e_in {ne}")
    assert rx < TOL and re < TOL
    assert nx == 0 and ne == 0
    assert torch.equal(x[:, 5], types.float())
    assert guard_ok(x_in, N * 6) and (not E or guard_ok(e_in, E))


def test_ln_partials_sum(env):
    """pdg_ln_partials_sum over 1, 255, 256, 257 and pdg_max_blocks() (sum, sumsq) pairs of positive partials spanning
    six decades: both outputs within nparts x 2^-53 x sum |x| of math.fsum."""
    lib, sh = env
    for nparts in (1, 255, 256, 257, lib.pdg_max_blocks()):
        g = torch.Generator().manual_seed(nparts)
        part = 10.0 ** (torch.rand(nparts, 2, generator=g, dtype=torch.float64) * 6 - 3)
        assert float(part.max() / part.min()) > (1e5 if nparts > 100 else 0)
        out, pd = guarded(2, dtype=torch.float64), part.cuda()
        assert lib.pdg_ln_partials_sum(p(pd), nparts, p(out), sh()) == 0
        torch.cuda.synchronize()
        o = out.cpu()
        worst = 0.0
        for k in (0, 1):
            ref = math.fsum(part[:, k].tolist())
            bound = nparts * 2.0 ** -53 * ref
            worst = max(worst, abs(float(o[k]) - ref) / bound)
            assert abs(float(o[k]) - ref) <= bound, (nparts, k, float(o[k]), ref)
        assert guard_ok(out, 2)
        note(f"ln_partials_sum nparts={nparts}: worst err/bound={worst:.3f}")
