"""The deferred weight-gradient kernels (csrc/pdg_wgrad.hip) at the op level, at the edges of their split-K row
schedule.  The reference is stated inline: dW = sum_seg G_seg^T X_seg and db = sum_seg colsum(G_seg) over the
concatenated rows, in int64 for the exact inputs and in float64 for the random ones.

  pdg_wgrad_segments        every (case, layout) row of TABLE, reduced with pdg_wgrad_reduce: exact inputs equal to
                            int64, random inputs within the project's bounds, every slab written, no over-read;
  pdg_wgrad_pairs           the same for both shared_x values: each product against its own operands (A0 != A1, so a
                            product that leaks into the other fails the exact comparison), the bias rows per the
                            header (column sums of A0 / A1 with shared X, of A0 in both slab sets otherwise), both
                            slab sets NaN-prefilled, zero-row segments with NULL pointers (the launcher allows NULL
                            where rows == 0; pdg_wgrad_segments promises no such thing and gets valid pointers);
  pdg_wgrad_segments_batch  1, 2 and 3 jobs of different totals and layouts in one launch, a job with fewer rows than
                            slabs beside a large one, each job against int64 / fp64 directly, NaN-prefilled slabs;
  pdg_wgrad_reduce, pdg_wgrad_reduce_batch, pdg_bwd_epilogue
                            16 jobs of integer slabs at the slab counts around the reducers' chunk (32), group (8)
                            and stride (64) edges, into gradients that hold non-integer values, ld = 384, col0 in
                            {0, 128, 256}: the three reducers give the same bits, those of old + the int64 sum; every
                            other column and the NaN guards around the gradients are untouched; grad_b = NULL writes
                            nothing; the batch reducer and the epilogue leave their slabs as they were; the epilogue
                            with and without its LayerNorm / narrow / encoder parts (those checked exactly too);
  pdg_wgrad_narrow          K in {1, 3, 6}, both transposes, rows around the 8-rows-per-block and the one-block-per-CU
                            edges of its grid: exact inputs equal to int64, random inputs within 1e-6, added onto
                            non-zero gradients, each nullable bias output given as NULL;
  pdg_wgrad_accum           (not called by the engine, still exported) exact inputs with one and two operand pairs,
                            accumulated twice into the same slabs.

Nothing is asserted about which rows land in which slab: that partition is what a faster kernel may change.  Only
the reduced gradient is checked, and that every slab is written.

Inputs.  Exact: integers drawn from {-4 .. 4} stored as fp32.  Each is exact in the first term of the three-term
bf16 split (the other two terms are zero), every product is at most 16 in magnitude and every partial sum at most
16 x 8209 = 131 344 < 2^24, so every fp32 sum is exact in any order, within a slab and across slabs: dW and the bias
sums must EQUAL the int64 reference.  A dropped, doubled or misattributed row, or a row read through the wrong
segment's pointer, changes an integer and fails whatever the summation order.  Random: randn operands against fp64
with the bounds the existing tests use (TOL_W, TOL_B, TOL_ENTRY below).  The operands of one (total, kind) are
drawn once and cut into segments per layout, so each reference is computed once.

Poison.  The segments of one operand lie in one buffer with three NaN rows after each segment's last row (a zero-row
segment is three NaN rows, or NULL for pdg_wgrad_pairs): a used over-read, or a row fetched through a neighbouring
segment's pointer at the wrong offset, turns the result NaN.  Every slab buffer is NaN-filled (the engine hands
these kernels torch.empty) and has one more NaN slab past nslabs: afterwards slabs 0 .. nslabs - 1 hold no NaN --
a block without rows wrote its zeros and its zero bias row, and they are zero in sum because the reduced gradient is
exact -- and the extra slab is still all NaN.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

L = 128
SL = L * L + L     # floats per slab: the 128 x 128 weight part and the 128 bias sums
MAX_SEGS = 32      # PDG_MAX_SEGS (include/pdivgnn.h)
NAN = float("nan")
# the existing bounds of tests/test_gpu_ops.py, restated (no new tolerance):
TOL_W = 2e-6       # relative L2 of dW against fp64 (test_wgrad_segments_reduce)
TOL_B = 1e-6       # relative L2 of the bias sums against fp64 (test_wgrad_segments_reduce, test_wgrad_pairs_vs_fp64)
TOL_ENTRY = 1e-6   # per entry |err| / sum_k |G||X| (test_wgrad_segments_dynamic_range): covers cancelling entries
TOL_NARROW = 1e-6  # relative L2 of the narrow gradient and its two bias sums (test_wgrad_narrow)

# (total_rows, nslabs): the smallest shapes that reach each path of the row schedule.  Block b owns the virtual rows
# [per b, per (b + 1)), per = ceil(total / nslabs) rounded up to 32; each 32-row step runs as two 16-row rounds with
# two rounds of row loads in flight; rows past the block's end are clamped on load and zeroed when staged.
#   (1, 1) (15, 1)  fewer rows than a round            (16, 1)  exactly one round: the second round is all padding
#   (17, 1)         one row past a round: skipping the last partial round drops row 16
#   (31, 1)         one row short of a unit            (32, 1)  exactly one unit
#   (33, 2)         per = 32: block 0 a full unit, block 1 holds one row
#   (77, 37)        per = 32: blocks 0 - 2 hold 32, 32, 13 rows, 34 blocks are empty and must write zeros
#   (456, 256)      the published mesh size on the engine's grid (one slab per CU): 14 full blocks, one of 8 rows,
#                   241 empty
#   (4099, 37)      per = 128: four units per block, block 32 holds 3 rows (ragged last round), blocks 33 - 36 empty
#   (8209, 256)     per = 64: two units per block, block 128 holds 17 rows, blocks 129 - 255 empty
# Segment layouts (cut = the first row of the next segment):
#   one      a single segment
#   head1    [1, total - 1]                            tail1    [total - 1, 1]
#   cuts     cuts inside a round, at a round edge and one past it: rows 7, 16, 17, 32, 33 where they fit (the cuts
#            at 16 and 17 make a one-row segment: a row of segment s read through segment s + 1's pointer fails)
#   zeros    zero-row segments first, last and two in a row in the middle (ties in the start[] table that the
#            binary search for a block's first segment runs over)
#   max32    32 segments (PDG_MAX_SEGS), cuts from a seeded generator such that 16-row rounds hold no boundary, one
#            and several (cuts32 below); totals of at least 456 rows
TABLE = [
    (1, 1, "one"), (1, 1, "zeros"),
    (15, 1, "one"), (15, 1, "cuts"),
    (16, 1, "one"), (16, 1, "tail1"),
    (17, 1, "one"), (17, 1, "cuts"),
    (31, 1, "one"), (31, 1, "head1"),
    (32, 1, "one"), (32, 1, "cuts"),
    (33, 2, "one"), (33, 2, "head1"), (33, 2, "tail1"), (33, 2, "cuts"), (33, 2, "zeros"),
    (77, 37, "one"), (77, 37, "tail1"), (77, 37, "cuts"), (77, 37, "zeros"),
    (456, 256, "one"), (456, 256, "head1"), (456, 256, "cuts"), (456, 256, "zeros"), (456, 256, "max32"),
    (4099, 37, "tail1"), (4099, 37, "cuts"), (4099, 37, "zeros"), (4099, 37, "max32"),
    (8209, 256, "one"), (8209, 256, "head1"), (8209, 256, "zeros"), (8209, 256, "max32"),
]
# several jobs in one launch (one nslabs for all of them): (nslabs, [(total, layout), ...])
BATCHES = [
    (37, [(77, "zeros")]),
    (37, [(33, "cuts"), (4099, "max32")]),                     # fewer rows than slabs beside a large job
    (256, [(8209, "head1"), (1, "one"), (456, "max32")]),      # a one-row job between two larger ones
    (37, [(17, "one"), (4099, "tail1"), (77, "cuts")]),
]
ACCUM_CASES = [(1, 1), (33, 2), (77, 37), (4099, 37)]
# slab counts around the reducers' edges: pdg_wgrad_reduce sums chunks of WR_CHUNK = 32 slabs, four at a time;
# pdg_wgrad_reduce_batch and pdg_bwd_epilogue give slab b to group b % 8 and walk in strides of 64; 2048 is
# pdg_max_blocks().  Four more fill the 16 jobs of one launch.
REDUCE_COUNTS = [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 256, 2048, 2, 100, 129, 511]
NARROW_K = [(1, 0), (1, 1), (3, 0), (3, 1), (6, 0), (6, 1)]


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


def p(t):
    return None if t is None else t.data_ptr()


def VP(ts):
    ts = list(ts)
    return (ctypes.c_void_p * len(ts))(*[p(t) for t in ts])


def IA(xs):
    xs = list(xs)
    return (ctypes.c_int * len(xs))(*xs)


def cuts32(total):
    """31 cuts for 32 segments: of the total // 16 full 16-row rounds, drawn in a seeded random order, three get three
    cuts, one gets two, twenty get one and the rest (at least four) none; a cut's offset in its round is random, so
    some fall on a round's first row."""
    gen = torch.Generator().manual_seed(3200 + total)
    rounds = torch.randperm(total // 16, generator=gen).tolist()
    per_round = [3, 3, 3, 2] + [1] * 20
    assert len(rounds) >= len(per_round) + 2
    cuts = []
    for r, k in zip(rounds, per_round):
        offs = (torch.randperm(16, generator=gen) if r else 1 + torch.randperm(15, generator=gen))[:k].tolist()
        cuts += [16 * r + o for o in offs]
    cuts.sort()
    held = [sum(1 for c in cuts if c // 16 == r) for r in range((total + 15) // 16)]
    assert len(cuts) == 31 and len(set(cuts)) == 31 and 0 < cuts[0] and cuts[-1] < total
    assert held.count(0) >= 2 and held.count(1) >= 2 and sum(1 for h in held if h >= 2) >= 2
    return cuts


def layout(name, total):
    """The segments' row counts."""
    if name == "one":
        return [total]
    if name == "head1":
        return [1, total - 1]
    if name == "tail1":
        return [total - 1, 1]
    if name == "zeros":
        return [0, total // 2, 0, 0, total - total // 2, 0]
    cuts = cuts32(total) if name == "max32" else [c for c in (7, 16, 17, 32, 33) if c < total]
    edges = [0] + cuts + [total]
    rows = [b - a for a, b in zip(edges, edges[1:])]
    assert sum(rows) == total and len(rows) <= MAX_SEGS and (name != "max32" or len(rows) == MAX_SEGS)
    return rows


class Data:
    """Three operands A0, A1, A2 of `total` rows (host, fp32) and the references formed from them, each made once:
    prod(i, j) = A_i^T A_j and colsum(i), in int64 for the exact kind and in float64 for the random kind, and
    scale(i, j) = |A_i|^T |A_j|, the yardstick of the per-entry bound."""

    def __init__(self, total, kind):
        gen = torch.Generator().manual_seed(7000 + total + (0 if kind == "exact" else 500000))
        if kind == "exact":
            self.A = [torch.randint(-4, 5, (total, L), generator=gen).float() for _ in range(3)]
        else:
            self.A = [torch.randn(total, L, generator=gen, dtype=torch.float64).float() for _ in range(3)]
        self.total, self.kind = total, kind
        self.ref_t = torch.int64 if kind == "exact" else torch.float64
        self._memo = {}

    def prod(self, i, j):
        if (i, j) not in self._memo:
            self._memo[i, j] = self.A[i].to(self.ref_t).T @ self.A[j].to(self.ref_t)
        return self._memo[i, j]

    def colsum(self, i):
        return self.A[i].to(self.ref_t).sum(0)

    def scale(self, i, j):
        if ("s", i, j) not in self._memo:
            self._memo["s", i, j] = self.A[i].double().abs().T @ self.A[j].double().abs()
        return self._memo["s", i, j]

    def segments(self, i, rows, null=()):
        """Operand i cut into device segments of rows[k] rows, three NaN rows after each (one buffer, one copy);
        the zero-row segments listed in `null` are None."""
        assert sum(rows) == self.total and all(rows[k] == 0 for k in null)
        buf = torch.full((self.total + 3 * len(rows), L), NAN)
        at, r0, spans = 0, 0, []
        for k, r in enumerate(rows):
            buf[at:at + r] = self.A[i][r0:r0 + r]
            spans.append((at, r))
            at, r0 = at + r + 3, r0 + r
        dev = buf.cuda()
        return [None if k in null else dev[a:a + r + 3] for k, (a, r) in enumerate(spans)]


_data = {}


def data(total, kind):
    if (total, kind) not in _data:
        _data[total, kind] = Data(total, kind)
    return _data[total, kind]


def nan_slabs(ns, sets=1):
    """`sets` slab sets of ns slabs, NaN-filled, each followed by one more NaN slab that must stay NaN."""
    return torch.full((sets, ns + 1, SL), NAN, device="cuda")


def slabs_written(slabs, ns, what):
    assert not bool(slabs[:ns].isnan().any()), f"{what}: a block left (part of) its slab unwritten"
    assert bool(slabs[ns].isnan().all()), f"{what}: the slab past nslabs was written"


def reduced(env, slabs, ns):
    """pdg_wgrad_reduce of a written slab set into zero gradients."""
    lib, sh, _ = env
    gW, gb = torch.zeros(L, L, device="cuda"), torch.zeros(L, device="cuda")
    assert lib.pdg_wgrad_reduce(p(slabs), ns, p(gW), L, 0, p(gb), sh()) == 0
    torch.cuda.synchronize()
    return gW, gb


def check(what, d, gW, gb, iW, ib):
    """The reduced gradient of the product A_iW[0]^T A_iW[1] and of the column sums of A_ib against d's references:
    equal for the exact kind; the three bounds for the random kind (the figures are printed before they are
    asserted)."""
    refW, refb = d.prod(*iW), d.colsum(ib)
    if d.kind == "exact":
        assert torch.equal(gW.double().cpu(), refW.double()), \
            f"{what}: dW differs from int64 in {int((gW.double().cpu() != refW.double()).sum())} entries"
        assert torch.equal(gb.double().cpu(), refb.double()), f"{what}: the bias sums differ from int64"
        return
    eW, eb = rel(gW, refW), rel(gb, refb)
    entry = float(((gW.double().cpu() - refW).abs() / d.scale(*iW)).max())
    print(f"WGRAD {what}: dW rel {eW:.3e} (bound {TOL_W:g}) bias rel {eb:.3e} (bound {TOL_B:g}) "
          f"worst entry |err| / sum|G||X| {entry:.3e} (bound {TOL_ENTRY:g})")
    assert eW < TOL_W and eb < TOL_B and entry < TOL_ENTRY, (what, eW, eb, entry)


# ------------------------------------------------------------------------------------------ the segment passes

@pytest.mark.parametrize("total,ns,lay", TABLE)
def test_wgrad_segments_vs_int64_and_fp64(env, total, ns, lay):
    """pdg_wgrad_segments (G = A0, X = A2) + pdg_wgrad_reduce: equal to int64 on the exact inputs, within the bounds
    on the random ones, all nslabs slabs written and the one past them untouched."""
    lib, sh, _ = env
    rows = layout(lay, total)
    for kind in ("exact", "random"):
        d = data(total, kind)
        G, X = d.segments(0, rows), d.segments(2, rows)
        slabs = nan_slabs(ns)[0]
        assert lib.pdg_wgrad_segments(len(rows), VP(G), VP(X), IA(rows), p(slabs), ns, sh()) == 0
        torch.cuda.synchronize()
        what = f"segments total={total} ns={ns} {lay} {kind}"
        slabs_written(slabs, ns, what)
        check(what, d, *reduced(env, slabs, ns), (0, 2), 0)


@pytest.mark.parametrize("shared_x", [1, 0])
@pytest.mark.parametrize("total,ns,lay", TABLE)
def test_wgrad_pairs_vs_int64_and_fp64(env, total, ns, lay, shared_x):
    """pdg_wgrad_pairs: shared_x: A0^T A2 and A1^T A2 with the column sums of A0 / A1; otherwise A0^T A1 and A0^T A2
    with the column sums of A0 in both slab sets.  Each product against its own operands (A0 != A1 != A2).  Every
    second zero-row segment carries NULL in all three arrays."""
    lib, sh, _ = env
    rows = layout(lay, total)
    null = [k for k, r in enumerate(rows) if r == 0][::2]
    prods = [((0, 2), 0), ((1, 2), 1)] if shared_x else [((0, 1), 0), ((0, 2), 0)]
    for kind in ("exact", "random"):
        d = data(total, kind)
        A = [d.segments(i, rows, null) for i in range(3)]
        slabs = nan_slabs(ns, 2)
        assert lib.pdg_wgrad_pairs(len(rows), VP(A[0]), VP(A[1]), VP(A[2]), IA(rows), shared_x, p(slabs[0]),
                                   p(slabs[1]), ns, sh()) == 0
        torch.cuda.synchronize()
        for k, (iW, ib) in enumerate(prods):
            what = f"pairs shared_x={shared_x} product {k} total={total} ns={ns} {lay} {kind}"
            slabs_written(slabs[k], ns, what)
            check(what, d, *reduced(env, slabs[k], ns), iW, ib)


@pytest.mark.parametrize("ns,jobs", BATCHES)
def test_wgrad_segments_batch_vs_int64_and_fp64(env, ns, jobs):
    """pdg_wgrad_segments_batch: every job of one launch against int64 / fp64 directly (not against the single-job
    kernel: a slab that neither writes compares equal there), NaN-prefilled slab sets."""
    lib, sh, _ = env
    for kind in ("exact", "random"):
        ds = [data(total, kind) for total, _ in jobs]
        rows = [layout(lay, total) for total, lay in jobs]
        G = [d.segments(0, r) for d, r in zip(ds, rows)]
        X = [d.segments(2, r) for d, r in zip(ds, rows)]
        slabs = nan_slabs(ns, len(jobs))
        assert lib.pdg_wgrad_segments_batch(len(jobs), IA(len(r) for r in rows), VP(t for g in G for t in g),
                                            VP(t for x in X for t in x), IA(n for r in rows for n in r),
                                            VP(slabs[j] for j in range(len(jobs))), ns, sh()) == 0
        torch.cuda.synchronize()
        for j, (total, lay) in enumerate(jobs):
            what = f"batch job {j + 1}/{len(jobs)} total={total} ns={ns} {lay} {kind}"
            slabs_written(slabs[j], ns, what)
            check(what, ds[j], *reduced(env, slabs[j], ns), (0, 2), 0)


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("total,ns", ACCUM_CASES)
def test_wgrad_accum_exact(env, total, ns, two):
    """pdg_wgrad_accum, one (A0, A2) and two (+ A1, A0) operand pairs, called twice on zeroed slabs (it accumulates):
    twice the int64 reference, the slab past nslabs untouched.  The operands end in three NaN rows."""
    lib, sh, _ = env
    d = data(total, "exact")
    (G,), (X,), (G2,), (X2,) = (d.segments(i, [total]) for i in (0, 2, 1, 0))
    slabs = nan_slabs(ns)[0]
    slabs[:ns] = 0
    for _ in range(2):
        assert lib.pdg_wgrad_accum(total, p(G), p(X), p(G2) if two else None, p(X2) if two else None, p(slabs), ns,
                                   sh()) == 0
    torch.cuda.synchronize()
    slabs_written(slabs, ns, f"accum total={total} ns={ns}")
    gW, gb = reduced(env, slabs, ns)
    refW = 2 * (d.prod(0, 2) + (d.prod(1, 0) if two else 0))
    refb = 2 * (d.colsum(0) + (d.colsum(1) if two else 0))
    assert torch.equal(gW.double().cpu(), refW.double()) and torch.equal(gb.double().cpu(), refb.double())


# ------------------------------------------------------------------------------------------ the slab reductions

class Grads:
    """One reduction job's gradients: grad_W (128 x 384, non-integer values) and, if `bias`, grad_b, each between
    two NaN guards in one buffer.  `col0` is the job's first column."""
    LD = 3 * L

    def __init__(self, j, col0, bias):
        gen = torch.Generator().manual_seed(9100 + j)
        self.col0, self.bias = col0, bias
        self.buf = torch.full((L + L * self.LD + L + L + L,), NAN)
        self.buf[L:L + L * self.LD] = torch.randn(L * self.LD, generator=gen)
        if bias:
            self.buf[2 * L + L * self.LD:3 * L + L * self.LD] = torch.randn(L, generator=gen)
        self.old = self.buf.clone()

    def dev(self):
        """A fresh device copy: (buffer, grad_W, grad_b or None)."""
        t = self.old.cuda()
        return t, t[L:L + L * self.LD].view(L, self.LD), t[2 * L + L * self.LD:3 * L + L * self.LD] if self.bias else None

    def expected(self, total):
        """old + the int64 slab sum `total` (SL entries) in the job's columns and its bias, one fp32 rounding per
        entry (the sums are integers below 2^24, exact in fp32, so a += of them rounds once); all else as before."""
        e = self.old.clone()
        W = e[L:L + L * self.LD].view(L, self.LD)
        c = slice(self.col0, self.col0 + L)
        W[:, c] = (W[:, c].double() + total[:L * L].view(L, L).double()).float()
        if self.bias:
            b = e[2 * L + L * self.LD:3 * L + L * self.LD]
            b[:] = (b.double() + total[L * L:].double()).float()
        return e


def same_bits(a, b):
    """Bitwise equality, NaN guards included."""
    return torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


@pytest.fixture(scope="module")
def reduce_jobs(env):
    """16 slab sets of REDUCE_COUNTS slabs (integers from {-4 .. 4}: every sum is at most 8192 and exact), their
    int64 sums, and the gradients they are added into: col0 cycles through 0, 128, 256; every third job has no
    grad_b."""
    gen = torch.Generator(device="cuda").manual_seed(9000)
    slabs = [torch.randint(-4, 5, (n, SL), device="cuda", generator=gen).float() for n in REDUCE_COUNTS]
    totals = [s.long().sum(0).cpu() for s in slabs]
    grads = [Grads(j, (0, L, 2 * L)[j % 3], j % 3 != 1) for j in range(len(REDUCE_COUNTS))]
    return slabs, totals, grads


def check_reduced(what, reduce_jobs, outs):
    _, totals, grads = reduce_jobs
    for j, (g, (buf, _, _)) in enumerate(zip(grads, outs)):
        assert same_bits(buf, g.expected(totals[j])), \
            f"{what}: job {j} ({REDUCE_COUNTS[j]} slabs, col0 {g.col0}, bias {g.bias}) is not old + the int64 sum"


def test_wgrad_reduce_exact(env, reduce_jobs):
    """pdg_wgrad_reduce at every slab count: old + the int64 sum in the target columns and in grad_b, every other
    column, the guards around grad_W and (grad_b = NULL) the buffer where a bias would lie bitwise unchanged."""
    lib, sh, _ = env
    slabs, _, grads = reduce_jobs
    outs = []
    for n, sl, g in zip(REDUCE_COUNTS, slabs, grads):
        buf, gW, gb = g.dev()
        assert lib.pdg_wgrad_reduce(p(sl.clone()), n, p(gW), g.LD, g.col0, p(gb), sh()) == 0   # overwrites its slabs
        outs.append((buf, gW, gb))
    torch.cuda.synchronize()
    check_reduced("pdg_wgrad_reduce", reduce_jobs, outs)


def test_wgrad_reduce_batch_exact(env, reduce_jobs):
    """pdg_wgrad_reduce_batch, its maximum of 16 jobs of different slab counts in one launch: the bits of
    pdg_wgrad_reduce (both equal old + the int64 sum), the slabs (const arguments) unchanged."""
    lib, sh, _ = env
    slabs, _, grads = reduce_jobs
    before = [s.clone() for s in slabs]
    outs = [g.dev() for g in grads]
    k = len(slabs)
    assert lib.pdg_wgrad_reduce_batch(k, VP(slabs), IA(REDUCE_COUNTS), VP(o[1] for o in outs), IA(g.LD for g in grads),
                                      IA(g.col0 for g in grads), VP(o[2] for o in outs), sh()) == 0
    torch.cuda.synchronize()
    check_reduced("pdg_wgrad_reduce_batch", reduce_jobs, outs)
    assert all(torch.equal(a, b) for a, b in zip(slabs, before)), "pdg_wgrad_reduce_batch changed its input slabs"


@pytest.mark.parametrize("others", [True, False])
def test_bwd_epilogue_slab_part_exact(env, reduce_jobs, others):
    """pdg_bwd_epilogue with its maximum of 16 slab reductions, alongside its other parts (4 LayerNorm groups, 2
    narrow finalizes, the edge encoder's sums) and with those absent: the slab part gives the bits of the other two
    reducers and leaves its slabs unchanged.  The other parts get integer-valued doubles and gradients of 0.5, so
    that they are checked exactly too: a block dealt to the wrong part shows in either."""
    lib, sh, _ = env
    slabs, _, grads = reduce_jobs
    before = [s.clone() for s in slabs]
    outs = [g.dev() for g in grads]
    k = len(slabs)
    gen = torch.Generator().manual_seed(9200)

    def ints(*shape):
        return torch.randint(-4, 5, shape, generator=gen).double()

    def half(*shape):
        return torch.full(shape, 0.5, device="cuda")

    ln_rows = [51, 40, 1, 13]
    ln_acc = [ints(r, 256) for r in ln_rows]
    nk = [(29, 3, 1), (17, 6, 0)]   # (parts, K, transpose)
    npart = [ints(n, L * K + L + K) for n, K, _ in nk]
    enc = ints(37, 2 * L)
    ln_g, ln_b = [half(L) for _ in ln_rows], [half(L) for _ in ln_rows]
    nW, nbw, nbn = [half(3, L), half(L, 6)], [None, half(L)], [half(3), None]
    w0, b0 = half(L), half(L)
    dv = [[t.cuda() for t in ts] for ts in (ln_acc, npart)]
    enc_d = enc.cuda()
    n_ln, n_np = (len(ln_rows), len(nk)) if others else (0, 0)
    assert lib.pdg_bwd_epilogue(k, VP(slabs), IA(REDUCE_COUNTS), VP(o[1] for o in outs), IA(g.LD for g in grads),
                                IA(g.col0 for g in grads), VP(o[2] for o in outs),
                                n_ln, VP(dv[0]), IA(ln_rows), VP(ln_g), VP(ln_b),
                                n_np, VP(dv[1]), IA(t[0] for t in nk), IA(t[1] for t in nk), IA(t[2] for t in nk),
                                VP(nW), VP(nbw), VP(nbn), p(enc_d) if others else None, 37 if others else 0,
                                p(w0) if others else None, p(b0) if others else None, sh()) == 0
    torch.cuda.synchronize()
    check_reduced(f"pdg_bwd_epilogue others={others}", reduce_jobs, outs)
    assert all(torch.equal(a, b) for a, b in zip(slabs, before)), "pdg_bwd_epilogue changed its input slabs"

    def added(t):
        return t.double().cpu() - 0.5

    if not others:
        assert all(float(added(t).abs().max()) == 0 for t in ln_g + ln_b + nW + [nbw[1], nbn[0], w0, b0])
        return
    for acc, g, b in zip(ln_acc, ln_g, ln_b):   # columns 0 .. 127 the bias sums, 128 .. 255 the weight sums
        assert torch.equal(added(b), acc.sum(0)[:L]) and torch.equal(added(g), acc.sum(0)[L:])
    for (n, K, tr), part, W, bw, bn in zip(nk, npart, nW, nbw, nbn):   # [T (128 x K) | wide sums | narrow sums]
        tot = part.sum(0)
        T = tot[:L * K].view(L, K)
        assert torch.equal(added(W), T.T if tr else T)
        assert bw is None or torch.equal(added(bw), tot[L * K:L * K + L])
        assert bn is None or torch.equal(added(bn), tot[L * K + L:])
    assert torch.equal(added(w0), enc.sum(0)[:L]) and torch.equal(added(b0), enc.sum(0)[L:])


# ------------------------------------------------------------------------------------------ the narrow gradient

def narrow_rows():
    """Rows around the edges of pdg_wgrad_narrow's grid, min(ceil(rows / 8), CUs) blocks of 8 half-wave rows with a
    grid-stride loop: 1, 7, 8, 9 (below, at and past one block), 8 CUs -+ 1 (the last block short of a row / the
    first grid-stride step), 4099 (many steps, ragged)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus, [1, 7, 8, 9, 8 * cus - 1, 8 * cus + 1, 4099]


@pytest.mark.parametrize("K,transpose", NARROW_K)
def test_wgrad_narrow_vs_int64_and_fp64(env, K, transpose):
    """pdg_wgrad_narrow: T = Wide^T Narrow (128 x K, or its transpose) and the two column sums.  Exact inputs, added
    onto gradients of 0.5 / -0.25 / 0.75: equal to old + int64 (|sum| <= 16 x 4099, so the fp32 sum is exact).
    Random inputs, added onto zeros as in test_wgrad_narrow (onto 0.75 a single small sum would be judged by the
    rounding of the addition): within 1e-6 of fp64.  Each bias output also given as NULL (the other outputs as
    before).  The partials scratch is NaN-filled, one part past the grid stays NaN; the operands end in three NaN
    rows."""
    lib, sh, _ = env
    cus, all_rows = narrow_rows()
    per = L * K + L + K
    for rows in all_rows:
        grid = min((rows + 7) // 8, cus)
        for kind in ("exact", "random"):
            gen = torch.Generator().manual_seed(9300 + rows + K)
            if kind == "exact":
                wide, narrow = (torch.randint(-4, 5, (rows, w), generator=gen).float() for w in (L, K))
            else:
                wide, narrow = (torch.randn(rows, w, generator=gen) for w in (L, K))
            rt = torch.int64 if kind == "exact" else torch.float64
            T = (wide.to(rt).T @ narrow.to(rt)).double()
            refs = (T.T if transpose else T, wide.to(rt).sum(0).double(), narrow.to(rt).sum(0).double())
            wide_d = torch.cat([wide, torch.full((3, L), NAN)]).cuda()
            narrow_d = torch.cat([narrow, torch.full((3, K), NAN)]).cuda()
            old = (0.5, -0.25, 0.75) if kind == "exact" else (0.0, 0.0, 0.0)
            for null in (None, "wide", "narrow"):
                part = torch.full((grid + 1, per), NAN, dtype=torch.float64, device="cuda")
                gW = torch.full((K, L) if transpose else (L, K), old[0], device="cuda")
                gbw = None if null == "wide" else torch.full((L,), old[1], device="cuda")
                gbn = None if null == "narrow" else torch.full((K,), old[2], device="cuda")
                assert lib.pdg_wgrad_narrow(rows, p(wide_d), p(narrow_d), K, transpose, p(part), p(gW), p(gbw), p(gbn),
                                            sh()) == 0
                torch.cuda.synchronize()
                what = f"narrow K={K} transpose={transpose} rows={rows} {kind} null={null}"
                assert not bool(part[:grid].isnan().any()) and bool(part[grid].isnan().all()), what
                got = list(zip((gW, gbw, gbn), old))
                if kind == "exact":
                    for (g, o), r in zip(got, refs):
                        assert g is None or torch.equal(g.double().cpu() - o, r), what
                else:
                    errs = [rel(g, r) for (g, _), r in zip(got, refs) if g is not None]
                    if null is None:
                        print(f"WGRAD {what}: rel " + " ".join(f"{e:.3e}" for e in errs) + f" (bound {TOL_NARROW:g})")
                    assert max(errs) < TOL_NARROW, (what, errs)
