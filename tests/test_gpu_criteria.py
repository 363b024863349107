"""The stress-criteria kernels (csrc/pdg_criteria.hip) on the GPU at the op level, against tests/criteria_ref.py
(fp64 numpy, pinned by tests/test_criteria_ref.py).

Bounds.  A table value is an fp64 expression of fp64 sums of non-negative terms formed from the same fp32 inputs
as the yardstick's: 1e-10 relative, the gate tests/test_gpu_metrics.py uses for the same kind of sums, leaves
room for the summation order and the few ulps of pow / exp / log.  argmax is exact.  A field or gradient value is
the fp64 value rounded once to fp32: within 2^-23 |ref| of the yardstick, plus 1e-10 x the largest |ref| of the
graph's gradient for the transcendental aggregates (pnorm, ks), whose node weights carry pow's / exp's error.
NaNs must sit where the yardstick puts them.  With PDG_CRITERIA_OP_ERRORS=<file> the measured worst cases are
written there (profiles/criteria_op_errors.txt)."""
import functools
import itertools
import os

import numpy as np
import pytest
import torch

import criteria_ref as R

pytestmark = pytest.mark.gpu

GUARD = 8
# a single node; sizes under, at and over a wave (64) and a workgroup (1024); an empty graph between two non-empty
# ones; 4,097 nodes, one row past the 4,096 whose criterion values a block keeps in registers
COUNTS = (1, 2, 63, 64, 65, 0, 1023, 1024, 1025, 4097)
WEIGHTS = ("none", "positive", "mixed", "excluded")
EXCLUDED = 2                      # the graph the "excluded" weights leave out entirely
PS = (1.0, 2.0, 8.0, 64.0)
RHOS = (1e-3, 1.0, 1e3)           # times 1 / the field's scale
_worst = {}


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _record():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    yield
    path = os.environ.get("PDG_CRITERIA_OP_ERRORS")
    if path:
        head = ("Op-level errors of pdg_stress_criteria / pdg_stress_criteria_bwd against the float64 restatement "
                "tests/criteria_ref.py\n(tests/test_gpu_criteria.py, one MI355X; reproduce with "
                "`PDG_CRITERIA_OP_ERRORS=<file> pytest tests/test_gpu_criteria.py`).\n\n"
                f"Ragged batch of {COUNTS} nodes,\nweights {WEIGHTS}, p {PS}, rho {RHOS} / scale, and the planted "
                "rows.\ntable: worst relative error (bound 1e-10).  field, g_sigma: worst |x - ref| / bound with "
                "bound = 2^-23 |ref|\n(+ 1e-10 max |ref| of the graph for pnorm and ks); must be <= 1 (0.5 is one "
                "fp32 rounding).\n")
        with open(path, "w") as f:
            f.write(head + "\n" + "\n".join(f"{k}: {v:.3e}" for k, v in sorted(_worst.items())) + "\n")


def note(key, value):
    _worst[key] = max(_worst.get(key, 0.0), float(value))


# ------------------------------------------------------------------------------ the batch
class Case:
    def __init__(self, graphs):
        self.counts = [len(g) for g in graphs]
        self.ptr = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        self.N = int(self.ptr[-1])
        self.sigma = np.concatenate([np.asarray(g, np.float32).reshape(-1, 3) for g in graphs])
        self.scale = float(np.nanmax(np.abs(self.sigma)))
        self.d_ptr = torch.from_numpy(self.ptr).to(dev(), torch.int32)
        self.d_sigma = torch.from_numpy(self.sigma).to(dev())

    def segment(self, g):
        return int(self.ptr[g]), int(self.ptr[g + 1])


@functools.lru_cache(maxsize=None)
def ragged() -> Case:
    rng = np.random.default_rng(17)
    return Case([(rng.normal(size=(n, 3)) * np.array([40.0, 25.0, 10.0]) + np.array([60.0, -35.0, 8.0]))
                 for n in COUNTS])


@functools.lru_cache(maxsize=None)
def weights_of(kind):
    """(numpy fp32 or None, device tensor or None)."""
    c = ragged()
    if kind == "none":
        return None, None
    rng = np.random.default_rng(WEIGHTS.index(kind))
    w = rng.uniform(0.25, 4.0, size=c.N).astype(np.float32)
    if kind == "mixed":
        u = rng.random(c.N)
        w[u < 0.1] = 0.0
        w[(u >= 0.1) & (u < 0.2)] = -1.5
        w[(u >= 0.2) & (u < 0.3)] = np.nan
        n0, _ = c.segment(COUNTS.index(4097))
        w[n0 + 4096] = 2.0          # the row past the cached ones takes part
    elif kind == "excluded":
        n0, n1 = c.segment(EXCLUDED)
        w[n0:n1] = 0.0
    return w, torch.from_numpy(w).to(dev())


def guarded(n, width):
    return torch.full((n + GUARD, width), float("nan"), dtype=torch.float32, device=dev())


def forward(ptr, sigma, w, cid, p, rho, fields=True):
    from pdg.lib import lib, ptr as P, stream_handle
    b, n = ptr.numel() - 1, sigma.shape[0]
    table = torch.full((b, 4), -7.0, dtype=torch.float64, device=dev())
    argmax = torch.full((b,), -7, dtype=torch.int32, device=dev())
    f = guarded(n, 6) if fields else None
    lib.pdg_stress_criteria(b, ptr.data_ptr(), sigma.data_ptr(), P(w), cid, p, rho, table.data_ptr(),
                            argmax.data_ptr(), P(f), stream_handle(dev()))
    return table, argmax, f


def backward(ptr, sigma, w, cid, aid, p, rho, table, argmax, gv=None):
    from pdg.lib import lib, ptr as P, stream_handle
    b, n = ptr.numel() - 1, sigma.shape[0]
    g = guarded(n, 3)
    lib.pdg_stress_criteria_bwd(b, ptr.data_ptr(), sigma.data_ptr(), P(w), cid, aid, p, rho, table.data_ptr(),
                                argmax.data_ptr(), P(gv), g.data_ptr(), stream_handle(dev()))
    return g


def bits(t):
    t = t.contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32).cpu()


def check_table(got, ref, what, key):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, got, ref)
    fin = ~np.isnan(ref)
    assert np.isfinite(ref[fin]).all(), what
    err = np.abs(got[fin] - ref[fin])
    rel = err / np.maximum(np.abs(ref[fin]), 1e-300)
    note(key, rel.max() if rel.size else 0.0)
    assert np.all(err <= 1e-10 * np.abs(ref[fin])), (what, got, ref)


def check_rounded(got, ref, what, key, extra=0.0):
    """got fp32 within 2^-23 |ref| + extra of the fp64 ref; NaNs where the ref has them."""
    got, ref = np.asarray(got), np.asarray(ref, np.float64)
    assert got.dtype == np.float32 and got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    fin = ~np.isnan(ref)
    err = np.abs(got[fin].astype(np.float64) - ref[fin])
    bound = 2.0 ** -23 * np.abs(ref[fin]) + extra
    ratio = err / np.maximum(bound, 1e-300)
    ratio[err == 0] = 0.0
    note(key, ratio.max() if ratio.size else 0.0)
    assert np.all(err <= bound), (what, float(ratio.max()))


def check_forward(c: Case, w, criterion, p, rho, table, argmax, f):
    ref_t, ref_a = R.batch_criteria(c.ptr, c.sigma, w, criterion, p, rho)
    what = f"{criterion} p={p} rho={rho}"
    for col, name in enumerate(R.AGGREGATES):
        check_table(table[:, col].cpu().numpy(), ref_t[:, col], f"{what} {name}", f"table {criterion} {name}")
    assert np.array_equal(argmax.cpu().numpy().astype(np.int64), ref_a), (what, argmax, ref_a)
    if f is not None:
        rf = R.fields(c.sigma, criterion)
        for col, name in enumerate(R.FIELDS):
            check_rounded(f[:c.N, col].cpu().numpy(), rf[name], f"{what} field {name}", f"field {name}")
        assert torch.isnan(f[c.N:]).all()
    return ref_t, ref_a


def check_backward(c: Case, w, criterion, aggregate, p, rho, g, gv=None):
    ref = R.batch_criteria_grad(c.ptr, c.sigma, w, criterion, aggregate, p, rho, gv)
    got = g[:c.N].cpu().numpy()
    what = f"{criterion} {aggregate} p={p} rho={rho}"
    for gi in range(len(c.counts)):
        n0, n1 = c.segment(gi)
        if n1 == n0:
            continue
        r = ref[n0:n1]
        extra = 1e-10 * float(np.nanmax(np.abs(r))) if aggregate in ("pnorm", "ks") and not np.isnan(r).all() else 0.0
        check_rounded(got[n0:n1], r, f"{what} graph {gi}", f"g_sigma {criterion} {aggregate}", extra)
        if w is not None:   # a row that takes no part is an exact zero row
            out = ~(w[n0:n1] > 0)
            assert (got[n0:n1][out] == 0).all(), what
    assert torch.isnan(g[c.N:]).all()


# ------------------------------------------------------------------------------ gates
@pytest.mark.parametrize("kind", WEIGHTS)
@pytest.mark.parametrize("criterion", R.CRITERIA)
def test_ragged_batch_against_the_yardstick(criterion, kind):
    c = ragged()
    assert tuple(c.counts) == COUNTS
    w, dw = weights_of(kind)
    cid = R.CRITERIA.index(criterion)
    e = COUNTS.index(0)
    done = set()
    for p, r in itertools.product(PS, RHOS):
        rho = r / c.scale
        table, argmax, f = forward(c.d_ptr, c.d_sigma, dw, cid, p, rho, fields=(p == PS[0] and r == RHOS[0]))
        ref_t, ref_a = check_forward(c, w, criterion, p, rho, table, argmax, f)
        assert torch.isnan(table[e]).all() and int(argmax[e]) == -1          # the empty graph
        if kind == "none":
            assert np.isfinite(ref_t[np.array(COUNTS) > 0]).all()
        if kind == "excluded":   # NaN values, but its fields are written
            assert torch.isnan(table[EXCLUDED]).all() and int(argmax[EXCLUDED]) == -1
            if f is not None:
                n0, n1 = c.segment(EXCLUDED)
                assert torch.isfinite(f[n0:n1]).all()
        # max and mean once, pnorm per p, ks per rho
        for aid, key in ((0, None), (1, None), (2, p), (3, r)):
            if (aid, key) in done:
                continue
            done.add((aid, key))
            g = backward(c.d_ptr, c.d_sigma, dw, cid, aid, p, rho, table, argmax)
            check_backward(c, w, criterion, R.AGGREGATES[aid], p, rho, g)
    assert len(done) == 2 + len(PS) + len(RHOS)


PLANTED = [
    [[0, 0, 0]] * 3,                                                  # 0: an all-zero graph
    [[3, 3, 0], [1, 0.5, 0.25]],                                      # 1: an isotropic maximum
    [[4, 0, 0], [1, 0.5, 0.25]],                                      # 2: s2 == 0, Tresca's 2 r == |s1| tie
    [[1, 0, 0], [5, 0, 0], [2, 0, 0], [5, 0, 0]],                     # 3: two equal maxima
    [[1e30, 0, 0], [5e29, 1e29, 0], [0, 0, 0]],                       # 4: no overflow
    [[1, 2, 3], [np.nan, 0, 0], [4, 5, 6]],                           # 5: a NaN row
    [[1, 2, 3], [np.nan, 0, 0], [4, 5, 6]],                           # 6: the same, the NaN row excluded
]


def test_planted_rows():
    c = Case(PLANTED)
    w = np.ones(c.N, np.float32)
    w[c.segment(6)[0] + 1] = 0.0
    dw = torch.from_numpy(w).to(dev())
    p, rho = 64.0, 1e3 / 1e30
    out = {}
    for cid, criterion in enumerate(R.CRITERIA):
        table, argmax, f = forward(c.d_ptr, c.d_sigma, dw, cid, p, rho)
        check_forward(c, w, criterion, p, rho, table, argmax, f)
        for aid, aggregate in enumerate(R.AGGREGATES):
            g = backward(c.d_ptr, c.d_sigma, dw, cid, aid, p, rho, table, argmax)
            check_backward(c, w, criterion, aggregate, p, rho, g)
            out[criterion, aggregate] = g[:c.N].cpu().numpy()
        out[criterion] = (table.cpu().numpy(), argmax.cpu().numpy())
    row = lambda g, i=0: c.segment(g)[0] + i
    for criterion in R.CRITERIA:
        t, a = out[criterion]
        # the zero graph: every value 0 (pnorm by its rule), the first node the peak, zero gradients, no NaN
        assert (t[0] == 0).all() and a[0] == 0
        for aggregate in R.AGGREGATES:
            assert (out[criterion, aggregate][row(0):row(0) + 3] == 0).all()
        # 1e30 with p = 64 and rho c = 1e3: finite values and gradients
        assert np.isfinite(t[4]).all() and a[4] == 0 and t[4, 0] == np.float64(np.float32(1e30))
        for aggregate in R.AGGREGATES:
            assert np.isfinite(out[criterion, aggregate][row(4):row(4) + 3]).all()
        # two equal maxima: the lowest index wins and carries the whole gradient
        assert a[3] == 1 and t[3, 0] == 5.0
        g = out[criterion, "max"][row(3):row(3) + 4]
        assert (g[[0, 2, 3]] == 0).all() and (g[1] != 0).any()
        # a NaN row that takes part makes the graph NaN; excluded it has no effect
        assert np.isnan(t[5]).all() and a[5] == -1 and np.isnan(out[criterion, "mean"][row(5):row(5) + 3]).all()
        assert np.isfinite(t[6]).all() and a[6] == 2
        g = out[criterion, "ks"][row(6):row(6) + 3]
        assert (g[1] == 0).all() and np.isfinite(g).all()
    # the isotropic tensor: d s1 = (1/2, 1/2, 0)
    assert out["rankine"][1][1] == 0 and (out["rankine", "max"][row(1)] == np.float32([0.5, 0.5, 0.0])).all()
    # s2 == 0 exactly: the 2 r branch wins the tie with |s1|, gradient 2 dr = (1, -1, 0)
    assert out["tresca"][1][2] == 0 and out["tresca"][0][2, 0] == 4.0
    assert (out["tresca", "max"][row(2)] == np.float32([1.0, -1.0, 0.0])).all()


@pytest.mark.parametrize("criterion", R.CRITERIA)
def test_each_graph_scores_the_same_alone_and_determinism(criterion):
    c = ragged()
    w, dw = weights_of("mixed")
    cid = R.CRITERIA.index(criterion)
    p, rho = 8.0, 1.0 / c.scale
    table, argmax, f = forward(c.d_ptr, c.d_sigma, dw, cid, p, rho)
    grads = [backward(c.d_ptr, c.d_sigma, dw, cid, aid, p, rho, table, argmax) for aid in range(4)]
    t2, a2, f2 = forward(c.d_ptr, c.d_sigma, dw, cid, p, rho)
    assert torch.equal(bits(t2), bits(table)) and torch.equal(a2, argmax) and torch.equal(bits(f2), bits(f))
    for aid in range(4):
        assert torch.equal(bits(backward(c.d_ptr, c.d_sigma, dw, cid, aid, p, rho, table, argmax)), bits(grads[aid]))
    for g, n in enumerate(c.counts):
        if n == 0:
            continue
        n0, n1 = c.segment(g)
        ptr = torch.tensor([0, n], dtype=torch.int32, device=dev())
        s1, w1 = c.d_sigma[n0:n1].contiguous(), dw[n0:n1].contiguous()
        t1, a1, f1 = forward(ptr, s1, w1, cid, p, rho)
        assert torch.equal(bits(t1[0]), bits(table[g])) and int(a1[0]) == int(argmax[g]), (g, n)
        assert torch.equal(bits(f1[:n]), bits(f[n0:n1])) and torch.isnan(f1[n:]).all(), (g, n)
        for aid in range(4):
            g1 = backward(ptr, s1, w1, cid, aid, p, rho, t1, a1)
            assert torch.equal(bits(g1[:n]), bits(grads[aid][n0:n1])) and torch.isnan(g1[n:]).all(), (g, n, aid)


def test_null_fields_and_weights_of_one():
    """The table does not depend on the optional outputs, and NULL weights are weights of 1."""
    c = ragged()
    ones = torch.ones(c.N, dtype=torch.float32, device=dev())
    for cid in range(3):
        a = forward(c.d_ptr, c.d_sigma, None, cid, 8.0, 1.0 / c.scale)
        b = forward(c.d_ptr, c.d_sigma, None, cid, 8.0, 1.0 / c.scale, fields=False)
        d = forward(c.d_ptr, c.d_sigma, ones, cid, 8.0, 1.0 / c.scale, fields=False)
        assert b[2] is None
        for x in (b, d):
            assert torch.equal(bits(a[0]), bits(x[0])) and torch.equal(a[1], x[1])
        for aid in range(4):
            ga = backward(c.d_ptr, c.d_sigma, None, cid, aid, 8.0, 1.0 / c.scale, a[0], a[1])
            gd = backward(c.d_ptr, c.d_sigma, ones, cid, aid, 8.0, 1.0 / c.scale, a[0], a[1])
            assert torch.equal(bits(ga), bits(gd))


def test_g_value_scales_exactly_by_powers_of_two():
    c = ragged()
    w, dw = weights_of("positive")
    b = len(c.counts)
    gv = torch.tensor([2.0 ** k for k in (3, -2, 0, 1, -5, 7, 4, -1, 2, -3)][:b], device=dev())
    per_node = torch.repeat_interleave(gv, torch.from_numpy(np.diff(c.ptr)).to(dev()))[:, None]
    for cid, aid in itertools.product(range(3), range(4)):
        p, rho = 8.0, 1.0 / c.scale
        table, argmax, _ = forward(c.d_ptr, c.d_sigma, dw, cid, p, rho, fields=False)
        one = backward(c.d_ptr, c.d_sigma, dw, cid, aid, p, rho, table, argmax)
        ones = backward(c.d_ptr, c.d_sigma, dw, cid, aid, p, rho, table, argmax, torch.ones(b, device=dev()))
        scaled = backward(c.d_ptr, c.d_sigma, dw, cid, aid, p, rho, table, argmax, gv)
        assert torch.equal(bits(one), bits(ones))
        assert torch.equal(bits(scaled[:c.N]), bits(one[:c.N] * per_node)), (cid, aid)
    table, argmax, _ = forward(c.d_ptr, c.d_sigma, dw, 1, p, rho, fields=False)
    scaled = backward(c.d_ptr, c.d_sigma, dw, 1, 2, p, rho, table, argmax, gv)
    check_backward(c, w, "tresca", "pnorm", p, rho, scaled, gv.cpu().numpy().astype(np.float64))


def test_both_calls_are_capturable_and_replay_bitwise():
    from pdg.lib import lib, stream_handle
    c = ragged()
    _, dw = weights_of("mixed")
    cid, aid, p, rho = 1, 3, 8.0, 1.0 / c.scale
    b = len(c.counts)
    eager_t, eager_a, eager_f = forward(c.d_ptr, c.d_sigma, dw, cid, p, rho)
    eager_g = backward(c.d_ptr, c.d_sigma, dw, cid, aid, p, rho, eager_t, eager_a)
    table = torch.full((b, 4), -7.0, dtype=torch.float64, device=dev())
    argmax = torch.full((b,), -7, dtype=torch.int32, device=dev())
    f, g = guarded(c.N, 6), guarded(c.N, 3)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = stream_handle(dev())
        lib.pdg_stress_criteria(b, c.d_ptr.data_ptr(), c.d_sigma.data_ptr(), dw.data_ptr(), cid, p, rho,
                                table.data_ptr(), argmax.data_ptr(), f.data_ptr(), s)
        lib.pdg_stress_criteria_bwd(b, c.d_ptr.data_ptr(), c.d_sigma.data_ptr(), dw.data_ptr(), cid, aid, p, rho,
                                    table.data_ptr(), argmax.data_ptr(), None, g.data_ptr(), s)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(table), bits(eager_t)) and torch.equal(argmax, eager_a)
    assert torch.equal(bits(f), bits(eager_f)) and torch.equal(bits(g), bits(eager_g))


def test_python_api():
    from gnn_local_stress import criteria as C
    c = ragged()
    w, dw = weights_of("mixed")
    rho = 1.0 / c.scale
    r = C.graph_criterion(c.d_sigma, c.d_ptr, "tresca", weights=dw, p=8.0, rho=rho, fields=True)
    table, argmax, f = forward(c.d_ptr, c.d_sigma, dw, 1, 8.0, rho)
    for i, k in enumerate(C.AGGREGATES):
        assert getattr(r, k).dtype == torch.float64 and torch.equal(bits(getattr(r, k)), bits(table[:, i])), k
    assert torch.equal(r.argmax, argmax.long()) and r.rho == rho and r.p == 8.0
    ok = r.argmax >= 0
    assert torch.equal(r.node[ok], (r.argmax + c.d_ptr[:-1].long())[ok]) and (r.node[~ok] == -1).all()
    assert list(r.fields) == list(C.FIELDS)
    for i, k in enumerate(C.FIELDS):
        assert torch.equal(bits(r.fields[k]), bits(f[:c.N, i])), k
    sf = C.stress_fields(c.d_sigma, "tresca")
    rf = R.fields(c.sigma, "tresca")
    for k in C.FIELDS:
        check_rounded(sf[k].cpu().numpy(), rf[k], f"stress_fields {k}", f"field {k}")
    g = C.graph_criterion_grad(c.d_sigma, c.d_ptr, "tresca", "ks", weights=dw, p=8.0, rho=rho)
    assert torch.equal(bits(g), bits(backward(c.d_ptr, c.d_sigma, dw, 1, 3, 8.0, rho, table, argmax)[:c.N]))
    # rho=None: ks with rho = 1, labelled as such; the gradient of ks then refuses
    assert C.graph_criterion(c.d_sigma, c.d_ptr).rho == 1.0
    with pytest.raises(ValueError, match="needs rho"):
        C.graph_criterion_grad(c.d_sigma, c.d_ptr, aggregate="ks")
    # a single graph without a batch object, and a ptr that does not cover the field
    n0, n1 = c.segment(4)
    one = C.graph_criterion(c.d_sigma[n0:n1], torch.tensor([0, n1 - n0]), "tresca", weights=dw[n0:n1], rho=rho)
    assert torch.equal(bits(one.max), bits(r.max[4:5])) and torch.equal(bits(one.ks), bits(r.ks[4:5]))
    with pytest.raises(ValueError, match="ptr must rise"):
        C.graph_criterion(c.d_sigma, torch.tensor([0, c.N + 1]))
    with pytest.raises(RuntimeError, match="HIP"):
        C.graph_criterion(c.d_sigma.cpu(), c.d_ptr)
