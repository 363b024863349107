"""The fp64 restatements of the loss and step-guard kernels (tests/loss_ref.py), which the GPU op tests hold the
kernels to, against the oracle: the dense oracle.epd_oracle.compute_divergence (tied to the upstream golden
vectors by test_oracle_golden.py), torch autograd through it, the plan's CPU path for the operator arrays, and the
closed form of the NMSE gradient.  The references are anchored to the model, not to a second derivation."""
import pytest
import torch

from golden_io import load
from loss_ref import (DIV_SIZES, abs_rows_left_out, build_div_csr, div_bwd_ref, div_fwd_ref, format_ref, loss_ref,
                      loss_reduce_ref, nmse_ref, nonfinite_ref, random_div_case)
from oracle import epd_oracle as O
from pdg.plan import GraphPlan

F64 = torch.float64
SCALE = 0.125 * 10 / len(DIV_SIZES)


def rel(a, b):
    return float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-300))


def golden_case():
    g = load("batch3_div")
    ptr = torch.from_numpy(g["ptr"]).long()
    rows, cols, vals = [], [], []
    for i, op in enumerate(g["op_divs"]):
        idx = op.indices()
        rows.append(idx[0] + ptr[i])
        cols.append(idx[1])
        vals.append(op.values())
    from types import SimpleNamespace
    return SimpleNamespace(ptr=ptr, N=int(ptr[-1]), B=ptr.numel() - 1, rows=torch.cat(rows), cols=torch.cat(cols),
                           vals=torch.cat(vals).float(), types=torch.from_numpy(g["nodes_types"]).reshape(-1),
                           sigma=torch.from_numpy(g["pred"]))


@pytest.fixture(scope="module", params=["batch3_div", "ragged"])
def case(request):
    c = golden_case() if request.param == "batch3_div" else random_div_case()
    c.name = request.param
    c.op = build_div_csr(c.ptr, c.rows, c.cols, c.vals, keep_beyond=True)
    return c


def dense_ops(c):
    """Each graph's operator as the sparse (n, >= 2 n) matrix the oracle takes (duplicates summed by to_dense)."""
    ops = []
    for g in range(c.B):
        lo, hi = int(c.ptr[g]), int(c.ptr[g + 1])
        m = (c.rows >= lo) & (c.rows < hi)
        ops.append(torch.sparse_coo_tensor(torch.stack([c.rows[m] - lo, c.cols[m]]), c.vals[m].double(),
                                           (hi - lo, 2 * (hi - lo) + 8)))
    return ops


def oracle_losses(c, sigma, strategy):
    out = []
    for g, op in enumerate(dense_ops(c)):
        lo, hi = int(c.ptr[g]), int(c.ptr[g + 1])
        out.append(None if hi == lo else O.compute_divergence(sigma[lo:hi], op, c.types[lo:hi].reshape(-1, 1), strategy))
    return out


def test_ragged_case_has_the_edges_it_claims():
    c = random_div_case()
    g = torch.searchsorted(c.ptr, c.rows, right=True) - 1
    ng = c.ptr[g + 1] - c.ptr[g]
    op = build_div_csr(c.ptr, c.rows, c.cols, c.vals, keep_beyond=True)
    per_row = op.a_rowptr[1:] - op.a_rowptr[:-1]
    beyond = float((c.cols >= 2 * ng).double().mean())
    assert c.sizes == DIV_SIZES and c.sizes[5] == 0 and c.N == sum(DIV_SIZES)
    assert int(per_row.min()) == 0 and int(per_row.max()) == 20 and float((per_row == 0).double().mean()) > 0.1
    assert 0.03 < beyond < 0.07 and int(c.cols.max() - 2 * ng[c.cols.argmax()]) < 8
    assert bool((c.cols < ng).any()) and bool(((c.cols >= ng) & (c.cols < 2 * ng)).any())
    starts = op.a_rowptr[:-1].long()
    unsorted = repeated = 0
    for v in range(c.N):
        r = op.a_col[starts[v]:starts[v] + per_row[v]]
        unsorted += bool((r[1:] < r[:-1]).any())
        repeated += r.unique().numel() < r.numel()
    assert unsorted > c.N // 2 and repeated > c.N // 10
    assert sorted(c.types.unique().tolist()) == [-1, 0, 1, 2]
    # the A^T arrays hold the in-range entries only
    assert int(op.at_rowptr[-1]) == int((c.cols < 2 * ng).sum()) < int(op.a_rowptr[-1]) == c.rows.numel()


@pytest.mark.parametrize("strategy", ["square", "abs"])
def test_div_fwd_ref_equals_dense_oracle(case, strategy):
    """div_fwd_ref's per-graph loss equals oracle.compute_divergence (dense, [:, :2n] sliced) to 1e-12; an empty
    graph gives NaN; entries at or beyond 2 n_g change nothing."""
    c = case
    div, loss, bound = div_fwd_ref(c.ptr, c.op.a_rowptr, c.op.a_col, c.op.a_val, c.types, c.sigma, strategy == "abs")
    for g, ref in enumerate(oracle_losses(c, c.sigma.double(), strategy)):
        if ref is None:
            assert bool(loss[g].isnan())
        else:
            assert abs(float(loss[g]) - float(ref)) <= 1e-12 * abs(float(ref)), (g, float(loss[g]), float(ref))
    op = build_div_csr(c.ptr, c.rows, c.cols, c.vals)
    div2, loss2, bound2 = div_fwd_ref(c.ptr, op.a_rowptr, op.a_col, op.a_val, c.types, c.sigma, strategy == "abs")
    assert torch.equal(div, div2) and torch.equal(bound, bound2) and torch.equal(loss.isnan(), loss2.isnan())
    assert torch.equal(loss[~loss.isnan()], loss2[~loss2.isnan()])
    masked = (c.types == 1) | (c.types == -1)
    assert float(div[masked].abs().max()) == 0 and float(bound[masked].abs().max()) == 0


@pytest.mark.parametrize("strategy", ["square", "abs"])
def test_div_bwd_ref_equals_oracle_autograd(case, strategy):
    """div_bwd_ref(div_fwd_ref(...)) equals autograd of scale * sum_g compute_divergence to 1e-12, everywhere
    for both strategies: torch's |.| has gradient sign(0) = 0 at 0, which is what the restatement (and the
    kernel) use, so the rows fed by an exactly zero div entry agree as well as those with |div| > 0.  loss_ref
    (autograd through div_fwd_ref) gives the same gradient."""
    c = case
    ra = strategy == "abs"
    div, _, _ = div_fwd_ref(c.ptr, c.op.a_rowptr, c.op.a_col, c.op.a_val, c.types, c.sigma, ra)
    gs, bound = div_bwd_ref(c.ptr, c.op.at_rowptr, c.op.at_row, c.op.at_comp, c.op.at_val, div, SCALE, ra)
    sig = c.sigma.double().requires_grad_(True)
    total = sum(l for l in oracle_losses(c, sig, strategy) if l is not None) * SCALE
    (ref,) = torch.autograd.grad(total, sig)
    assert rel(gs, ref) < 1e-12
    fed = gs.abs().sum(1) > 0
    assert rel(gs[fed], ref[fed]) < 1e-12 and float((gs - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    div2, g2 = loss_ref(c.ptr, c.op.a_rowptr, c.op.a_col, c.op.a_val, c.types, c.sigma, SCALE, ra)
    assert torch.equal(div, div2) and rel(g2, ref) < 1e-12
    assert bool((bound >= 0).all()) and bool((bound[fed] > 0).any(1).all())


def test_builder_equals_the_plans_cpu_path(case):
    """build_div_csr equals pdg.plan.GraphPlan._build_div (the torch planner) array for array."""
    c = case
    plan = GraphPlan(torch.zeros(2, 0, dtype=torch.int64), c.N, c.ptr, c.rows, c.cols, c.vals, planner="torch")
    op = build_div_csr(c.ptr, c.rows, c.cols, c.vals)
    for k in ("a_rowptr", "a_col", "a_val", "at_rowptr", "at_row", "at_comp", "at_val"):
        mine, theirs = getattr(op, k), getattr(plan, k)
        assert mine.dtype == theirs.dtype and torch.equal(mine, theirs), k


def test_abs_rows_left_out_stay_under_the_cap():
    """The composed 'abs' GPU test leaves out the g_sigma rows fed by a div entry with 0 < |div64| <
    1e-4 rms(div64) and asserts they are at most 0.1 % of the rows; with the committed seed the reference alone
    stays under that cap."""
    c = random_div_case()
    op = build_div_csr(c.ptr, c.rows, c.cols, c.vals, keep_beyond=True)
    div, _, _ = div_fwd_ref(c.ptr, op.a_rowptr, op.a_col, op.a_val, c.types, c.sigma, True)
    out = abs_rows_left_out(op, div)
    print(f"rows left out: {int(out.sum())} of {c.N} ({float(out.double().mean()):.2e})")
    assert int(out.sum()) <= 1e-3 * c.N


def test_nmse_ref_equals_closed_form():
    g = torch.Generator().manual_seed(3)
    sizes = (17, 2, 300, 25)
    ptr = torch.tensor([0] + list(torch.tensor(sizes).cumsum(0)))
    gt, pred = torch.randn(sum(sizes), 3, generator=g), torch.randn(sum(sizes), 3, generator=g)
    loss, den, grad = nmse_ref(ptr, gt, pred, 0.125)
    for b in range(len(sizes)):
        t, p = gt[ptr[b]:ptr[b + 1]].double(), pred[ptr[b]:ptr[b + 1]].double()
        d = (t - t.mean(0)).square().sum(0)
        assert rel(den[b], d) < 1e-12
        assert abs(float(loss[b]) - float(((t - p).square().sum(0) / d).mean())) < 1e-12 * float(loss[b])
        assert rel(grad[ptr[b]:ptr[b + 1]], 0.125 * -2 * (t - p) / (3 * d)) < 1e-12


def test_one_liners():
    nan, inf = float("nan"), float("inf")
    x = torch.tensor([0.0, 3e38, 1e-45])
    assert nonfinite_ref(x, None) == 0 and nonfinite_ref(x, 1.0) == 0
    assert nonfinite_ref(x, 0.0) == 1 and nonfinite_ref(x, -0.0) == 1
    assert all(nonfinite_ref(torch.tensor([0.0, v]), 1.0) == 1 for v in (nan, inf, -inf))
    assert nonfinite_ref(torch.empty(0), None) == 0
    ln, ld = torch.tensor([1.0, 2.0]), torch.tensor([0.5, 0.25])
    assert loss_reduce_ref(ln, ld, 0.5, 4.0, None) == [1.0, 1.5, 3.0, 4.5]
    assert loss_reduce_ref(ln, None, 0.5, 4.0, 0.0) == [0.0, 1.5, 0.0, 1.5]
    stats = {k: torch.tensor(v) for k, v in dict(mean_pos=1.0, std_pos=2.0, mean_mean_stress=3.0, std_mean_stress=4.0,
                                                 mean_edge_weight=5.0, std_edge_weight=0.5).items()}
    pos, ms = torch.tensor([[3.0, 5.0]]), torch.tensor([[7.0, 11.0, -1.0]])
    ea, perm, types = torch.tensor([6.0, 4.0]), torch.tensor([1, 0]), torch.tensor([-1])
    x, e = format_ref(stats, pos, ms, types, ea, perm, True)
    assert x.tolist() == [[1.0, 2.0, -1.0, 1.0, 2.0, -1.0]] and e.tolist() == [-2.0, 2.0]
    x, e = format_ref(stats, pos, ms, types, ea, perm, False)
    assert x.tolist() == [[7.0, 11.0, -1.0, 3.0, 5.0, -1.0]] and e.tolist() == [4.0, 6.0]
