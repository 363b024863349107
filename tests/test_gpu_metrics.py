"""The evaluation-metrics kernels (csrc/pdg_metrics.hip) and gnn_local_stress.metrics on the GPU.

Yardsticks: the reference's own functions through tests/golden/eval_metrics.npz, and tests/metrics_ref.py
(fp64 numpy, pinned to that fixture by tests/test_metrics_ref.py) for arbitrary shapes.

Bounds.  A table value is a quotient of fp64 sums of non-negative terms formed from the same fp32
inputs as the yardstick's: both sides are within n 2^-53 of the exact sum (below 1e-12 at these
sizes) and 1e-10 relative leaves room for the different summation order.  A field value is that fp64
value rounded once to fp32: within 2^-23 |ref| + 1e-30 of the fp64 yardstick.  Infinities and NaNs
(zero denominators, the empty graph) must sit where numpy puts them.
"""
import functools
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import metrics_ref as R

pytestmark = pytest.mark.gpu

FIXTURE = Path(__file__).resolve().parent / "golden" / "eval_metrics.npz"
GOLDEN = ("plate8", "hole12", "plate17")
GUARD = 8
# a single node (zero denominators); sizes under, at and over a wave (64) and a workgroup (1024); an
# empty graph between two non-empty ones; 5,041 nodes (past the 4,096 a block keeps in registers)
COUNTS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 0, 5041)
STRATEGIES = ("square", "abs")
MEAN, STD = 12.5, 37.25          # exact in fp32


def dev():
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------ cases
def random_graph(n: int, rng):
    """gt, pred (n, 3) f32, labels (n) i64 and a random COO operator of n rows (graph-local rows and
    columns): empty rows, one row of 200 to 249 entries (n >= 2), duplicate entries, columns up to
    2n + 2 (those at or beyond 2n are for the plan to drop), about 5 % of the labels each of +1 / -1."""
    gt = (rng.normal(size=(n, 3)) * np.array([40.0, 25.0, 10.0]) + np.array([60.0, -35.0, 8.0])).astype(np.float32)
    pred = (gt + rng.normal(size=(n, 3)) * np.array([6.0, 4.0, 3.0])).astype(np.float32)
    labels = rng.choice(np.array([0, 1, -1]), size=n, p=[0.9, 0.05, 0.05]).astype(np.int64)
    k = rng.integers(1, 25, size=n)
    k[rng.random(n) < 0.2] = 0
    if n == 1:
        k[0] = 5
    elif n >= 2:
        k[n - 1] = 200 + int(rng.integers(0, 50))
        labels[n - 1] = 0
    if n >= 5:   # both signs on rows that have entries, an unmasked empty row
        labels[:4] = (0, 1, -1, 0)
        k[:4] = (7, 9, 11, 0)
    rows = np.repeat(np.arange(n), k)
    cols = rng.integers(0, 2 * n + 3, size=len(rows))
    vals = rng.normal(size=len(rows)).astype(np.float32)
    return gt, pred, labels, rows, cols, vals


def p1_graph(n: int, hole: float, seed: int):
    """A hole plate with its own smooth stress field, P1 divergence operator and labels; pred = gt + noise."""
    from pdg import meshgen
    s = meshgen.hole_plate(n, hole_radius=hole, seed=seed)
    rng = np.random.default_rng(seed)
    pred = (s.local_stress + rng.normal(size=s.local_stress.shape) * 4.0).astype(np.float32)
    return s.local_stress, pred, s.node_types, s.op_div_rows, s.op_div_cols, s.op_div_vals


class Case:
    """One batch on the device with its plan-built operator, and the pieces the yardstick needs."""

    def __init__(self, graphs, mean=MEAN, std=STD):
        from pdg.plan import GraphPlan
        self.mean, self.std = float(np.float32(mean)), float(np.float32(std))
        self.counts = [len(g[0]) for g in graphs]
        self.ptr = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        N = int(self.ptr[-1])
        self.gt = np.concatenate([g[0] for g in graphs]).astype(np.float32).reshape(N, 3)
        self.pred = np.concatenate([g[1] for g in graphs]).astype(np.float32).reshape(N, 3)
        self.labels = np.concatenate([g[2] for g in graphs]).astype(np.int64)
        rows = np.concatenate([g[3] + self.ptr[i] for i, g in enumerate(graphs)]).astype(np.int64)
        cols = np.concatenate([g[4] for g in graphs]).astype(np.int64)
        vals = np.concatenate([g[5] for g in graphs]).astype(np.float32)
        d = dev()
        plan = GraphPlan.__new__(GraphPlan)
        plan.n_nodes, plan.n_edges, plan.n_graphs = N, 0, len(graphs)
        plan.ptr = torch.from_numpy(self.ptr).to(d, torch.int32)
        plan.has_div = True
        plan._build_div_device(torch.from_numpy(rows), torch.from_numpy(cols), torch.from_numpy(vals))
        plan.validate()
        self.plan = plan
        # the plan keeps the entries below column 2 n_g, a row's entries in their given order
        n_of_row = np.repeat(np.array(self.counts, np.int64), self.counts)
        keep = cols < 2 * n_of_row[rows]
        self.a_rowptr = plan.a_rowptr.cpu().numpy().astype(np.int64)
        self.a_col, self.a_val = plan.a_col.cpu().numpy().astype(np.int64), plan.a_val.cpu().numpy()
        assert np.array_equal(self.a_rowptr, np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=N))]))
        assert 0 < keep.sum() and np.array_equal(np.sort(self.a_val), np.sort(vals[keep]))
        self.dropped = int((~keep).sum())
        self.d_gt, self.d_pred = torch.from_numpy(self.gt).to(d), torch.from_numpy(self.pred).to(d)
        self.d_types = torch.from_numpy(self.labels).to(d)

    def graph_csr(self, g):
        n0, n1 = int(self.ptr[g]), int(self.ptr[g + 1])
        rp = self.a_rowptr[n0:n1 + 1]
        return rp - rp[0], self.a_col[rp[0]:rp[-1]], self.a_val[rp[0]:rp[-1]]

    @functools.lru_cache(maxsize=None)
    def reference(self, strategy):
        out = []
        for g in range(len(self.counts)):
            n0, n1 = int(self.ptr[g]), int(self.ptr[g + 1])
            out.append(R.graph_metrics(self.gt[n0:n1], self.pred[n0:n1], self.graph_csr(g), self.labels[n0:n1],
                                       self.mean, self.std, strategy))
        return out


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    rng = np.random.default_rng({"shapes": 5, "big": 6, "p1": 7}[name])
    if name == "shapes":
        return Case([random_graph(n, rng) for n in COUNTS])
    if name == "big":
        return Case([random_graph(20000, rng)])
    return Case([p1_graph(25, 0.3005, 7), p1_graph(9, 0.25, 8)])


# ------------------------------------------------------------------------------ launches
def guarded(n, width=None):
    """An fp32 field buffer of n rows and GUARD more, all NaN."""
    shape = (n + GUARD,) if width is None else (n + GUARD, width)
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev())


def launch(n_graphs, ptr, gt, pred, types, a_rowptr, a_col, a_val, mean, std, strategy, fields=True):
    """Both kernels (pdg_eval_div on pred and on gt) on device tensors.  Tables as fp64 tensors; fields in
    guarded buffers (None without `fields`)."""
    from pdg.lib import lib, stream_handle
    d, n = dev(), gt.shape[0]
    s = stream_handle(d)
    rabs = int(strategy == "abs")
    o = {"nmse_table": torch.full((n_graphs, 6), -7.0, dtype=torch.float64, device=d)}
    for k, w in (("err_field", 4), ("vm_gt", None), ("vm_pred", None), ("norm", None), ("norm_std", None),
                 ("norm_fem", None), ("norm_fem_std", None)):
        o[k] = guarded(n, w) if fields else None
    f = (lambda k: o[k].data_ptr()) if fields else (lambda k: None)
    lib.pdg_eval_nmse(n_graphs, ptr.data_ptr(), gt.data_ptr(), pred.data_ptr(), o["nmse_table"].data_ptr(),
                      f("err_field"), f("vm_gt"), f("vm_pred"), s)
    col = a_col if a_col.numel() else a_rowptr     # no entries: never read, but not NULL
    val = a_val if a_val.numel() else a_rowptr
    for tag, sigma in (("", pred), ("_fem", gt)):
        o["div_table" + tag] = torch.full((n_graphs, 2), -7.0, dtype=torch.float64, device=d)
        lib.pdg_eval_div(n_graphs, ptr.data_ptr(), a_rowptr.data_ptr(), col.data_ptr(), val.data_ptr(),
                         types.data_ptr(), sigma.data_ptr(), mean, std, rabs, o["div_table" + tag].data_ptr(),
                         f("norm" + tag), f("norm" + tag + "_std"), s)
    torch.cuda.synchronize()
    return o


@functools.lru_cache(maxsize=None)
def run_case(name, strategy, fields=True):
    c = case(name)
    p = c.plan
    return launch(p.n_graphs, p.ptr, c.d_gt, c.d_pred, c.d_types, p.a_rowptr, p.a_col, p.a_val, c.mean, c.std,
                  strategy, fields)


TABLES = ("nmse_table", "div_table", "div_table_fem")
FIELDS = ("err_field", "vm_gt", "vm_pred", "norm", "norm_std", "norm_fem", "norm_fem_std")


def bits(t):
    """A tensor's bit pattern (NaNs compare equal to themselves)."""
    t = t.contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32).cpu()


def check_table(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, got, ref)
    assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), (what, got, ref)   # +-inf
    err = np.abs(got[fin] - ref[fin])
    print(f"{what}: max rel err {float((err / np.maximum(np.abs(ref[fin]), 1e-300)).max()) if fin.any() else 0:.3e}")
    assert np.all(err <= 1e-10 * np.abs(ref[fin])), (what, got, ref)


def check_field(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref, np.float64)
    assert got.dtype == np.float32 and got.shape == ref.shape, what
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    assert np.array_equal(got[~fin & ~np.isnan(ref)].astype(np.float64), ref[~fin & ~np.isnan(ref)]), what
    err = np.abs(got[fin].astype(np.float64) - ref[fin])
    assert np.all(err <= 2.0 ** -23 * np.abs(ref[fin]) + 1e-30), (what, float(err.max()))


def check_against_reference(c: Case, o, strategy):
    ref = c.reference(strategy)
    for g, r in enumerate(ref):
        n0, n1 = int(c.ptr[g]), int(c.ptr[g + 1])
        for k in TABLES:
            check_table(o[k][g].cpu().numpy(), r[k], f"graph {g} (n={n1 - n0}) {k} {strategy}")
        for k in FIELDS:
            check_field(o[k][n0:n1].cpu().numpy(), r[k], f"graph {g} (n={n1 - n0}) {k}")
    N = int(c.ptr[-1])
    for k in FIELDS:   # nothing past row N
        assert torch.isnan(o[k][N:]).all() and o[k][N:].shape[0] == GUARD, k


# ------------------------------------------------------------------------------ gates
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_fixture(strategy):
    """Every value the reference's functions gave, the three cases scored in one batch."""
    with np.load(FIXTURE, allow_pickle=False) as f:
        gold = {k: f[k] for k in f.files}
    g = [{k[len(n) + 1:]: v for k, v in gold.items() if k.startswith(n + "_")} for n in GOLDEN]
    i = STRATEGIES.index(strategy)
    for gi in g:   # one standardisation per call: the fixture's cases are scored one call each, then batched
        c = Case([(gi["gt"], gi["pred"], gi["labels"], gi["op_rows"], gi["op_cols"], gi["op_vals"])],
                 gi["mean"], gi["std"])
        assert c.dropped == 0
        p = c.plan
        o = launch(1, p.ptr, c.d_gt, c.d_pred, c.d_types, p.a_rowptr, p.a_col, p.a_val, c.mean, c.std, strategy)
        check_table(o["nmse_table"][0].cpu().numpy(), [*gi["nmse_c"], gi["nmse"], gi["nmse_vm"], gi["r2"]], "nmse")
        check_table(o["nmse_table"][0].cpu().numpy(), [*gi["nmse_c_std"], gi["nmse_std"], gi["nmse_vm"], gi["r2_std"]],
                    "nmse against the standardised reference")
        check_table(o["div_table"][0].cpu().numpy(), gi["div"][i], "div")
        check_table(o["div_table_fem"][0].cpu().numpy(), gi["div_fem"][i], "div_fem")
        n = len(gi["gt"])
        check_field(o["err_field"][:n].cpu().numpy(), gi["err_field"], "err_field")
        check_field(o["vm_gt"][:n].cpu().numpy(), gi["vm_gt"], "vm_gt")
        check_field(o["vm_pred"][:n].cpu().numpy(), gi["vm_pred"], "vm_pred")
        for tag in ("", "_fem"):
            check_field(o["norm" + tag][:n].cpu().numpy(), gi["norm" + tag][0], "norm" + tag)
            check_field(o["norm" + tag + "_std"][:n].cpu().numpy(), gi["norm" + tag][1], "norm_std" + tag)
        for k in FIELDS:
            assert torch.isnan(o[k][n:]).all()
    # the three in one batch (one mean / std for all: the first case's) against the yardstick
    c = Case([(x["gt"], x["pred"], x["labels"], x["op_rows"], x["op_cols"], x["op_vals"]) for x in g],
             g[0]["mean"], g[0]["std"])
    p = c.plan
    o = launch(3, p.ptr, c.d_gt, c.d_pred, c.d_types, p.a_rowptr, p.a_col, p.a_val, c.mean, c.std, strategy)
    check_against_reference(c, o, strategy)
    for j, gi in enumerate(g):
        check_table(o["nmse_table"][j].cpu().numpy(), [*gi["nmse_c"], gi["nmse"], gi["nmse_vm"], gi["r2"]], "nmse")
        check_table(o["div_table"][j, 0].cpu().numpy(), gi["div"][i][0], "div raw")


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("name", ["shapes", "big", "p1"])
def test_shapes_against_the_yardstick(name, strategy):
    c = case(name)
    assert name != "shapes" or (tuple(c.counts) == COUNTS and c.dropped > 0)
    assert (c.labels == 1).any() and (c.labels == -1).any()
    assert (np.diff(c.a_rowptr) == 0).any() and (np.diff(c.a_rowptr) >= 200).any() or name == "p1"
    o = run_case(name, strategy)
    check_against_reference(c, o, strategy)
    if name == "shapes":
        e = COUNTS.index(0)
        for k in TABLES:
            assert torch.isnan(o[k][e]).all(), k
        # a single node: zero denominators give numpy's infinities
        assert torch.isinf(o["nmse_table"][0, :5]).all() and o["nmse_table"][0, 5] == float("-inf")


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_each_graph_scores_the_same_alone_and_determinism(strategy):
    c = case("shapes")
    o = run_case("shapes", strategy)
    p = c.plan
    again = launch(p.n_graphs, p.ptr, c.d_gt, c.d_pred, c.d_types, p.a_rowptr, p.a_col, p.a_val, c.mean, c.std,
                   strategy)
    for k in TABLES + FIELDS:
        assert torch.equal(bits(again[k]), bits(o[k])), k
    for g, n in enumerate(c.counts):
        if n == 0:
            continue
        n0, n1 = int(c.ptr[g]), int(c.ptr[g + 1])
        e0, e1 = int(c.a_rowptr[n0]), int(c.a_rowptr[n1])
        ptr = torch.tensor([0, n], dtype=torch.int32, device=dev())
        rp = (p.a_rowptr[n0:n1 + 1] - e0).contiguous()
        alone = launch(1, ptr, c.d_gt[n0:n1].contiguous(), c.d_pred[n0:n1].contiguous(), c.d_types[n0:n1].contiguous(),
                       rp, p.a_col[e0:e1].contiguous(), p.a_val[e0:e1].contiguous(), c.mean, c.std, strategy)
        for k in TABLES:
            assert torch.equal(bits(alone[k][0]), bits(o[k][g])), (g, n, k)
        for k in FIELDS:
            assert torch.equal(bits(alone[k][:n]), bits(o[k][n0:n1])), (g, n, k)
            assert torch.isnan(alone[k][n:]).all()


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_null_optional_outputs_give_the_same_tables(strategy):
    for name in ("shapes", "p1"):
        a, b = run_case(name, strategy), run_case(name, strategy, False)
        for k in TABLES:
            assert torch.equal(bits(a[k]), bits(b[k])), (name, k)
        assert all(b[k] is None for k in FIELDS)


def sparse_op(c: Case, g):
    rp, col, val = c.graph_csr(g)
    n = c.counts[g]
    row = np.repeat(np.arange(n), np.diff(rp))
    return torch.sparse_coo_tensor(torch.from_numpy(np.stack([row, col])), torch.from_numpy(val), (n, 2 * n))


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_consistent_with_the_training_losses(strategy):
    """The shipped fp32 losses on the same graph: 1e-5 relative."""
    from gnn_local_stress import losses
    for name, graphs in (("p1", (0, 1)), ("shapes", (4, 7, 9))):
        c, o = case(name), run_case(name, strategy)
        for g in graphs:
            n0, n1 = int(c.ptr[g]), int(c.ptr[g + 1])
            div = float(losses.compute_divergence(c.d_pred[n0:n1].contiguous(), sparse_op(c, g),
                                                  c.d_types[n0:n1].contiguous(), strategy))
            nmse = float(losses.normalized_mse_loss_single(c.d_gt[n0:n1].contiguous(), c.d_pred[n0:n1].contiguous()))
            got_div = float(o["div_table"][g, 0].float())
            got_nmse = float(o["nmse_table"][g, 3].float())
            print(f"{name} graph {g}: div {got_div} loss {div}; nmse {got_nmse} loss {nmse}")
            assert abs(got_div - div) <= 1e-5 * abs(div), (name, g, got_div, div)
            assert abs(got_nmse - nmse) <= 1e-5 * abs(nmse), (name, g, got_nmse, nmse)


def test_norm_masks_only_the_external_boundary():
    c, o = case("p1"), run_case("p1", "square")
    N = int(c.ptr[-1])
    ext, inn = torch.from_numpy(c.labels == 1), torch.from_numpy(c.labels == -1)
    assert int(inn.sum()) > 10 and int(ext.sum()) > 10
    for k in ("norm", "norm_std", "norm_fem", "norm_fem_std"):
        f = o[k][:N].cpu()
        assert (f[ext] == 0).all() and (f[inn] > 0).all(), k


# ------------------------------------------------------------------------------ public API
def api_batch(with_operator=True):
    from pdg import graph, meshgen
    samples = [meshgen.hole_plate(11, hole_radius=0.25, seed=21), meshgen.hole_plate(9, seed=22),
               meshgen.hole_plate(13, hole_radius=0.2, seed=23)]
    datas = [graph.sample_to_data(s) for s in samples]
    if not with_operator:
        for d in datas:
            del d.__dict__["op_div_matrix"]
    batch = graph.Batch.from_data_list(datas).to(dev())
    g = torch.Generator().manual_seed(3)
    pred = (batch.local_stress.cpu() + 4.0 * torch.randn(batch.local_stress.shape, generator=g)).to(dev())
    return samples, batch, pred


def test_batch_metrics_and_the_single_graph_functions():
    from gnn_local_stress import metrics
    samples, batch, pred = api_batch()
    gt = batch.local_stress
    for strategy in STRATEGIES:
        m = metrics.batch_metrics(pred, gt, batch, MEAN, STD, strategy, fields=True)
        lean = metrics.batch_metrics(pred, gt, batch, MEAN, STD, strategy)
        assert set(lean) == set(metrics.NMSE_COLUMNS + metrics.DIV_COLUMNS)
        assert set(m) == set(lean) | {"nmse_field", "von_mises_gt", "von_mises_pred", "div_norm", "div_norm_standard",
                                      "div_norm_fem", "div_norm_fem_standard"}
        for k in lean:
            assert lean[k].dtype == torch.float64 and lean[k].shape == (3,)
            assert torch.equal(bits(lean[k]), bits(m[k])), k
        ptr = batch.ptr.cpu().numpy()
        for g, s in enumerate(samples):
            n0, n1 = int(ptr[g]), int(ptr[g + 1])
            csr = R.coo_to_csr(s.num_nodes, s.op_div_rows, s.op_div_cols, s.op_div_vals)
            r = R.graph_metrics(gt[n0:n1].cpu().numpy(), pred[n0:n1].cpu().numpy(), csr, s.node_types, MEAN, STD,
                                strategy)
            check_table([float(m[k][g]) for k in metrics.NMSE_COLUMNS], r["nmse_table"], "api nmse")
            check_table([float(m[k][g]) for k in metrics.DIV_COLUMNS], [*r["div_table"], *r["div_table_fem"]], "api div")
            check_field(m["nmse_field"][n0:n1].cpu().numpy(), r["err_field"], "api err")
            check_field(m["div_norm_fem_standard"][n0:n1].cpu().numpy(), r["norm_fem_std"], "api norm")
    # the script's single-graph functions on graph 1
    n0, n1 = int(ptr[1]), int(ptr[2])
    g1, p1 = gt[n0:n1].contiguous(), pred[n0:n1].contiguous()
    one = metrics.normalized_mse_loss_single(g1, p1)
    assert one.dtype == torch.float64 and torch.equal(bits(one), bits(m["nmse"][1]))
    three = metrics.normalized_mse_loss_single(g1, p1, reduce=False)
    assert torch.equal(bits(three), bits(torch.stack([m[k][1] for k in ("nmse_xx", "nmse_yy", "nmse_xy")])))
    assert torch.equal(bits(metrics.normalized_mse_loss_element_wise(g1, p1)), bits(m["nmse_field"][n0:n1, :3]))
    assert torch.equal(bits(metrics.von_mises_stress(p1[:, 0], p1[:, 1], p1[:, 2])), bits(m["von_mises_pred"][n0:n1]))
    norm = metrics.compute_divergence_norm_field(p1, batch[1].op_div_matrix, batch.nodes_types[n0:n1])
    assert torch.equal(bits(norm), bits(m["div_norm"][n0:n1]))


def test_batch_without_operator_cpu_tensors_and_bad_strategy():
    from gnn_local_stress import metrics
    _, batch, pred = api_batch(with_operator=False)
    m = metrics.batch_metrics(pred, batch.local_stress, batch, MEAN, STD, fields=True)
    assert set(m) == set(metrics.NMSE_COLUMNS) | {"nmse_field", "von_mises_gt", "von_mises_pred"}
    _, full, _ = api_batch()
    ref = metrics.batch_metrics(pred, full.local_stress, full, MEAN, STD)
    for k in metrics.NMSE_COLUMNS:
        assert torch.equal(bits(m[k]), bits(ref[k])), k
    with pytest.raises(RuntimeError, match="HIP metrics need tensors on a HIP device"):
        metrics.batch_metrics(pred.cpu(), full.local_stress, full, MEAN, STD)
    with pytest.raises(RuntimeError, match="HIP"):
        metrics.batch_metrics(pred, full.local_stress.cpu(), full, MEAN, STD)
    with pytest.raises(RuntimeError, match="HIP"):
        metrics.normalized_mse_loss_single(pred.cpu(), pred.cpu())
    with pytest.raises(AttributeError, match="reduce_strategy"):
        metrics.batch_metrics(pred, full.local_stress, full, MEAN, STD, reduce_strategy="raw")


def test_evaluate_inference_end_to_end(tmp_path):
    import pandas as pd
    from gnn_local_stress import metrics, vtk_io
    samples, batch, pred = api_batch()
    ptr = batch.ptr.cpu().numpy()
    gt_dir, inf_dir = tmp_path / "gt", tmp_path / "inference"
    (inf_dir / "fields").mkdir(parents=True)
    gt_dir.mkdir()
    meshes, datas, outs = [], [], []
    for i, s in enumerate(samples):
        mesh, data = gt_dir / f"hole_plate_mesh_{i}.vtk", gt_dir / f"hole_plate_mesh_{i}.npz"
        vtk_io.write_legacy_vtk(mesh, s.pos, s.faces, point_type="float")
        arrays = dict(stress_field=s.local_stress, mean_stress=s.mean_stress.astype(np.float64),
                      op_div_matrix_data=s.op_div_vals, op_div_matrix_col_indices=s.op_div_cols.astype(np.int32),
                      op_div_matrix_row_indices=s.op_div_rows.astype(np.int32),
                      op_div_matrix_shape=np.array([s.num_nodes, 2 * s.num_nodes]), node_labels=s.node_types)
        np.savez(data, **arrays)
        arrays["stress_field"] = pred[int(ptr[i]):int(ptr[i + 1])].cpu().numpy()
        out = inf_dir / "fields" / f"hole_plate_mesh_{i}.npz"
        np.savez(out, **arrays)
        meshes.append(mesh.as_posix()), datas.append(data.as_posix()), outs.append(out.as_posix())
    pd.DataFrame({"mesh_filename": meshes, "data_filename": datas}).to_csv(gt_dir / "dataset.csv", index=False)
    pd.DataFrame({"mesh_filename": meshes, "data_filename": outs}).to_csv(inf_dir / "dataset.csv", index=False)
    (inf_dir / "normalize_params.json").write_text(json.dumps({"mean_local_stress": MEAN, "std_local_stress": STD}))

    gt = batch.local_stress
    want = metrics.batch_metrics(pred, gt, batch, MEAN, STD, "abs")
    summary = metrics.evaluate_inference(gt_dir / "dataset.csv", inf_dir, dev(), batch_size=2, reduce_strategy="abs")
    table = pd.read_csv(inf_dir / "metrics.csv", index_col="sample", float_precision="round_trip")
    assert list(table.columns) == list(metrics.NMSE_COLUMNS + metrics.DIV_COLUMNS) and list(table.index) == [0, 1, 2]
    for k in table.columns:
        assert np.array_equal(table[k].to_numpy(), want[k].cpu().numpy()), k
    assert summary == json.loads((inf_dir / "summary.json").read_text())
    nmse = want["nmse"].cpu().numpy()
    assert summary["samples"] == 3 and summary["mean_nmse"] == float(nmse.mean())
    assert summary["best_nmse_indices"] == [int(i) for i in np.argsort(nmse)]
    assert summary["worst_nmse_indices"] == [int(i) for i in np.argsort(nmse)[::-1]]
    assert summary["mean_div_standard"] == float(want["div_standard"].cpu().numpy().mean())
    assert summary["mean_div_fem_standard"] == float(want["div_fem_standard"].cpu().numpy().mean())
    assert summary["div_standard_below_fem"] == int((want["div_standard"] < want["div_fem_standard"]).sum())

    # the script's swapped roles: the NMSE call with the two fields exchanged, the divergences as before
    metrics.evaluate_inference(gt_dir / "dataset.csv", inf_dir, dev(), batch_size=3, reduce_strategy="abs",
                               swap_like_reference=True)
    swapped = pd.read_csv(inf_dir / "metrics.csv", index_col="sample", float_precision="round_trip")
    exchanged = metrics.batch_metrics(gt, pred, batch, MEAN, STD, "abs")
    for k in metrics.NMSE_COLUMNS:
        assert np.array_equal(swapped[k].to_numpy(), exchanged[k].cpu().numpy()), k
        assert not np.array_equal(swapped[k].to_numpy(), table[k].to_numpy()), k
    for k in metrics.DIV_COLUMNS:
        assert np.array_equal(swapped[k].to_numpy(), table[k].to_numpy()), k
