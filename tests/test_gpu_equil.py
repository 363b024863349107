"""pdg_equilibrate and gnn_local_stress.equilibrate on the device against tests/equil_ref.py.

Meshes: triangles n = 9 with a hole of 0.25 (72 nodes: most of the 1024 threads own no row), triangles n = 17 and
quads n = 17 with a hole of 0.2 (252 nodes each; the quad operator has cond(S) ~ 670 against ~ 23).  Field:
``local_stress`` plus 5 % seeded noise.  Weights: the nodal areas and None.  rtol = 1e-4.

Every bound is derived, none measured:

* the kernel's status bit 2 is its own definition of "the true residual exceeds 2 rtol |C in|"; the host recomputes
  that ratio in fp64 from the returned fp32 field and holds it to 2 rtol;
* the reported and the host ratio are fp64 sums of the same fp32 data in different orders: they differ by ~1e-12 of
  |sigma| against a residual of ~1e-4 of the initial one, far inside the 1 % asked;
* accuracy: sigma' - sigma* = u + n with u in range(W^-1 C^T) and n in null(C).  C u = C sigma' (the true residual
  rho), so |u|_W^2 = rho^T S^+ rho <= |rho|^2 / lambda_min, and |sigma - sigma*|_W^2 = b^T S^+ b >= |b|^2 /
  lambda_max with b = C sigma: |u|_W <= sqrt(cond(S)) (|rho| / |b|) |sigma - sigma*|_W.  n is the projection of
  the roundings of forming and storing sigma' (one fp32 rounding of an fp64 value, 2^-24 |sigma'| an element),
  which the residual does not see: 8 x 2^-24 |sigma|_W covers it.  The transpose is the same statement for
  x = W^-1 g, since P^T = W P W^-1;
* adjointness: |<P x, g> - <x, P^T g>| <= |P x - P* x|_W |g|_W^-1 + |x|_W |P^T g - P*^T g|_W^-1, the two bounds
  above times the other side's norm (<P* x, g> = <x, P*^T g> exactly).
"""
import numpy as np
import pytest
import torch

import equil_ref as R
import homog_ref as H

pytestmark = pytest.mark.gpu

RTOL = 1e-4
NAMES = ("tri9", "tri17", "quad17")
U = 2.0 ** -53


def _data(name, sigma=None, node_types=None):
    """The mesh as a Data with its operator, the host's nodal areas and cell area, and `sigma` as local_stress."""
    from pdg import graph
    s = R.mesh(name)
    d = graph.sample_to_data(s)
    w, cell = R.areas(s)
    d.node_area = torch.from_numpy(w)
    d.cell_area = torch.tensor([cell], dtype=torch.float64)
    if sigma is not None:
        d.local_stress = torch.from_numpy(np.ascontiguousarray(sigma))
    if node_types is not None:
        t = torch.from_numpy(np.asarray(node_types, np.int64)).reshape(-1, 1)
        d.nodes_types, d.surfaces_nodes_for_div = t, t
    return d


def _batch(datas):
    from pdg import graph
    return graph.Batch.from_data_list(datas).to("cuda")


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


class Case:
    """The three meshes in one batch of unequal sizes; per mesh the field, the areas, the operator and the dense
    fp64 projections for both metrics, computed once."""

    def __init__(self):
        self.samples = [R.mesh(k) for k in NAMES]
        self.sigma = [R.noisy_field(s, seed=11 + i) for i, s in enumerate(self.samples)]
        self.w = [R.areas(s)[0] for s in self.samples]
        self.cell = [R.areas(s)[1] for s in self.samples]
        self.op = [R.Operator.of(s) for s in self.samples]
        self.dense = {"area": [R.Dense(o, w) for o, w in zip(self.op, self.w)], None: [R.Dense(o) for o in self.op]}
        self.cond = {k: [d.cond() for d in v] for k, v in self.dense.items()}
        rng = np.random.default_rng(5)
        self.g = [rng.standard_normal(s.shape).astype(np.float32) for s in self.sigma]
        self.ptr = np.concatenate([[0], np.cumsum([s.num_nodes for s in self.samples])])
        assert len(set(np.diff(self.ptr))) > 1
        self.batch = _batch([_data(k, s) for k, s in zip(NAMES, self.sigma)])
        self.d_sigma = self.batch.local_stress
        self.d_g = torch.from_numpy(np.concatenate(self.g)).cuda()

    def weights(self, key, i):
        return self.w[i] if key == "area" else None

    def rows(self, t, i):
        return t[int(self.ptr[i]):int(self.ptr[i + 1])]


@pytest.fixture(scope="module")
def case():
    return Case()


@pytest.fixture(scope="module")
def solved(case):
    """weights -> (sigma' and table of equilibrate, P^T g and table of equilibrate_grad), one batch call each."""
    from gnn_local_stress import equilibrate as E
    out = {}
    for key in ("area", None):
        fwd = E.equilibrate(case.d_sigma, case.batch, key, rtol=RTOL, return_info=True)
        bwd = E.equilibrate_grad(case.d_g, case.batch, key, rtol=RTOL, return_info=True)
        torch.cuda.synchronize()
        out[key] = tuple((o.cpu().numpy(), t.cpu().numpy()) for o, t in (fwd, bwd))
    return out


def _forward_bound(case, key, i, out):
    """(|out - sigma*|_W, its bound, the host's residual ratio) of graph i."""
    op, d, w = case.op[i], case.dense[key][i], case.weights(key, i)
    sigma = case.sigma[i]
    star = d.project(sigma)
    ratio = op.defect(out) / op.defect(sigma)
    bound = np.sqrt(case.cond[key][i]) * ratio * R.wnorm(sigma - star, w) + 8 * 2.0 ** -24 * R.wnorm(sigma, w)
    return R.wnorm(out - star, w), bound, ratio


def _transpose_bound(case, key, i, out):
    """The same for P^T g in the W^-1 norm: (|W^-1 (out - P*^T g)|_W, its bound, the host's ratio)."""
    op, d, w = case.op[i], case.dense[key][i], case.weights(key, i)
    g = case.g[i]
    iw = 1.0 / d.W.reshape(-1, 3)
    want = d.project_t(g)
    ratio = op.defect(out * iw) / op.defect(g * iw)
    bound = (np.sqrt(case.cond[key][i]) * ratio * R.wnorm((g - want) * iw, w)
             + 8 * 2.0 ** -24 * R.wnorm(g * iw, w))
    return R.wnorm((out - want) * iw, w), bound, ratio


@pytest.mark.parametrize("key", ["area", None])
def test_converges_and_reports_its_true_residual(case, solved, key):
    (out, table), (out_t, table_t) = solved[key]
    assert table.shape == (3, 4) and out.dtype == np.float32 and out.shape == (case.ptr[-1], 3)
    for i, name in enumerate(NAMES):
        op, iw = case.op[i], 1.0 / case.dense[key][i].W.reshape(-1, 3)
        for what, tb, o, x, pre in (("P", table, out, case.sigma[i], 1.0), ("P^T", table_t, out_t, case.g[i], iw)):
            b, res, it, status = tb[i]
            o = case.rows(o, i).astype(np.float64)
            host_b, host_res = op.defect(x * pre), op.defect(o * pre)
            print(f"{name} weights={key} {what}: {int(it)} iterations, |b| {b:.6e} (host {host_b:.6e}), reported "
                  f"ratio {res / b:.4e}, host ratio {host_res / host_b:.4e}, status {int(status)}")
            assert status == 0 and 0 < it <= 1000
            assert host_res / host_b <= 2 * RTOL
            assert abs(res / b - host_res / host_b) <= 0.01 * (host_res / host_b)
            assert abs(b - host_b) <= 1e-9 * host_b


@pytest.mark.parametrize("key", ["area", None])
def test_against_the_fp64_projection(case, solved, key):
    (out, _), (out_t, _) = solved[key]
    for i, name in enumerate(NAMES):
        err, bound, ratio = _forward_bound(case, key, i, case.rows(out, i).astype(np.float64))
        print(f"{name} weights={key}: cond(S) {case.cond[key][i]:.1f}, ratio {ratio:.3e}, |s' - s*|_W / bound "
              f"{err / bound:.3e}")
        assert err <= bound
        err, bound, ratio = _transpose_bound(case, key, i, case.rows(out_t, i).astype(np.float64))
        print(f"{name} weights={key} transpose: ratio {ratio:.3e}, err / bound {err / bound:.3e}")
        assert err <= bound


@pytest.mark.parametrize("key", ["area", None])
def test_transpose_is_the_adjoint(case, solved, key):
    (out, _), (out_t, _) = solved[key]
    for i, name in enumerate(NAMES):
        w, d = case.weights(key, i), case.dense[key][i]
        iw = 1.0 / d.W.reshape(-1, 3)
        px, ptg = case.rows(out, i).astype(np.float64), case.rows(out_t, i).astype(np.float64)
        x, g = case.sigma[i].astype(np.float64), case.g[i].astype(np.float64)
        lhs, rhs = float(np.sum(px * g)), float(np.sum(x * ptg))
        _, bound_p, _ = _forward_bound(case, key, i, px)
        _, bound_t, _ = _transpose_bound(case, key, i, ptg)
        tol = bound_p * R.wnorm(g * iw, w) + bound_t * R.wnorm(x, w)
        print(f"{name} weights={key}: <P x, g> {lhs:.9e}, <x, P^T g> {rhs:.9e}, |difference| / tol "
              f"{abs(lhs - rhs) / tol:.3e}")
        assert abs(lhs - rhs) <= tol


def test_a_graph_alone_gets_its_batch_rows_bitwise(case):
    from gnn_local_stress import equilibrate as E
    for key in ("area", None):
        for fn, x in ((E.equilibrate, case.d_sigma), (E.equilibrate_grad, case.d_g)):
            out, table = fn(x, case.batch, key, rtol=RTOL, return_info=True)
            again, table2 = fn(x, case.batch, key, rtol=RTOL, return_info=True)
            assert torch.equal(_bits(out), _bits(again)) and torch.equal(_bits(table), _bits(table2))
            for i, name in enumerate(NAMES):
                xi = case.rows(x, i).contiguous()
                alone, t1 = fn(xi, _batch([_data(name)]), key, rtol=RTOL, return_info=True)
                assert torch.equal(_bits(alone), _bits(case.rows(out, i))), (name, key)
                assert torch.equal(_bits(t1[0]), _bits(table[i])), (name, key)


def test_graphs_with_nothing_to_remove_and_bad_weights(case):
    from gnn_local_stress import equilibrate as E
    s9, s17 = case.sigma[0], case.sigma[1]
    n9 = len(s9)
    normal, t_normal = E.equilibrate(case.rows(case.d_sigma, 1).contiguous(), _batch([_data("tri17")]), "area",
                                     rtol=RTOL, return_info=True)
    # no interior node | a zero field | the normal graph
    b = _batch([_data("tri9", s9, np.ones(n9)), _data("tri9", np.zeros_like(s9)), _data("tri17", s17)])
    out, table = E.equilibrate(b.local_stress, b, "area", rtol=RTOL, return_info=True)
    assert torch.equal(_bits(out[:2 * n9]), _bits(b.local_stress[:2 * n9]))
    assert table[:2].cpu().tolist() == [[0.0, 0.0, 0.0, 0.0]] * 2
    assert torch.equal(_bits(out[2 * n9:]), _bits(normal)) and torch.equal(_bits(table[2]), _bits(t_normal[0]))
    assert float(E.divergence_defect(b.local_stress, b)[0]) == 0.0
    # max_iter = 0: the field as it is, the defect reported and flagged
    out, table = E.equilibrate(case.d_sigma, case.batch, "area", rtol=RTOL, max_iter=0, return_info=True)
    assert torch.equal(_bits(out), _bits(case.d_sigma))
    t = table.cpu().numpy()
    defect = E.divergence_defect(case.d_sigma, case.batch).cpu().numpy()
    for i in range(3):
        want = case.op[i].defect(case.sigma[i])
        assert t[i, 2] == 0 and int(t[i, 3]) & E.NOT_CONVERGED and not int(t[i, 3]) & E.BAD_WEIGHT
        assert abs(t[i, 0] - want) <= 1e-9 * want and t[i, 1] == t[i, 0] and defect[i] == t[i, 0]
    # one zero weight (and a NaN, a negative and an infinite one): bit 4, the rows as they were, the neighbour as ever
    b = _batch([_data("tri9", s9), _data("tri17", s17)])
    for bad in (0.0, float("nan"), -1.0, float("inf")):
        w = b.node_area.clone()
        w[5] = bad
        out, table = E.equilibrate(b.local_stress, b, w, rtol=RTOL, return_info=True)
        assert int(table[0, 3]) == E.BAD_WEIGHT and float(table[0, 2]) == 0.0, bad
        assert torch.equal(_bits(out[:n9]), _bits(b.local_stress[:n9])), bad
        assert torch.equal(_bits(out[n9:]), _bits(normal)) and torch.equal(_bits(table[1]), _bits(t_normal[0])), bad


def test_an_empty_graph_gets_a_nan_row(case):
    """A ptr with an empty segment between two graphs, through the C ABI (a Batch cannot hold an empty graph)."""
    from pdg.lib import lib, stream_handle
    from pdg.plan import plan_for
    plan = plan_for(case.batch)
    n = int(case.ptr[-1])
    ptr = torch.tensor([0, case.ptr[1], case.ptr[1], case.ptr[2], n], dtype=torch.int32, device="cuda")
    types = case.batch.nodes_types.reshape(-1).contiguous()
    nbytes = lib.pdg_equilibrate_scratch_bytes(n, 4)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.full_like(case.d_sigma, -7.0)
    table = torch.full((4, 4), -7.0, dtype=torch.float64, device="cuda")
    args = [t.data_ptr() for t in (plan.a_rowptr, plan.a_col, plan.a_val, plan.at_rowptr, plan.at_row, plan.at_comp,
                                   plan.at_val, types, case.batch.node_area, case.d_sigma)]
    lib.pdg_equilibrate(4, ptr.data_ptr(), n, *args, 0, RTOL, 1000, out.data_ptr(), table.data_ptr(),
                        scratch.data_ptr(), nbytes, stream_handle(out.device))
    from gnn_local_stress import equilibrate as E
    want, t_want = E.equilibrate(case.d_sigma, case.batch, "area", rtol=RTOL, return_info=True)
    assert torch.isnan(table[1]).all()
    assert torch.equal(_bits(out), _bits(want)) and torch.equal(_bits(table[[0, 2, 3]]), _bits(t_want))


def test_mean_after_the_projection(case):
    from gnn_local_stress import equilibrate as E, homogenise
    plain = E.equilibrate(case.d_sigma, case.batch, "area", rtol=RTOL)
    out, table = E.equilibrate(case.d_sigma, case.batch, "area", rtol=RTOL, mean="cell", return_info=True)
    assert torch.equal(_bits(out), _bits(homogenise.enforce_mean(plain, case.batch, convention="cell")))
    d = homogenise.mean_defect(out, case.batch, convention="cell").cpu().numpy()
    plain, out = plain.cpu().numpy(), out.cpu().numpy()
    for i, name in enumerate(NAMES):
        s, w, D, op = case.samples[i], case.w[i], case.cell[i], case.op[i]
        ptr = np.array([0, s.num_nodes])
        before, after = case.rows(plain, i), case.rows(out, i)
        # tests/test_gpu_homog.py's tolerance for enforce_mean
        _, mag1 = H.graph_wmean(ptr, before, w)
        _, mag2 = H.graph_wmean(ptr, after, w)
        t = s.mean_stress.astype(np.float64)
        n = float(s.num_nodes)
        tol = 2.0 ** -24 * mag2[0, 1:] / D + 2.0 * (n + 3.0) * U * (mag1[0, 1:] / D + mag2[0, 1:] / D + np.abs(t))
        assert np.all(np.abs(d[i]) <= tol), name
        # the divergence: 2 rtol from the projection plus what the constant shift adds, |C shift| / |C sigma|
        shift = (case.dense["area"][i].mean_shift(before, t, D) - before)[0]
        extra = op.defect(np.tile(shift, (s.num_nodes, 1))) / op.defect(case.sigma[i])
        ratio = op.defect(after) / op.defect(case.sigma[i])
        print(f"{name}: mean defect / tol {np.max(np.abs(d[i]) / tol):.3e}, shift {shift}, divergence ratio "
              f"{ratio:.3e} (constant-shift term {extra:.3e})")
        assert ratio <= 2 * RTOL + extra


def test_the_call_replays_from_a_captured_graph(case):
    from gnn_local_stress import equilibrate as E
    other = torch.from_numpy(np.concatenate([R.noisy_field(s, seed=40 + i) for i, s in enumerate(case.samples)])).cuda()
    eager, t_eager = E.equilibrate(other, case.batch, "area", rtol=RTOL, return_info=True)
    static_in = case.d_sigma.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, table = E.equilibrate(static_in, case.batch, "area", rtol=RTOL, return_info=True)
    static_in.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(eager)) and torch.equal(_bits(table), _bits(t_eager))


def test_python_layer_refusals_on_the_device(case):
    from gnn_local_stress import equilibrate as E
    from pdg import graph
    d, b = case.d_sigma, case.batch
    bare = graph.Batch.from_data_list([graph.sample_to_data(s) for s in case.samples]).to("cuda")
    with pytest.raises(ValueError, match="mesh_fields=True"):
        E.equilibrate(d, bare)
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        E.equilibrate(d[:, :2], b, None)
    with pytest.raises(ValueError, match="'area', None or a tensor"):
        E.equilibrate(d, b, "volume")
    with pytest.raises(RuntimeError, match="autograd"):
        E.equilibrate(d.clone().requires_grad_(True), b, None)
    with pytest.raises(ValueError, match="rtol"):
        E.equilibrate(d, b, None, rtol=0.0)
    with pytest.raises(ValueError, match="max_iter"):
        E.equilibrate(d, b, None, max_iter=-1)
    with pytest.raises(ValueError, match="divergence operator"):
        E.equilibrate(d, b.ptr, None)
    with pytest.raises(ValueError, match="rows"):
        E.equilibrate(d[:-1].contiguous(), b, None)
    with pytest.raises(ValueError, match="weights for"):
        E.equilibrate(d, b, b.node_area[:5])
