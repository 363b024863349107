"""The FEM cell solver on the device (gnn_local_stress/fem.py, csrc/pdg_fem.hip) against the independent fp64
restatement tests/fem_ref.py (scipy: assembled K, periodic reduction, one node pinned, sparse LU).

Meshes: pdg.meshgen.hole_plate(n, r, seed=3) with (n, r) = (9, 0.25) 72 nodes, (13, 0.3) 132, (17, 0.2) 252 and
(37, 0.2), which has more than 1024 nodes: the strided ownership and the ragged last pass.  The stress bound is
2^-22 max|sigma_ref| per graph and load case: the fp32 rounding of the output; the solver's own error at rtol = 1e-10
is ~ 6e-11 relative, 1000 x below it."""
import numpy as np
import pytest
import torch

import fem_ref as R
from pdg import meshgen

pytestmark = pytest.mark.gpu

MESHES = ((9, 0.25), (13, 0.3), (17, 0.2), (37, 0.2))
RTOL = 1e-10
BOUND = 2.0 ** -22


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _dev(s):
    return torch.from_numpy(s.pos).cuda(), torch.from_numpy(s.faces).cuda()


class Case:
    def __init__(self):
        from gnn_local_stress import fem
        self.samples = [meshgen.hole_plate(n, r, seed=3) for n, r in MESHES]
        self.cells = [R.cell(s.pos, s.faces) for s in self.samples]
        self.direct = [[R.solve_direct(c, e)[0] for e in R.UNIT] for c in self.cells]
        self.ref = [[R.fields(c, e, u) for e, u in zip(R.UNIT, us)] for c, us in zip(self.cells, self.direct)]
        self.pcg_its = [[R.pcg(c, e, rtol=RTOL)[1] for e in R.UNIT] for c in self.cells]
        self.mesh = [_dev(s) for s in self.samples]
        self.plans = [fem.FemPlan.from_mesh(p, f) for p, f in self.mesh]
        self.unit = torch.eye(3, dtype=torch.float64, device="cuda").reshape(1, 3, 3)
        self.solo = [fem.solve_cells(pl, p, self.unit, rtol=RTOL) for pl, (p, f) in zip(self.plans, self.mesh)]
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def case():
    return Case()


def test_plate_without_a_hole_is_trivial_and_exact():
    from gnn_local_stress import fem
    s = meshgen.hole_plate(9, 0.0, seed=3)
    pts, fcs = _dev(s)
    plan = fem.FemPlan.from_mesh(pts, fcs)
    out = fem.solve_cells(plan, pts, torch.eye(3, dtype=torch.float64, device="cuda").reshape(1, 3, 3), rtol=RTOL)
    table = out.table.cpu().numpy()[0]
    assert np.all(table[:, 3] == fem.TRIVIAL) and np.all(table[:, 0] == 0) and np.all(table[:, 2] == 0)
    assert not out.ut.cpu().numpy().any()
    c = R.stiffness()
    for l, eps in enumerate(R.UNIT):
        want = c @ eps
        err = np.abs(out.stress[l].cpu().numpy().astype(np.float64) - want).max() / np.abs(want).max()
        print(f"no hole, case {l}: |b| = {table[l, 1]:.3e}, nodal stress error {err:.3e} (bound {BOUND:.3e})")
        assert err <= BOUND
        assert np.abs(out.strain[l].cpu().numpy().astype(np.float64) - eps).max() <= BOUND
        assert np.abs(out.mean_stress[0, l].cpu().numpy() - want).max() <= 1e-12 * np.abs(want).max()


def test_plan_matches_the_restatement(case):
    for s, c, plan in zip(case.samples, case.cells, case.plans):
        assert np.array_equal(plan.rep.cpu().numpy(), c.rep)
        rp, item = plan.item_rowptr.cpu().numpy(), plan.item.cpu().numpy()
        key = c.rep[s.faces.ravel()]
        assert rp[0] == 0 and rp[-1] == 3 * len(s.faces) and np.array_equal(np.diff(rp), np.bincount(key, minlength=len(c.rep)))
        for v in range(len(c.rep)):
            row = item[rp[v]:rp[v + 1]]
            assert np.array_equal(row, np.where(key == v)[0])          # ascending, images' corners included
        assert np.array_equal(plan.rverts.cpu().numpy(), key)


def test_against_the_direct_solve(case):
    from gnn_local_stress import fem
    for i, ((n, r), c, out) in enumerate(zip(MESHES, case.cells, case.solo)):
        table = out.table.cpu().numpy()[0]
        stress = out.stress.cpu().numpy().astype(np.float64)
        ut = out.ut.cpu().numpy()
        for l, eps in enumerate(R.UNIT):
            ref = case.ref[i][l]
            err = np.abs(stress[l] - ref.stress).max() / np.abs(ref.stress).max()
            res = R.residual(c, eps, ut[l])
            print(f"n={n} r={r} case {l}: {int(table[l, 0])} iterations (numpy PCG {case.pcg_its[i][l]}), stress error "
                  f"{err:.3e} (bound {BOUND:.3e}), table residual {table[l, 2]:.3e}, recomputed {res:.3e}")
            assert table[l, 3] == fem.CONVERGED
            assert err <= BOUND
            assert table[l, 0] <= 2 * case.pcg_its[i][l]
            assert table[l, 2] <= RTOL
            assert res <= 2 * RTOL
            assert abs(table[l, 1] - np.linalg.norm(R.rhs(c, eps)[0])) <= 1e-9 * table[l, 1]
            assert np.abs(ut[l][c.reps].mean(0)).max() <= 1e-12 * np.abs(ut[l]).max()
            assert np.array_equal(ut[l], ut[l][c.rep])                 # an image holds its representative's row
            e_err = np.abs(out.strain[l].cpu().numpy() - ref.strain).max() / np.abs(ref.strain).max()
            assert e_err <= BOUND
            assert np.abs(out.mean_stress[0, l].cpu().numpy() - ref.mean_stress).max() <= 1e-9 * np.abs(ref.mean_stress).max()
            assert np.abs(out.mean_stress_material[0, l].cpu().numpy() - ref.mean_stress_material).max() \
                <= 1e-9 * np.abs(ref.mean_stress_material).max()
        assert abs(float(out.material_area[0]) - case.ref[i][0].material_area) <= 1e-12 * case.ref[i][0].material_area
        assert float(out.cell_area[0]) == case.ref[i][0].cell_area


def test_a_graph_is_bitwise_the_same_inside_a_batch(case):
    from gnn_local_stress import fem
    order = [0, 1, None, 2, 3]                       # an empty segment in the middle
    plans = [fem.FemPlan.empty("cuda") if i is None else case.plans[i] for i in order]
    plan = fem.FemPlan.collate(plans)
    pts = torch.cat([case.mesh[i][0] for i in order if i is not None])
    out = fem.solve_cells(plan, pts, case.unit.expand(len(order), 3, 3).contiguous(), rtol=RTOL)
    ptr = plan.ptr.cpu().numpy()
    assert plan.n_graphs == 5 and ptr[2] == ptr[3]
    for g, i in enumerate(order):
        if i is None:
            assert torch.isnan(out.table[g]).all() and torch.isnan(out.mean_stress[g]).all()
            continue
        solo, a, b = case.solo[i], int(ptr[g]), int(ptr[g + 1])
        assert torch.equal(_bits(out.table[g]), _bits(solo.table[0]))
        assert torch.equal(_bits(out.ut[:, a:b]), _bits(solo.ut))
        assert torch.equal(_bits(out.stress[:, a:b]), _bits(solo.stress))
        assert torch.equal(_bits(out.strain[:, a:b]), _bits(solo.strain))
        assert torch.equal(_bits(out.mean_stress[g]), _bits(solo.mean_stress[0]))
        assert torch.equal(_bits(out.mean_stress_material[g]), _bits(solo.mean_stress_material[0]))


def test_iteration_cap_returns_the_current_iterate(case):
    from gnn_local_stress import fem
    out = fem.solve_cells(case.plans[1], case.mesh[1][0], case.unit, rtol=RTOL, max_iter=5)
    table = out.table.cpu().numpy()[0]
    assert np.all(table[:, 3] == fem.MAX_ITER) and np.all(table[:, 0] == 5)
    assert np.all(np.isfinite(table)) and np.all(table[:, 2] > RTOL)
    assert torch.isfinite(out.stress).all() and torch.isfinite(out.ut).all()


def test_imposed_mean_stress_and_effective_stiffness(case):
    from gnn_local_stress import fem
    pts, fcs = case.mesh[1]
    target = np.array([120.0, -40.0, 25.0])
    sol = fem.solve_cell(pts, fcs, stress=target, rtol=RTOL)
    got = sol.mean_stress.cpu().numpy()
    print(f"imposed mean stress: relative miss {np.abs(got - target).max() / np.abs(target).max():.3e}")
    assert np.abs(got - target).max() <= 1e-9 * np.abs(target).max()
    ce = fem.effective_stiffness(pts, fcs, rtol=RTOL).cpu().numpy()
    ref = R.effective_stiffness(case.cells[1])
    print(f"C_eff: difference to fem_ref {np.abs(ce - ref).max() / np.abs(ref).max():.3e}, asymmetry "
          f"{np.abs(ce - ce.T).max() / np.abs(ce).max():.3e}")
    assert np.abs(ce - ref).max() <= 1e-9 * np.abs(ref).max()
    assert np.abs(ce - ce.T).max() <= 1e-9 * np.abs(ce).max()
    assert np.abs(sol.mean_strain.cpu().numpy() - np.linalg.solve(ref, target)).max() <= 1e-8 * np.abs(np.linalg.solve(ref, target)).max()
    # the field is the restatement's under that strain, and the localisation tensor gives the same field
    eps = sol.mean_strain.cpu().numpy()
    f = R.fields(case.cells[1], eps, R.solve_direct(case.cells[1], eps)[0])
    assert np.abs(sol.stress.cpu().numpy() - f.stress).max() <= BOUND * np.abs(f.stress).max()
    A = fem.localisation_tensor(pts, fcs, rtol=RTOL)
    assert A.shape == (case.samples[1].num_nodes, 3, 3) and A.dtype == torch.float32
    field = torch.einsum("nij,j->ni", A.double(), torch.from_numpy(target).cuda()).cpu().numpy()
    assert np.abs(field - f.stress).max() <= 4 * BOUND * np.abs(f.stress).max()     # 3 rounded terms + the sum


def test_unweighted_nodal_average(case):
    from gnn_local_stress import fem
    out = fem.solve_cells(case.plans[0], case.mesh[0][0], case.unit, rtol=RTOL, nodal="count")
    for l, eps in enumerate(R.UNIT):
        ref = R.fields(case.cells[0], eps, case.direct[0][l], "count")
        err = np.abs(out.stress[l].cpu().numpy() - ref.stress).max() / np.abs(ref.stress).max()
        assert err <= BOUND
        assert np.abs(ref.stress - case.ref[0][l].stress).max() > 100 * BOUND * np.abs(ref.stress).max()
    assert torch.equal(_bits(out.mean_stress), _bits(case.solo[0].mean_stress))


def test_degenerate_face_and_non_periodic_boundary_raise(case):
    from gnn_local_stress import fem
    s = case.samples[0]
    pts, fcs = case.mesh[0]
    flat = fcs.clone()
    flat[0, 2] = flat[0, 0]                                   # (a, b, a): det == 0 exactly
    with pytest.raises(ValueError, match="zero area"):
        fem.solve_cell(pts, flat, strain=(1e-3, 0.0, 0.0))
    bad = pts.clone()
    k = int(np.where(s.pos[:, 0] == s.pos[:, 0].max())[0][3])
    bad[k, 1] += 0.25
    with pytest.raises(ValueError, match="mesh is not periodic"):
        fem.FemPlan.from_mesh(bad, fcs)
    out = fcs.clone()
    out[1, 1] = s.num_nodes
    with pytest.raises(ValueError, match="outside"):
        fem.FemPlan.from_mesh(pts, out)
    with pytest.raises(ValueError, match="finite"):
        fem.solve_cell(pts, fcs, strain=(float("nan"), 0.0, 0.0))
    with pytest.raises(ValueError, match="out of scope"):
        fem.FemPlan.from_mesh(pts, torch.zeros(4, 4, dtype=torch.int64, device="cuda"))


def test_write_sample_round_trip_and_training_step(case, tmp_path):
    import pandas as pd
    from gnn_local_stress import datasets, fem, models
    from pdg import devgraph
    from pdg.collate import DeviceGraphStore
    from pdg.trainer import Trainer
    strains = ((1e-3, -5e-4, 2e-4), (-2e-4, 8e-4, 1e-3))
    for i, eps in enumerate(strains):
        row = fem.write_sample(tmp_path, i, *case.mesh[i], eps, rtol=RTOL, meta={"seed": 3, "hole_plate_radius": 25.0})
        assert tuple(row) == fem.CSV_COLUMNS
    df = pd.read_csv(tmp_path / "dataset.csv")
    assert tuple(df.columns) == fem.CSV_COLUMNS and len(df) == 2 and list(df["n_nodes"]) == [72, 132]
    for i, eps in enumerate(strains):
        pts, fcs = case.mesh[i]
        sol = fem.solve_cell(pts, fcs, strain=eps, rtol=RTOL)
        with np.load(df["data_filename"][i]) as f:
            assert set(f.files) == {"stress_field", "mean_stress", "mean_strain", "mean_stress_material",
                                    "op_div_matrix_data", "op_div_matrix_col_indices", "op_div_matrix_row_indices",
                                    "op_div_matrix_shape", "op_mean_stress", "node_labels"}
            assert np.array_equal(f["mean_strain"], np.array(eps))
            assert np.array_equal(f["mean_stress"], sol.mean_stress.cpu().numpy())
            assert abs(f["op_mean_stress"].sum() - float(sol.material_area / sol.cell_area)) <= 1e-6
        g = datasets.load_sample(df["mesh_filename"][i], df["data_filename"][i])
        assert torch.equal(g.pos, pts.cpu()) and torch.equal(g.face, fcs.cpu().T)
        assert torch.equal(_bits(g.local_stress), _bits(sol.stress.cpu()))
        assert torch.equal(g.mean_stress[0], sol.mean_stress.float().cpu())
        assert torch.equal(g.nodes_types[:, 0], torch.from_numpy(case.samples[i].node_types))
        assert torch.equal(g.op_div_matrix.to_dense(), devgraph.p1_divergence(pts, fcs).cpu().to_dense())
        data = fem.fem_targets(pts, fcs, eps, rtol=RTOL)
        assert torch.equal(_bits(data.local_stress.cpu()), _bits(g.local_stress))
        assert torch.equal(data.mean_stress.cpu(), g.mean_stress) and torch.equal(data.edge_index.cpu(), g.edge_index)
    ds = datasets.MeshStressFieldDatasetInMemory(df)
    store = DeviceGraphStore(ds.graphs, "cuda")
    torch.manual_seed(69)
    model = models.EncodeProcessDecode(input_edges_features_size=1, input_nodes_features_size=6,
                                       message_passing_steps=2, latent_size=128, output_nodes_features_size=3,
                                       **{k: v.cuda() for k, v in ds.stats().items()}).cuda()
    out = Trainer(model, lr=1e-3, divergence=True, divergence_penalty=10.0).step(store.batch([0, 1]))
    assert np.isfinite(float(out["total"]))


def test_the_call_replays_from_a_captured_graph(case):
    from gnn_local_stress import fem
    plan, (pts, fcs) = case.plans[2], case.mesh[2]
    elem = fem.element_table(plan, pts)
    other = torch.tensor([[[1e-3, -5e-4, 2e-4], [0.0, 1.0, 0.0], [3e-4, 3e-4, -1e-3]]], dtype=torch.float64, device="cuda")
    eager = fem.solve_cells(plan, pts, other, rtol=RTOL, elements=elem)
    static_in = case.unit.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fem.solve_cells(plan, pts, static_in, rtol=RTOL, elements=elem)
    static_in.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in ((out.stress, eager.stress), (out.strain, eager.strain), (out.ut, eager.ut), (out.table, eager.table),
                 (out.mean_stress, eager.mean_stress)):
        assert torch.equal(_bits(a), _bits(b))
    assert (out.table[0, :, 3] == fem.CONVERGED).all()
