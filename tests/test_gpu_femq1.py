"""The Q1 FEM cell solver on the device (gnn_local_stress/fem_q1.py, csrc/pdg_femq1.hip) against the independent fp64
restatement tests/femq1_ref.py (scipy: assembled Q1 K, periodic reduction, one node pinned, sparse LU).

Meshes: pdg.meshgen.quad_hole_plate(n, r, seed=3) with (n, r) = (9, 0.25) 72 nodes, (13, 0.3) 132, (17, 0.2) 252 and
(37, 0.2) 1208, which has more than 1024 nodes: the strided ownership and the ragged last pass.  The bounds are those
of tests/test_gpu_fem.py: the stress bound is 2^-22 max|sigma_ref| per graph and load case, the fp32 rounding of the
output; the solver's own error at rtol = 1e-10 is some 1e-11 relative (tests/test_femq1_ref.py), far below it."""
import numpy as np
import pytest
import torch

import femq1_ref as R
from pdg import meshgen

pytestmark = pytest.mark.gpu

MESHES = ((9, 0.25), (13, 0.3), (17, 0.2), (37, 0.2))
NODES = (72, 132, 252, 1208)
RTOL = 1e-10
BOUND = 2.0 ** -22


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _dev(s):
    return torch.from_numpy(s.pos).cuda(), torch.from_numpy(s.faces).cuda()


class Case:
    def __init__(self):
        from gnn_local_stress import fem_q1
        self.samples = [meshgen.quad_hole_plate(n, r, seed=3) for n, r in MESHES]
        assert tuple(s.num_nodes for s in self.samples) == NODES
        self.cells = [R.cell(s.pos, s.faces) for s in self.samples]
        self.direct = [[R.solve_direct(c, e)[0] for e in R.UNIT] for c in self.cells]
        self.ref = [[R.fields(c, e, u) for e, u in zip(R.UNIT, us)] for c, us in zip(self.cells, self.direct)]
        self.pcg_its = [[R.pcg(c, e, rtol=RTOL)[1] for e in R.UNIT] for c in self.cells]
        self.mesh = [_dev(s) for s in self.samples]
        self.plans = [fem_q1.FemPlan.from_mesh(p, f) for p, f in self.mesh]
        self.unit = torch.eye(3, dtype=torch.float64, device="cuda").reshape(1, 3, 3)
        self.solo = [fem_q1.solve_cells(pl, p, self.unit, rtol=RTOL) for pl, (p, f) in zip(self.plans, self.mesh)]
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def case():
    return Case()


def test_plate_without_a_hole_is_trivial_and_exact():
    from gnn_local_stress import fem_q1
    s = meshgen.quad_hole_plate(9, 0.0, seed=3)
    pts, fcs = _dev(s)
    plan = fem_q1.FemPlan.from_mesh(pts, fcs)
    out = fem_q1.solve_cells(plan, pts, torch.eye(3, dtype=torch.float64, device="cuda").reshape(1, 3, 3), rtol=RTOL)
    table = out.table.cpu().numpy()[0]
    assert np.all(table[:, 3] == fem_q1.TRIVIAL) and np.all(table[:, 0] == 0) and np.all(table[:, 2] == 0)
    assert not out.ut.cpu().numpy().any()
    c = R.stiffness()
    for l, eps in enumerate(R.UNIT):
        want = c @ eps
        err = np.abs(out.stress[l].cpu().numpy().astype(np.float64) - want).max() / np.abs(want).max()
        print(f"no hole, case {l}: |b| = {table[l, 1]:.3e}, nodal stress error {err:.3e} (bound {BOUND:.3e})")
        assert err <= BOUND
        assert np.abs(out.strain[l].cpu().numpy().astype(np.float64) - eps).max() <= BOUND
        assert np.abs(out.mean_stress[0, l].cpu().numpy() - want).max() <= 1e-12 * np.abs(want).max()


def test_plan_and_element_table_match_the_restatement(case):
    from gnn_local_stress import fem_q1
    for s, c, plan, (pts, fcs) in zip(case.samples, case.cells, case.plans, case.mesh):
        assert np.array_equal(plan.rep.cpu().numpy(), c.rep)
        rp, item = plan.item_rowptr.cpu().numpy(), plan.item.cpu().numpy()
        key = c.rep[s.faces.ravel()]
        assert rp[0] == 0 and rp[-1] == 4 * len(s.faces)
        assert np.array_equal(np.diff(rp), np.bincount(key, minlength=len(c.rep)))
        for v in range(len(c.rep)):
            assert np.array_equal(item[rp[v]:rp[v + 1]], np.where(key == v)[0])   # ascending, images' corners included
        assert np.array_equal(plan.rverts.cpu().numpy(), key)
        elem = fem_q1.element_table(plan, pts).cpu().numpy().reshape(-1, 4, 9)
        assert elem[:, :, 0].min() > 0
        # fp64 from the same float32 coordinates in another order of operations.  A derivative of x is a sum of four
        # terms of size <= 0.4 x 100 that comes to ~ h / 2 >= 1.4: 4 x 40 x 2^-53 / 1.4 ~ 1.3e-14 relative; det J
        # and a gradient are a handful of products and one quotient of those: 1e-12 holds with room
        assert np.abs(elem[:, :, 0] - c.det).max() <= 1e-12 * np.abs(c.det).max()
        grad = np.stack([c.B[:, :, 0, 0::2], c.B[:, :, 1, 1::2]], 2).reshape(-1, 4, 8)
        assert np.abs(elem[:, :, 1:] - grad).max() <= 1e-12 * np.abs(grad).max()


def test_against_the_direct_solve(case):
    from gnn_local_stress import fem_q1
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
            assert table[l, 3] == fem_q1.CONVERGED
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
    from gnn_local_stress import fem_q1
    order = [2, 0, None, 3, 1]                       # shuffled, an empty segment in the middle
    plans = [fem_q1.FemPlan.empty("cuda") if i is None else case.plans[i] for i in order]
    plan = fem_q1.FemPlan.collate(plans)
    pts = torch.cat([case.mesh[i][0] for i in order if i is not None])
    out = fem_q1.solve_cells(plan, pts, case.unit.expand(len(order), 3, 3).contiguous(), rtol=RTOL)
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
    from gnn_local_stress import fem_q1
    out = fem_q1.solve_cells(case.plans[1], case.mesh[1][0], case.unit, rtol=RTOL, max_iter=5)
    table = out.table.cpu().numpy()[0]
    assert np.all(table[:, 3] == fem_q1.MAX_ITER) and np.all(table[:, 0] == 5)
    assert np.all(np.isfinite(table)) and np.all(table[:, 2] > RTOL)
    assert torch.isfinite(out.stress).all() and torch.isfinite(out.ut).all()


def test_imposed_mean_stress_and_effective_stiffness(case):
    from gnn_local_stress import fem_q1
    pts, fcs = case.mesh[1]
    target = np.array([120.0, -40.0, 25.0])
    sol = fem_q1.solve_cell(pts, fcs, stress=target, rtol=RTOL)
    got = sol.mean_stress.cpu().numpy()
    print(f"imposed mean stress: relative miss {np.abs(got - target).max() / np.abs(target).max():.3e}")
    assert np.abs(got - target).max() <= 1e-9 * np.abs(target).max()
    ce = fem_q1.effective_stiffness(pts, fcs, rtol=RTOL).cpu().numpy()
    ref = R.effective_stiffness(case.cells[1])
    print(f"C_eff: difference to femq1_ref {np.abs(ce - ref).max() / np.abs(ref).max():.3e}, asymmetry "
          f"{np.abs(ce - ce.T).max() / np.abs(ce).max():.3e}")
    assert np.abs(ce - ref).max() <= 1e-9 * np.abs(ref).max()
    assert np.abs(ce - ce.T).max() <= 1e-9 * np.abs(ce).max()
    # the field is the restatement's under that strain, and the localisation tensor gives the same field
    eps = sol.mean_strain.cpu().numpy()
    f = R.fields(case.cells[1], eps, R.solve_direct(case.cells[1], eps)[0])
    assert np.abs(sol.stress.cpu().numpy() - f.stress).max() <= BOUND * np.abs(f.stress).max()
    A = fem_q1.localisation_tensor(pts, fcs, rtol=RTOL)
    assert A.shape == (case.samples[1].num_nodes, 3, 3) and A.dtype == torch.float32
    field = torch.einsum("nij,j->ni", A.double(), torch.from_numpy(target).cuda()).cpu().numpy()
    assert np.abs(field - f.stress).max() <= 4 * BOUND * np.abs(f.stress).max()     # 3 rounded terms + the sum


def test_unweighted_nodal_average(case):
    from gnn_local_stress import fem_q1
    out = fem_q1.solve_cells(case.plans[0], case.mesh[0][0], case.unit, rtol=RTOL, nodal="count")
    for l, eps in enumerate(R.UNIT):
        ref = R.fields(case.cells[0], eps, case.direct[0][l], "count")
        err = np.abs(out.stress[l].cpu().numpy() - ref.stress).max() / np.abs(ref.stress).max()
        assert err <= BOUND
        assert np.abs(ref.stress - case.ref[0][l].stress).max() > 100 * BOUND * np.abs(ref.stress).max()
    assert torch.equal(_bits(out.mean_stress), _bits(case.solo[0].mean_stress))
    assert torch.equal(_bits(out.mean_stress_material), _bits(case.solo[0].mean_stress_material))
    assert torch.equal(_bits(out.ut), _bits(case.solo[0].ut))


def test_a_clockwise_mesh_is_accepted(case):
    from gnn_local_stress import fem_q1
    pts, fcs = case.mesh[0]
    cw = fcs.flip(1).contiguous()
    plan = fem_q1.FemPlan.from_mesh(pts, cw)
    assert float(fem_q1.element_table(plan, pts).reshape(-1, 4, 9)[:, :, 0].max()) < 0
    out = fem_q1.solve_cells(plan, pts, case.unit, rtol=RTOL)
    assert (out.table[0, :, 3] == fem_q1.CONVERGED).all()
    for l in range(3):
        ref = case.ref[0][l]
        assert np.abs(out.stress[l].cpu().numpy() - ref.stress).max() <= BOUND * np.abs(ref.stress).max()
        assert np.abs(out.mean_stress[0, l].cpu().numpy() - ref.mean_stress).max() <= 1e-9 * np.abs(ref.mean_stress).max()
    assert abs(float(out.material_area[0]) - case.ref[0][0].material_area) <= 1e-12 * case.ref[0][0].material_area


def test_degenerate_faces_and_non_periodic_boundary_raise(case):
    from gnn_local_stress import fem_q1
    s = case.samples[0]
    pts, fcs = case.mesh[0]
    bow = fcs.clone()
    bow[0] = fcs[0, [0, 2, 1, 3]]                            # two crossing sides: det J changes sign
    with pytest.raises(ValueError, match="not all strictly of one sign"):
        fem_q1.solve_cell(pts, bow, strain=(1e-3, 0.0, 0.0))
    flat = fcs.clone()
    flat[0] = fcs[0, [0, 0, 3, 3]]                           # collapsed onto a side: det J == 0 exactly
    with pytest.raises(ValueError, match="zero area"):
        fem_q1.solve_cell(pts, flat, strain=(1e-3, 0.0, 0.0))
    with pytest.raises(ValueError, match="not all strictly of one sign"):
        fem_q1.effective_stiffness(pts, bow)
    bad = pts.clone()
    k = int(np.where(s.pos[:, 0] == s.pos[:, 0].max())[0][3])
    bad[k, 1] += 0.25
    with pytest.raises(ValueError, match="mesh is not periodic"):
        fem_q1.FemPlan.from_mesh(bad, fcs)
    out = fcs.clone()
    out[1, 1] = s.num_nodes
    with pytest.raises(ValueError, match="outside"):
        fem_q1.FemPlan.from_mesh(pts, out)
    with pytest.raises(ValueError, match="finite"):
        fem_q1.solve_cell(pts, fcs, strain=(float("nan"), 0.0, 0.0))
    tri = torch.zeros(4, 3, dtype=torch.int64, device="cuda")
    for call in (lambda: fem_q1.FemPlan.from_mesh(pts, tri), lambda: fem_q1.solve_cell(pts, tri, strain=(1.0, 0.0, 0.0)),
                 lambda: fem_q1.effective_stiffness(pts, tri), lambda: fem_q1.fem_targets(pts, tri, (1.0, 0.0, 0.0))):
        with pytest.raises(ValueError, match="the Q1 solver takes quads only"):
            call()


def test_write_sample_round_trip_and_training_step(case, tmp_path):
    import pandas as pd
    from gnn_local_stress import datasets, fem_q1, models
    from pdg import devgraph
    from pdg.collate import DeviceGraphStore
    from pdg.trainer import Trainer
    strains = ((1e-3, -5e-4, 2e-4), (-2e-4, 8e-4, 1e-3))
    for i, eps in enumerate(strains):
        row = fem_q1.write_sample(tmp_path, i, *case.mesh[i], eps, rtol=RTOL,
                                  meta={"seed": 3, "hole_plate_radius": 25.0})
        assert tuple(row) == fem_q1.CSV_COLUMNS
    df = pd.read_csv(tmp_path / "dataset.csv")
    assert tuple(df.columns) == fem_q1.CSV_COLUMNS and len(df) == 2 and list(df["n_nodes"]) == [72, 132]
    datas = []
    for i, eps in enumerate(strains):
        pts, fcs = case.mesh[i]
        sol = fem_q1.solve_cell(pts, fcs, strain=eps, rtol=RTOL)
        raw = open(df["mesh_filename"][i], "rb").read()
        k = raw.index(b"\n", raw.index(b"CELL_TYPES %d" % len(fcs))) + 1
        assert b"DATASET UNSTRUCTURED_GRID" in raw
        assert np.all(np.frombuffer(raw[k:k + 4 * len(fcs)], ">i4") == 9)  # VTK_QUAD, big-endian as legacy VTK is
        with np.load(df["data_filename"][i]) as f:
            assert set(f.files) == {"stress_field", "mean_stress", "mean_strain", "mean_stress_material",
                                    "op_div_matrix_data", "op_div_matrix_col_indices", "op_div_matrix_row_indices",
                                    "op_div_matrix_shape", "op_mean_stress", "node_labels"}
            assert np.array_equal(f["mean_strain"], np.array(eps))
            assert np.array_equal(f["mean_stress"], sol.mean_stress.cpu().numpy())
            assert abs(f["op_mean_stress"].sum() - float(sol.material_area / sol.cell_area)) <= 1e-6
        g = datasets.load_sample(df["mesh_filename"][i], df["data_filename"][i])
        assert torch.equal(g.pos, pts.cpu()) and torch.equal(g.face, fcs.cpu().T) and g.face.shape[0] == 4
        assert torch.equal(_bits(g.local_stress), _bits(sol.stress.cpu()))
        assert torch.equal(g.mean_stress[0], sol.mean_stress.float().cpu())
        assert torch.equal(g.nodes_types[:, 0], torch.from_numpy(case.samples[i].node_types))
        assert torch.equal(g.op_div_matrix.to_dense(), devgraph.p1_divergence(pts, fcs, cells="quad").cpu().to_dense())
        data = fem_q1.fem_targets(pts, fcs, eps, rtol=RTOL)
        assert torch.equal(_bits(data.local_stress.cpu()), _bits(g.local_stress))
        assert torch.equal(data.mean_stress.cpu(), g.mean_stress) and torch.equal(data.edge_index.cpu(), g.edge_index)
        datas.append(data)
    ds = datasets.MeshStressFieldDatasetInMemory(df)
    store = DeviceGraphStore(datas, "cuda")                  # the fem_targets graphs themselves
    torch.manual_seed(69)
    model = models.EncodeProcessDecode(input_edges_features_size=1, input_nodes_features_size=6,
                                       message_passing_steps=2, latent_size=128, output_nodes_features_size=3,
                                       **{k: v.cuda() for k, v in ds.stats().items()}).cuda()
    out = Trainer(model, lr=1e-3, divergence=True, divergence_penalty=10.0).step(store.batch([0, 1]))
    assert np.isfinite(float(out["total"]))


def test_the_call_replays_from_a_captured_graph(case):
    from gnn_local_stress import fem_q1
    plan, (pts, fcs) = case.plans[2], case.mesh[2]
    with pytest.raises(ValueError, match="36"):
        fem_q1.solve_cells(plan, pts, case.unit, elements=torch.zeros(plan.n_faces, 8, dtype=torch.float64, device="cuda"))
    elem = fem_q1.element_table(plan, pts)
    other = torch.tensor([[[1e-3, -5e-4, 2e-4], [0.0, 1.0, 0.0], [3e-4, 3e-4, -1e-3]]], dtype=torch.float64, device="cuda")
    eager = fem_q1.solve_cells(plan, pts, other, rtol=RTOL, elements=elem)
    static_in = case.unit.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="needs elements=element_table"):
            fem_q1.solve_cells(plan, pts, static_in, rtol=RTOL)
        out = fem_q1.solve_cells(plan, pts, static_in, rtol=RTOL, elements=elem)
    static_in.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in ((out.stress, eager.stress), (out.strain, eager.strain), (out.ut, eager.ut), (out.table, eager.table),
                 (out.mean_stress, eager.mean_stress)):
        assert torch.equal(_bits(a), _bits(b))
    assert (out.table[0, :, 3] == fem_q1.CONVERGED).all()
