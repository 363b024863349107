"""The Q1 hyperelastic cell solver on the device (gnn_local_stress/hyperelastic_q1.py, csrc/pdg_hyperq1.hip) against
the independent fp64 restatement tests/hyperq1_ref.py (scipy: Gauss-point residual and tangent assembled, periodic
reduction, one node pinned, sparse LU inside Newton with load stepping and the same backtracking rule).

Meshes: pdg.meshgen.quad_hole_plate(n, r, seed=3), default jitter, with (n, r) = (9, 0.25) 72 nodes, (13, 0.3) 132 and
(37, 0.2), which has 1208 nodes and 1104 faces, more of both than a workgroup has threads (512): the strided row and
element passes and their ragged last rounds.  Loads (hyper_ref.LOADS): two logarithmic strains from the reference's
+-0.15 box and one of 1e-4, in hyper_ref.N_STEPS = 4 load steps at rtol = 1e-10.  The bounds are those of
tests/test_gpu_hyper.py: the field bound is 2^-22 max|ref| per graph and load case, the fp32 rounding of the output
(the solver's own error at rtol = 1e-10 is below 1e-9 relative); the reference is solved to rtol = 1e-12 under the two
large loads and, where the rounding of P leaves no such residual, to 1e-10 under the small one.
tests/test_hyperq1_ref.py finds every (mesh, load) pair converged and its tangent positive definite at every state."""
import numpy as np
import pytest
import torch

import hyper_ref as H
import hyperq1_ref as Q
from pdg import meshgen

pytestmark = pytest.mark.gpu

RTOL = 1e-10
BOUND = 2.0 ** -22
STEPS = H.N_STEPS


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _dev(s):
    return torch.from_numpy(s.pos).cuda(), torch.from_numpy(s.faces).cuda()


def _v3(m):
    return np.array([m[0, 0], m[1, 1], m[0, 1]])


def _ref_rtol(eps):
    return 1e-12 if abs(eps[0]) > 1e-3 else 1e-10


class Case:
    def __init__(self):
        from gnn_local_stress import fem_q1, hyperelastic_q1 as hq
        self.samples = [meshgen.quad_hole_plate(n, r, seed=3) for n, r in Q.MESHES]
        assert tuple(s.num_nodes for s in self.samples) == Q.NODES
        self.pbs = [Q.problem(s.pos, s.faces) for s in self.samples]
        self.Fb = [Q.deformation_gradient(e) for e in H.LOADS]
        self.direct = [[Q.newton_direct(pb, F, rtol=_ref_rtol(e), n_steps=STEPS) for e, F in zip(H.LOADS, self.Fb)]
                       for pb in self.pbs]
        self.ref = [[Q.fields(pb, F, d.ut) for F, d in zip(self.Fb, ds)] for pb, ds in zip(self.pbs, self.direct)]
        self.counts = [[Q.newton_pcg(pb, F, rtol=RTOL, n_steps=STEPS) for F in self.Fb] for pb in self.pbs]
        self.mesh = [_dev(s) for s in self.samples]
        self.plans = [fem_q1.FemPlan.from_mesh(p, f) for p, f in self.mesh]
        self.F = torch.from_numpy(np.stack(self.Fb)).cuda().reshape(1, len(H.LOADS), 2, 2)
        self.solo = [hq.solve_cells(pl, p, self.F, rtol=RTOL, n_steps=STEPS) for pl, (p, f) in zip(self.plans, self.mesh)]
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def case():
    return Case()


def _check_fields(out, l, ref, what):
    for name, got, want in (("stress", out.stress[l], ref.stress), ("log strain", out.log_strain[l], ref.log_strain)):
        err = np.abs(got.cpu().numpy().astype(np.float64) - want).max() / np.abs(want).max()
        print(f"{what}: {name} error {err:.3e} (bound {BOUND:.3e})")
        assert err <= BOUND


def _check_means(out, l, ref, what):
    for name in ("mean_stress", "mean_pk1", "mean_stress_material"):
        got, want = getattr(out, name)[0, l].cpu().numpy(), getattr(ref, name)
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"{what}: {name} error {err:.3e} (bound 1e-9)")
        assert err <= 1e-9


def test_against_the_direct_solve(case):
    from gnn_local_stress import hyperelastic_q1 as hq
    for i, ((n, r), pb, out) in enumerate(zip(Q.MESHES, case.pbs, case.solo)):
        table = out.table.cpu().numpy()[0]
        ut = out.ut.cpu().numpy()
        for l, eps in enumerate(H.LOADS):
            ref, d, cnt = case.ref[i][l], case.direct[i][l], case.counts[i][l]
            assert d.status == Q.CONVERGED and cnt.status == Q.CONVERGED
            res = Q.residual(pb, case.Fb[l], ut[l])
            print(f"n={n} r={r} load {eps}: {int(table[l, 0])} steps, {int(table[l, 1])} Newton (numpy {cnt.newton}), "
                  f"{int(table[l, 2])} PCG (numpy {cnt.pcg}), table residual {table[l, 4]:.3e}, recomputed {res:.3e}")
            assert table[l, 5] == hq.CONVERGED and table[l, 0] == STEPS
            assert table[l, 4] <= RTOL
            assert res <= 2 * RTOL
            _check_fields(out, l, ref, f"n={n} load {l}")
            _check_means(out, l, ref, f"n={n} load {l}")
            assert np.array_equal(ut[l], ut[l][pb.c.rep])              # an image holds its representative's row
            assert np.abs(ut[l][pb.c.reps].mean(0)).max() <= 1e-12 * np.abs(ut[l]).max()
            assert table[l, 1] <= 2 * cnt.newton and table[l, 2] <= 2 * cnt.pcg
            want = case.samples[i].pos.astype(np.float64) @ case.Fb[l].T + ut[l]
            assert np.array_equal(out.deformed[l].cpu().numpy(), want.astype(np.float32))
        assert abs(float(out.material_area[0]) - case.ref[i][0].material_area) <= 1e-12 * case.ref[i][0].material_area
        assert float(out.cell_area[0]) == case.ref[i][0].cell_area


def test_quadratic_volumetric_term_and_unweighted_average(case):
    from gnn_local_stress import hyperelastic_q1 as hq
    pb = Q.problem(case.samples[0].pos, case.samples[0].faces, volumetric="quadratic")
    out = hq.solve_cells(case.plans[0], case.mesh[0][0], case.F, volumetric="quadratic", rtol=RTOL, n_steps=STEPS)
    cnt = hq.solve_cells(case.plans[0], case.mesh[0][0], case.F, rtol=RTOL, n_steps=STEPS, nodal="count")
    ut = out.ut.cpu().numpy()
    for l, eps in enumerate(H.LOADS):
        d = Q.newton_direct(pb, case.Fb[l], rtol=_ref_rtol(eps), n_steps=STEPS)
        c = Q.newton_pcg(pb, case.Fb[l], rtol=RTOL, n_steps=STEPS)
        ref = Q.fields(pb, case.Fb[l], d.ut)
        assert d.status == Q.CONVERGED and c.status == Q.CONVERGED
        assert out.table[0, l, 5] == hq.CONVERGED and out.table[0, l, 0] == STEPS
        assert float(out.table[0, l, 4]) <= RTOL and Q.residual(pb, case.Fb[l], ut[l]) <= 2 * RTOL
        assert out.table[0, l, 1] <= 2 * c.newton and out.table[0, l, 2] <= 2 * c.pcg
        _check_fields(out, l, ref, f"quadratic load {l}")
        _check_means(out, l, ref, f"quadratic load {l}")
        if abs(eps[0]) > 1e-3:     # the two energies differ at second order in J - 1
            assert np.abs(ref.stress - case.ref[0][l].stress).max() > 100 * BOUND * np.abs(ref.stress).max()
        ref_c = Q.fields(case.pbs[0], case.Fb[l], case.direct[0][l].ut, "count")
        _check_fields(cnt, l, ref_c, f"count load {l}")
        _check_means(cnt, l, ref_c, f"count load {l}")
        assert np.abs(ref_c.stress - case.ref[0][l].stress).max() > 100 * BOUND * np.abs(ref_c.stress).max()
    assert torch.equal(_bits(cnt.mean_stress), _bits(case.solo[0].mean_stress))
    assert torch.equal(_bits(cnt.ut), _bits(case.solo[0].ut)) and torch.equal(_bits(cnt.table), _bits(case.solo[0].table))


def test_plate_without_a_hole_needs_no_iteration_and_is_exact(case):
    from gnn_local_stress import fem_q1, hyperelastic_q1 as hq
    s = meshgen.quad_hole_plate(9, 0.0, seed=3)
    pts, fcs = _dev(s)
    plan = fem_q1.FemPlan.from_mesh(pts, fcs)
    det = fem_q1.element_table(plan, pts).reshape(-1, 4, 9)[:, :, 0]
    assert float(det.max() - det.min()) > 1e-3 * float(det.mean())        # jittered: the quads are not all alike
    out = hq.solve_cells(plan, pts, case.F, rtol=RTOL, n_steps=STEPS)
    table = out.table.cpu().numpy()[0]
    assert np.all(table[:, 5] == hq.CONVERGED) and np.all(table[:, 0] == STEPS)
    assert np.all(table[:, 1] == 0) and np.all(table[:, 2] == 0) and np.all(table[:, 4] <= RTOL)
    assert not out.ut.cpu().numpy().any()
    for l, Fb in enumerate(case.Fb):
        want = _v3(H.cauchy(Fb))
        err = np.abs(out.stress[l].cpu().numpy().astype(np.float64) - want).max() / np.abs(want).max()
        print(f"no hole, load {l}: nodal stress error {err:.3e} (bound {BOUND:.3e})")
        assert err <= BOUND
        le = H.log_strain(Fb)
        want_e = np.array([le[0, 0], le[1, 1], 2 * le[0, 1]])
        assert np.abs(out.log_strain[l].cpu().numpy().astype(np.float64) - want_e).max() <= BOUND * np.abs(want_e).max()


def test_a_clockwise_mesh_gives_the_same_fields(case):
    """Every face's vertex order reversed: the Gauss points are visited in another order, so not bitwise."""
    from gnn_local_stress import fem_q1, hyperelastic_q1 as hq
    pts, fcs = case.mesh[0]
    cw = fcs.flip(1).contiguous()
    plan = fem_q1.FemPlan.from_mesh(pts, cw)
    assert float(fem_q1.element_table(plan, pts).reshape(-1, 4, 9)[:, :, 0].max()) < 0
    out = hq.solve_cells(plan, pts, case.F, rtol=RTOL, n_steps=STEPS)
    assert (out.table[0, :, 5] == hq.CONVERGED).all() and (out.table[0, :, 4] <= RTOL).all()
    for l in range(len(H.LOADS)):
        _check_fields(out, l, case.ref[0][l], f"clockwise load {l}")
        _check_means(out, l, case.ref[0][l], f"clockwise load {l}")
    assert abs(float(out.material_area[0]) - case.ref[0][0].material_area) <= 1e-12 * case.ref[0][0].material_area


def test_a_graph_is_bitwise_the_same_inside_a_batch(case):
    from gnn_local_stress import fem_q1, hyperelastic_q1 as hq
    order = [2, None, 0, 1]                          # shuffled, an empty segment in the middle
    plan = fem_q1.FemPlan.collate([fem_q1.FemPlan.empty("cuda") if i is None else case.plans[i] for i in order])
    pts = torch.cat([case.mesh[i][0] for i in order if i is not None])
    out = hq.solve_cells(plan, pts, case.F.expand(len(order), -1, 2, 2).contiguous(), rtol=RTOL, n_steps=STEPS)
    ptr = plan.ptr.cpu().numpy()
    assert plan.n_graphs == 4 and ptr[1] == ptr[2]
    for g, i in enumerate(order):
        if i is None:
            assert torch.isnan(out.table[g]).all() and torch.isnan(out.mean_stress[g]).all()
            continue
        solo, a, b = case.solo[i], int(ptr[g]), int(ptr[g + 1])
        assert torch.equal(_bits(out.table[g]), _bits(solo.table[0]))
        for name in ("ut", "stress", "log_strain", "deformed"):
            assert torch.equal(_bits(getattr(out, name)[:, a:b]), _bits(getattr(solo, name))), name
        for name in ("mean_stress", "mean_pk1", "mean_stress_material"):
            assert torch.equal(_bits(getattr(out, name)[g]), _bits(getattr(solo, name)[0])), name


def test_caps(case):
    from gnn_local_stress import hyperelastic_q1 as hq
    plan, (pts, fcs) = case.plans[0], case.mesh[0]
    F = case.F[:, :2].contiguous()
    out = hq.solve_cells(plan, pts, F, rtol=RTOL, n_steps=STEPS, max_newton=1)
    table = out.table.cpu().numpy()[0]
    assert np.all(table[:, 5] == hq.MAX_ITER) and np.all(table[:, 0] == 0) and np.all(table[:, 1] == 1)
    assert np.all(np.isfinite(table)) and np.all(table[:, 4] > RTOL)
    assert torch.isfinite(out.stress).all() and torch.isfinite(out.ut).all() and out.ut.abs().max() > 0
    out = hq.solve_cells(plan, pts, F, rtol=RTOL, n_steps=STEPS, max_pcg=3, max_newton=1000)
    table = out.table.cpu().numpy()[0]
    print(f"max_pcg = 3: status {table[:, 5]}, Newton {table[:, 1]}, PCG {table[:, 2]}, residual {table[:, 4]}")
    assert np.all(np.isfinite(table)) and np.all(table[:, 2] <= 3 * table[:, 1])
    assert torch.isfinite(out.stress).all() and torch.isfinite(out.log_strain).all() and torch.isfinite(out.ut).all()


def test_host_checks(case):
    from gnn_local_stress import fem, hyperelastic_q1 as hq
    plan, (pts, fcs) = case.plans[0], case.mesh[0]
    for kw in (dict(mu=0.0), dict(kappa=float("inf")), dict(volumetric="cubic"), dict(n_steps=0), dict(n_steps=10001),
               dict(rtol=0.0), dict(rtol=1.0), dict(eta=1.0), dict(eta=0.0), dict(nodal="sum")):
        with pytest.raises(ValueError):
            hq.solve_cells(plan, pts, case.F, **kw)
    for bad in ([[1.0, 0.0], [0.0, -1.0]], [[1.0, 2.0], [0.5, 1.0]]):                # det < 0, det == 0
        with pytest.raises(ValueError, match="det F must be > 0"):
            hq.solve_cell(pts, fcs, F=bad)
        with pytest.raises(ValueError, match="det F must be > 0"):
            hq.solve_cells(plan, pts, torch.tensor(bad, dtype=torch.float64).reshape(1, 1, 2, 2))
    with pytest.raises(ValueError, match="finite"):
        hq.solve_cells(plan, pts, torch.full((1, 1, 2, 2), float("nan"), dtype=torch.float64))
    with pytest.raises(ValueError, match="F must be"):
        hq.solve_cells(plan, pts, case.F.expand(2, -1, 2, 2).contiguous())
    t = meshgen.hole_plate(9, 0.25, seed=3)
    tp, tf = _dev(t)
    with pytest.raises(ValueError, match=r"fem_q1.FemPlan .*gnn_local_stress.hyperelastic$"):      # a triangle plan
        hq.solve_cells(fem.FemPlan.from_mesh(tp, tf), tp, case.F)
    for call in (lambda: hq.solve_cell(tp, tf, strain=(0.1, 0.0, 0.0)), lambda: hq.hyper_targets(tp, tf, (0.1, 0.0, 0.0)),
                 lambda: hq.write_sample("unused", 0, tp, tf, (0.1, 0.0, 0.0))):            # an (F, 3) mesh
        with pytest.raises(ValueError, match=r"takes quads only: a triangle mesh \(faces \(F, 3\)\) goes to "
                                             r"gnn_local_stress.hyperelastic$"):
            call()
    for call in (lambda: hq.solve_cell(pts.cpu(), fcs.cpu(), strain=(0.1, 0.0, 0.0)),
                 lambda: hq.solve_cells(plan, pts.cpu(), case.F), lambda: hq.hyper_targets(pts.cpu(), fcs, (0.1, 0.0, 0.0))):
        with pytest.raises(RuntimeError, match="HIP"):
            call()
    with pytest.raises(ValueError, match="36"):
        hq.solve_cells(plan, pts, case.F, elements=torch.zeros(plan.n_faces, 8, dtype=torch.float64, device="cuda"))
    sol = hq.solve_cell(pts, fcs, F=case.Fb[0], rtol=RTOL, n_steps=STEPS)          # F= and strain= are one problem
    assert torch.equal(_bits(sol.stress), _bits(case.solo[0].stress[0]))
    assert np.abs(sol.mean_strain.cpu().numpy() - np.array(H.LOADS[0])).max() <= 1e-14


def test_capture_replay_and_a_nan_load(case):
    from gnn_local_stress import fem_q1, hyperelastic_q1 as hq
    plan, (pts, fcs) = case.plans[1], case.mesh[1]
    elem = fem_q1.element_table(plan, pts)
    other = case.F[:, [1, 0, 2]].contiguous()
    eager = hq.solve_cells(plan, pts, other, rtol=RTOL, n_steps=STEPS, elements=elem)
    static_in = case.F.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="needs elements=fem_q1.element_table"):
            hq.solve_cells(plan, pts, static_in, rtol=RTOL, n_steps=STEPS)
        out = hq.solve_cells(plan, pts, static_in, rtol=RTOL, n_steps=STEPS, elements=elem)
    static_in.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    for name in ("stress", "log_strain", "ut", "table", "mean_stress", "mean_pk1", "deformed"):
        assert torch.equal(_bits(getattr(out, name)), _bits(getattr(eager, name))), name
    assert (out.table[0, :, 5] == hq.CONVERGED).all()
    # a NaN in F under capture: no host check; the kernel returns, BREAKDOWN, NaN rows; the other cases are untouched
    bad = other.clone()
    bad[0, 1, 0, 1] = float("nan")
    static_in.copy_(bad)
    graph.replay()
    torch.cuda.synchronize()
    assert out.table[0, 1, 5] == hq.BREAKDOWN and out.table[0, 1, 0] == 0 and out.table[0, 1, 1] == 0
    assert torch.isnan(out.ut[1]).all() and torch.isnan(out.stress[1]).all() and torch.isnan(out.table[0, 1, 4])
    for l in (0, 2):
        assert torch.equal(_bits(out.stress[l]), _bits(eager.stress[l]))
        assert torch.equal(_bits(out.table[0, l]), _bits(eager.table[0, l]))
    static_in.copy_(other)                           # and the replay after it is clean again
    graph.replay()
    torch.cuda.synchronize()
    for name in ("stress", "log_strain", "ut", "table", "mean_stress"):
        assert torch.equal(_bits(getattr(out, name)), _bits(getattr(eager, name))), name


def test_write_sample_round_trip_and_training_step(case, tmp_path):
    import pandas as pd
    from gnn_local_stress import datasets, fem, hyperelastic_q1 as hq, models
    from pdg import devgraph
    from pdg.collate import DeviceGraphStore
    from pdg.trainer import Trainer
    for i, eps in enumerate(H.LOADS[:2]):
        row = hq.write_sample(tmp_path, i, *case.mesh[i], eps, rtol=RTOL, n_steps=STEPS, meta={"seed": 3})
        assert tuple(row) == fem.CSV_COLUMNS
    df = pd.read_csv(tmp_path / "dataset.csv")
    assert tuple(df.columns) == fem.CSV_COLUMNS and len(df) == 2 and list(df["n_nodes"]) == [72, 132]
    datas = []
    for i, eps in enumerate(H.LOADS[:2]):
        pts, fcs = case.mesh[i]
        sol = hq.solve_cell(pts, fcs, strain=eps, rtol=RTOL, n_steps=STEPS)
        raw = open(df["mesh_filename"][i], "rb").read()
        k = raw.index(b"\n", raw.index(b"CELL_TYPES %d" % len(fcs))) + 1
        assert b"DATASET UNSTRUCTURED_GRID" in raw
        assert np.all(np.frombuffer(raw[k:k + 4 * len(fcs)], ">i4") == 9)  # VTK_QUAD, big-endian as legacy VTK is
        with np.load(df["data_filename"][i]) as f:
            assert set(f.files) == {"stress_field", "mean_stress", "mean_strain", "mean_stress_reference_mesh",
                                    "op_div_matrix_data", "op_div_matrix_col_indices", "op_div_matrix_row_indices",
                                    "op_div_matrix_shape", "node_labels"}
            assert np.array_equal(f["mean_strain"], np.array(eps))
            assert np.array_equal(f["mean_stress"], sol.mean_stress.cpu().numpy())
        g = datasets.load_sample(df["mesh_filename"][i], df["data_filename"][i])
        assert torch.equal(g.pos, pts.cpu()) and torch.equal(g.face, fcs.cpu().T) and g.face.shape[0] == 4
        assert torch.equal(_bits(g.local_stress), _bits(sol.stress.cpu()))
        assert torch.equal(g.mean_stress[0], sol.mean_stress.float().cpu())
        assert torch.equal(g.nodes_types[:, 0], torch.from_numpy(case.samples[i].node_types))
        op = devgraph.p1_divergence(sol.deformed, fcs, cells="quad").cpu().to_dense()
        assert torch.equal(g.op_div_matrix.to_dense(), op)                                # on the deformed mesh
        assert not torch.equal(op, devgraph.p1_divergence(pts, fcs, cells="quad").cpu().to_dense())
        data = hq.hyper_targets(pts, fcs, eps, rtol=RTOL, n_steps=STEPS)
        assert torch.equal(data.nodes_types.cpu()[:, 0], torch.from_numpy(case.samples[i].node_types))
        assert torch.equal(_bits(data.local_stress.cpu()), _bits(g.local_stress))
        assert torch.equal(data.mean_stress.cpu(), g.mean_stress) and torch.equal(data.edge_index.cpu(), g.edge_index)
        assert torch.equal(data.op_div_matrix.cpu().to_dense(), op) and torch.equal(data.pos.cpu(), g.pos)
        datas.append(data)
    ds = datasets.MeshStressFieldDatasetInMemory(df)
    store = DeviceGraphStore(datas, "cuda")                  # the hyper_targets graphs themselves
    torch.manual_seed(69)
    model = models.EncodeProcessDecode(input_edges_features_size=1, input_nodes_features_size=6,
                                       message_passing_steps=2, latent_size=128, output_nodes_features_size=3,
                                       **{k: v.cuda() for k, v in ds.stats().items()}).cuda()
    out = Trainer(model, lr=1e-3, divergence=True, divergence_penalty=10.0).step(store.batch([0, 1]))
    assert np.isfinite(float(out["total"]))
