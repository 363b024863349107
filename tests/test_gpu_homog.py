"""The homogenisation layer on the device against its host restatements: pdg_nodal_areas against
pdg.meshgen.nodal_areas, pdg_graph_wmean / pdg_mean_correct against tests/homog_ref.py, and the Python layer built
on them (devgraph.nodal_areas, homogenise, sensitivity.mean_localisation, inference.predict_mesh).

Every bound is derived, none measured.  With u = 2^-53:

* areas: both sides round one fp64 sum of the same non-negative terms to fp32; the sums differ by ~1e-15 relative
  at most, so the results lie at most one fp32 ulp apart: 2^-23 |want|;
* sums of n_g fp64 additions in any order, of products that are exact (two 24-bit significands):
  |got - want| <= 2 n_g u sum |w x| (the restatement's own sums are math.fsum's, exact to one rounding);
* a corrected element is one fp32 rounding of sigma + shift, the fp64 shift's own error being far below it:
  2^-23 (|sigma| + |shift|);
* the average of a corrected field sigma' misses the target by the outputs' fp32 roundings, 2^-24 sum w |sigma'| / D,
  plus fp64 terms: the two sums' errors, n u (sum |w sigma| + sum |w sigma'|) / D, and the shift's arithmetic
  (t D - S) / W with W within n u of exact and three roundings, (n + 3) u (|t| + sum |w sigma| / D); together below
  2 (n + 3) u (sum |w sigma| / D + sum |w sigma'| / D + |t|).
"""
import numpy as np
import pytest
import torch

import homog_ref as R
from test_meshfields_host import renumbered

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _plate(n, hole=0.0, seed=3):
    from pdg import meshgen
    return meshgen.hole_plate(n=n, hole_radius=hole, seed=seed)


def _meshes():
    """name -> (pos, faces): no hole (81 nodes), a hole of radius 20 in the plate of side 100 (hole_plate takes the
    radius as a fraction of the side: 0.2), 1,225 nodes (a thread of the per-graph kernels owns more than
    one row), the hole plate renumbered with its faces shuffled, and three-dimensional points."""
    a, b, c = _plate(9), _plate(13, 0.2), _plate(35)
    assert a.num_nodes == 81 and c.num_nodes == 1225 and b.num_nodes < 169
    pos2, faces2, _ = renumbered(b.pos, b.faces)
    z = np.random.default_rng(1).uniform(-1, 1, (b.num_nodes, 1)).astype(np.float32)
    return {"plate9": (a.pos, a.faces), "hole13": (b.pos, b.faces), "plate35": (c.pos, c.faces),
            "renumbered": (pos2, faces2), "points3d": (np.concatenate([b.pos, z], 1), b.faces)}


MESHES = _meshes()


def _dev(pos, faces):
    return (torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float32)).cuda(),
            torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)).cuda())


def _areas_raw(pos, faces):
    """pdg_nodal_areas itself: (area, bbox, status) as numpy, no exception for any status."""
    from pdg.lib import lib, stream_handle
    pts, fcs = _dev(pos, faces)
    n, dim = pts.shape
    nf = len(fcs)
    nbytes = lib.pdg_mesh_fields_scratch_bytes(n, nf)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    area = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    bbox = torch.full((4,), -7.0, dtype=torch.float32, device="cuda")
    status = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    lib.pdg_nodal_areas(n, pts.data_ptr(), dim, nf, fcs.data_ptr() if nf else None, area.data_ptr(), bbox.data_ptr(),
                        status.data_ptr(), scratch.data_ptr(), nbytes, stream_handle(pts.device))
    return area.cpu().numpy(), bbox.cpu().numpy(), int(status.item())


def _check_areas(got, want, what):
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bound = 2.0 ** -23 * np.abs(want.astype(np.float64))
    print(f"{what}: {len(want)} nodes, bitwise equal {np.mean(got == want):.4f}, max err / bound "
          f"{np.max(err / np.maximum(bound, 1e-300)):.3e}")
    assert np.all(err <= bound)


@pytest.mark.parametrize("name", sorted(MESHES))
def test_areas_are_the_host_restatement(name):
    from pdg import meshgen
    from pdg.devgraph import nodal_areas
    pos, faces = MESHES[name]
    want, wbox = meshgen.nodal_areas(pos, faces)
    got, bbox, status = _areas_raw(pos, faces)
    assert status == 0
    _check_areas(got, want, name)
    assert bbox.dtype == np.float32 and np.array_equal(bbox.view(np.int32), wbox.view(np.int32))
    out = nodal_areas(*_dev(pos, faces))
    assert out.area.is_cuda and out.area.dtype == torch.float32 and np.array_equal(out.area.cpu().numpy(), got)
    b = wbox.astype(np.float64)
    assert out.cell_area.is_cuda and out.cell_area.dtype == torch.float64 and out.cell_area.shape == (1,)
    assert float(out.cell_area) == (b[1] - b[0]) * (b[3] - b[2])
    # two calls agree bitwise: the sums do not depend on the order in which the slot atomics land
    assert np.array_equal(_areas_raw(pos, faces)[0], got)


def test_unreferenced_nodes_zero_area_faces_and_no_faces():
    from pdg import meshgen
    pos, faces = MESHES["hole13"]
    base, bbox, _ = _areas_raw(pos, faces)
    pos2 = np.concatenate([pos, np.array([[40.0, 60.0]], np.float32)])
    faces2 = np.concatenate([faces[:5], np.array([[0, 1, 1], [2, 2, 2]], np.int64), faces[5:]])
    got, box2, status = _areas_raw(pos2, faces2)
    assert status == 0 and got[-1] == 0.0 and not np.signbit(got[-1])   # exactly +0
    assert np.array_equal(got[:-1], base) and np.array_equal(box2, bbox)
    _check_areas(got, meshgen.nodal_areas(pos2, faces2)[0], "with a free node and two flat faces")
    got, box0, status = _areas_raw(pos, np.zeros((0, 3), np.int64))
    assert status == 0 and not got.any() and np.array_equal(box0, bbox)


def test_out_of_range_face_is_ignored_and_reported():
    from pdg.devgraph import nodal_areas
    pos, faces = MESHES["hole13"]
    n = len(pos)
    base, bbox, _ = _areas_raw(pos, faces)
    bad = np.concatenate([faces[:7], np.array([[0, 1, n], [-1, 2, 3]], np.int64), faces[7:]])
    got, box, status = _areas_raw(pos, bad)
    assert status == 1 and np.array_equal(got, base) and np.array_equal(box, bbox)   # the mesh without those faces
    with pytest.raises(ValueError, match="outside"):
        nodal_areas(*_dev(pos, bad))
    with pytest.raises(ValueError, match="triangle"):
        nodal_areas(_dev(pos, faces)[0], torch.zeros(2, 4, dtype=torch.int64, device="cuda"))
    assert np.array_equal(nodal_areas(*_dev(pos, faces)).area.cpu().numpy(), base)   # and the process goes on


# ------------------------------------------------------------------------------------------ per-graph sums
class Case:
    """The three plates, an empty graph between them and a graph whose weights are all zero; weights = the nodal
    areas with some zeros, one negative and one NaN; one random field of 9 columns (its first 1 and 3 are the
    narrower fields); the restatement's tables, computed once."""

    def __init__(self):
        from pdg import meshgen
        rng = np.random.default_rng(7)
        names = ("plate9", "hole13", "plate35")
        areas = [meshgen.nodal_areas(*MESHES[k]) for k in names]
        counts = [len(areas[0][0]), len(areas[1][0]), 0, len(areas[2][0]), 7]
        self.ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.B, self.N = len(counts), int(self.ptr[-1])
        self.EMPTY, self.DEAD = 2, 4
        w = np.concatenate([areas[0][0], areas[1][0], areas[2][0], np.zeros(7, np.float32)])
        self.excluded = np.array([3, 50, 90, 91, 400, 1300])
        w[self.excluded] = [0.0, 0.0, -2.5, np.nan, 0.0, 0.0]
        self.w = w
        boxes = [a[1].astype(np.float64) for a in areas]
        cell = [(b[1] - b[0]) * (b[3] - b[2]) for b in boxes]
        self.cell = np.array([cell[0], cell[1], 1.0, cell[2], 49.0])
        self.x = rng.normal(0.0, 50.0, (self.N, 9)).astype(np.float32)
        self.target = rng.normal(0.0, 30.0, (self.B, 3)).astype(np.float32)
        self.ref = {c: R.graph_wmean(self.ptr, self.x[:, :c], self.w) for c in (1, 3, 9)}
        self.d_ptr = torch.from_numpy(self.ptr.astype(np.int32)).cuda()
        self.d_w = torch.from_numpy(self.w).cuda()
        self.d_x = torch.from_numpy(self.x).cuda()
        self.d_cell = torch.from_numpy(self.cell).cuda()
        self.d_target = torch.from_numpy(self.target).cuda()

    def rows(self, c):
        return self.d_x[:, :c].contiguous()

    def n_g(self):
        return np.diff(self.ptr).astype(np.float64)


@pytest.fixture(scope="module")
def case():
    return Case()


def _wmean(d_ptr, d_rows, d_w):
    from pdg.lib import lib, stream_handle
    b, c = d_ptr.numel() - 1, d_rows.shape[1]
    table = torch.full((b, c + 1), -7.0, dtype=torch.float64, device="cuda")
    lib.pdg_graph_wmean(b, d_ptr.data_ptr(), d_rows.data_ptr(), c, d_w.data_ptr() if d_w is not None else None,
                        table.data_ptr(), stream_handle(d_rows.device))
    return table


def _correct(d_ptr, d_sigma, table, d_target, d_denom, out=None):
    from pdg.lib import lib, stream_handle
    if out is None:
        out = torch.full_like(d_sigma, -7.0)
    lib.pdg_mean_correct(d_ptr.numel() - 1, d_ptr.data_ptr(), d_sigma.data_ptr(), table.data_ptr(),
                         d_target.data_ptr(), d_denom.data_ptr() if d_denom is not None else None, out.data_ptr(),
                         stream_handle(d_sigma.device))
    return out


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


@pytest.mark.parametrize("c", [1, 3, 9])
def test_sums_against_the_restatement(case, c):
    want, mag = case.ref[c]
    got_t = _wmean(case.d_ptr, case.rows(c), case.d_w)
    got = got_t.cpu().numpy()
    bound = 2.0 * case.n_g()[:, None] * U * mag
    err = np.abs(got - want)
    print(f"n_cols={c}: max err / bound {np.max(err[bound > 0] / bound[bound > 0]):.3e}, W {got[:, 0].tolist()}")
    assert np.all(err <= bound)
    assert not got[case.EMPTY].any() and not got[case.DEAD].any()      # W = 0, sums 0: exact zeros
    # two calls agree bitwise
    assert torch.equal(_bits(_wmean(case.d_ptr, case.rows(c), case.d_w)), _bits(got_t))
    # each graph alone gets its batch row bitwise
    rows = case.rows(c)
    for g in range(case.B):
        n0, n1 = int(case.ptr[g]), int(case.ptr[g + 1])
        if n1 == n0:
            continue
        alone = _wmean(torch.tensor([0, n1 - n0], dtype=torch.int32, device="cuda"), rows[n0:n1].contiguous(),
                       case.d_w[n0:n1].contiguous())
        assert torch.equal(_bits(alone[0]), _bits(got_t[g])), g
    # the rows that take no part change nothing, whatever they hold
    x2 = rows.clone()
    x2[torch.from_numpy(case.excluded).cuda()] = float("nan")
    x2[int(case.ptr[case.DEAD]):] = float("inf")
    assert torch.equal(_bits(_wmean(case.d_ptr, x2, case.d_w)), _bits(got_t))


def test_null_weights_are_ones(case):
    rows = case.rows(3)
    none = _wmean(case.d_ptr, rows, None)
    ones = _wmean(case.d_ptr, rows, torch.ones(case.N, dtype=torch.float32, device="cuda"))
    assert torch.equal(_bits(none), _bits(ones))
    want, mag = R.graph_wmean(case.ptr, case.x[:, :3], None)
    assert np.all(np.abs(none.cpu().numpy() - want) <= 2.0 * case.n_g()[:, None] * U * mag)
    assert none[:, 0].cpu().numpy().tolist() == case.n_g().tolist()


# ------------------------------------------------------------------------------------------ mean correction
@pytest.mark.parametrize("convention", R.CONVENTIONS)
def test_correction_against_the_restatement(case, convention):
    sigma = case.x[:, :3]
    d_sigma = case.rows(3)
    table = _wmean(case.d_ptr, d_sigma, case.d_w)
    cellwise = convention == "cell"
    got_t = _correct(case.d_ptr, d_sigma, table, case.d_target, case.d_cell if cellwise else None)
    got = got_t.cpu().numpy()
    want, shift = R.mean_correct(case.ptr, sigma, case.ref[3][0], case.target, case.cell if cellwise else None)
    live = np.repeat(np.isfinite(shift).all(1), np.diff(case.ptr))
    assert live.sum() == case.N - 7 and np.isnan(shift[case.EMPTY]).all() and np.isnan(shift[case.DEAD]).all()
    err = np.abs(got[live].astype(np.float64) - want[live])
    bound = 2.0 ** -23 * (np.abs(sigma[live].astype(np.float64)) + np.abs(np.repeat(shift, np.diff(case.ptr), 0)[live]))
    print(f"{convention}: max err / bound {np.max(err / bound):.3e}")
    assert np.all(err <= bound)
    # the graph without a participating node: NaN rows; every other row finite, the excluded ones shifted too
    assert np.isnan(got[~live]).all() and np.isfinite(got[live]).all()
    assert np.all(got[case.excluded] != sigma[case.excluded])

    # the corrected field's average, taken by a second pdg_graph_wmean, is the target
    t2 = _wmean(case.d_ptr, got_t, case.d_w).cpu().numpy()
    _, mag1 = case.ref[3]
    _, mag2 = R.graph_wmean(case.ptr, np.where(np.isfinite(got), got, 0.0), case.w)
    for g in range(case.B):
        if g in (case.EMPTY, case.DEAD):
            continue
        D = case.cell[g] if cellwise else t2[g, 0]
        n = float(case.ptr[g + 1] - case.ptr[g])
        t = case.target[g].astype(np.float64)
        tol = 2.0 ** -24 * mag2[g, 1:] / D + 2.0 * (n + 3.0) * U * (mag1[g, 1:] / D + mag2[g, 1:] / D + np.abs(t))
        miss = np.abs(t2[g, 1:] / D - t)
        print(f"  graph {g}: |<sigma'> - t| / tol {np.max(miss / tol):.3e}")
        assert np.all(miss <= tol), g

    # out may alias sigma
    inplace = d_sigma.clone()
    _correct(case.d_ptr, inplace, table, case.d_target, case.d_cell if cellwise else None, out=inplace)
    assert torch.equal(_bits(inplace), _bits(got_t))
    # a graph's rows do not depend on its neighbours: the last plate alone
    g = 3
    n0, n1 = int(case.ptr[g]), int(case.ptr[g + 1])
    p1 = torch.tensor([0, n1 - n0], dtype=torch.int32, device="cuda")
    s1, w1 = d_sigma[n0:n1].contiguous(), case.d_w[n0:n1].contiguous()
    alone = _correct(p1, s1, _wmean(p1, s1, w1), case.d_target[g:g + 1].contiguous(),
                     case.d_cell[g:g + 1].contiguous() if cellwise else None)
    assert torch.equal(_bits(alone), _bits(got_t[n0:n1]))


def test_both_launches_replay_from_a_captured_graph(case):
    from pdg.lib import lib, stream_handle
    d_sigma = case.rows(3)
    eager_t = _wmean(case.d_ptr, d_sigma, case.d_w)
    eager_o = _correct(case.d_ptr, d_sigma, eager_t, case.d_target, case.d_cell)
    table = torch.full((case.B, 4), -7.0, dtype=torch.float64, device="cuda")
    out = torch.full_like(d_sigma, -7.0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = stream_handle(d_sigma.device)
        lib.pdg_graph_wmean(case.B, case.d_ptr.data_ptr(), d_sigma.data_ptr(), 3, case.d_w.data_ptr(), table.data_ptr(), s)
        lib.pdg_mean_correct(case.B, case.d_ptr.data_ptr(), d_sigma.data_ptr(), table.data_ptr(),
                             case.d_target.data_ptr(), case.d_cell.data_ptr(), out.data_ptr(), s)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(table), _bits(eager_t)) and torch.equal(_bits(out), _bits(eager_o))


def test_python_layer_is_the_two_launches(case):
    from gnn_local_stress import homogenise as H
    from pdg.lib import lib
    d_sigma = case.rows(3)
    table = _wmean(case.d_ptr, d_sigma, case.d_w)
    ptr = torch.from_numpy(case.ptr)
    avg = H.graph_average(case.d_x, ptr, case.d_w, case.d_cell)
    t9 = _wmean(case.d_ptr, case.d_x, case.d_w)
    assert torch.equal(avg.total_weight, t9[:, 0]) and torch.equal(avg.integral, t9[:, 1:])
    assert avg.integral.shape == (case.B, 9) and avg.integral.dtype == torch.float64
    assert torch.equal(_bits(avg.mean_cell), _bits(t9[:, 1:] / case.d_cell[:, None]))
    assert torch.equal(_bits(avg.mean_material), _bits(t9[:, 1:] / t9[:, :1]))
    assert torch.equal(avg.fraction, t9[:, 0] / case.d_cell)
    assert torch.isnan(avg.mean_material[case.EMPTY]).all() and torch.isnan(avg.mean_material[case.DEAD]).all()
    one = H.graph_average(case.d_x[:, 0], ptr, case.d_w)
    assert one.integral.shape == (case.B, 1) and one.mean_cell is None and one.fraction is None
    for convention in H.CONVENTIONS:
        denom = case.d_cell if convention == "cell" else None
        want = _correct(case.d_ptr, d_sigma, table, case.d_target, denom)
        calls, names = lib.calls, []
        lib.hook = names.append
        try:
            got = H.enforce_mean(d_sigma, ptr, case.d_target, convention, case.d_w, case.d_cell)
        finally:
            lib.hook = None
        assert names == ["pdg_graph_wmean", "pdg_mean_correct"] and lib.calls == calls + 2
        assert got.dtype == torch.float32 and torch.equal(_bits(got), _bits(want))
        d = H.mean_defect(d_sigma, ptr, case.d_target, convention, case.d_w, case.d_cell)
        mean = table[:, 1:] / (case.d_cell[:, None] if denom is not None else table[:, :1])
        assert d.dtype == torch.float64 and torch.equal(_bits(d), _bits(mean - case.d_target.double()))
    with pytest.raises(ValueError, match="needs the cell's area"):
        H.enforce_mean(d_sigma, ptr, case.d_target, "cell", case.d_w)
    with pytest.raises(ValueError, match="one value per graph"):
        H.enforce_mean(d_sigma, ptr, case.d_target, "cell", case.d_w, case.d_cell[:2])
    with pytest.raises(ValueError, match="weights for"):
        H.graph_average(d_sigma, ptr, case.d_w[:5])


# ------------------------------------------------------------------------------------------------ model level
@pytest.fixture(scope="module")
def served():
    from gnn_local_stress.models import EncodeProcessDecode
    s = _plate(13, 0.2)
    torch.manual_seed(69)
    stats = {k: torch.tensor(v) for k, v in {"mean_pos": 50.0, "std_pos": 29.0, "mean_mean_stress": 0.0,
                                             "std_mean_stress": 60.0, "mean_local_stress": 0.0,
                                             "std_local_stress": 60.0, "mean_edge_weight": 9.0,
                                             "std_edge_weight": 4.0}.items()}
    model = EncodeProcessDecode(input_edges_features_size=1, message_passing_steps=3, latent_size=128,
                                input_nodes_features_size=6, output_nodes_features_size=3, **stats).to("cuda")
    model.eval()
    return s, model


def test_graphs_and_batches_carry_the_areas(served):
    from pdg import graph, meshgen
    from pdg.devgraph import convert_mesh_to_graph
    s, _ = served
    t = _plate(9)
    plain = convert_mesh_to_graph(*_dev(s.pos, s.faces), s.mean_stress)
    assert plain.node_area is None and plain.cell_area is None            # the default changes nothing
    gs = [convert_mesh_to_graph(*_dev(p.pos, p.faces), p.mean_stress, torch.from_numpy(p.node_types), areas=True)
          for p in (s, t)]
    want, wbox = meshgen.nodal_areas(s.pos, s.faces)
    _check_areas(gs[0].node_area.cpu().numpy(), want, "graph.node_area")
    b = graph.Batch.from_data_list(gs)
    assert b.node_area.shape == (s.num_nodes + t.num_nodes,) and b.node_area.dtype == torch.float32
    assert b.cell_area.shape == (2,) and b.cell_area.dtype == torch.float64
    assert torch.equal(b.node_area, torch.cat([g.node_area for g in gs]))
    assert torch.equal(b[1].cell_area, gs[1].cell_area) and torch.equal(b[1].node_area, gs[1].node_area)
    b2 = graph.Batch.from_data_list([gs[0], plain])
    assert b2.node_area is None and b2.cell_area is None


def test_mean_localisation_is_the_average_of_the_localisation_tensor(served):
    from gnn_local_stress import homogenise as H
    from gnn_local_stress.sensitivity import localisation_tensor, mean_localisation
    from pdg import graph
    from pdg.devgraph import convert_mesh_to_graph
    s, model = served
    t = _plate(9)
    b = graph.Batch.from_data_list(
        [convert_mesh_to_graph(*_dev(p.pos, p.faces), p.mean_stress, torch.from_numpy(p.node_types), areas=True)
         for p in (s, t)]).to("cuda")
    N = s.num_nodes + t.num_nodes
    A = localisation_tensor(model, b)
    avg = H.graph_average(A.reshape(N, 9), b)
    M = mean_localisation(model, b)
    assert M.shape == (2, 3, 3) and M.dtype == torch.float64 and torch.isfinite(M).all()
    assert torch.equal(_bits(M.reshape(2, 9)), _bits(avg.mean_cell))
    Mm = mean_localisation(model, b, convention="material")
    assert torch.equal(_bits(Mm.reshape(2, 9)), _bits(avg.mean_material))
    # explicit weights and cell areas are the batch's own
    assert torch.equal(_bits(mean_localisation(model, b, weights=b.node_area, cell_area=b.cell_area)), _bits(M))


@pytest.mark.parametrize("convention", R.CONVENTIONS)
def test_predict_mesh_enforces_the_mean(served, convention):
    from gnn_local_stress import homogenise as H
    from gnn_local_stress.inference import predict_mesh
    from pdg import meshgen
    from pdg.devgraph import convert_mesh_to_graph
    s, model = served
    with torch.no_grad():
        ref = model(convert_mesh_to_graph(*_dev(s.pos, s.faces), s.mean_stress)).local_stress
    plain = predict_mesh(model, (s.pos, s.faces), s.mean_stress)
    assert torch.equal(plain.local_stress, ref) and plain.node_area is None    # the default stays bitwise
    out = predict_mesh(model, (s.pos, s.faces), s.mean_stress, enforce_mean=convention)
    assert out.local_stress.shape == ref.shape and out.local_stress.dtype == torch.float32
    assert out.node_area.shape == (s.num_nodes,) and out.cell_area.shape == (1,)
    assert torch.equal(_bits(out.local_stress), _bits(H.enforce_mean(ref, out, convention=convention)))
    shift = (out.local_stress.double() - ref.double())
    assert float(shift.abs().max()) > 0
    d = H.mean_defect(out.local_stress, out, convention=convention).cpu().numpy()[0]
    before = H.mean_defect(ref, out, convention=convention).cpu().numpy()[0]
    w, box = meshgen.nodal_areas(s.pos, s.faces)
    ptr = np.array([0, s.num_nodes])
    t1, mag1 = R.graph_wmean(ptr, ref.cpu().numpy(), w)
    _, mag2 = R.graph_wmean(ptr, out.local_stress.cpu().numpy(), w)
    D = float(out.cell_area) if convention == "cell" else t1[0, 0]
    t = s.mean_stress.astype(np.float64)
    n = float(s.num_nodes)
    tol = 2.0 ** -24 * mag2[0, 1:] / D + 2.0 * (n + 3.0) * U * (mag1[0, 1:] / D + mag2[0, 1:] / D + np.abs(t))
    print(f"{convention}: defect before {before}, after {d}, |after| / tol {np.max(np.abs(d) / tol):.3e}")
    assert np.all(np.abs(d) <= tol)
