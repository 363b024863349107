"""Node labels and the P1 divergence operator built on the device (csrc/pdg_meshfields.hip) against
their host restatements (pdg.meshgen.node_labels, pdg.meshgen.p1_divergence_operator), and the
bare-mesh serving path built on them (devgraph.convert_mesh_to_graph without labels,
inference.predict_mesh).

Operator values: both sides add the same fp64 terms and round the sum once to fp32; they differ only
in the order of the additions.  A term is at most max|vals| in size and an entry has a handful of
them, so the fp64 sums differ by ~1e-15 max|vals|: after rounding, by at most one fp32 ulp of the
entry (<= 2^-23 |host|) where the sum is of normal size, and by the fp64 noise itself where the terms
cancel (a structural zero) -- the 1e-9 max|vals| term, far above it."""
import numpy as np
import pytest
import torch

from test_meshfields_host import PLATES, plate, renumbered, two_hole_plate

pytestmark = pytest.mark.gpu


def _dev(pos, faces):
    return (torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float32)).cuda(),
            torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int64)).cuda())


def _labels_and_info(pos, faces):
    """pdg_node_labels itself: (labels, info) as numpy, no exception for any status."""
    from pdg.lib import lib, stream_handle
    pts, fcs = _dev(pos, faces)
    n, dim = pts.shape
    nbytes = lib.pdg_mesh_fields_scratch_bytes(n, len(fcs))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    labels = torch.full((n,), 99, dtype=torch.int64, device="cuda")
    info = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    lib.pdg_node_labels(n, pts.data_ptr(), dim, len(fcs), fcs.data_ptr(), labels.data_ptr(), info.data_ptr(),
                        scratch.data_ptr(), nbytes, stream_handle(pts.device))
    return labels.cpu().numpy(), info.cpu().numpy().tolist()


def _check_labels(pos, faces):
    from pdg import meshgen
    from pdg.devgraph import node_labels
    want, ncomp, next_ = meshgen.node_labels(pos, faces)
    got, info = _labels_and_info(pos, faces)
    assert info == [ncomp, next_, 0]
    assert np.array_equal(got, want)
    lab = node_labels(*_dev(pos, faces), strict=False)
    assert lab.dtype == torch.int64 and lab.is_cuda and np.array_equal(lab.cpu().numpy(), want)
    return want


@pytest.mark.parametrize("n,hole", PLATES)
@pytest.mark.parametrize("jitter", [True, False])
@pytest.mark.parametrize("periodic", [True, False])
def test_labels_are_the_host_restatement(n, hole, jitter, periodic):
    s = plate(n, hole, jitter, periodic)
    want = _check_labels(s.pos, s.faces)
    assert np.array_equal(want, s.node_types)


@pytest.mark.parametrize("n,hole,nodes", [(186, 0.29, 25556), (160, 0.3, 18440)])
def test_labels_of_the_published_mesh_size(n, hole, nodes):
    """The published sweep's largest plate (25,556 nodes: hole_plate(186, 0.29), bench.py PUBLISHED_SWEEP)
    and hole_plate(160, 0.3): many scan blocks, ~1,000 boundary nodes in the component search."""
    s = plate(n, hole)
    assert s.num_nodes == nodes
    assert np.array_equal(_check_labels(s.pos, s.faces), s.node_types)


def test_labels_with_three_dimensional_points_and_renumbering():
    s = plate(24, 0.3)
    pts3 = np.concatenate([s.pos, np.random.default_rng(1).uniform(-1, 1, (s.num_nodes, 1)).astype(np.float32)], 1)
    assert np.array_equal(_check_labels(pts3, s.faces), s.node_types)
    pos2, faces2, perm = renumbered(s.pos, s.faces)
    assert np.array_equal(_check_labels(pos2, faces2)[perm], s.node_types)
    # a node of no face, on the bounding box, stays 0
    pos = np.concatenate([s.pos, np.array([[200.0, 200.0]], np.float32)])
    assert _check_labels(pos, s.faces)[-1] == 0


def test_strict_mode_is_the_two_region_assertion():
    from pdg.devgraph import node_labels
    s = plate(24, 0.3)
    assert np.array_equal(node_labels(*_dev(s.pos, s.faces)).cpu().numpy(), s.node_types)   # strict by default
    solid = plate(9, 0.0)
    with pytest.raises(ValueError, match="Expected 2 regions"):
        node_labels(*_dev(solid.pos, solid.faces))
    assert np.array_equal(_check_labels(solid.pos, solid.faces), solid.node_types)
    pos, faces, rims = two_hole_plate()
    with pytest.raises(ValueError, match="Expected 2 regions"):
        node_labels(*_dev(pos, faces), strict=True)
    lab = _check_labels(pos, faces)
    assert set(np.where(lab == -1)[0].tolist()) == rims[0] | rims[1]


def test_bow_tie_is_a_non_manifold_boundary():
    from pdg.devgraph import node_labels
    pos = np.array([[0, 0], [1, 0], [0, 1], [-1, 0], [0, -1]], np.float32)
    faces = np.array([[0, 1, 2], [0, 3, 4]], np.int64)
    for strict in (True, False):
        with pytest.raises(ValueError, match="non-manifold"):
            node_labels(*_dev(pos, faces), strict=strict)
    got, info = _labels_and_info(pos, faces)
    assert info == [1, 1, 2] and np.array_equal(got, np.ones(5, np.int64))   # labels are still written


def test_out_of_range_face_is_ignored_and_reported():
    from pdg.devgraph import node_labels, p1_divergence
    s = plate(9, 0.25)
    n = s.num_nodes
    faces = np.concatenate([s.faces, np.array([[0, 1, n], [-1, 2, 3]], np.int64)])
    with pytest.raises(ValueError, match="outside"):
        node_labels(*_dev(s.pos, faces))
    with pytest.raises(ValueError, match="outside"):
        p1_divergence(*_dev(s.pos, faces))
    got, info = _labels_and_info(s.pos, faces)
    assert info == [2, 1, 1] and np.array_equal(got, s.node_types)          # the mesh without those faces
    assert np.array_equal(node_labels(*_dev(s.pos, s.faces)).cpu().numpy(), s.node_types)   # and the process goes on


@pytest.mark.parametrize("n,hole,jitter", [(9, 0.25, True), (24, 0.3, True), (71, 0.2, True), (24, 0.3, False)])
def test_operator_is_the_host_operator(n, hole, jitter):
    from pdg import meshgen
    from pdg.devgraph import p1_divergence
    s = plate(n, hole, jitter)
    rows, cols, vals = meshgen.p1_divergence_operator(s.pos, s.faces)
    op = p1_divergence(*_dev(s.pos, s.faces))
    assert op.is_coalesced() and op.shape == (s.num_nodes, 2 * s.num_nodes) and op.dtype == torch.float32
    idx = op.indices().cpu().numpy()
    assert idx.dtype == np.int64 and np.array_equal(idx[0], rows) and np.array_equal(idx[1], cols)
    got = op.values().cpu().numpy().astype(np.float64)
    want = vals.astype(np.float64)
    err = np.abs(got - want)
    bound = 2.0 ** -23 * np.abs(want) + 1e-9 * np.abs(want).max()
    print(f"n={n} nnz={len(want)} max err {err.max():.3e} max err/bound {np.max(err / bound):.3e} "
          f"bitwise equal {np.mean(got == want):.4f}")
    assert np.all(err <= bound)
    # the same mesh renumbered: the same operator, permuted
    pos2, faces2, perm = renumbered(s.pos, s.faces)
    r2, c2, v2 = meshgen.p1_divergence_operator(pos2, faces2)
    op2 = p1_divergence(*_dev(pos2, faces2))
    i2 = op2.indices().cpu().numpy()
    assert np.array_equal(i2[0], r2) and np.array_equal(i2[1], c2)
    e2 = np.abs(op2.values().cpu().numpy().astype(np.float64) - v2)
    assert np.all(e2 <= 2.0 ** -23 * np.abs(v2) + 1e-9 * np.abs(v2).max())


def test_operator_skips_a_degenerate_face():
    from pdg import meshgen
    from pdg.lib import lib, stream_handle
    s = plate(9, 0.25)
    faces = np.concatenate([s.faces, np.array([[0, 1, 1]], np.int64)])     # zero area
    pts, fcs = _dev(s.pos, faces)
    n, nf = s.num_nodes, len(faces)
    nbytes = lib.pdg_mesh_fields_scratch_bytes(n, nf)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    idx = torch.empty(2, 18 * nf, dtype=torch.int64, device="cuda")
    vals = torch.empty(18 * nf, dtype=torch.float32, device="cuda")
    cnt = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    lib.pdg_p1_div_operator(n, pts.data_ptr(), 2, nf, fcs.data_ptr(), idx[0].data_ptr(), idx[1].data_ptr(),
                            vals.data_ptr(), 18 * nf, cnt.data_ptr(), cnt[1:].data_ptr(), scratch.data_ptr(), nbytes,
                            stream_handle(pts.device))
    nnz, status = cnt.tolist()
    rows, cols, want = meshgen.p1_divergence_operator(s.pos, s.faces)
    assert status == 1 and nnz == len(rows)
    assert np.array_equal(idx[0, :nnz].cpu().numpy(), rows) and np.array_equal(idx[1, :nnz].cpu().numpy(), cols)
    assert np.all(np.abs(vals[:nnz].cpu().numpy().astype(np.float64) - want)
                  <= 2.0 ** -23 * np.abs(want) + 1e-9 * np.abs(want).max())


@pytest.fixture(scope="module")
def served():
    """A 456-node plate, a model, and the current path's prediction from hole_plate's labels."""
    from gnn_local_stress.models import EncodeProcessDecode
    from pdg.devgraph import convert_mesh_to_graph
    s = plate(25, 0.3005, seed=4)
    assert s.num_nodes == 456
    torch.manual_seed(69)
    stats = {k: torch.tensor(v) for k, v in {"mean_pos": 50.0, "std_pos": 29.0, "mean_mean_stress": 0.0,
                                             "std_mean_stress": 60.0, "mean_local_stress": 0.0,
                                             "std_local_stress": 60.0, "mean_edge_weight": 9.0,
                                             "std_edge_weight": 4.0}.items()}
    model = EncodeProcessDecode(input_edges_features_size=1, message_passing_steps=3, latent_size=128,
                                input_nodes_features_size=6, output_nodes_features_size=3, **stats).to("cuda")
    model.eval()
    pts, fcs = _dev(s.pos, s.faces)
    with torch.no_grad():
        ref = model(convert_mesh_to_graph(pts, fcs, s.mean_stress, torch.from_numpy(s.node_types))).local_stress
    return s, model, ref


def test_graph_without_labels_feeds_the_model(served):
    from pdg.devgraph import convert_mesh_to_graph
    s, model, ref = served
    pts, fcs = _dev(s.pos, s.faces)
    g = convert_mesh_to_graph(pts, fcs, s.mean_stress)
    assert np.array_equal(g.nodes_types.cpu().numpy().ravel(), s.node_types) and g.op_div_matrix is None
    with torch.no_grad():
        assert torch.equal(model(g).local_stress, ref)
    assert convert_mesh_to_graph(pts, fcs, s.mean_stress, divergence=True).op_div_matrix.shape == (456, 912)


def test_predict_mesh_from_a_vtk_file(served, tmp_path):
    from gnn_local_stress import losses, vtk_io
    from gnn_local_stress.inference import predict_mesh
    from pdg import graph
    s, model, ref = served
    path = tmp_path / "plate.vtk"
    vtk_io.write_legacy_vtk(path, s.pos, s.faces, point_type="float")
    out = predict_mesh(model, path, s.mean_stress)
    assert torch.equal(out.local_stress, ref)
    assert np.array_equal(out.nodes_types.cpu().numpy().ravel(), s.node_types)
    out2, div = predict_mesh(model, (s.pos, s.faces), s.mean_stress, divergence=True)
    assert torch.equal(out2.local_stress, ref)
    host_op = graph.sample_to_data(s).op_div_matrix.cuda()
    want = losses.compute_divergence(ref, host_op, torch.from_numpy(s.node_types).cuda().reshape(-1, 1))
    assert float(want) > 0
    assert abs(float(div) - float(want)) <= 1e-5 * abs(float(want))
    quads = np.array([[0, 1, 26, 25]], np.int64)
    with pytest.raises(ValueError, match="triangle"):
        predict_mesh(model, (s.pos, quads), s.mean_stress)
