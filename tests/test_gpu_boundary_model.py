"""The model-level entry points of the boundary residuals: convert_mesh_to_graph(..., boundary=True) and Batch carry
the vectors, predict_mesh(..., boundary=True) returns the residuals of its own prediction, and
sensitivity.boundary_gradients is one forward, the two boundary launches and one backward, checked against the
separate public calls and, through the adjoint identity, against the tangent pass."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TAN_TOL = 3e-5     # tests/test_gpu_tangent_model.py::test_adjoint_identity_with_input_gradients


def _plate(n, hole=0.0, seed=3):
    from pdg import meshgen
    return meshgen.hole_plate(n=n, hole_radius=hole, seed=seed)


def _dev(pos, faces):
    return (torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float32)).cuda(),
            torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)).cuda())


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32).cpu()


def _dot(a, b):
    return float((a.double().cpu().reshape(-1) * b.double().cpu().reshape(-1)).sum())


def _norm(*ts):
    return float(sum(float(t.double().cpu().pow(2).sum()) for t in ts) ** 0.5)


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


@pytest.fixture(scope="module")
def batch(served):
    from pdg import graph
    from pdg.devgraph import convert_mesh_to_graph
    s, _ = served
    t = _plate(9, 0.25, seed=4)
    gs = [convert_mesh_to_graph(*_dev(p.pos, p.faces), p.mean_stress, torch.from_numpy(p.node_types), boundary=True)
          for p in (s, t)]
    return gs, graph.Batch.from_data_list(gs).to("cuda")


def test_graphs_and_batches_carry_the_vectors(served, batch):
    from pdg import graph, meshgen
    from pdg.devgraph import convert_mesh_to_graph
    s, _ = served
    gs, b = batch
    plain = convert_mesh_to_graph(*_dev(s.pos, s.faces), s.mean_stress)
    assert plain.boundary_vec is None and plain.boundary_len is None          # the default changes nothing
    assert sorted(plain.keys()) == sorted(k for k in gs[0].keys() if not k.startswith("boundary_"))
    want_v, want_l = meshgen.boundary_vectors(s.pos, s.faces)
    got_v, got_l = gs[0].boundary_vec.cpu().numpy(), gs[0].boundary_len.cpu().numpy()
    assert np.all(np.abs(got_v.astype(np.float64) - want_v) <= 2.0 ** -23 * np.abs(want_v.astype(np.float64)))
    assert np.all(np.abs(got_l.astype(np.float64) - want_l) <= 2.0 ** -23 * np.abs(want_l.astype(np.float64)))
    n = sum(g.num_nodes for g in gs)
    assert b.boundary_vec.shape == (n, 2) and b.boundary_vec.dtype == torch.float32
    assert b.boundary_len.shape == (n,) and b.boundary_len.dtype == torch.float32
    assert torch.equal(b.boundary_vec, torch.cat([g.boundary_vec for g in gs]))
    assert torch.equal(b[1].boundary_len, gs[1].boundary_len) and torch.equal(b[1].boundary_vec, gs[1].boundary_vec)
    b2 = graph.Batch.from_data_list([gs[0], plain])
    assert b2.boundary_vec is None and b2.boundary_len is None
    # the vectors vanish off the boundary and the labels agree with them
    on = gs[0].nodes_types.reshape(-1) != 0
    assert bool((gs[0].boundary_len[on] > 0).all()) and not gs[0].boundary_len[~on].any()


def test_predict_mesh_returns_the_residuals_of_its_own_prediction(served):
    from gnn_local_stress import boundary as Bd
    from gnn_local_stress.inference import predict_mesh
    s, model = served
    plain = predict_mesh(model, (s.pos, s.faces), s.mean_stress)
    out = predict_mesh(model, (s.pos, s.faces), s.mean_stress, boundary=True)
    assert isinstance(out, tuple) and len(out) == 2
    data, res = out
    assert torch.equal(_bits(data.local_stress), _bits(plain.local_stress)) and plain.boundary_vec is None
    assert data.boundary_vec.shape == (s.num_nodes, 2) and data.boundary_len.shape == (s.num_nodes,)
    want = Bd.boundary_residuals(data.local_stress, data)
    for k in ("L_int", "L_ext", "T2", "F_int", "F_ext", "P2", "n_pairs", "traction_rms", "traction_max",
              "periodic_rms", "argmax", "node"):
        assert torch.equal(_bits(getattr(res, k)), _bits(getattr(want, k))), k
    assert float(res.traction_rms) > 0 and float(res.periodic_rms) > 0 and int(res.argmax) >= 0
    assert float(res.n_pairs) == 2 * 13 + 2
    print(f"untrained model: traction rms {float(res.traction_rms):.4e}, max {float(res.traction_max):.4e}, "
          f"hole force {res.hole_force.tolist()}, cell force {res.cell_force.tolist()}, "
          f"periodic rms {float(res.periodic_rms):.4e}")
    three = predict_mesh(model, (s.pos, s.faces), s.mean_stress, divergence=True, boundary=True)
    two = predict_mesh(model, (s.pos, s.faces), s.mean_stress, divergence=True)
    assert len(three) == 3 and len(two) == 2
    assert torch.equal(_bits(three[0].local_stress), _bits(plain.local_stress))
    assert torch.equal(_bits(three[1]), _bits(two[1])) and torch.equal(_bits(three[2].T2), _bits(res.T2))
    # a non-periodic graph has no jump: 0 / 0 stays NaN
    _, free = predict_mesh(model, (s.pos, s.faces), s.mean_stress, periodic=False, boundary=True)
    assert float(free.n_pairs) == 0 and torch.isnan(free.periodic_rms).all() and float(free.traction_rms) > 0


@pytest.mark.parametrize("traction,periodic", [(1.0, 0.0), (0.0, 1.0), (0.6, "tensor")])
def test_boundary_gradients_is_the_separate_calls(served, batch, traction, periodic):
    from gnn_local_stress import boundary as Bd
    from gnn_local_stress.sensitivity import boundary_gradients, input_gradients
    _, model = served
    _, b = batch
    if periodic == "tensor":
        periodic = torch.tensor([1.5, -0.25], device="cuda")
    before = [None if p.grad is None else p.grad.clone() for p in model.parameters()]
    got = boundary_gradients(model, b, traction=traction, periodic=periodic)
    gy = Bd.boundary_residuals_grad(got.local_stress, b, traction=traction, periodic=periodic)
    assert torch.equal(_bits(got.grad_output), _bits(gy)) and float(gy.abs().max()) > 0
    ref = input_gradients(model, b, gy)
    for k in ("local_stress", "mean_stress", "pos", "edge_attr", "load"):
        assert torch.equal(_bits(getattr(got, k)), _bits(getattr(ref, k))), k
        assert not getattr(got, k).requires_grad
    r = Bd.boundary_residuals(got.local_stress, b)
    gt = torch.as_tensor(traction, dtype=torch.float64, device="cuda").expand(2)
    gp = torch.as_tensor(periodic, dtype=torch.float64, device="cuda").expand(2)
    want = torch.where(gt == 0, torch.zeros_like(gt), gt * r.T2 / r.L_int) \
        + torch.where(gp == 0, torch.zeros_like(gp), gp * r.P2 / r.n_pairs)
    assert got.value.shape == (2,) and got.value.dtype == torch.float64 and torch.equal(_bits(got.value), _bits(want))
    for p, g0 in zip(model.parameters(), before):
        assert (p.grad is None) if g0 is None else torch.equal(p.grad, g0)
    # where the zero-stress guard fires every gradient is zero
    z = b.to("cuda")
    z.mean_stress = torch.zeros_like(b.mean_stress)
    gz = boundary_gradients(model, z, traction=traction, periodic=periodic)
    for k in ("local_stress", "mean_stress", "pos", "edge_attr", "load", "grad_output"):
        assert not getattr(gz, k).any(), k


def test_adjoint_identity_with_the_tangent_pass(served, batch):
    """sum_g <load[g], dSigma_g> = sum_n <grad_output(n), d_local_stress(n)> for d_local_stress the tangent of
    d_load = dSigma, under the bound of test_adjoint_identity_with_input_gradients: 3e-5 (|u| |J v| + |J^T u| |v|)
    with u = grad_output, v = dSigma broadcast to the nodes and J^T u = the mean_stress gradient."""
    from gnn_local_stress.sensitivity import boundary_gradients, input_tangents
    _, model = served
    _, b = batch
    d_load = torch.randn(2, 3, generator=torch.Generator().manual_seed(9)).cuda()
    s = boundary_gradients(model, b, traction=1.0, periodic=0.5)
    t = input_tangents(model, b, d_load=d_load)
    counts = (b.ptr[1:] - b.ptr[:-1]).to("cuda")
    v = torch.repeat_interleave(d_load, counts, dim=0)
    lhs, rhs = _dot(s.load, d_load), _dot(s.grad_output, t.d_local_stress)
    bound = TAN_TOL * (_norm(s.grad_output) * _norm(t.d_local_stress) + _norm(s.mean_stress) * _norm(v))
    print(f"adjoint: <load, dSigma> {lhs:.6e} <gy, J dSigma> {rhs:.6e} diff {abs(lhs - rhs):.2e} bound {bound:.2e}")
    assert torch.equal(_bits(t.local_stress), _bits(s.local_stress))
    assert lhs != 0.0 and abs(lhs - rhs) <= bound
