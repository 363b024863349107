"""The Python layer of the sampling operator (gnn_local_stress/sampling.py, predict_mesh(sample=), sensitivity.
sample_gradients) on hole_plate(13, 0.2) and the quad plate, against the host restatement (tests/sample_ref.py) and
against the entry points it is composed of.  Bounds as in tests/test_gpu_sample.py: a sample differs from the nodal
interpolant by at most 2^-24 |want| + sum_k wb |f_k| + nv u sum |w f|, wb the weights' bound of the kernel's own cell."""
import numpy as np
import pytest
import torch

import sample_ref as R
from gpu_common import dataset_stats, make_batch
from test_gpu_sample import E32, U, _wbound

pytestmark = pytest.mark.gpu

TAN_TOL = 3e-5   # tests/test_gpu_tangent_model.py's, for the same identity


def _sample(kind):
    from pdg import meshgen
    return meshgen.hole_plate(13, 0.2) if kind == "tri" else meshgen.quad_hole_plate(13, 0.2)


_kept = {}


def _setup(kind):
    """(sample, batch on the device, model, locator), once per kind; the model seeded as the model tests seed theirs."""
    if kind not in _kept:
        from gnn_local_stress.models import EncodeProcessDecode
        from gnn_local_stress.sampling import PointLocator
        s = _sample(kind)
        b = make_batch([s])
        torch.manual_seed(69)
        stats = {k: float(v) for k, v in dataset_stats(b).items()}
        m = EncodeProcessDecode(input_edges_features_size=1, message_passing_steps=2, latent_size=128,
                                input_nodes_features_size=6, output_nodes_features_size=3,
                                **{k: torch.as_tensor(v).float() for k, v in stats.items()}).cuda()
        loc = PointLocator(torch.from_numpy(s.pos).cuda(), torch.from_numpy(s.faces).cuda())
        _kept[kind] = (s, b, m, loc)
    return _kept[kind]


def _slack(s, cell, field):
    """sum_k (wb + 2^-24) |f_k| over the nodes of ``cell``: what the weights' errors can move a sample by."""
    nodes = s.faces[cell]
    return (_wbound(s.pos[nodes].astype(np.float64)) + E32) * np.abs(field[nodes]).sum(0)


@pytest.mark.parametrize("kind", ["tri", "quad"])
def test_line_profile_endpoints_on_nodes_reproduce_the_nodal_values(kind):
    from gnn_local_stress.sampling import line_profile
    s, _, _, loc = _setup(kind)
    field = torch.from_numpy(s.local_stress).cuda()
    i, j = 3, s.num_nodes - 5
    dist, xy, v = line_profile(loc, field, s.pos[i], s.pos[j], n=50)
    assert xy.shape == (50, 2) and v.shape == (50, 3) and dist.shape == (50,)
    assert np.array_equal(xy[0].cpu().numpy(), s.pos[i]) and np.array_equal(xy[-1].cpu().numpy(), s.pos[j])
    assert float(dist[0]) == 0.0 and abs(float(dist[-1]) - np.linalg.norm(s.pos[j] - s.pos[i])) <= 1e-4
    ends = loc.locate(xy[[0, -1]]).cell.cpu().numpy()
    for row, node, cell in ((0, i, ends[0]), (-1, j, ends[1])):
        assert cell >= 0 and node in s.faces[cell]
        want = s.local_stress[node].astype(np.float64)
        got = v[row].cpu().numpy().astype(np.float64)
        assert (np.abs(got - want) <= E32 * np.abs(want) + _slack(s, cell, s.local_stress)).all(), (row, got, want)
    one = line_profile(loc, field[:, 0].contiguous(), s.pos[i], s.pos[j], n=50)[2]
    assert one.shape == (50,) and torch.equal(one.nan_to_num(1e9), v[:, 0].nan_to_num(1e9))


@pytest.mark.parametrize("kind", ["tri", "quad"])
def test_raster_holds_fill_exactly_where_the_restatement_sees_no_cell(kind):
    from gnn_local_stress.sampling import raster, raster_points
    s, _, _, loc = _setup(kind)
    field = torch.from_numpy(s.local_stress).cuda()
    nx, ny = 24, 17
    pts = raster_points(loc, nx, ny)
    cell, _ = R.locate(s.pos, s.faces, pts.cpu().numpy())
    hole = (cell < 0).reshape(ny, nx)
    assert 0 < hole.sum() < nx * ny / 2
    img = raster(loc, field, nx, ny, fill=-9.0)
    assert img.shape == (ny, nx, 3)
    assert np.array_equal((img.cpu().numpy() == -9.0).all(-1), hole)
    assert np.array_equal(torch.isnan(raster(loc, field, nx, ny)).all(-1).cpu().numpy(), hole)
    assert raster(loc, field[:, 1].contiguous(), nx, ny).shape == (ny, nx)
    # pixel (row 0, column 0) is the lower left corner's, half a pixel inside the box
    bb = R.bbox_of(s.pos).astype(np.float64)
    assert np.allclose(pts[0].cpu().numpy(), [bb[0] + (bb[2] - bb[0]) / nx / 2, bb[1] + (bb[3] - bb[1]) / ny / 2])


def test_transfer_field_of_a_linear_field_between_two_meshes_of_the_sweep():
    """hole_plate(13, 0.2) -> the nodes of hole_plate(24, 0.3): the linear field is reproduced where the coarse
    plate has material.  The coarse plate lacks every cell with a vertex inside its hole, so its material ends up to
    one coarse cell beyond the radius and some of the finer plate's rim nodes lie in no coarse cell: they give -1,
    as many as the restatement counts."""
    from gnn_local_stress.sampling import transfer_field
    from pdg import meshgen
    src, dst = meshgen.hole_plate(13, 0.2), meshgen.hole_plate(24, 0.3)
    lin = lambda p: 3.0 + 0.25 * p[:, 0] - 0.5 * p[:, 1]   # noqa: E731
    f = lin(src.pos.astype(np.float64)).astype(np.float32)
    got, plan = transfer_field(torch.from_numpy(src.pos).cuda(), torch.from_numpy(src.faces).cuda(),
                               torch.from_numpy(f).cuda(), torch.from_numpy(dst.pos).cuda(), return_plan=True)
    assert got.shape == (dst.num_nodes,)
    cell = plan.cell.cpu().numpy()
    ref_cell, _ = R.locate(src.pos, src.faces, dst.pos)
    assert int((cell < 0).sum()) == int((ref_cell < 0).sum()) and np.array_equal(cell < 0, ref_cell < 0)
    assert int(plan.n_outside.item()) == int((ref_cell < 0).sum())
    want = lin(dst.pos.astype(np.float64))
    g = got.cpu().numpy().astype(np.float64)
    assert np.isnan(g[cell < 0]).all()
    for q in np.nonzero(cell >= 0)[0]:
        tol = E32 * abs(want[q]) + _slack(src, cell[q], f[:, None])[0] + 3 * U * np.abs(f[src.faces[cell[q]]]).sum()
        assert abs(g[q] - want[q]) <= tol, (q, g[q], want[q], tol)


@pytest.mark.parametrize("kind", ["tri", "quad"])
def test_predict_mesh_sample_attaches_the_samples_and_changes_nothing_else(kind):
    from gnn_local_stress.inference import predict_mesh
    from gnn_local_stress.sampling import sample_field
    s, _, model, _ = _setup(kind)
    rng = np.random.default_rng(21)
    xy = rng.uniform(-10, 110, size=(300, 2)).astype(np.float32)
    plain = predict_mesh(model, (s.pos, s.faces), s.mean_stress, cells="any")
    data = predict_mesh(model, (s.pos, s.faces), s.mean_stress, cells="any", sample=xy)
    assert type(data) is type(plain) and torch.equal(data.local_stress, plain.local_stress)
    assert "samples" not in plain.__dict__ and "sample_plan" not in plain.__dict__ and data.samples.shape == (300, 3)
    again = sample_field(data.local_stress, data.sample_plan)
    assert torch.equal(data.samples.isnan(), again.isnan())
    assert torch.equal(data.samples.nan_to_num(0.0), again.nan_to_num(0.0))
    # the mesh is periodic by default: points beyond the cell are wrapped into it, only the hole gives NaN
    ref_cell, _ = R.locate(s.pos, s.faces, xy, periodic=True)
    assert np.array_equal(data.sample_plan.cell.cpu().numpy() < 0, ref_cell < 0) and (ref_cell < 0).any()
    assert np.array_equal(data.samples.isnan().all(1).cpu().numpy(), ref_cell < 0)
    # the other return shapes are the ones without `sample`
    d0, div0 = predict_mesh(model, (s.pos, s.faces), s.mean_stress, divergence=True, cells="any")
    d1, div1 = predict_mesh(model, (s.pos, s.faces), s.mean_stress, divergence=True, cells="any", sample=xy[:7])
    assert torch.equal(d0.local_stress, d1.local_stress) and torch.equal(div0, div1) and d1.samples.shape == (7, 3)
    with pytest.raises(TypeError):
        predict_mesh(model, (s.pos, s.faces), s.mean_stress, True, False, None, False, "any", xy)   # keyword only


@pytest.mark.parametrize("kind", ["tri", "quad"])
def test_sample_gradients_is_input_gradients_of_the_transposed_cotangent(kind):
    """Bitwise input_gradients(model, batch, S^T g), with the samples of the same forward; and the adjoint identity
    <g, S (J d)> = <J^T S^T g, d> against input_tangents for one random load direction d, with the tolerance of
    tests/test_gpu_tangent_model.py's adjoint test, 3e-5 (|u| |J d| + |J^T u| |d|) for u = S^T g, plus S's own
    rounding 2 * 2^-24 sum |g| |S J d| (S and S^T use the same fp32 weights)."""
    from gnn_local_stress.sampling import sample_field, sample_field_grad
    from gnn_local_stress.sensitivity import input_gradients, input_tangents, sample_gradients
    s, b, model, loc = _setup(kind)
    gen = torch.Generator().manual_seed(35)
    xy = (torch.rand(200, 2, generator=gen) * 120 - 10).cuda()
    g = torch.randn(200, 3, generator=gen).cuda()
    d = torch.randn(1, 3, generator=gen).cuda()
    plan = loc.locate(xy)
    assert 0 < int(plan.n_outside.item()) < 200
    sg = sample_gradients(model, b, plan, g)
    u = sample_field_grad(g, plan)
    ref = input_gradients(model, b, u)
    for name in ("local_stress", "mean_stress", "pos", "edge_attr", "load"):
        assert torch.equal(getattr(sg, name), getattr(ref, name)), name
    assert torch.equal(sg.grad_output, u)
    mine = sample_field(ref.local_stress, plan)
    assert torch.equal(sg.samples.isnan(), mine.isnan()) and torch.equal(sg.samples.nan_to_num(0), mine.nan_to_num(0))
    assert all(p.grad is None for p in model.parameters())
    t = input_tangents(model, b, d_load=d)
    sjd = sample_field(t.d_local_stress, plan, fill=0.0).double()
    lhs = float((g.double() * sjd).sum())
    rhs = float((sg.load.double() * d.double()).sum())
    norm = lambda x: float(x.double().norm())   # noqa: E731
    bound = TAN_TOL * (norm(u) * norm(t.d_local_stress) + norm(sg.load) * norm(d)) \
        + 2 * E32 * float((g.double().abs() * sjd.abs()).sum())
    print(f"adjoint:{kind} <g, S J d> {lhs:.6e} <JT ST g, d> {rhs:.6e} diff {abs(lhs - rhs):.2e} bound {bound:.2e}")
    assert abs(lhs - rhs) <= bound
