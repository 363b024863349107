"""gnn_local_stress.sensitivity.criterion_gradients: the sensitivity of a stress criterion's per-graph aggregate in
one call (one engine forward, the two criterion launches, one engine backward), against the same quantity put
together from the separate public calls, and against the tangent pass through the adjoint identity.

That input_gradients itself is unchanged by the split of its body is gated by the untouched
tests/test_gpu_ingrad_model.py (values against the oracle and the reference's fixture) and
tests/test_gpu_engine_launches.py (the engine's launch sequences); here its launch sequence is compared with the
one criterion_gradients runs around the two criterion launches."""
import pytest
import torch

from gpu_common import dataset_stats, make_batch

pytestmark = pytest.mark.gpu

TAN_TOL = 3e-5     # tests/test_gpu_tangent_model.py::test_adjoint_identity_with_input_gradients
FIELDS = ("local_stress", "mean_stress", "pos", "edge_attr", "load")
CASES = [("von_mises", "pnorm"), ("tresca", "ks"), ("rankine", "max"), ("von_mises", "mean")]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _model(steps, stats):
    from gnn_local_stress.models import EncodeProcessDecode
    torch.manual_seed(69)
    m = EncodeProcessDecode(input_edges_features_size=1, message_passing_steps=steps, latent_size=128,
                            input_nodes_features_size=6, output_nodes_features_size=3,
                            **{k: torch.as_tensor(v).float() for k, v in stats.items()})
    return m.to("cuda")


_cache = {}


def _batch():
    """(a 2-graph hole-plate batch, its statistics, participation weights with zeros, one rho for its stresses)."""
    if not _cache:
        from pdg import meshgen
        b = make_batch([meshgen.hole_plate(9, hole_radius=0.2, seed=4), meshgen.hole_plate(12, hole_radius=0.25, seed=6)])
        stats = {k: float(v) for k, v in dataset_stats(b).items()}
        gen = torch.Generator().manual_seed(5)
        w = torch.rand(b.num_nodes, generator=gen) + 0.5
        w[torch.rand(b.num_nodes, generator=gen) < 0.2] = 0.0
        _cache["b"] = (b, stats, w.cuda(), 4.0 / float(b.local_stress.abs().max()))
    return _cache["b"]


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32).cpu()


def _dot(a, b):
    return float((a.double().cpu().reshape(-1) * b.double().cpu().reshape(-1)).sum())


def _norm(*ts):
    return float(sum(float(t.double().cpu().pow(2).sum()) for t in ts) ** 0.5)


@pytest.mark.parametrize("steps,criterion,aggregate", [(2, c, a) for c, a in CASES] + [(10, "tresca", "pnorm")])
def test_one_call_equals_the_separate_calls_bitwise(steps, criterion, aggregate):
    from gnn_local_stress import criteria as C
    from gnn_local_stress.sensitivity import criterion_gradients, input_gradients
    b, stats, w, rho = _batch()
    model = _model(steps, stats)
    gv = torch.tensor([2.0, -0.75], device="cuda")
    kw = dict(weights=w, p=6.0, rho=rho)
    got = criterion_gradients(model, b, criterion, aggregate, g_value=gv, **kw)
    y = model(b).local_stress.detach()       # the training-mode forward, the one both sensitivity calls run
    gy = C.graph_criterion_grad(y, b, criterion, aggregate, g_value=gv, **kw)
    ref = input_gradients(model, b, gy)
    assert torch.equal(_bits(got.grad_output), _bits(gy))
    for k in FIELDS:
        assert torch.equal(_bits(getattr(got, k)), _bits(getattr(ref, k))), k
        assert not getattr(got, k).requires_grad
    assert float(got.grad_output.abs().max()) > 0 and float(got.load.abs().max()) > 0
    assert (got.grad_output[w == 0] == 0).all()
    # value and argmax are graph_criterion's of the returned field
    c = C.graph_criterion(got.local_stress, b, criterion, **kw)
    assert got.value.dtype == torch.float64 and torch.equal(_bits(got.value), _bits(getattr(c, aggregate)))
    assert torch.equal(got.argmax, c.argmax) and (got.argmax >= 0).all() and torch.isfinite(got.value).all()
    assert all(p.grad is None for p in model.parameters())


def test_launch_sequence_is_input_gradients_plus_the_two_criterion_launches():
    from gnn_local_stress.sensitivity import criterion_gradients, input_gradients
    from pdg.lib import lib
    b, stats, w, rho = _batch()
    model = _model(2, stats)
    got = criterion_gradients(model, b, "von_mises", "pnorm", weights=w)      # warm: plan and engine built
    one, two = [], []
    lib.hook = one.append
    try:
        criterion_gradients(model, b, "von_mises", "pnorm", weights=w)
        lib.hook = two.append
        input_gradients(model, b, got.grad_output)
    finally:
        lib.hook = None
    i = one.index("pdg_stress_criteria")
    assert one[i:i + 2] == ["pdg_stress_criteria", "pdg_stress_criteria_bwd"]
    assert one[:i] + one[i + 2:] == two and two[-1] == "pdg_graph_colsum3"
    assert "pdg_stress_criteria" not in two


@pytest.mark.parametrize("criterion,aggregate", CASES)
def test_adjoint_identity_with_the_tangent_pass(criterion, aggregate):
    """sum_g <load[g], dSigma_g> = sum_n <grad_output(n), d_local_stress(n)> for d_local_stress the tangent of
    d_load = dSigma, under the bound of test_adjoint_identity_with_input_gradients: 3e-5 (|u| |J v| + |J^T u| |v|)
    with u = grad_output, v = dSigma broadcast to the nodes and J^T u = the mean_stress gradient."""
    from gnn_local_stress.sensitivity import criterion_gradients, input_tangents
    b, stats, w, rho = _batch()
    model = _model(2, stats)
    d_load = torch.randn(2, 3, generator=torch.Generator().manual_seed(9)).cuda()
    g = criterion_gradients(model, b, criterion, aggregate, weights=w, p=6.0, rho=rho)
    t = input_tangents(model, b, d_load=d_load)
    counts = (b.ptr[1:] - b.ptr[:-1]).to("cuda")
    v = torch.repeat_interleave(d_load, counts, dim=0)
    lhs, rhs = _dot(g.load, d_load), _dot(g.grad_output, t.d_local_stress)
    bound = TAN_TOL * (_norm(g.grad_output) * _norm(t.d_local_stress) + _norm(g.mean_stress) * _norm(v))
    print(f"adjoint:{criterion}:{aggregate} <load, dSigma> {lhs:.6e} <gy, J dSigma> {rhs:.6e} "
          f"diff {abs(lhs - rhs):.2e} bound {bound:.2e}")
    assert torch.equal(_bits(t.local_stress), _bits(g.local_stress))
    assert lhs != 0.0 and abs(lhs - rhs) <= bound


def test_standardised_field_without_scale_output():
    """scale_output=False: the criterion is evaluated on the standardised field the model then returns."""
    from gnn_local_stress import criteria as C
    from gnn_local_stress.sensitivity import criterion_gradients
    b, stats, w, _ = _batch()
    model = _model(2, stats)
    got = criterion_gradients(model, b, "tresca", "mean", weights=w, scale_output=False)
    y = model(b, scale_output=False).local_stress.detach()
    assert torch.equal(_bits(got.local_stress), _bits(y))
    assert torch.equal(_bits(got.value), _bits(C.graph_criterion(y, b, "tresca", weights=w).mean))
    assert torch.equal(_bits(got.grad_output), _bits(C.graph_criterion_grad(y, b, "tresca", "mean", weights=w)))


def test_zero_stress_guard_gives_zero_gradients_and_a_zero_fields_values():
    from gnn_local_stress.sensitivity import criterion_gradients
    from pdg import meshgen
    b = make_batch([meshgen.hole_plate(9, seed=2)])
    b.mean_stress = torch.zeros_like(b.mean_stress)
    model = _model(2, {k: 1.0 for k in ("mean_pos", "std_pos", "mean_mean_stress", "std_mean_stress",
                                        "mean_local_stress", "std_local_stress", "mean_edge_weight",
                                        "std_edge_weight")})
    for aggregate in ("max", "mean", "pnorm", "ks"):
        g = criterion_gradients(model, b, "von_mises", aggregate, rho=1.0)
        for k in FIELDS + ("grad_output",):
            assert float(getattr(g, k).abs().max()) == 0.0, k
        assert g.value.shape == (1,) and float(g.value[0]) == 0.0 and int(g.argmax[0]) == 0
        assert g.edge_attr.shape == b.edge_attr.shape and g.load.shape == (1, 3)


def test_cpu_batch_and_bad_names_raise():
    from gnn_local_stress.sensitivity import criterion_gradients
    b, stats, w, rho = _batch()
    model = _model(2, stats)
    with pytest.raises(RuntimeError, match="HIP"):
        criterion_gradients(model, b.to("cpu"), "von_mises", "pnorm")
    with pytest.raises(RuntimeError, match="HIP"):
        criterion_gradients(model, b, "von_mises", "pnorm", weights=w.cpu())
    with pytest.raises(ValueError, match="max, mean, pnorm, ks"):
        criterion_gradients(model, b, "von_mises", "p-norm")
    with pytest.raises(ValueError, match="needs rho"):
        criterion_gradients(model, b, "von_mises", "ks")
