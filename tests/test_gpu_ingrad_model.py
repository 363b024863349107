"""gnn_local_stress.sensitivity.input_gradients (the explicit vector-Jacobian product of the HIP forward with
respect to mean_stress, pos and edge_attr) against the oracle's autograd in float64.

Gate (the one tests/test_gpu_model.py::test_training_step_matches_oracle_fp32_and_fp64 uses): every gradient
within max(3e-5, 2 x the fp32 oracle's own distance to fp64) in relative L2, local_stress within 1e-5.  Every
comparison is printed (pytest -s) with both distances, the margins to the bound on record."""
import numpy as np
import pytest
import torch

from golden_io import GOLDEN
from gpu_common import dataset_stats, golden_batch, make_batch, rel

pytestmark = pytest.mark.gpu

OUT_TOL = 1e-5
GRAD_TOL = 3e-5
FIELDS = ("mean_stress", "pos", "edge_attr")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _model(steps, stats, params=None):
    from gnn_local_stress.models import EncodeProcessDecode
    torch.manual_seed(69)
    m = EncodeProcessDecode(input_edges_features_size=1, message_passing_steps=steps, latent_size=128,
                            input_nodes_features_size=6, output_nodes_features_size=3,
                            **{k: torch.as_tensor(v).float() for k, v in stats.items()})
    if params is not None:
        m.load_state_dict(params)
    return m.to("cuda")


def _oracle(params, stats, b, gy, steps, dtype, scale_output, scale_input):
    from oracle import epd_oracle as O
    P = {k: v.detach().cpu().to(dtype) for k, v in params.items()}
    st = {k: torch.as_tensor(v).cpu().to(dtype) for k, v in stats.items()}
    pos, ms, ea = (t.detach().cpu().to(dtype).requires_grad_(True) for t in (b.pos, b.mean_stress, b.edge_attr))
    y = O.epd_forward(P, st, pos, ms, b.nodes_types.cpu(), b.edge_index.cpu(), ea, steps, scale_output=scale_output,
                      scale_input=scale_input)
    if not ea.numel():
        gm, gp = torch.autograd.grad((y * gy.cpu().to(dtype)).sum(), [ms, pos])
        return y.detach(), dict(mean_stress=gm, pos=gp, edge_attr=torch.zeros_like(ea))
    gm, gp, gea = torch.autograd.grad((y * gy.cpu().to(dtype)).sum(), [ms, pos, ea])
    return y.detach(), dict(mean_stress=gm, pos=gp, edge_attr=gea)


def _ragged_batch():
    """Three graphs of unequal sizes, the first with an isolated node appended."""
    from pdg import graph, meshgen
    datas = [graph.sample_to_data(meshgen.hole_plate(n, hole_radius=r, seed=s))
             for n, r, s in ((7, 0.2, 4), (12, 0.25, 6), (9, 0.15, 8))]
    d = datas[0]
    d.pos = torch.cat([d.pos, torch.tensor([[50.0, 50.0]])])
    d.mean_stress = torch.cat([d.mean_stress, d.mean_stress[:1]])
    d.local_stress = torch.cat([d.local_stress, d.local_stress[:1]])
    d.nodes_types = torch.cat([d.nodes_types, torch.zeros(1, 1, dtype=torch.int64)])
    d.surfaces_nodes_for_div = d.nodes_types
    return graph.Batch.from_data_list(datas).to("cuda")


def _single_batch():
    from pdg import meshgen
    return make_batch([meshgen.hole_plate(9, seed=2)])


_batches = {}


def _batch(kind):
    if kind not in _batches:
        b = _single_batch() if kind == "single" else _ragged_batch()
        gy = torch.randn(b.num_nodes, 3, generator=torch.Generator().manual_seed(11)).cuda()
        _batches[kind] = (b, {k: float(v) for k, v in dataset_stats(b).items()}, gy)
    return _batches[kind]


def _check(case, g, ref64, ref32, y64):
    assert rel(g.local_stress, y64) < OUT_TOL, rel(g.local_stress, y64)
    errs = {}
    for k in FIELDS:
        got = getattr(g, k)
        assert got.shape == ref64[k].shape or got.reshape(-1).shape == ref64[k].reshape(-1).shape
        errs[k] = [rel(got.reshape(-1), ref64[k].reshape(-1)), rel(ref32[k].reshape(-1), ref64[k].reshape(-1))]
    print(case, f"rule max({GRAD_TOL}, 2 x fp32 vs fp64)", {k: [f"{e:.2e}" for e in v] for k, v in errs.items()})
    for k, (e, e32) in errs.items():
        assert e <= max(GRAD_TOL, 2 * e32), (case, k, e, e32)


@pytest.mark.parametrize("scale_input", [True, False])
@pytest.mark.parametrize("scale_output", [True, False])
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("kind", ["single", "ragged"])
def test_input_gradients_match_oracle_fp32_and_fp64(kind, steps, scale_output, scale_input):
    from gnn_local_stress.sensitivity import input_gradients
    b, stats, gy = _batch(kind)
    model = _model(steps, stats)
    g = input_gradients(model, b, gy, scale_output=scale_output, scale_input=scale_input)
    params = model.state_dict()
    y64, r64 = _oracle(params, stats, b, gy, steps, torch.float64, scale_output, scale_input)
    _, r32 = _oracle(params, stats, b, gy, steps, torch.float32, scale_output, scale_input)
    assert g.edge_attr.shape == b.edge_attr.shape and g.load.shape == (b.ptr.numel() - 1, 3)
    _check(f"ingrad:{kind}:s{steps}:o{int(scale_output)}:i{int(scale_input)}", g, r64, r32, y64)


@pytest.mark.parametrize("case", ["tiny_periodic", "batch3_div"])
def test_input_gradients_match_reference_fixture(case):
    """The reference's own autograd values (tests/golden/input_grads.npz) in the place of the fp32 oracle:
    local_stress within 1e-5 of the reference's, every gradient within max(3e-5, 2 x the reference's own
    distance to fp64) of fp64."""
    from gnn_local_stress.sensitivity import input_gradients
    g, batch = golden_batch(case)
    z = np.load(GOLDEN / "input_grads.npz", allow_pickle=False)
    t = lambda k: torch.from_numpy(z[f"{case}.{k}"])
    steps = int(g["steps"])
    model = _model(steps, g["stats"], g["params"])
    gy = t("grad_output").cuda()
    got = input_gradients(model, batch, gy)
    assert rel(got.local_stress, t("local_stress")) < OUT_TOL
    st = {k: float(v) for k, v in g["stats"].items()}
    y64, r64 = _oracle(g["params"], st, batch, gy, steps, torch.float64, True, True)
    _check(f"ingrad:golden:{case}", got, r64, {k: t(k) for k in FIELDS}, y64)


def test_properties_of_one_call():
    """load = the per-graph row sums; parameters' .grad stay None; a second call is bitwise the same; works
    under no_grad; the autograd route still refuses; CPU tensors raise."""
    from gnn_local_stress.sensitivity import input_gradients
    b, stats, gy = _batch("ragged")
    model = _model(2, stats)
    g1 = input_gradients(model, b, gy)
    with torch.no_grad():
        g2 = input_gradients(model, b, gy)
    for k in FIELDS + ("local_stress", "load"):
        assert torch.equal(getattr(g1, k), getattr(g2, k)), k
        assert not getattr(g1, k).requires_grad
    assert all(p.grad is None for p in model.parameters())
    ptr = b.ptr.tolist()
    for i in range(len(ptr) - 1):
        ref = g1.mean_stress[ptr[i]:ptr[i + 1]].double().sum(0)
        bound = 2.0 ** -24 * ref.abs() + 1e-12 * g1.mean_stress[ptr[i]:ptr[i + 1]].double().abs().sum(0)
        assert ((g1.load[i].double() - ref).abs() <= bound).all(), (i, g1.load[i], ref)
    bb, _, _ = _batch("single")
    bb.pos = bb.pos.clone().requires_grad_(True)
    try:
        with pytest.raises(NotImplementedError, match="pos"):
            model(bb)
        # the explicit route takes such inputs: they are read, never differentiated through
        assert input_gradients(model, bb, torch.ones(bb.num_nodes, 3, device="cuda")).pos.shape == bb.pos.shape
    finally:
        bb.pos = bb.pos.detach()
    with pytest.raises(RuntimeError, match="HIP"):
        input_gradients(model, b, gy.cpu())


def test_zero_stress_guard_gives_zeros():
    from gnn_local_stress.sensitivity import input_gradients
    from pdg import meshgen
    b = make_batch([meshgen.hole_plate(9, seed=2)])
    b.mean_stress = torch.zeros_like(b.mean_stress)
    model = _model(2, {k: 1.0 for k in ("mean_pos", "std_pos", "mean_mean_stress", "std_mean_stress",
                                        "mean_local_stress", "std_local_stress", "mean_edge_weight",
                                        "std_edge_weight")})
    g = input_gradients(model, b, torch.ones(b.num_nodes, 3, device="cuda"))
    for k in FIELDS + ("local_stress", "load"):
        assert float(getattr(g, k).abs().max()) == 0.0, k
    assert g.edge_attr.shape == b.edge_attr.shape and g.load.shape == (1, 3)


def test_edgeless_batch():
    """No edge: an empty edge_attr gradient, no edge launch, node gradients against fp64."""
    from gnn_local_stress.sensitivity import input_gradients
    from pdg import graph, meshgen
    from pdg.lib import lib
    datas = []
    for s in meshgen.make_dataset(2, n=9, hole_radius=(0.15, 0.25), seed=8):
        d = graph.sample_to_data(s)
        d.edge_index = d.edge_index[:, :0]
        d.edge_attr = d.edge_attr[:0]
        datas.append(d)
    b = graph.Batch.from_data_list(datas).to("cuda")
    stats = {k: float(v) for k, v in dataset_stats(b).items() if k not in ("mean_edge_weight", "std_edge_weight")}
    stats.update(mean_edge_weight=0.0, std_edge_weight=1.0)
    model = _model(3, stats)
    gy = torch.randn(b.num_nodes, 3, generator=torch.Generator().manual_seed(12)).cuda()
    names = []
    lib.hook = names.append
    try:
        g = input_gradients(model, b, gy)
    finally:
        lib.hook = None
    assert "pdg_node_enc_gin" in names and "pdg_edge_enc_gin" not in names
    assert g.edge_attr.numel() == 0 and g.edge_attr.shape == b.edge_attr.shape
    y64, r64 = _oracle(model.state_dict(), stats, b, gy, 3, torch.float64, True, True)
    _, r32 = _oracle(model.state_dict(), stats, b, gy, 3, torch.float32, True, True)
    assert rel(g.local_stress, y64) < OUT_TOL
    for k in ("mean_stress", "pos"):
        e, e32 = rel(getattr(g, k), r64[k]), rel(r32[k], r64[k])
        assert e <= max(GRAD_TOL, 2 * e32), (k, e, e32)
