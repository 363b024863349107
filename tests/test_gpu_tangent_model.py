"""gnn_local_stress.sensitivity.input_tangents / localisation_tensor (the Jacobian-vector product of the HIP
forward with respect to mean_stress, pos and edge_attr) against torch.func.jvp of the float64 oracle evaluated
in the GPU forward's own relu region (gpu_common.capture_forward + gpu_relu_masks + ReluRegion(masks=...)): the
tangent pass uses exactly those masks.

Gate (the project's, tests/test_gpu_ingrad_model.py): d_local_stress within max(3e-5, 2 x the fp32 oracle's own
JVP distance to fp64) in relative L2, local_stress within 1e-5.  Every comparison is printed (pytest -s) with
both distances, the margins to the bound on record.  Cases and builders as in tests/test_gpu_ingrad_model.py."""
import pytest
import torch

from gpu_common import capture_forward, dataset_stats, gpu_relu_masks, make_batch, rel

pytestmark = pytest.mark.gpu

OUT_TOL = 1e-5
TAN_TOL = 3e-5


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
    """(batch, stats, seeded directions for mean_stress, pos, edge_attr, a seeded cotangent u)."""
    if kind not in _batches:
        b = _single_batch() if kind == "single" else _ragged_batch()
        gen = torch.Generator().manual_seed(31)
        dirs = tuple(torch.randn(t.shape, generator=gen).cuda() for t in (b.mean_stress, b.pos, b.edge_attr))
        u = torch.randn(b.num_nodes, 3, generator=gen).cuda()
        _batches[kind] = (b, {k: float(v) for k, v in dataset_stats(b).items()}, dirs, u)
    return _batches[kind]


def _oracle_jvp(params, stats, b, dirs, steps, dtype, scale_output, scale_input, masks):
    """(y, J dirs) of the oracle in `dtype` inside the relu region `masks`."""
    from oracle import epd_oracle as O
    P = {k: v.detach().cpu().to(dtype) for k, v in params.items()}
    st = {k: torch.as_tensor(v).cpu().to(dtype) for k, v in stats.items()}
    prim = tuple(t.detach().cpu().to(dtype) for t in (b.mean_stress, b.pos, b.edge_attr))
    tang = tuple(t.detach().cpu().to(dtype) for t in dirs)
    nt, ei = b.nodes_types.cpu(), b.edge_index.cpu()

    def f(ms, pos, ea):
        return O.epd_forward(P, st, pos, ms, nt, ei, ea, steps, scale_output=scale_output, scale_input=scale_input,
                             region=O.ReluRegion(masks=masks))
    y, dy = torch.func.jvp(f, prim, tang)
    return y.detach(), dy.detach()


def _tangent_and_refs(model, b, stats, dirs, steps, scale_output, scale_input):
    from gnn_local_stress.sensitivity import input_tangents
    cap = capture_forward(model)
    t = input_tangents(model, b, d_mean_stress=dirs[0], d_pos=dirs[1], d_edge_attr=dirs[2],
                       scale_output=scale_output, scale_input=scale_input)
    masks = gpu_relu_masks(cap["ctx"])
    params = model.state_dict()
    y64, d64 = _oracle_jvp(params, stats, b, dirs, steps, torch.float64, scale_output, scale_input, masks)
    _, d32 = _oracle_jvp(params, stats, b, dirs, steps, torch.float32, scale_output, scale_input, masks)
    return t, y64, d64, d32


def _check(case, t, y64, d64, d32):
    ey, e, e32 = rel(t.local_stress, y64), rel(t.d_local_stress, d64), rel(d32, d64)
    print(case, f"local_stress {ey:.2e} (bound {OUT_TOL:.0e}); d_local_stress {e:.2e}, fp32 oracle {e32:.2e} "
                f"(rule max({TAN_TOL}, 2 x fp32 vs fp64) = {max(TAN_TOL, 2 * e32):.2e})")
    assert ey < OUT_TOL, (case, ey)
    assert e <= max(TAN_TOL, 2 * e32), (case, e, e32)


@pytest.mark.parametrize("scale_input", [True, False])
@pytest.mark.parametrize("scale_output", [True, False])
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("kind", ["single", "ragged"])
def test_input_tangents_match_oracle_fp32_and_fp64(kind, steps, scale_output, scale_input):
    b, stats, dirs, _ = _batch(kind)
    model = _model(steps, stats)
    t, y64, d64, d32 = _tangent_and_refs(model, b, stats, dirs, steps, scale_output, scale_input)
    assert t.d_local_stress.shape == (b.num_nodes, 3) and t.local_stress.shape == (b.num_nodes, 3)
    _check(f"tangent:{kind}:s{steps}:o{int(scale_output)}:i{int(scale_input)}", t, y64, d64, d32)


def _dot(a, b):
    return float((a.double().cpu().reshape(-1) * b.double().cpu().reshape(-1)).sum())


def _norm(*ts):
    return float(sum(float(t.double().cpu().pow(2).sum()) for t in ts) ** 0.5)


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("kind", ["single", "ragged"])
def test_adjoint_identity_with_input_gradients(kind, steps):
    """|<u, J v> - <J^T u, v>| <= 3e-5 (|u| |J v| + |J^T u| |v|): what the two per-output gates imply by
    Cauchy-Schwarz."""
    from gnn_local_stress.sensitivity import input_gradients, input_tangents
    b, stats, dirs, u = _batch(kind)
    model = _model(steps, stats)
    t = input_tangents(model, b, d_mean_stress=dirs[0], d_pos=dirs[1], d_edge_attr=dirs[2])
    g = input_gradients(model, b, u)
    gs = (g.mean_stress, g.pos, g.edge_attr)
    lhs, rhs = _dot(u, t.d_local_stress), sum(_dot(gi, di) for gi, di in zip(gs, dirs))
    bound = TAN_TOL * (_norm(u) * _norm(t.d_local_stress) + _norm(*gs) * _norm(*dirs))
    print(f"adjoint:{kind}:s{steps} <u, Jv> {lhs:.6e} <JTu, v> {rhs:.6e} diff {abs(lhs - rhs):.2e} bound {bound:.2e}")
    assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("kind", ["single", "ragged"])
def test_localisation_tensor(kind):
    """Column j is bitwise input_tangents(d_load=e_j); contracted with a cotangent it meets input_gradients' load
    under the adjoint bound.  The graph LayerNorm's statistics span the whole batch, so the graphs of a batch are
    coupled: with the cotangent u restricted to graph g, sum_{n in g} u[n, i] A[n, i, j] = <u_g, J (e_j on every
    graph)> = sum over all graphs g' of load_{u_g}[g', j] (one graph: load[graph, j] itself)."""
    from gnn_local_stress.sensitivity import input_gradients, input_tangents, localisation_tensor
    b, stats, _, u = _batch(kind)
    model = _model(2, stats)
    A = localisation_tensor(model, b)
    N, B = b.num_nodes, b.ptr.numel() - 1
    assert A.shape == (N, 3, 3)
    for j in range(3):
        e = torch.zeros(B, 3, device="cuda")
        e[:, j] = 1.0
        assert torch.equal(A[:, :, j], input_tangents(model, b, d_load=e).d_local_stress), j
    ptr = b.ptr.tolist()
    for gi in range(B):
        ug = torch.zeros_like(u)
        ug[ptr[gi]:ptr[gi + 1]] = u[ptr[gi]:ptr[gi + 1]]
        g = input_gradients(model, b, ug)
        for j in range(3):
            lhs, rhs = _dot(ug, A[:, :, j]), float(g.load[:, j].double().sum())
            bound = TAN_TOL * (_norm(ug) * _norm(A[:, :, j]) + _norm(g.mean_stress) * N ** 0.5)
            print(f"localisation:{kind} graph {gi} column {j}: {lhs:.6e} vs {rhs:.6e} diff {abs(lhs - rhs):.2e} "
                  f"bound {bound:.2e}")
            assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("kind", ["single", "ragged"])
def test_chain_edge_lengths_equals_explicit_edge_direction(kind):
    from gnn_local_stress.sensitivity import input_tangents
    from tangent_ref import edge_len_tan_ref
    b, stats, dirs, _ = _batch(kind)
    model = _model(2, stats)
    dlen = edge_len_tan_ref(b.edge_index[0], b.edge_index[1], b.pos, dirs[1], b.edge_attr)
    assert float(dlen.abs().max()) > 0 and int((b.edge_attr.reshape(-1) == 0).sum()) > 0   # periodic pairs present
    t1 = input_tangents(model, b, d_pos=dirs[1], chain_edge_lengths=True)
    t2 = input_tangents(model, b, d_pos=dirs[1], d_edge_attr=dlen.float().view(b.edge_attr.shape).cuda())
    t0 = input_tangents(model, b, d_pos=dirs[1])
    e = rel(t1.d_local_stress, t2.d_local_stress)
    print(f"chain_edge_lengths:{kind} {e:.2e} (bound {TAN_TOL}); the chained part is "
          f"{rel(t0.d_local_stress, t2.d_local_stress):.2e} of the tangent")
    assert e <= TAN_TOL
    assert rel(t0.d_local_stress, t2.d_local_stress) > 100 * TAN_TOL   # the edge lengths matter in this case
    with pytest.raises(ValueError, match="d_pos"):
        input_tangents(model, b, d_load=torch.ones(b.ptr.numel() - 1, 3, device="cuda"), chain_edge_lengths=True)


def test_d_load_is_the_broadcast_mean_stress_direction():
    from gnn_local_stress.sensitivity import input_tangents
    b, stats, dirs, _ = _batch("ragged")
    model = _model(2, stats)
    B = b.ptr.numel() - 1
    d_load = torch.randn(B, 3, generator=torch.Generator().manual_seed(32)).cuda()
    counts = (b.ptr[1:] - b.ptr[:-1]).cpu()
    per_node = torch.repeat_interleave(d_load.cpu(), counts, dim=0).cuda()
    t1 = input_tangents(model, b, d_load=d_load, d_mean_stress=dirs[0])
    t2 = input_tangents(model, b, d_mean_stress=dirs[0] + per_node)
    assert torch.equal(t1.d_local_stress, t2.d_local_stress)


def test_properties_of_one_call():
    """A second call is bitwise the same; two tangent passes on one forward do not disturb each other;
    parameters' .grad stay None; works under no_grad; the autograd route still refuses; CPU tensors, wrong
    shapes and no direction raise; sync mode is refused by the engine."""
    from gnn_local_stress.sensitivity import input_tangents
    from pdg.engine import PARAM_NAMES
    b, stats, dirs, _ = _batch("ragged")
    model = _model(2, stats)
    kw = dict(d_mean_stress=dirs[0], d_pos=dirs[1], d_edge_attr=dirs[2])
    t1 = input_tangents(model, b, **kw)
    with torch.no_grad():
        t2 = input_tangents(model, b, **kw)
    for k in ("local_stress", "d_local_stress"):
        assert torch.equal(getattr(t1, k), getattr(t2, k)), k
        assert not getattr(t1, k).requires_grad
    assert all(p.grad is None for p in model.parameters())
    # one forward, passes A, B, A again on its context: ctx is only read
    cap = capture_forward(model)
    input_tangents(model, b, d_pos=dirs[1])
    ctx, eng = cap["ctx"], model._engine_for(torch.device("cuda:0"))
    P = {n: model.get_parameter(n).detach() for n in PARAM_NAMES}
    P["_std_local_stress"] = model.stats_tensor(torch.device("cuda:0"))[5:6]
    N, E = ctx.plan.n_nodes, ctx.plan.n_edges
    gen = torch.Generator().manual_seed(33)
    xa, ea = torch.randn(N, 6, generator=gen).cuda(), torch.randn(E, generator=gen).cuda()
    xb, eb = torch.randn(N, 6, generator=gen).cuda(), torch.zeros(E).cuda()
    ya = eng.tangent(P, ctx, xa, ea)
    yb = eng.tangent(P, ctx, xb, eb)
    ya2 = eng.tangent(P, ctx, xa, ea)
    assert torch.equal(ya, ya2) and not torch.equal(ya, yb)
    # linear: J (a + b) = J a + J b to rounding
    yab = eng.tangent(P, ctx, xa + xb, ea + eb)
    assert rel(yab, ya + yb) < 1e-5
    eng.sync = ("group", N, E)
    try:
        with pytest.raises(ValueError, match="sync"):
            eng.tangent(P, ctx, xa, ea)
    finally:
        eng.sync = None
    with pytest.raises(ValueError, match="at least one"):
        input_tangents(model, b)
    with pytest.raises(RuntimeError, match="HIP"):
        input_tangents(model, b, d_pos=dirs[1].cpu())
    with pytest.raises(ValueError, match="shape"):
        input_tangents(model, b, d_pos=dirs[1][:-1])
    with pytest.raises(ValueError, match="shape"):
        input_tangents(model, b, d_load=torch.ones(1, 3, device="cuda"))
    bb, _, _, _ = _batch("single")
    bb.pos = bb.pos.clone().requires_grad_(True)
    try:
        with pytest.raises(NotImplementedError, match="pos"):
            model(bb)
        assert input_tangents(model, bb, d_load=torch.ones(1, 3, device="cuda")).d_local_stress.shape == (bb.num_nodes, 3)
    finally:
        bb.pos = bb.pos.detach()


def test_cpu_batch_raises():
    from gnn_local_stress.sensitivity import input_tangents, localisation_tensor
    from pdg import graph, meshgen
    b = graph.Batch.from_data_list([graph.sample_to_data(meshgen.hole_plate(9, seed=2))])
    _, stats, _, _ = _batch("single")
    model = _model(1, stats)
    with pytest.raises(RuntimeError, match="HIP"):
        input_tangents(model, b, d_pos=torch.zeros(b.pos.shape))
    with pytest.raises(RuntimeError, match="HIP"):
        localisation_tensor(model, b)


def test_zero_stress_guard_gives_zeros():
    from gnn_local_stress.sensitivity import input_tangents, localisation_tensor
    from pdg import meshgen
    b = make_batch([meshgen.hole_plate(9, seed=2)])
    b.mean_stress = torch.zeros_like(b.mean_stress)
    model = _model(2, {k: 1.0 for k in ("mean_pos", "std_pos", "mean_mean_stress", "std_mean_stress",
                                        "mean_local_stress", "std_local_stress", "mean_edge_weight",
                                        "std_edge_weight")})
    t = input_tangents(model, b, d_load=torch.ones(1, 3, device="cuda"))
    assert t.local_stress.shape == (b.num_nodes, 3) and t.d_local_stress.shape == (b.num_nodes, 3)
    assert float(t.local_stress.abs().max()) == 0.0 and float(t.d_local_stress.abs().max()) == 0.0
    A = localisation_tensor(model, b)
    assert A.shape == (b.num_nodes, 3, 3) and float(A.abs().max()) == 0.0


def test_edgeless_batch():
    """No edge: no edge launch, the aggregate tangent is zero, the node directions against fp64."""
    from gnn_local_stress.sensitivity import input_tangents
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
    gen = torch.Generator().manual_seed(34)
    dirs = (torch.randn(b.mean_stress.shape, generator=gen).cuda(), torch.randn(b.pos.shape, generator=gen).cuda(),
            torch.zeros(b.edge_attr.shape).cuda())
    cap = capture_forward(model)
    names = []
    lib.hook = names.append
    try:
        t = input_tangents(model, b, d_mean_stress=dirs[0], d_pos=dirs[1], d_edge_attr=dirs[2])
    finally:
        lib.hook = None
    assert "pdg_node_net_tan" in names and "pdg_decoder_tan" in names
    assert not {"pdg_edge_tan", "pdg_edge_enc_tan", "pdg_segment_sum_tan"} & set(names)
    masks = gpu_relu_masks(cap["ctx"])
    y64, d64 = _oracle_jvp(model.state_dict(), stats, b, dirs, 3, torch.float64, True, True, masks)
    _, d32 = _oracle_jvp(model.state_dict(), stats, b, dirs, 3, torch.float32, True, True, masks)
    _check("tangent:edgeless", t, y64, d64, d32)
