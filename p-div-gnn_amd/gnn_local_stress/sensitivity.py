"""Input gradients of ``EncodeProcessDecode`` on the HIP path: an explicit vector-Jacobian product.

The reference model is a plain PyTorch module, so its users can differentiate the predicted stress
field with respect to the imposed mean stress, the node coordinates and the edge lengths (load
identification from an observed field, sensitivity of a peak stress to the load, shape sensitivities
of the hole).  The HIP ``forward`` refuses inputs that require grad (its registered autograd backward
produces parameter gradients only); this module is the supported route:

    g = input_gradients(model, batch, grad_output)
    g.mean_stress, g.pos, g.edge_attr, g.load, g.local_stress

One forward and one backward of the engine (pdg.engine) with two more launches next to the encoders'
backward (pdg_node_enc_gin, pdg_edge_enc_gin) and one per-graph reduction (pdg_graph_colsum3).

The cotangent of a peak stress depends on the forward output of the same call, so a failure criterion's
aggregate (gnn_local_stress.criteria) is differentiated in one call, with one forward:

    c = criterion_gradients(model, batch, "von_mises", "pnorm", weights=w, p=8.0)
    c.value, c.argmax, c.load, c.pos, c.grad_output

The boundary residuals (gnn_local_stress.boundary: the mean-square traction on the hole's edge and the mean-square
jump across the periodic connections) are differentiated the same way:

    s = boundary_gradients(model, batch, traction=1.0, periodic=0.0)
    s.value, s.load, s.pos, s.grad_output

The prediction at points that are not nodes (gnn_local_stress.sampling: a virtual strain gauge) takes the samples'
cotangent to the nodes with S^T first:

    v = sample_gradients(model, batch, plan, grad_samples)
    v.samples, v.load, v.pos, v.grad_output

The other direction, how the whole field moves when an input moves, is the Jacobian-vector product:

    t = input_tangents(model, batch, d_load=...)          # t.local_stress, t.d_local_stress
    A = localisation_tensor(model, batch)                 # A[n, i, j] = d sigma_i(n) / d Sigma_j
    M = mean_localisation(model, batch)                   # (B, 3, 3): the volume average of A, I when consistent

One forward and one tangent pass per direction (pdg.engine.EPDEngine.tangent, csrc/pdg_tangent.hip): the
forward linearised at its own stored activations, so the relu masks are those of the fp32 forward.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from pdg.engine import PARAM_NAMES, InputGrads
from pdg.lib import lib, stream_handle
from pdg.plan import plan_for


@dataclass
class InputGradients:
    """``local_stress`` (N, 3): the forward output of the same call.  ``mean_stress`` (N, 3), ``pos`` (N, 2),
    ``edge_attr`` (the shape of the batch's ``edge_attr``, in its edge order): d <grad_output, local_stress> /
    d input.  ``pos`` goes through the node features only: the model takes ``edge_attr`` as an independent
    input.  ``load`` (B, 3): per graph the sum of its nodes' ``mean_stress`` rows, the gradient with respect to
    that graph's imposed mean stress when it is broadcast to every node."""
    local_stress: torch.Tensor
    mean_stress: torch.Tensor
    pos: torch.Tensor
    edge_attr: torch.Tensor
    load: torch.Tensor


def input_gradients(model, mesh_graph, grad_output: torch.Tensor, scale_output: bool = True,
                    scale_input: bool = True) -> InputGradients:
    """The vector-Jacobian product of ``model.forward(mesh_graph, scale_output, scale_input).local_stress``
    with the cotangent ``grad_output`` (N, 3), with respect to ``mean_stress``, ``pos`` and ``edge_attr``
    (``nodes_types`` is an integer label and gets none).  Works with or without ``torch.no_grad()``, never
    touches a parameter's ``.grad``, and raises on CPU tensors like the rest of the HIP path.  Where the
    forward's zero-stress guard fires (models.py:294-299) the output and every gradient are zero."""
    if mesh_graph.pos.device.type != "cuda" or grad_output.device.type != "cuda":
        raise RuntimeError("input_gradients runs on the MI355X HIP path only; move the batch and grad_output to a "
                           "HIP device (the CPU restatement lives in oracle/ and is test-only)")
    _check_sizes(model)
    ms = mesh_graph.mean_stress
    if tuple(grad_output.shape) != tuple(ms.shape):
        raise ValueError(f"grad_output must have the shape of local_stress {tuple(ms.shape)}, "
                         f"got {tuple(grad_output.shape)}")
    with torch.no_grad():
        fw = _vjp_forward(model, mesh_graph, scale_output, scale_input)
        if fw.y is None:
            return _zero_gradients(fw.plan, mesh_graph.edge_attr, ms.device)
        return _vjp_backward(fw, mesh_graph.edge_attr, grad_output.detach().float().contiguous(), scale_input)


def _check_sizes(model) -> None:
    if model.input_nodes_features_size != 6 or model.input_edges_features_size != 1 \
            or model.output_nodes_features_size != 3:
        raise ValueError("HIP path supports the reference feature sizes (6 node, 1 edge, 3 outputs)")


@dataclass
class _Forward:
    """What the backward part needs of the forward part; ``y`` and ``ctx`` are None where the zero-stress guard
    fired."""
    plan: object
    eng: object
    P: dict
    stats8: torch.Tensor
    y: torch.Tensor | None
    ctx: object


def _vjp_forward(model, mesh_graph, scale_output: bool, scale_input: bool) -> _Forward:
    """The forward part of ``input_gradients``: the guard and the status word of a plan built here in one host
    read (as in forward), then the engine's need_grad forward."""
    pos, ms, edge_attr = mesh_graph.pos, mesh_graph.mean_stress, mesh_graph.edge_attr
    dev = pos.device
    s = stream_handle(dev)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    plan = plan_for(mesh_graph, status=flag[1:])
    msf = ms.detach().float().contiguous()
    lib.pdg_any_nonzero(msf.data_ptr(), msf.numel(), flag.data_ptr(), s)
    nonzero, status = flag.tolist()
    if not plan._checked:
        if plan.status.data_ptr() == flag[1:].data_ptr():
            try:
                plan.check_status(status)
            except AssertionError:
                mesh_graph.__dict__.pop("_plan_cache", None)
                raise
        else:
            plan.validate()
    if not nonzero:
        return _Forward(plan, None, {}, None, None, None)
    eng = model._engine_for(dev)
    P = {n: model.get_parameter(n).detach() for n in PARAM_NAMES}
    stats8 = model.stats_tensor(dev)
    y, ctx = eng.forward(P, stats8, plan, pos.detach().float().contiguous(), msf,
                         mesh_graph.nodes_types.reshape(-1).to(torch.int64).contiguous(),
                         edge_attr.detach().reshape(-1).float().contiguous(), model.message_passing_steps,
                         bool(scale_input), bool(scale_output), True)
    if scale_output:
        P["_std_local_stress"] = stats8[5:6]
    return _Forward(plan, eng, P, stats8, y, ctx)


def _zero_gradients(plan, edge_attr, dev) -> InputGradients:
    f32 = dict(dtype=torch.float32, device=dev)
    N, B = plan.n_nodes, plan.n_graphs
    return InputGradients(local_stress=torch.zeros(N, 3, **f32), mean_stress=torch.zeros(N, 3, **f32),
                          pos=torch.zeros(N, 2, **f32), edge_attr=torch.zeros(edge_attr.shape, **f32),
                          load=torch.zeros(B, 3, **f32))


def _vjp_backward(fw: _Forward, edge_attr, grad_output: torch.Tensor, scale_input: bool) -> InputGradients:
    """The backward part of ``input_gradients``: the engine's backward with ``input_grads`` on the forward's
    context, then the per-graph column sums (pdg_graph_colsum3)."""
    plan, P, stats8 = fw.plan, fw.P, fw.stats8
    dev = stats8.device
    f32 = dict(dtype=torch.float32, device=dev)
    N, E, B = plan.n_nodes, plan.n_edges, plan.n_graphs
    # the engine's backward fuses the weight gradients into the input-gradient chain: they land in scratch
    # accumulators that are dropped here, never in a parameter's .grad
    G = {n: torch.zeros_like(p) for n, p in P.items() if n in PARAM_NAMES}
    ig = InputGrads(mean_stress=torch.empty(N, 3, **f32), pos=torch.empty(N, 2, **f32),
                    edge_attr=torch.empty(E, **f32), stats8=stats8, scale_input=bool(scale_input))
    fw.eng.backward(P, fw.ctx, grad_output, G, input_grads=ig)
    load = torch.empty(B, 3, **f32)
    lib.pdg_graph_colsum3(B, plan.ptr.data_ptr(), ig.mean_stress.data_ptr(), load.data_ptr(), stream_handle(dev))
    return InputGradients(local_stress=fw.y, mean_stress=ig.mean_stress, pos=ig.pos,
                          edge_attr=ig.edge_attr.view(edge_attr.shape), load=load)


@dataclass
class CriterionGradients(InputGradients):
    """The fields of ``InputGradients`` for the cotangent ``grad_output`` (N, 3) = ``g_value[g]`` times the
    gradient of graph g's aggregate with respect to ``local_stress``, and ``value`` (B,) fp64, that aggregate of
    the chosen criterion over ``local_stress``, with ``argmax`` (B,) int64, the graph-local index of the first
    node that attains the criterion's maximum (-1 for a NaN graph)."""
    value: torch.Tensor = None
    argmax: torch.Tensor = None
    grad_output: torch.Tensor = None


def criterion_gradients(model, mesh_graph, criterion: str = "von_mises", aggregate: str = "pnorm", weights=None,
                        p: float = 8.0, rho: float | None = None, g_value=None, scale_output: bool = True,
                        scale_input: bool = True) -> CriterionGradients:
    """The sensitivity of a stress criterion's per-graph aggregate (``gnn_local_stress.criteria``: ``criterion``
    one of von_mises / tresca / rankine, ``aggregate`` one of max / mean / pnorm / ks, ``weights`` the
    participation weights, ``p``, ``rho``; ``aggregate='ks'`` needs ``rho``) with respect to ``mean_stress``,
    ``pos``, ``edge_attr`` and each graph's ``load``, in one call: one engine forward, the two criterion launches
    on its output (pdg_stress_criteria, pdg_stress_criteria_bwd), one engine backward with that cotangent and the
    per-graph column sums.  ``g_value`` (B,) scales each graph's cotangent (None: ones), so the gradients are
    those of sum_g g_value[g] J_g.  With ``scale_output=False`` the criterion is evaluated on the standardised
    field (local_stress - mean) / std the model then returns, not on a stress.  Where the zero-stress guard fires
    every gradient is zero and ``value`` / ``argmax`` are those of a zero field.  Works with or without
    ``torch.no_grad()``, never touches a parameter's ``.grad``, raises on CPU tensors."""
    from . import criteria as C
    cid = C._id(criterion, C.CRITERIA, "criterion")
    aid = C._aggregate_id(aggregate, rho)
    p, rho = C._check_p_rho(p, rho)
    dev = mesh_graph.pos.device
    if dev.type != "cuda":
        raise RuntimeError("criterion_gradients runs on the MI355X HIP path only; move the batch to a HIP device "
                           "(the CPU restatement lives in oracle/ and is test-only)")
    _check_sizes(model)
    with torch.no_grad():
        fw = _vjp_forward(model, mesh_graph, scale_output, scale_input)
        plan = fw.plan
        w = C._weights_of(weights, plan.n_nodes, dev)
        if fw.y is None:
            z = _zero_gradients(plan, mesh_graph.edge_attr, dev)
            table, argmax, _ = C._forward(plan.ptr, z.local_stress, w, cid, p, rho, False)
            return CriterionGradients(**vars(z), value=table[:, aid], argmax=argmax.long(),
                                      grad_output=torch.zeros_like(z.local_stress))
        table, argmax, gy = C._grad(plan.ptr, fw.y, w, cid, aid, p, rho, g_value)
        g = _vjp_backward(fw, mesh_graph.edge_attr, gy, scale_input)
        return CriterionGradients(**vars(g), value=table[:, aid], argmax=argmax.long(), grad_output=gy)


@dataclass
class BoundaryGradients(InputGradients):
    """The fields of ``InputGradients`` for the cotangent ``grad_output`` (N, 3) = the gradient of sum_g
    traction[g] T2_g / L_int,g + periodic[g] P2_g / n_pairs,g with respect to ``local_stress``, and ``value`` (B,)
    fp64, graph g's term of that sum (NaN where a denominator is 0)."""
    value: torch.Tensor = None
    grad_output: torch.Tensor = None


def boundary_gradients(model, mesh_graph, traction=1.0, periodic=0.0, scale_output: bool = True,
                       scale_input: bool = True) -> BoundaryGradients:
    """The sensitivity of the boundary residuals of the prediction (``gnn_local_stress.boundary``: ``traction``
    times the mean-square traction on the hole's edge T2 / L_int plus ``periodic`` times the mean-square jump across
    the periodic connections P2 / n_pairs; the weights are scalars or (B,) tensors) with respect to
    ``mean_stress``, ``pos``, ``edge_attr`` and each graph's ``load``, in one call: one engine forward, the two
    boundary launches on its output (pdg_boundary_residuals, pdg_boundary_residuals_bwd), one engine backward with
    that cotangent and the per-graph column sums.  The batch carries ``boundary_vec`` / ``boundary_len``
    (``convert_mesh_to_graph(..., boundary=True)``).  ``pos`` here goes through the node features only: the
    dependence of the boundary vectors on the coordinates is not chained (nor, as in ``input_gradients``, that of
    ``edge_attr``).  With ``scale_output=False`` the residuals are those of the standardised field the model then
    returns, not of a stress.  Where the zero-stress guard fires every gradient is zero and ``value`` is that of a
    zero field.  Works with or without ``torch.no_grad()``, never touches a parameter's ``.grad``, raises on CPU
    tensors."""
    from . import boundary as Bd
    dev = mesh_graph.pos.device
    if dev.type != "cuda":
        raise RuntimeError("boundary_gradients runs on the MI355X HIP path only; move the batch to a HIP device "
                           "(the CPU restatement is test-only, tests/boundary_ref.py)")
    _check_sizes(model)
    with torch.no_grad():
        fw = _vjp_forward(model, mesh_graph, scale_output, scale_input)
        B = fw.plan.n_graphs
        gt, gp = Bd._weight(traction, B, dev, "traction"), Bd._weight(periodic, B, dev, "periodic")

        def value(table):
            # a term whose weight is 0 is switched off, as in the backward launch: 0 * (0 / 0) stays out
            zero = torch.zeros(B, dtype=torch.float64, device=dev)
            return (torch.where(gt == 0, zero, gt * table[:, 2] / table[:, 0])
                    + torch.where(gp == 0, zero, gp * table[:, 7] / table[:, 8]))

        if fw.y is None:
            z = _zero_gradients(fw.plan, mesh_graph.edge_attr, dev)
            table, _ = Bd._forward(Bd._setup(z.local_stress, mesh_graph, None, None, True))
            return BoundaryGradients(**vars(z), value=value(table), grad_output=torch.zeros_like(z.local_stress))
        table, _, gy = Bd._grad(Bd._setup(fw.y, mesh_graph, None, None, True), gt, gp)
        g = _vjp_backward(fw, mesh_graph.edge_attr, gy, scale_input)
        return BoundaryGradients(**vars(g), value=value(table), grad_output=gy)


@dataclass
class SampleGradients(InputGradients):
    """The fields of ``InputGradients`` for the cotangent ``grad_output`` (N, 3) = S^T ``grad_samples``, and
    ``samples`` (Q, 3), the prediction of the same call at the plan's points (``fill`` where no cell holds one)."""
    samples: torch.Tensor = None
    grad_output: torch.Tensor = None


def sample_gradients(model, mesh_graph, plan, grad_samples: torch.Tensor, node_offset: int = 0,
                     fill: float = float("nan"), scale_output: bool = True,
                     scale_input: bool = True) -> SampleGradients:
    """The sensitivity of the prediction at arbitrary points (``gnn_local_stress.sampling``: ``plan`` from
    ``PointLocator.locate``, a virtual strain gauge at every query point) with respect to ``mean_stress``, ``pos``,
    ``edge_attr`` and each graph's ``load``: ``input_gradients`` with ``grad_output = sample_field_grad(grad_samples,
    plan)``, the cotangent (Q, 3) on the samples carried to the nodes by S^T, and the samples of the same forward.
    ``node_offset`` is the first row of the plan's mesh inside a batch (``batch.ptr[g]``).  ``pos`` goes through the
    node features only: the dependence of the weights on the query and node positions is not chained.  Works with or
    without ``torch.no_grad()``, never touches a parameter's ``.grad``, raises on CPU tensors."""
    from . import sampling
    n = int(mesh_graph.mean_stress.shape[0])
    with torch.no_grad():
        gy = sampling.sample_field_grad(grad_samples, plan, n_nodes=n, node_offset=node_offset)
        g = input_gradients(model, mesh_graph, gy, scale_output, scale_input)
        samples = sampling.sample_field(g.local_stress, plan, fill, node_offset)
    return SampleGradients(**vars(g), samples=samples, grad_output=gy)


@dataclass
class InputTangents:
    """``local_stress`` (N, 3): the forward output of the same call.  ``d_local_stress`` (N, 3): the Jacobian of
    ``local_stress`` with respect to (``mean_stress``, ``pos``, ``edge_attr``) applied to the given directions."""
    local_stress: torch.Tensor
    d_local_stress: torch.Tensor


def _checked_forward(model, mesh_graph, scale_output: bool, scale_input: bool, what: str):
    """The guard, the plan and a need_grad forward as ``input_gradients`` runs them (the guard and the status
    word of a plan built here in one host read).  Returns (plan, engine, P, stats8, y, ctx); y and ctx are
    None where the zero-stress guard fires."""
    pos, ms, edge_attr = mesh_graph.pos, mesh_graph.mean_stress, mesh_graph.edge_attr
    dev = pos.device
    if dev.type != "cuda":
        raise RuntimeError(f"{what} runs on the MI355X HIP path only; move the batch to a HIP device (the CPU "
                           "restatement lives in oracle/ and is test-only)")
    if model.input_nodes_features_size != 6 or model.input_edges_features_size != 1 \
            or model.output_nodes_features_size != 3:
        raise ValueError("HIP path supports the reference feature sizes (6 node, 1 edge, 3 outputs)")
    s = stream_handle(dev)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    plan = plan_for(mesh_graph, status=flag[1:])
    msf = ms.detach().float().contiguous()
    lib.pdg_any_nonzero(msf.data_ptr(), msf.numel(), flag.data_ptr(), s)
    nonzero, status = flag.tolist()
    if not plan._checked:
        if plan.status.data_ptr() == flag[1:].data_ptr():
            try:
                plan.check_status(status)
            except AssertionError:
                mesh_graph.__dict__.pop("_plan_cache", None)
                raise
        else:
            plan.validate()
    eng = model._engine_for(dev)
    P = {n: model.get_parameter(n).detach() for n in PARAM_NAMES}
    stats8 = model.stats_tensor(dev)
    if scale_output:
        P["_std_local_stress"] = stats8[5:6]
    if not nonzero:
        return plan, eng, P, stats8, None, None
    y, ctx = eng.forward(P, stats8, plan, pos.detach().float().contiguous(), msf,
                         mesh_graph.nodes_types.reshape(-1).to(torch.int64).contiguous(),
                         edge_attr.detach().reshape(-1).float().contiguous(), model.message_passing_steps,
                         bool(scale_input), bool(scale_output), True)
    return plan, eng, P, stats8, y, ctx


def _direction(t, shape, name, dev):
    if t is None:
        return None
    if t.device.type != "cuda":
        raise RuntimeError(f"input_tangents runs on the MI355X HIP path only; move {name} to a HIP device")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have the shape {tuple(shape)}, got {tuple(t.shape)}")
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


def _formatted_directions(plan, stats8, scale_input, d_ms, d_pos, d_ea, d_load):
    """(dx_in (N, 6), de_in (E,) in plan order): the directions through pdg_format_inputs' linear map
    (models.py:140-162: / std with scale_input; the node-type column has tangent 0)."""
    N, E = plan.n_nodes, plan.n_edges
    dev = stats8.device
    dx_in = torch.zeros(N, 6, dtype=torch.float32, device=dev)
    if d_load is not None:   # broadcast to the nodes of each graph: the adjoint of InputGradients.load
        ptr = plan.ptr.long()
        per_node = torch.repeat_interleave(d_load, ptr[1:] - ptr[:-1], dim=0, output_size=N)
        d_ms = per_node if d_ms is None else d_ms + per_node
    if d_ms is not None:
        dx_in[:, 0:3] = d_ms / stats8[3] if scale_input else d_ms
    if d_pos is not None:
        dx_in[:, 3:5] = d_pos / stats8[1] if scale_input else d_pos
    if d_ea is None:
        de_in = torch.zeros(E, dtype=torch.float32, device=dev)
    else:
        de_in = d_ea.reshape(-1)[plan.perm.long()]
        de_in = (de_in / stats8[7] if scale_input else de_in).contiguous()
    return dx_in, de_in


def input_tangents(model, mesh_graph, d_mean_stress=None, d_pos=None, d_edge_attr=None, d_load=None,
                   scale_output: bool = True, scale_input: bool = True,
                   chain_edge_lengths: bool = False) -> InputTangents:
    """The Jacobian-vector product of ``model.forward(mesh_graph, scale_output, scale_input).local_stress`` with
    the input directions ``d_mean_stress`` (N, 3), ``d_pos`` (N, 2), ``d_edge_attr`` (the shape of the batch's
    ``edge_attr``, in its edge order) and ``d_load`` (B, 3), a change of each graph's imposed mean stress,
    broadcast to its nodes and added to ``d_mean_stress`` (the adjoint of ``InputGradients.load``).  Missing
    directions are zero; at least one must be given.  The model takes ``edge_attr`` as an independent input:
    ``chain_edge_lengths=True`` adds the change of the edge lengths that follows ``d_pos`` (pdg_edge_len_tan;
    periodic pairs and coincident nodes keep their constant length 0), so that ``d_pos`` is the total derivative
    for a mesh whose lengths follow its nodes.  The linearisation is the fp32 forward's own: its stored relu
    masks.  Works with or without ``torch.no_grad()``, never touches a parameter's ``.grad``, raises on CPU
    tensors; where the forward's zero-stress guard fires the output and the tangent are zero."""
    given = (d_mean_stress, d_pos, d_edge_attr, d_load)
    if all(d is None for d in given):
        raise ValueError("input_tangents needs at least one of d_mean_stress, d_pos, d_edge_attr, d_load")
    if chain_edge_lengths and d_pos is None:
        raise ValueError("chain_edge_lengths=True needs d_pos")
    with torch.no_grad():
        plan, eng, P, stats8, y, ctx = _checked_forward(model, mesh_graph, scale_output, scale_input,
                                                        "input_tangents")
        dev = stats8.device
        N, E, B = plan.n_nodes, plan.n_edges, plan.n_graphs
        edge_attr = mesh_graph.edge_attr
        d_ms = _direction(d_mean_stress, (N, 3), "d_mean_stress", dev)
        d_p = _direction(d_pos, (N, 2), "d_pos", dev)
        d_ea = _direction(d_edge_attr, edge_attr.shape, "d_edge_attr", dev)
        d_ld = _direction(d_load, (B, 3), "d_load", dev)
        f32 = dict(dtype=torch.float32, device=dev)
        if y is None:
            return InputTangents(local_stress=torch.zeros(N, 3, **f32), d_local_stress=torch.zeros(N, 3, **f32))
        if chain_edge_lengths and E:
            ei = mesh_graph.edge_index.to(torch.int64).contiguous()
            dlen = torch.empty(E, **f32)
            lib.pdg_edge_len_tan(E, N, ei[0].data_ptr(), ei[1].data_ptr(),
                                 mesh_graph.pos.detach().float().contiguous().data_ptr(), d_p.data_ptr(),
                                 edge_attr.detach().reshape(-1).float().contiguous().data_ptr(), dlen.data_ptr(),
                                 stream_handle(dev))
            d_ea = dlen.view(edge_attr.shape) if d_ea is None else d_ea + dlen.view(edge_attr.shape)
        dx_in, de_in = _formatted_directions(plan, stats8, scale_input, d_ms, d_p, d_ea, d_ld)
        return InputTangents(local_stress=y, d_local_stress=eng.tangent(P, ctx, dx_in, de_in))


def localisation_tensor(model, mesh_graph, scale_output: bool = True, scale_input: bool = True) -> torch.Tensor:
    """The stress localisation tensor ``A[n, i, j] = d local_stress[n, i] / d Sigma_j`` (N, 3, 3), Sigma the
    imposed mean stress of node n's graph: one forward and three tangent passes with ``d_load = e_j``; column j
    is bitwise ``input_tangents(..., d_load=e_j).d_local_stress``.  Zeros where the zero-stress guard fires."""
    with torch.no_grad():
        plan, eng, P, stats8, y, ctx = _checked_forward(model, mesh_graph, scale_output, scale_input,
                                                        "localisation_tensor")
        N, E, B = plan.n_nodes, plan.n_edges, plan.n_graphs
        A = torch.zeros(N, 3, 3, dtype=torch.float32, device=stats8.device)
        if y is None:
            return A
        for j in range(3):
            d_load = torch.zeros(B, 3, dtype=torch.float32, device=stats8.device)
            d_load[:, j] = 1.0
            dx_in, de_in = _formatted_directions(plan, stats8, scale_input, None, None, None, d_load)
            A[:, :, j] = eng.tangent(P, ctx, dx_in, de_in)
        return A


def mean_localisation(model, mesh_graph, weights=None, cell_area=None, convention: str = "cell",
                      scale_output: bool = True, scale_input: bool = True) -> torch.Tensor:
    """(B, 3, 3) fp64: the volume average of ``localisation_tensor`` per graph, d <sigma>_i / d Sigma_j, its nine
    columns averaged in one ``pdg_graph_wmean`` call (``gnn_local_stress.homogenise.graph_average``;
    ``weights``, ``cell_area`` and ``convention`` as there, the batch's ``node_area`` / ``cell_area`` by
    default).  The identity for a mean-consistent model.  The graph LayerNorm's statistics run over the whole
    batch and couple its graphs, so for a batch this is the response to moving every graph's load at once."""
    from . import homogenise as H
    # refused before the forward and the three tangent passes
    cellwise = H._convention(convention, cell_area if cell_area is not None else H._of_batch(mesh_graph, "cell_area"))
    A = localisation_tensor(model, mesh_graph, scale_output, scale_input)
    avg = H.graph_average(A.reshape(A.shape[0], 9), mesh_graph, weights, cell_area)
    return (avg.mean_cell if cellwise else avg.mean_material).reshape(-1, 3, 3)
