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
    pos, ms, edge_attr = mesh_graph.pos, mesh_graph.mean_stress, mesh_graph.edge_attr
    dev = pos.device
    if dev.type != "cuda" or grad_output.device.type != "cuda":
        raise RuntimeError("input_gradients runs on the MI355X HIP path only; move the batch and grad_output to a "
                           "HIP device (the CPU restatement lives in oracle/ and is test-only)")
    if model.input_nodes_features_size != 6 or model.input_edges_features_size != 1 \
            or model.output_nodes_features_size != 3:
        raise ValueError("HIP path supports the reference feature sizes (6 node, 1 edge, 3 outputs)")
    if tuple(grad_output.shape) != tuple(ms.shape):
        raise ValueError(f"grad_output must have the shape of local_stress {tuple(ms.shape)}, "
                         f"got {tuple(grad_output.shape)}")
    with torch.no_grad():
        f32 = dict(dtype=torch.float32, device=dev)
        s = stream_handle(dev)
        # the guard and the status word of a plan built here in one host read, as in forward
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
        N, E, B = plan.n_nodes, plan.n_edges, plan.n_graphs
        if not nonzero:
            return InputGradients(local_stress=torch.zeros(N, 3, **f32), mean_stress=torch.zeros(N, 3, **f32),
                                  pos=torch.zeros(N, 2, **f32), edge_attr=torch.zeros(edge_attr.shape, **f32),
                                  load=torch.zeros(B, 3, **f32))
        eng = model._engine_for(dev)
        P = {n: model.get_parameter(n).detach() for n in PARAM_NAMES}
        stats8 = model.stats_tensor(dev)
        y, ctx = eng.forward(P, stats8, plan, pos.detach().float().contiguous(), msf,
                             mesh_graph.nodes_types.reshape(-1).to(torch.int64).contiguous(),
                             edge_attr.detach().reshape(-1).float().contiguous(), model.message_passing_steps,
                             bool(scale_input), bool(scale_output), True)
        if scale_output:
            P["_std_local_stress"] = stats8[5:6]
        # the engine's backward fuses the weight gradients into the input-gradient chain: they land in scratch
        # accumulators that are dropped here, never in a parameter's .grad
        G = {n: torch.zeros_like(p) for n, p in P.items() if n in PARAM_NAMES}
        ig = InputGrads(mean_stress=torch.empty(N, 3, **f32), pos=torch.empty(N, 2, **f32),
                        edge_attr=torch.empty(E, **f32), stats8=stats8, scale_input=bool(scale_input))
        eng.backward(P, ctx, grad_output.detach().float().contiguous(), G, input_grads=ig)
        load = torch.empty(B, 3, **f32)
        lib.pdg_graph_colsum3(B, plan.ptr.data_ptr(), ig.mean_stress.data_ptr(), load.data_ptr(), s)
        return InputGradients(local_stress=y, mean_stress=ig.mean_stress, pos=ig.pos,
                              edge_attr=ig.edge_attr.view(edge_attr.shape), load=load)
