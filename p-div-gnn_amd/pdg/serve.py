"""Inference forward of one fixed mesh graph replayed from a HIP graph (serving).

The reference's published timing (``scripts/benchmark_gnn_fem.py:81-100,540-567``) runs
``EncodeProcessDecode.forward`` on ONE mesh for several imposed mean strains: the graph (edges,
lengths, periodic pairs, node labels) is the same every time, only ``mean_stress`` changes.  At
the sizes of that sweep (458 - 25,556 nodes) the forward is ~50 launches of a few microseconds
each, so host launch work and the reference's host-side zero-stress check (``models.py:294-299``,
one synchronisation) cost as much as the kernels.  :class:`CapturedForward` records the whole
forward once - the guard as ``pdg_any_nonzero`` + ``pdg_zero_unless`` on the device, the format /
encode / 10 message-passing steps / decode launches of :class:`pdg.engine.EPDEngine` - and replays
it per sample: one graph launch, no host synchronisation.

Results are bitwise those of ``model(graph)`` on the same inputs (same kernels, same order;
``tests/test_gpu_published.py``).  The captured graph reads the model's parameters and the
statistics in place (a changed parameter tensor object or statistic needs a new capture,
:meth:`CapturedForward.stale` tells), the graph's ``pos`` / ``nodes_types`` / ``edge_attr`` at
their addresses, and its own ``mean_stress`` buffer, which :meth:`__call__` refills.
"""
from __future__ import annotations

import torch

from .engine import PARAM_NAMES
from .lib import lib, stream_handle
from .plan import plan_for


class CapturedForward:
    """``model(graph, scale_output, scale_input).local_stress`` as one HIP-graph replay.

    ``model``: a ``gnn_local_stress.models.EncodeProcessDecode`` on the graph's device;
    ``graph``: a Data / Batch on that device (its plan is built once here)."""

    def __init__(self, model, graph, scale_output: bool = True, scale_input: bool = True) -> None:
        dev = graph.pos.device
        if dev.type != "cuda":
            raise RuntimeError("CapturedForward needs a graph on a HIP device (no CPU fallback)")
        self.model = model
        self.device = dev
        self.plan = plan_for(graph)
        self.plan.validate()   # construction synchronises anyway; replays never read the status word
        self.eng = model._engine_for(dev)
        self.params = [model.get_parameter(n).detach() for n in PARAM_NAMES]
        self.P = dict(zip(PARAM_NAMES, self.params))
        self.stats8 = model.stats_tensor(dev)
        # the captured kernels read these at fixed addresses
        self.pos = graph.pos.float().contiguous()
        self.types = graph.nodes_types.reshape(-1).to(torch.int64).contiguous()
        self.edge_attr = graph.edge_attr.reshape(-1).float().contiguous()
        self.mean_stress = graph.mean_stress.float().contiguous().clone()
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.steps = model.message_passing_steps
        self.scale_output, self.scale_input = bool(scale_output), bool(scale_input)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):   # warm the allocator on the capture stream
            self._run()
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.y = self._run()
        self.launches = self._count_launches()

    def _run(self) -> torch.Tensor:
        s = stream_handle(self.device)
        ms = self.mean_stress
        lib.pdg_any_nonzero(ms.data_ptr(), ms.numel(), self.flag.data_ptr(), s)
        y, _ = self.eng.forward(self.P, self.stats8, self.plan, self.pos, ms, self.types, self.edge_attr,
                                self.steps, self.scale_input, self.scale_output, False)
        lib.pdg_zero_unless(self.flag.data_ptr(), y.data_ptr(), y.numel(), s)
        return y

    def _count_launches(self) -> int:
        """Library calls of one forward (each one kernel launch or memset node of the graph)."""
        n0 = lib.calls
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            self._run()
        torch.cuda.current_stream(self.device).wait_stream(side)
        return lib.calls - n0

    def stale(self) -> bool:
        """True when the model's parameters or statistics are no longer the captured tensors."""
        cur = [self.model.get_parameter(n) for n in PARAM_NAMES]
        return any(a.data_ptr() != b.data_ptr() for a, b in zip(cur, self.params)) or \
            self.model.stats_tensor(self.device) is not self.stats8

    def __call__(self, mean_stress=None) -> torch.Tensor:
        """Replay the forward; ``mean_stress``: this sample's (N, 3) field or (3,) imposed mean
        (broadcast to every node as ``benchmark_gnn_fem.py:404-407`` does), copied into the captured
        buffer first.  Returns the captured output buffer (overwritten by the next call)."""
        if mean_stress is not None:
            m = torch.as_tensor(mean_stress, dtype=torch.float32, device=self.device)
            self.mean_stress.copy_(m.expand_as(self.mean_stress) if m.dim() == 1 else m)
        self.graph.replay()
        return self.y
