"""Device graph plan: the CSR view of a (batched) graph that the HIP kernels consume.

Built once per batch from the reference's inputs (``edge_index`` coalesced,
i.e. sorted by (src, dst) — ``datasets.py:119``; per-graph node offsets
``ptr``; the divergence operators) and cached on the batch object:

* dst-sorted edge order (stable, so within a destination the sources stay
  ascending = the order PyG's ``scatter_add_`` accumulates in);
* ``rowptr_dst`` (N+1) over that order, ``src``/``dst`` of each sorted edge,
  ``perm`` = original edge id of each sorted edge (for ``edge_attr``);
* ``perm_src``/``rowptr_src``: the sorted edges grouped by source, for the
  backward of the ``x[src]`` gathers;
* divergence operator A in CSR over global rows with graph-local columns, and
  A^T grouped by global node (``at_*``) for the backward SpMV.

Edge order is internal: the model only returns node outputs
(``models.py:322-326``), so the reordering is invisible to callers.
"""
from __future__ import annotations

import torch


def _rowptr(keys: torch.Tensor, n: int) -> torch.Tensor:
    counts = torch.bincount(keys, minlength=n)
    rp = torch.zeros(n + 1, dtype=torch.int64, device=keys.device)
    rp[1:] = torch.cumsum(counts, 0)
    return rp.to(torch.int32)


class GraphPlan:
    """``planner``: "auto" builds a HIP tensor's plan with the device planner (csrc/pdg_plan.hip:
    no host read, no ATen sort) and a CPU tensor's with the torch code below; "torch" forces the
    torch code on any device (A/B, and the yardstick of tests/test_gpu_plan.py).

    The device planner checks the endpoints on the device: ``status`` is one int32 there, non-zero
    when an endpoint (or a divergence entry) was out of range, in which case it was treated as
    node 0 (the entry dropped) so that the plan stays in range.  :meth:`validate` reads it.
    ``status``: where to keep that word (a 1-element int32 HIP tensor, e.g. a slice of a buffer
    the caller reads back anyway); the plan allocates its own by default."""

    status = None        # device status word (device planner only)
    _checked = True      # nothing to read: the torch code asserts the range while it builds

    def __init__(self, edge_index: torch.Tensor, num_nodes: int, ptr: torch.Tensor | None = None,
                 op_rows: torch.Tensor | None = None, op_cols: torch.Tensor | None = None,
                 op_vals: torch.Tensor | None = None, planner: str = "auto",
                 status: torch.Tensor | None = None) -> None:
        if planner not in ("auto", "torch"):
            raise ValueError("planner must be 'auto' or 'torch'")
        dev = edge_index.device
        n = int(num_nodes)
        self.n_nodes = n
        self.n_edges = int(edge_index.shape[1])
        if dev.type == "cuda" and planner == "auto":
            self._build_device(edge_index, ptr, op_rows, op_cols, op_vals, status)
            return
        src = edge_index[0].long()
        dst = edge_index[1].long()
        if self.n_edges:
            assert int(src.max()) < n and int(dst.max()) < n and int(src.min()) >= 0 and int(dst.min()) >= 0, \
                "edge_index out of range"
        key = dst * n + src
        order = torch.sort(key, stable=True).indices
        self.perm = order.to(torch.int32)
        self.src = src[order].to(torch.int32).contiguous()
        self.dst = dst[order].to(torch.int32).contiguous()
        self.rowptr_dst = _rowptr(dst, n)
        key2 = self.src.long() * n + self.dst.long()
        self.perm_src = torch.sort(key2, stable=True).indices.to(torch.int32).contiguous()
        self.rowptr_src = _rowptr(src, n)
        if ptr is None:
            ptr = torch.tensor([0, n], dtype=torch.int64, device=dev)
        self.ptr = ptr.to(dev).to(torch.int32).contiguous()
        self.n_graphs = int(self.ptr.numel() - 1)
        self.has_div = op_rows is not None
        if self.has_div:
            self._build_div(op_rows.to(dev).long(), op_cols.to(dev).long(), op_vals.to(dev).float())

    def _build_div(self, rows: torch.Tensor, cols: torch.Tensor, vals: torch.Tensor) -> None:
        n = self.n_nodes
        ptr = self.ptr.long()
        g = torch.searchsorted(ptr, rows, right=True) - 1
        off = ptr[g]
        ng = ptr[g + 1] - off
        keep = cols < 2 * ng          # reference slices [:, :2N_i] (gnn_train.py:74)
        rows, cols, vals, off, ng = rows[keep], cols[keep], vals[keep], off[keep], ng[keep]
        order = torch.sort(rows, stable=True).indices
        self.a_rowptr = _rowptr(rows, n)
        self.a_col = cols[order].to(torch.int32).contiguous()
        self.a_val = vals[order].contiguous()
        node = off + torch.where(cols < ng, cols, cols - ng)
        comp = (cols >= ng).to(torch.int32)
        order_t = torch.sort(node, stable=True).indices
        self.at_rowptr = _rowptr(node, n)
        self.at_row = rows[order_t].to(torch.int32).contiguous()
        self.at_comp = comp[order_t].contiguous()
        self.at_val = vals[order_t].contiguous()

    def validate(self) -> None:
        """Raise the torch planner's ``AssertionError`` when the device planner met an endpoint out
        of range (one host read of the status word, once per plan)."""
        if self._checked:
            return
        self.check_status(int(self.status.item()))

    def check_status(self, status: int) -> None:
        """:meth:`validate` for a caller that has read the status word itself."""
        if status:
            raise AssertionError("edge_index out of range")
        self._checked = True

    def _build_device(self, edge_index, ptr, op_rows, op_cols, op_vals, status) -> None:
        from .lib import lib, stream_handle
        dev = edge_index.device
        n, E = self.n_nodes, self.n_edges
        i32 = dict(dtype=torch.int32, device=dev)
        if status is None:
            status = torch.empty(1, **i32)
        elif status.dtype != torch.int32 or status.numel() != 1 or status.device != dev:
            raise ValueError("status must be one int32 on the plan's device")
        self.status, self._checked = status, False
        if ptr is None:
            self.ptr = torch.arange(2, **i32) * n            # [0, n] without a host-to-device copy
        else:
            self.ptr = ptr.to(dev).to(torch.int32).contiguous()
        self.n_graphs = int(self.ptr.numel() - 1)
        self.has_div = op_rows is not None
        nnz = int(op_rows.numel()) if self.has_div else 0
        nbytes = lib.pdg_graph_plan_scratch_bytes(n, E, nnz)
        if nbytes < 0:
            raise ValueError(f"graph plan: unsupported sizes (nodes {n}, edges {E}, operator entries {nnz})")
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        s = stream_handle(dev)
        ei = edge_index.long().contiguous()
        for k in ("perm", "src", "dst", "perm_src"):
            setattr(self, k, torch.empty(E, **i32))
        self.rowptr_dst, self.rowptr_src = torch.empty(n + 1, **i32), torch.empty(n + 1, **i32)
        lib.pdg_graph_plan(n, E, ei[0].data_ptr() if E else None, ei[1].data_ptr() if E else None,
                           *(getattr(self, k).data_ptr() if E else None for k in ("perm", "src", "dst")),
                           self.rowptr_dst.data_ptr(), self.perm_src.data_ptr() if E else None,
                           self.rowptr_src.data_ptr(), status.data_ptr(), scratch.data_ptr(), nbytes, s)
        if self.has_div:
            self._build_div_device(op_rows, op_cols, op_vals, scratch)

    def _build_div_device(self, op_rows, op_cols, op_vals, scratch=None) -> None:
        """``_build_div`` by pdg_div_plan.  Without ``scratch`` (a divergence-only plan, no pdg_graph_plan
        before it) the status word is cleared here."""
        from .lib import lib, stream_handle
        dev, n = self.ptr.device, self.n_nodes
        i32 = dict(dtype=torch.int32, device=dev)
        rows, cols = op_rows.to(dev).long().contiguous(), op_cols.to(dev).long().contiguous()
        vals = op_vals.to(dev).float().contiguous()
        nnz = int(rows.numel())
        clear = scratch is None
        if clear:
            nbytes = lib.pdg_graph_plan_scratch_bytes(n, 0, nnz)
            if nbytes < 0:
                raise ValueError(f"divergence plan: unsupported sizes (nodes {n}, operator entries {nnz})")
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            self.status, self._checked = torch.empty(1, **i32), False
        self.a_rowptr, self.at_rowptr = torch.empty(n + 1, **i32), torch.empty(n + 1, **i32)
        a_col, at_row, at_comp = (torch.empty(nnz, **i32) for _ in range(3))
        a_val, at_val = (torch.empty(nnz, dtype=torch.float32, device=dev) for _ in range(2))
        nz = bool(nnz)
        lib.pdg_div_plan(n, self.n_graphs, self.ptr.data_ptr(), nnz, *(t.data_ptr() if nz else None
                                                                       for t in (rows, cols, vals)),
                         self.a_rowptr.data_ptr(), *(t.data_ptr() if nz else None for t in (a_col, a_val)),
                         self.at_rowptr.data_ptr(), *(t.data_ptr() if nz else None for t in (at_row, at_comp, at_val)),
                         self.status.data_ptr(), int(clear), scratch.data_ptr(), scratch.numel(), stream_handle(dev))
        # the kept count depends on the data (columns beyond 2 N_g are dropped): the planner's only
        # host read, and only with a divergence operator
        kept = int(self.a_rowptr[n].item()) if nz else 0
        self.a_col, self.a_val = a_col[:kept], a_val[:kept]
        self.at_row, self.at_comp, self.at_val = at_row[:kept], at_comp[:kept], at_val[:kept]


def plan_for(data, planner: str = "auto", status: torch.Tensor | None = None) -> GraphPlan:
    """Return (and cache on ``data``) the plan of a Data/Batch-like object.  ``planner`` and
    ``status`` (see :class:`GraphPlan`) matter only when the plan is built here, not for a cached one."""
    plan = data.__dict__.get("_plan_cache") if hasattr(data, "__dict__") else None
    ei = data.edge_index
    key = (ei.data_ptr(), tuple(ei.shape), ei.device)
    if plan is not None and plan[0] == key:
        return plan[1]
    ptr = data.__dict__.get("ptr") if hasattr(data, "__dict__") else None
    rows = data.__dict__.get("op_div_rows") if hasattr(data, "__dict__") else None
    p = GraphPlan(ei, data.num_nodes if hasattr(data, "num_nodes") else data.pos.shape[0], ptr,
                  rows, data.__dict__.get("op_div_cols") if rows is not None else None,
                  data.__dict__.get("op_div_vals") if rows is not None else None, planner=planner, status=status)
    try:
        data.__dict__["_plan_cache"] = (key, p)
    except Exception:
        pass
    return p
