"""The device graph planner (csrc/pdg_plan.hip through pdg.plan.GraphPlan on a HIP tensor) against
the torch planner run on the CPU copies of the same tensors: every plan array bit for bit, with its
dtype, shape and contiguity, and the four scalars.  The yardstick never touches the kernels."""
import numpy as np
import pytest
import torch

from gpu_common import dataset_stats, dev
from pdg import graph, meshgen
from pdg.plan import GraphPlan, plan_for
from test_gpu_collate import PLAN_KEYS, _datasets

pytestmark = pytest.mark.gpu

EDGE_KEYS = PLAN_KEYS[:7]


def _same(p_dev: GraphPlan, p_cpu: GraphPlan) -> None:
    assert (p_dev.n_nodes, p_dev.n_edges, p_dev.n_graphs, p_dev.has_div) == \
        (p_cpu.n_nodes, p_cpu.n_edges, p_cpu.n_graphs, p_cpu.has_div)
    for k in (PLAN_KEYS if p_cpu.has_div else EDGE_KEYS):
        a, b = getattr(p_dev, k), getattr(p_cpu, k)
        assert a.device.type == "cuda" and a.is_contiguous(), k
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        assert torch.equal(a.cpu(), b), k


def _both(ei: torch.Tensor, n: int, ptr=None, op=None):
    """(device plan, CPU torch plan) of the same CPU tensors."""
    op = op or (None, None, None)
    p_cpu = GraphPlan(ei, n, ptr, *op)
    to = lambda t: None if t is None else t.to(dev())   # noqa: E731
    p_dev = GraphPlan(to(ei), n, to(ptr), *(to(t) for t in op))
    return p_dev, p_cpu


def _edges(n: int, e: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, n, (2, e), generator=g, dtype=torch.int64)


def test_single_mesh_without_ptr_or_operator():
    d = graph.sample_to_data(meshgen.hole_plate(5))
    p_dev = plan_for(d.to(dev()))
    p_cpu = plan_for(d)
    assert not p_cpu.has_div and p_cpu.n_graphs == 1
    _same(p_dev, p_cpu)
    p_dev.validate()


def test_host_collated_batch_with_operator():
    """ptr, the divergence CSR and CSR^T, one non-periodic graph among six."""
    b = graph.Batch.from_data_list(_datasets())
    p_dev, p_cpu = plan_for(b.to(dev())), plan_for(b)
    assert p_cpu.has_div and p_cpu.n_graphs == 6
    _same(p_dev, p_cpu)
    p_dev.validate()


def test_random_multigraph_ties_and_empty_rows():
    """Unsorted endpoints, duplicate edges, self-loops, isolated nodes (the first and the last node
    among them): ties exercise stability, rowptr the empty rows at both ends."""
    n, e = 37, 2000
    ei = 1 + _edges(n - 4, e, 11)            # nodes 0 and 34..36 never appear
    ei[:, 100:140] = ei[:, 300:340]          # duplicates
    ei[1, 500:530] = ei[0, 500:530]          # self-loops
    ei[:, 700:720] = ei[:, 100:120]          # triplicates
    used = set(ei.flatten().tolist())
    assert 0 not in used and n - 1 not in used and len(set(range(n)) - used) >= 3
    assert torch.unique(ei, dim=1).shape[1] < e and bool((ei[0] == ei[1]).any())
    _same(*_both(ei, n))


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_scan_block_boundaries(n):
    _same(*_both(_edges(n, 4 * n, 100 + n), n))


def test_hub_row_beyond_every_threshold():
    """A star with hub degree 3000 in both directions plus 500 duplicate hub edges, shuffled: the
    hub's row (3500 slots in the dst and in the src grouping) is longer than the one-thread and the
    in-LDS limits of the row sort."""
    n, hub = 3001, 1234
    leaves = torch.tensor([v for v in range(n) if v != hub])
    h = torch.full_like(leaves, hub)
    ei = torch.cat([torch.stack([h, leaves]), torch.stack([leaves, h])], 1)
    g = torch.Generator().manual_seed(3)
    ei = torch.cat([ei, ei[:, torch.randint(0, ei.shape[1], (500,), generator=g)]], 1)
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)]
    assert int((ei[1] == hub).sum()) > 3000 and int((ei[0] == hub).sum()) > 3000
    _same(*_both(ei, n))


def test_row_lengths_around_the_sort_thresholds():
    """Rows of exactly 32 / 33 slots (one thread | workgroup in LDS) and 2048 / 2049 (LDS | global
    memory), an empty row last; sources drawn from few values, so ties are long."""
    deg = [32, 33, 2048, 2049, 0]
    dst = torch.cat([torch.full((d,), r, dtype=torch.int64) for r, d in enumerate(deg)])
    g = torch.Generator().manual_seed(5)
    src = torch.randint(0, 4, (dst.numel(),), generator=g, dtype=torch.int64)
    ei = torch.stack([src, dst])[:, torch.randperm(dst.numel(), generator=g)]
    _same(*_both(ei, len(deg)))
    _same(*_both(ei.flip(0), len(deg)))


def test_no_edges():
    p_dev, p_cpu = _both(torch.zeros(2, 0, dtype=torch.int64), 7)
    _same(p_dev, p_cpu)
    for k in ("perm", "src", "dst", "perm_src"):
        assert getattr(p_dev, k).numel() == 0 and getattr(p_dev, k).dtype == torch.int32
    assert not bool(p_dev.rowptr_dst.any()) and not bool(p_dev.rowptr_src.any())
    torch.cuda.synchronize()
    p_dev.validate()


def test_divergence_filter_drops_columns_beyond_2n():
    datas = _datasets()[:3]
    b = graph.Batch.from_data_list(datas)
    lo, hi = int(b.ptr[1]), int(b.ptr[2])           # the middle graph
    ng = hi - lo
    extra_rows = torch.tensor([lo, lo + 3, hi - 1, lo + 3, lo + ng // 2])
    extra_cols = torch.tensor([2 * ng, 2 * ng + 5, 3 * ng, 2 * ng, 2 * ng + 1])
    extra_vals = torch.tensor([1.5, -2.0, 3.25, 0.5, -0.125])
    at = b.op_div_rows.numel() // 2                 # not coalesced any more: spliced into the middle
    rows = torch.cat([b.op_div_rows[:at], extra_rows, b.op_div_rows[at:]])
    cols = torch.cat([b.op_div_cols[:at], extra_cols, b.op_div_cols[at:]])
    vals = torch.cat([b.op_div_vals[:at], extra_vals, b.op_div_vals[at:]])
    p_dev, p_cpu = _both(b.edge_index, b.num_nodes, b.ptr, (rows, cols, vals))
    assert p_cpu.a_col.numel() == rows.numel() - 5 != rows.numel()
    _same(p_dev, p_cpu)
    p_dev.validate()


def test_status_word_and_clamped_plan():
    """Endpoints out of range: validate() raises, yet every index array is in range and equals the
    plan of the edge_index with those endpoints replaced by node 0.  Only the plan is built."""
    d = graph.sample_to_data(meshgen.hole_plate(5))
    n = d.num_nodes
    ei = d.edge_index.clone()
    ei[0, 7] = n
    ei[1, 40] = -1
    p_bad = GraphPlan(ei.to(dev()), n)
    with pytest.raises(AssertionError, match="out of range"):
        p_bad.validate()
    with pytest.raises(AssertionError, match="out of range"):
        GraphPlan(ei, n)                              # the torch planner's assertion, same message
    e = p_bad.n_edges
    for k, bound in (("perm", e), ("src", n), ("dst", n), ("perm_src", e), ("rowptr_dst", e + 1),
                     ("rowptr_src", e + 1)):
        t = getattr(p_bad, k)
        assert int(t.min()) >= 0 and int(t.max()) < bound, k
    fixed = ei.clone()
    fixed[0, 7] = 0
    fixed[1, 40] = 0
    _same(p_bad, GraphPlan(fixed, n))
    GraphPlan(d.edge_index.to(dev()), n).validate()   # a clean graph passes


def test_plan_for_makes_no_host_synchronisation(monkeypatch):
    """plan_for on a fresh Data without a divergence operator completes under
    torch.cuda.set_sync_debug_mode("error"), and with torch.sort / bincount / searchsorted and
    Tensor.item / max / min made to raise.  Both methods are in force: the sync-debug mode is checked
    here to raise on this torch build for the torch planner (the planner of the parent commit), and
    the patched functions cover what the mode would not see."""
    sample = meshgen.hole_plate(5)
    d = graph.sample_to_data(sample).to(dev())
    d_old = graph.sample_to_data(sample).to(dev())
    torch.cuda.synchronize()

    def boom(*a, **k):
        raise AssertionError("the device planner called a host-paced torch function")

    old = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        with monkeypatch.context() as m:
            for name in ("sort", "bincount", "searchsorted"):
                m.setattr(torch, name, boom)
            for name in ("item", "max", "min"):
                m.setattr(torch.Tensor, name, boom)
            p = plan_for(d)
        with pytest.raises(RuntimeError, match="synchroniz"):
            plan_for(d_old, planner="torch")
    finally:
        torch.cuda.set_sync_debug_mode(old)
    _same(p, plan_for(graph.sample_to_data(sample)))
    p.validate()


def _model(d):
    from gnn_local_stress.models import EncodeProcessDecode
    torch.manual_seed(69)
    stats = {k: torch.tensor(float(v)) for k, v in dataset_stats(d).items()}
    return EncodeProcessDecode(input_edges_features_size=1, message_passing_steps=3, latent_size=128,
                               input_nodes_features_size=6, output_nodes_features_size=3, **stats).to(dev())


def test_model_output_does_not_depend_on_the_planner():
    from pdg.serve import CapturedForward
    sample = meshgen.hole_plate(9)
    d_new = graph.sample_to_data(sample).to(dev())
    d_old = graph.sample_to_data(sample).to(dev())
    model = _model(d_new)
    p_old = plan_for(d_old, planner="torch")
    assert p_old.status is None
    with torch.no_grad():
        y_new = model(d_new).local_stress.clone()
        y_old = model(d_old).local_stress.clone()
    assert plan_for(d_new).status is not None and plan_for(d_old) is p_old
    assert bool(y_new.any()) and torch.equal(y_new, y_old)
    cap = CapturedForward(model, d_new)
    assert torch.equal(cap(d_new.mean_stress).clone(), y_new)


def test_model_refuses_a_graph_out_of_range():
    """The forward reads the plan's status word with the zero-stress flag and raises before anything
    downstream is launched; the bad plan is not kept."""
    d = graph.sample_to_data(meshgen.hole_plate(5))
    d.edge_index = d.edge_index.clone()
    d.edge_index[1, 3] = d.num_nodes + 5
    d = d.to(dev())
    model = _model(graph.sample_to_data(meshgen.hole_plate(5)))
    for _ in range(2):
        with pytest.raises(AssertionError, match="out of range"), torch.no_grad():
            model(d)
        assert "_plan_cache" not in d.__dict__
