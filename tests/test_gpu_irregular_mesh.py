"""The device mesh kernels (csrc/pdg_graph.hip, csrc/pdg_meshfields.hip, and the P1 cell solve built on the same
meshes) on irregular meshes and hub nodes (tests/irregular_meshes.py), against the host restatements of pdg.meshgen
on the same arrays.  Every other mesh of the suite is a structured grid, whose longest row of any grouping is 24
slots: there, csrc/pdg_group.hpp's sort_emit_kernel only ever takes its first branch.

pdg_group.hpp sorts a row of m slots by one thread (m <= 32, "short"), by the workgroup in LDS (m <= 2048, "tile")
or by the workgroup in global memory ("global").  The hub's row of a mesh with a hub of k faces holds

    policy       fan_disk(k)            quad_fan(k)    pinwheel(k)   what the slots are
    EdgeByMin    2 k  (hub id 0)        2 k            2 k           the k spokes, each a side of two faces (pinwheel:
                 0    (hub id N - 1)                                 2 k edges of one face each, all on the boundary)
    PairByRow    3 k                    4 k            3 k           (hub, column node) once per face and corner
    FaceByNode   k                      k              k             the hub's faces
    EndByNode    2                      2              2 k           boundary edges at a node: 2 on any manifold mesh,
                                                                     so only the pinwheel's pinched hub has a long row

and pdg_graph.hip's row of the hub 2 k slots (one thread sorts it: k stays <= 2049).  The branch each case reaches,
s / t / g for short / tile / global, by the hub's row (every other row of these meshes is short):

    fan_disk k    10  11  16  17  32  33  682  683  1024  1025  2048  2049
      EdgeByMin   s   s   s   t   t   t   t    t    t     g     g     g      (hub id 0; with the hub last: all s)
      PairByRow   s   t   t   t   t   t   t    g    g     g     g     g
      FaceByNode  s   s   s   s   s   t   t    t    t     t     t     g
    quad_fan k    2   3   8   9   128  129  512  513
      EdgeByMin   s   s   s   s   t    t    t    t
      PairByRow   s   s   s   t   t    t    t    g
      FaceByNode  s   s   s   s   t    t    t    t
    pinwheel k    16  17  1024  1025
      EdgeByMin   s   t   t     g
      EndByNode   s   t   t     g
      PairByRow   t   t   g     g
      FaceByNode  s   s   t     t

so every policy runs all three branches, each at its two thresholds.  (The quad fan's k = 2, 3, 128, 129 are kept
as cases; the device's row of the hub holds 4 k slots, not the 16 k of a first estimate, so 8, 9, 512, 513 are the
thresholds.)  fan_annulus gives the component search a 700-node rim with scattered ids, refined_plate valences 3 to
16 side by side and the periodic pairs, two_column_strip a periodic pair on the column of a mesh edge.

Bounds.  Integer outputs and the fp32 edge lengths are bitwise the host's (tests/test_gpu_devgraph.py).  Operator:
|got - want| <= 2^-23 |want| + 1e-9 max|want| for every entry, the hub's row included (tests/test_gpu_meshfields.py):
the second term pays for the order of the fp64 additions, and on the CPU the hub's face-order sums are 2.2e-16 from
their exact sums at k = 2049, 4.1e-8 of that term (tests/test_irregular_meshes_host.py
test_order_of_the_hub_sums_stays_under_the_operator_bound), so no separate hub bound is needed.  Areas and boundary
vectors: both sides add the same fp64 terms in the same order, the hub's k (or 2 k) terms too, and round once:
|got - want| <= 2^-23 |want| and exact zeros where the host has them (tests/test_gpu_quadmesh.py,
tests/test_gpu_homog.py); the total area and the closed-boundary sums of the device's output meet the invariants of
tests/test_irregular_meshes_host.py.  Every output buffer is GUARD elements longer than its capacity, pre-filled,
and the tail must come back untouched."""
import functools

import numpy as np
import pytest
import torch

import irregular_meshes as M
from test_irregular_meshes_host import check_area_and_closed_boundaries

pytestmark = pytest.mark.gpu

GUARD = 5
ST_NONMANIFOLD = 2      # info[2] of pdg_node_labels and *status of pdg_boundary_vectors: bit 2

CASES = {}
for _k in (10, 11, 32, 33, 682, 683, 2048, 2049):
    CASES[f"disk{_k}_hub_first"] = functools.partial(M.fan_disk, _k, 2, 0)
    CASES[f"disk{_k}_hub_last"] = functools.partial(M.fan_disk, _k, 2, -1)
for _k in (16, 17, 1024, 1025):      # 2 k crosses 32 and 2048: EdgeByMin's thresholds
    CASES[f"disk{_k}_hub_first"] = functools.partial(M.fan_disk, _k, 2, 0)
for _k in (33, 683):
    CASES[f"disk{_k}_renumbered"] = functools.partial(M.fan_disk, _k, 2, 0, renumber=5)
for _k in (33, 700):
    CASES[f"annulus{_k}"] = functools.partial(M.fan_annulus, _k, 2)
    CASES[f"annulus{_k}_renumbered"] = functools.partial(M.fan_annulus, _k, 2, renumber=5)
for _k in (2, 3, 8, 9, 128, 129, 512, 513):
    CASES[f"quad_fan{_k}"] = functools.partial(M.quad_fan, _k)
CASES["quad_fan129_renumbered"] = functools.partial(M.quad_fan, 129, renumber=2)
for _k in (16, 17, 1024, 1025):
    CASES[f"pinwheel{_k}"] = functools.partial(M.pinwheel, _k)
CASES["pinwheel17_renumbered"] = functools.partial(M.pinwheel, 17, renumber=4)
CASES["refined13_periodic"] = functools.partial(M.refined_plate, 13, 0.2, True)
CASES["refined24_open"] = functools.partial(M.refined_plate, 24, 0.3, False, splits=60, flips=50)
CASES["refined24_open_renumbered"] = functools.partial(M.refined_plate, 24, 0.3, False, splits=60, flips=50, renumber=7)
CASES["strip"] = M.two_column_strip
CASES["strip_renumbered"] = functools.partial(M.two_column_strip, renumber=3)

PERIODIC = ("refined13_periodic", "strip", "strip_renumbered")


@functools.lru_cache(maxsize=None)
def mesh(name):
    return CASES[name]()


def _dev(m):
    return torch.from_numpy(m.pos).cuda(), torch.from_numpy(m.faces).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _guarded(size, dtype):
    """A device buffer of size + GUARD elements, NaN (99 for integers) everywhere."""
    return torch.full((size + GUARD,), float("nan") if dtype.is_floating_point else 99, dtype=dtype, device="cuda")


def _tail_untouched(buf, size):
    t = buf[size:].cpu()
    return bool(torch.isnan(t).all()) if buf.dtype.is_floating_point else bool((t == 99).all())


def _entry(what, m, bvec=False):
    """(entry point, its leading arguments, scratch, scratch bytes, stream): pdg_<what> for triangles, the _cells
    entry point for quads."""
    from pdg.lib import lib, stream_handle
    pts, fcs = _dev(m)
    (n, dim), (nf, nv) = pts.shape, fcs.shape
    if what == "mesh_graph":
        nbytes = lib.pdg_mesh_graph_scratch_bytes(n, nf) if nv == 3 else lib.pdg_mesh_graph_cells_scratch_bytes(n, nf, nv)
    elif nv == 3:
        nbytes = lib.pdg_boundary_vectors_scratch_bytes(n, nf) if bvec else lib.pdg_mesh_fields_scratch_bytes(n, nf)
    else:
        nbytes = (lib.pdg_boundary_vectors_cells_scratch_bytes if bvec else lib.pdg_mesh_fields_cells_scratch_bytes)(n, nf, nv)
    if nv == 3:
        fn = getattr(lib, "pdg_p1_div_operator" if what == "div_operator" else f"pdg_{what}")
        head = (n, pts.data_ptr(), dim, nf, fcs.data_ptr())
    else:
        fn = getattr(lib, f"pdg_{what}_cells")
        head = (n, pts.data_ptr(), dim, nf, nv, fcs.data_ptr())
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    return fn, head, (pts, fcs, scratch), (scratch.data_ptr(), nbytes, stream_handle(pts.device))


def graph_raw(m, periodic):
    """pdg_mesh_graph[_cells] itself into guarded buffers: (edge_index, edge_attr) as numpy."""
    from pdg.devgraph import SIDE_MAX
    fn, head, keep, tail = _entry("mesh_graph", m)
    cap = 2 * m.faces.size + (4 * SIDE_MAX + 4 if periodic else 0)
    rows, cols, ea, cnt = (_guarded(cap, torch.int64), _guarded(cap, torch.int64), _guarded(cap, torch.float32),
                           _guarded(1, torch.int32))
    fn(*head, int(periodic), rows.data_ptr(), cols.data_ptr(), ea.data_ptr(), cap, cnt.data_ptr(), *tail)
    e = int(cnt[0].item())
    assert e >= 0
    assert _tail_untouched(rows, cap) and _tail_untouched(cols, cap) and _tail_untouched(ea, cap) and _tail_untouched(cnt, 1)
    return torch.stack([rows[:e], cols[:e]]).cpu().numpy(), ea[:e].cpu().numpy()


def labels_raw(m):
    fn, head, keep, tail = _entry("node_labels", m)
    n = m.num_nodes
    labels, info = _guarded(n, torch.int64), _guarded(3, torch.int32)
    fn(*head, labels.data_ptr(), info.data_ptr(), *tail)
    assert _tail_untouched(labels, n) and _tail_untouched(info, 3)
    return labels[:n].cpu().numpy(), info[:3].tolist()


def operator_raw(m):
    fn, head, keep, tail = _entry("div_operator", m)
    cap = 2 * m.faces.shape[1] * m.faces.size
    rows, cols, vals, cnt = (_guarded(cap, torch.int64), _guarded(cap, torch.int64), _guarded(cap, torch.float32),
                             _guarded(2, torch.int32))
    fn(*head, rows.data_ptr(), cols.data_ptr(), vals.data_ptr(), cap, cnt.data_ptr(), cnt[1:].data_ptr(), *tail)
    nnz, status = cnt[:2].tolist()
    assert _tail_untouched(rows, cap) and _tail_untouched(cols, cap) and _tail_untouched(vals, cap) and _tail_untouched(cnt, 2)
    return rows[:nnz].cpu().numpy(), cols[:nnz].cpu().numpy(), vals[:nnz].cpu().numpy(), status


def areas_raw(m):
    fn, head, keep, tail = _entry("nodal_areas", m)
    n = m.num_nodes
    area, bbox, status = _guarded(n, torch.float32), _guarded(4, torch.float32), _guarded(1, torch.int32)
    fn(*head, area.data_ptr(), bbox.data_ptr(), status.data_ptr(), *tail)
    assert _tail_untouched(area, n) and _tail_untouched(bbox, 4) and _tail_untouched(status, 1)
    return area[:n].cpu().numpy(), bbox[:4].cpu().numpy(), int(status[0].item())


def bvec_raw(m):
    fn, head, keep, tail = _entry("boundary_vectors", m, bvec=True)
    n = m.num_nodes
    vec, length, status = _guarded(2 * n, torch.float32), _guarded(n, torch.float32), _guarded(1, torch.int32)
    fn(*head, vec.data_ptr(), length.data_ptr(), status.data_ptr(), *tail)
    assert _tail_untouched(vec, 2 * n) and _tail_untouched(length, n) and _tail_untouched(status, 1)
    return vec[:2 * n].cpu().numpy().reshape(n, 2), length[:n].cpu().numpy(), int(status[0].item())


def _cells(m):
    return "quad" if m.faces.shape[1] == 4 else "triangle"


def _check_rounded(got, want, what):
    """tests/test_gpu_quadmesh.py's check of a rounded fp64 sum: one fp32 ulp, and the host's exact zeros."""
    g, w = got.astype(np.float64), want.astype(np.float64)
    err = np.abs(g - w)
    bound = 2.0 ** -23 * np.abs(w)
    ratio = float(np.max(err / np.maximum(bound, 1e-300)))
    print(f"{what}: bitwise equal {np.mean(got == want):.4f}, max err / bound {ratio:.3e}")
    assert np.all(err <= bound)
    assert not got[want == 0].any()
    return ratio


# --------------------------------------------------------------------------------------------------- the graph
@pytest.mark.parametrize("name", CASES)
def test_graph_is_the_host_graph(name):
    from pdg.devgraph import mesh_graph
    m = mesh(name)
    periodic = name in PERIODIC
    want_ei, want_ea = M.host_graph(m.pos, m.faces, periodic)
    ei, ea = graph_raw(m, periodic)
    assert np.array_equal(ei, want_ei)
    assert np.array_equal(_bits(ea), _bits(want_ea))
    if m.hub is not None and not name.startswith("refined"):
        assert (ei[0] == m.hub).sum() == M.valences(m.faces, m.num_nodes)[m.hub] * (2 if name.startswith("pinwheel") else 1)
    dei, dea = mesh_graph(*_dev(m), periodic, cells=_cells(m))
    assert dei.dtype == torch.int64 and dea.dtype == torch.float32 and dei.is_cuda
    assert np.array_equal(dei.cpu().numpy(), ei) and np.array_equal(_bits(dea.cpu().numpy()), _bits(ea))


@pytest.mark.parametrize("renumber", [None, 3])
def test_a_periodic_pair_on_a_mesh_edge_keeps_the_length(renumber):
    """The strip's left-right pairs are mesh edges too: flag bit 1 beside flag bit 0 on one column of a row of
    pdg_graph.hip.  The coalesced attribute is the length (the strip's width), by hand and not through the host."""
    from pdg import meshgen
    m = M.two_column_strip(renumber=renumber)
    ei, ea = graph_raw(m, True)
    width = np.float32(m.pos[:, 0].max() - m.pos[:, 0].min())
    left, right = np.where(m.pos[:, 0] == m.pos[:, 0].min())[0], np.where(m.pos[:, 0] == m.pos[:, 0].max())[0]
    got = {(a, b): w for a, b, w in zip(*ei.tolist(), ea.tolist())}
    assert len(got) == ei.shape[1]                                    # coalesced: every pair once
    for a in left.tolist():
        b = int(right[m.pos[right, 1] == m.pos[a, 1]][0])
        assert got[(a, b)] == width and got[(b, a)] == width and width > 0
    pr, pc = meshgen.periodic_pairs(m.pos)
    mesh_edges = set(zip(*M.host_graph(m.pos, m.faces, False)[0].tolist()))
    only = [e for e in zip(pr.tolist(), pc.tolist()) if e not in mesh_edges]
    assert len(only) == 8 and all(got[e] == 0.0 for e in only)       # lower <-> upper and the corners' diagonals


# -------------------------------------------------------------------------------------------------- the labels
@pytest.mark.parametrize("name", CASES)
def test_labels_are_the_host_restatement(name):
    from pdg import meshgen
    from pdg.devgraph import node_labels
    m = mesh(name)
    want, ncomp, next_ = meshgen.node_labels(m.pos, m.faces)
    assert np.array_equal(want, m.labels)
    got, info = labels_raw(m)
    pinched = name.startswith("pinwheel")
    assert info == [ncomp, next_, ST_NONMANIFOLD if pinched else 0]   # never ST_CAP, never a range error
    assert np.array_equal(got, want)
    if pinched:
        with pytest.raises(ValueError, match="non-manifold"):
            node_labels(*_dev(m), strict=False, cells=_cells(m))
    else:
        lab = node_labels(*_dev(m), strict=False, cells=_cells(m))
        assert lab.dtype == torch.int64 and lab.is_cuda and np.array_equal(lab.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ the operator
@pytest.mark.parametrize("name", CASES)
def test_operator_is_the_host_operator(name):
    from pdg import meshgen
    from pdg.devgraph import p1_divergence
    m = mesh(name)
    n = m.num_nodes
    rows, cols, vals = meshgen.cell_divergence_operator(m.pos, m.faces)
    grow, gcol, gval, status = operator_raw(m)
    assert status == 0
    assert np.array_equal(grow, rows) and np.array_equal(gcol, cols)
    key = grow * (2 * n) + gcol
    assert np.all(key[1:] > key[:-1])                                  # coalesced: sorted, every entry once
    got, want = gval.astype(np.float64), vals.astype(np.float64)
    err = np.abs(got - want)
    bound = 2.0 ** -23 * np.abs(want) + 1e-9 * np.abs(want).max()
    hub = rows == m.hub if m.hub is not None else np.zeros(len(rows), bool)
    print(f"{name}: nnz {len(want)}, max err / bound {np.max(err / bound):.3e}"
          + (f", on the hub's {int(hub.sum())} entries {np.max(err[hub] / bound[hub]):.3e}" if hub.any() else "")
          + f", bitwise equal {np.mean(gval == vals):.4f}")
    assert np.all(err <= bound)
    op = p1_divergence(*_dev(m), cells=_cells(m))
    assert op.is_coalesced() and op.shape == (n, 2 * n) and op.dtype == torch.float32
    assert np.array_equal(op.indices().cpu().numpy(), np.stack([grow, gcol]))
    assert np.array_equal(_bits(op.values().cpu().numpy()), _bits(gval))


# ------------------------------------------------------------------------------- areas and boundary vectors
@pytest.mark.parametrize("name", CASES)
def test_areas_and_boundary_vectors_are_the_host_restatement(name):
    from pdg import meshgen
    from pdg.devgraph import boundary_vectors, nodal_areas
    m = mesh(name)
    pinched = name.startswith("pinwheel")
    want, wbox = meshgen.nodal_areas(m.pos, m.faces)
    area, bbox, status = areas_raw(m)
    assert status == 0 and np.array_equal(_bits(bbox), _bits(wbox))
    _check_rounded(area, want, f"{name} area")
    assert np.all(area > 0)
    wvec, wlen = meshgen.boundary_vectors(m.pos, m.faces)
    bvec, blen, status = bvec_raw(m)
    assert status == (ST_NONMANIFOLD if pinched else 0)
    _check_rounded(bvec, wvec, f"{name} bvec")
    _check_rounded(blen, wlen, f"{name} blen")
    assert np.array_equal(blen > 0, m.labels != 0)
    if not pinched:                  # the invariants of tests/test_irregular_meshes_host.py, of the device's output
        check_area_and_closed_boundaries(m, area, bvec, f"{name} (device)")
        bv = boundary_vectors(*_dev(m), cells=_cells(m))
        assert np.array_equal(_bits(bv.vec.cpu().numpy()), _bits(bvec))
        assert np.array_equal(_bits(bv.length.cpu().numpy()), _bits(blen))
    out = nodal_areas(*_dev(m), cells=_cells(m))
    assert out.area.is_cuda and np.array_equal(_bits(out.area.cpu().numpy()), _bits(area))
    b = wbox.astype(np.float64)
    assert out.cell_area.dtype == torch.float64 and float(out.cell_area) == (b[1] - b[0]) * (b[3] - b[2])


def test_two_calls_are_bitwise_equal():
    """The atomics' arrival order differs between calls (the slots of the hub's 2049-slot operator row are claimed
    by atomicAdd); the sorted rows and everything computed from them must not."""
    m = mesh("disk683_renumbered")
    for fn in (lambda: graph_raw(m, False), lambda: labels_raw(m), lambda: operator_raw(m), lambda: areas_raw(m),
               lambda: bvec_raw(m)):
        first, second = fn(), fn()
        for a, b in zip(first, second):
            if isinstance(a, np.ndarray):
                assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
            else:
                assert a == b


# ------------------------------------------------------------------------------------------------- downstream
def test_refined_plate_feeds_the_model():
    """convert_mesh_to_graph on the refined periodic plate, bare (labels and operator from the mesh), then one forward
    of a 2-step model: the output of the host-built graph of the same arrays, as
    tests/test_gpu_devgraph.py::test_convert_mesh_to_graph_feeds_the_model has it for the grid."""
    from gnn_local_stress.models import EncodeProcessDecode
    from pdg import graph, meshgen
    from pdg.devgraph import convert_mesh_to_graph
    m = mesh("refined13_periodic")
    ei, ea = M.host_graph(m.pos, m.faces, True)
    rows, cols, vals = meshgen.p1_divergence_operator(m.pos, m.faces)
    mean = np.array([30.0, -20.0, 10.0], np.float32)
    s = meshgen.MeshSample(pos=m.pos, faces=m.faces, node_types=m.labels, edge_index=ei, edge_attr=ea, op_div_rows=rows,
                           op_div_cols=cols, op_div_vals=vals, mean_stress=mean,
                           local_stress=np.zeros((m.num_nodes, 3), np.float32))
    host = graph.sample_to_data(s).to("cuda")
    dev = convert_mesh_to_graph(*_dev(m), mean, divergence=True)
    assert torch.equal(dev.edge_index, host.edge_index) and torch.equal(dev.edge_attr, host.edge_attr)
    assert torch.equal(dev.nodes_types, host.nodes_types)
    assert torch.equal(dev.op_div_matrix.indices(), host.op_div_matrix.indices())
    want = host.op_div_matrix.values().double()
    assert bool(((dev.op_div_matrix.values().double() - want).abs() <= 2.0 ** -23 * want.abs() + 1e-9 * want.abs().max()).all())
    torch.manual_seed(69)
    stats = {k: torch.tensor(v) for k, v in {"mean_pos": 50.0, "std_pos": 29.0, "mean_mean_stress": 0.0,
                                             "std_mean_stress": 60.0, "mean_local_stress": 0.0,
                                             "std_local_stress": 60.0, "mean_edge_weight": 9.0,
                                             "std_edge_weight": 4.0}.items()}
    model = EncodeProcessDecode(input_edges_features_size=1, message_passing_steps=2, latent_size=128,
                                input_nodes_features_size=6, output_nodes_features_size=3, **stats).to("cuda")
    with torch.no_grad():
        a = model(host).local_stress
        b = model(dev).local_stress
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_cell_solve_on_the_refined_plate():
    """gnn_local_stress.fem's P1 cell solve (csrc/pdg_fem.hip: one thread walks a representative's rowptr / item row)
    on the refined periodic plate, valences 3 to 16: the assertions, bound and reference of
    tests/test_gpu_fem.py::test_against_the_direct_solve.  tests/fem_ref.py needs nothing of a grid: it pairs the
    sides by exact coordinates and assembles from the faces."""
    import fem_ref as R
    from gnn_local_stress import fem
    rtol, bound = 1e-10, 2.0 ** -22
    m = mesh("refined13_periodic")
    c = R.cell(m.pos, m.faces)
    pts, fcs = _dev(m)
    plan = fem.FemPlan.from_mesh(pts, fcs)
    assert np.array_equal(plan.rep.cpu().numpy(), c.rep)
    rp, item = plan.item_rowptr.cpu().numpy(), plan.item.cpu().numpy()
    key = c.rep[m.faces.ravel()]
    assert np.array_equal(np.diff(rp), np.bincount(key, minlength=len(c.rep))) and np.diff(rp).max() >= 12
    assert np.array_equal(item, np.argsort(key, kind="stable"))        # every row ascending
    out = fem.solve_cells(plan, pts, torch.eye(3, dtype=torch.float64, device="cuda").reshape(1, 3, 3), rtol=rtol)
    table = out.table.cpu().numpy()[0]
    stress = out.stress.cpu().numpy().astype(np.float64)
    ut = out.ut.cpu().numpy()
    for l, eps in enumerate(R.UNIT):
        ref = R.fields(c, eps, R.solve_direct(c, eps)[0])
        its = R.pcg(c, eps, rtol=rtol)[1]
        err = np.abs(stress[l] - ref.stress).max() / np.abs(ref.stress).max()
        res = R.residual(c, eps, ut[l])
        print(f"case {l}: {int(table[l, 0])} iterations (numpy PCG {its}), stress error {err:.3e} (bound {bound:.3e}), "
              f"table residual {table[l, 2]:.3e}, recomputed {res:.3e}")
        assert table[l, 3] == fem.CONVERGED
        assert err <= bound
        assert table[l, 0] <= 2 * its
        assert table[l, 2] <= rtol
        assert res <= 2 * rtol
        assert abs(table[l, 1] - np.linalg.norm(R.rhs(c, eps)[0])) <= 1e-9 * table[l, 1]
        assert np.abs(ut[l][c.reps].mean(0)).max() <= 1e-12 * np.abs(ut[l]).max()
        assert np.array_equal(ut[l], ut[l][c.rep])
        e_err = np.abs(out.strain[l].cpu().numpy() - ref.strain).max() / np.abs(ref.strain).max()
        assert e_err <= bound
        assert np.abs(out.mean_stress[0, l].cpu().numpy() - ref.mean_stress).max() <= 1e-9 * np.abs(ref.mean_stress).max()
        assert np.abs(out.mean_stress_material[0, l].cpu().numpy() - ref.mean_stress_material).max() \
            <= 1e-9 * np.abs(ref.mean_stress_material).max()
        if l == 0:
            assert abs(float(out.material_area[0]) - ref.material_area) <= 1e-12 * ref.material_area
            assert float(out.cell_area[0]) == ref.cell_area
