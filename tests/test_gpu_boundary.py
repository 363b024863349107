"""The boundary residuals on the device against their host restatements: pdg_boundary_vectors against
pdg.meshgen.boundary_vectors, pdg_boundary_residuals / pdg_boundary_residuals_bwd against tests/boundary_ref.py,
and the Python layer built on them (devgraph.boundary_vectors, gnn_local_stress.boundary).

Every bound is derived, none measured.  With u = 2^-53:

* vectors: both sides round one fp64 value to fp32, formed from the same terms in the same order; the fp64 values
  differ by a few u relative at most (the square root), so the results lie at most one fp32 ulp apart:
  2^-23 |want|, and exact zeros sit where the restatement has exact zeros;
* table: a column is a sum of at most n terms in some order, n = the graph's rows plus its periodic edges:
  |got - want| <= 2 n u sum |terms| for the two summations (the restatement's is math.fsum's, exact to one
  rounding).  A term is formed with a handful of fp64 roundings: fx = sxx mx + sxy my (exact products, one
  addition: u (|sxx mx| + |sxy my|)), |f|^2 / blen (three multiplications and additions, one division) and
  |sigma(n) - sigma(src)|^2 likewise: below 8 u times the term taken on absolute values, on each side, hence
  (2 n + 16) u mag with mag the sum of the terms taken on absolute values (boundary_ref's third result).  L_int,
  L_ext and n_pairs have exact terms and fall under the same bound;
* gradient: one fp32 rounding of an fp64 value whose own error is a few u of the sum of the absolute values of
  its terms: 2^-23 mag per element.
"""
import numpy as np
import pytest
import torch

import boundary_ref as R
from test_meshfields_host import renumbered

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _plate(n, hole=0.0, seed=3):
    from pdg import meshgen
    return meshgen.hole_plate(n=n, hole_radius=hole, seed=seed)


SAMPLES = {"plate9": _plate(9), "hole13": _plate(13, 0.2), "plate35": _plate(35)}


def _meshes():
    a, b, c = (SAMPLES[k] for k in ("plate9", "hole13", "plate35"))
    assert a.num_nodes == 81 and c.num_nodes == 1225 and b.num_nodes < 169
    pos2, faces2, _ = renumbered(b.pos, b.faces)
    z = np.random.default_rng(1).uniform(-1, 1, (b.num_nodes, 1)).astype(np.float32)
    return {"plate9": (a.pos, a.faces), "hole13": (b.pos, b.faces), "plate35": (c.pos, c.faces),
            "renumbered": (pos2, faces2), "points3d": (np.concatenate([b.pos, z], 1), b.faces)}


MESHES = _meshes()


def _dev(pos, faces):
    return (torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float32)).cuda(),
            torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)).cuda())


def _vectors_raw(pos, faces):
    """pdg_boundary_vectors itself: (bvec, blen, status) as numpy, no exception for any status."""
    from pdg.lib import lib, stream_handle
    pts, fcs = _dev(pos, faces)
    n, dim = pts.shape
    nf = len(fcs)
    nbytes = lib.pdg_boundary_vectors_scratch_bytes(n, nf)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    bvec = torch.full((n, 2), -7.0, dtype=torch.float32, device="cuda")
    blen = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    status = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    lib.pdg_boundary_vectors(n, pts.data_ptr(), dim, nf, fcs.data_ptr() if nf else None, bvec.data_ptr(),
                             blen.data_ptr(), status.data_ptr(), scratch.data_ptr(), nbytes, stream_handle(pts.device))
    return bvec.cpu().numpy(), blen.cpu().numpy(), int(status.item())


def _check_vectors(got, want, what):
    for g, w, nm in ((got[0], want[0], "bvec"), (got[1], want[1], "blen")):
        err = np.abs(g.astype(np.float64) - w.astype(np.float64))
        bound = 2.0 ** -23 * np.abs(w.astype(np.float64))
        print(f"{what} {nm}: bitwise equal {np.mean(g == w):.4f}, max err / bound "
              f"{np.max(err / np.maximum(bound, 1e-300)):.3e}")
        assert np.all(err <= bound)
        assert not g[w == 0].any()


@pytest.mark.parametrize("name", sorted(MESHES))
def test_vectors_are_the_host_restatement(name):
    from pdg import meshgen
    from pdg.devgraph import boundary_vectors
    pos, faces = MESHES[name]
    want = meshgen.boundary_vectors(pos, faces)
    bvec, blen, status = _vectors_raw(pos, faces)
    assert status == 0
    _check_vectors((bvec, blen), want, name)
    assert int((blen > 0).sum()) == int((want[1] > 0).sum()) > 0
    out = boundary_vectors(*_dev(pos, faces))
    assert out.vec.is_cuda and out.vec.dtype == torch.float32 and np.array_equal(out.vec.cpu().numpy(), bvec)
    assert out.length.shape == (len(pos),) and np.array_equal(out.length.cpu().numpy(), blen)
    # two calls agree bitwise: the sums do not depend on the order in which the slot atomics land
    again = _vectors_raw(pos, faces)
    assert np.array_equal(again[0], bvec) and np.array_equal(again[1], blen)


def _clean_call_still_works():
    from pdg import meshgen
    pos, faces = MESHES["hole13"]
    bvec, blen, status = _vectors_raw(pos, faces)
    assert status == 0
    _check_vectors((bvec, blen), meshgen.boundary_vectors(pos, faces), "clean call")


def test_status_out_of_range_face_is_ignored():
    from pdg.devgraph import boundary_vectors
    pos, faces = MESHES["hole13"]
    n = len(pos)
    base = _vectors_raw(pos, faces)
    bad = np.concatenate([faces[:7], np.array([[0, 1, n], [-1, 2, 3]], np.int64), faces[7:]])
    bvec, blen, status = _vectors_raw(pos, bad)
    assert status == 1 and np.array_equal(bvec, base[0]) and np.array_equal(blen, base[1])
    with pytest.raises(ValueError, match="outside"):
        boundary_vectors(*_dev(pos, bad))
    with pytest.raises(ValueError, match="triangle"):
        boundary_vectors(_dev(pos, faces)[0], torch.zeros(2, 4, dtype=torch.int64, device="cuda"))
    _clean_call_still_works()


def test_status_two_triangles_touching_at_one_vertex():
    from pdg import meshgen
    from pdg.devgraph import boundary_vectors
    pos = np.array([[0, 0], [2, 0], [1, 1], [0, 2], [2, 2.5]], np.float32)
    faces = np.array([[0, 1, 2], [2, 4, 3]], np.int64)
    bvec, blen, status = _vectors_raw(pos, faces)
    assert status == 2                                  # node 2 holds four boundary edges; outputs still written
    _check_vectors((bvec, blen), meshgen.boundary_vectors(pos, faces), "bow tie")
    assert np.all(blen > 0)
    with pytest.raises(ValueError, match="non-manifold"):
        boundary_vectors(*_dev(pos, faces))
    _clean_call_still_works()


def test_status_zero_area_boundary_face():
    from pdg import meshgen
    from pdg.devgraph import boundary_vectors
    pos = np.array([[0, 0], [1, 0], [0, 1], [0.5, 0.5]], np.float32)
    faces = np.array([[0, 1, 2], [1, 2, 3]], np.int64)   # the second face is flat: 3 is the midpoint of (1, 2)
    bvec, blen, status = _vectors_raw(pos, faces)
    assert status == 4
    want = meshgen.boundary_vectors(pos, faces)
    _check_vectors((bvec, blen), want, "flat face")
    # node 3 lies on flat edges only: length and no vector
    assert blen[3] > 0 and not bvec[3].any()
    out = boundary_vectors(*_dev(pos, faces))           # no error
    assert np.array_equal(out.length.cpu().numpy(), blen)
    _clean_call_still_works()


def test_status_no_faces():
    pos, _ = MESHES["hole13"]
    bvec, blen, status = _vectors_raw(pos, np.zeros((0, 3), np.int64))
    assert status == 0 and not bvec.any() and not blen.any()
    _clean_call_still_works()


# ------------------------------------------------------------------------------------------ per-graph residuals
class Case:
    """The three plates as one batch (graph 0 has no hole, graph 2 spans more than 1,024 rows), host vectors and
    labels, one random field, the graph plan, the restatement's table; `empty` inserts a graph without rows
    between graph 0 and graph 1."""

    def __init__(self, empty=False):
        from pdg import meshgen
        from pdg.plan import GraphPlan
        names = ("plate9", "hole13", "plate35")
        ss = [SAMPLES[k] for k in names]
        counts = [s.num_nodes for s in ss]
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.graph_rows = [(int(off[i]), int(off[i + 1])) for i in range(3)]
        if empty:
            counts = [counts[0], 0, counts[1], counts[2]]
        self.ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.B, self.N = len(counts), int(self.ptr[-1])
        self.samples = ss
        self.ei = np.concatenate([s.edge_index + off[i] for i, s in enumerate(ss)], 1)
        self.ea = np.concatenate([s.edge_attr for s in ss])
        vecs = [meshgen.boundary_vectors(s.pos, s.faces) for s in ss]
        self.bvec = np.concatenate([v[0] for v in vecs])
        self.blen = np.concatenate([v[1] for v in vecs])
        self.labels = np.concatenate([s.node_types for s in ss])
        self.sigma = np.random.default_rng(7).normal(0.0, 50.0, (self.N, 3)).astype(np.float32)
        self.ref = R.residuals(self.ptr, self.sigma, self.bvec, self.blen, self.labels, (self.ei, self.ea))
        self.d_ptr = torch.from_numpy(self.ptr.astype(np.int32)).cuda()
        self.d_sigma = torch.from_numpy(self.sigma).cuda()
        self.d_bvec = torch.from_numpy(self.bvec).cuda()
        self.d_blen = torch.from_numpy(self.blen).cuda()
        self.d_labels = torch.from_numpy(self.labels).cuda()
        self.d_ei = torch.from_numpy(self.ei).cuda()
        self.d_ea = torch.from_numpy(self.ea).cuda()
        plan = GraphPlan(self.d_ei, self.N, self.d_ptr)
        plan.validate()
        self.plan = plan
        self.edges = (plan.rowptr_dst, plan.src, plan.perm, self.d_ea)

    def terms(self):
        """Per graph: its rows plus its periodic edges."""
        zero = self.ea == 0
        dst = self.ei[1][zero]
        return np.array([(self.ptr[g + 1] - self.ptr[g]) + np.sum((dst >= self.ptr[g]) & (dst < self.ptr[g + 1]))
                         for g in range(self.B)], np.float64)


@pytest.fixture(scope="module")
def case():
    return Case()


def _res(d_ptr, d_sigma, d_bvec, d_blen, d_labels, edges):
    from pdg.lib import lib, ptr as p_, stream_handle
    b = d_ptr.numel() - 1
    table = torch.full((b, 9), -7.0, dtype=torch.float64, device="cuda")
    argmax = torch.full((b,), -7, dtype=torch.int32, device="cuda")
    lib.pdg_boundary_residuals(b, d_ptr.data_ptr(), d_sigma.data_ptr(), d_bvec.data_ptr(), d_blen.data_ptr(),
                               d_labels.data_ptr(), *(p_(e) for e in (edges or (None,) * 4)), table.data_ptr(),
                               argmax.data_ptr(), stream_handle(d_sigma.device))
    return table, argmax


def _bwd(d_ptr, d_sigma, d_bvec, d_blen, d_labels, edges, table, gt, gp):
    from pdg.lib import lib, ptr as p_, stream_handle
    out = torch.full_like(d_sigma, -7.0)
    lib.pdg_boundary_residuals_bwd(d_ptr.numel() - 1, d_ptr.data_ptr(), d_sigma.data_ptr(), d_bvec.data_ptr(),
                                   d_blen.data_ptr(), d_labels.data_ptr(), *(p_(e) for e in (edges or (None,) * 4)),
                                   table.data_ptr(), p_(gt), p_(gp), out.data_ptr(), stream_handle(d_sigma.device))
    return out


def _case_res(c, sigma=None, edges="plan"):
    return _res(c.d_ptr, c.d_sigma if sigma is None else sigma, c.d_bvec, c.d_blen, c.d_labels,
                c.edges if edges == "plan" else None)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _check_table(got, argmax, ref, terms, what):
    want, wam, mag = ref
    bound = (2.0 * terms[:, None] + 16.0) * U * mag
    err = np.abs(got - want)
    pos = bound > 0
    print(f"{what}: max err / bound {np.max(err[pos] / bound[pos]):.3e}, argmax {argmax.tolist()}, "
          f"T2 / L_int {(got[:, 2] / np.maximum(got[:, 0], 1e-300)).tolist()}")
    assert np.all(err <= bound)
    assert np.array_equal(argmax, wam)


def test_table_against_the_restatement(case):
    table, argmax = _case_res(case)
    _check_table(table.cpu().numpy(), argmax.cpu().numpy(), case.ref, case.terms(), "three plates")
    got = table.cpu().numpy()
    assert got[0, 0] == 0 and got[0, 2] == 0 and argmax[0] == -1          # no hole
    assert got[1, 0] > 0 and got[1, 2] > 0 and argmax[1] >= 0 and np.all(got[:, 8] > 0) and np.all(got[:, 7] > 0)
    side = [int(np.sum(s.pos[:, 0] == s.pos[:, 0].max())) for s in case.samples]
    assert got[:, 8].tolist() == [2.0 * k + 2 for k in side]
    # two calls agree bitwise
    t2, a2 = _case_res(case)
    assert torch.equal(_bits(t2), _bits(table)) and torch.equal(a2, argmax)


def test_null_edges_leave_the_periodic_columns_zero(case):
    table, argmax = _case_res(case, edges=None)
    full, fam = _case_res(case)
    assert not table[:, 7:].any() and torch.equal(_bits(table[:, :7]), _bits(full[:, :7])) and torch.equal(argmax, fam)
    ref = R.residuals(case.ptr, case.sigma, case.bvec, case.blen, case.labels, None)
    _check_table(table.cpu().numpy(), argmax.cpu().numpy(), ref, np.diff(case.ptr).astype(np.float64), "no edges")


def test_an_empty_graph_in_the_middle(case):
    c = Case(empty=True)
    table, argmax = _case_res(c)
    _check_table(table.cpu().numpy(), argmax.cpu().numpy(), c.ref, c.terms(), "with an empty graph")
    assert not table[1].any() and int(argmax[1]) == -1
    full, fam = _case_res(case)
    keep = [0, 2, 3]
    assert torch.equal(_bits(table[keep]), _bits(full)) and torch.equal(argmax[keep], fam)


def test_each_graph_alone_gets_its_batch_row_bitwise(case):
    from pdg.plan import GraphPlan
    full, fam = _case_res(case)
    for g, (n0, n1) in enumerate(case.graph_rows):
        s = case.samples[g]
        ei = torch.from_numpy(s.edge_index).cuda()
        plan = GraphPlan(ei, n1 - n0)
        plan.validate()
        ptr = torch.tensor([0, n1 - n0], dtype=torch.int32, device="cuda")
        alone, aam = _res(ptr, case.d_sigma[n0:n1].contiguous(), case.d_bvec[n0:n1].contiguous(),
                          case.d_blen[n0:n1].contiguous(), case.d_labels[n0:n1].contiguous(),
                          (plan.rowptr_dst, plan.src, plan.perm, torch.from_numpy(s.edge_attr).cuda()))
        assert torch.equal(_bits(alone[0]), _bits(full[g])) and int(aam[0]) == int(fam[g]), g


def test_nan_rule(case):
    full, fam = _case_res(case)
    n0, n1 = case.graph_rows[1]
    hole = n0 + int(np.flatnonzero(case.labels[n0:n1] == -1)[3])
    ext = n0 + int(np.flatnonzero(case.labels[n0:n1] == 1)[5])
    for node, nan_cols, fine_cols in ((hole, [2, 3, 4], [0, 1, 5, 6, 7, 8]), (ext, [5, 6], [0, 1, 2, 3, 4, 8])):
        sigma = case.d_sigma.clone()
        sigma[node, 2] = float("nan")        # sxy enters both components of the force
        table, argmax = _case_res(case, sigma=sigma)
        assert torch.isnan(table[1, nan_cols]).all() and int(argmax[1]) == -1
        assert torch.equal(_bits(table[1, fine_cols]), _bits(full[1, fine_cols]))
        for g in (0, 2):    # the other graphs are bitwise unchanged
            assert torch.equal(_bits(table[g]), _bits(full[g])) and int(argmax[g]) == int(fam[g])
    # rows that take no part change nothing, whatever they hold: a zero, negative or NaN length excludes a node
    blen = case.d_blen.clone()
    ext_nodes = np.flatnonzero(case.labels[n0:n1] == 1)[:3] + n0
    blen[torch.from_numpy(ext_nodes).cuda()] = torch.tensor([0.0, -1.0, float("nan")], device="cuda")
    bvec = case.d_bvec.clone()
    bvec[torch.from_numpy(ext_nodes).cuda()] = float("nan")
    t2, a2 = _res(case.d_ptr, case.d_sigma, bvec, blen, case.d_labels, case.edges)
    b2 = case.blen.copy()
    b2[ext_nodes] = [0.0, -1.0, np.nan]
    v2 = case.bvec.copy()
    v2[ext_nodes] = np.nan
    ref = R.residuals(case.ptr, case.sigma, v2, b2, case.labels, (case.ei, case.ea))
    assert np.isfinite(ref[0]).all()
    _check_table(t2.cpu().numpy(), a2.cpu().numpy(), ref, case.terms(), "excluded nodes")


def _check_grad(got, want, mag, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    err = np.abs(got.astype(np.float64)[~nan] - want[~nan])
    bound = 2.0 ** -23 * mag[~nan]
    print(f"{what}: max err / bound {np.max(err[bound > 0] / bound[bound > 0]):.3e}, NaN elements {int(nan.sum())}, "
          f"non-zero rows {int(np.any(want != 0, 1).sum())}")
    assert np.all(err <= bound)
    assert not got[~nan][mag[~nan] == 0].any()          # exact zeros where no term applies


@pytest.mark.parametrize("term", ["traction", "periodic", "both"])
def test_gradient_against_the_restatement(case, term):
    table, _ = _case_res(case)
    gt = np.array([0.7, 1.3, -0.4]) if term != "periodic" else None
    gp = np.array([2.0, -0.5, 0.9]) if term != "traction" else None
    d = [None if g is None else torch.from_numpy(g).cuda() for g in (gt, gp)]
    got = _bwd(case.d_ptr, case.d_sigma, case.d_bvec, case.d_blen, case.d_labels, case.edges, table, *d)
    want, mag = R.residuals_grad(case.ptr, case.sigma, case.bvec, case.blen, case.labels, (case.ei, case.ea),
                                 table.cpu().numpy(), gt, gp)
    _check_grad(got.cpu().numpy(), want, mag, term)
    assert np.isfinite(want).all() and float(got.abs().max()) > 0
    if term == "traction":
        assert not got[case.d_labels != -1].any()
    again = _bwd(case.d_ptr, case.d_sigma, case.d_bvec, case.d_blen, case.d_labels, case.edges, table, *d)
    assert torch.equal(_bits(again), _bits(got))


def test_gradient_nan_rows_zero_weights_and_null_edges(case):
    table, _ = _case_res(case)
    broken = table.clone()
    broken[1, 0] = 0.0      # the hole plate's L_int
    broken[2, 8] = 0.0      # the large plate's n_pairs
    ones = torch.ones(3, dtype=torch.float64, device="cuda")
    got = _bwd(case.d_ptr, case.d_sigma, case.d_bvec, case.d_blen, case.d_labels, case.edges, broken, ones, ones)
    want, mag = R.residuals_grad(case.ptr, case.sigma, case.bvec, case.blen, case.labels, (case.ei, case.ea),
                                 broken.cpu().numpy(), np.ones(3), np.ones(3))
    assert np.isnan(want).any()
    _check_grad(got.cpu().numpy(), want, mag, "zero denominators")
    # both weights NULL, or zero: exact zeros everywhere, NaN inputs included
    sigma = case.d_sigma.clone()
    sigma[5] = float("nan")
    zeros = torch.zeros(3, dtype=torch.float64, device="cuda")
    for gt, gp in ((None, None), (zeros, zeros)):
        out = _bwd(case.d_ptr, sigma, case.d_bvec, case.d_blen, case.d_labels, case.edges, broken, gt, gp)
        assert not out.any()
    # without edges the periodic term is 0 and the traction term what it was
    a = _bwd(case.d_ptr, case.d_sigma, case.d_bvec, case.d_blen, case.d_labels, None, table, ones, ones)
    b = _bwd(case.d_ptr, case.d_sigma, case.d_bvec, case.d_blen, case.d_labels, case.edges, table, ones, None)
    assert torch.equal(_bits(a), _bits(b))


def test_both_launches_replay_from_a_captured_graph(case):
    from pdg.lib import lib, stream_handle
    gt = torch.tensor([0.7, 1.3, -0.4], dtype=torch.float64, device="cuda")
    gp = torch.tensor([2.0, -0.5, 0.9], dtype=torch.float64, device="cuda")
    eager_t, eager_a = _case_res(case)
    eager_o = _bwd(case.d_ptr, case.d_sigma, case.d_bvec, case.d_blen, case.d_labels, case.edges, eager_t, gt, gp)
    table = torch.full((3, 9), -7.0, dtype=torch.float64, device="cuda")
    argmax = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    out = torch.full_like(case.d_sigma, -7.0)
    common = [t.data_ptr() for t in (case.d_ptr, case.d_sigma, case.d_bvec, case.d_blen, case.d_labels, *case.edges)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = stream_handle(out.device)
        lib.pdg_boundary_residuals(3, *common, table.data_ptr(), argmax.data_ptr(), s)
        lib.pdg_boundary_residuals_bwd(3, *common, table.data_ptr(), gt.data_ptr(), gp.data_ptr(), out.data_ptr(), s)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(table), _bits(eager_t)) and torch.equal(argmax, eager_a)
    assert torch.equal(_bits(out), _bits(eager_o))


def test_python_layer_is_the_two_launches(case):
    from gnn_local_stress import boundary as Bd
    from pdg import graph
    from pdg.lib import lib
    from pdg.plan import plan_for
    batch = graph.Data(edge_index=case.d_ei, edge_attr=case.d_ea, nodes_types=case.d_labels.reshape(-1, 1),
                       pos=torch.zeros(case.N, 2, device="cuda"), ptr=torch.from_numpy(case.ptr),
                       boundary_vec=case.d_bvec, boundary_len=case.d_blen)
    plan_for(batch).validate()
    table, argmax = _case_res(case)

    def run(fn):
        calls, names = lib.calls, []
        lib.hook = names.append
        try:
            out = fn()
        finally:
            lib.hook = None
        return out, names, lib.calls - calls

    r, names, n = run(lambda: Bd.boundary_residuals(case.d_sigma, batch))
    assert names == ["pdg_boundary_residuals"] and n == 1
    for k, col in (("L_int", 0), ("L_ext", 1), ("T2", 2), ("P2", 7), ("n_pairs", 8)):
        assert getattr(r, k).dtype == torch.float64 and torch.equal(_bits(getattr(r, k)), _bits(table[:, col])), k
    assert torch.equal(_bits(r.F_int), _bits(table[:, 3:5])) and torch.equal(_bits(r.hole_force), _bits(table[:, 3:5]))
    assert torch.equal(_bits(r.F_ext), _bits(table[:, 5:7])) and torch.equal(_bits(r.cell_force), _bits(table[:, 5:7]))
    assert torch.equal(_bits(r.traction_rms), _bits(torch.sqrt(table[:, 2] / table[:, 0])))
    assert torch.equal(_bits(r.periodic_rms), _bits(torch.sqrt(table[:, 7] / table[:, 8])))
    assert torch.isnan(r.traction_rms[0]) and torch.isnan(r.traction_max[0])        # 0 / 0 stays NaN: no hole
    assert r.argmax.dtype == torch.int64 and torch.equal(r.argmax, argmax.long())
    assert r.node.tolist() == [-1, int(argmax[1]) + int(case.ptr[1]), -1]
    fx, fy, _, _ = R.forces(case.sigma, case.bvec)
    i = int(r.node[1])
    q = np.sqrt(fx[i] * fx[i] + fy[i] * fy[i]) / case.blen[i]
    assert abs(float(r.traction_max[1]) - q) <= 8 * U * q
    assert float(r.traction_max[1]) >= float(r.traction_rms[1]) > 0
    r0, names, n = run(lambda: Bd.boundary_residuals(case.d_sigma, batch, periodic=False))
    assert n == 1 and not r0.P2.any() and torch.isnan(r0.periodic_rms).all()
    assert torch.equal(_bits(r0.T2), _bits(r.T2))
    gp = torch.tensor([2.0, -0.5, 0.9], dtype=torch.float64, device="cuda")
    want = _bwd(case.d_ptr, case.d_sigma, case.d_bvec, case.d_blen, case.d_labels, case.edges, table,
                torch.full((3,), 1.5, dtype=torch.float64, device="cuda"), gp)
    g, names, n = run(lambda: Bd.boundary_residuals_grad(case.d_sigma, batch, traction=1.5, periodic=gp))
    assert names == ["pdg_boundary_residuals", "pdg_boundary_residuals_bwd"] and n == 2
    assert g.dtype == torch.float32 and torch.equal(_bits(g), _bits(want))
    # explicit vectors are the batch's own; without any, the error says how to get them
    bare = graph.Data(edge_index=case.d_ei, edge_attr=case.d_ea, nodes_types=case.d_labels,
                      pos=torch.zeros(case.N, 2, device="cuda"), ptr=torch.from_numpy(case.ptr))
    r2 = Bd.boundary_residuals(case.d_sigma, bare, case.d_bvec, case.d_blen)
    assert torch.equal(_bits(r2.T2), _bits(r.T2)) and torch.equal(_bits(r2.P2), _bits(r.P2))
    with pytest.raises(ValueError, match="boundary=True"):
        Bd.boundary_residuals(case.d_sigma, bare)
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        Bd.boundary_residuals(case.d_sigma[:, :2], batch)
    with pytest.raises(ValueError, match="boundary_vec must be"):
        Bd.boundary_residuals(case.d_sigma, batch, case.d_bvec[:5], case.d_blen)
    with pytest.raises(ValueError, match="one value per graph"):
        Bd.boundary_residuals_grad(case.d_sigma, batch, traction=torch.ones(2, device="cuda"))
