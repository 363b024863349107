"""The fused physics loss on the device (pdg_phys_loss_fwd, pdg_phys_loss_bwd, pdg_loss_reduce_phys;
csrc/pdg_physloss.hip) against its fp64 host restatement (tests/physloss_ref.py), on the smallest inputs at which
the kernels can still go wrong: one batch of four triangle plates (periodic with a hole; not periodic, so no jump
term; no hole, so no traction term; more rows than the per-graph workgroup has threads) and one quad plate.

Bounds, none measured:

* table and loss: 1e-10 relative, the bound the criteria, homogenisation and boundary kernels are held to (both
  sides form the same fp64 terms; they differ by the order of at most a few thousand additions);
* gradient rows: one fp32 rounding of an fp64 value whose own error is a few 2^-53 of the sum of the absolute
  values of its terms, as tests/test_gpu_boundary.py derives it: 2^-23 mag per element, with the old value's
  magnitude added to mag under `accumulate` (it is one more term of the sum that is rounded once).
"""
import numpy as np
import pytest
import torch

import physloss_ref as R

pytestmark = pytest.mark.gpu

REL = 1e-10
SCALE = np.array([0.7 / 4, 1.3 / 4, 0.4 / 4], np.float32)


class Case(R.Inputs):
    def __init__(self, samples):
        from pdg.plan import GraphPlan
        super().__init__(samples)
        c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.d_ptr = c(self.ptr.astype(np.int32))
        self.d_y, self.d_affine = c(self.y), c(self.affine)
        self.d_bvec, self.d_blen, self.d_labels = c(self.bvec), c(self.blen), c(self.labels)
        self.d_area, self.d_cell, self.d_target = c(self.area), c(self.cell), c(self.target)
        self.d_ea = c(self.ea)
        plan = GraphPlan(c(self.ei), self.N, self.d_ptr)
        plan.validate()
        self.plan = plan

    def dev(self, boundary=True, edges=True, mean=True, with_denom=True, **over):
        """The ten group arguments as device tensors (None for a group that is not given)."""
        v = dict(bvec=self.d_bvec, blen=self.d_blen, labels=self.d_labels, rowptr=self.plan.rowptr_dst,
                 src=self.plan.src, perm=self.plan.perm, ea=self.d_ea, area=self.d_area, denom=self.d_cell,
                 target=self.d_target)
        v.update(over)
        if not boundary:
            v.update(bvec=None, blen=None, labels=None)
        if not edges:
            v.update(rowptr=None, src=None, perm=None, ea=None)
        if not mean:
            v.update(area=None, target=None, denom=None)
        if not with_denom:
            v.update(denom=None)
        return [v[k] for k in ("bvec", "blen", "labels", "rowptr", "src", "perm", "ea", "area", "denom", "target")]


@pytest.fixture(scope="module")
def cases():
    tri, quad = R.cases()
    assert tri[3].num_nodes > 1024      # each thread of the per-graph workgroup owns more than one row
    return {"tri": Case(tri), "quad": Case(quad)}


def _fwd(c, groups, y=None, ptr=None, table=None, loss=None):
    from pdg.lib import lib, ptr as p_, stream_handle
    d_ptr = c.d_ptr if ptr is None else ptr
    b = d_ptr.numel() - 1
    table = torch.full((b, 12), -7.0, dtype=torch.float64, device="cuda") if table is None else table
    loss = torch.full((b, 3), -7.0, dtype=torch.float32, device="cuda") if loss is None else loss
    lib.pdg_phys_loss_fwd(b, d_ptr.data_ptr(), (c.d_y if y is None else y).data_ptr(), c.d_affine.data_ptr(),
                          *(p_(g) for g in groups), table.data_ptr(), loss.data_ptr(), stream_handle(table.device))
    return table, loss


def _bwd(c, groups, table, scale, accumulate=False, gy=None, y=None):
    from pdg.lib import lib, ptr as p_, stream_handle
    out = torch.full_like(c.d_y, -7.0) if gy is None else gy.clone()
    sc = torch.from_numpy(np.asarray(scale, np.float32)).cuda()
    lib.pdg_phys_loss_bwd(c.B, c.d_ptr.data_ptr(), c.N, (c.d_y if y is None else y).data_ptr(), c.d_affine.data_ptr(),
                          *(p_(g) for g in groups), table.data_ptr(), sc.data_ptr(), int(accumulate), out.data_ptr(),
                          stream_handle(out.device))
    return out


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _check_table(got, loss, want, what):
    err = np.abs(got - want)
    bound = REL * np.abs(want)
    print(f"{what}: max relative error {np.max(err[want != 0] / np.abs(want[want != 0])):.3e}; loss {loss.tolist()}")
    assert np.all(err <= bound)                      # an exact zero where the restatement has one
    assert np.array_equal(loss, got[:, 9:12].astype(np.float32))


@pytest.mark.parametrize("name", ["tri", "quad"])
@pytest.mark.parametrize("denom", [True, False])
def test_table_and_loss_against_the_restatement(cases, name, denom):
    c = cases[name]
    table, loss = _fwd(c, c.dev(with_denom=denom))
    want, _ = R.forward(c.ptr, c.y, c.affine, **c.groups(denom))
    got = table.cpu().numpy()
    _check_table(got, loss.cpu().numpy(), want, f"{name} denom={denom}")
    assert np.all(got[:, 9:12][want[:, 9:12] != 0] > 0)
    if name == "tri":
        assert got[1, 3] == 0 and got[1, 10] == 0 and got[2, 0] == 0 and got[2, 9] == 0     # the absent terms
        assert got[0, 9] > 0 and got[0, 10] > 0 and np.all(got[:, 11] > 0) and got[3, 9] > 0 and got[3, 10] > 0
    # from call to call
    t2, l2 = _fwd(c, c.dev(with_denom=denom))
    assert torch.equal(_bits(t2), _bits(table)) and torch.equal(_bits(l2), _bits(loss))


def test_null_groups_are_absent_terms(cases):
    c = cases["tri"]
    full, _ = _fwd(c, c.dev())
    for drop, cols in (("boundary", [0, 1, 9]), ("edges", [2, 3, 10]), ("mean", [4, 5, 6, 7, 8, 11])):
        table, loss = _fwd(c, c.dev(**{drop: False}))
        keep = [k for k in range(12) if k not in cols]
        assert not table[:, cols].any() and torch.equal(_bits(table[:, keep]), _bits(full[:, keep])), drop
        g = _bwd(c, c.dev(**{drop: False}), table, SCALE)
        w = SCALE.copy()
        w[{"boundary": 0, "edges": 1, "mean": 2}[drop]] = 0.0
        assert torch.equal(_bits(g), _bits(_bwd(c, c.dev(), full, w))), drop


def test_each_graph_alone_gets_its_batch_row_bitwise(cases):
    from pdg.plan import GraphPlan
    c = cases["tri"]
    full, floss = _fwd(c, c.dev())
    for g in range(c.B):
        n0, n1 = int(c.ptr[g]), int(c.ptr[g + 1])
        s = c.samples[g]
        plan = GraphPlan(torch.from_numpy(s.edge_index).cuda(), n1 - n0)
        plan.validate()
        ptr = torch.tensor([0, n1 - n0], dtype=torch.int32, device="cuda")
        cut = lambda t: t[n0:n1].contiguous()
        groups = [cut(c.d_bvec), cut(c.d_blen), cut(c.d_labels), plan.rowptr_dst, plan.src, plan.perm,
                  torch.from_numpy(s.edge_attr).cuda(), cut(c.d_area), c.d_cell[g:g + 1].contiguous(),
                  c.d_target[g:g + 1].contiguous()]
        alone, aloss = _fwd(c, groups, y=cut(c.d_y), ptr=ptr)
        assert torch.equal(_bits(alone[0]), _bits(full[g])) and torch.equal(_bits(aloss[0]), _bits(floss[g])), g


def _check_grad(got, want, mag, what):
    assert np.isfinite(want).all() and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - want)
    bound = 2.0 ** -23 * mag
    print(f"{what}: max err / bound {np.max(err[bound > 0] / bound[bound > 0]):.3e}, "
          f"non-zero rows {int(np.any(want != 0, 1).sum())} of {len(want)}")
    assert np.all(err <= bound)
    assert not got[mag == 0].any()          # exact zeros where no term applies


@pytest.mark.parametrize("name", ["tri", "quad"])
@pytest.mark.parametrize("accumulate", [False, True])
def test_gradient_against_the_restatement(cases, name, accumulate):
    c = cases[name]
    table, _ = _fwd(c, c.dev())
    old = np.random.default_rng(3).normal(0.0, 1e-3, (c.N, 3)).astype(np.float32)
    got = _bwd(c, c.dev(), table, SCALE, accumulate, torch.from_numpy(old).cuda() if accumulate else None)
    want, mag = R.backward(c.ptr, c.y, c.affine, table.cpu().numpy(), SCALE, **c.groups())
    assert np.any(want != 0)
    if accumulate:
        # rows without a term keep the old value exactly: (float)((double)old + 0)
        none = mag == 0
        assert np.array_equal(got.cpu().numpy()[none], old[none])
        want, mag = want + old.astype(np.float64), mag + np.abs(old.astype(np.float64))
        _check_grad(got.cpu().numpy(), want, mag, f"{name} accumulate")
    else:
        _check_grad(got.cpu().numpy(), want, mag, name)
    # one term at a time: the rows of the others are exact zeros
    if name == "tri" and not accumulate:
        n = c.ptr
        t = _bwd(c, c.dev(), table, [1.0, 0.0, 0.0]).cpu().numpy()
        p = _bwd(c, c.dev(), table, [0.0, 1.0, 0.0]).cpu().numpy()
        m = _bwd(c, c.dev(), table, [0.0, 0.0, 1.0]).cpu().numpy()
        assert not t[c.labels != -1].any() and not t[n[2]:n[3]].any() and t[n[0]:n[1]].any() and t[n[3]:].any()
        assert not p[n[1]:n[2]].any() and p[n[0]:n[1]].any() and p[n[2]:n[3]].any()
        inner = np.ones(c.N, bool)
        inner[c.ei[1][c.ea == 0]] = False
        assert not p[inner].any()
        assert m.all()          # every node of these meshes has an area
    again = _bwd(c, c.dev(), table, SCALE, accumulate, torch.from_numpy(old).cuda() if accumulate else None)
    assert torch.equal(_bits(again), _bits(got))


def test_zero_weights_give_exact_zeros_whatever_the_inputs_hold(cases):
    c = cases["tri"]
    n0 = int(c.ptr[0])
    hole = n0 + int(np.flatnonzero(c.labels[:c.ptr[1]] == -1)[2])
    seam = int(c.ei[1][c.ea == 0][0])
    clean, _ = _fwd(c, c.dev())
    for k, node in ((0, hole), (1, seam), (2, 5)):
        y = c.d_y.clone()
        y[node, 2] = float("nan")            # sxy enters both components of the force
        table, loss = _fwd(c, c.dev(), y=y)
        assert torch.isnan(loss[0, k]) and torch.isnan(table[0, 9 + k])      # a participating NaN is not hidden
        for g in (1, 2, 3):
            assert torch.equal(_bits(table[g]), _bits(clean[g]))
        assert not _bwd(c, c.dev(), table, np.zeros(3, np.float32), y=y).any()
    # a NaN that only one term reads, that term's weight 0 and the others on: bitwise the clean gradient
    bvec, target = c.d_bvec.clone(), c.d_target.clone()
    bvec[hole] = float("nan")
    target[0] = float("nan")
    y = c.d_y.clone()
    y[seam, 2] = float("nan")     # a node of the cell's edge: no traction term reads it
    assert c.labels[seam] == 1
    for w, kw in (([0.0, SCALE[1], SCALE[2]], dict(groups=c.dev(bvec=bvec))),
                  ([SCALE[0], SCALE[1], 0.0], dict(groups=c.dev(target=target))),
                  ([SCALE[0], 0.0, 0.0], dict(groups=c.dev(), y=y))):
        table, loss = _fwd(c, kw["groups"], y=kw.get("y"))
        assert torch.isnan(loss[0]).any()
        out = _bwd(c, kw["groups"], table, w, y=kw.get("y"))
        assert torch.equal(_bits(out), _bits(_bwd(c, c.dev(), clean, w))), w
    # a NaN table entry under a zero weight
    broken = clean.clone()
    broken[:, [1, 2, 5, 6, 7]] = float("nan")
    assert not _bwd(c, c.dev(), broken, np.zeros(3, np.float32)).any()
    old = torch.full_like(c.d_y, 0.25)
    assert torch.equal(_bwd(c, c.dev(), broken, np.zeros(3, np.float32), True, old), old)


def test_absent_denominators_follow_the_training_rule(cases):
    """No participating area, or a cell area that is not > 0: the mean term is absent for that graph, not NaN."""
    c = cases["tri"]
    area = c.area.copy()
    area[c.ptr[0]:c.ptr[1]] = 0.0
    area[c.ptr[1] + 3] = np.nan           # one excluded row in a graph that keeps its term
    cell = c.cell.copy()
    cell[2] = 0.0
    groups = c.dev(area=torch.from_numpy(area).cuda(), denom=torch.from_numpy(cell).cuda())
    table, loss = _fwd(c, groups)
    want, _ = R.forward(c.ptr, c.y, c.affine, boundary=(c.bvec, c.blen, c.labels), edges=(c.ei, c.ea),
                        mean=(area, c.target, cell))
    _check_table(table.cpu().numpy(), loss.cpu().numpy(), want, "absent mean terms")
    assert loss[0, 2] == 0 and loss[2, 2] == 0 and loss[1, 2] > 0 and loss[3, 2] > 0
    g = _bwd(c, groups, table, [0.0, 0.0, 1.0]).cpu().numpy()
    n = c.ptr
    assert not g[n[0]:n[1]].any() and not g[n[2]:n[3]].any() and not g[n[1] + 3].any()
    assert np.isfinite(g).all() and g[n[1]:n[2]].any() and g[n[3]:].any()


def test_reduce_against_the_restatement(cases):
    from pdg.lib import lib, stream_handle
    c = cases["tri"]
    _, loss = _fwd(c, c.dev())
    rng = np.random.default_rng(2)
    ln, ld = rng.uniform(0.1, 1.0, c.B).astype(np.float32), rng.uniform(0.1, 1.0, c.B).astype(np.float32)
    d = lambda a: torch.from_numpy(a).cuda()
    d_ln, d_ld, flag = d(ln), d(ld), torch.ones(1, device="cuda")

    def run(ldiv, scale):
        out7 = torch.full((7,), -7.0, device="cuda")
        lib.pdg_loss_reduce_phys(c.B, d_ln.data_ptr(), ldiv.data_ptr() if ldiv is not None else None, loss.data_ptr(),
                                 0.25, 2.5, d(np.asarray(scale, np.float32)).data_ptr(), flag.data_ptr(),
                                 out7.data_ptr(), stream_handle(out7.device))
        out4 = torch.full((4,), -7.0, device="cuda")
        lib.pdg_loss_reduce(c.B, d_ln.data_ptr(), ldiv.data_ptr() if ldiv is not None else None, 0.25, 2.5,
                            flag.data_ptr(), out4.data_ptr(), stream_handle(out7.device))
        return out7.cpu().numpy(), out4.cpu().numpy()

    for ldiv, hd in ((d_ld, ld), (None, None)):
        # all weights 0: the step's own four values bitwise, then exact zeros
        out7, out4 = run(ldiv, [0.0, 0.0, 0.0])
        assert np.array_equal(out7[:4].view(np.int32), out4.view(np.int32)) and not out7[4:].any()
        out7, out4 = run(ldiv, SCALE)
        want = R.reduce(ln, hd, loss.cpu().numpy(), 0.25, 2.5, SCALE)
        assert np.array_equal(out7[:3].view(np.int32), out4[:3].view(np.int32))
        # each term: an fp64 sum rounded to fp32 and one fp32 product; the total: four more fp32 additions
        assert np.all(np.abs(out7[4:].astype(np.float64) - want[4:]) <= 2.0 ** -23 * np.abs(want[4:]))
        assert abs(float(out7[3]) - float(want[3])) <= 4 * 2.0 ** -23 * float(want[3])
        assert out7[3] > out4[3]


def test_the_pair_replays_from_a_captured_graph(cases):
    from pdg.lib import lib, ptr as p_, stream_handle
    c = cases["tri"]
    eager_t, eager_l = _fwd(c, c.dev())
    old = torch.full_like(c.d_y, 0.125)
    eager_g = _bwd(c, c.dev(), eager_t, SCALE, True, old)
    table = torch.full((c.B, 12), -7.0, dtype=torch.float64, device="cuda")
    loss = torch.full((c.B, 3), -7.0, dtype=torch.float32, device="cuda")
    gy = torch.empty_like(c.d_y)
    sc = torch.from_numpy(SCALE).cuda()
    common = [c.d_y.data_ptr(), c.d_affine.data_ptr()] + [p_(g) for g in c.dev()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = stream_handle(gy.device)
        gy.copy_(old)
        lib.pdg_phys_loss_fwd(c.B, c.d_ptr.data_ptr(), *common, table.data_ptr(), loss.data_ptr(), s)
        lib.pdg_phys_loss_bwd(c.B, c.d_ptr.data_ptr(), c.N, *common, table.data_ptr(), sc.data_ptr(), 1,
                              gy.data_ptr(), s)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(table), _bits(eager_t)) and torch.equal(_bits(loss), _bits(eager_l))
        assert torch.equal(_bits(gy), _bits(eager_g))
