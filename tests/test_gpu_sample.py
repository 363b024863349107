"""The sampling kernels (csrc/pdg_sample.hip) at the op level against the host restatement (tests/sample_ref.py).

Bounds, with u = 2^-53, d the cell's diameter (its longest vertex distance) and every fp32 difference of two fp32
coordinates exact in fp64:

* weights, triangles: |w - w_exact| <= 2^-24 + 32 u d^2 / |A|, A the cell's area: the fp64 error of two 2 x 2
  determinants of fp32 differences (each product <= d^2, a handful of roundings each, divided by det = 2 A) plus
  the one fp32 rounding of a number in [0, 1].
* weights, quads: the kernel solves F(t) = k2 t^2 + k1 t + k0 = 0 in closed form (pdg_sample.hip).  Write D = d^2
  and J for the smallest |det J| over the cell, which a bilinear map attains at a corner (det J is linear in
  (s, t)): J = min_k |(p_k+1 - p_k) x (p_k-1 - p_k)| <= D.  e, f, h are no longer than d and g = (a - b) + (c - d)
  no longer than 2 d (one rounding per component), so |k0| <= D, |k2| <= 2 D, |k1| <= 3 D and each, a sum of one or
  two differences of products, is off by at most 16 u D.  disc = k1^2 - 4 k0 k2 inherits 2 |k1| 16 u D + 4 (|k0| +
  |k2|) 16 u D = 288 u D^2 and adds three roundings of numbers <= 17 D^2: at most 2^9 u D^2.  sqrt(disc) = |det J|
  >= J at the solution, so r = sqrt(disc) is off by at most 2^8 u D^2 / J + u r.  The two branches are chosen so
  that numerator and denominator add numbers of one sign: t = -2 k0 / (k1 + sg r) has |denominator| >= r >= J,
  and t = (sg r - k1) / (2 k2) with |t| <= 1 + TOL has |2 k2| >= r >= J, either way
  |dt| <= (2^8 u D^2 / J + 2^6 u D) / J <= 2^9 u (D / J)^2.
  s = (h - f t) . v / v . v with v = e + g t; det J = v x (f + g s) and |f + g s| <= d give v . v >= J^2 / D.
  The numerator moves by at most (|f . v| + |(h - f t) . g|) |dt| <= 7 D |dt| and the denominator by 2 |v . g|
  |dt| <= 12 D |dt|, their own evaluation adds 2^4 u D each, so |ds| <= (19 D |dt| + 2^5 u D) D / J^2 <= 2^14 u
  (D / J)^4.  A weight is a product of two of s, 1 - s, t, 1 - t, all within [-TOL, 1 + TOL]:
  |w - w_exact| <= 2^-24 + 2^15 u (D / J)^4, the first term being the one fp32 rounding.  Every term is derived, so
  nothing is taken from a measurement; for orientation only, test_locate_and_sample[quad13-257-box] prints the
  largest D / J of the plate, the kernel's largest error over its bound, and the largest difference between the
  restatement's Newton run in fp64 and in longdouble (DESIGN.md quotes them).
* values, against the restatement fed the kernel's own cell and weights: |got - want| <= 2^-24 |want| + nv u sum
  |w f| (the products are exact in fp64, nv - 1 additions, one rounding to fp32).
* transpose: |got - want| <= 2^-24 |want| + m_n u sum |w g| per node, m_n the node's entry count.
"""
import numpy as np
import pytest
import torch

import sample_ref as R
from test_meshfields_host import renumbered

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
E32 = 2.0 ** -24


# ----------------------------------------------------------------------------------------------------- meshes
def _mesh(name):
    from pdg import meshgen
    if name == "sq_tri":
        return np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32), np.array([[0, 1, 2], [0, 2, 3]]), None
    if name == "sq_quad":
        return np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32), np.array([[0, 1, 2, 3]]), None
    hole = (50.0, 50.0, 12.0)                 # points this close to the centre are in the hole of radius 20
    if name == "plate9":
        s = meshgen.hole_plate(9)
        return s.pos, s.faces, None
    if name == "plate71":
        s = meshgen.hole_plate(71, 0.2)
        return s.pos, s.faces, hole
    if name == "quad13":
        s = meshgen.quad_hole_plate(13, 0.2)
        return s.pos, s.faces, hole
    s = meshgen.hole_plate(13, 0.2)
    pos, faces = s.pos, s.faces
    if name == "renum":
        pos, faces, _ = renumbered(pos, faces)
    elif name == "cw":
        faces = faces[:, ::-1].copy()
    elif name == "3d":
        pos = np.concatenate([pos, np.full((len(pos), 1), 3.5, np.float32)], 1)
    elif name == "degen":
        faces = np.concatenate([faces, [[faces[5, 0], faces[5, 0], faces[5, 1]]]], 0)
    else:
        assert name == "plate13", name
    return pos, faces, hole


def _queries(pos, faces, hole, nq, seed=5):
    """(queries (nq, 2) fp32, the cell of each centroid query or -1): centroids, nodes, midpoints of interior
    edges, points on the external boundary, points in the hole and points outside the box."""
    rng = np.random.default_rng(seed)
    p = pos[:, :2].astype(np.float64)
    ok = np.array([R.det_exact(p[f]) != 0 for f in faces])
    nv = faces.shape[1]
    sides = np.sort(np.concatenate([faces[ok][:, [j, (j + 1) % nv]] for j in range(nv)], 0), 1)
    ue, cnt = np.unique(sides, axis=0, return_counts=True)
    mids = p[ue[cnt == 2]].mean(1)
    x0, y0, x1, y1 = R.bbox_of(pos).astype(np.float64)
    bnd = p[ue[cnt == 1]]
    onbox = ((bnd[:, :, 0] == x0).all(1) | (bnd[:, :, 0] == x1).all(1) | (bnd[:, :, 1] == y0).all(1)
             | (bnd[:, :, 1] == y1).all(1))
    bnd = bnd[onbox].mean(1)
    lx, ly = x1 - x0, y1 - y0
    outside = np.stack([x0 + lx * rng.uniform(-0.4, 1.4, 64), y1 + ly * rng.uniform(0.01, 0.5, 64)], 1)
    outside[::2] = np.stack([x0 - lx * rng.uniform(0.01, 0.5, 32), y0 + ly * rng.uniform(-0.4, 1.4, 32)], 1)
    cid = np.nonzero(ok)[0]
    cent = p[faces[cid]].mean(1)
    if hole is not None:
        r, th = hole[2] * np.sqrt(rng.uniform(0, 1, 64)), rng.uniform(0, 2 * np.pi, 64)
        inhole = np.stack([hole[0] + r * np.cos(th), hole[1] + r * np.sin(th)], 1)
    else:
        inhole = outside[:0]
    share = {"cent": 0.3, "nodes": 0.2, "mids": 0.2, "bnd": 0.1, "hole": 0.1, "out": 0.1}
    sets = {"cent": cent, "nodes": p, "mids": mids, "bnd": bnd, "hole": inhole, "out": outside}
    q, which = [], []
    for k, frac in share.items():
        want = max(int(round(frac * nq)), 1) if nq > 1 else int(k == "cent")
        if len(sets[k]) == 0 or want == 0:
            continue
        pick = rng.integers(0, len(sets[k]), want)
        q.append(sets[k][pick])
        which.append(cid[pick] if k == "cent" else -np.ones(want, np.int64))
    q, which = np.concatenate(q), np.concatenate(which)
    while len(q) < nq:                                   # fill up with centroids
        pick = rng.integers(0, len(cent), nq - len(q))
        q, which = np.concatenate([q, cent[pick]]), np.concatenate([which, cid[pick]])
    return q[:nq].astype(np.float32), which[:nq]


def _wbound(pts):
    """The weights' bound of the module docstring for the cell with vertices ``pts`` (nv, 2) fp64."""
    d2 = max(float(((a - b) ** 2).sum()) for a in pts for b in pts)
    if len(pts) == 3:
        return E32 + 32 * U * d2 / (abs(float(R.det_exact(pts))) / 2)
    return E32 + 2.0 ** 15 * U * _d2_over_j(pts) ** 4


def _d2_over_j(pts):
    """D / J of the module docstring for a quad's vertices (4, 2) fp64."""
    d2 = max(float(((a - b) ** 2).sum()) for a in pts for b in pts)
    cross = lambda u, v: abs(float(u[0] * v[1] - u[1] * v[0]))   # noqa: E731
    return d2 / min(cross(pts[(k + 1) % 4] - pts[k], pts[k - 1] - pts[k]) for k in range(4))


_cache = {}


def _case(name, nq, periodic):
    """Everything a test needs of one (mesh, query set), computed once: device tensors, the restatement's answer."""
    key = (name, nq, periodic)
    if key not in _cache:
        pos, faces, hole = _mesh(name)
        q, which = _queries(pos, faces, hole, nq)
        if periodic:
            bb = R.bbox_of(pos).astype(np.float64)
            k = np.random.default_rng(9).integers(-2, 3, size=q.shape)
            q = (q.astype(np.float64) + k * np.array([bb[2] - bb[0], bb[3] - bb[1]])).astype(np.float32)
        cell, w = R.locate(pos, faces, q, periodic)
        qw = R.wrap(q, R.bbox_of(pos)) if periodic else q.astype(np.float64)
        _cache[key] = dict(pos=pos, faces=faces, q=q, qw=qw, which=which, cell=cell, w=w,
                           dpos=torch.from_numpy(pos).cuda(), dfaces=torch.from_numpy(faces).cuda(),
                           dq=torch.from_numpy(q).cuda())
    return _cache[key]


def _value_check(got, want, mag, nv, what):
    tol = E32 * np.abs(want) + nv * U * mag
    err = np.abs(got.astype(np.float64) - want)
    print(f"{what}: values max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(tol, 1e-300)):.3f}")
    assert (err <= tol).all(), what


CASES = [("sq_tri", 1, False), ("sq_tri", 257, False), ("sq_quad", 257, False), ("plate9", 257, False),
         ("plate13", 4096, False), ("plate13", 257, True), ("quad13", 257, False), ("quad13", 257, True),
         ("plate71", 4096, False), ("renum", 257, False), ("cw", 257, False), ("3d", 257, False),
         ("degen", 257, False)]


@pytest.mark.parametrize("name,nq,periodic", CASES, ids=[f"{n}-{q}-{'per' if p else 'box'}" for n, q, p in CASES])
def test_locate_and_sample(name, nq, periodic):
    from gnn_local_stress.sampling import PointLocator, sample_field
    c = _case(name, nq, periodic)
    pos, faces, nv = c["pos"], c["faces"], c["faces"].shape[1]
    p64 = pos[:, :2].astype(np.float64)
    loc = PointLocator(c["dpos"], c["dfaces"], periodic=periodic)
    assert loc.degenerate == (1 if name == "degen" else 0) and not loc.retried
    if name == "plate71":
        assert loc.gx * loc.gy > 1024                                    # the bins cross a scan block
    assert np.array_equal(loc.bbox.cpu().numpy(), R.bbox_of(pos))
    bp = loc.bin_ptr.cpu().numpy()
    assert bp[0] == 0 and (np.diff(bp) >= 0).all() and bp[-1] == loc.entries <= loc.capacity
    plan = loc.locate(c["dq"])
    cell, w = plan.cell.cpu().numpy(), plan.weights.cpu().numpy()
    assert plan.cell.dtype == torch.int32 and w.shape == (nq, nv)
    # the same points are inside; the centroids' cells are equal exactly
    assert np.array_equal(cell >= 0, c["cell"] >= 0)
    assert np.array_equal(plan.inside.cpu().numpy(), cell >= 0)
    assert int(plan.n_outside.item()) == int((cell < 0).sum())
    cent = c["which"] >= 0
    assert np.array_equal(cell[cent], c["which"][cent]) and np.array_equal(c["cell"][cent], c["which"][cent])
    assert (w[cell < 0] == 0).all() and (w >= 0).all()
    # the weights against the exact weights of the kernel's own cell
    worst = 0.0
    for i in np.nonzero(cell >= 0)[0]:
        cp = p64[faces[cell[i]]]
        exact = R.cell_weights(c["qw"][i], cp)
        assert exact is not None and all(x >= -R.TOL * 1.001 for x in exact), (i, cell[i])
        err = max(abs(float(max(x, 0)) - float(g)) for x, g in zip(exact, w[i]))
        worst = max(worst, err / _wbound(cp))
        assert err <= _wbound(cp), (i, cell[i], err, _wbound(cp))
    print(f"{name}-{nq}: weights max err / bound {worst:.3f}")
    if name == "quad13" and not periodic:
        dev64 = 0.0
        dj = max(_d2_over_j(p64[f]) for f in faces)
        print(f"quad13: largest d^2 / J {dj:.3f}")
        for i in np.nonzero(cell >= 0)[0][:64]:
            cp = p64[faces[cell[i]]]
            a, b = R.quad_weights(c["qw"][i], cp, np.float64), R.quad_weights(c["qw"][i], cp)
            dev64 = max(dev64, max(abs(float(x) - float(y)) for x, y in zip(a, b)))
        print(f"quad13: the restatement in fp64 against longdouble, largest weight difference {dev64:.3e}")
    # values: the restatement fed the kernel's own cell and weights, and the restatement's own answer
    ncol = {1: 1, 257: 3, 4096: 5}[nq]
    field = np.random.default_rng(3).normal(size=(len(pos), ncol)).astype(np.float32)
    got = sample_field(torch.from_numpy(field).cuda(), plan, fill=-3.0).cpu().numpy()
    assert got.shape == (nq, ncol) and (got[cell < 0] == -3.0).all()
    want = R.sample(field, faces, cell, w, fill=-3.0)
    _value_check(got, want, R.sample_abs(field, faces, cell, w), nv, f"{name}-{nq}")
    own = R.sample(field, faces, c["cell"], c["w"], fill=-3.0)
    for i in np.nonzero(cell >= 0)[0]:                                   # either neighbour: the value agrees
        nodes = np.union1d(faces[cell[i]], faces[c["cell"][i]])
        slack = (_wbound(p64[faces[cell[i]]]) + _wbound(p64[faces[c["cell"][i]]])) * np.abs(field[nodes]).sum(0)
        assert (np.abs(got[i] - own[i]) <= E32 * np.abs(own[i]) + slack).all(), (i, cell[i], c["cell"][i])
    flat = sample_field(torch.from_numpy(field[:, 0].copy()).cuda(), plan, fill=-3.0)
    assert flat.shape == (nq,) and np.array_equal(flat.cpu().numpy(), got[:, 0])
    nan = sample_field(torch.from_numpy(field).cuda(), plan)
    assert torch.isnan(nan[plan.cell < 0]).all() and not torch.isnan(nan[plan.cell >= 0]).any()


def test_node_offset_addresses_one_mesh_of_a_batched_field():
    from gnn_local_stress.sampling import PointLocator, sample_field, sample_field_grad
    a, b = _case("plate9", 257, False), _case("plate13", 257, True)
    na, nb = len(a["pos"]), len(b["pos"])
    rng = np.random.default_rng(4)
    field = torch.from_numpy(rng.normal(size=(na + nb, 3)).astype(np.float32)).cuda()
    plan = PointLocator(b["dpos"], b["dfaces"], periodic=True).locate(b["dq"])
    got = sample_field(field, plan, node_offset=na)
    assert torch.equal(got.isnan(), plan.cell[:, None].expand(-1, 3) < 0)
    assert torch.equal(got.nan_to_num(7.0), sample_field(field[na:].clone(), plan).nan_to_num(7.0))
    cell, w = plan.cell.cpu().numpy(), plan.weights.cpu().numpy()
    want = R.sample(field.cpu().numpy(), b["faces"], cell, w, fill=0.0, node_offset=na)
    _value_check(got.nan_to_num(0.0).cpu().numpy(), want,
                 R.sample_abs(field.cpu().numpy(), b["faces"], cell, w, node_offset=na), 3, "node_offset")
    g = torch.from_numpy(rng.normal(size=(257, 3)).astype(np.float32)).cuda()
    gt = sample_field_grad(g, plan, node_offset=na)
    assert gt.shape == (na + nb, 3) and (gt[:na] == 0).all() and torch.equal(gt[na:], sample_field_grad(g, plan))
    with pytest.raises(ValueError, match="no room"):
        sample_field(field, plan, node_offset=na + 1)
    with pytest.raises(ValueError, match="no room"):
        sample_field_grad(g, plan, n_nodes=nb, node_offset=1)


def test_bin_overflow_sets_the_flag_and_writes_nothing_past_capacity():
    from gnn_local_stress.sampling import PointLocator
    from pdg.lib import lib, stream_handle
    c = _case("plate13", 4096, False)
    loc = PointLocator(c["dpos"], c["dfaces"])
    total, cap = loc.entries, loc.entries - 1
    n, nf = len(c["pos"]), len(c["faces"])
    dev = c["dpos"].device
    nbytes = lib.pdg_cell_bins_scratch_bytes(loc.gx, loc.gy)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    cells = torch.full((cap + 1,), -77, dtype=torch.int32, device=dev)   # the last word is the guard
    bin_ptr = torch.empty(loc.gx * loc.gy + 1, dtype=torch.int32, device=dev)
    bbox = torch.empty(4, dtype=torch.float32, device=dev)
    info = torch.empty(4, dtype=torch.int32, device=dev)
    lib.pdg_cell_bins(n, c["dpos"].data_ptr(), 2, nf, 3, c["dfaces"].data_ptr(), loc.gx, loc.gy, bin_ptr.data_ptr(),
                      cells.data_ptr(), cap, bbox.data_ptr(), info.data_ptr(), scratch.data_ptr(), nbytes,
                      stream_handle(dev))
    assert info.tolist() == [total, 1, 0, 0]
    assert int(cells[cap]) == -77 and int((cells[:cap] == -77).sum()) == 0
    assert torch.equal(bin_ptr, loc.bin_ptr)
    # the exact capacity fits; the Python layer gets there by its one retry
    small = PointLocator(c["dpos"], c["dfaces"], capacity=cap)
    assert small.retried and small.capacity == total == small.entries
    p0, p1 = loc.locate(c["dq"]), small.locate(c["dq"])
    assert torch.equal(p0.cell, p1.cell) and torch.equal(p0.weights, p1.weights)
    assert torch.equal(torch.sort(loc.bin_cells[:total])[0], torch.sort(small.bin_cells[:total])[0])


@pytest.mark.parametrize("name", ["plate13", "quad13"])
def test_result_does_not_depend_on_the_order_inside_a_bin(name):
    """The same queries against the mesh with its faces reversed: the same values within the value bound, and the
    cell ids map through the reversal wherever the containing cell is unique (where the restatement's smallest weight
    is > 0: the point is strictly inside)."""
    from gnn_local_stress.sampling import PointLocator, sample_field
    c = _case(name, 257, False)
    nf, nv = len(c["faces"]), c["faces"].shape[1]
    rev = torch.from_numpy(c["faces"][::-1].copy()).cuda()
    p0 = PointLocator(c["dpos"], c["dfaces"]).locate(c["dq"])
    p1 = PointLocator(c["dpos"], rev).locate(c["dq"])
    unique = torch.tensor([cl >= 0 and min(w) > 0 for cl, w in zip(c["cell"], c["w"])]).cuda()
    assert int(unique.sum()) > 100
    assert torch.equal(p1.cell[unique], nf - 1 - p0.cell[unique]) and torch.equal(p0.cell < 0, p1.cell < 0)
    assert torch.equal(p0.weights[unique], p1.weights[unique])
    field = torch.from_numpy(np.random.default_rng(6).normal(size=(len(c["pos"]), 3)).astype(np.float32)).cuda()
    v0, v1 = sample_field(field, p0, fill=0.0).cpu().numpy(), sample_field(field, p1, fill=0.0).cpu().numpy()
    f = field.cpu().numpy()
    cell0, cell1 = p0.cell.cpu().numpy(), p1.cell.cpu().numpy()
    frev = c["faces"][::-1]
    p64 = c["pos"][:, :2].astype(np.float64)
    for i in np.nonzero(cell0 >= 0)[0]:
        a, b = c["faces"][cell0[i]], frev[cell1[i]]
        slack = (_wbound(p64[a]) + _wbound(p64[b])) * np.abs(f[np.union1d(a, b)]).sum(0)
        assert (np.abs(v0[i] - v1[i]) <= E32 * np.abs(v0[i]) + slack + nv * U * np.abs(f[a]).sum(0)).all(), i


@pytest.mark.parametrize("name,nq,periodic", [("plate13", 4096, False), ("quad13", 257, True)])
def test_transpose(name, nq, periodic):
    from gnn_local_stress.sampling import PointLocator, sample_field, sample_field_grad
    c = _case(name, nq, periodic)
    faces, nv, n = c["faces"], c["faces"].shape[1], len(c["pos"])
    plan = PointLocator(c["dpos"], c["dfaces"], periodic=periodic).locate(c["dq"])
    cell, w = plan.cell.cpu().numpy(), plan.weights.cpu().numpy()
    rowptr, entries = plan.csr()
    assert plan.csr()[0] is rowptr                                       # built once
    rp, en = R.csr(faces, cell, n)
    assert rowptr.dtype == torch.int32 and np.array_equal(rowptr.cpu().numpy(), rp)
    assert np.array_equal(entries.cpu().numpy()[:rp[-1]], en)
    rng = np.random.default_rng(8)
    ncol = 3 if nq == 4096 else 5
    g = rng.normal(size=(nq, ncol)).astype(np.float32)
    dg = torch.from_numpy(g).cuda()
    got = sample_field_grad(dg, plan)
    assert torch.equal(got, sample_field_grad(dg, plan))                 # bitwise from call to call
    want, mag, m = R.sample_T(g, faces, cell, w, n)
    tol = E32 * np.abs(want) + m[:, None] * U * mag
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    print(f"transpose {name}: max err {err.max():.3e}, longest row {m.max()}, untouched nodes {(m == 0).sum()}")
    assert (err <= tol).all()
    assert (got.cpu().numpy()[m == 0] == 0).all()
    # outside queries add nothing, whatever their cotangent holds
    g2 = g.copy()
    g2[cell < 0] = np.nan
    assert (cell < 0).any() and torch.equal(sample_field_grad(torch.from_numpy(g2).cuda(), plan), got)
    one = sample_field_grad(dg[:, 0].contiguous(), plan)
    assert one.shape == (n,) and torch.equal(one, sample_field_grad(dg[:, :1].contiguous(), plan)[:, 0])
    # adjointness: <S f, g> = <f, S^T g> within the sum of the two bounds
    f = rng.normal(size=(n, ncol)).astype(np.float32)
    sf = sample_field(torch.from_numpy(f).cuda(), plan, fill=0.0).cpu().numpy().astype(np.float64)
    lhs, rhs = float((sf * g).sum()), float((f.astype(np.float64) * got.cpu().numpy()).sum())
    sabs = R.sample_abs(f, faces, cell, w)
    bound = float(((E32 * np.abs(sf) + nv * U * sabs) * np.abs(g)).sum() + (tol * np.abs(f)).sum())
    print(f"adjoint {name}: <Sf, g> {lhs:.9e} <f, STg> {rhs:.9e} diff {abs(lhs - rhs):.2e} bound {bound:.2e}")
    assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("nq", [1024, 4096])
def test_heavy_row(nq):
    """Every query inside one cell of the 2-triangle square: rows of nq entries (the diagonal's two nodes hold them
    all), sorted by the workgroup in LDS (1,024) and in global memory (4,096 > the 2,048-slot tile)."""
    from gnn_local_stress.sampling import PointLocator, sample_field_grad
    c = _case("sq_tri", 1, False)
    rng = np.random.default_rng(12)
    a, b = rng.uniform(0.05, 0.45, nq), rng.uniform(0.05, 0.45, nq)
    q = np.stack([a + b + 0.05, b], 1).astype(np.float32)                # strictly inside (0,0) (1,0) (1,1)
    plan = PointLocator(c["dpos"], c["dfaces"]).locate(torch.from_numpy(q).cuda())
    cell, w = plan.cell.cpu().numpy(), plan.weights.cpu().numpy()
    assert (cell == 0).all()
    rowptr, entries = plan.csr()
    rp, en = R.csr(c["faces"], cell, 4)
    assert list(np.diff(rp)) == [nq, nq, nq, 0]
    assert np.array_equal(rowptr.cpu().numpy(), rp) and np.array_equal(entries.cpu().numpy(), en)
    g = rng.normal(size=(nq, 3)).astype(np.float32)
    got = sample_field_grad(torch.from_numpy(g).cuda(), plan)
    want, mag, m = R.sample_T(g, c["faces"], cell, w, 4)
    assert (np.abs(got.cpu().numpy() - want) <= E32 * np.abs(want) + m[:, None] * U * mag).all()
    assert (got[3] == 0).all()


def test_python_layer_refuses_what_it_cannot_do():
    from gnn_local_stress.sampling import PointLocator, sample_field, sample_field_grad
    c = _case("plate9", 257, False)
    with pytest.raises(RuntimeError, match="HIP"):
        PointLocator(c["dpos"].cpu(), c["dfaces"].cpu())
    with pytest.raises(ValueError, match="triangle"):
        PointLocator(c["dpos"], _case("sq_quad", 257, False)["dfaces"], cells="triangle")
    bad = c["dfaces"].clone()
    bad[3, 1] = len(c["pos"])
    with pytest.raises(ValueError, match="outside"):
        PointLocator(c["dpos"], bad)
    loc = PointLocator(c["dpos"], c["dfaces"])
    with pytest.raises(RuntimeError, match="HIP"):
        loc.locate(c["dq"].cpu())
    with pytest.raises(ValueError, match="query points"):
        loc.locate(c["dq"][:, :1])
    plan = loc.locate(c["dq"])
    f = torch.zeros(len(c["pos"]), 3, device="cuda", requires_grad=True)
    with pytest.raises(RuntimeError, match="no autograd route"):
        sample_field(f, plan)
    with torch.no_grad():
        assert sample_field(f, plan).shape == (257, 3)
    with pytest.raises(ValueError, match="rows"):
        sample_field_grad(torch.zeros(5, 3, device="cuda"), plan)
    empty = loc.locate(torch.zeros(0, 2, device="cuda"))
    assert sample_field(f.detach(), empty).shape == (0, 3)
    assert (sample_field_grad(torch.zeros(0, 3, device="cuda"), empty) == 0).all()
