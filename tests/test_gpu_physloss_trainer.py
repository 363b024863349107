"""Trainer(physics=PhysicsPenalty(...)): the boundary and mean-consistency penalties in the training step.

1. all weights 0: parameters and nmse / div / total bitwise those of physics=None;
2. non-zero weights: the parameter gradient against autograd on the fp64 oracle, the three terms written in torch
   below on the oracle's standardised output.  The bound is measured in the same test, not fixed: the discrepancy of
   the divergence-only step against the same oracle on the same batch, times two (the new terms add fp64-formed
   cotangents to the same fp32 backward, so nothing should grow by more).  With PDG_PHYSLOSS_ERRORS=<file> both
   figures are written there (profiles/physloss_errors.txt);
3. capture=True replays the eager step bitwise;
4. twenty steps with only the traction weight on one hole plate lower the reported traction term (first value
   against last: a trend, not a rate);
5. two ranks, equal shards, dp_mode="sync", in the pattern of tests/test_gpu_dist.py: the one-device step within
   that file's tolerances, the seven tail values the global minibatch's;
6. a batch without the mesh fields is refused.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import physloss_ref as R

pytestmark = pytest.mark.gpu

STEPS_MP = 3
WEIGHTS = dict(traction=0.5, periodic=2.0, mean=1.0)
STATS = {"mean_pos": 50.0, "std_pos": 29.0, "mean_mean_stress": 0.0, "std_mean_stress": 60.0,
         "mean_local_stress": 7.5, "std_local_stress": 60.0, "mean_edge_weight": 9.0, "std_edge_weight": 4.0}


def _datas(samples, fields=True):
    from pdg import devgraph, graph
    out = []
    for s in samples:
        d = graph.sample_to_data(s)
        d.face = torch.from_numpy(np.ascontiguousarray(s.faces.T))
        if fields:
            devgraph.attach_mesh_fields(d, "cuda")
        out.append(d)
    return out


def _batch(samples, fields=True):
    from pdg.graph import Batch
    return Batch.from_data_list(_datas(samples, fields)).to("cuda")


def _model():
    from gnn_local_stress.models import EncodeProcessDecode
    torch.manual_seed(69)
    return EncodeProcessDecode(input_edges_features_size=1, message_passing_steps=STEPS_MP, latent_size=128,
                               input_nodes_features_size=6, output_nodes_features_size=3,
                               **{k: torch.tensor(v) for k, v in STATS.items()}).to("cuda")


def _trainer(physics, divergence=True, **kw):
    from pdg.trainer import Trainer
    return Trainer(_model(), lr=1e-3, divergence=divergence, divergence_penalty=10.0, physics=physics, **kw)


@pytest.fixture(scope="module")
def plates():
    return R.cases()[0][:3]      # periodic with a hole; not periodic; no hole


def test_zero_weights_are_the_step_without_physics(plates):
    from pdg.trainer import PhysicsPenalty
    b = _batch(plates)
    runs = []
    for physics in (None, PhysicsPenalty()):
        tr = _trainer(physics)
        outs = []
        for _ in range(3):
            o = tr.step(b)
            outs.append([o[k].clone() for k in ("nmse", "div", "total")])
        if physics is not None:
            assert all(float(o[k]) == 0.0 for k in ("traction", "periodic", "mean"))
        torch.cuda.synchronize()
        runs.append((outs, tr.flat_p.clone(), tr.flat_g.clone()))
    (o0, p0, g0), (o1, p1, g1) = runs
    for a, c in zip(o0, o1):
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, c))
    assert torch.equal(g0, g1) and torch.equal(p0, p1)


def _physics_torch(pred, b, weights, convention="cell"):
    """The three per-batch terms (each already weight / B times its sum over the graphs) in torch on the
    standardised field `pred`, in its dtype, with the training rule: a graph without a term adds nothing."""
    dt = pred.dtype
    std, mean = torch.tensor(STATS["std_local_stress"], dtype=dt), torch.tensor(STATS["mean_local_stress"], dtype=dt)
    z = pred + mean / std
    ptr = b.ptr.tolist()
    B = len(ptr) - 1
    labels = b.nodes_types.reshape(-1).cpu()
    bvec, blen, area = b.boundary_vec.cpu().to(dt), b.boundary_len.cpu().to(dt), b.node_area.cpu().to(dt)
    cell = b.cell_area.cpu().to(dt)
    src, dst = b.edge_index.cpu()
    seam = b.edge_attr.reshape(-1).cpu() == 0
    terms = [pred.new_zeros(()), pred.new_zeros(()), pred.new_zeros(())]
    for g in range(B):
        n0, n1 = ptr[g], ptr[g + 1]
        rows = torch.arange(n0, n1)
        hole = rows[(labels[rows] == -1) & (blen[rows] > 0)]
        if len(hole):
            fx = z[hole, 0] * bvec[hole, 0] + z[hole, 2] * bvec[hole, 1]
            fy = z[hole, 2] * bvec[hole, 0] + z[hole, 1] * bvec[hole, 1]
            terms[0] = terms[0] + ((fx * fx + fy * fy) / blen[hole]).sum() / blen[hole].sum()
        e = seam & (dst >= n0) & (dst < n1)
        if int(e.sum()):
            d = z[dst[e]] - z[src[e]]
            terms[1] = terms[1] + (0.5 * (d * d).sum()) / (0.5 * int(e.sum()))
        w = area[rows]
        W = w.sum()
        D = cell[g] if convention == "cell" else W
        if float(W) > 0 and float(D) > 0:
            S = (w[:, None] * z[rows]).sum(0)
            target = b.mean_stress[n0].cpu().to(dt) / std
            terms[2] = terms[2] + ((S / D - target) ** 2).sum()
    return [t * (weights[k] / B) for t, k in zip(terms, ("traction", "periodic", "mean"))]


def _oracle(P0, b, weights):
    """(flat fp64 gradient of the divergence-only loss, of the loss with the physics terms, the losses)."""
    from oracle import epd_oracle as O
    from pdg.engine import PARAM_NAMES
    P = {k: v.detach().cpu().double().requires_grad_(True) for k, v in P0.items()}
    st = {k: torch.tensor(v, dtype=torch.float64) for k, v in STATS.items()}
    c = b.to("cpu")
    pred = O.epd_forward(P, st, c.pos.double(), c.mean_stress.double(), c.nodes_types, c.edge_index,
                         c.edge_attr.double(), STEPS_MP, scale_output=False)
    gt = (c.local_stress.double() - st["mean_local_stress"]) / st["std_local_stress"]
    total, nmse, div = O.batch_loss(pred, gt, c.ptr, [d.op_div_matrix.double() for d in c._data_list], c.nodes_types,
                                    True, 10.0)
    terms = _physics_torch(pred, c, weights)
    full = total + terms[0] + terms[1] + terms[2]
    names = list(PARAM_NAMES)
    g_div = torch.autograd.grad(total, [P[n] for n in names], retain_graph=True)
    g_all = torch.autograd.grad(full, [P[n] for n in names])
    flat = lambda gs: torch.cat([g.reshape(-1) for g in gs])
    return flat(g_div), flat(g_all), [float(v) for v in (nmse, div, *terms, full)]


def test_gradient_against_autograd_on_the_fp64_oracle(plates):
    from gpu_common import rel
    from pdg.trainer import PhysicsPenalty
    b = _batch(plates)
    tr0 = _trainer(None)
    P0 = {k: v.detach().clone() for k, v in tr0.model.state_dict().items()}
    tr0.step(b)
    g0 = tr0.flat_g.detach().double().cpu()
    tr1 = _trainer(PhysicsPenalty(**WEIGHTS))
    out = tr1.step(b)
    g1 = tr1.flat_g.detach().double().cpu()
    ref_div, ref_all, losses = _oracle(P0, b, WEIGHTS)
    e_div, e_all = rel(g0, ref_div), rel(g1, ref_all)
    grew = float((ref_all - ref_div).norm() / ref_div.norm())
    got = [float(out[k]) for k in ("nmse", "div", "traction", "periodic", "mean", "total")]
    line = (f"divergence-only step against the fp64 oracle: {e_div:.3e}; with the physics terms {WEIGHTS}: {e_all:.3e} "
            f"(bound 2 x {e_div:.3e}); the terms move the gradient by {grew:.3e} of its norm; losses {got} "
            f"against {losses}")
    print(line)
    path = os.environ.get("PDG_PHYSLOSS_ERRORS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")
    assert grew > 1e-2                       # the terms matter to this gradient
    # nmse and div: the 1e-5 the existing step tests hold the losses to.  The three terms are quadratic forms of an
    # fp32 forward that is itself within 1e-5 of fp64, with cancellation in the jump's differences and in the
    # defect S / D - target; the kernels' own arithmetic is held to 1e-10 at the op level, so this comparison only
    # has to catch a wrong weight, normaliser or input: 1e-3
    tols = [1e-5 * abs(losses[0]), 1e-5 * abs(losses[1])] + [1e-3 * abs(w) for w in losses[2:5]]
    tols.append(sum(tols))
    for a, w, t in zip(got, losses, tols):
        assert abs(a - w) <= t, (got, losses)
    assert all(g > 0 for g in got[2:5])
    assert e_all <= 2 * e_div, (e_all, e_div)


def test_capture_replays_the_eager_step_bitwise(plates):
    from pdg.trainer import PhysicsPenalty
    b1, b2 = _batch(plates), _batch(plates[:2])
    runs = []
    for capture in (False, True):
        tr = _trainer(PhysicsPenalty(**WEIGHTS), capture=capture)
        vals = []
        for b in (b1, b1, b2, b2, b1):
            o = tr.step(b)
            vals.append([float(o[k]) for k in ("total", "traction", "periodic", "mean")])
        torch.cuda.synchronize()
        runs.append((vals, tr.flat_p.clone(), tr.flat_g.clone()))
    (v0, p0, g0), (v1, p1, g1) = runs
    assert v0 == v1 and torch.equal(g0, g1) and torch.equal(p0, p1)
    assert len({v[0] for v in v0}) > 1


def test_traction_weight_lowers_the_traction_term(plates):
    from pdg.trainer import PhysicsPenalty
    b = _batch(plates[:1])
    tr = _trainer(PhysicsPenalty(traction=10.0), divergence=False)
    vals = []
    for _ in range(20):
        o = tr.step(b)
        vals.append(o["traction"].clone())
        assert float(o["periodic"]) == 0.0 and float(o["mean"]) == 0.0
    vals = [float(v) for v in vals]
    print("traction term over twenty steps:", [f"{v:.4e}" for v in vals])
    assert vals[0] > 0 and vals[-1] < vals[0]


def test_a_batch_without_the_mesh_fields_is_refused(plates):
    from pdg.trainer import PhysicsPenalty
    bare = _batch(plates, fields=False)
    tr = _trainer(PhysicsPenalty(**WEIGHTS))
    with pytest.raises(ValueError, match="mesh_fields=True"):
        tr.step(bare)
    with pytest.raises(TypeError, match="PhysicsPenalty"):
        _trainer({"traction": 1.0})
    # the material convention needs no cell area
    b = _batch(plates)
    del b.cell_area
    with pytest.raises(ValueError, match="cell_area"):
        tr.step(b)
    out = _trainer(PhysicsPenalty(mean=1.0, convention="material")).step(b)
    assert float(out["mean"]) > 0


def test_batch_loss_returns_the_three_terms_and_their_gradient(plates):
    from gnn_local_stress import losses
    from gpu_common import rel
    from pdg.trainer import PhysicsPenalty
    b = _batch(plates)
    phys = PhysicsPenalty(**WEIGHTS)
    tr = _trainer(phys)
    out = tr.step(b)
    model = _model()
    pred = model(b, scale_output=False).local_stress
    gt = (b.local_stress - model.mean_local_stress) / model.std_local_stress
    plain = losses.batch_loss(pred, b, gt, divergence=True, divergence_penalty=10.0)
    assert len(plain) == 3
    total, nmse, div, t, p, m = losses.batch_loss(pred, b, gt, divergence=True, divergence_penalty=10.0, physics=phys,
                                                  mean_local_stress=model.mean_local_stress,
                                                  std_local_stress=model.std_local_stress)
    assert torch.equal(nmse, plain[1]) and torch.equal(div, plain[2])
    for a, k in ((t, "traction"), (p, "periodic"), (m, "mean"), (total, "total")):
        assert abs(float(a) - float(out[k])) <= 4 * 2.0 ** -23 * abs(float(out[k])), k    # a few fp32 roundings apart
    model.zero_grad()
    total.backward()
    for name, prm in model.named_parameters():
        # two routes through the same fp32 backward: the bound tests/test_gpu_dist.py holds such pairs to
        assert rel(prm.grad, tr.G[name]) < 1e-4, name
    with pytest.raises(ValueError, match="mean_local_stress"):
        losses.batch_loss(pred, b, gt, physics=phys)
    with pytest.raises(ValueError, match="mesh_fields=True"):
        losses.batch_loss(pred, _batch(plates, fields=False), gt, physics=phys, mean_local_stress=0.0,
                          std_local_stress=1.0)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    sys.path[:0] = [str(root), str(root / "p-div-gnn_amd"), str(root / "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    torch.cuda.set_device(torch.device("cuda:0"))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pdg import meshgen
        from pdg.trainer import PhysicsPenalty
        samples = [meshgen.hole_plate(9, hole_radius=0.2, seed=11 + i) for i in range(4)]
        shards = [[0, 1], [2, 3]]
        tr = _trainer(PhysicsPenalty(**WEIGHTS), process_group=dist.group.WORLD, dp_mode="sync")
        out = tr.step(_batch([samples[i] for i in shards[rank]]), n_global_graphs=4)
        torch.cuda.synchronize()
        g = tr.flat_g.detach().double().cpu()
        tail = tr._bucket[-7:].detach().double().cpu()
        vals = [float(out[k]) for k in ("nmse", "div", "total", "traction", "periodic", "mean")]
        if rank == 0:
            one = _trainer(PhysicsPenalty(**WEIGHTS))
            ref = one.step(_batch(samples))
            torch.cuda.synchronize()
            rg = one.flat_g.detach().double().cpu()
            rv = [float(ref[k]) for k in ("nmse", "div", "total", "traction", "periodic", "mean")]
            q.put((float((g - rg).norm() / rg.norm()), vals, rv, tail.tolist()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_in_sync_mode_are_the_one_device_step():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    gerr, vals, ref, tail = q.get(timeout=400)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    print(f"two ranks against one device: gradient {gerr:.3e}; losses {vals} against {ref}; tail {tail}")
    assert gerr < 1e-4, gerr                      # tests/test_gpu_dist.py's tolerances
    for a, w in zip(vals, ref):
        assert abs(a - w) <= 1e-5 * abs(w), (vals, ref)
    # the bucket's tail is seven wide: the flag summed over the ranks, then the global minibatch's six values
    assert len(tail) == 7 and tail[0] == 2.0
    assert tail[1:] == pytest.approx([vals[0], vals[1], vals[2], vals[3], vals[4], vals[5]], rel=0, abs=0)
    assert all(v > 0 for v in vals)
