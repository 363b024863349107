"""End-to-end parity of the HIP EncodeProcessDecode + losses (SURVEY §4 tiers T2):

* against the reference-generated golden fixtures (tests/golden, the reference's
  own models.py / gnn_train.py run under the PyG stand-in);
* against the CPU oracle (oracle/epd_oracle.py) at larger sizes, in fp32 and
  fp64, so the GPU error is judged against the fp32 noise floor of the
  reference's own CPU path.

Tolerance (north_star: "within 1e-5 rel fp32"): relative L2 error of the
output field and of the losses <= 1e-5.  Gradients against the oracle at larger
sizes: each parameter's gradient must be as close to the float64 restatement as
the reference's own fp32 CPU result is, within a factor 2, and never worse than
3e-5 relative L2.  Golden cases (a few hundred nodes, up to 10
tied steps): there a gradient's distance to fp64 is decided by which relu
pre-activations within rounding of zero flip (one flipped bit of 3.6e6 moves
node_encoder.0.weight's gradient by 7e-5 in the fp32 oracle on one host, 5e-6
with the GPU's association of the same sums: tools/grad_err_stages.py,
profiles/r05_grad_err_stages.txt), so the gradient is compared with fp64 IN THE
GPU FORWARD'S OWN RELU REGION, within GOLDEN_FACTOR = 2 of the fp32 oracle's
distance in its own region (floor MASKED_FLOOR), and every flipped bit must have
a pre-activation within FLIP_EPS of zero.  Two fp32 evaluations of the HIP path
with different kernel variants are compared at VARIANT_TOL = 1e-4: they may
differ in such a bit.  Every gradient comparison against fp64 is appended to
gpurun_out/parity.jsonl.
"""
import pytest
import torch

from golden_io import CASES
from gpu_common import capture_forward, dataset_stats, golden_batch, gpu_relu_masks, make_batch, mask_flips, rel

pytestmark = pytest.mark.gpu

OUT_TOL = 1e-5
GRAD_TOL = 3e-5
GOLDEN_FACTOR = 2.0
MASKED_FLOOR = 1e-6
FLIP_EPS = 1e-5
FLIP_MAX = 8
VARIANT_TOL = 1e-4


def _log_grads(case, model, g64, ref32, factor=2.0, floor=GRAD_TOL, extra=None):
    """Append every parameter's gradient error vs fp64 beside the fp32 reference's own to
    gpurun_out/parity.jsonl (the margins to the bound on record, not only "passed")."""
    import json
    import os
    from pathlib import Path
    errs = {n: (rel(p.grad, g64[n]), ref32[n]) for n, p in model.named_parameters()}
    worst = max(errs, key=lambda n: errs[n][0] / max(floor, factor * errs[n][1]))
    rec = {"case": case, "worst_grad": [worst, *errs[worst]],
           "worst_margin": errs[worst][0] / max(floor, factor * errs[worst][1]),
           "max_grad_err": max(e[0] for e in errs.values()),
           "grad_tol_rule": f"max({floor}, {factor:g} x fp32 vs fp64)", **(extra or {})}
    out = Path(os.environ.get("GRAFT_REPO_ROOT", Path(__file__).resolve().parents[1])) / "gpurun_out"
    try:
        out.mkdir(exist_ok=True)
        with open(out / "parity.jsonl", "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


def _model(steps, stats, params=None):
    from gnn_local_stress.models import EncodeProcessDecode
    torch.manual_seed(69)
    m = EncodeProcessDecode(input_edges_features_size=1, message_passing_steps=steps, latent_size=128,
                            input_nodes_features_size=6, output_nodes_features_size=3,
                            **{k: torch.as_tensor(v).float() for k, v in stats.items()})
    if params is not None:
        m.load_state_dict(params)
    return m.to("cuda")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


@pytest.mark.parametrize("case", CASES)
def test_forward_and_grads_match_golden(case):
    """Output and losses against the golden (the reference run on its fp32 CPU path) and fp64; every
    gradient against fp64 evaluated in the GPU forward's own relu region ("relu
    region"): within GOLDEN_FACTOR = 2 of the fp32 oracle's distance to fp64 in ITS own region.
    Every relu bit where the GPU's forward and fp64's differ must have a pre-activation within
    FLIP_EPS of zero (relative to the layer's rms), and there may be at most FLIP_MAX of them."""
    from gnn_local_stress import losses
    from oracle.epd_oracle import ReluRegion
    g, batch = golden_batch(case)
    steps = int(g["steps"])
    model = _model(steps, g["stats"], g["params"])
    with torch.no_grad():
        out = model(batch, scale_output=True).local_stress
    assert rel(out, g["out_scaled"]) < OUT_TOL, rel(out, g["out_scaled"])
    cap = capture_forward(model)
    pred = model(batch, scale_output=False).local_stress
    assert rel(pred.detach(), g["pred"]) < OUT_TOL
    gt = (batch.local_stress - model.mean_local_stress) / model.std_local_stress
    total, nmse, div = losses.batch_loss(pred, batch, gt, divergence=bool(g["divergence"]),
                                         divergence_penalty=float(g["penalty"]))
    assert abs(float(nmse) - float(g["loss_nmse"])) <= OUT_TOL * abs(float(g["loss_nmse"]))
    assert abs(float(total.detach()) - float(g["loss_total"])) <= OUT_TOL * abs(float(g["loss_total"]))
    model.zero_grad()
    total.backward()
    st = {k: float(v) for k, v in g["stats"].items()}
    a = (g["params"], st, batch, steps)
    kw = dict(divergence=bool(g["divergence"]), penalty=float(g["penalty"]))
    r64, r32 = ReluRegion(keep=True), ReluRegion(keep=True)
    _, _, g64 = _oracle_grads(*a, torch.float64, region=r64, **kw)
    _, _, g32 = _oracle_grads(*a, torch.float32, region=r32, **kw)
    gmask = gpu_relu_masks(cap["ctx"])
    # fp64 in the GPU's relu region, and in the fp32 oracle's (its noise floor without the flips)
    _, _, g64_gpu = _oracle_grads(*a, torch.float64, region=ReluRegion(masks=gmask), **kw)
    m32 = {k: v > 0 for k, v in r32.keep.items()}
    _, _, g64_32 = _oracle_grads(*a, torch.float64, region=ReluRegion(masks=m32), **kw)
    flips = mask_flips(gmask, r64.keep)
    n_relu = sum(v.numel() for v in gmask.values())
    ref32 = {n: rel(g32[n], g64_32[n]) for n in g64}
    _log_grads(f"golden:{case}", model, g64_gpu, ref32, GOLDEN_FACTOR, floor=MASKED_FLOOR,
               extra={"flips": flips, "n_relu": n_relu,
                      "unmasked": {n: [rel(p.grad, g64[n]), rel(g["grads"][n], g64[n]), rel(g32[n], g64[n])]
                                   for n, p in model.named_parameters()}})
    assert len(flips) <= FLIP_MAX and all(h <= FLIP_EPS * rms for _, _, h, rms in flips), flips
    for name, p in model.named_parameters():
        err = rel(p.grad, g64_gpu[name])
        assert err <= max(MASKED_FLOOR, GOLDEN_FACTOR * ref32[name]), (name, err, ref32[name])
        # the reference's own fp32 gradient: the two distances to fp64 bound it (a flipped bit's step
        # in either evaluation is the same exact-arithmetic jump as in fp64)
        d = rel(p.grad, g["grads"][name])
        assert d <= max(GRAD_TOL, 1.5 * (rel(p.grad, g64[name]) + rel(g["grads"][name], g64[name]))), (name, d)


def test_per_graph_losses_match_oracle():
    from gnn_local_stress import losses
    from oracle import epd_oracle as O
    g, batch = golden_batch("batch3_div")
    pred = torch.from_numpy(g["pred"]).cuda().requires_grad_(True)
    gt = torch.from_numpy(g["gt_std"]).cuda()
    ptr = g["ptr"]
    for i in range(len(ptr) - 1):
        s, t = int(ptr[i]), int(ptr[i + 1])
        p_cpu = pred.detach().cpu()[s:t].clone().requires_grad_(True)
        ref = O.normalized_mse_loss_single(gt.cpu()[s:t], p_cpu)
        got = losses.normalized_mse_loss_single(ground_truth_local_stress=gt[s:t], predicted_local_stress=pred[s:t])
        assert abs(float(got) - float(ref)) <= 1e-6 * abs(float(ref))
        types = batch.nodes_types[s:t]
        for strat in ("square", "abs"):
            ref_d = O.compute_divergence(p_cpu, g["op_divs"][i], types.cpu(), strat)
            got_d = losses.compute_divergence(pred[s:t], g["op_divs"][i].cuda(), types, reduce_strategy=strat)
            assert abs(float(got_d) - float(ref_d)) <= 1e-5 * abs(float(ref_d)), strat
            gref, = torch.autograd.grad(ref_d, p_cpu)
            ggot, = torch.autograd.grad(got_d, pred)
            assert rel(ggot[s:t], gref) < 1e-5
    with pytest.raises(AttributeError):
        losses.compute_divergence(pred[:5], g["op_divs"][0].cuda(), batch.nodes_types[:5], reduce_strategy="cube")


def _oracle_grads(model_params, stats, batch, steps, dtype, divergence, penalty, scale_output=False, region=None):
    from oracle import epd_oracle as O
    P = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in model_params.items()}
    st = {k: torch.as_tensor(v).cpu().to(dtype) for k, v in stats.items()}
    b = batch
    args = (b.pos.cpu().to(dtype), b.mean_stress.cpu().to(dtype), b.nodes_types.cpu(), b.edge_index.cpu(),
            b.edge_attr.cpu().to(dtype))
    pred = O.epd_forward(P, st, *args, steps, scale_output=scale_output, region=region)
    gt = (b.local_stress.cpu().to(dtype) - st["mean_local_stress"]) / st["std_local_stress"]
    if scale_output:    # loss on the unscaled field: exercises the d(unscale)/dy = std factor
        gt = b.local_stress.cpu().to(dtype)
    ops = [d.op_div_matrix.to(dtype) for d in b._data_list]
    total, nmse, div = O.batch_loss(pred, gt, b.ptr, ops, b.nodes_types.cpu(), divergence, penalty)
    total.backward()
    return pred.detach(), float(total), {k: v.grad for k, v in P.items()}


@pytest.mark.parametrize("nmesh,ngraph,steps,divergence,scale_output",
                         [(21, 2, 10, True, False), (31, 1, 4, False, False), (17, 3, 3, True, True)])
def test_training_step_matches_oracle_fp32_and_fp64(nmesh, ngraph, steps, divergence, scale_output):
    """(17, 3, 3, True, True): backward through the output unscaling (models.py:318-321,
    y * std_local_stress + mean_local_stress) with the loss on the physical field."""
    from gnn_local_stress import losses
    from pdg import meshgen
    samples = meshgen.make_dataset(ngraph, n=nmesh, hole_radius=(0.15, 0.3), seed=5)
    batch = make_batch(samples)
    stats = {k: float(v) for k, v in dataset_stats(batch).items()}
    model = _model(steps, stats)
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    pred = model(batch, scale_output=scale_output).local_stress
    gt = (batch.local_stress - model.mean_local_stress) / model.std_local_stress
    if scale_output:
        gt = batch.local_stress
    total, _, _ = losses.batch_loss(pred, batch, gt, divergence=divergence, divergence_penalty=10.0)
    model.zero_grad()
    total.backward()
    p32, t32, g32 = _oracle_grads(params, stats, batch, steps, torch.float32, divergence, 10.0, scale_output)
    p64, t64, g64 = _oracle_grads(params, stats, batch, steps, torch.float64, divergence, 10.0, scale_output)
    floor = rel(p32, p64)
    assert rel(pred.detach(), p32) < OUT_TOL, (rel(pred.detach(), p32), floor)
    assert rel(pred.detach(), p64) < OUT_TOL
    assert abs(float(total) - t64) <= OUT_TOL * abs(t64)
    _log_grads(f"oracle:{nmesh}x{ngraph}:s{steps}", model, g64, {n: rel(g32[n], g64[n]) for n in g64})
    for name, p in model.named_parameters():
        ref32 = rel(g32[name], g64[name])
        assert rel(p.grad, g64[name]) <= max(GRAD_TOL, 2 * ref32), (name, rel(p.grad, g64[name]), ref32)


@pytest.mark.parametrize("steps,fused,chunked", [(33, True, ("Wa", "Wb", "Wn1a", "Wn1b", "Wn2")),
                                                  (17, False, ("W2",))])
def test_more_than_32_segments_match_oracle(steps, fused, chunked):
    """The engine's chunked deferred weight-gradient path (more than PDG_MAX_SEGS = 32 segments per weight: 32-segment
    chunks, each reduced at once by pdg_wgrad_reduce before the next chunk overwrites the same slabs) on one 9 x 9
    hole plate.  steps = 33, fused edge backward: the Wa / Wb and node_net.0 pair passes and node_net.2 have 33
    segments each (a second chunk of one segment).  steps = 17, fused_edge_wgrad off: edge_net.2 has 17 message + 16
    edge-update segments.  The segment counts are read from the backward itself and the launches from the library
    hook, so the test cannot pass without taking the chunked path.  Every gradient against fp64 in the GPU forward's
    own relu region (a deep network cannot fail on a relu bit), within max(GRAD_TOL, GOLDEN_FACTOR x the fp32
    oracle's own distance to fp64 in its region): a lost or doubled chunk moves a gradient by percent."""
    from gnn_local_stress import losses
    from oracle.epd_oracle import ReluRegion
    from pdg import meshgen
    from pdg.lib import lib
    batch = make_batch([meshgen.hole_plate(9, seed=2)])
    stats = {k: float(v) for k, v in dataset_stats(batch).items()}
    model = _model(steps, stats)
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    eng = model._engine_for(batch.pos.device)
    eng.fused_edge_wgrad = fused
    seen, names = {}, []
    wgrads, epilogue = eng._bwd_wgrads, eng._bwd_epilogue

    def spy_wgrads(b):
        seen.update({k: len(v) for k, v in b.segs.items()})
        before, lib.hook = lib.hook, names.append
        try:
            return wgrads(b)
        finally:
            lib.hook = before

    def spy_epilogue(b):
        seen["reds"] = len(b.reds)
        return epilogue(b)

    eng._bwd_wgrads, eng._bwd_epilogue = spy_wgrads, spy_epilogue
    cap = capture_forward(model)
    pred = model(batch, scale_output=False).local_stress
    gt = (batch.local_stress - model.mean_local_stress) / model.std_local_stress
    total, _, _ = losses.batch_loss(pred, batch, gt, divergence=True, divergence_penalty=10.0)
    model.zero_grad()
    total.backward()
    torch.cuda.synchronize()
    # the chunked path ran: 33 segments for each weight named, two launches (32 + 1 segments) per pass, every chunk
    # reduced at once; every other weight in one chunk, its reduction left to the epilogue
    assert all(seen[k] == 33 for k in chunked), seen
    assert all(n <= 32 for k, n in seen.items() if k not in chunked and k != "reds"), seen
    pair_sets = 2 if "Wa" in chunked else 0
    single = len(chunked) - 2 * pair_sets
    assert names.count("pdg_wgrad_pairs") == 2 + pair_sets
    assert names.count("pdg_wgrad_segments") == 2 * single
    assert names.count("pdg_wgrad_reduce") == 4 * pair_sets + 2 * single
    a = (params, stats, batch, steps)
    kw = dict(divergence=True, penalty=10.0)
    r32 = ReluRegion(keep=True)
    _, _, g32 = _oracle_grads(*a, torch.float32, region=r32, **kw)
    _, _, g64_gpu = _oracle_grads(*a, torch.float64, region=ReluRegion(masks=gpu_relu_masks(cap["ctx"])), **kw)
    _, _, g64_32 = _oracle_grads(*a, torch.float64, region=ReluRegion(masks={k: v > 0 for k, v in r32.keep.items()}),
                                 **kw)
    ref32 = {n: rel(g32[n], g64_32[n]) for n in g64_gpu}
    _log_grads(f"chunked:9x1:s{steps}:fused{int(fused)}", model, g64_gpu, ref32, GOLDEN_FACTOR,
               extra={"segments": {k: v for k, v in seen.items() if k != "reds"}, "epilogue_reductions": seen["reds"],
                      "max_fp32_oracle_err": max(ref32.values())})
    for name, p in model.named_parameters():
        assert bool(p.grad.isfinite().all()) and bool(g32[name].isfinite().all()), name
        err = rel(p.grad, g64_gpu[name])
        print(f"CHUNKED s{steps} fused={int(fused)} {name}: {err:.3e} (fp32 oracle {ref32[name]:.3e})")
        assert err <= max(GRAD_TOL, GOLDEN_FACTOR * ref32[name]), (name, err, ref32[name])


def test_input_gradients_are_refused():
    """Gradients w.r.t. the mesh inputs are not produced by the HIP backward: asking for them
    raises instead of silently returning None."""
    from pdg import meshgen
    batch = make_batch([meshgen.hole_plate(9, seed=2)])
    model = _model(2, {k: float(v) for k, v in dataset_stats(batch).items()})
    batch.pos = batch.pos.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="pos"):
        model(batch)
    with torch.no_grad():                 # inference never needs them
        assert model(batch).local_stress.shape == (batch.num_nodes, 3)


def test_zero_mean_stress_guard_returns_zeros():
    from pdg import meshgen
    batch = make_batch([meshgen.hole_plate(9, seed=2)])
    batch.mean_stress = torch.zeros_like(batch.mean_stress)
    model = _model(2, {k: 1.0 for k in ("mean_pos", "std_pos", "mean_mean_stress", "std_mean_stress",
                                        "mean_local_stress", "std_local_stress", "mean_edge_weight",
                                        "std_edge_weight")})
    out = model(batch)
    assert out.local_stress.shape == batch.mean_stress.shape
    assert float(out.local_stress.abs().max()) == 0.0 and not out.local_stress.requires_grad


def test_isolated_node_and_ragged_batch():
    """A node with no incident edge (in-degree 0) and graphs of unequal sizes."""
    from pdg import graph, meshgen
    from oracle import epd_oracle as O
    s1 = meshgen.hole_plate(7, seed=4)
    s2 = meshgen.hole_plate(12, hole_radius=0.25, seed=6)
    d1 = graph.sample_to_data(s1)
    # append an isolated node to graph 1
    d1.pos = torch.cat([d1.pos, torch.tensor([[50.0, 50.0]])])
    d1.mean_stress = torch.cat([d1.mean_stress, d1.mean_stress[:1]])
    d1.local_stress = torch.cat([d1.local_stress, d1.local_stress[:1]])
    d1.nodes_types = torch.cat([d1.nodes_types, torch.zeros(1, 1, dtype=torch.int64)])
    d1.surfaces_nodes_for_div = d1.nodes_types
    b = graph.Batch.from_data_list([d1, graph.sample_to_data(s2)]).to("cuda")
    stats = {k: float(v) for k, v in dataset_stats(b).items()}
    model = _model(3, stats)
    with torch.no_grad():
        out = model(b, scale_output=True).local_stress
    P = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    st = {k: torch.tensor(v) for k, v in stats.items()}
    ref = O.epd_forward(P, st, b.pos.cpu(), b.mean_stress.cpu(), b.nodes_types.cpu(), b.edge_index.cpu(),
                        b.edge_attr.cpu(), 3, scale_output=True)
    assert rel(out, ref) < OUT_TOL


@pytest.mark.parametrize("nmesh,ngraph,steps", [(41, 3, 4), (9, 1, 3)])
def test_fused_edge_weight_gradients_match_separate_passes(nmesh, ngraph, steps):
    """pdg_edge_bwd_w2 + pdg_edge_gout_wc (weight gradients fused into the edge backward,
    slabs accumulated over the steps) against pdg_edge_bwd + pdg_wgrad_segments: every
    parameter gradient and the input-gradient chain agree to VARIANT_TOL.  The two variants also
    run different edge-encoder forwards (pdg_edge_enc_fwd's bf16x6 W2 product vs pdg_encoder_fwd's
    fp32 MFMAs, since the unfused backward needs the stored layer-1 output), so they are two fp32
    evaluations that may differ in a relu bit within rounding of zero: with the bf16x6 node encoder
    (round 5) one such bit moves node_encoder.0.weight's gradient by 1.8e-5 at (41, 3) (the golden and
    oracle gates against fp64 are unchanged).
    (41, 3): ~15k edges, several 32-row rounds per block and a ragged last round;
    (9, 1): fewer edges than blocks x 32 (empty blocks)."""
    from gnn_local_stress import losses
    from pdg import meshgen
    samples = meshgen.make_dataset(ngraph, n=nmesh, hole_radius=(0.15, 0.3), seed=7)
    batch = make_batch(samples)
    stats = {k: float(v) for k, v in dataset_stats(batch).items()}
    grads = {}
    for fused in (True, False):
        model = _model(steps, stats)
        model._engine_for(batch.pos.device).fused_edge_wgrad = fused
        pred = model(batch, scale_output=False).local_stress
        gt = (batch.local_stress - model.mean_local_stress) / model.std_local_stress
        total, _, _ = losses.batch_loss(pred, batch, gt, divergence=True, divergence_penalty=10.0)
        total.backward()
        grads[fused] = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    for name, g in grads[True].items():
        assert rel(g, grads[False][name]) < VARIANT_TOL, (name, rel(g, grads[False][name]))


@pytest.mark.parametrize("nmesh,ngraph,steps", [(41, 3, 4), (9, 1, 3)])
def test_gz1e_from_gc_matches_stored_gz1e(nmesh, ngraph, steps):
    """The shipped edge backward stores no gz1e: pdg_pq_scatter_bwd forms it per row as gC - gz1m.
    Against the form that stores gz1e, gP / gQ differ by one fp32 rounding of |gC| per row, so every
    parameter gradient agrees to 1e-6 (the loss and output bitwise: the forward is untouched)."""
    from gnn_local_stress import losses
    from pdg import meshgen
    samples = meshgen.make_dataset(ngraph, n=nmesh, hole_radius=(0.15, 0.3), seed=7)
    batch = make_batch(samples)
    stats = {k: float(v) for k, v in dataset_stats(batch).items()}
    grads, losses_ = {}, {}
    for e_sum in (True, False):
        model = _model(steps, stats)
        model._engine_for(batch.pos.device).gz1e_from_gc = e_sum
        pred = model(batch, scale_output=False).local_stress
        gt = (batch.local_stress - model.mean_local_stress) / model.std_local_stress
        total, _, _ = losses.batch_loss(pred, batch, gt, divergence=True, divergence_penalty=10.0)
        total.backward()
        losses_[e_sum] = float(total)
        grads[e_sum] = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    assert losses_[True] == losses_[False]
    for name, g in grads[True].items():
        assert rel(g, grads[False][name]) < 1e-6, (name, rel(g, grads[False][name]))


@pytest.mark.parametrize("nmesh,ngraph,steps", [(41, 3, 4), (9, 1, 3)])
def test_forward_variants_agree(nmesh, ngraph, steps):
    """The two edge-forward kernels of the engine: pdg_edge_fwd_coop (default: block-cooperative, C and W2
    in unbiased bf16x6) and pdg_edge_fwd (LDS weights, C in fp32 MFMAs).  Output (training and inference)
    agree to 1e-5 and every parameter gradient to VARIANT_TOL (two fp32 evaluations may differ in a relu
    mask bit whose pre-activation is within rounding of zero)."""
    from gnn_local_stress import losses
    from pdg import meshgen
    samples = meshgen.make_dataset(ngraph, n=nmesh, hole_radius=(0.15, 0.3), seed=7)
    batch = make_batch(samples)
    stats = {k: float(v) for k, v in dataset_stats(batch).items()}
    res = {}
    for coop in (True, False):
        model = _model(steps, stats)
        eng = model._engine_for(batch.pos.device)
        eng.coop_fwd = coop
        with torch.no_grad():
            y_inf = model(batch, scale_output=True).local_stress.clone()
        pred = model(batch, scale_output=False).local_stress
        gt = (batch.local_stress - model.mean_local_stress) / model.std_local_stress
        total, _, _ = losses.batch_loss(pred, batch, gt, divergence=True, divergence_penalty=10.0)
        total.backward()
        res[coop] = (y_inf, pred.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()})
    (y0, p0, g0), (y1, p1, g1) = res[False], res[True]
    assert rel(y1, y0) < 1e-5 and rel(p1, p0) < 1e-5
    for name, g in g1.items():
        assert rel(g, g0[name]) < VARIANT_TOL, (name, rel(g, g0[name]))


def test_edgeless_batch_matches_oracle():
    """A batch whose graphs have no edge at all (SURVEY §4 T1 'E=0 graphs'): as in the reference,
    every message aggregate is zero and the edge parameters get zero gradients; output and every
    parameter gradient match the fp64 oracle (the oracle runs the reference's ops on empty
    tensors), with the divergence loss on."""
    from gnn_local_stress import losses
    from pdg import graph, meshgen
    datas = []
    for s in meshgen.make_dataset(2, n=9, hole_radius=(0.15, 0.25), seed=8):
        d = graph.sample_to_data(s)
        d.edge_index = d.edge_index[:, :0]
        d.edge_attr = d.edge_attr[:0]
        datas.append(d)
    batch = graph.Batch.from_data_list(datas).to("cuda")
    assert batch.num_edges == 0
    stats = {k: float(v) for k, v in dataset_stats(batch).items() if k not in ("mean_edge_weight",
                                                                                "std_edge_weight")}
    stats.update(mean_edge_weight=0.0, std_edge_weight=1.0)
    steps = 3
    model = _model(steps, stats)
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    pred = model(batch, scale_output=False).local_stress
    gt = (batch.local_stress - model.mean_local_stress) / model.std_local_stress
    total, _, _ = losses.batch_loss(pred, batch, gt, divergence=True, divergence_penalty=10.0)
    model.zero_grad()
    total.backward()
    p64, t64, g64 = _oracle_grads(params, stats, batch, steps, torch.float64, True, 10.0, False)
    assert rel(pred.detach(), p64) < OUT_TOL
    assert abs(float(total) - t64) <= OUT_TOL * abs(t64)
    for name, p in model.named_parameters():
        ref = g64[name]
        if float(ref.abs().max()) == 0.0:
            assert float(p.grad.abs().max()) == 0.0, name        # the edge branch: exactly zero
        else:
            assert rel(p.grad, ref) <= GRAD_TOL, (name, rel(p.grad, ref))
