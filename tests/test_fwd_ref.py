"""The fp64 restatements of the per-step forward (tests/fwd_ref.py), which tests/test_gpu_fwd.py holds the forward
kernels to, against oracle.epd_oracle (_mlp, processor_step, graph_layer_norm: the model's own code path), and a
check that the comparisons the GPU tests make, on the inputs they use, can tell the closed forms from six subtly
wrong ones."""
import pytest
import torch

import fwd_ref as F
from edge_bwd_ref import L, LN_EPS, hub_graph
from golden_io import load
from oracle import epd_oracle as O

TOL = 1e-12   # fp64 on both sides, the sums in different orders
EDGE_CASES = [1, 15, 16, 17, 31, 32, 33, 77, 257, 4099, 8193]   # the E of tests/test_gpu_fwd.py's CASES


def rel(a, b):
    return float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-300))


def oracle_chain(p, x_in, e_in, src, dst, steps):
    """(x, e) after the encoders and after every step, and the decoder's output, through the oracle's own pieces."""
    ei = torch.stack([src, dst])
    x, e = O._mlp(x_in, p, "node_encoder"), O._mlp(e_in, p, "edge_encoder")
    lat = [(x, e)]
    for _ in range(steps):
        x, e = O.processor_step(p, x, e, ei)
        lat.append((x, e))
    return lat, O._mlp(x, p, "node_decoder", layer_norm=False)


def check_chain(p, x_in, e_in, src, dst, steps):
    lat, y = oracle_chain(p, x_in, e_in, src, dst, steps)
    enc, rs, dec = F.forward_ref(p, x_in, e_in, src, dst, steps)
    for t, r in enumerate(rs):   # the step's inputs are the oracle's latents before it
        assert rel(r.x_t, lat[t][0]) < TOL and rel(r.e_t, lat[t][1]) < TOL, t
    # the last step's edge update is not evaluated (eu = False); the one before it gives the oracle's e
    assert rel(dec.x_S, lat[-1][0]) < TOL and rel(dec.y, y) < TOL
    ln = lambda a, g, b: O.graph_layer_norm(a, g, b)
    r = rs[0]
    x0, e0 = lat[0]
    msg = ln(r.a2m, p["processor.edge_net.4.weight"], p["processor.edge_net.4.bias"])
    aggr = torch.zeros_like(x0).index_add_(0, dst, msg)
    assert rel(r.aggr, aggr) < TOL
    assert rel(F.ln_res_ref(r.a2e, r.st_e, p["processor.edge_net.4.weight"], p["processor.edge_net.4.bias"], e0),
               lat[1][1]) < TOL
    assert rel(F.ln_res_ref(r.a2n, r.st_n, p["processor.node_net.4.weight"], p["processor.node_net.4.bias"], x0),
               lat[1][0]) < TOL
    assert rel(r.P[dst] + r.Q[src], torch.cat([x0[dst], x0[src]], 1) @ p["processor.edge_net.0.weight"][:, :2 * L].T) < TOL


def test_eps_is_the_oracles():
    assert LN_EPS == O.LN_EPS and float(F.EPS32) == float(torch.tensor(1e-5, dtype=torch.float32))


def test_step_ref_equals_oracle_on_hub_graph():
    N, src, dst = hub_graph(77)[:3]
    p = {k: v.double() for k, v in O.init_params(seed=3).items()}
    g = torch.Generator().manual_seed(5)
    for k in p:   # LayerNorm weights / biases off their initial 1 / 0
        if k.endswith(".4.weight") or k.endswith(".4.bias"):
            p[k] = p[k] + 0.2 * torch.randn(L, generator=g, dtype=torch.float64)
    x_in = torch.randn(N, 6, generator=g, dtype=torch.float64)
    e_in = torch.randn(77, 1, generator=g, dtype=torch.float64)
    check_chain(p, x_in, e_in, src, dst, 3)


def test_step_ref_equals_oracle_on_golden_tiny_periodic():
    gd = load("tiny_periodic")
    p = {k: v.double() for k, v in gd["params"].items()}
    st = {k: v.double() for k, v in gd["stats"].items()}
    f = lambda k: torch.from_numpy(gd[k])
    x_in, e_in = O.format_inputs(st, f("pos").double(), f("mean_stress").double(), f("nodes_types").double(),
                                 f("edge_attr").double(), True)
    ei = f("edge_index")
    order = torch.sort(ei[1] * x_in.shape[0] + ei[0], stable=True).indices   # dst-sorted, as the plan delivers them
    src, dst = ei[0][order], ei[1][order]
    check_chain(p, x_in, e_in[order], src, dst, int(gd["steps"]))
    # and the whole model, output scaling included, against the oracle's forward in the caller's edge order
    stats8 = torch.stack([st[k] for k in O.STAT_KEYS])
    _, _, dec = F.forward_ref(p, x_in, e_in[order], src, dst, int(gd["steps"]), stats8, True)
    y = O.epd_forward(p, st, f("pos").double(), f("mean_stress").double(), f("nodes_types").double(), ei,
                      f("edge_attr").double(), int(gd["steps"]))
    assert rel(dec.y, y) < TOL


def test_ln_stat_ref_fields():
    a = torch.relu(torch.randn(33, L, dtype=torch.float64)).float()
    s = F.ln_stat_ref(a)
    assert abs(s.mean_d - float(a.double().mean())) < TOL and abs(s.std_d - float(a.double().std(unbiased=False))) < TOL
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    assert s.mean == float(f32(s.mean_d)) and s.std_ == float(f32(s.std_d))
    assert s.den == float(f32(s.std_) + f32(1e-5)) and s.rstd == float(f32(1.0) / f32(s.den))
    assert F.fp32_fields(0.0, float(f32(1.0) - f32(1e-5)))[2:] == (1.0, 1.0)   # the unit statistics of the exact family


# ------------------------------------------------------------------------------------------ wrong restatements

@pytest.mark.parametrize("kind,cond", [("hub", "p"), ("ends", "c")])
@pytest.mark.parametrize("E", EDGE_CASES)
def test_gpu_inputs_tell_wrong_edge_forms_apart(E, kind, cond):
    """On the randn inputs of the GPU suite's edge cases, each wrong form of the edge step lies at least 1000 x the
    bound the GPU test applies to that output away from the closed form (the exact family needs no such margin: it
    demands equality, and the wrong forms below differ on it too)."""
    N, src, dst = F.graph_of(kind, E)
    i = F.randn_edge_inputs(E, N, cond)
    st = F.ln_stat_ref(i.a2_prev)
    tol = F.TOL if cond == "p" else F.TOL_LN
    args = lambda **k: {**dict(a2_prev=i.a2_prev, stat=st, g=i.g, b=i.b, e_res=i.e_res, src=src, dst=dst, P=i.P, Q=i.Q,
                               W1=i.W1, b1=i.b1, W2=i.W2, b2=i.b2), **k}
    r = F.edge_step_ref(**args())
    swapped = F.edge_step_ref(**args(src=dst, dst=src))            # the message takes P[src] + Q[dst]
    if not bool((src == dst).all()):
        assert rel(swapped.a1m, r.a1m) > 1000 * tol and rel(swapped.a2m, r.a2m) > 1000 * tol
    nores = F.edge_step_ref(**args(e_res=None))                     # residual dropped
    assert rel(nores.e_t, r.e_t) > 1000 * tol
    if cond == "c":                                                 # den = std: only where eps counts
        noeps = F.edge_step_ref(**args(stat=F.SimpleNamespace(**{**st.__dict__, "den_d": st.std_d})))
        assert 0.02 < LN_EPS / st.std_d < 1.0
        assert rel(noeps.e_t, r.e_t) > 1000 * tol and rel(noeps.a2m, r.a2m) > 1000 * tol
    x = F.exact_edge_inputs(E, N)
    xa = dict(a2_prev=x.a2_prev, stat=F.UNIT, g=x.g, b=x.b, e_res=x.e_res, P=x.P, Q=x.Q, W1=x.W1, b1=x.b1, W2=x.W2, b2=x.b2)
    rx = F.edge_step_ref(src=src, dst=dst, **xa)
    assert float(rx.a2m.max()) < 2 ** 11 and float(rx.a2e.max()) < 2 ** 11 and float(rx.a2m.max()) > 0
    if not bool((src == dst).all()):
        assert not torch.equal(F.edge_step_ref(src=dst, dst=src, **xa).a1m, rx.a1m)
    assert not torch.equal(F.edge_step_ref(src=src, dst=dst, **{**xa, "e_res": None}).e_t, rx.e_t)


NODE_N = [1, 15, 16, 17, 33, 77, 4099, 257]   # the N of tests/test_gpu_fwd.py's NODE_CASES
SEG_N = [8, 9, 77, 64 * 256 + 9]              # its segment-sum sizes with rows (the last: 256 CUs)


@pytest.mark.parametrize("cond", ["p", "c"])
@pytest.mark.parametrize("N", NODE_N)
def test_gpu_inputs_tell_swapped_wa_wb_apart(N, cond):
    """Wa / Wb swapped in the node pre-pass, everything else the same, on fwd_ref.node_inputs (the GPU suite's): P
    and Q at least 1000 x their bound away; and unequal in the integer-exact family."""
    tol = F.TOL if cond == "p" else F.TOL_LN
    for c in (cond, "x"):
        i = F.node_inputs(N, c)
        st = F.UNIT if c == "x" else F.ln_stat_ref(i.a2n)
        swapped = torch.cat([i.W1[:, L:2 * L], i.W1[:, :L], i.W1[:, 2 * L:]], 1)
        r, sw = F.node_pq_ref(i.a2n, st, i.g, i.b, i.x_res, i.W1), F.node_pq_ref(i.a2n, st, i.g, i.b, i.x_res, swapped)
        assert torch.equal(sw.x_t, r.x_t)
        if c == "x":
            assert not torch.equal(sw.P, r.P) and not torch.equal(sw.Q, r.Q)
        else:
            assert rel(sw.P, r.P) > 1000 * tol and rel(sw.Q, r.Q) > 1000 * tol


@pytest.mark.parametrize("cond", ["p", "c"])
@pytest.mark.parametrize("N", SEG_N)
def test_gpu_inputs_tell_layernorm_after_the_sum_apart(N, cond):
    """LayerNorm applied to the summed rows instead of per row, on fwd_ref.seg_inputs (the GPU suite's)."""
    tol = F.TOL if cond == "p" else F.TOL_LN
    for c in (cond, "x"):
        i = F.seg_inputs(N, c)
        st = F.UNIT if c == "x" else F.ln_stat_ref(i.rows)
        aggr, _ = F.segment_sum_ref(i.dst, i.rows, st, i.g, i.b, N)
        raw, _ = F.segment_sum_ref(i.dst, i.rows, None, None, None, N)
        late = F.ln_res_ref(raw, st, i.g, i.b) * (i.deg > 0).unsqueeze(1)
        if c == "x":
            assert not torch.equal(late, aggr)
        else:
            assert rel(late, aggr) > 1000 * tol


@pytest.mark.parametrize("cond", ["p", "c"])
def test_statistics_arrays_bound_and_sample_std(cond):
    """The statistics tests' arrays (fwd_ref.stat_array): the derived bound on mean_d / std_d stays below TOL_STAT =
    1e-9 at every nparts, and the sample std (relative 1 / (2 n) of std_d, 1.3e-6 at n = 3001 x 128) lies 1000 x
    TOL_STAT away."""
    a, ref = F.stat_array(cond)
    for nparts in F.NPARTS:
        b_mean, b_std = F.stat_bound(a.numel(), nparts, ref)
        assert b_mean <= b_std < F.TOL_STAT
    assert abs(float(a.double().std()) / ref.std_d - 1) > 1000 * F.TOL_STAT
