"""The float64 restatements of the tangent-pass entry points (tests/tangent_ref.py), which the GPU op tests hold
the kernels of csrc/pdg_tangent.hip to, anchored to torch.func.jvp through the oracle: the JVP itself against
central differences and against autograd's VJP (the adjoint identity), the composed restatement against the JVP
to 1e-10, and the single pieces against the JVP of the function they linearise.  Then the dtype / explicit-totals
variants against those forms, and wrong restatements on the inputs of tests/test_gpu_tangent_ops.py."""
import pytest
import torch

import tangent_ref as R
from oracle import epd_oracle as O
from pdg import graph, meshgen

D = torch.float64
COMPOSED_TOL = 1e-10
FD_TOL = 1e-6     # the bound tests/test_ingrad_ref.py holds the oracle's VJP to against central differences
ADJ_TOL = 1e-12


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


def _case():
    b = graph.Batch.from_data_list([graph.sample_to_data(meshgen.hole_plate(9, seed=2))])
    st = {"mean_pos": b.pos.mean(), "std_pos": b.pos.std(), "mean_mean_stress": b.mean_stress.mean(),
          "std_mean_stress": b.mean_stress.std(), "mean_local_stress": b.local_stress.mean(),
          "std_local_stress": b.local_stress.std(), "mean_edge_weight": b.edge_attr.mean(),
          "std_edge_weight": b.edge_attr.std()}
    st = {k: v.double() for k, v in st.items()}
    P = {k: v.double() for k, v in O.init_params().items()}
    gen = torch.Generator().manual_seed(21)
    dirs = (torch.randn(b.mean_stress.shape, dtype=D, generator=gen), torch.randn(b.pos.shape, dtype=D, generator=gen),
            torch.randn(b.edge_attr.shape, dtype=D, generator=gen))
    return b, st, P, dirs


def _f(P, st, b, steps, scale_output=True, scale_input=True):
    return lambda ms, pos, ea: O.epd_forward(P, st, pos, ms, b.nodes_types, b.edge_index, ea, steps,
                                             scale_output=scale_output, scale_input=scale_input)


def _jvp(P, st, b, steps, dirs, scale_output=True, scale_input=True):
    prim = (b.mean_stress.double(), b.pos.double(), b.edge_attr.double())
    return torch.func.jvp(_f(P, st, b, steps, scale_output, scale_input), prim, tuple(dirs))


def test_oracle_jvp_meets_central_differences_and_the_adjoint_identity():
    b, st, P, dirs = _case()
    steps = 3
    y, dy = _jvp(P, st, b, steps, dirs)
    f = _f(P, st, b, steps)
    prim = (b.mean_stress.double(), b.pos.double(), b.edge_attr.double())
    # a unit-variance direction in every entry of all three inputs at once (rms 43, 59, 14).  Measured error
    # against the step: 1e-6: 6.3e-7, 1e-7: 1.1e-5, 1e-8: 8e-5 (cancellation, growing as 1 / h);
    # 1e-5 x the input rms: 1.1e-2 (relu kinks inside the interval: every relu depends on the direction)
    h = 1e-6
    with torch.no_grad():
        fd = (f(*(p + h * d for p, d in zip(prim, dirs))) - f(*(p - h * d for p, d in zip(prim, dirs)))) / (2 * h)
    print("jvp vs central differences", rel(fd, dy))
    assert rel(fd, dy) < FD_TOL, rel(fd, dy)
    u = torch.randn(y.shape, dtype=D, generator=torch.Generator().manual_seed(22))
    req = tuple(p.clone().requires_grad_(True) for p in prim)
    g = torch.autograd.grad((f(*req) * u).sum(), req)
    lhs, rhs = float((u * dy).sum()), sum(float((gi * di).sum()) for gi, di in zip(g, dirs))
    print("adjoint identity", abs(lhs - rhs) / abs(lhs))
    assert abs(lhs - rhs) <= ADJ_TOL * abs(lhs)


@pytest.mark.parametrize("scale_input", [True, False])
@pytest.mark.parametrize("scale_output", [True, False])
@pytest.mark.parametrize("steps", [1, 3])
def test_composed_restatement_equals_jvp(steps, scale_output, scale_input):
    b, st, P, dirs = _case()
    y, dy = _jvp(P, st, b, steps, dirs, scale_output, scale_input)
    ry, rdy = R.epd_tangent(P, st, b.pos, b.mean_stress, b.nodes_types, b.edge_index, b.edge_attr, steps, *dirs,
                            scale_output=scale_output, scale_input=scale_input)
    print(f"s{steps} o{int(scale_output)} i{int(scale_input)}: y {rel(ry, y):.1e} dy {rel(rdy, dy):.1e}")
    assert rel(ry, y) < COMPOSED_TOL and rel(rdy, dy) < COMPOSED_TOL, (rel(ry, y), rel(rdy, dy))


def test_each_direction_alone_and_linearity():
    """A direction in one input only (the others zero) sums to the joint tangent: the composition is linear."""
    b, st, P, dirs = _case()
    z = [torch.zeros_like(d) for d in dirs]
    args = (P, st, b.pos, b.mean_stress, b.nodes_types, b.edge_index, b.edge_attr, 2)
    _, joint = R.epd_tangent(*args, *dirs)
    parts = [R.epd_tangent(*args, *[dirs[j] if j == i else z[j] for j in range(3)])[1] for i in range(3)]
    assert all(float(p.norm()) > 0 for p in parts)
    assert rel(sum(parts), joint) < 1e-12


def test_layer_norm_tangent_equals_jvp():
    gen = torch.Generator().manual_seed(23)
    a = torch.relu(torch.randn(37, 128, dtype=D, generator=gen) + 0.3)
    da = torch.randn(37, 128, dtype=D, generator=gen) + 0.7
    g, bb = torch.randn(128, dtype=D, generator=gen), torch.randn(128, dtype=D, generator=gen)
    _, ref = torch.func.jvp(lambda x: O.graph_layer_norm(x, g, bb), (a,), (da,))
    assert rel(R.ln_tan(da, a, g), ref) < 1e-12
    t1, t2 = R.pairs_ref(da, a)
    assert abs(float(t1) - float(da.sum())) <= 1e-12 * float(da.abs().sum())
    assert abs(float(t2)) > 1e-3 * float(da.norm() * (a - a.mean()).norm())   # both terms matter in this draw
    # a constant tensor: sigma = 0, the second term is defined as 0 (the kernels' choice)
    assert torch.isfinite(R.ln_tan(da, torch.ones_like(a), g)).all()


def test_edge_length_tangent_equals_jvp_and_is_zero_on_zero_lengths():
    gen = torch.Generator().manual_seed(24)
    N, E = 40, 300
    pos, dpos = torch.randn(N, 2, dtype=D, generator=gen), torch.randn(N, 2, dtype=D, generator=gen)
    src, dst = torch.randint(0, N, (E,), generator=gen), torch.randint(0, N, (E,), generator=gen)
    src[:7] = dst[:7]                       # coincident endpoints: length 0
    ln = (pos[src] - pos[dst]).norm(dim=1)
    ln[7:12] = 0.0                          # periodic pairs: distinct nodes, a constant length 0
    got = R.edge_len_tan_ref(src, dst, pos, dpos, ln)
    assert float(got[:12].abs().max()) == 0.0
    _, ref = torch.func.jvp(lambda p: (p[src[12:]] - p[dst[12:]]).norm(dim=1), (pos,), (dpos,))
    keep = ln[12:] > 0
    assert rel(got[12:][keep], ref[keep]) < 1e-12


# ---------------------------------------------------------------- the dtype / explicit-totals variants and the inputs
# of tests/test_gpu_tangent_ops.py: with totals and statistics left at their defaults they are the functions
# anchored above; on the GPU suite's own inputs, wrong restatements are >= 1000 x the GPU tolerance away.

WRONG_FACTOR = 1000
_inputs = {}


def _in(M, cond):
    if (M, cond) not in _inputs:
        _inputs[(M, cond)] = R.tan_inputs(M, cond)
    return _inputs[(M, cond)]


def _old(i):
    """Today's functions, restated with ln_tan itself (the form anchored to the JVP)."""
    dx = R.ln_tan(i.da_prev, i.a_prev, i.g) + i.res.double()
    W1, W2 = i.We1.double(), i.W2.double()
    C = dx @ W1[:, 256:].T
    dP, dQ = i.dP.double(), i.dQ.double()
    m = (((C + dP[i.dst] + dQ[i.src]) * (i.a1 > 0)) @ W2.T) * (i.a2 > 0)
    dy = ((dx @ i.Wd1.double().T) * (i.a1 > 0)) @ i.Wd2.double().T * i.std_out
    return dx, dx @ W1[:, :128].T, m, dy


@pytest.mark.parametrize("cond", ["p", "c"])
def test_variants_at_their_defaults_equal_the_anchored_functions(cond):
    i = _in(77, cond)
    dx, dP, m, dy = _old(i)
    assert rel(R.ln_tan_given(i.da_prev, i.a_prev, i.g), R.ln_tan(i.da_prev, i.a_prev, i.g)) < 1e-12
    t = R.pairs_ref(i.da_prev, i.a_prev)
    st = R.stat_of(i.a_prev)
    for kw in ({}, {"totals": t, "stat": st}):
        x, P_, _ = R.node_pre_tan_ref(i.da_prev, i.a_prev, i.g, i.res, i.We1, **kw)
        assert rel(x, dx) < 1e-12 and rel(P_, dP) < 1e-12
        e, m_, _ = R.edge_tan_ref(i.da_prev, i.a_prev, i.g, i.res, i.src, i.dst, i.dP, i.dQ, i.We1, i.W2, i.a1, i.a2, **kw)
        assert rel(e, dx) < 1e-12 and rel(m_, m) < 1e-12
        assert rel(R.decoder_tan_ref(i.da_prev, i.a_prev, i.g, i.res, i.Wd1, i.a1, i.Wd2, i.std_out, **kw), dy) < 1e-12
    s = R.seg_tan_inputs(25, cond)
    t_rows = R.ln_tan(s.da_prev, s.a_prev, s.g)
    idx = torch.repeat_interleave(torch.arange(s.N), s.deg)
    want = torch.zeros(s.N, 128, dtype=D).index_add_(0, idx, t_rows)
    assert rel(R.segment_sum_tan_ref(s.rowptr, s.da_prev, s.a_prev, s.g), want) < 1e-12


@pytest.mark.parametrize("cond", ["p", "c"])
def test_inputs_make_both_layer_norm_terms_count_and_fp32_stays_inside_its_bound(cond):
    """The two assertions of the GPU suite on its inputs, the small-sigma conditioning's eps / sigma, and the fp32
    restatement's own distance (the GPU bound of conditioning "c" is ROW_FACTOR x it) below TOL_LN."""
    for M in (1, 17, 77, 4099):
        i = _in(M, cond)
        st = R.stat_of(i.a_prev)
        t1, t2 = R.pairs_ref(i.da_prev, i.a_prev)
        xc = i.a_prev.double() - st.mean_d
        assert abs(float(t1)) / i.da_prev.numel() > 0.3
        assert abs(float(t2)) > 0.2 * float(i.da_prev.double().norm() * xc.norm())
        if cond == "c":
            assert 0.02 < 1e-5 / st.std_d < 1.0
        kw = dict(totals=(t1, t2), stat=st)
        r64 = R.node_pre_tan_ref(i.da_prev, i.a_prev, i.g, i.res, i.We1, **kw)
        r32 = R.node_pre_tan_ref(i.da_prev, i.a_prev, i.g, i.res, i.We1, torch.float32, **kw)
        for a, b in zip(r32, r64):
            assert rel(a, b) < (R.TOL if cond == "p" else R.TOL_LN) / R.ROW_FACTOR, (M, rel(a, b))


def _far(name, wrong, ref, tol):
    d = rel(wrong, ref)
    print(f"{name}: {d:.2e} (needs {WRONG_FACTOR * tol:.1e})")
    assert d >= WRONG_FACTOR * tol, (name, d, tol)


@pytest.mark.parametrize("cond", ["p", "c"])
def test_wrong_restatements_are_far_outside_the_gpu_bounds(cond):
    """On the GPU suite's inputs at (77, 37).  The GPU tolerance: TOL in "p"; in "c" ROW_FACTOR x the fp32
    restatement's distance of the same output, at most ROW_FACTOR x TOL_LN: the figure used here.  `den` for sigma
    in c2 is told apart in "c" only (eps / sigma ~ 2e-5 in "p": the reason the conditioning exists)."""
    i = _in(77, cond)
    tol = R.TOL if cond == "p" else R.ROW_FACTOR * R.TOL_LN
    st = R.stat_of(i.a_prev)
    t1, t2 = R.pairs_ref(i.da_prev, i.a_prev)
    pre = lambda **kw: R.node_pre_tan_ref(i.da_prev, i.a_prev, i.g, kw.pop("res", i.res), i.We1, stat=st, **kw)
    ref = pre(totals=(t1, t2))
    if cond == "c":
        wrong = pre(totals=(t1, t2 * st.std_d / st.den_d))       # c2 = T2 / (n den^3)
        for k, nm in enumerate(("dx", "dP", "dQ")):
            _far(f"den for sigma in c2, {nm}", wrong[k], ref[k], tol)
    for nm, w in (("T1 dropped", pre(totals=(0.0, t2))), ("T2 dropped", pre(totals=(t1, 0.0))),
                  ("residual dropped", pre(totals=(t1, t2), res=None))):
        for k in range(3):
            _far(f"{nm} [{k}]", w[k], ref[k], tol)
    dec = lambda **kw: R.decoder_tan_ref(i.da_prev, i.a_prev, i.g, kw.pop("res", i.res), i.Wd1, i.a1, i.Wd2, i.std_out,
                                         stat=st, **kw)
    dref = dec(totals=(t1, t2))
    _far("decoder: T2 dropped", dec(totals=(t1, 0.0)), dref, tol)
    _far("decoder: residual dropped", dec(totals=(t1, t2), res=None), dref, tol)
    # the edge tangent: gathers swapped, the mask of a1 for a2
    args = (i.da_prev, i.a_prev, i.g, i.res)
    e = R.edge_tan_ref(*args, i.src, i.dst, i.dP, i.dQ, i.We1, i.W2, i.a1, i.a2, i.a1b, i.a2b)
    sw = R.edge_tan_ref(*args, i.dst, i.src, i.dP, i.dQ, i.We1, i.W2, i.a1, i.a2, i.a1b, i.a2b)
    _far("dP[src] + dQ[dst] for the message", sw[1], e[1], tol)
    _far("dP[dst] + dQ[src] for the edge update", sw[2], e[2], tol)
    mk = R.edge_tan_ref(*args, i.src, i.dst, i.dP, i.dQ, i.We1, i.W2, i.a1, i.a1, i.a1b, i.a1b)
    _far("mask of a1 for a2 (message)", mk[1], e[1], tol)
    _far("mask of a1 for a2 (edge update)", mk[2], e[2], tol)
    # node_net: Wn1a / Wn1b swapped, the mask of a1 for a2
    nref = R.node_net_tan_ref(i.rows2, i.res, i.Wn1, i.W2, i.a1, i.a2)
    _far("Wn1a / Wn1b swapped", R.node_net_tan_ref(i.res, i.rows2, i.Wn1, i.W2, i.a1, i.a2), nref, R.TOL)
    _far("node_net: mask of a1 for a2", R.node_net_tan_ref(i.rows2, i.res, i.Wn1, i.W2, i.a1, i.a1), nref, R.TOL)
    _far("node_enc: mask of a1 for a2", R.node_enc_tan_ref(i.dx_in, i.a1, i.W0n, i.W2, i.a1),
         R.node_enc_tan_ref(i.dx_in, i.a1, i.W0n, i.W2, i.a2), R.TOL)
    # the aggregation: LayerNorm tangent after the segment sum
    for N in (25, 57, 40):
        s = R.seg_tan_inputs(N, cond)
        sref = R.segment_sum_tan_ref(s.rowptr, s.da_prev, s.a_prev, s.g)
        idx = torch.repeat_interleave(torch.arange(s.N), s.deg)
        sum_ = lambda x: torch.zeros(s.N, 128, dtype=D).index_add_(0, idx, x.double())
        _far(f"LayerNorm after the segment sum N={N}", R.ln_tan(sum_(s.da_prev), sum_(s.a_prev), s.g), sref, tol)
        ss = R.stat_of(s.a_prev)
        u1, u2 = R.pairs_ref(s.da_prev, s.a_prev)
        seg = lambda t: R.segment_sum_tan_ref(s.rowptr, s.da_prev, s.a_prev, s.g, totals=t, stat=ss)
        _far(f"segment sum: T1 dropped N={N}", seg((0.0, u2)), sref, tol)
        _far(f"segment sum: T2 dropped N={N}", seg((u1, 0.0)), sref, tol)
        if cond == "c":
            _far(f"segment sum: den for sigma N={N}", seg((u1, u2 * ss.std_d / ss.den_d)), sref, tol)


def test_integer_exact_family_is_integer_and_small():
    """Every value of the integer-exact family's references is an integer below 2^24, with the hand-made totals
    (n EXACT_K, 0) split over any number of pairs."""
    for M in (1, 33, 77):
        i = _in(M, "x")
        n = M * 128
        for npairs in (1, 5, 65):
            pr = R.exact_pairs(n, npairs)
            assert float(pr[0::2].sum()) == n * R.EXACT_K and float(pr[1::2].sum()) == 0.0
        kw = dict(totals=(n * R.EXACT_K, 0.0), stat=R.unit_stat(n))
        outs = list(R.node_pre_tan_ref(i.da_prev, i.a_prev, i.g, i.res, i.We1, **kw))
        outs += list(R.edge_tan_ref(i.da_prev, i.a_prev, i.g, i.res, i.src, i.dst, i.dP, i.dQ, i.We1, i.W2, i.a1, i.a2,
                                    i.a1b, i.a2b, **kw))
        outs.append(R.decoder_tan_ref(i.da_prev, i.a_prev, i.g, i.res, i.Wd1, i.a1, i.Wd2, i.std_out, **kw))
        outs.append(R.node_net_tan_ref(i.rows2, i.res, i.Wn1, i.W2, i.a1, i.a2))
        outs.append(R.node_enc_tan_ref(i.dx_in, i.a1, i.W0n, i.W2, i.a2))
        outs.append(R.edge_enc_tan_ref(i.de_in, i.e_in, i.w0e, i.b0e, i.W2, i.a2))
        for o in outs:
            assert torch.equal(o, o.round()) and float(o.abs().max()) < 2 ** 24 and float(o.abs().max()) > 0
        # the outputs differ from a neighbouring c1: the totals are felt
        other = R.node_pre_tan_ref(i.da_prev, i.a_prev, i.g, i.res, i.We1, totals=(n * (R.EXACT_K + 1), 0.0), stat=kw["stat"])
        assert not torch.equal(other[0], outs[0])


def test_chain_composition_fp32_stays_inside_the_model_tier():
    """The chain of the GPU suite: the fp32 composition's distance from the fp64 one, ROW_FACTOR x which is the GPU
    bound, leaves that bound below the model tier's 3e-5 and above the rounding of one fp32 product."""
    c = R.chain_inputs()
    d64, d32 = R.chain_ref(c), R.chain_ref(c, torch.float32)
    e = rel(d32, d64)
    print(f"chain N={c.N} E={c.E}: fp32 composition {e:.2e}")
    assert d64.shape == (c.N, 3) and float(d64.norm()) > 0
    assert 1e-8 < e and R.ROW_FACTOR * e < 3e-5
