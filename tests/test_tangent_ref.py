"""The float64 restatements of the tangent-pass entry points (tests/tangent_ref.py), which the GPU op tests hold
the kernels of csrc/pdg_tangent.hip to, anchored to torch.func.jvp through the oracle: the JVP itself against
central differences and against autograd's VJP (the adjoint identity), the composed restatement against the JVP
to 1e-10, and the single pieces against the JVP of the function they linearise."""
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
