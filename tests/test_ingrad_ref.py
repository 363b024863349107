"""The fp64 closed form of the encoders' input gradients (tests/ingrad_ref.py), which the GPU op tests hold
pdg_node_enc_gin / pdg_edge_enc_gin to, against torch autograd through the oracle with requires_grad inputs
and against central finite differences; and the oracle's own input gradients against the reference's
(tests/golden/input_grads.npz, the reference's models.py under the PyG stand-in)."""
import numpy as np
import pytest
import torch

from golden_io import GOLDEN, load
from ingrad_ref import encoder_input_grads
from oracle import epd_oracle as O
from pdg import graph, meshgen

# relative to the input's rms.  Measured on the oracle alone, error of the probed entries per input
# (mean_stress, pos, edge_attr), the differences taken per output element before the sum with gy:
#   1e-4: 1.7e-4 (a relu kink inside a probed interval: ~1e5 relus depend on one input)
#   1e-5: 4e-8, 5e-8, 2e-7     1e-6: 8e-7, 8e-7, 1.3e-6     1e-7: 5e-6, 8e-6, 4e-5
# below 1e-5 the error grows as 1 / h (cancellation through the graph-global LayerNorm statistics), above it
# the kinks take over; 1e-5 leaves a factor 5 to the bound
FD_STEP = 1e-5
FD_TOL = 1e-6
GOLDEN_TOL = 1e-5  # what the oracle's parameter gradients are held to against the fixtures


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


def _case(kind):
    if kind == "single":
        datas = [graph.sample_to_data(meshgen.hole_plate(9, seed=2))]
    else:
        datas = [graph.sample_to_data(s) for s in meshgen.make_dataset(3, n=7, hole_radius=(0.15, 0.3), seed=5)]
    b = graph.Batch.from_data_list(datas)
    st = {"mean_pos": b.pos.mean(), "std_pos": b.pos.std(), "mean_mean_stress": b.mean_stress.mean(),
          "std_mean_stress": b.mean_stress.std(), "mean_local_stress": b.local_stress.mean(),
          "std_local_stress": b.local_stress.std(), "mean_edge_weight": b.edge_attr.mean(),
          "std_edge_weight": b.edge_attr.std()}
    st = {k: v.double() for k, v in st.items()}
    P = {k: v.double() for k, v in O.init_params().items()}
    gy = torch.randn(b.pos.shape[0], 3, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    return b, st, P, gy


def _oracle_vjp(P, st, b, gy, steps, scale_output, scale_input, latents=None):
    """(y, [g_mean_stress, g_pos, g_edge_attr] + the gradients of `latents` outputs) by torch autograd."""
    pos = b.pos.double().requires_grad_(True)
    ms = b.mean_stress.double().requires_grad_(True)
    ea = b.edge_attr.double().requires_grad_(True)
    lat = [] if latents else None
    y = O.epd_forward(P, st, pos, ms, b.nodes_types, b.edge_index, ea, steps, scale_output=scale_output,
                      scale_input=scale_input, latents=lat)
    wrt = [ms, pos, ea] + (list(lat[0]) if latents else [])
    return y.detach(), torch.autograd.grad((y * gy).sum(), wrt)


@pytest.mark.parametrize("scale_input", [True, False])
@pytest.mark.parametrize("kind,steps", [("single", 1), ("batch", 3)])
def test_closed_form_equals_autograd(kind, steps, scale_input):
    """Autograd's gradients of the encoder outputs x_0 / e_0 pushed through the closed form give autograd's
    gradients of mean_stress, pos and edge_attr to 1e-12 (fp64 on both sides, sums in different orders)."""
    b, st, P, gy = _case(kind)
    _, (gm, gp, gea, gx0, ge0) = _oracle_vjp(P, st, b, gy, steps, True, scale_input, latents=True)
    cm, cp, cea = encoder_input_grads(P, st, b.pos.double(), b.mean_stress.double(), b.nodes_types,
                                      b.edge_attr.double(), gx0, ge0, scale_input)
    assert rel(cm, gm) < 1e-12 and rel(cp, gp) < 1e-12 and rel(cea, gea) < 1e-12, \
        (rel(cm, gm), rel(cp, gp), rel(cea, gea))


@pytest.mark.parametrize("scale_output", [True, False])
def test_oracle_input_gradients_match_finite_differences(scale_output):
    """Central differences of <gy, y> in fp64 on a handful of entries of each input, step FD_STEP x the
    input's rms, against the oracle's autograd (and so, by the test above, the closed form) to FD_TOL."""
    b, st, P, gy = _case("single")
    steps = 2
    _, (gm, gp, gea) = _oracle_vjp(P, st, b, gy, steps, scale_output, True)
    base = {"mean_stress": b.mean_stress.double(), "pos": b.pos.double(), "edge_attr": b.edge_attr.double()}

    def f(inp):
        with torch.no_grad():
            return O.epd_forward(P, st, inp["pos"], inp["mean_stress"], b.nodes_types, b.edge_index,
                                 inp["edge_attr"], steps, scale_output=scale_output)

    gen = torch.Generator().manual_seed(4)
    for name, g in (("mean_stress", gm), ("pos", gp), ("edge_attr", gea)):
        x = base[name]
        h = FD_STEP * float(x.pow(2).mean().sqrt())
        idx = torch.randperm(x.numel(), generator=gen)[:5]
        fd = []
        for i in idx:
            d = torch.zeros_like(x).view(-1)
            d[i] = h
            d = d.view_as(x)
            fd.append(float(((f({**base, name: x + d}) - f({**base, name: x - d})) * gy).sum()) / (2 * h))
        fd, an = torch.tensor(fd, dtype=torch.float64), g.reshape(-1)[idx]
        assert rel(fd, an) < FD_TOL, (name, rel(fd, an), fd, an)


@pytest.mark.parametrize("case", ["tiny_periodic", "batch3_div"])
def test_oracle_input_gradients_match_reference(case):
    """The oracle's autograd input gradients against the reference's own (its models.py under the PyG stand-in,
    with the fixture's seeded cotangent), evaluated in float64 inside the reference run's relu region.  The
    reference ran in float32: a relu pre-activation within rounding of zero can land on the other side than
    in exact arithmetic, one such bit moves these gradients by a finite step (8e-4 on batch3_div), and a float32
    rerun flips other bits on another host or thread count (3e-3 on tiny_periodic with 8 threads, 2.9e-4 on
    batch3_div on another CPU; DESIGN.md section 5, "relu region").  The fixture records the reference's region
    as its difference from the float64 one, so this comparison is the same on every host."""
    g = load(case)
    z = np.load(GOLDEN / "input_grads.npz", allow_pickle=False)
    t = lambda k: torch.from_numpy(z[f"{case}.{k}"])
    d = torch.float64
    P = {k: v.to(d) for k, v in g["params"].items()}
    st = {k: v.to(d) for k, v in g["stats"].items()}
    steps = int(g["steps"])
    pos = torch.from_numpy(g["pos"]).to(d).requires_grad_(True)
    ms = torch.from_numpy(g["mean_stress"]).to(d).requires_grad_(True)
    ea = torch.from_numpy(g["edge_attr"]).to(d).requires_grad_(True)
    rest = (torch.from_numpy(g["nodes_types"]), torch.from_numpy(g["edge_index"]))
    own = O.ReluRegion(keep=True)
    with torch.no_grad():
        O.epd_forward(P, st, pos, ms, rest[0], rest[1], ea, steps, region=own)
    masks = {k: (v > 0).clone() for k, v in own.keep.items()}
    keys = [str(k) for k in z[f"{case}.flip_keys"]]
    assert keys == sorted(masks)
    for ki, i in z[f"{case}.flips"]:
        m = masks[keys[int(ki)]].view(-1)
        m[int(i)] = ~m[int(i)]
    y = O.epd_forward(P, st, pos, ms, rest[0], rest[1], ea, steps, scale_output=True, scale_input=True,
                      region=O.ReluRegion(masks=masks))
    gm, gp, gea = torch.autograd.grad((y * t("grad_output").to(d)).sum(), [ms, pos, ea])
    assert rel(y.detach(), t("local_stress")) < GOLDEN_TOL
    for name, got in (("mean_stress", gm), ("pos", gp), ("edge_attr", gea)):
        assert got.shape == t(name).shape
        print(case, name, rel(got, t(name)))
        assert rel(got, t(name)) < GOLDEN_TOL, (name, rel(got, t(name)))
