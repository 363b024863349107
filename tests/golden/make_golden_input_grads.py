"""Generate tests/golden/input_grads.npz from the REFERENCE code: the reference model's own autograd
gradients with respect to mean_stress, pos and edge_attr.

Run where the reference checkout is available (never shipped), after make_golden.py:

    python tests/golden/make_golden_input_grads.py

The reference's models.EncodeProcessDecode runs under make_golden.py's PyG stand-in on the batches of the
``tiny_periodic`` and ``batch3_div`` cases (the same builders, seeds and parameter initialisation, checked
against those fixtures), with the three inputs requiring grad; <grad_output, local_stress> is
back-propagated for a seeded cotangent.  Per case the file holds ``grad_output``, ``local_stress``
(scale_output = scale_input = True) and the gradients ``mean_stress`` (N, 3), ``pos`` (N, 2),
``edge_attr`` (E,).  Data only.

The reference runs in float32, and a relu pre-activation within rounding of zero can come out on the other
side than in exact arithmetic; one such bit moves these gradients by a finite step (8e-4 on batch3_div), and
which bits flip depends on the host's summation order.  So the file also records the reference run's relu
region as its difference from the float64 one: ``flip_keys`` (the oracle's ReluRegion keys) and ``flips``
(rows of key index, flat element index).  They are found with the oracle run in float32 on one thread, which
reproduces the reference's output and gradients bit for bit on the generating host (asserted below); a reader
evaluates the oracle in float64 inside that region and meets the reference's values to float32 rounding on
any host.
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parents[1]))

import make_golden as MG  # noqa: E402
from pdg import meshgen  # noqa: E402

CASES = {
    "tiny_periodic": (lambda: [meshgen.hole_plate(9, seed=1)], True, 2),
    "batch3_div": (lambda: meshgen.make_dataset(3, n=13, hole_radius=(0.15, 0.3), seed=7), True, 3),
}


def run_case(name, samples, periodic, steps, models, datasets, gnn_train):
    graphs = [MG.reference_graph(s, periodic, datasets) for s in samples]
    batch = MG.StubBatch.from_list(graphs)
    st = {
        "mean_pos": batch.pos.mean(), "std_pos": batch.pos.std(),
        "mean_mean_stress": batch.mean_stress.mean(), "std_mean_stress": batch.mean_stress.std(),
        "mean_local_stress": batch.local_stress.mean(), "std_local_stress": batch.local_stress.std(),
        "mean_edge_weight": batch.edge_attr.mean(), "std_edge_weight": batch.edge_attr.std(),
    }
    torch.manual_seed(gnn_train.SEED)
    model = models.EncodeProcessDecode(input_edges_features_size=1, input_nodes_features_size=6,
                                       message_passing_steps=steps, latent_size=128,
                                       output_nodes_features_size=3, **st)
    fix = np.load(HERE / f"{name}.npz", allow_pickle=False)
    for k, v in model.state_dict().items():
        assert np.array_equal(v.numpy(), fix[f"param.{k}"]), f"{name}: parameter {k} differs from the fixture"
    for k in ("pos", "mean_stress", "edge_attr", "edge_index"):
        assert np.array_equal(getattr(batch, k).numpy(), fix[k]), f"{name}: input {k} differs from the fixture"
    for k in ("pos", "mean_stress", "edge_attr"):
        setattr(batch, k, getattr(batch, k).clone().requires_grad_(True))
    out = model.forward(batch, scale_output=True, scale_input=True).local_stress
    gy = torch.randn(out.shape, generator=torch.Generator().manual_seed(1234 + steps))
    gm, gp, gea = torch.autograd.grad((out * gy).sum(), [batch.mean_stress, batch.pos, batch.edge_attr])
    assert np.allclose(out.detach().numpy(), fix["out_scaled"], rtol=0, atol=0)
    flip_keys, flips = relu_flips(model, st, batch, gy, steps, (out.detach(), gm, gp, gea))
    print(f"{name}: {len(flips)} relu bits differ from float64: {[(flip_keys[k], i) for k, i in flips]}")
    print(f"{name}: N={out.shape[0]} E={gea.shape[0]} |g_ms|={float(gm.norm()):.4e} |g_pos|={float(gp.norm()):.4e} "
          f"|g_ea|={float(gea.norm()):.4e}")
    return {f"{name}.grad_output": gy.numpy(), f"{name}.local_stress": out.detach().numpy(),
            f"{name}.mean_stress": gm.numpy(), f"{name}.pos": gp.numpy(), f"{name}.edge_attr": gea.numpy(),
            f"{name}.flip_keys": np.array(flip_keys), f"{name}.flips": np.array(flips, np.int64).reshape(-1, 2)}


def relu_flips(model, st, batch, gy, steps, ref):
    """The relu bits of the reference run that differ from the float64 evaluation (see the module docstring)."""
    from oracle import epd_oracle as O
    keep = {}
    for dt in (torch.float32, torch.float64):
        P = {k: v.detach().to(dt) for k, v in model.state_dict().items()}
        s = {k: v.to(dt) for k, v in st.items()}
        pos, ms, ea = (getattr(batch, k).detach().to(dt).requires_grad_(True) for k in ("pos", "mean_stress", "edge_attr"))
        region = O.ReluRegion(keep=True)
        y = O.epd_forward(P, s, pos, ms, batch.nodes_types, batch.edge_index, ea, steps, region=region)
        if dt == torch.float32:
            got = (y.detach(), *torch.autograd.grad((y * gy).sum(), [ms, pos, ea]))
            assert all(torch.equal(a, b) for a, b in zip(got, ref)), "the float32 oracle is not the reference bit for bit"
        keep[dt] = region.keep
    keys = sorted(keep[torch.float64])
    flips = []
    for ki, k in enumerate(keys):
        d = (keep[torch.float32][k] > 0) != (keep[torch.float64][k] > 0)
        flips += [(ki, int(i)) for i in d.reshape(-1).nonzero().reshape(-1)]
    return keys, flips


def main():
    MG.install_stubs()
    os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(MG.REF))
    sys.path.insert(0, str(MG.REF / "scripts"))
    torch.set_num_threads(1)
    from gnn_local_stress import datasets, models  # reference package
    import gnn_train  # reference script module

    rec = {}
    for name, (mk, periodic, steps) in CASES.items():
        rec.update(run_case(name, mk(), periodic, steps, models, datasets, gnn_train))
    np.savez_compressed(HERE / "input_grads.npz", **rec)


if __name__ == "__main__":
    main()
