"""The engine's launch sequence, pinned: the ordered names of the C-ABI entry points one
EPDEngine.forward / EPDEngine.backward issues (what pdg.serve captures into a HIP graph and the bench
counts), per case, against tests/golden/engine_launches.json.

The golden was recorded by tests/golden/make_engine_launches.py with the engine as it was before its
forward and backward were split into phases; a change of the engine's structure must leave every list as
it is, a change of the sequence itself re-records the file on purpose.

Names only (pdg.lib.lib.hook gets the entry-point name after every status-returning call), so each case
costs one small forward and backward.  The cases are the smallest that reach each branch of the engine:
first / middle / last step (steps = 3) and a step that is all three (steps = 1) on a mesh with fewer edges
than blocks x 32, inference and training, each kept kernel variant off, the edgeless batch, an inference
forward on either side of INFER_PIPE_MIN_EDGES, and more than 32 segments per deferred weight gradient.
"""
import json
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "engine_launches.json"

# hole_plate(INFER_N) is the smallest single mesh with at least INFER_PIPE_MIN_EDGES edges
# (33456 at n = 75, 32566 at n = 74: asserted in record())
INFER_N = 75

# case -> (batch, steps, training, engine attributes set to a non-default value)
CASES = {
    "infer_s3": ("mesh9", 3, False, {}),
    "train_s3": ("mesh9", 3, True, {}),
    "train_s3_unfused_wgrad": ("mesh9", 3, True, {"fused_edge_wgrad": False}),
    "train_s3_stored_gz1e": ("mesh9", 3, True, {"gz1e_from_gc": False}),
    "train_s3_plain_edge_fwd": ("mesh9", 3, True, {"coop_fwd": False}),
    "infer_s1": ("mesh9", 1, False, {}),
    "train_s1": ("mesh9", 1, True, {}),
    "train_edgeless_s3": ("edgeless", 3, True, {}),
    "infer_at_pipe_min_edges": ("at_min", 2, False, {}),
    "infer_below_pipe_min_edges": ("below_min", 2, False, {}),
    "train_s33_unfused_wgrad": ("mesh9", 33, True, {"fused_edge_wgrad": False}),
}


def _batch(kind):
    from gpu_common import dataset_stats, make_batch
    from pdg import graph, meshgen
    from pdg.engine import INFER_PIPE_MIN_EDGES
    if kind == "edgeless":   # the batch of test_gpu_model.py::test_edgeless_batch_matches_oracle
        datas = []
        for s in meshgen.make_dataset(2, n=9, hole_radius=(0.15, 0.25), seed=8):
            d = graph.sample_to_data(s)
            d.edge_index = d.edge_index[:, :0]
            d.edge_attr = d.edge_attr[:0]
            datas.append(d)
        batch = graph.Batch.from_data_list(datas).to("cuda")
        stats = {k: float(v) for k, v in dataset_stats(batch).items()}
        stats.update(mean_edge_weight=0.0, std_edge_weight=1.0)
        return batch, stats
    if kind == "mesh9":
        samples = meshgen.make_dataset(1, n=9, hole_radius=(0.15, 0.3), seed=7)
        assert samples[0].num_edges < 256 * 32
    else:
        samples = [meshgen.hole_plate(INFER_N if kind == "at_min" else INFER_N - 1, seed=2)]
        assert (samples[0].num_edges >= INFER_PIPE_MIN_EDGES) == (kind == "at_min"), samples[0].num_edges
    batch = make_batch(samples)
    return batch, {k: float(v) for k, v in dataset_stats(batch).items()}


def record(case) -> dict:
    """{"forward": [...], "backward": [...]}: the entry points called inside the engine's forward and
    backward of one model call (and one loss.backward() when training), in order."""
    from gnn_local_stress import losses
    from gnn_local_stress.models import EncodeProcessDecode
    from pdg.lib import lib
    kind, steps, training, attrs = CASES[case]
    batch, stats = _batch(kind)
    torch.manual_seed(69)
    model = EncodeProcessDecode(input_edges_features_size=1, message_passing_steps=steps, latent_size=128,
                                input_nodes_features_size=6, output_nodes_features_size=3,
                                **{k: torch.as_tensor(v).float() for k, v in stats.items()}).to("cuda")
    eng = model._engine_for(batch.pos.device)
    for k, v in attrs.items():
        assert hasattr(eng, k)
        setattr(eng, k, v)
    out = {"forward": [], "backward": []}

    def hooked(phase, fn):
        def run(*a, **k):
            before, lib.hook = lib.hook, out[phase].append
            try:
                return fn(*a, **k)
            finally:
                lib.hook = before
        return run

    eng.forward, eng.backward = hooked("forward", eng.forward), hooked("backward", eng.backward)
    if not training:
        with torch.no_grad():
            model(batch, scale_output=True)
    else:
        pred = model(batch, scale_output=False).local_stress
        gt = (batch.local_stress - model.mean_local_stress) / model.std_local_stress
        total, _, _ = losses.batch_loss(pred, batch, gt, divergence=True, divergence_penalty=10.0)
        total.backward()
    torch.cuda.synchronize()
    assert lib.hook is None
    return out


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def test_golden_has_exactly_these_cases():
    assert set(json.loads(GOLDEN.read_text())) == set(CASES)


@pytest.mark.parametrize("case", CASES)
def test_engine_launch_sequence_matches_golden(case):
    want = json.loads(GOLDEN.read_text())[case]
    got = record(case)
    assert got["forward"] and (got["backward"] or not CASES[case][2])
    for phase in ("forward", "backward"):
        assert got[phase] == want[phase], (case, phase)
