"""bench.py's command line: a plain run times --config only (the CPU baselines, the sub-results and the
published sweep are behind --full), and --dump-outputs writes the last timed step's results as float32
.npy files."""
import numpy as np
import torch

import bench


def test_plain_run_is_the_main_line_only():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None
    assert bench.parse_args(["--full"]).full is True
    # the options that take parts of --full away are still accepted on their own
    a = bench.parse_args(["--no-cpu-baseline", "--no-extras", "--no-sweep", "--dump-outputs", "d"])
    assert a.full is False and a.dump_outputs == "d"


class _Trainer:
    flat_g = torch.arange(5, dtype=torch.float32)
    flat_p = torch.arange(5, dtype=torch.float32) * 2


def test_training_step_outputs_are_losses_flag_gradient_and_parameters(tmp_path):
    out = {"nmse": torch.tensor(0.25), "total": torch.tensor(0.5), "skipped": torch.zeros(1, dtype=torch.int32)}
    arrays = bench.last_step_outputs(out, _Trainer, infer=False)
    assert sorted(arrays) == ["grad", "nmse", "params", "skipped", "total"]
    bench.write_outputs(str(tmp_path / "o"), arrays, rank=0, world=1)
    got = {p.stem: np.load(p) for p in (tmp_path / "o").glob("*.npy")}
    assert sorted(got) == sorted(arrays)
    assert all(v.dtype == np.float32 for v in got.values())
    assert got["total"] == 0.5 and got["skipped"].tolist() == [0.0]
    assert got["grad"].tolist() == [0, 1, 2, 3, 4] and got["params"].tolist() == [0, 2, 4, 6, 8]


def test_inference_outputs_are_the_stress_field(tmp_path):
    y = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    arrays = bench.last_step_outputs({"total": y.abs().mean(), "local_stress": y}, None, infer=True)
    assert sorted(arrays) == ["local_stress", "total"]
    bench.write_outputs(str(tmp_path), arrays, rank=1, world=2)
    assert np.load(tmp_path / "local_stress_rank1.npy").tolist() == y.tolist()
