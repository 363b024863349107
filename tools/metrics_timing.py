"""Time gnn_local_stress.metrics.batch_metrics against the numpy restatement (tests/metrics_ref.py).

    python tools/metrics_timing.py [--out profiles/metrics_timing.json]

Two batches: 512 graphs of about 1,000 nodes and 8 graphs of 5,041 nodes (hole plates with their P1
operators; a few distinct meshes repeated, the kernels do not care).  The device side is
batch_metrics (three launches and their output allocations) between HIP events, one warm run, the
median of 5; then each of the three launches alone, the same way.  The host side is the per-graph loop
of metrics_ref.graph_metrics over the same batch (numpy, at most 16 threads), wall clock, once.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "p-div-gnn_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))
for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(v, "16")

import numpy as np  # noqa: E402
import torch  # noqa: E402

MEAN, STD = 12.5, 37.25
CASES = (("512 x ~1,000 nodes", 512, 32, 0.1), ("8 x 5,041 nodes", 8, 71, 0.0))


def timed(fn, runs: int = 5) -> float:
    """Median milliseconds of fn() between HIP events, after one warm run."""
    from pdg.hiptimer import Event
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = Event(), Event()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def one_case(name: str, graphs: int, n: int, hole: float) -> dict:
    import metrics_ref as R
    from gnn_local_stress import metrics
    from pdg import graph, meshgen
    from pdg.plan import plan_for
    dev = torch.device("cuda:0")
    distinct = [meshgen.hole_plate(n, hole_radius=hole, seed=100 + i) for i in range(min(graphs, 8))]
    samples = [distinct[i % len(distinct)] for i in range(graphs)]
    batch = graph.Batch.from_data_list([graph.sample_to_data(s) for s in samples]).to(dev)
    plan = plan_for(batch)
    gt = batch.local_stress
    pred = gt + 4.0 * torch.randn(gt.shape, generator=torch.Generator().manual_seed(1)).to(dev)
    types = batch.nodes_types
    out = {"case": name, "graphs": graphs, "nodes": int(plan.n_nodes), "operator_entries": int(plan.a_col.numel())}
    out["batch_metrics_ms"] = timed(lambda: metrics.batch_metrics(pred, gt, batch, MEAN, STD))
    out["batch_metrics_fields_ms"] = timed(lambda: metrics.batch_metrics(pred, gt, batch, MEAN, STD, fields=True))
    out["pdg_eval_nmse_us"] = 1e3 * timed(lambda: metrics._eval_nmse(plan, gt, pred, False))
    out["pdg_eval_div_us"] = 1e3 * timed(lambda: metrics._eval_div(plan, types, pred, MEAN, STD, False, False))
    # the host loop on the same inputs
    ptr = batch.ptr.cpu().numpy()
    g64, p64 = gt.cpu().numpy(), pred.cpu().numpy()
    csrs = {id(s): R.coo_to_csr(s.num_nodes, s.op_div_rows, s.op_div_cols, s.op_div_vals) for s in distinct}
    t = time.perf_counter()
    host = [R.graph_metrics(g64[ptr[i]:ptr[i + 1]], p64[ptr[i]:ptr[i + 1]], csrs[id(s)], s.node_types, MEAN, STD)
            for i, s in enumerate(samples)]
    out["numpy_ms"] = 1e3 * (time.perf_counter() - t)
    m = metrics.batch_metrics(pred, gt, batch, MEAN, STD)
    want = np.array([h["nmse_table"][3] for h in host])
    out["nmse_max_rel_diff"] = float(np.max(np.abs(m["nmse"].cpu().numpy() - want) / want))
    out["speedup"] = out["numpy_ms"] / out["batch_metrics_ms"]
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "metrics_timing.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "host_threads": int(os.environ["OMP_NUM_THREADS"]),
           "cases": [one_case(*c) for c in CASES]}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
