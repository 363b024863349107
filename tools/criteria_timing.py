"""Time the stress-criteria launches and gnn_local_stress.sensitivity.criterion_gradients on one MI355X
-> profiles/criteria_timing.json.

    python tools/criteria_timing.py [--out profiles/criteria_timing.json]

Two cases, each in a child process of its own under its own time limit (the run stops at the first that fails):
the config-2 batch (8 x 5,041-node periodic meshes) and the config-5 single 100,489-node mesh.  HIP events
(pdg.hiptimer), one warm run, median of 5:
* pdg_stress_criteria (with and without the fields) and pdg_stress_criteria_bwd beside pdg_eval_nmse on the same
  field, per criterion and, for the backward, per aggregate;
* criterion_gradients end to end beside a separate forward followed by graph_criterion_grad and input_gradients."""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for _p in (ROOT, ROOT / "p-div-gnn_amd"):
    sys.path.insert(0, str(_p))

REPS = 5
CASES = {"config2": (2, 300), "config5": (5, 420)}    # bench config, time limit of the child in seconds


def run_case(config: int) -> dict:
    import torch

    import bench
    from gnn_local_stress import criteria as C
    from gnn_local_stress.models import EncodeProcessDecode
    from gnn_local_stress.sensitivity import criterion_gradients, input_gradients
    from pdg import hiptimer
    from pdg.lib import lib, stream_handle
    from pdg.plan import plan_for

    dev = torch.device("cuda:0")
    cfg = bench.CONFIGS[config]
    batch, _ = bench.build_batch(cfg, 69, dev)
    torch.manual_seed(69)
    model = EncodeProcessDecode(input_edges_features_size=1, message_passing_steps=cfg["steps"], latent_size=128,
                                input_nodes_features_size=6, output_nodes_features_size=3,
                                **bench.dataset_stats(batch)).to(dev)
    ptr = plan_for(batch).ptr
    B, N = ptr.numel() - 1, int(batch.num_nodes)
    sigma = batch.local_stress.detach().float().contiguous()
    pred = (sigma + 0.05 * sigma.std() * torch.randn_like(sigma)).contiguous()
    rho = 4.0 / float(sigma.abs().max())
    s = stream_handle(dev)

    def timed(fn):
        a, b = hiptimer.Event(), hiptimer.Event()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def median(fn, scale=1.0):
        fn()
        torch.cuda.synchronize()
        return statistics.median(timed(fn) * scale for _ in range(REPS))

    table6 = torch.empty(B, 6, dtype=torch.float64, device=dev)
    table = torch.empty(B, 4, dtype=torch.float64, device=dev)
    argmax = torch.empty(B, dtype=torch.int32, device=dev)
    fields = torch.empty(N, 6, device=dev)
    g_sigma = torch.empty(N, 3, device=dev)
    us = {"pdg_eval_nmse": median(lambda: lib.pdg_eval_nmse(B, ptr.data_ptr(), sigma.data_ptr(), pred.data_ptr(),
                                                            table6.data_ptr(), None, None, None, s), 1e3)}
    for cid, crit in enumerate(C.CRITERIA):
        fwd = lambda f: lib.pdg_stress_criteria(B, ptr.data_ptr(), sigma.data_ptr(), None, cid, 8.0, rho,
                                                table.data_ptr(), argmax.data_ptr(), f, s)
        us[f"pdg_stress_criteria[{crit}]"] = median(lambda: fwd(None), 1e3)
        us[f"pdg_stress_criteria[{crit}, fields]"] = median(lambda: fwd(fields.data_ptr()), 1e3)
        for aid, agg in enumerate(C.AGGREGATES):
            us[f"pdg_stress_criteria_bwd[{crit}, {agg}]"] = median(
                lambda: lib.pdg_stress_criteria_bwd(B, ptr.data_ptr(), sigma.data_ptr(), None, cid, aid, 8.0, rho,
                                                    table.data_ptr(), argmax.data_ptr(), None, g_sigma.data_ptr(), s),
                1e3)
    res = {"graphs": B, "nodes": N, "edges": int(batch.num_edges), "steps": cfg["steps"], "kernels_us": us}
    res["forward_over_eval_nmse"] = max(us[f"pdg_stress_criteria[{c}]"] for c in C.CRITERIA) / us["pdg_eval_nmse"]

    def separate():
        y = model(batch).local_stress.detach()
        input_gradients(model, batch, C.graph_criterion_grad(y, batch, "von_mises", "pnorm", p=8.0))

    res["criterion_gradients_ms"] = median(lambda: criterion_gradients(model, batch, "von_mises", "pnorm", p=8.0))
    res["forward_then_grad_then_input_gradients_ms"] = median(separate)
    res["device"] = torch.cuda.get_device_name(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "criteria_timing.json"))
    ap.add_argument("--case", choices=sorted(CASES), help="run one case in this process and print its JSON")
    args = ap.parse_args()
    if args.case:
        print("RESULT " + json.dumps(run_case(CASES[args.case][0])))
        return 0
    out = {"method": f"HIP events, one warm run, median of {REPS}, one process per case", "cases": {}}
    for name, (_, limit) in CASES.items():
        try:
            r = subprocess.run([sys.executable, __file__, "--case", name], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {limit} s; stopping", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"{name}: exit {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        out["cases"][name] = json.loads(line[len("RESULT "):])
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
