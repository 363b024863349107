"""Time gnn_local_stress.sensitivity.input_gradients on the config-2 batch (8 x 5,041-node periodic meshes:
N = 40,328, E = 239,744) on one MI355X -> profiles/ingrad_timing.json.

    python tools/ingrad_timing.py [--out profiles/ingrad_timing.json]

HIP events (pdg.hiptimer), one warm run, median of 5, one process:
* input_gradients end to end beside a training forward + backward (model(batch) then backward of
  <grad_output, local_stress>) of the same model and batch;
* each new kernel beside the existing encoder-backward kernel that reads the same operands, bracketed inside
  the same backward (the engine's per-launch timing): pdg_edge_enc_gin / pdg_edge_enc_bwd and
  pdg_node_enc_gin / pdg_mlp2_bwd_coop; pdg_graph_colsum3 alone."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for _p in (ROOT, ROOT / "p-div-gnn_amd"):
    sys.path.insert(0, str(_p))

import torch  # noqa: E402

KERNELS = ("edge_enc_gin", "edge_enc_bwd", "node_enc_gin", "node_enc_bwd")
REPS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ingrad_timing.json"))
    args = ap.parse_args()
    import bench
    from gnn_local_stress.models import EncodeProcessDecode
    from gnn_local_stress.sensitivity import input_gradients
    from pdg import hiptimer
    from pdg.lib import lib, stream_handle

    dev = torch.device("cuda:0")
    cfg = bench.CONFIGS[2]
    batch, _ = bench.build_batch(cfg, 69, dev)
    torch.manual_seed(69)
    model = EncodeProcessDecode(input_edges_features_size=1, message_passing_steps=cfg["steps"], latent_size=128,
                                input_nodes_features_size=6, output_nodes_features_size=3,
                                **bench.dataset_stats(batch)).to(dev)
    gy = torch.randn(batch.num_nodes, 3, device=dev)
    eng = model._engine_for(dev)

    def timed(fn):
        a, b = hiptimer.Event(), hiptimer.Event()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def train_step():
        model.zero_grad(set_to_none=True)
        (model(batch).local_stress * gy).sum().backward()

    res = {}
    for name, fn in (("input_gradients", lambda: input_gradients(model, batch, gy)), ("train_fwd_bwd", train_step)):
        fn()
        torch.cuda.synchronize()
        res[name + "_ms"] = statistics.median(timed(fn) for _ in range(REPS))
    per = {k: [] for k in KERNELS}
    for i in range(REPS + 1):
        eng.timed = {k: [] for k in KERNELS}
        g = input_gradients(model, batch, gy)
        torch.cuda.synchronize()
        if i:
            for k in KERNELS:
                (a, b), = eng.timed[k]
                per[k].append(a.elapsed_time(b) * 1e3)
    eng.timed = None
    load = torch.empty(batch.ptr.numel() - 1, 3, device=dev)
    from pdg.plan import plan_for
    ptr = plan_for(batch).ptr
    col = lambda: lib.pdg_graph_colsum3(load.shape[0], ptr.data_ptr(), g.mean_stress.data_ptr(), load.data_ptr(),
                                        stream_handle(dev))
    col()
    torch.cuda.synchronize()
    res["kernels_us"] = {k: statistics.median(v) for k, v in per.items()}
    res["kernels_us"]["graph_colsum3"] = statistics.median(timed(col) * 1e3 for _ in range(REPS))
    k = res["kernels_us"]
    res["edge_enc_gin_over_edge_enc_bwd"] = k["edge_enc_gin"] / k["edge_enc_bwd"]
    res["node_enc_gin_over_node_enc_bwd"] = k["node_enc_gin"] / k["node_enc_bwd"]
    res.update(nodes=int(batch.num_nodes), edges=int(batch.num_edges), steps=cfg["steps"], reps=REPS,
               device=torch.cuda.get_device_name(0), method="HIP events, one warm run, median of 5, one process")
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
