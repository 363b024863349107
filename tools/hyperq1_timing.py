"""Wall time of the hyperelastic cell solve on quads (gnn_local_stress.hyperelastic_q1.solve_cells) beside the triangle
solve (gnn_local_stress.hyperelastic.solve_cells) on meshgen's hole plates of the same n: a record, not a criterion.

    python tools/hyperq1_timing.py --out profiles/hyperq1_timing.json --commit <the commit measured>

One load case, hyper_ref.LOADS[0] = (0.15, -0.10, 0.08) in 10 load steps at rtol 1e-10, the element table passed in
(nothing read back inside the timed region): solve + nodal + sums launches between two events on the current stream,
3 warm-up calls of each, then 15 repeats alternating the two solvers; median and [min, max] in milliseconds."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "p-div-gnn_amd"), str(ROOT / "tests")]

import torch  # noqa: E402

MESHES = ((9, 0.25), (13, 0.3), (37, 0.2), (71, 0.2))
LOAD = (0.15, -0.10, 0.08)
STEPS, WARMUP, REPEATS = 10, 3, 15


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="unknown")
    args = ap.parse_args()
    from gnn_local_stress import fem, fem_q1, hyperelastic as hy, hyperelastic_q1 as hq
    from pdg import meshgen
    F = hy.deformation_gradient(LOAD).reshape(1, 1, 2, 2).cuda()
    rows = []
    for n, r in MESHES:
        q, t = meshgen.quad_hole_plate(n, r, seed=3), meshgen.hole_plate(n, r, seed=3)
        qp, qf = torch.from_numpy(q.pos).cuda(), torch.from_numpy(q.faces).cuda()
        tp, tf = torch.from_numpy(t.pos).cuda(), torch.from_numpy(t.faces).cuda()
        qplan, tplan = fem_q1.FemPlan.from_mesh(qp, qf), fem.FemPlan.from_mesh(tp, tf)
        qel, tel = fem_q1.element_table(qplan, qp), fem.element_table(tplan, tp)
        calls = {"q1": lambda: hq.solve_cells(qplan, qp, F, n_steps=STEPS, elements=qel),
                 "p1": lambda: hy.solve_cells(tplan, tp, F, n_steps=STEPS, elements=tel)}
        for fn in calls.values():
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        last = {}
        for _ in range(REPEATS):
            for k, fn in calls.items():
                dt, last[k] = _timed(fn)
                ms[k].append(dt)
        row = {"n": n, "r": r}
        for k, plan in (("q1", qplan), ("p1", tplan)):
            table = last[k].table.cpu().numpy()[0, 0]
            row[k] = {"nodes": plan.n_nodes, "faces": plan.n_faces, "status": int(table[5]),
                      "newton_iterations": int(table[1]), "pcg_iterations": int(table[2]),
                      "ms_median": round(statistics.median(ms[k]), 4), "ms_min": round(min(ms[k]), 4),
                      "ms_max": round(max(ms[k]), 4)}
        print(row, flush=True)
        rows.append(row)
    doc = {"what": f"solve_cells (1 load case {LOAD}, {STEPS} load steps, rtol 1e-10, element table passed in): solve "
                   f"+ nodal + sums launches, device events, {REPEATS} alternating repeats after {WARMUP} warm-up "
                   "calls; q1 = hyperelastic_q1 on quad_hole_plate(n, r, seed=3) (512-thread workgroup), p1 = "
                   "hyperelastic on hole_plate(n, r, seed=3) (1024-thread workgroup)",
           "commit": args.commit, "device": torch.cuda.get_device_name(0), "rows": rows}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
