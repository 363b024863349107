"""Generate tests/golden/engine_launches.json: per case of tests/test_gpu_engine_launches.py, the ordered
names of the C-ABI entry points the engine's forward and backward call.

Run on a machine with an MI355X, from the repository root, after building the library:

    python tests/golden/make_engine_launches.py

It uses only pdg.lib.lib.hook, the model's ``_engine_for`` and the engine's variant attributes (through
the test module's ``record``), so it runs unchanged on the engine as it was before a restructuring: record
there, restructure, and the test must pass against the file as recorded.  Re-record only when the launch
sequence is meant to change.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
for p in (HERE.parent, ROOT / "p-div-gnn_amd", ROOT):
    sys.path.insert(0, str(p))


def main():
    import test_gpu_engine_launches as T
    rec = {}
    for case in T.CASES:
        rec[case] = T.record(case)
        print(case, len(rec[case]["forward"]), "forward,", len(rec[case]["backward"]), "backward calls")
    T.GOLDEN.write_text(json.dumps(rec, indent=0, sort_keys=True) + "\n")
    print(T.GOLDEN.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
