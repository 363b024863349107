"""The register budget of csrc/pdg_hyper.hip, from the compiler's own resource remarks (what ``build.py --report``
collects): a 1024-thread workgroup leaves a thread 128 VGPRs, and a value spilled to scratch memory inside the
solver's loops is reloaded in every inner iteration.  ``own_index()`` and the LDS words of ``hyper_solve_kernel`` keep
it from happening; a toolchain that hoists differently would bring it back, and this test says so."""
import re
import subprocess

import build as pdg_build


def test_the_hyperelastic_kernels_spill_nothing_to_scratch(tmp_path):
    src = pdg_build.CSRC / "pdg_hyper.hip"
    cmd = [pdg_build.hipcc(), *pdg_build.FLAGS, "--cuda-device-only", "-c", str(src), "-o", str(tmp_path / "hyper.o"),
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    kernels = {k: v for k, v in rows.items() if re.search(r"hyper_(solve|nodal|sums)_kernel", k)}
    assert len(kernels) == 3
    for name, v in kernels.items():
        print(name[:48], v)
        assert v["VGPRs Spill"] == 0 and v["ScratchSize"] == 0 and v["VGPRs"] <= 128
