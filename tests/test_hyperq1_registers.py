"""The register budget of csrc/pdg_hyperq1.hip, from the compiler's own resource remarks (what ``build.py --report``
collects), as tests/test_hyper_registers.py for the triangle kernels: a value spilled to scratch memory inside the
solver's loops is reloaded in every inner iteration.  A workgroup of T threads leaves a thread 512 / (T / 256) VGPRs;
the solver runs 512 threads (four Gauss points a face do not fit the 128 registers of 1024), and ``own_index()``, the
rolled Gauss-point loops and the LDS words of ``hyperq1_solve_kernel`` keep it inside that budget; a toolchain that
hoists or unrolls differently would bring the spills back, and this test says so."""
import re
import subprocess

import build as pdg_build

SRC = pdg_build.CSRC / "pdg_hyperq1.hip"


def _threads():
    """The workgroup size of every kernel, from its __launch_bounds__ and the constants of the source."""
    code = SRC.read_text()
    consts = {k: int(v) for k, v in re.findall(r"constexpr int (\w+) = (\d+);", code)}
    out = {}
    for bound, name in re.findall(r"__launch_bounds__\((\w+)\) void (\w+)\(", code):
        out[name] = consts[bound] if bound in consts else int(bound)
    return out


def test_the_q1_hyperelastic_kernels_spill_nothing_to_scratch(tmp_path):
    cmd = [pdg_build.hipcc(), *pdg_build.FLAGS, "--cuda-device-only", "-c", str(SRC), "-o", str(tmp_path / "hq1.o"),
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
    threads = _threads()
    assert set(threads) == {"hyperq1_solve_kernel", "hyperq1_nodal_kernel", "hyperq1_sums_kernel"}
    assert threads["hyperq1_solve_kernel"] in (512, 1024)
    kernels = {}
    for mangled, v in rows.items():
        m = re.search(r"hyperq1_(solve|nodal|sums)_kernel", mangled)
        if m:
            kernels[m.group(0)] = v
    assert set(kernels) == set(threads)
    for name, v in kernels.items():
        budget = 512 // max(threads[name] // 256, 1)
        print(name, f"{threads[name]} threads, budget {budget}", v)
        assert v["VGPRs Spill"] == 0 and v["ScratchSize"] == 0 and v["VGPRs"] <= budget
