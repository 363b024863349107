"""CPU-side checks of the FEM C ABI (pdg_fem_elements, pdg_fem_solve_scratch_bytes, pdg_fem_solve and pdg_fem_stress
in csrc/pdg_fem.hip): declared, bound with matching pointer / integer kinds, exported, bad arguments refused before any
HIP call; the conventions the header states; and the Python layer's own refusals."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "pdivgnn.h"
SOURCE = ROOT / "p-div-gnn_amd" / "csrc" / "pdg_fem.hip"
NAMES = ("pdg_fem_elements", "pdg_fem_solve_scratch_bytes", "pdg_fem_solve", "pdg_fem_stress")
CALLS = ("pdg_fem_elements", "pdg_fem_solve", "pdg_fem_stress")


def _params(name):
    """(C type, name) of every parameter of `name` in include/pdivgnn.h."""
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    m = re.search(rf"\b(?:int|long)\s+{name}\s*\(([^)]*)\)\s*;", text, re.S)
    assert m, f"{name} is not declared in include/pdivgnn.h"
    out = []
    for a in m.group(1).split(","):
        nm = re.findall(r"\w+", a)[-1]
        out.append((a.strip()[:a.strip().rfind(nm)].strip(), nm))
    return out


def test_header_and_signatures_hold_the_fem_calls():
    from pdg.lib import _RESTYPES, SIGNATURES
    kinds = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double}
    for name in NAMES:
        params = _params(name)
        assert name in SIGNATURES, name
        assert len(SIGNATURES[name]) == len(params), name
        for ctype, (ctext, nm) in zip(SIGNATURES[name], params):
            assert ctype is (ctypes.c_void_p if "*" in ctext else kinds[ctext]), (name, nm)
    assert _RESTYPES["pdg_fem_solve_scratch_bytes"] is ctypes.c_long
    assert not any(n in _RESTYPES for n in CALLS)
    assert [n for _, n in _params("pdg_fem_solve_scratch_bytes")] == ["n_nodes", "n_cases"]
    assert [n for _, n in _params("pdg_fem_elements")] == [
        "n_nodes", "points", "dim", "n_faces", "verts", "elem", "status", "stream"]
    assert [n for _, n in _params("pdg_fem_solve")] == [
        "n_graphs", "n_cases", "ptr", "n_nodes", "points", "dim", "n_faces", "verts", "rverts", "rep", "item_rowptr",
        "item", "elem", "strains", "young", "poisson", "rtol", "max_iter", "ut", "table", "scratch", "scratch_bytes",
        "stream"]
    assert [n for _, n in _params("pdg_fem_stress")] == [
        "n_graphs", "n_cases", "ptr", "fptr", "n_nodes", "points", "dim", "n_faces", "verts", "rep", "item_rowptr",
        "item", "elem", "strains", "ut", "young", "poisson", "nodal", "stress", "strain", "sums", "stream"]
    k = dict((n, t) for t, n in _params("pdg_fem_solve"))
    assert k["ut"] == k["table"] == "double*" and k["elem"] == k["strains"] == "const double*"
    assert k["points"] == "const float*" and k["rep"] == k["item"] == k["verts"] == "const int*"
    assert k["rtol"] == k["young"] == k["poisson"] == "double" and k["scratch_bytes"] == "long"
    k = dict((n, t) for t, n in _params("pdg_fem_stress"))
    assert k["stress"] == k["strain"] == "float*" and k["sums"] == "double*" and k["ut"] == "const double*"


def test_header_states_the_conventions():
    text = " ".join(HEADER.read_text().replace("\n *", "\n").split())   # the comment's line prefix is not text
    for phrase in ("|b|_2 <= 1e-12 |b_abs|_2", "the right-hand side is rounding noise", "status TRIVIAL",
                   "0 CONVERGED, 1 TRIVIAL, 2 MAX_ITER, 3 BREAKDOWN", "clamped to [0, 100000]",
                   "alone and inside any batch", "it can be captured", "no float atomics", "no memset",
                   "the true final relative residual", "zero mean over the representatives",
                   "no input makes the workgroup spin", "NaN table row", "the node's own corners (not its images')",
                   "rows of image nodes are empty", "each as written there, contraction off",
                   "One persistent workgroup of 1024 threads per (graph, load case)"):
        assert phrase in text, phrase


def test_library_exports_the_fem_calls_and_the_source_is_built():
    import build as pdg_build
    from pdg.lib import lib, source_hash
    dll = lib.load()
    for name in NAMES:
        assert hasattr(dll, name), name
    assert SOURCE.is_file()
    assert pdg_build.source_hash() == source_hash() == lib.pdg_source_hash().decode()


def test_scratch_size():
    from pdg.lib import lib
    f = lib.pdg_fem_solve_scratch_bytes
    for bad in ((0, 1), (-1, 1), (10, 0), (10, -3), (10, 65), (2 ** 29, 1), (2 ** 31 - 1, 1)):
        assert f(*bad) < 0, bad
    # x, r, p, A p, 1 / diag: 2 doubles a node each, per load case
    assert f(1, 1) >= 80 and f(5041 * 8, 3) >= 80 * 5041 * 8 * 3 and f(100, 64) >= 80 * 100 * 64
    assert f(2 ** 29 - 1, 1) >= 80 * (2 ** 29 - 1)


def _args(name, null=(), **vals):
    """Arguments of `name`: every pointer a distinct 16-byte-aligned fake address 2^32 apart (never dereferenced: the
    checks run on the host before any HIP call) except those in `null` and the stream."""
    from pdg.lib import lib
    v = {"n_graphs": 3, "n_cases": 3, "n_nodes": 100, "n_faces": 150, "dim": 2, "young": 1e5, "poisson": 0.3,
         "rtol": 1e-10, "max_iter": 10, "nodal": 0, "scratch_bytes": lib.pdg_fem_solve_scratch_bytes(100, 3)}
    v.update(vals)
    out = []
    for i, (ctext, nm) in enumerate(_params(name)):
        if "*" in ctext:
            out.append(None if nm in null or nm == "stream" else v.get(nm, 0x100000000 * (i + 1)))
        else:
            out.append(v[nm])
    return out


def test_fem_calls_refuse_bad_arguments():
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-side argument checks only: never called with fake pointers where a GPU is present")
    from pdg.lib import PdgError, lib
    for name in CALLS:
        fn = getattr(lib, name)
        pointers = [nm for ctext, nm in _params(name) if "*" in ctext and nm != "stream"]
        for nm in pointers:                      # every pointer is required
            with pytest.raises(PdgError, match="null argument"):
                fn(*_args(name, null=(nm,)))
        sizes = [{"n_nodes": 0}, {"n_nodes": -5}, {"n_nodes": 2 ** 29}, {"n_faces": 0}, {"n_faces": 2 ** 29},
                 {"dim": 1}, {"dim": 4}]
        if name != "pdg_fem_elements":
            sizes += [{"n_graphs": 0}, {"n_graphs": -1}, {"n_graphs": 65536}, {"n_cases": 0}, {"n_cases": 65}]
        for bad in sizes:
            with pytest.raises(PdgError, match="bad sizes"):
                fn(*_args(name, **bad))
            with pytest.raises(PdgError, match="bad sizes"):   # the sizes are refused first, whatever else is wrong
                fn(*_args(name, null=("points",), young=-1.0, **bad))
    for name in ("pdg_fem_solve", "pdg_fem_stress"):
        fn = getattr(lib, name)
        for bad in ({"young": 0.0}, {"young": -1.0}, {"young": float("inf")}, {"young": float("nan")},
                    {"poisson": 0.5}, {"poisson": -1.0}, {"poisson": float("nan")}):
            with pytest.raises(PdgError, match="young must be finite and > 0, poisson in"):
                fn(*_args(name, **bad))
    for bad in (0.0, -1e-5, 1.0, float("nan"), float("inf")):
        with pytest.raises(PdgError, match="rtol"):
            lib.pdg_fem_solve(*_args("pdg_fem_solve", rtol=bad))
    need = lib.pdg_fem_solve_scratch_bytes(100, 3)
    for short in (need - 1, 0, -1):
        with pytest.raises(PdgError, match="scratch too small"):
            lib.pdg_fem_solve(*_args("pdg_fem_solve", scratch_bytes=short))
    for bad in (-1, 2):
        with pytest.raises(PdgError, match="nodal"):
            lib.pdg_fem_stress(*_args("pdg_fem_stress", nodal=bad))


def test_the_kernels_follow_the_per_graph_conventions():
    """Kernel launches and nothing else on the stream; no float atomics; contraction off; the iteration cap and the
    noise rule are in the source as the header states them."""
    code = re.sub(r"//[^\n]*", "", SOURCE.read_text())
    assert code.count("hipLaunchKernelGGL") == 5       # clear + elements, solve, nodal + sums
    for banned in ("hipMemset", "hipMemcpy", "hipMalloc", "hipStreamSynchronize", "hipDeviceSynchronize",
                   "atomicAdd", "atomicExch", "atomicCAS"):
        assert banned not in code, banned
    assert set(re.findall(r"\batomic\w+", code)) == {"atomicOr"}        # the element table's status bits only
    solve = code[code.index("void fem_solve_kernel"):code.index("element_fields")]
    assert "atomic" not in solve
    assert code.count("fp contract(off)") == 4
    assert "FEM_MAX_ITER = 100000" in code and "FEM_NOISE = 1e-12" in code and "FEM_T = 1024" in code
    assert "max_iter > FEM_MAX_ITER ? FEM_MAX_ITER" in code


def test_python_layer_refusals():
    import torch
    from gnn_local_stress import fem
    from pdg import meshgen
    s = meshgen.hole_plate(5)
    pts, fcs = torch.from_numpy(s.pos), torch.from_numpy(s.faces)
    for call in (lambda: fem.FemPlan.from_mesh(pts, fcs), lambda: fem.solve_cell(pts, fcs, strain=(1.0, 0.0, 0.0)),
                 lambda: fem.effective_stiffness(pts, fcs), lambda: fem.localisation_tensor(pts, fcs),
                 lambda: fem.fem_targets(pts, fcs, (1.0, 0.0, 0.0)),
                 lambda: fem.write_sample("unused", 0, pts, fcs, (1.0, 0.0, 0.0))):
        with pytest.raises(RuntimeError, match="HIP"):
            call()
    for call in (lambda: fem.FemPlan.from_mesh(pts, fcs, cells="quad"),
                 lambda: fem.solve_cell(pts, fcs, strain=(1.0, 0.0, 0.0), cells="quad"),
                 lambda: fem.effective_stiffness(pts, fcs, cells="any")):
        with pytest.raises(ValueError, match="quads are out of scope"):
            call()
    with pytest.raises(ValueError, match="exactly one of"):
        fem.solve_cell(pts, fcs)
    with pytest.raises(ValueError, match="exactly one of"):
        fem.solve_cell(pts, fcs, strain=(1.0, 0.0, 0.0), stress=(1.0, 0.0, 0.0))
    for bad in (0.5, -1.0, 0.7, float("nan")):
        with pytest.raises(ValueError, match="poisson"):
            fem.stiffness(poisson=bad)
    for bad in (0.0, -3.0, float("inf")):
        with pytest.raises(ValueError, match="young"):
            fem.stiffness(young=bad)
    c = fem.stiffness()
    assert abs(float(c[0, 0]) - 1e5 / 0.91) < 1e-9 and float(c[2, 2]) == float(c[0, 0]) * 0.7 / 2.0
    assert fem.STATUS == ("CONVERGED", "TRIVIAL", "MAX_ITER", "BREAKDOWN")
    assert fem.COLUMNS == ("iterations", "rhs_norm", "residual", "status")
    assert (fem.YOUNG, fem.POISSON, fem.MAX_ITER_CAP) == (1e5, 0.3, 100000)
