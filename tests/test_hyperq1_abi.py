"""CPU-side checks of the Q1 hyperelastic C ABI (pdg_hyperq1_solve_scratch_bytes, pdg_hyperq1_solve and
pdg_hyperq1_stress in csrc/pdg_hyperq1.hip): declared argument for argument as the triangle calls, bound with matching
pointer / integer kinds, exported, bad arguments refused before any HIP call with the triangle calls' messages in their
order; the scratch size; the source conventions; and the Python layer's own refusals
(gnn_local_stress/hyperelastic_q1.py)."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "pdivgnn.h"
CSRC = ROOT / "p-div-gnn_amd" / "csrc"
SOURCE = CSRC / "pdg_hyperq1.hip"
NAMES = ("pdg_hyperq1_solve_scratch_bytes", "pdg_hyperq1_solve", "pdg_hyperq1_stress")
CALLS = ("pdg_hyperq1_solve", "pdg_hyperq1_stress")


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


def test_header_and_signatures_hold_the_q1_hyper_calls():
    from pdg.lib import _RESTYPES, SIGNATURES
    kinds = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double}
    for name in NAMES:
        params = _params(name)
        assert name in SIGNATURES, name
        assert len(SIGNATURES[name]) == len(params), name
        for ctype, (ctext, nm) in zip(SIGNATURES[name], params):
            assert ctype is (ctypes.c_void_p if "*" in ctext else kinds[ctext]), (name, nm)
        # argument for argument the triangle call: the same types and names in the same order
        assert params == _params(name.replace("pdg_hyperq1_", "pdg_hyper_")), name
        assert SIGNATURES[name] == SIGNATURES[name.replace("pdg_hyperq1_", "pdg_hyper_")], name
    assert _RESTYPES["pdg_hyperq1_solve_scratch_bytes"] is ctypes.c_long
    assert not any(n in _RESTYPES for n in CALLS)
    text = HEADER.read_text()
    assert text.index("Q1 FEM targets */") < text.index("int pdg_femq1_stress") \
        < text.index("Q1 hyperelastic FEM targets */") < text.index("long pdg_hyperq1_solve_scratch_bytes")


def test_header_states_the_conventions():
    text = HEADER.read_text()
    text = " ".join(text[text.index("Q1 hyperelastic FEM targets */"):].replace("\n *", "\n").split())
    for phrase in ("elem (n_faces, 36) fp64", "4 face + corner", "F_g = Fbar + sum_k ut_k (x) grad N_k(g)",
                   "w_g = |det J_g|", "Phi = sum_f sum_g w_g W(F_g)",
                   "their order and their messages are those of pdg_hyper_solve and pdg_hyper_stress",
                   "One persistent workgroup of 512 threads per (graph, load case)", "t + 512",
                   "nothing may spill inside the solver's loops", "in ascending item order", "no scatter",
                   "no float atomics", "no memset", "alone and inside any batch", "it can be captured",
                   "word for word", "|r|_2 <= rtol |f_abs|_2", "no input makes the workgroup spin",
                   "any of its four J_g is <= 0 or not finite", "56 doubles a face",
                   "seven 2 n_nodes fp64 vectors and 56 doubles per face",
                   "the 2 x 2 rule integrates grad N det J exactly", "the node's own corners (not its images')",
                   "the Gauss point nearest that corner", "deformed weight w_g J_g", "Two kernel launches"):
        assert phrase in text, phrase


def test_library_exports_the_q1_hyper_calls_and_the_source_is_built():
    import build as pdg_build
    from pdg.lib import lib, source_hash
    dll = lib.load()
    for name in NAMES:
        assert hasattr(dll, name), name
    assert SOURCE.is_file()
    assert pdg_build.source_hash() == source_hash() == lib.pdg_source_hash().decode()


def test_scratch_size():
    from pdg.lib import lib
    f = lib.pdg_hyperq1_solve_scratch_bytes
    for bad in ((0, 1, 1), (-1, 1, 1), (10, 0, 1), (10, -2, 1), (10, 10, 0), (10, 10, 65), (2 ** 29, 1, 1),
                (1, 2 ** 29, 1)):
        assert f(*bad) < 0 and lib.pdg_hyper_solve_scratch_bytes(*bad) < 0, bad      # the same ranges are refused
    # seven 2 n vectors and 4 x 14 = 56 doubles a face, per load case
    for n, nf, cases in ((1, 1, 1), (1208, 1104, 3), (100, 150, 64), (2 ** 29 - 1, 2 ** 29 - 1, 1),
                         (2 ** 29 - 1, 2 ** 29 - 1, 64)):
        need = (7 * 2 * n + 56 * nf) * 8 * cases
        assert need <= f(n, nf, cases) < need + 256 and f(n, nf, cases) % 256 == 0


def _args(name, null=(), **vals):
    """Arguments of `name`: every pointer a distinct 16-byte-aligned fake address 2^32 apart (never dereferenced: the
    checks run on the host before any HIP call) except those in `null` and the stream."""
    from pdg.lib import lib
    v = {"n_graphs": 3, "n_cases": 3, "n_nodes": 100, "n_faces": 150, "dim": 2, "mu": 3.0, "kappa": 10.0,
         "volumetric": 0, "rtol": 1e-10, "n_steps": 4, "max_newton": 5, "eta": 1e-4, "max_pcg": 10, "nodal": 0,
         "scratch_bytes": lib.pdg_hyperq1_solve_scratch_bytes(100, 150, 3)}
    v.update(vals)
    out = []
    for i, (ctext, nm) in enumerate(_params(name)):
        if "*" in ctext:
            out.append(None if nm in null or nm == "stream" else v.get(nm, 0x100000000 * (i + 1)))
        else:
            out.append(v[nm])
    return out


def test_q1_hyper_calls_refuse_bad_arguments():
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-side argument checks only: never called with fake pointers where a GPU is present")
    from pdg.lib import PdgError, lib
    for name in CALLS:
        fn = getattr(lib, name)
        for nm in [nm for ctext, nm in _params(name) if "*" in ctext and nm != "stream"]:   # every pointer is required
            with pytest.raises(PdgError, match=f"{name}: null argument"):
                fn(*_args(name, null=(nm,)))
        sizes = [{"n_nodes": 0}, {"n_nodes": -5}, {"n_nodes": 2 ** 29}, {"n_faces": 0}, {"n_faces": 2 ** 29},
                 {"n_graphs": 0}, {"n_graphs": -1}, {"n_graphs": 65536}, {"n_cases": 0}, {"n_cases": 65}]
        if name == "pdg_hyperq1_stress":
            sizes += [{"dim": 1}, {"dim": 4}]
        for bad in sizes:
            with pytest.raises(PdgError, match=f"{name}: bad sizes"):
                fn(*_args(name, **bad))
            with pytest.raises(PdgError, match="bad sizes"):   # the sizes are refused first, whatever else is wrong
                fn(*_args(name, null=("ptr",), mu=-1.0, **bad))
        with pytest.raises(PdgError, match="null argument"):   # a null pointer before the material
            fn(*_args(name, null=("elem",), mu=-1.0))
        for bad in ({"mu": 0.0}, {"mu": -1.0}, {"mu": float("inf")}, {"mu": float("nan")}, {"kappa": 0.0},
                    {"kappa": float("nan")}, {"volumetric": 2}, {"volumetric": -1}):
            with pytest.raises(PdgError, match="mu and kappa must be finite and > 0, volumetric 0"):
                fn(*_args(name, **bad))
    solve = lib.pdg_hyperq1_solve
    for bad in ({"rtol": 0.0}, {"rtol": 1.0}, {"rtol": float("nan")}, {"eta": 0.0}, {"eta": 1.0}, {"eta": -1e-3}):
        with pytest.raises(PdgError, match="rtol and eta must be in"):
            solve(*_args("pdg_hyperq1_solve", **bad))
    for bad in (0, -1, 10001):
        with pytest.raises(PdgError, match=r"n_steps must be in \[1, 10000\]"):
            solve(*_args("pdg_hyperq1_solve", n_steps=bad))
    need = lib.pdg_hyperq1_solve_scratch_bytes(100, 150, 3)
    for short in (need - 1, 0, -1, lib.pdg_hyper_solve_scratch_bytes(100, 150, 3)):   # the triangle size is too small
        with pytest.raises(PdgError, match="scratch too small"):
            solve(*_args("pdg_hyperq1_solve", scratch_bytes=short))
    # the order: the material, then rtol and eta, then n_steps, then the scratch
    with pytest.raises(PdgError, match="mu and kappa"):
        solve(*_args("pdg_hyperq1_solve", mu=0.0, rtol=2.0, n_steps=0, scratch_bytes=0))
    with pytest.raises(PdgError, match="rtol and eta"):
        solve(*_args("pdg_hyperq1_solve", rtol=2.0, n_steps=0, scratch_bytes=0))
    with pytest.raises(PdgError, match="n_steps"):
        solve(*_args("pdg_hyperq1_solve", n_steps=0, scratch_bytes=0))
    for bad in (-1, 2):
        with pytest.raises(PdgError, match="nodal"):
            lib.pdg_hyperq1_stress(*_args("pdg_hyperq1_stress", nodal=bad))
    with pytest.raises(PdgError, match="mu and kappa"):          # the material before nodal
        lib.pdg_hyperq1_stress(*_args("pdg_hyperq1_stress", kappa=0.0, nodal=5))


def test_the_refusals_are_the_triangle_calls_word_for_word():
    """The host checks of the two files differ in the calls' names alone (and in what the nodal weights are called)."""
    def checks(path, prefix):
        code = path.read_text()
        code = code[code.index('extern "C" int'):]
        return [re.sub(r"\s+", " ", m).replace(prefix, "pdg_X_").replace("HQ_", "HY_")
                for m in re.findall(r"PDG_CHECK_ARG\((.*?)\);", code, re.S)]
    q1, tri = checks(SOURCE, "pdg_hyperq1_"), checks(CSRC / "pdg_hyper.hip", "pdg_hyper_")
    assert len(q1) == len(tri) == 10
    assert [c.replace("deformed weights", "deformed-area weights") for c in q1] == tri


def test_the_kernels_follow_the_per_graph_conventions():
    """Kernel launches and nothing else on the stream; no atomics at all; contraction off for the whole file and in
    the shared law; the caps are in the source as the header states them; the Gauss-point loops stay rolled; the law
    and the mesh helpers are shared, not restated; the solver is the triangle solver's text."""
    code = re.sub(r"//[^\n]*", "", SOURCE.read_text())
    assert code.count("hipLaunchKernelGGL") == 3       # solve, nodal + sums
    for banned in ("hipMemset", "hipMemcpy", "hipMalloc", "hipStreamSynchronize", "hipDeviceSynchronize", "atomic"):
        assert banned not in code, banned
    assert code.index("#pragma clang fp contract(off)") < code.index("namespace {")
    for phrase in ("HQ_T = 512", "HQ_ES = 4 * HQ_GS", "HQ_GS = 14", "HQ_VECS = 7", "HQ_HALVINGS = 10",
                   "HQ_ARMIJO = 1e-4", "HQ_MAX_STEPS = 10000", "HQ_MAX_NEWTON = 1000", "HQ_MAX_PCG = 100000",
                   "HQ_PHI_NOISE = 32.0 * 2.220446049250313e-16",
                   "__launch_bounds__(HQ_T) void hyperq1_solve_kernel", '#include "pdg_femmesh.hpp"',
                   '#include "pdg_neohooke.hpp"', '#include "pdg_reduce.hpp"', "row_range4(", "item_of4(",
                   "block_sum_k_wave_major("):
        assert phrase in code, phrase
    assert code.count("#pragma unroll 1") >= 4 and code.count("for (int g = 0; g < 4; ++g)") == 3
    law = (CSRC / "pdg_neohooke.hpp").read_text()
    assert "#pragma clang fp contract(off)" in law
    tri = re.sub(r"//[^\n]*", "", (CSRC / "pdg_hyper.hip").read_text())
    for shared in ("struct Law", "double jm23(", "double trace1(", "void energy(", "void stress_tangent(",
                   "int face_state(", "double inverse_diag("):
        assert shared in law and shared not in code and shared not in tri, shared
    assert "void kirchhoff(" in law and "void log_strain(" in law
    assert '#include "pdg_neohooke.hpp"' in tri and "struct Mesh" not in code

    def solver(text, kernel):
        text = text[text.index(f"void {kernel}("):]
        text = text[text.index("{"):text.index("\n}\n")]
        return re.sub(r"\s+", " ", text)
    q1 = solver(code, "hyperq1_solve_kernel").replace("HQ_", "HY_").replace("row_range4(", "row_range(")
    assert q1 == solver(tri, "hyper_solve_kernel")


def test_python_layer_refusals():
    import torch
    from gnn_local_stress import fem, fem_q1, hyperelastic as hy, hyperelastic_q1 as hq
    from pdg import meshgen
    s = meshgen.quad_hole_plate(5)
    pts, fcs = torch.from_numpy(s.pos), torch.from_numpy(s.faces)
    assert fcs.shape[1] == 4
    for call in (lambda: hq.solve_cell(pts, fcs, strain=(0.1, 0.0, 0.0)),
                 lambda: hq.solve_cell(pts, fcs, F=[[1.1, 0.0], [0.0, 1.0]]),
                 lambda: hq.hyper_targets(pts, fcs, (0.1, 0.0, 0.0)),
                 lambda: hq.write_sample("unused", 0, pts, fcs, (0.1, 0.0, 0.0)),
                 lambda: hq.solve_cells(fem_q1.FemPlan.empty("cpu"), pts[:0], torch.zeros(1, 1, 2, 2))):
        with pytest.raises(RuntimeError, match="HIP"):
            call()
    with pytest.raises(ValueError, match="exactly one of"):
        hq.solve_cell(pts, fcs)
    with pytest.raises(ValueError, match="exactly one of"):
        hq.solve_cell(pts, fcs, strain=(0.1, 0.0, 0.0), F=torch.eye(2))
    with pytest.raises(ValueError, match=r"fem_q1.FemPlan .*goes to gnn_local_stress.hyperelastic$"):
        hq.solve_cells(fem.FemPlan.empty("cpu"), pts[:0], torch.zeros(1, 1, 2, 2))
    assert hq.FemPlan is fem_q1.FemPlan and hq.element_table is fem_q1.element_table and hq.ELEM == 36
    assert hq.STATUS == fem.STATUS and (hq.CONVERGED, hq.MAX_ITER, hq.BREAKDOWN) == (0, 2, 3)
    assert hq.COLUMNS == ("load_steps", "newton_iterations", "pcg_iterations", "force_norm", "residual", "status")
    assert (hq.MU, hq.KAPPA, hq.VOLUMETRIC, hq.NODAL, hq.MAX_CASES) == (3.0, 10.0, ("log", "quadratic"),
                                                                        ("area", "count"), 64)
    assert hq.HyperFields is hy.HyperFields and hq.HyperSolution is hy.HyperSolution
    assert hq.deformation_gradient is hy.deformation_gradient
    assert "hyperelastic_q1" in hy.__doc__ and "Triangles only" in hy.__doc__
