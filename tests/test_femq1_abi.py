"""CPU-side checks of the Q1 FEM C ABI (pdg_femq1_elements, pdg_femq1_solve_scratch_bytes, pdg_femq1_solve and
pdg_femq1_stress in csrc/pdg_femq1.hip): declared argument for argument as the triangle calls, bound with matching
pointer / integer kinds, exported, bad arguments refused before any HIP call with the triangle calls' messages in
their order; the source conventions; and the Python layer's own refusals (gnn_local_stress/fem_q1.py)."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "pdivgnn.h"
SOURCE = ROOT / "p-div-gnn_amd" / "csrc" / "pdg_femq1.hip"
NAMES = ("pdg_femq1_elements", "pdg_femq1_solve_scratch_bytes", "pdg_femq1_solve", "pdg_femq1_stress")
CALLS = ("pdg_femq1_elements", "pdg_femq1_solve", "pdg_femq1_stress")


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


def test_header_and_signatures_hold_the_q1_calls():
    from pdg.lib import _RESTYPES, SIGNATURES
    kinds = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double}
    for name in NAMES:
        params = _params(name)
        assert name in SIGNATURES, name
        assert len(SIGNATURES[name]) == len(params), name
        for ctype, (ctext, nm) in zip(SIGNATURES[name], params):
            assert ctype is (ctypes.c_void_p if "*" in ctext else kinds[ctext]), (name, nm)
        # argument for argument the triangle call: the same types and names in the same order
        assert params == _params(name.replace("pdg_femq1_", "pdg_fem_")), name
        assert SIGNATURES[name] == SIGNATURES[name.replace("pdg_femq1_", "pdg_fem_")], name
    assert _RESTYPES["pdg_femq1_solve_scratch_bytes"] is ctypes.c_long
    assert not any(n in _RESTYPES for n in CALLS)
    text = HEADER.read_text()
    assert text.index("FEM targets */") < text.index("Hyperelastic FEM targets */") < text.index("Q1 FEM targets */") \
        < text.index("int pdg_femq1_elements")


def test_header_states_the_conventions():
    text = HEADER.read_text()
    text = " ".join(text[text.index("Q1 FEM targets */"):].replace("\n *", "\n").split())
    for phrase in ("elem (n_faces, 36) fp64", "det J, dN/dx[4], dN/dy[4]", "the one nearest corner g",
                   "not all strictly of one sign", "a clockwise quad (all four det J < 0) is accepted",
                   "4 face + corner", "one persistent workgroup of 1024 threads per (graph, load case)",
                   "in ascending order", "no scatter", "80 bytes per node and case", "No float atomics",
                   "no memset", "alone and inside any batch", "it can be captured",
                   "the node's own corners (not its images')", "the Gauss point nearest that corner",
                   "clamp of max_iter to [0, 100000]", "their order and their messages are those of the triangle"):
        assert phrase in text, phrase


def test_library_exports_the_q1_calls_and_the_source_is_built():
    import build as pdg_build
    from pdg.lib import lib, source_hash
    dll = lib.load()
    for name in NAMES:
        assert hasattr(dll, name), name
    assert SOURCE.is_file()
    assert pdg_build.source_hash() == source_hash() == lib.pdg_source_hash().decode()


def test_scratch_size():
    from pdg.lib import lib
    f = lib.pdg_femq1_solve_scratch_bytes
    for bad in ((0, 1), (-1, 1), (10, 0), (10, -3), (10, 65), (2 ** 29, 1), (2 ** 31 - 1, 1)):
        assert f(*bad) < 0, bad
    # x, r, p, A p, 1 / diag: 2 doubles a node each, per load case; the triangle solver's rule
    for sizes in ((1, 1), (5041 * 8, 3), (100, 64), (2 ** 29 - 1, 1), (1208, 3)):
        assert f(*sizes) >= 80 * sizes[0] * sizes[1] and f(*sizes) % 256 == 0
        assert f(*sizes) == lib.pdg_fem_solve_scratch_bytes(*sizes)


def _args(name, null=(), **vals):
    """Arguments of `name`: every pointer a distinct 16-byte-aligned fake address 2^32 apart (never dereferenced: the
    checks run on the host before any HIP call) except those in `null` and the stream."""
    from pdg.lib import lib
    v = {"n_graphs": 3, "n_cases": 3, "n_nodes": 100, "n_faces": 150, "dim": 2, "young": 1e5, "poisson": 0.3,
         "rtol": 1e-10, "max_iter": 10, "nodal": 0, "scratch_bytes": lib.pdg_femq1_solve_scratch_bytes(100, 3)}
    v.update(vals)
    out = []
    for i, (ctext, nm) in enumerate(_params(name)):
        if "*" in ctext:
            out.append(None if nm in null or nm == "stream" else v.get(nm, 0x100000000 * (i + 1)))
        else:
            out.append(v[nm])
    return out


def test_q1_calls_refuse_bad_arguments():
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-side argument checks only: never called with fake pointers where a GPU is present")
    from pdg.lib import PdgError, lib
    for name in CALLS:
        fn = getattr(lib, name)
        pointers = [nm for ctext, nm in _params(name) if "*" in ctext and nm != "stream"]
        for nm in pointers:                      # every pointer is required
            with pytest.raises(PdgError, match=f"{name}: null argument"):
                fn(*_args(name, null=(nm,)))
        sizes = [{"n_nodes": 0}, {"n_nodes": -5}, {"n_nodes": 2 ** 29}, {"n_faces": 0}, {"n_faces": 2 ** 29},
                 {"dim": 1}, {"dim": 4}]
        if name != "pdg_femq1_elements":
            sizes += [{"n_graphs": 0}, {"n_graphs": -1}, {"n_graphs": 65536}, {"n_cases": 0}, {"n_cases": 65}]
        for bad in sizes:
            with pytest.raises(PdgError, match=f"{name}: bad sizes"):
                fn(*_args(name, **bad))
            with pytest.raises(PdgError, match="bad sizes"):   # the sizes are refused first, whatever else is wrong
                fn(*_args(name, null=("points",), young=-1.0, **bad))
    for name in ("pdg_femq1_solve", "pdg_femq1_stress"):
        fn = getattr(lib, name)
        for bad in ({"young": 0.0}, {"young": -1.0}, {"young": float("inf")}, {"young": float("nan")},
                    {"poisson": 0.5}, {"poisson": -1.0}, {"poisson": float("nan")}):
            with pytest.raises(PdgError, match="young must be finite and > 0, poisson in"):
                fn(*_args(name, **bad))
        with pytest.raises(PdgError, match="null argument"):   # a null pointer before the material
            fn(*_args(name, null=("elem",), young=-1.0))
    for bad in (0.0, -1e-5, 1.0, float("nan"), float("inf")):
        with pytest.raises(PdgError, match="rtol"):
            lib.pdg_femq1_solve(*_args("pdg_femq1_solve", rtol=bad))
    with pytest.raises(PdgError, match="young"):               # the material before rtol, rtol before the scratch
        lib.pdg_femq1_solve(*_args("pdg_femq1_solve", young=0.0, rtol=2.0, scratch_bytes=0))
    with pytest.raises(PdgError, match="rtol"):
        lib.pdg_femq1_solve(*_args("pdg_femq1_solve", rtol=2.0, scratch_bytes=0))
    need = lib.pdg_femq1_solve_scratch_bytes(100, 3)
    for short in (need - 1, 0, -1):
        with pytest.raises(PdgError, match="scratch too small"):
            lib.pdg_femq1_solve(*_args("pdg_femq1_solve", scratch_bytes=short))
    for bad in (-1, 2):
        with pytest.raises(PdgError, match="nodal"):
            lib.pdg_femq1_stress(*_args("pdg_femq1_stress", nodal=bad))
    with pytest.raises(PdgError, match="young"):               # the material before nodal
        lib.pdg_femq1_stress(*_args("pdg_femq1_stress", young=0.0, nodal=5))


def test_the_kernels_follow_the_per_graph_conventions():
    """Kernel launches and nothing else on the stream; no float atomics; contraction off; the iteration cap and the
    noise rule are in the source as the header states them; the Gauss-point loops stay rolled."""
    code = re.sub(r"//[^\n]*", "", SOURCE.read_text())
    assert code.count("hipLaunchKernelGGL") == 5       # clear + elements, solve, nodal + sums
    for banned in ("hipMemset", "hipMemcpy", "hipMalloc", "hipStreamSynchronize", "hipDeviceSynchronize",
                   "atomicAdd", "atomicExch", "atomicCAS"):
        assert banned not in code, banned
    assert set(re.findall(r"\batomic\w+", code)) == {"atomicOr"}        # the element table's status bits only
    solve = code[code.index("void stress_of"):code.index("face_displacements")]
    assert "void femq1_solve_kernel" in solve and "atomic" not in solve
    assert code.count("fp contract(off)") == 4
    assert "Q1_MAX_ITER = 100000" in code and "Q1_NOISE = 1e-12" in code and "Q1_T = 1024" in code
    assert "max_iter > Q1_MAX_ITER ? Q1_MAX_ITER" in code
    assert "__launch_bounds__(Q1_T) void femq1_solve_kernel" in code
    force = code[code.index("void corner_force"):code.index("void apply_row")]
    assert "#pragma unroll 1" in force and "for (int g = 0; g < 4; ++g)" in force
    for shared in ('#include "pdg_femmesh.hpp"', '#include "pdg_reduce.hpp"', "row_range4(", "item_of4(",
                   "block_sum_k_wave_major("):
        assert shared in code, shared
    mesh = (SOURCE.parent / "pdg_femmesh.hpp").read_text()
    assert "row_range4" in mesh and "item_of4" in mesh and "struct Mesh" not in code


def test_triangle_sources_are_untouched_by_the_quad_solver():
    """The quad solver lives beside the triangle solvers: neither their sources nor their modules name it."""
    csrc = SOURCE.parent
    for f in (csrc / "pdg_fem.hip", csrc / "pdg_hyper.hip", ROOT / "p-div-gnn_amd" / "gnn_local_stress" / "fem.py",
              ROOT / "p-div-gnn_amd" / "gnn_local_stress" / "hyperelastic.py"):
        text = f.read_text()
        assert "femq1" not in text and "fem_q1" not in text and "item_of4" not in text, f.name


def test_python_layer_refusals():
    import torch
    from gnn_local_stress import fem, fem_q1
    from pdg import meshgen
    s = meshgen.quad_hole_plate(5)
    pts, fcs = torch.from_numpy(s.pos), torch.from_numpy(s.faces)
    assert fcs.shape[1] == 4
    for call in (lambda: fem_q1.FemPlan.from_mesh(pts, fcs),
                 lambda: fem_q1.solve_cell(pts, fcs, strain=(1.0, 0.0, 0.0)),
                 lambda: fem_q1.solve_cell(pts, fcs, stress=(1.0, 0.0, 0.0)),
                 lambda: fem_q1.effective_stiffness(pts, fcs), lambda: fem_q1.localisation_tensor(pts, fcs),
                 lambda: fem_q1.fem_targets(pts, fcs, (1.0, 0.0, 0.0)),
                 lambda: fem_q1.write_sample("unused", 0, pts, fcs, (1.0, 0.0, 0.0)),
                 lambda: fem_q1.element_table(fem_q1.FemPlan.empty("cpu"), pts[:0]),
                 lambda: fem_q1.solve_cells(fem_q1.FemPlan.empty("cpu"), pts[:0], torch.zeros(1, 1, 3))):
        with pytest.raises(RuntimeError, match="HIP"):
            call()
    with pytest.raises(ValueError, match="exactly one of"):
        fem_q1.solve_cell(pts, fcs)
    with pytest.raises(ValueError, match="exactly one of"):
        fem_q1.solve_cell(pts, fcs, strain=(1.0, 0.0, 0.0), stress=(1.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="fem_q1.FemPlan"):
        fem_q1.solve_cells(fem.FemPlan.empty("cpu"), pts[:0], torch.zeros(1, 1, 3))
    with pytest.raises(ValueError, match="quad plans only"):
        fem_q1.FemPlan.collate([fem_q1.FemPlan.empty("cpu"), fem.FemPlan.empty("cpu")])
    batch = fem_q1.FemPlan.collate([fem_q1.FemPlan.empty("cpu")] * 2)
    assert isinstance(batch, fem_q1.FemPlan) and batch.n_graphs == 2 and batch.sizes == ((0, 0), (0, 0))
    assert batch.item_rowptr.tolist() == [0] and batch.ptr.tolist() == [0, 0, 0]
    assert [f.name for f in fem_q1.FemPlan.__dataclass_fields__.values()] == \
        [f.name for f in fem.FemPlan.__dataclass_fields__.values()]
    assert fem_q1.STATUS == ("CONVERGED", "TRIVIAL", "MAX_ITER", "BREAKDOWN")
    assert fem_q1.COLUMNS == ("iterations", "rhs_norm", "residual", "status") and fem_q1.NODAL == ("area", "count")
    assert (fem_q1.YOUNG, fem_q1.POISSON, fem_q1.MAX_CASES, fem_q1.MAX_ITER_CAP) == (1e5, 0.3, 64, 100000)
    assert fem_q1.CSV_COLUMNS is fem.CSV_COLUMNS and fem_q1.stiffness is fem.stiffness
    assert fem_q1.FemFields is fem.FemFields and fem_q1.CellSolution is fem.CellSolution
