"""CPU-side checks of the hyperelastic C ABI (pdg_hyper_solve_scratch_bytes, pdg_hyper_solve and pdg_hyper_stress in
csrc/pdg_hyper.hip): declared, bound with matching pointer / integer kinds, exported, bad arguments refused before any
HIP call; the conventions the header states; and the Python layer's own refusals."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "pdivgnn.h"
SOURCE = ROOT / "p-div-gnn_amd" / "csrc" / "pdg_hyper.hip"
NAMES = ("pdg_hyper_solve_scratch_bytes", "pdg_hyper_solve", "pdg_hyper_stress")
CALLS = ("pdg_hyper_solve", "pdg_hyper_stress")


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


def test_header_and_signatures_hold_the_hyper_calls():
    from pdg.lib import _RESTYPES, SIGNATURES
    kinds = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double}
    for name in NAMES:
        params = _params(name)
        assert name in SIGNATURES, name
        assert len(SIGNATURES[name]) == len(params), name
        for ctype, (ctext, nm) in zip(SIGNATURES[name], params):
            assert ctype is (ctypes.c_void_p if "*" in ctext else kinds[ctext]), (name, nm)
    assert _RESTYPES["pdg_hyper_solve_scratch_bytes"] is ctypes.c_long
    assert not any(n in _RESTYPES for n in CALLS)
    assert [n for _, n in _params("pdg_hyper_solve_scratch_bytes")] == ["n_nodes", "n_faces", "n_cases"]
    assert [n for _, n in _params("pdg_hyper_solve")] == [
        "n_graphs", "n_cases", "ptr", "fptr", "n_nodes", "n_faces", "rverts", "rep", "item_rowptr", "item", "elem",
        "fbar", "mu", "kappa", "volumetric", "rtol", "n_steps", "max_newton", "eta", "max_pcg", "ut", "table",
        "scratch", "scratch_bytes", "stream"]
    assert [n for _, n in _params("pdg_hyper_stress")] == [
        "n_graphs", "n_cases", "ptr", "fptr", "n_nodes", "points", "dim", "n_faces", "verts", "rep", "item_rowptr",
        "item", "elem", "fbar", "ut", "mu", "kappa", "volumetric", "nodal", "stress", "strain", "sums", "stream"]
    k = dict((n, t) for t, n in _params("pdg_hyper_solve"))
    assert k["ut"] == k["table"] == "double*" and k["elem"] == k["fbar"] == "const double*"
    assert k["rep"] == k["item"] == k["rverts"] == k["fptr"] == "const int*"
    assert k["rtol"] == k["eta"] == k["mu"] == k["kappa"] == "double" and k["scratch_bytes"] == "long"
    k = dict((n, t) for t, n in _params("pdg_hyper_stress"))
    assert k["stress"] == k["strain"] == "float*" and k["sums"] == "double*" and k["ut"] == "const double*"


def test_header_states_the_conventions():
    text = " ".join(HEADER.read_text().replace("\n *", "\n").split())
    for phrase in ("Hyperelastic FEM targets", "U = kappa (J ln J - J + 1)", "U = kappa / 2 (J - 1)^2",
                   "|r|_2 <= rtol |f_abs|_2", "a truncation and not a failure", "alpha = 1, 1/2, .. 2^-10",
                   "Phi(x + alpha d) <= Phi(x) - 1e-4 alpha r.d", "0 CONVERGED; 2 MAX_ITER", "3 BREAKDOWN",
                   "no input makes the workgroup spin", "alone and inside any batch", "it can be captured",
                   "no float atomics", "no memset", "seven 2 n_nodes fp64 vectors and 14 doubles per face",
                   "the true final relative residual", "the node's own corners (not its images')",
                   "weighted by the deformed area area J_e", "1/2 ln(F F^T)"):
        assert phrase in text, phrase


def test_library_exports_the_hyper_calls_and_the_source_is_built():
    import build as pdg_build
    from pdg.lib import lib, source_hash
    dll = lib.load()
    for name in NAMES:
        assert hasattr(dll, name), name
    assert SOURCE.is_file()
    assert pdg_build.source_hash() == source_hash() == lib.pdg_source_hash().decode()


def test_scratch_size():
    from pdg.lib import lib
    f = lib.pdg_hyper_solve_scratch_bytes
    for bad in ((0, 1, 1), (-1, 1, 1), (10, 0, 1), (10, -2, 1), (10, 10, 0), (10, 10, 65), (2 ** 29, 1, 1),
                (1, 2 ** 29, 1)):
        assert f(*bad) < 0, bad
    # seven 2 n vectors and 14 doubles a face, per load case
    for n, nf, cases in ((1, 1, 1), (1208, 2216, 3), (100, 150, 64), (2 ** 29 - 1, 2 ** 29 - 1, 1)):
        need = (7 * 2 * n + 14 * nf) * 8 * cases
        assert need <= f(n, nf, cases) < need + 256


def _args(name, null=(), **vals):
    """Arguments of `name`: every pointer a distinct 16-byte-aligned fake address 2^32 apart (never dereferenced: the
    checks run on the host before any HIP call) except those in `null` and the stream."""
    from pdg.lib import lib
    v = {"n_graphs": 3, "n_cases": 3, "n_nodes": 100, "n_faces": 150, "dim": 2, "mu": 3.0, "kappa": 10.0,
         "volumetric": 0, "rtol": 1e-10, "n_steps": 4, "max_newton": 5, "eta": 1e-4, "max_pcg": 10, "nodal": 0,
         "scratch_bytes": lib.pdg_hyper_solve_scratch_bytes(100, 150, 3)}
    v.update(vals)
    out = []
    for i, (ctext, nm) in enumerate(_params(name)):
        if "*" in ctext:
            out.append(None if nm in null or nm == "stream" else v.get(nm, 0x100000000 * (i + 1)))
        else:
            out.append(v[nm])
    return out


def test_hyper_calls_refuse_bad_arguments():
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-side argument checks only: never called with fake pointers where a GPU is present")
    from pdg.lib import PdgError, lib
    for name in CALLS:
        fn = getattr(lib, name)
        for nm in [nm for ctext, nm in _params(name) if "*" in ctext and nm != "stream"]:   # every pointer is required
            with pytest.raises(PdgError, match="null argument"):
                fn(*_args(name, null=(nm,)))
        sizes = [{"n_nodes": 0}, {"n_nodes": -5}, {"n_nodes": 2 ** 29}, {"n_faces": 0}, {"n_faces": 2 ** 29},
                 {"n_graphs": 0}, {"n_graphs": -1}, {"n_graphs": 65536}, {"n_cases": 0}, {"n_cases": 65}]
        if name == "pdg_hyper_stress":
            sizes += [{"dim": 1}, {"dim": 4}]
        for bad in sizes:
            with pytest.raises(PdgError, match="bad sizes"):
                fn(*_args(name, **bad))
            with pytest.raises(PdgError, match="bad sizes"):   # the sizes are refused first, whatever else is wrong
                fn(*_args(name, null=("ptr",), mu=-1.0, **bad))
        for bad in ({"mu": 0.0}, {"mu": -1.0}, {"mu": float("inf")}, {"mu": float("nan")}, {"kappa": 0.0},
                    {"kappa": float("nan")}, {"volumetric": 2}, {"volumetric": -1}):
            with pytest.raises(PdgError, match="mu and kappa must be finite and > 0, volumetric 0"):
                fn(*_args(name, **bad))
    for bad in ({"rtol": 0.0}, {"rtol": 1.0}, {"rtol": float("nan")}, {"eta": 0.0}, {"eta": 1.0}, {"eta": -1e-3}):
        with pytest.raises(PdgError, match="rtol and eta"):
            lib.pdg_hyper_solve(*_args("pdg_hyper_solve", **bad))
    for bad in (0, -1, 10001):
        with pytest.raises(PdgError, match="n_steps"):
            lib.pdg_hyper_solve(*_args("pdg_hyper_solve", n_steps=bad))
    need = lib.pdg_hyper_solve_scratch_bytes(100, 150, 3)
    for short in (need - 1, 0, -1):
        with pytest.raises(PdgError, match="scratch too small"):
            lib.pdg_hyper_solve(*_args("pdg_hyper_solve", scratch_bytes=short))
    for bad in (-1, 2):
        with pytest.raises(PdgError, match="nodal"):
            lib.pdg_hyper_stress(*_args("pdg_hyper_stress", nodal=bad))


def test_the_kernels_follow_the_per_graph_conventions():
    """Kernel launches and nothing else on the stream; no atomics at all; contraction off for the whole file; the caps
    are in the source as the header states them; the mesh helpers are shared with pdg_fem.hip, not restated."""
    code = re.sub(r"//[^\n]*", "", SOURCE.read_text())
    assert code.count("hipLaunchKernelGGL") == 3       # solve, nodal + sums
    for banned in ("hipMemset", "hipMemcpy", "hipMalloc", "hipStreamSynchronize", "hipDeviceSynchronize", "atomic"):
        assert banned not in code, banned
    assert code.index("#pragma clang fp contract(off)") < code.index("namespace {")
    for phrase in ("HY_T = 1024", "HY_ES = 14", "HY_VECS = 7", "HY_HALVINGS = 10", "HY_ARMIJO = 1e-4",
                   "HY_MAX_STEPS = 10000", "HY_MAX_NEWTON = 1000", "HY_MAX_PCG = 100000",
                   "__launch_bounds__(HY_T) void hyper_solve_kernel", '#include "pdg_femmesh.hpp"'):
        assert phrase in code, phrase
    assert "struct Mesh" not in code
    fem = (SOURCE.parent / "pdg_fem.hip").read_text()
    assert '#include "pdg_femmesh.hpp"' in fem and "struct Mesh" not in fem
    assert "struct Mesh" in (SOURCE.parent / "pdg_femmesh.hpp").read_text()


def test_python_layer_refusals():
    import torch
    from gnn_local_stress import fem, hyperelastic as hy
    from pdg import meshgen
    s = meshgen.hole_plate(5)
    pts, fcs = torch.from_numpy(s.pos), torch.from_numpy(s.faces)
    for call in (lambda: hy.solve_cell(pts, fcs, strain=(0.1, 0.0, 0.0)),
                 lambda: hy.solve_cell(pts, fcs, F=[[1.1, 0.0], [0.0, 1.0]]),
                 lambda: hy.hyper_targets(pts, fcs, (0.1, 0.0, 0.0)),
                 lambda: hy.write_sample("unused", 0, pts, fcs, (0.1, 0.0, 0.0))):
        with pytest.raises(RuntimeError, match="HIP"):
            call()
    with pytest.raises(ValueError, match="quads are out of scope"):
        hy.solve_cell(pts, fcs, strain=(0.1, 0.0, 0.0), cells="quad")
    with pytest.raises(ValueError, match="exactly one of"):
        hy.solve_cell(pts, fcs)
    with pytest.raises(ValueError, match="exactly one of"):
        hy.solve_cell(pts, fcs, strain=(0.1, 0.0, 0.0), F=torch.eye(2))
    with pytest.raises(ValueError, match="finite"):
        hy.deformation_gradient((float("nan"), 0.0, 0.0))
    for bad in (dict(mu=0.0), dict(mu=float("inf")), dict(kappa=-1.0), dict(kappa=float("nan")),
                dict(volumetric="cubic")):
        with pytest.raises(ValueError, match="mu|kappa|volumetric"):
            hy._law(**{**dict(mu=3.0, kappa=10.0, volumetric="log"), **bad})
    f = hy.deformation_gradient((0.15, -0.10, 0.08))
    assert f.dtype == torch.float64 and torch.equal(f, f.T)
    assert abs(float(torch.linalg.det(f)) - 2.718281828459045 ** 0.05) <= 1e-14
    assert torch.allclose(hy._log_strain_of(f), torch.tensor([0.15, -0.10, 0.08], dtype=torch.float64), atol=1e-14)
    assert hy.STATUS == fem.STATUS and (hy.CONVERGED, hy.MAX_ITER, hy.BREAKDOWN) == (0, 2, 3)
    assert hy.COLUMNS == ("load_steps", "newton_iterations", "pcg_iterations", "force_norm", "residual", "status")
    assert (hy.MU, hy.KAPPA, hy.VOLUMETRIC) == (3.0, 10.0, ("log", "quadratic"))
