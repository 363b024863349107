"""CPU-side checks of the equilibration C ABI (pdg_equilibrate_scratch_bytes and pdg_equilibrate in
csrc/pdg_equil.hip): declared, bound with matching pointer / integer kinds, exported, bad arguments refused before
any HIP call; and the Python layer's own refusals."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "pdivgnn.h"
NAMES = ("pdg_equilibrate_scratch_bytes", "pdg_equilibrate")
REQUIRED = ("ptr", "a_rowptr", "a_col", "a_val", "at_rowptr", "at_row", "at_comp", "at_val", "node_types", "in", "out",
            "table", "scratch")
OPTIONAL = ("weights",)


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


def test_header_and_signatures_hold_the_equilibration_calls():
    from pdg.lib import _RESTYPES, SIGNATURES
    kinds = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float}
    for name in NAMES:
        params = _params(name)
        assert name in SIGNATURES, name
        assert len(SIGNATURES[name]) == len(params), name
        for ctype, (ctext, nm) in zip(SIGNATURES[name], params):
            assert ctype is (ctypes.c_void_p if "*" in ctext else kinds[ctext]), (name, nm)
    assert _RESTYPES["pdg_equilibrate_scratch_bytes"] is ctypes.c_long and "pdg_equilibrate" not in _RESTYPES
    assert [n for _, n in _params("pdg_equilibrate_scratch_bytes")] == ["n_nodes", "n_graphs"]
    assert [n for _, n in _params("pdg_equilibrate")] == [
        "n_graphs", "ptr", "n_nodes", "a_rowptr", "a_col", "a_val", "at_rowptr", "at_row", "at_comp", "at_val",
        "node_types", "weights", "in", "transpose", "rtol", "max_iter", "out", "table", "scratch", "scratch_bytes",
        "stream"]
    k = dict((n, t) for t, n in _params("pdg_equilibrate"))
    assert k["table"] == "double*" and k["out"] == "float*" and k["in"] == k["weights"] == "const float*"
    assert k["node_types"] == "const int64_t*" and k["rtol"] == "float" and k["scratch_bytes"] == "long"
    # the operator arrays are pdg_div_plan's outputs, name for name
    plan = dict((n, t) for t, n in _params("pdg_div_plan"))
    for nm in ("a_rowptr", "a_col", "a_val", "at_rowptr", "at_row", "at_comp", "at_val"):
        assert k[nm] == "const " + plan[nm], nm


def test_header_states_the_conventions():
    text = " ".join(HEADER.read_text().split())
    for phrase in ("S = C W^-1 C^T", "node_types[v] == 0", "W = diag(w, w, 2 w)", "entries with col >= 2 n ignored",
                   "as pdg_div_plan writes both", "the true final residual", "bitwise copy of in",
                   "alone and inside any batch", "it can be captured", "no float atomics", "overlaps in"):
        assert phrase in text, phrase


def test_library_exports_the_equilibration_calls_and_the_source_is_built():
    import build as pdg_build
    from pdg.lib import CSRC, lib, source_hash
    dll = lib.load()
    for name in NAMES:
        assert hasattr(dll, name), name
    assert (CSRC / "pdg_equil.hip").is_file()
    assert pdg_build.source_hash() == source_hash() == lib.pdg_source_hash().decode()


def test_scratch_size():
    from pdg.lib import lib
    f = lib.pdg_equilibrate_scratch_bytes
    for bad in ((0, 1), (-1, 1), (10, 0), (10, -3), (2 ** 29, 1), (2 ** 31 - 1, 1)):
        assert f(*bad) < 0, bad
    # lam, r, p, S p (2 floats a node each) and the work field (3): 44 bytes a node, whatever the graph count
    assert f(1, 1) >= 44 and f(5041 * 8, 8) >= 44 * 5041 * 8 and f(5041 * 8, 8) == f(5041 * 8, 1)
    assert f(2 ** 29 - 1, 1) >= 44 * (2 ** 29 - 1)


def _args(null=(), **vals):
    """Arguments of pdg_equilibrate: every pointer a distinct 16-byte-aligned fake address 2^32 apart (never
    dereferenced: the checks run on the host before any HIP call) except those in `null` and the stream."""
    from pdg.lib import lib
    v = {"n_graphs": 3, "n_nodes": 100, "transpose": 0, "rtol": 1e-5, "max_iter": 10,
         "scratch_bytes": lib.pdg_equilibrate_scratch_bytes(100, 3)}
    v.update(vals)
    out = []
    for i, (ctext, nm) in enumerate(_params("pdg_equilibrate")):
        if "*" in ctext:
            out.append(None if nm in null or nm == "stream" else v.get(nm, 0x100000000 * (i + 1)))
        else:
            out.append(v[nm])
    return out


def test_equilibrate_refuses_bad_arguments():
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-side argument checks only: never called with fake pointers where a GPU is present")
    from pdg.lib import PdgError, lib
    fn = lib.pdg_equilibrate
    pointers = [nm for ctext, nm in _params("pdg_equilibrate") if "*" in ctext and nm != "stream"]
    assert sorted(pointers) == sorted(REQUIRED + OPTIONAL)
    for nm in REQUIRED:
        with pytest.raises(PdgError, match="null argument"):
            fn(*_args(null=(nm,)))
        with pytest.raises(PdgError, match="null argument"):
            fn(*_args(null=OPTIONAL + (nm,)))
    for bad in ({"n_graphs": 0}, {"n_graphs": -1}, {"n_nodes": 0}, {"n_nodes": -5}, {"n_nodes": 2 ** 29}):
        with pytest.raises(PdgError, match="bad sizes"):
            fn(*_args(**bad))
        # the sizes are refused first, whatever else is wrong
        with pytest.raises(PdgError, match="bad sizes"):
            fn(*_args(null=("ptr", "weights"), rtol=-1.0, **bad))
    for bad in (0.0, -1e-5, float("nan"), float("inf")):
        with pytest.raises(PdgError, match="rtol"):
            fn(*_args(rtol=bad))
    with pytest.raises(PdgError, match="max_iter"):
        fn(*_args(max_iter=-1))
    need = lib.pdg_equilibrate_scratch_bytes(100, 3)
    for short in (need - 1, 0, -1):
        with pytest.raises(PdgError, match="scratch too small"):
            fn(*_args(scratch_bytes=short))
    base = 0x7000000000
    for shift in (0, 4, 100 * 12 - 4, -(100 * 12 - 4)):   # the same array, and every partial overlap
        with pytest.raises(PdgError, match="alias"):
            fn(*_args(**{"in": base, "out": base + shift}))
    src = (ROOT / "p-div-gnn_amd" / "csrc" / "pdg_equil.hip").read_text()
    check = re.search(r'PDG_CHECK_ARG\(([^;]*?),\s*"pdg_equilibrate: null argument', src, re.S).group(1)
    assert not re.search(r"\bweights\b", check)


def test_the_kernel_follows_the_per_graph_conventions():
    """One kernel launch and nothing else on the stream; no atomics; sums folded in a fixed order."""
    src = (ROOT / "p-div-gnn_amd" / "csrc" / "pdg_equil.hip").read_text()
    code = re.sub(r"//[^\n]*", "", src)
    assert code.count("hipLaunchKernelGGL") == 1
    for banned in ("hipMemset", "hipMemcpy", "hipMalloc", "hipStreamSynchronize", "hipDeviceSynchronize", "atomic"):
        assert banned not in code, banned
    assert "fp contract(off)" in code


def test_python_layer_refuses_cpu_tensors_bad_shapes_and_batches_without_what_it_needs():
    import torch
    from gnn_local_stress import equilibrate as E
    from gnn_local_stress.inference import predict_mesh
    from pdg import graph, meshgen
    sample = meshgen.hole_plate(5)
    b = graph.Batch.from_data_list([graph.sample_to_data(sample)])
    s = torch.zeros(sample.num_nodes, 3)
    for call in (lambda: E.equilibrate(s, b), lambda: E.equilibrate_grad(s, b, None), lambda: E.divergence_defect(s, b)):
        with pytest.raises(RuntimeError, match="HIP"):
            call()
    assert E.COLUMNS == ("defect", "residual", "iterations", "status")
    assert (E.NOT_CONVERGED, E.ABOVE_TWICE_RTOL, E.BAD_WEIGHT) == (1, 2, 4)
    with pytest.raises(ValueError, match="cell, material"):   # refused before anything is looked at
        E.equilibrate(s, b, None, mean="box")
    m_args = dict(latent_size=128, input_nodes_features_size=6, output_nodes_features_size=3)
    from gnn_local_stress.models import EncodeProcessDecode
    with pytest.raises(ValueError, match="cell, material"):
        predict_mesh(EncodeProcessDecode(1, 2, **m_args), (sample.pos, sample.faces), sample.mean_stress,
                     enforce_mean="box", equilibrate=True)
