"""CPU-side checks of the homogenisation C ABI (pdg_nodal_areas in csrc/pdg_meshfields.hip, pdg_graph_wmean and
pdg_mean_correct in csrc/pdg_homog.hip): declared, bound with matching pointer / integer kinds, exported, bad
arguments refused before any HIP call; and the Python layer's own refusals."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "pdivgnn.h"
NAMES = ("pdg_nodal_areas", "pdg_graph_wmean", "pdg_mean_correct")
OPTIONAL = {"pdg_nodal_areas": (), "pdg_graph_wmean": ("weights",), "pdg_mean_correct": ("denom",)}
REQUIRED = {"pdg_nodal_areas": ("points", "faces", "area", "bbox", "status", "scratch"),
            "pdg_graph_wmean": ("ptr", "rows", "table"),
            "pdg_mean_correct": ("ptr", "sigma", "table", "target", "out")}


def _params(name):
    """(C type, name) of every parameter of `name` in include/pdivgnn.h."""
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", text, re.S)
    assert m, f"{name} is not declared in include/pdivgnn.h"
    out = []
    for a in m.group(1).split(","):
        nm = re.findall(r"\w+", a)[-1]
        out.append((a.strip()[:a.strip().rfind(nm)].strip(), nm))
    return out


def test_header_and_signatures_hold_the_homogenisation_calls():
    from pdg.lib import _RESTYPES, SIGNATURES
    kinds = {"int": ctypes.c_int, "long": ctypes.c_long}
    for name in NAMES:
        params = _params(name)
        assert name in SIGNATURES, name
        assert len(SIGNATURES[name]) == len(params), name
        for ctype, (ctext, nm) in zip(SIGNATURES[name], params):
            assert ctype is (ctypes.c_void_p if "*" in ctext else kinds[ctext]), (name, nm)
        assert name not in _RESTYPES
    assert [n for _, n in _params("pdg_nodal_areas")] == [
        "n_nodes", "points", "dim", "n_faces", "faces", "area", "bbox", "status", "scratch", "scratch_bytes", "stream"]
    assert [n for _, n in _params("pdg_graph_wmean")] == [
        "n_graphs", "ptr", "rows", "n_cols", "weights", "table", "stream"]
    assert [n for _, n in _params("pdg_mean_correct")] == [
        "n_graphs", "ptr", "sigma", "table", "target", "denom", "out", "stream"]
    wm, mc = (dict((n, t) for t, n in _params(name)) for name in NAMES[1:])
    assert wm["table"] == "double*" and wm["rows"] == wm["weights"] == "const float*"
    assert mc["table"] == mc["denom"] == "const double*" and mc["out"] == "float*" and mc["sigma"] == "const float*"


def test_header_states_the_conventions():
    text = " ".join(HEADER.read_text().split())
    for phrase in ("generate_dataset.py:73-82", "generate_dataset.py:278-289", "area_f / 3", "(xmin, xmax, ymin, ymax)",
                   "weight is > 0", "D_g = W_g", "may alias sigma", "participating or not", "NaN shift",
                   "alone and inside any batch", "a node of no face gets exactly 0"):
        assert phrase in text, phrase


def test_library_exports_the_homogenisation_calls():
    from pdg.lib import lib
    dll = lib.load()
    for name in NAMES:
        assert hasattr(dll, name), name


def test_the_source_is_built_and_hashed():
    """build.py compiles every csrc/*.hip, and both source hashes read the same list."""
    import build as pdg_build
    from pdg.lib import CSRC, lib, source_hash
    assert (CSRC / "pdg_homog.hip").is_file()
    assert pdg_build.source_hash() == source_hash() == lib.pdg_source_hash().decode()


def _args(name, null=(), **vals):
    """Arguments of `name`: every pointer a distinct 16-byte-aligned fake address (never dereferenced: the checks
    run on the host before any HIP call) except those in `null` and the stream."""
    from pdg.lib import lib
    v = {"n_graphs": 3, "n_cols": 3, "n_nodes": 100, "n_faces": 150, "dim": 2,
         "scratch_bytes": lib.pdg_mesh_fields_scratch_bytes(100, 150)}
    v.update(vals)
    out = []
    for i, (ctext, nm) in enumerate(_params(name)):
        out.append((None if nm in null or nm == "stream" else 0x100000 + 0x1000 * i) if "*" in ctext else v[nm])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_homogenisation_calls_refuse_bad_arguments(name):
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-side argument checks only: never called with fake pointers where a GPU is present")
    from pdg.lib import PdgError, lib
    fn = getattr(lib, name)
    pointers = [nm for ctext, nm in _params(name) if "*" in ctext and nm != "stream"]
    assert sorted(pointers) == sorted(REQUIRED[name] + OPTIONAL[name])
    for nm in REQUIRED[name]:
        with pytest.raises(PdgError, match="null argument"):
            fn(*_args(name, null=(nm,)))
        with pytest.raises(PdgError, match="null argument"):
            fn(*_args(name, null=OPTIONAL[name] + (nm,)))
    if name == "pdg_nodal_areas":
        for bad in ({"n_nodes": 0}, {"n_nodes": -1}, {"n_faces": -1}, {"dim": 1}, {"dim": 4}, {"n_faces": 2 ** 31 // 9}):
            with pytest.raises(PdgError, match="bad sizes"):
                fn(*_args(name, **bad))
        need = lib.pdg_mesh_fields_scratch_bytes(100, 150)
        with pytest.raises(PdgError, match="scratch too small"):
            fn(*_args(name, scratch_bytes=need - 1))
        # faces may be NULL for a mesh without faces: the only refusal left is the one provoked here
        with pytest.raises(PdgError, match="scratch too small"):
            fn(*_args(name, null=("faces",), n_faces=0, scratch_bytes=lib.pdg_mesh_fields_scratch_bytes(100, 0) - 1))
        return
    for bad in (0, -1):
        with pytest.raises(PdgError, match="bad sizes"):
            fn(*_args(name, n_graphs=bad))
        # the sizes are refused first, whatever else is wrong; the optional pointers pass as NULL
        with pytest.raises(PdgError, match="bad sizes"):
            fn(*_args(name, null=OPTIONAL[name] + ("ptr",), n_graphs=bad))
    if name == "pdg_graph_wmean":
        for bad in (0, -1, 10):
            with pytest.raises(PdgError, match="bad sizes"):
                fn(*_args(name, n_cols=bad))
    src = (ROOT / "p-div-gnn_amd" / "csrc" / "pdg_homog.hip").read_text()
    check = re.search(rf'PDG_CHECK_ARG\(([^;]*?),\s*"{name}: null argument', src, re.S).group(1)
    for nm in OPTIONAL[name]:
        assert not re.search(rf"\b{nm}\b", check), nm


def test_scratch_size_is_unchanged_by_the_areas():
    """pdg_nodal_areas lives in the labels' layout: 3 F slots twice fit the 9 F the operator needs."""
    from pdg.lib import lib
    f = lib.pdg_mesh_fields_scratch_bytes
    assert f(25556, 50000) >= 2 * 8 * 9 * 50000 and f(100, 0) >= 4 * 6 * 100


def test_python_layer_refuses_cpu_tensors_bad_shapes_and_unknown_names():
    import torch
    from gnn_local_stress import homogenise as H
    from pdg import devgraph
    s = torch.zeros(4, 3)
    ptr = torch.tensor([0, 4])
    cell = torch.ones(1, dtype=torch.float64)
    for call in (lambda: H.graph_average(s, ptr), lambda: H.graph_average(s[:, 0], ptr),
                 lambda: H.mean_defect(s, ptr, torch.zeros(1, 3), cell_area=cell),
                 lambda: H.enforce_mean(s, ptr, torch.zeros(1, 3), "material")):
        with pytest.raises(RuntimeError, match="HIP"):
            call()
    with pytest.raises(RuntimeError, match="device tensors"):
        devgraph.nodal_areas(torch.zeros(4, 2), torch.zeros(2, 3, dtype=torch.int64))
    for fn in (H.mean_defect, H.enforce_mean):
        with pytest.raises(ValueError, match="cell, material"):
            fn(s, ptr, torch.zeros(1, 3), "box")
        with pytest.raises(ValueError, match=r"\(N, 3\)"):
            fn(torch.zeros(4, 2), ptr, torch.zeros(1, 3), "material")
        with pytest.raises(ValueError, match=r"\(N, 3\)"):
            fn(torch.zeros(4), ptr, torch.zeros(1, 3), "material")
    with pytest.raises(ValueError, match="C <= 9"):
        H.graph_average(torch.zeros(4, 10), ptr)
    with pytest.raises(ValueError, match="C <= 9"):
        H.graph_average(torch.zeros(4, 3, 3), ptr)
    assert H.CONVENTIONS == ("cell", "material")


def test_mean_localisation_and_predict_mesh_refuse_unknown_conventions():
    import torch
    from gnn_local_stress.inference import predict_mesh
    from gnn_local_stress.models import EncodeProcessDecode
    from gnn_local_stress.sensitivity import mean_localisation
    from pdg import graph, meshgen
    m = EncodeProcessDecode(1, 2, latent_size=128, input_nodes_features_size=6, output_nodes_features_size=3)
    sample = meshgen.hole_plate(5)
    b = graph.Batch.from_data_list([graph.sample_to_data(sample)])
    with pytest.raises(ValueError, match="cell, material"):
        mean_localisation(m, b, convention="box")
    with pytest.raises(ValueError, match="needs the cell's area"):
        mean_localisation(m, b)
    with pytest.raises(RuntimeError, match="HIP"):
        mean_localisation(m, b, convention="material")
    with pytest.raises(ValueError, match="cell, material"):
        predict_mesh(m, (sample.pos, sample.faces), sample.mean_stress, enforce_mean="box")
