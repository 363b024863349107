"""CPU-side checks of the boundary-residual C ABI (pdg_boundary_vectors in csrc/pdg_meshfields.hip,
pdg_boundary_residuals and pdg_boundary_residuals_bwd in csrc/pdg_boundary.hip): declared, bound with matching
pointer / integer kinds, exported, bad arguments refused before any HIP call; and the Python layer's own refusals."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "pdivgnn.h"
NAMES = ("pdg_boundary_vectors", "pdg_boundary_residuals", "pdg_boundary_residuals_bwd")
EDGES = ("rowptr_dst", "src", "perm", "edge_attr")
OPTIONAL = {"pdg_boundary_vectors": (), "pdg_boundary_residuals": EDGES,
            "pdg_boundary_residuals_bwd": EDGES + ("g_traction", "g_periodic")}
REQUIRED = {"pdg_boundary_vectors": ("points", "faces", "bvec", "blen", "status", "scratch"),
            "pdg_boundary_residuals": ("ptr", "sigma", "bvec", "blen", "labels", "table", "argmax"),
            "pdg_boundary_residuals_bwd": ("ptr", "sigma", "bvec", "blen", "labels", "table", "out")}


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


def test_header_and_signatures_hold_the_boundary_calls():
    from pdg.lib import _RESTYPES, SIGNATURES
    kinds = {"int": ctypes.c_int, "long": ctypes.c_long}
    for name in NAMES:
        params = _params(name)
        assert name in SIGNATURES, name
        assert len(SIGNATURES[name]) == len(params), name
        for ctype, (ctext, nm) in zip(SIGNATURES[name], params):
            assert ctype is (ctypes.c_void_p if "*" in ctext else kinds[ctext]), (name, nm)
        assert name not in _RESTYPES
    assert [n for _, n in _params("pdg_boundary_vectors")] == [
        "n_nodes", "points", "dim", "n_faces", "faces", "bvec", "blen", "status", "scratch", "scratch_bytes", "stream"]
    assert [n for _, n in _params("pdg_boundary_residuals")] == [
        "n_graphs", "ptr", "sigma", "bvec", "blen", "labels", "rowptr_dst", "src", "perm", "edge_attr", "table",
        "argmax", "stream"]
    assert [n for _, n in _params("pdg_boundary_residuals_bwd")] == [
        "n_graphs", "ptr", "sigma", "bvec", "blen", "labels", "rowptr_dst", "src", "perm", "edge_attr", "table",
        "g_traction", "g_periodic", "out", "stream"]
    fw, bw = (dict((n, t) for t, n in _params(name)) for name in NAMES[1:])
    assert fw["table"] == "double*" and fw["argmax"] == "int*" and fw["labels"] == "const int64_t*"
    assert bw["table"] == bw["g_traction"] == bw["g_periodic"] == "const double*" and bw["out"] == "float*"
    assert SIGNATURES["pdg_boundary_vectors_scratch_bytes"] == [ctypes.c_int, ctypes.c_int]
    assert _RESTYPES["pdg_boundary_vectors_scratch_bytes"] is ctypes.c_long
    assert re.search(r"\blong\s+pdg_boundary_vectors_scratch_bytes\s*\(int n_nodes, int n_faces\)\s*;",
                     HEADER.read_text())


def test_header_states_the_conventions():
    text = " ".join(HEADER.read_text().split())
    for phrase in ("r = (yb - ya, -(xb - xa))", "r . (pc - pa) > 0", "ascending order of the edge's other endpoint",
                   "gets exact zeros", "lumped traction integral", "blen[n] > 0", "edge_attr is exactly 0",
                   "may all be NULL", "maximum would hide the NaN", "alone and inside any batch",
                   "appear in both directions", "either may be NULL (taken as 0)", "partial edge arguments",
                   "pdg_mesh_fields_scratch_bytes is unchanged"):
        assert phrase in text, phrase


def test_library_exports_the_boundary_calls():
    from pdg.lib import lib
    dll = lib.load()
    for name in NAMES + ("pdg_boundary_vectors_scratch_bytes",):
        assert hasattr(dll, name), name


def test_the_source_is_built_and_hashed():
    import build as pdg_build
    from pdg.lib import CSRC, lib, source_hash
    assert (CSRC / "pdg_boundary.hip").is_file()
    assert pdg_build.source_hash() == source_hash() == lib.pdg_source_hash().decode()


def test_scratch_sizes():
    """The boundary vectors size their own scratch (6 F endpoint slots twice over); the mesh fields' size is what
    it was: the maximum of the labels' and the operator's layouts, 256-byte aligned blocks."""
    from pdg.lib import lib
    own, old = lib.pdg_boundary_vectors_scratch_bytes, lib.pdg_mesh_fields_scratch_bytes
    assert own(100, 150) >= 8 * (6 + 3 + 6) * 150 + 4 * 3 * 150 + 4 * (4 * 100 + 2)
    assert own(100, 0) > 0 and own(0, 10) == -1 and own(10, -1) == -1 and own(10, 2 ** 31 // 9) == -1
    # the values the mesh fields' size function gave before the boundary vectors were added
    assert [old(100, 150), old(25556, 50000), old(7, 0)] == [24320, 7707392, 6400]


def _args(name, null=(), **vals):
    """Arguments of `name`: every pointer a distinct 16-byte-aligned fake address (never dereferenced: the checks
    run on the host before any HIP call) except those in `null` and the stream."""
    from pdg.lib import lib
    v = {"n_graphs": 3, "n_nodes": 100, "n_faces": 150, "dim": 2,
         "scratch_bytes": lib.pdg_boundary_vectors_scratch_bytes(100, 150)}
    v.update(vals)
    out = []
    for i, (ctext, nm) in enumerate(_params(name)):
        out.append((None if nm in null or nm == "stream" else 0x100000 + 0x1000 * i) if "*" in ctext else v[nm])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_boundary_calls_refuse_bad_arguments(name):
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
    if name == "pdg_boundary_vectors":
        for bad in ({"n_nodes": 0}, {"n_nodes": -1}, {"n_faces": -1}, {"dim": 1}, {"dim": 4}, {"n_faces": 2 ** 31 // 9}):
            with pytest.raises(PdgError, match="bad sizes"):
                fn(*_args(name, **bad))
        need = lib.pdg_boundary_vectors_scratch_bytes(100, 150)
        with pytest.raises(PdgError, match="scratch too small"):
            fn(*_args(name, scratch_bytes=need - 1))
        # faces may be NULL for a mesh without faces: the only refusal left is the one provoked here
        with pytest.raises(PdgError, match="scratch too small"):
            fn(*_args(name, null=("faces",), n_faces=0,
                      scratch_bytes=lib.pdg_boundary_vectors_scratch_bytes(100, 0) - 1))
        return
    for bad in (0, -1):
        with pytest.raises(PdgError, match="bad sizes"):
            fn(*_args(name, n_graphs=bad))
        # the sizes are refused first, whatever else is wrong; the optional pointers pass as NULL
        with pytest.raises(PdgError, match="bad sizes"):
            fn(*_args(name, null=OPTIONAL[name] + ("ptr",), n_graphs=bad))
    # the four edge arguments come together or not at all
    for k in range(1, 4):
        with pytest.raises(PdgError, match="partial edge arguments"):
            fn(*_args(name, null=EDGES[:k]))
        with pytest.raises(PdgError, match="partial edge arguments"):
            fn(*_args(name, null=EDGES[k:]))


def test_python_layer_refuses_cpu_tensors_bad_shapes_and_missing_vectors():
    import torch
    from gnn_local_stress import boundary as B
    from gnn_local_stress.models import EncodeProcessDecode
    from gnn_local_stress.sensitivity import boundary_gradients
    from pdg import devgraph, graph, meshgen
    sample = meshgen.hole_plate(5)
    b = graph.Batch.from_data_list([graph.sample_to_data(sample)])
    n = sample.num_nodes
    s = torch.zeros(n, 3)
    for call in (lambda: B.boundary_residuals(s, b), lambda: B.boundary_residuals_grad(s, b)):
        with pytest.raises(RuntimeError, match="HIP"):
            call()
    with pytest.raises(RuntimeError, match="device tensors"):
        devgraph.boundary_vectors(torch.zeros(4, 2), torch.zeros(2, 3, dtype=torch.int64))
    m = EncodeProcessDecode(1, 2, latent_size=128, input_nodes_features_size=6, output_nodes_features_size=3)
    with pytest.raises(RuntimeError, match="HIP"):
        boundary_gradients(m, b)
    assert "boundary_vec" in graph._NODE_KEYS and "boundary_len" in graph._NODE_KEYS
    # the batch carries host vectors through the collate as it does node_area
    bvec, blen = meshgen.boundary_vectors(sample.pos, sample.faces)
    datas = [graph.sample_to_data(sample) for _ in range(2)]
    for d in datas:
        d.boundary_vec, d.boundary_len = torch.from_numpy(bvec), torch.from_numpy(blen)
    both = graph.Batch.from_data_list(datas)
    assert both.boundary_vec.shape == (2 * n, 2) and both.boundary_len.shape == (2 * n,)
    assert torch.equal(both[1].boundary_vec, datas[1].boundary_vec)
    assert graph.Batch.from_data_list([datas[0], graph.sample_to_data(sample)]).boundary_vec is None
