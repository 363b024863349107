"""CPU-side checks of the C ABI for faces of nv vertices (the *_cells entry points of csrc/pdg_graph.hip and
csrc/pdg_meshfields.hip): declared, exported, bound; scratch sizing is host arithmetic that grows with nv and equals
the triangle functions' at nv = 3; arguments are refused on the host before any HIP call."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "pdivgnn.h"
SIZES = {"pdg_mesh_graph_cells_scratch_bytes": "pdg_mesh_graph_scratch_bytes",
         "pdg_mesh_fields_cells_scratch_bytes": "pdg_mesh_fields_scratch_bytes",
         "pdg_boundary_vectors_cells_scratch_bytes": "pdg_boundary_vectors_scratch_bytes"}
CALLS = {"pdg_mesh_graph_cells": "pdg_mesh_graph", "pdg_node_labels_cells": "pdg_node_labels",
         "pdg_div_operator_cells": "pdg_p1_div_operator", "pdg_nodal_areas_cells": "pdg_nodal_areas",
         "pdg_boundary_vectors_cells": "pdg_boundary_vectors"}


def _params(name):
    """(is pointer, name) of every parameter of `name` in include/pdivgnn.h."""
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    m = re.search(rf"\b(?:int|long)\s+{name}\s*\(([^)]*)\)\s*;", text, re.S)
    assert m, name
    return [("*" in a, re.findall(r"\w+", a)[-1]) for a in m.group(1).split(",")]


def test_header_signatures_and_library_hold_the_cells_entry_points():
    from pdg.lib import _RESTYPES, SIGNATURES, lib
    dll = lib.load()
    for name, old in {**SIZES, **CALLS}.items():
        params = _params(name)
        assert hasattr(dll, name), name
        assert len(SIGNATURES[name]) == len(params), name
        for ctype, (is_ptr, nm) in zip(SIGNATURES[name], params):
            assert (ctype is ctypes.c_void_p) == is_ptr, (name, nm)
        # the triangle call's parameters with `int nv` after n_faces
        names = [nm for _, nm in params]
        want = [nm for _, nm in _params(old)]
        k = want.index("n_faces") + 1
        assert names == want[:k] + ["nv"] + want[k:], name
    for name in SIZES:
        assert _RESTYPES[name] is ctypes.c_long
    for name in CALLS:
        assert name not in _RESTYPES


def test_scratch_sizes_are_host_arithmetic_that_grows_with_nv():
    from pdg.lib import lib
    meshes = [(1, 0), (1, 1), (100, 150), (1521, 1444), (25556, 50000)]
    for name, old in SIZES.items():
        f, f3 = getattr(lib, name), getattr(lib, old)
        for n, nf in meshes:
            assert f(n, nf, 3) == f3(n, nf) > 0, (name, n, nf)            # the sizes the triangle calls always had
            assert f(n, nf, 4) >= f(n, nf, 3), (name, n, nf)
        assert f(25556, 50000, 4) > f(25556, 50000, 3)
        for nv in (0, 2, 5, -4):
            assert f(100, 150, nv) < 0, (name, nv)
        assert f(0, 10, 4) < 0 and f(10, -1, 4) < 0
    # the operator's nv^2 F pairs, unsorted and sorted, as 64-bit slots
    assert lib.pdg_mesh_fields_cells_scratch_bytes(1600, 1500, 4) >= 2 * 8 * 16 * 1500
    # nv^2 n_faces + 1024 must stay below 2^31: a face count the triangle call takes is too many quads
    nf = 2 ** 31 // 16
    assert lib.pdg_mesh_fields_scratch_bytes(10, nf) > 0 and lib.pdg_mesh_fields_cells_scratch_bytes(10, nf, 3) > 0
    assert lib.pdg_mesh_fields_cells_scratch_bytes(10, nf, 4) < 0
    assert lib.pdg_boundary_vectors_cells_scratch_bytes(10, nf, 4) < 0


def _args(name, null=None, **ints):
    """Arguments of `name`: sizes of a small quad mesh, every pointer a distinct fake address (never dereferenced:
    the checks run on the host before any HIP call) except `null` and the stream."""
    from pdg.lib import lib
    size = {"pdg_mesh_graph_cells": lib.pdg_mesh_graph_cells_scratch_bytes,
            "pdg_boundary_vectors_cells": lib.pdg_boundary_vectors_cells_scratch_bytes}.get(
                name, lib.pdg_mesh_fields_cells_scratch_bytes)
    vals = {"n_nodes": 100, "n_faces": 81, "nv": 4, "dim": 2, "periodic": 0,
            "capacity": 32 * 81 if name == "pdg_div_operator_cells" else 8 * 81}
    vals.update(ints)
    vals.setdefault("scratch_bytes", size(100, 81, 4))
    out = []
    for i, (is_ptr, nm) in enumerate(_params(name)):
        out.append((None if nm in (null, "stream") else 0x100000 + 0x1000 * i) if is_ptr else vals[nm])
    return out


@pytest.mark.parametrize("name", sorted(CALLS))
def test_cells_entry_points_refuse_bad_arguments(name):
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-side argument checks only: never called with fake pointers where a GPU is present")
    from pdg.lib import PdgError, lib
    fn = getattr(lib, name)
    for nv in (5, 2, 0, -3):
        with pytest.raises(PdgError, match="nv must be 3"):
            fn(*_args(name, nv=nv))
    for bad in ({"n_nodes": 0}, {"n_nodes": -1}, {"n_faces": -1}, {"dim": 1}, {"dim": 4}):
        with pytest.raises(PdgError, match="bad sizes"):
            fn(*_args(name, **bad))
    if name != "pdg_mesh_graph_cells":
        with pytest.raises(PdgError, match="bad sizes"):
            fn(*_args(name, n_faces=2 ** 31 // 16))
    for is_ptr, nm in _params(name):
        if is_ptr and nm != "stream":
            with pytest.raises(PdgError, match="null argument"):
                fn(*_args(name, null=nm))
    need = _args(name)[[nm for _, nm in _params(name)].index("scratch_bytes")]
    with pytest.raises(PdgError, match="scratch too small"):
        fn(*_args(name, scratch_bytes=need - 1))
    # a scratch sized for triangles does not serve quads
    small = {"pdg_mesh_graph_cells": lib.pdg_mesh_graph_scratch_bytes,
             "pdg_boundary_vectors_cells": lib.pdg_boundary_vectors_scratch_bytes}.get(
                 name, lib.pdg_mesh_fields_scratch_bytes)(100, 81)
    assert small < need
    with pytest.raises(PdgError, match="scratch too small"):
        fn(*_args(name, scratch_bytes=small))
    if name == "pdg_div_operator_cells":
        with pytest.raises(PdgError, match="capacity below 32"):
            fn(*_args(name, capacity=32 * 81 - 1))
    if name == "pdg_mesh_graph_cells":
        with pytest.raises(PdgError, match="capacity below 8"):
            fn(*_args(name, capacity=8 * 81 - 1))
        with pytest.raises(PdgError, match="capacity"):
            fn(*_args(name, periodic=1))                       # no room for the periodic pairs
