"""CPU-side checks of the mesh-field C ABI (csrc/pdg_meshfields.hip): declared, bound, scratch
sizing is host arithmetic, and arguments are refused before any HIP call."""
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "pdivgnn.h"
NAMES = ("pdg_mesh_fields_scratch_bytes", "pdg_node_labels", "pdg_p1_div_operator")


def _params(name):
    """(is pointer, name) of every parameter of `name` in include/pdivgnn.h."""
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    m = re.search(rf"\b(?:int|long)\s+{name}\s*\(([^)]*)\)\s*;", text, re.S)
    assert m, name
    return [("*" in a, re.findall(r"\w+", a)[-1]) for a in m.group(1).split(",")]


def test_header_and_signatures_hold_the_mesh_fields():
    import ctypes
    from pdg.lib import _RESTYPES, SIGNATURES
    for name in NAMES:
        params = _params(name)
        assert len(SIGNATURES[name]) == len(params), name
        for ctype, (is_ptr, nm) in zip(SIGNATURES[name], params):
            assert (ctype is ctypes.c_void_p) == is_ptr, (name, nm)
    assert _RESTYPES["pdg_mesh_fields_scratch_bytes"] is ctypes.c_long
    assert "pdg_node_labels" not in _RESTYPES and "pdg_p1_div_operator" not in _RESTYPES
    names = [n for _, n in _params("pdg_node_labels")]
    for arg in ("points", "dim", "faces", "labels", "info", "scratch", "scratch_bytes", "stream"):
        assert arg in names
    names = [n for _, n in _params("pdg_p1_div_operator")]
    for arg in ("points", "faces", "rows", "cols", "vals", "capacity", "nnz", "status", "scratch", "stream"):
        assert arg in names


def test_header_states_the_deliberate_deviations():
    text = " ".join(HEADER.read_text().split())
    assert "x == ymin" in text and "deliberate" in text
    assert "divides by zero" in text


def test_library_exports_the_mesh_fields():
    from pdg.lib import lib
    dll = lib.load()
    for name in NAMES:
        assert hasattr(dll, name), name


def test_scratch_bytes_is_host_arithmetic():
    from pdg.lib import lib
    f = lib.pdg_mesh_fields_scratch_bytes
    n, nf = 25556, 50000
    # the operator's 9 F pairs, unsorted and sorted, as 64-bit slots; the labels' per-node arrays
    assert f(n, nf) >= 2 * 8 * 9 * nf
    assert f(n, 0) >= 4 * 6 * n
    assert f(7, 0) > 0 and f(1, 1) > 0
    sizes = [(1, 0), (1, 1), (100, 0), (100, 150), (100, 151), (101, 151), (5041, 9800), (25556, 50000)]
    for a, b in zip(sizes, sizes[1:]):
        assert f(*a) <= f(*b), (a, b)
    assert f(n, 2 * nf) > f(n, nf) and f(40 * n, nf) > f(n, nf)
    for bad in ((0, 10), (-3, 10), (10, -1), (2 ** 31 - 2, 10), (10, 2 ** 31 // 9)):
        assert f(*bad) < 0, bad


def _args(name, null=None, **ints):
    """Arguments of `name`: sizes of a small mesh, every pointer a distinct fake address (never
    dereferenced: the checks run on the host before any HIP call) except `null` and the stream."""
    from pdg.lib import lib
    vals = {"n_nodes": 100, "n_faces": 150, "dim": 2, "capacity": 18 * 150,
            "scratch_bytes": lib.pdg_mesh_fields_scratch_bytes(100, 150)}
    vals.update(ints)
    out = []
    for i, (is_ptr, nm) in enumerate(_params(name)):
        out.append((None if nm in (null, "stream") else 0x100000 + 0x1000 * i) if is_ptr else vals[nm])
    return out


@pytest.mark.parametrize("name", ["pdg_node_labels", "pdg_p1_div_operator"])
def test_mesh_fields_refuse_bad_arguments(name):
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-side argument checks only: never called with fake pointers where a GPU is present")
    from pdg.lib import PdgError, lib
    fn = getattr(lib, name)
    for is_ptr, nm in _params(name):
        if is_ptr and nm != "stream":
            with pytest.raises(PdgError, match="null argument"):
                fn(*_args(name, null=nm))
    need = lib.pdg_mesh_fields_scratch_bytes(100, 150)
    with pytest.raises(PdgError, match="scratch too small"):
        fn(*_args(name, scratch_bytes=need - 1))
    for bad in ({"n_nodes": 0}, {"n_nodes": -1}, {"n_faces": -1}, {"dim": 1}, {"dim": 4},
                {"n_faces": 2 ** 31 // 9}):
        with pytest.raises(PdgError, match="bad sizes"):
            fn(*_args(name, **bad))
    if name == "pdg_p1_div_operator":
        with pytest.raises(PdgError, match="capacity"):
            fn(*_args(name, capacity=18 * 150 - 1))
