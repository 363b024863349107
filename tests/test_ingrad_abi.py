"""CPU-side checks of the input-gradient entry points (csrc/pdg_ingrad.hip): declared in
include/pdivgnn.h, exported by the library, bound with matching ctypes signatures, and refusing bad
arguments on the host before any HIP call."""
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "pdivgnn.h"
NAMES = ("pdg_edge_enc_gin", "pdg_node_enc_gin", "pdg_graph_colsum3")
INTS = {"n_edges": 1000, "n_nodes": 1000, "n_graphs": 3, "nblocks": 256, "lb_npairs": 4, "scale_input": 1}
# every pointer but these is required (lb or lb_pairs: one of the two; stats8: with scale_input)
OPTIONAL = {"lb", "stream"}


def _params(name):
    """(kind, name) of every parameter of `name` in the header."""
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", text, re.S)
    assert m, f"{name} is not declared in include/pdivgnn.h"
    out = []
    for a in m.group(1).split(","):
        a = a.strip()
        out.append(("ptr" if "*" in a else "int", re.findall(r"\w+", a)[-1]))
    return out


def _args(name, null=None, **ints):
    """Arguments with every pointer a distinct 16-byte-aligned fake address (never dereferenced: the checks
    run on the host before any HIP call) except `null` and the optional ones, which are NULL."""
    out = []
    for i, (kind, nm) in enumerate(_params(name)):
        if kind == "ptr":
            out.append(None if nm == null or nm in OPTIONAL else 0x100000 + 0x1000 * i)
        else:
            out.append(ints.get(nm, INTS[nm]))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_bound(name):
    from pdg.lib import SIGNATURES, lib
    params = _params(name)
    assert hasattr(lib.load(), name)
    assert name in SIGNATURES and len(SIGNATURES[name]) == len(params)
    import ctypes
    for (kind, nm), ct in zip(params, SIGNATURES[name]):
        assert (ct is ctypes.c_void_p) == (kind == "ptr"), (name, nm)


@pytest.mark.parametrize("name,size", [("pdg_edge_enc_gin", "n_edges"), ("pdg_node_enc_gin", "n_nodes"),
                                       ("pdg_graph_colsum3", "n_graphs")])
def test_non_positive_sizes_are_refused(name, size):
    """With every pointer NULL as well: nothing could be launched even if the size check were missing."""
    from pdg.lib import PdgError, lib
    for v in (0, -5):
        args = [None if kind == "ptr" else (v if nm == size else INTS[nm]) for kind, nm in _params(name)]
        with pytest.raises(PdgError, match="must be"):
            getattr(lib, name)(*args)
    if name != "pdg_graph_colsum3":
        for v in (0, -1, 1 << 20):
            args = [None if kind == "ptr" else (v if nm == "nblocks" else INTS[nm]) for kind, nm in _params(name)]
            with pytest.raises(PdgError, match="bad sizes"):
                getattr(lib, name)(*args)


@pytest.mark.parametrize("name", NAMES)
def test_null_required_arguments_are_refused(name):
    """Each required pointer in turn NULL, the others fake addresses: refused on the host."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-side argument checks only: never called with fake pointers where a GPU is present")
    from pdg.lib import PdgError, lib
    required = [nm for kind, nm in _params(name) if kind == "ptr" and nm not in OPTIONAL]
    assert len(required) >= 3
    for nm in required:
        with pytest.raises(PdgError, match="null argument"):
            getattr(lib, name)(*_args(name, nm))
    if name != "pdg_graph_colsum3":
        # stats8 may be NULL only without scale_input; then the next check (lb / lb_pairs both NULL) refuses
        with pytest.raises(PdgError, match="null argument"):
            getattr(lib, name)(*_args(name, "lb_pairs", scale_input=0))
