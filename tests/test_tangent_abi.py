"""CPU-side checks of the tangent-pass entry points (csrc/pdg_tangent.hip): declared in include/pdivgnn.h,
exported by the library, bound with matching ctypes signatures, and refusing bad arguments on the host before
any HIP call."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "pdivgnn.h"
# name -> its row-count arguments
NAMES = {
    "pdg_node_enc_tan": ("n_nodes",), "pdg_edge_enc_tan": ("n_edges",), "pdg_node_pre_tan": ("n_nodes",),
    "pdg_edge_tan": ("n_edges", "n_nodes"), "pdg_segment_sum_tan": ("n_nodes", "n_edges"),
    "pdg_node_net_tan": ("n_nodes",), "pdg_decoder_tan": ("n_nodes",), "pdg_edge_len_tan": ("n_edges", "n_nodes"),
}
INTS = {"n_edges": 1000, "n_nodes": 300, "nblocks": 256, "npairs": 4, "scale_output": 1, "with_edge_update": 1}
# every pointer but these is required (the residuals: absent at step 0; std_out: with scale_output; the edge
# update's operands: with_edge_update, both covered below)
OPTIONAL = {"dx_res", "de_res", "stream"}
ROW_KERNELS = [n for n in NAMES if n != "pdg_edge_len_tan"]


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


def _all_null(name, **ints):
    return [None if kind == "ptr" else ints.get(nm, INTS[nm]) for kind, nm in _params(name)]


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_bound(name):
    from pdg.lib import SIGNATURES, lib
    params = _params(name)
    assert hasattr(lib.load(), name)
    assert name in SIGNATURES and len(SIGNATURES[name]) == len(params)
    for (kind, nm), ct in zip(params, SIGNATURES[name]):
        assert (ct is ctypes.c_void_p) == (kind == "ptr"), (name, nm)
    assert [nm for _, nm in params][-1] == "stream"
    assert ("nblocks" in [nm for _, nm in params]) == (name in ROW_KERNELS)


@pytest.mark.parametrize("name", NAMES)
def test_non_positive_sizes_are_refused(name):
    """With every pointer NULL as well: nothing could be launched even if the size check were missing."""
    from pdg.lib import PdgError, lib
    for size in NAMES[name]:
        for v in (0, -5):
            with pytest.raises(PdgError, match="must be"):
                getattr(lib, name)(*_all_null(name, **{size: v}))


@pytest.mark.parametrize("name", ROW_KERNELS)
def test_row_count_bound_and_bad_nblocks_are_refused(name):
    """A block's buffer resources span rows x 512 bytes in an int: 2^22 rows and more are refused; nblocks
    outside 1 .. pdg_max_blocks() is refused."""
    from pdg.lib import PdgError, lib
    for size in NAMES[name]:
        with pytest.raises(PdgError, match="must be"):
            getattr(lib, name)(*_all_null(name, **{size: 1 << 22}))
    for v in (0, -1, lib.pdg_max_blocks() + 1, 1 << 20):
        with pytest.raises(PdgError, match="bad sizes"):
            getattr(lib, name)(*_all_null(name, nblocks=v))
    if "npairs" in [nm for _, nm in _params(name)]:
        for v in (0, -1, lib.pdg_max_blocks() + 1):
            with pytest.raises(PdgError, match="bad sizes"):
                getattr(lib, name)(*_all_null(name, npairs=v))


@pytest.mark.parametrize("name", NAMES)
def test_null_required_arguments_are_refused(name):
    """Each required pointer in turn NULL, the others fake addresses: refused on the host."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-side argument checks only: never called with fake pointers where a GPU is present")
    from pdg.lib import PdgError, lib
    required = [nm for kind, nm in _params(name) if kind == "ptr" and nm not in OPTIONAL]
    assert len(required) >= 6
    for nm in required:
        with pytest.raises(PdgError, match="null argument"):
            getattr(lib, name)(*_args(name, nm))
    if name == "pdg_decoder_tan":
        # std_out may be NULL only without scale_output; then the next required pointer refuses
        with pytest.raises(PdgError, match="null argument"):
            args = _args(name, "std_out", scale_output=0)
            args[[nm for _, nm in _params(name)].index("dy")] = None
            lib.pdg_decoder_tan(*args)
    if name == "pdg_edge_tan":
        # the edge update's operands may be NULL only without with_edge_update; then part_m refuses
        names = [nm for _, nm in _params(name)]
        args = _args(name, with_edge_update=0)
        for nm in ("a1e", "a2e", "st_e", "da2e", "part_e", "part_m"):
            args[names.index(nm)] = None
        with pytest.raises(PdgError, match="null argument"):
            lib.pdg_edge_tan(*args)
