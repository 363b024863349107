"""CPU-side checks of the device graph planner's C ABI (csrc/pdg_plan.hip): declared, bound,
scratch sizing is host arithmetic, and arguments are refused before any HIP call."""
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "pdivgnn.h"
NAMES = ("pdg_graph_plan_scratch_bytes", "pdg_graph_plan", "pdg_div_plan")


def _params(name):
    """(is pointer, name) of every parameter of `name` in include/pdivgnn.h."""
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    m = re.search(rf"\b(?:int|long)\s+{name}\s*\(([^)]*)\)\s*;", text, re.S)
    assert m, name
    return [("*" in a, re.findall(r"\w+", a)[-1]) for a in m.group(1).split(",")]


def test_header_and_signatures_hold_the_planner():
    from pdg.lib import _RESTYPES, SIGNATURES
    for name in NAMES:
        assert len(SIGNATURES[name]) == len(_params(name)), name
    assert "pdg_graph_plan_scratch_bytes" in _RESTYPES
    names = [n for _, n in _params("pdg_graph_plan")]
    for out in ("perm", "src", "dst", "rowptr_dst", "perm_src", "rowptr_src", "status"):
        assert out in names
    names = [n for _, n in _params("pdg_div_plan")]
    for out in ("a_rowptr", "a_col", "a_val", "at_rowptr", "at_row", "at_comp", "at_val", "status"):
        assert out in names


def test_library_exports_the_planner():
    from pdg.lib import lib
    dll = lib.load()
    for name in NAMES:
        assert hasattr(dll, name), name


def test_scratch_bytes_is_host_arithmetic():
    from pdg.lib import lib
    f = lib.pdg_graph_plan_scratch_bytes
    n, e, nnz = 5041, 29968, 60000
    # the packed 64-bit slots of the larger grouping, two fill counters per node, the scan's block sums
    assert f(n, e, nnz) >= 8 * max(e, nnz) + 4 * 2 * n + 4 * ((n + 1023) // 1024 + 1)
    assert f(n, e, 0) >= 8 * e + 4 * 2 * n + 4 * ((n + 1023) // 1024 + 1)
    assert f(n, 2 * e, 0) > f(n, e, 0) and f(2 * n, e, 0) > f(n, e, 0) and f(n, e, 4 * e) > f(n, e, 0)
    assert f(7, 0, 0) > 0
    for bad in ((0, 10, 0), (-3, 10, 0), (10, -1, 0), (10, 0, -1), (10, 2 ** 31, 0), (2 ** 31 - 2, 10, 0)):
        assert f(*bad) < 0, bad


def _args(name, null=None, scratch_bytes=None):
    """Arguments of `name`: sizes of a small graph, every pointer a distinct fake address (never
    dereferenced: the checks run on the host before any HIP call) except `null` and the stream."""
    from pdg.lib import lib
    ints = {"n_nodes": 100, "n_edges": 600, "n_graphs": 2, "nnz": 900, "clear_status": 1,
            "scratch_bytes": lib.pdg_graph_plan_scratch_bytes(100, 600, 900)}
    if scratch_bytes is not None:
        ints["scratch_bytes"] = scratch_bytes
    out = []
    for i, (is_ptr, nm) in enumerate(_params(name)):
        out.append((None if nm in (null, "stream") else 0x100000 + 0x1000 * i) if is_ptr else ints[nm])
    return out


@pytest.mark.parametrize("name", ["pdg_graph_plan", "pdg_div_plan"])
def test_planner_refuses_null_and_small_scratch(name):
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-side argument checks only: never called with fake pointers where a GPU is present")
    from pdg.lib import PdgError, lib
    fn = getattr(lib, name)
    for is_ptr, nm in _params(name):
        if is_ptr and nm != "stream":
            with pytest.raises(PdgError, match="null argument"):
                fn(*_args(name, null=nm))
    need = lib.pdg_graph_plan_scratch_bytes(100, 600 if name == "pdg_graph_plan" else 0,
                                            0 if name == "pdg_graph_plan" else 900)
    with pytest.raises(PdgError, match="scratch too small"):
        fn(*_args(name, scratch_bytes=need - 1))
    with pytest.raises(PdgError, match="bad sizes"):
        fn(*[0 if nm == "n_nodes" else a for a, (_, nm) in zip(_args(name), _params(name))])
    with pytest.raises(PdgError, match="bad sizes"):
        fn(*[2 ** 31 if nm in ("n_edges", "nnz") else a for a, (_, nm) in zip(_args(name), _params(name))])
