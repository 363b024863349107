"""CPU-side checks of the C ABI of the sampling operator (csrc/pdg_sample.hip): declared, exported, bound with
matching pointer and integer parameters; the scratch sizes are host arithmetic, positive, monotone and negative on
bad sizes; every limit is refused on the host before any HIP call."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "pdivgnn.h"
SIZES = ("pdg_cell_bins_scratch_bytes", "pdg_sample_csr_scratch_bytes")
CALLS = ("pdg_cell_bins", "pdg_locate_points", "pdg_sample_field", "pdg_sample_csr", "pdg_sample_field_bwd")
INT_TYPES = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float}


def _params(name):
    """(C type or '*', name) of every parameter of `name` in include/pdivgnn.h."""
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    m = re.search(rf"\b(?:int|long)\s+{name}\s*\(([^)]*)\)\s*;", text, re.S)
    assert m, name
    out = []
    for a in m.group(1).split(","):
        words = re.findall(r"\w+", a)
        out.append(("*" if "*" in a else words[-2], words[-1]))
    return out


def test_header_signatures_and_library_hold_the_sampling_entry_points():
    from pdg.lib import _RESTYPES, SIGNATURES, lib
    dll = lib.load()
    for name in SIZES + CALLS:
        params = _params(name)
        assert hasattr(dll, name), name
        assert len(SIGNATURES[name]) == len(params), name
        for ctype, (kind, nm) in zip(SIGNATURES[name], params):
            assert ctype is (ctypes.c_void_p if kind == "*" else INT_TYPES[kind]), (name, nm)
    for name in CALLS:
        assert name not in _RESTYPES
        names = [nm for _, nm in _params(name)]
        assert names[-1] == "stream"
        if "n_faces" in names:
            assert names[names.index("n_faces") + 1] == "nv", name       # `int nv` follows n_faces
    for name in SIZES:
        assert _RESTYPES[name] is ctypes.c_long


def test_scratch_sizes_are_host_arithmetic():
    from pdg.lib import lib
    bins, csr = lib.pdg_cell_bins_scratch_bytes, lib.pdg_sample_csr_scratch_bytes
    last = 0
    for g in (1, 2, 7, 33, 160, 1024):
        assert bins(g, g) >= last > -1 and bins(g, g) >= bins(g, 1) > 0 and bins(g, g) >= bins(1, g) > 0
        last = bins(g, g)
    assert bins(1024, 1024) >= 4 * 1024 * 1024                           # one fill counter per bin
    for bad in ((0, 4), (4, 0), (-1, 4), (4, -3), (46341, 46341), (2 ** 16, 2 ** 15)):
        assert bins(*bad) < 0, bad
    assert bins(46340, 46340) > 0                                        # 46340^2 + 1024 < 2^31
    for nv in (3, 4):
        last = 0
        for n, nq in ((1, 0), (1, 1), (100, 257), (1521, 4096), (25556, 2 ** 20)):
            assert csr(n, nq, nv) >= last and csr(n, nq, nv) > 0
            last = csr(n, nq, nv)
        assert csr(25556, 2 ** 20, nv) >= 8 * nv * 2 ** 20               # a 64-bit slot per (query, vertex)
        assert csr(100, 2 ** 31 // nv - 1, nv) > 0 and csr(100, 2 ** 31 // nv + 1, nv) < 0
        assert csr(0, 10, nv) < 0 and csr(10, -1, nv) < 0 and csr(2 ** 31 - 1024, 10, nv) < 0
    assert csr(100, 1000, 4) >= csr(100, 1000, 3)
    for nv in (0, 2, 5, -4):
        assert csr(100, 10, nv) < 0


VALS = {"n_nodes": 100, "n_faces": 81, "nv": 4, "dim": 2, "periodic": 0, "gx": 7, "gy": 7, "capacity": 600,
        "n_q": 257, "n_rows": 100, "n_cols": 3, "node_offset": 0, "fill": 0.0}


def _args(name, null=None, **over):
    """Arguments of `name`: sizes of a small quad mesh, every pointer a distinct fake address (never dereferenced:
    the checks run on the host before any HIP call) except `null` and the stream."""
    from pdg.lib import lib
    vals = dict(VALS)
    vals.update(over)
    if "scratch_bytes" not in vals:
        vals["scratch_bytes"] = (lib.pdg_cell_bins_scratch_bytes(7, 7) if name == "pdg_cell_bins"
                                 else lib.pdg_sample_csr_scratch_bytes(100, 257, 4))
    out = []
    for i, (kind, nm) in enumerate(_params(name)):
        out.append((None if nm in (null, "stream") else 0x100000 + 0x1000 * i) if kind == "*" else vals[nm])
    return out


BAD_SIZES = {
    "pdg_cell_bins": [{"n_nodes": 0}, {"n_faces": -1}, {"dim": 1}, {"dim": 4}, {"gx": 0}, {"gy": 0}, {"gy": -2},
                      {"gx": 46341, "gy": 46341}, {"capacity": 0}, {"capacity": 2 ** 31},
                      {"n_faces": 2 ** 31 // 4}],
    "pdg_locate_points": [{"n_nodes": 0}, {"n_faces": -1}, {"dim": 1}, {"dim": 4}, {"gx": 0}, {"gy": 0},
                          {"gx": 46341, "gy": 46341}, {"capacity": 0}, {"capacity": 2 ** 31}, {"n_q": -1},
                          {"n_q": 2 ** 31 // 4}],
    "pdg_sample_field": [{"n_q": -1}, {"n_q": 2 ** 31 // 4}, {"n_faces": -1}, {"n_rows": 0}, {"n_cols": 0},
                         {"n_cols": -1}, {"node_offset": -1}, {"node_offset": 100}],
    "pdg_sample_csr": [{"n_nodes": 0}, {"n_faces": -1}, {"n_q": -1}, {"n_q": 2 ** 31 // 4},
                       {"n_nodes": 2 ** 31 - 1024}],
    "pdg_sample_field_bwd": [{"n_nodes": 0}, {"n_q": -1}, {"n_q": 2 ** 31 // 4}, {"n_cols": 0}],
}


@pytest.mark.parametrize("name", CALLS)
def test_sampling_entry_points_refuse_bad_arguments(name):
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-side argument checks only: never called with fake pointers where a GPU is present")
    from pdg.lib import PdgError, lib
    fn = getattr(lib, name)
    for nv in (5, 2, 0, -3):
        with pytest.raises(PdgError, match="nv must be 3"):
            fn(*_args(name, nv=nv))
    for bad in BAD_SIZES[name]:
        with pytest.raises(PdgError, match="bad sizes"):
            fn(*_args(name, **bad))
    # n_q * nv just below 2^31 passes the size check (and is then refused for a null pointer, not for its size)
    if name != "pdg_cell_bins":
        with pytest.raises(PdgError, match="null argument"):
            fn(*_args(name, null="cell" if name != "pdg_sample_field_bwd" else "rowptr", n_q=2 ** 31 // 4 - 1))
    for kind, nm in _params(name):
        if kind == "*" and nm != "stream":
            with pytest.raises(PdgError, match="null argument"):
                fn(*_args(name, null=nm))
    if "scratch_bytes" in [nm for _, nm in _params(name)]:
        need = _args(name)[[nm for _, nm in _params(name)].index("scratch_bytes")]
        with pytest.raises(PdgError, match="scratch too small"):
            fn(*_args(name, scratch_bytes=need - 1))
        with pytest.raises(PdgError, match="scratch too small"):
            fn(*_args(name, scratch_bytes=0))
