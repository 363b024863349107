"""CPU-side checks of the fused physics loss's C ABI (pdg_phys_loss_fwd, pdg_phys_loss_bwd and pdg_loss_reduce_phys
in csrc/pdg_physloss.hip): declared, bound with matching pointer / integer kinds, exported, bad arguments refused
before any HIP call; and the Python layer's own refusals."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "pdivgnn.h"
NAMES = ("pdg_phys_loss_fwd", "pdg_phys_loss_bwd", "pdg_loss_reduce_phys")
BOUNDARY = ("bvec", "blen", "labels")
EDGES = ("rowptr_dst", "src", "perm", "edge_attr")
MEAN = ("area", "target")
OPTIONAL = BOUNDARY + EDGES + MEAN + ("denom",)
REQUIRED = {"pdg_phys_loss_fwd": ("ptr", "y", "affine", "table", "loss"),
            "pdg_phys_loss_bwd": ("ptr", "y", "affine", "table", "scale", "g_y")}
COMMON = ["bvec", "blen", "labels", "rowptr_dst", "src", "perm", "edge_attr", "area", "denom", "target"]


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


def test_header_and_signatures_hold_the_calls():
    from pdg.lib import _RESTYPES, SIGNATURES
    kinds = {"int": ctypes.c_int, "float": ctypes.c_float}
    for name in NAMES:
        params = _params(name)
        assert name in SIGNATURES, name
        assert len(SIGNATURES[name]) == len(params), name
        for ctype, (ctext, nm) in zip(SIGNATURES[name], params):
            assert ctype is (ctypes.c_void_p if "*" in ctext else kinds[ctext]), (name, nm)
        assert name not in _RESTYPES
    assert [n for _, n in _params("pdg_phys_loss_fwd")] == ["n_graphs", "ptr", "y", "affine"] + COMMON + [
        "table", "loss", "stream"]
    assert [n for _, n in _params("pdg_phys_loss_bwd")] == ["n_graphs", "ptr", "n_nodes", "y", "affine"] + COMMON + [
        "table", "scale", "accumulate", "g_y", "stream"]
    assert [n for _, n in _params("pdg_loss_reduce_phys")] == [
        "n_graphs", "loss_nmse", "loss_div", "loss_phys", "scale_nmse", "scale_div", "scale_phys", "zero_flag", "out",
        "stream"]
    fw, bw = (dict((n, t) for t, n in _params(name)) for name in NAMES[:2])
    assert fw["table"] == "double*" and fw["loss"] == "float*" and fw["denom"] == "const double*"
    assert fw["labels"] == "const int64_t*" and fw["affine"] == fw["target"] == "const float*"
    assert bw["table"] == "const double*" and bw["scale"] == "const float*" and bw["g_y"] == "float*"
    # the step's own reduce is left as it was
    assert [n for _, n in _params("pdg_loss_reduce")] == [
        "n_graphs", "loss_nmse", "loss_div", "scale_nmse", "scale_div", "zero_flag", "out", "stream"]


def test_header_states_the_conventions():
    text = " ".join(HEADER.read_text().split())
    for phrase in ("z = y + mean / std formed in fp64", "each given together or all NULL",
                   "a term whose denominator is not > 0 is absent", "its loss is exactly 0",
                   "A NaN in a participating input still gives a NaN loss", "(float)((double)g_y_old + term)",
                   "exactly 0 switches its term off", "alone and inside any batch", "a partial group"):
        assert phrase in text, phrase


def test_library_exports_the_calls():
    from pdg.lib import lib
    dll = lib.load()
    for name in NAMES:
        assert hasattr(dll, name), name


def test_the_source_is_built_and_hashed():
    import build as pdg_build
    from pdg.lib import CSRC, lib, source_hash
    assert (CSRC / "pdg_physloss.hip").is_file()
    assert pdg_build.source_hash() == source_hash() == lib.pdg_source_hash().decode()


def _args(name, null=(), **vals):
    """Arguments of `name`: every pointer a distinct 16-byte-aligned fake address (never dereferenced: the checks
    run on the host before any HIP call) except those in `null` and the stream."""
    v = {"n_graphs": 3, "n_nodes": 100, "accumulate": 1, "scale_nmse": 0.5, "scale_div": 0.5}
    v.update(vals)
    out = []
    for i, (ctext, nm) in enumerate(_params(name)):
        out.append((None if nm in null or nm == "stream" else 0x100000 + 0x1000 * i) if "*" in ctext else v[nm])
    return out


@pytest.mark.parametrize("name", NAMES[:2])
def test_calls_refuse_bad_arguments(name):
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-side argument checks only: never called with fake pointers where a GPU is present")
    from pdg.lib import PdgError, lib
    fn = getattr(lib, name)
    pointers = [nm for ctext, nm in _params(name) if "*" in ctext and nm != "stream"]
    assert sorted(pointers) == sorted(REQUIRED[name] + OPTIONAL)
    for nm in REQUIRED[name]:       # NULL table, loss, g_y among them
        with pytest.raises(PdgError, match="null argument"):
            fn(*_args(name, null=(nm,)))
        with pytest.raises(PdgError, match="null argument"):
            fn(*_args(name, null=OPTIONAL + (nm,)))
    for bad in (0, -1):
        with pytest.raises(PdgError, match="bad sizes"):
            fn(*_args(name, n_graphs=bad))
        # the sizes are refused first, whatever else is wrong; the optional pointers pass as NULL
        with pytest.raises(PdgError, match="bad sizes"):
            fn(*_args(name, null=OPTIONAL + ("ptr",), n_graphs=bad))
    if name == "pdg_phys_loss_bwd":
        for bad in (0, -5):
            with pytest.raises(PdgError, match="bad sizes"):
                fn(*_args(name, n_nodes=bad))
    # each group comes together or not at all
    for group, what in ((BOUNDARY, "partial boundary arguments"), (EDGES, "partial edge arguments"),
                        (MEAN, "partial mean arguments")):
        for k in range(1, len(group)):
            with pytest.raises(PdgError, match=what):
                fn(*_args(name, null=group[:k]))
            with pytest.raises(PdgError, match=what):
                fn(*_args(name, null=group[k:]))
    # denom goes with area and target only
    with pytest.raises(PdgError, match="partial mean arguments"):
        fn(*_args(name, null=MEAN))


def test_reduce_refuses_bad_arguments():
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-side argument checks only: never called with fake pointers where a GPU is present")
    from pdg.lib import PdgError, lib
    fn, name = lib.pdg_loss_reduce_phys, "pdg_loss_reduce_phys"
    for bad in (0, -1):
        with pytest.raises(PdgError, match="bad sizes"):
            fn(*_args(name, n_graphs=bad))
    for null in (("loss_nmse",), ("out",), ("loss_phys",), ("scale_phys",)):
        with pytest.raises(PdgError, match="null argument"):
            fn(*_args(name, null=null))


def test_python_layer_refusals():
    import torch
    from pdg import devgraph, graph, meshgen
    from pdg.trainer import PhysicsPenalty
    p = PhysicsPenalty()
    assert (p.traction, p.periodic, p.mean, p.convention) == (0.0, 0.0, 0.0, "cell") and not p.active
    assert PhysicsPenalty(mean=0.5, convention="material").active
    with pytest.raises(ValueError, match="convention"):
        PhysicsPenalty(convention="box")
    with pytest.raises(ValueError, match="negative"):
        PhysicsPenalty(traction=-1.0)
    d = graph.sample_to_data(meshgen.hole_plate(5))
    with pytest.raises(RuntimeError, match="HIP"):
        devgraph.attach_mesh_fields(d, "cpu")
    d.face = None
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="face"):
            devgraph.attach_mesh_fields(d, "cuda")
