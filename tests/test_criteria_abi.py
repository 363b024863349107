"""CPU-side checks of the stress-criteria C ABI (csrc/pdg_criteria.hip): declared, bound with matching pointer /
integer / double kinds, exported, and bad arguments refused before any HIP call; the Python layer's own refusals."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "pdivgnn.h"
NAMES = ("pdg_stress_criteria", "pdg_stress_criteria_bwd")
OPTIONAL = {"pdg_stress_criteria": ("weights", "fields"), "pdg_stress_criteria_bwd": ("weights", "g_value")}
REQUIRED = {"pdg_stress_criteria": ("ptr", "sigma", "table", "argmax"),
            "pdg_stress_criteria_bwd": ("ptr", "sigma", "table", "argmax", "g_sigma")}


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


def test_header_and_signatures_hold_the_criteria():
    from pdg.lib import _RESTYPES, SIGNATURES
    for name in NAMES:
        params = _params(name)
        assert name in SIGNATURES, name
        assert len(SIGNATURES[name]) == len(params), name
        for ctype, (ctext, nm) in zip(SIGNATURES[name], params):
            want = ctypes.c_void_p if "*" in ctext else {"int": ctypes.c_int, "double": ctypes.c_double}[ctext]
            assert ctype is want, (name, nm)
        assert name not in _RESTYPES
    assert [n for _, n in _params("pdg_stress_criteria")] == [
        "n_graphs", "ptr", "sigma", "weights", "criterion", "p", "rho", "table", "argmax", "fields", "stream"]
    assert [n for _, n in _params("pdg_stress_criteria_bwd")] == [
        "n_graphs", "ptr", "sigma", "weights", "criterion", "aggregate", "p", "rho", "table", "argmax", "g_value",
        "g_sigma", "stream"]
    fwd, bwd = (dict((n, t) for t, n in _params(name)) for name in NAMES)
    assert fwd["table"] == "double*" and fwd["argmax"] == "int*" and fwd["fields"] == "float*"
    assert bwd["table"] == "const double*" and bwd["argmax"] == "const int*" and bwd["g_sigma"] == "float*"
    assert fwd["p"] == fwd["rho"] == bwd["p"] == bwd["rho"] == "double"


def test_header_states_the_conventions():
    text = " ".join(HEADER.read_text().split())
    for phrase in ("datasets.py:82", "max(2 r, |s1|, |s2|)", "the first winning an exact tie", "sign(0) = 0",
                   "weight is > 0", "a subgradient", "one block sum"):
        assert phrase in text, phrase


def test_library_exports_the_criteria():
    from pdg.lib import lib
    dll = lib.load()
    for name in NAMES:
        assert hasattr(dll, name), name


def _args(name, null=(), **vals):
    """Arguments of `name`: every pointer a distinct 16-byte-aligned fake address (never dereferenced: the checks
    run on the host before any HIP call) except those in `null` and the stream."""
    v = {"n_graphs": 3, "criterion": 1, "aggregate": 2, "p": 8.0, "rho": 0.5}
    v.update(vals)
    out = []
    for i, (ctext, nm) in enumerate(_params(name)):
        out.append((None if nm in null or nm == "stream" else 0x100000 + 0x1000 * i) if "*" in ctext else v[nm])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_criteria_refuse_bad_arguments(name):
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
        # with every optional pointer NULL too: only the required one is refused
        with pytest.raises(PdgError, match="null argument"):
            fn(*_args(name, null=OPTIONAL[name] + (nm,)))
    for bad in (0, -1):
        with pytest.raises(PdgError, match="n_graphs must be > 0"):
            fn(*_args(name, n_graphs=bad))
        # the size is refused first, whatever else is wrong
        with pytest.raises(PdgError, match="n_graphs must be > 0"):
            fn(*_args(name, null=("ptr", "table"), n_graphs=bad, criterion=7))
    for bad in (3, -1):
        with pytest.raises(PdgError, match="criterion must be 0, 1 or 2"):
            fn(*_args(name, criterion=bad))
    for bad in (0.5, float("inf"), float("nan"), -2.0):
        with pytest.raises(PdgError, match="p must be finite and >= 1"):
            fn(*_args(name, p=bad))
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(PdgError, match="rho must be finite and > 0"):
            fn(*_args(name, rho=bad))
    if name == "pdg_stress_criteria_bwd":
        for bad in (4, -1):
            with pytest.raises(PdgError, match="aggregate must be 0, 1, 2 or 3"):
                fn(*_args(name, aggregate=bad))
    # the optional pointers pass the argument check as NULL: the only refusal left is the one provoked here
    with pytest.raises(PdgError, match="n_graphs must be > 0"):
        fn(*_args(name, null=OPTIONAL[name], n_graphs=0))
    src = (ROOT / "p-div-gnn_amd" / "csrc" / "pdg_criteria.hip").read_text()
    check = re.search(rf'PDG_CHECK_ARG\(([^;]*?),\s*"{name}: null argument', src, re.S).group(1)
    for nm in OPTIONAL[name]:
        assert not re.search(rf"\b{nm}\b", check), nm


def test_python_layer_refuses_cpu_tensors_and_unknown_names():
    import torch
    from gnn_local_stress import criteria as C
    s = torch.zeros(4, 3)
    ptr = torch.tensor([0, 4])
    for call in (lambda: C.stress_fields(s), lambda: C.graph_criterion(s, ptr),
                 lambda: C.graph_criterion_grad(s, ptr, "tresca", "mean")):
        with pytest.raises(RuntimeError, match="HIP"):
            call()
    with pytest.raises(ValueError, match="von_mises, tresca, rankine"):
        C.stress_fields(s, "mises")
    with pytest.raises(ValueError, match="von_mises, tresca, rankine"):
        C.graph_criterion(s, ptr, criterion="principal")
    with pytest.raises(ValueError, match="max, mean, pnorm, ks"):
        C.graph_criterion_grad(s, ptr, "tresca", "softmax")
    # rho has the unit of 1 / stress: no default is guessed for the gradient of ks
    with pytest.raises(ValueError, match="needs rho"):
        C.graph_criterion_grad(s, ptr, "tresca", "ks")
    assert C.CRITERIA == ("von_mises", "tresca", "rankine") and C.AGGREGATES == ("max", "mean", "pnorm", "ks")


def test_criterion_gradients_refuses_a_cpu_batch_and_unknown_names():
    import torch
    from gnn_local_stress.models import EncodeProcessDecode
    from gnn_local_stress.sensitivity import criterion_gradients
    from pdg import graph, meshgen
    m = EncodeProcessDecode(1, 2, latent_size=128, input_nodes_features_size=6, output_nodes_features_size=3)
    b = graph.Batch.from_data_list([graph.sample_to_data(meshgen.hole_plate(5))])
    with pytest.raises(RuntimeError, match="HIP"):
        criterion_gradients(m, b)
    with pytest.raises(ValueError, match="von_mises, tresca, rankine"):
        criterion_gradients(m, b, criterion="mises")
    with pytest.raises(ValueError, match="needs rho"):
        criterion_gradients(m, b, aggregate="ks")
