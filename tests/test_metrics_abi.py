"""CPU-side checks of the evaluation-metrics C ABI (csrc/pdg_metrics.hip): declared, bound with matching
pointer / integer / float kinds, exported, and bad arguments refused before any HIP call."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "pdivgnn.h"
NAMES = ("pdg_eval_nmse", "pdg_eval_div")
OPTIONAL = {"pdg_eval_nmse": ("err_field", "vm_gt", "vm_pred"), "pdg_eval_div": ("norm", "norm_std")}


def _params(name):
    """(C type, name) of every parameter of `name` in include/pdivgnn.h."""
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", text, re.S)
    assert m, name
    out = []
    for a in m.group(1).split(","):
        nm = re.findall(r"\w+", a)[-1]
        out.append((a.strip()[:a.strip().rfind(nm)].strip(), nm))
    return out


def test_header_and_signatures_hold_the_metrics():
    from pdg.lib import _RESTYPES, SIGNATURES
    for name in NAMES:
        params = _params(name)
        assert len(SIGNATURES[name]) == len(params), name
        for ctype, (ctext, nm) in zip(SIGNATURES[name], params):
            want = ctypes.c_void_p if "*" in ctext else {"int": ctypes.c_int, "float": ctypes.c_float}[ctext]
            assert ctype is want, (name, nm)
        assert name not in _RESTYPES
    assert [n for _, n in _params("pdg_eval_nmse")] == ["n_graphs", "ptr", "gt", "pred", "table", "err_field",
                                                        "vm_gt", "vm_pred", "stream"]
    assert [n for _, n in _params("pdg_eval_div")] == ["n_graphs", "ptr", "a_rowptr", "a_col", "a_val", "node_types",
                                                       "sigma", "mean", "std", "reduce_abs", "table", "norm",
                                                       "norm_std", "stream"]
    kinds = dict((n, t) for t, n in _params("pdg_eval_nmse") + _params("pdg_eval_div"))
    assert kinds["table"] == "double*" and kinds["node_types"] == "const int64_t*" and kinds["err_field"] == "float*"


def test_header_cites_the_reference_and_states_the_r2_deviation():
    text = " ".join(HEADER.read_text().split())
    for cite in ("compare_results.py:333-348", ":351-364", ":713-726", "compare_results.py:647-673", ":122-141"):
        assert cite in text, cite
    assert "r2_score" in text and "NOT reproduced" in text


def test_library_exports_the_metrics():
    from pdg.lib import lib
    dll = lib.load()
    for name in NAMES:
        assert hasattr(dll, name), name


def _args(name, null=(), **vals):
    """Arguments of `name`: every pointer a distinct 16-byte-aligned fake address (never dereferenced: the
    checks run on the host before any HIP call) except those in `null` and the stream."""
    v = {"n_graphs": 3, "mean": 0.5, "std": 2.0, "reduce_abs": 0}
    v.update(vals)
    out = []
    for i, (ctext, nm) in enumerate(_params(name)):
        out.append((None if nm in null or nm == "stream" else 0x100000 + 0x1000 * i) if "*" in ctext else v[nm])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_metrics_refuse_bad_arguments(name):
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-side argument checks only: never called with fake pointers where a GPU is present")
    from pdg.lib import PdgError, lib
    fn = getattr(lib, name)
    for ctext, nm in _params(name):
        if "*" in ctext and nm != "stream" and nm not in OPTIONAL[name]:
            with pytest.raises(PdgError, match="null argument"):
                fn(*_args(name, null=(nm,)))
    for bad in (0, -1):
        with pytest.raises(PdgError, match="n_graphs must be > 0"):
            fn(*_args(name, n_graphs=bad))
        # the size is refused first, whatever else is wrong
        with pytest.raises(PdgError, match="n_graphs must be > 0"):
            fn(*_args(name, null=("ptr", "table"), n_graphs=bad))
    if name == "pdg_eval_div":
        for z in (0.0, -0.0):
            with pytest.raises(PdgError, match="std must be non-zero"):
                fn(*_args(name, std=z))
        # refused with the optional outputs NULL as well: the check does not depend on them
        with pytest.raises(PdgError, match="std must be non-zero"):
            fn(*_args(name, null=OPTIONAL[name], std=0.0))
    else:
        with pytest.raises(PdgError, match="16-byte aligned"):
            a = _args(name)
            a[[n for _, n in _params(name)].index("err_field")] += 4
            fn(*a)


@pytest.mark.parametrize("name", NAMES)
def test_optional_outputs_pass_the_argument_check_as_null(name):
    """With every optional output NULL the only refusal left is the one provoked here (the size), so the
    argument check accepted the NULL outputs; no launch happens either way."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-side argument checks only: never called with fake pointers where a GPU is present")
    from pdg.lib import PdgError, lib
    fn = getattr(lib, name)
    required = [nm for ctext, nm in _params(name) if "*" in ctext and nm != "stream" and nm not in OPTIONAL[name]]
    for nm in required:
        with pytest.raises(PdgError, match="null argument"):
            fn(*_args(name, null=OPTIONAL[name] + (nm,)))
    src = (ROOT / "p-div-gnn_amd" / "csrc" / "pdg_metrics.hip").read_text()
    check = re.search(rf'PDG_CHECK_ARG\(([^;]*?),\s*"{name}: null argument', src, re.S).group(1)
    for nm in OPTIONAL[name]:
        assert not re.search(rf"\b{nm}\b", check), nm
