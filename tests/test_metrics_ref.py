"""tests/metrics_ref.py (the numpy yardstick of the GPU metrics tests) against the reference's own
evaluation functions, recorded in tests/golden/eval_metrics.npz by tests/golden/make_golden_metrics.py.
CPU only.  Both sides are fp64 on the same fp32 inputs; they differ by the summation order at most,
so every value agrees to 1e-12 relative."""
from pathlib import Path

import numpy as np
import pytest

import metrics_ref as R

FIXTURE = Path(__file__).resolve().parent / "golden" / "eval_metrics.npz"
CASES = ("plate8", "hole12", "plate17")
RTOL = 1e-12


@pytest.fixture(scope="module")
def golden():
    with np.load(FIXTURE, allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def case(golden, name):
    return {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + "_")}


def close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    err = np.abs(a - b)
    assert np.all(err <= RTOL * np.abs(b)), (what, float((err / np.maximum(np.abs(b), 1e-300)).max()))


def test_fixture_is_small_and_has_an_internal_boundary(golden):
    assert FIXTURE.stat().st_size < 200_000
    sizes = [len(case(golden, c)["gt"]) for c in CASES]
    assert all(50 <= n <= 500 for n in sizes) and len(set(sizes)) == 3
    assert (case(golden, "hole12")["labels"] == -1).any() and (case(golden, "hole12")["labels"] == 1).any()
    for c in CASES:
        g = case(golden, c)
        assert g["gt"].dtype == np.float32 and g["pred"].dtype == np.float32 and g["op_vals"].dtype == np.float32
        assert g["mean"].dtype == np.float32 and g["std"].dtype == np.float32


@pytest.mark.parametrize("name", CASES)
def test_nmse_r2_and_von_mises_equal_the_reference(golden, name):
    g = case(golden, name)
    gt, pred = g["gt"], g["pred"]
    close(R.nmse(gt, pred, reduce=False), g["nmse_c"], "nmse_c")
    close(R.nmse(gt, pred), g["nmse"], "nmse")
    close(R.von_mises(*gt.T), g["vm_gt"], "vm_gt")
    close(R.von_mises(*pred.T), g["vm_pred"], "vm_pred")
    close(R.nmse(R.von_mises(*gt.T), R.von_mises(*pred.T)), g["nmse_vm"], "nmse_vm")
    close(R.nmse_element_wise(R.with_von_mises(gt), R.with_von_mises(pred)), g["err_field"], "err_field")
    close(R.r2(gt, pred), g["r2"], "r2")
    # sklearn's r2_score is 1 - nmse
    close(1.0 - R.nmse(gt, pred), g["r2"], "1 - nmse")
    close(1.0 - g["nmse"], g["r2"], "fixture: 1 - nmse")
    # the standardised NMSE and R2 equal the raw ones mathematically (an affine map of both fields);
    # numerically they are separate computations on both sides
    gs, ps = R.standardize(gt, g["mean"], g["std"]), R.standardize(pred, g["mean"], g["std"])
    close(R.nmse(gs, ps, reduce=False), g["nmse_c_std"], "nmse_c_std")
    close(R.nmse(gs, ps), g["nmse_std"], "nmse_std")
    close(R.r2(gs, ps), g["r2_std"], "r2_std")
    close(g["nmse_std"], g["nmse"], "fixture: standardised nmse == raw")
    close(g["r2_std"], g["r2"], "fixture: standardised r2 == raw")
    close(R.nmse(gs, ps), R.nmse(gt, pred), "standardised nmse == raw")
    # graph_metrics assembles the same numbers
    m = R.graph_metrics(gt, pred)
    close(m["nmse_table"], [*g["nmse_c"], g["nmse"], g["nmse_vm"], g["r2"]], "nmse_table")
    close(m["err_field"], g["err_field"], "graph err_field")


@pytest.mark.parametrize("name", CASES)
def test_divergence_scalars_and_norm_fields_equal_the_reference(golden, name):
    g = case(golden, name)
    n = len(g["gt"])
    csr = R.coo_to_csr(n, g["op_rows"], g["op_cols"], g["op_vals"])
    for tag, field in (("", g["pred"]), ("_fem", g["gt"])):
        d = R.div_sigma(field, *csr)
        ds = R.div_sigma(R.standardize(field, g["mean"], g["std"]), *csr)
        for i, strategy in enumerate(("square", "abs")):
            close([R.divergence(d, g["labels"], strategy), R.divergence(ds, g["labels"], strategy)],
                  g["div" + tag][i], f"div{tag} {strategy}")
        close(np.stack([R.divergence_norm(d, g["labels"]), R.divergence_norm(ds, g["labels"])]),
              g["norm" + tag], f"norm{tag}")
    for i, strategy in enumerate(("square", "abs")):
        m = R.graph_metrics(g["gt"], g["pred"], csr, g["labels"], g["mean"], g["std"], strategy)
        close(m["div_table"], g["div"][i], "div_table")
        close(m["div_table_fem"], g["div_fem"][i], "div_table_fem")
        close([m["norm"], m["norm_std"]], g["norm"], "norm")
        close([m["norm_fem"], m["norm_fem_std"]], g["norm_fem"], "norm_fem")
    with pytest.raises(AttributeError):
        R.divergence(d, g["labels"], "raw")


def test_degenerate_graphs_follow_numpy():
    one = R.graph_metrics([[1.0, 2.0, 3.0]], [[1.5, 2.0, 3.0]])
    assert np.isposinf(one["nmse_table"][0]) and np.isnan(one["nmse_table"][1:4]).all()   # 0.25 / 0, 0 / 0
    assert np.isposinf(one["nmse_table"][4]) and np.isnan(one["nmse_table"][5])
    inf = R.graph_metrics([[1.0, 2.0, 3.0]], [[1.5, 2.5, 3.5]])["nmse_table"]
    assert np.isposinf(inf[:5]).all() and np.isneginf(inf[5])
    empty = R.graph_metrics(np.zeros((0, 3)), np.zeros((0, 3)), (np.zeros(1, np.int64), [], []), [])
    assert np.isnan(empty["nmse_table"]).all() and np.isnan(empty["div_table"]).all()
    assert empty["err_field"].shape == (0, 4) and empty["norm"].shape == (0,)
