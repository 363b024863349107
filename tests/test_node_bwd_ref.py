"""The fp64 restatements of the per-step node backward and of the backward's two ends (tests/node_bwd_ref.py),
which the GPU op tests hold pdg_node_bwd_coop, pdg_gemm_sum2_coop, pdg_decoder_bwd_coop, pdg_mlp2_bwd_coop and
pdg_ln_colsum_nodes to, against torch autograd through the model's own graph LayerNorm
(oracle.epd_oracle.graph_layer_norm), and a check that the comparison the GPU tests make can tell the true
restatement from six subtly wrong ones."""
import pytest
import torch

from edge_bwd_ref import L, LN_EPS, hub_graph, ln_bwd, worst_row
from node_bwd_ref import colsums, colsums_nodes, decoder_bwd_ref, gemm_sum2_ref, mlp2_bwd_ref, node_bwd_ref
from oracle import epd_oracle as O

TOL = 1e-12   # fp64 on both sides, the sums in different orders (tests/test_edge_bwd_ref.py)


def rel(a, b):
    return float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-300))


def gen(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)


def test_eps_is_the_oracles():
    assert LN_EPS == O.LN_EPS


@pytest.mark.parametrize("N", [1, 17, 300])
def test_node_bwd_equals_autograd(N):
    """One step of node_net as the model runs it (models.py:240-243): a1n = relu(Wn1 [aggr | x] + bn1), a2n =
    relu(Wn2 a1n + bn2), x_next = LN(a2n) + x.  The loss <gy, x_next> makes autograd deliver gz2, gz1, gaggr
    (= d / d aggr), gx_part (= d / d x: the Wn1b path plus the residual) and the LayerNorm's weight / bias
    gradients, the column sums."""
    rn = gen(31 * N)
    Wn1a, Wn1b, Wn2 = (rn(L, L) / L ** 0.5 for _ in range(3))
    bn1, bn2 = rn(L) * 0.1, rn(L) * 0.1 + 0.1
    gl, bl = (rn(L) * 0.3 + 1.0).requires_grad_(True), (rn(L) * 0.1).requires_grad_(True)
    aggr, x = rn(N, L).requires_grad_(True), rn(N, L).requires_grad_(True)
    gy = rn(N, L)
    z1 = aggr @ Wn1a.T + x @ Wn1b.T + bn1
    a1 = torch.relu(z1)
    z2 = a1 @ Wn2.T + bn2
    a2 = torch.relu(z2)
    for t in (z1, z2, a2):
        t.retain_grad()
    ((O.graph_layer_norm(a2, gl, bl) + x) * gy).sum().backward()
    r = node_bwd_ref(gy, a2, a1, gl, Wn2.T, Wn1a.T, Wn1b.T)
    assert rel(r.ga2, a2.grad) < TOL and rel(r.gz2, z2.grad) < TOL and rel(r.gz1, z1.grad) < TOL
    assert rel(r.gaggr, aggr.grad) < TOL and rel(r.gx_part, x.grad) < TOL
    assert rel(r.ln.col_gy, bl.grad) < TOL and rel(r.ln.col_gyx, gl.grad) < TOL
    cols, S1, S2 = colsums(gy, a2, gl)
    assert rel(cols, torch.cat([bl.grad, gl.grad])) < TOL
    gd = gl.detach()
    assert float(S1) == float((gd * cols[:L]).sum()) and float(S2) == float((gd * cols[L:]).sum())
    assert float(S1) == float(r.ln.S1) and float(S2) == float(r.ln.S2)
    assert r.ln.count == N * L and rel(r.ln.std, a2.detach().std(unbiased=False)) < TOL


@pytest.mark.parametrize("res", [True, False])
@pytest.mark.parametrize("N", [1, 33])
def test_gemm_sum2_equals_autograd(N, res):
    """gx_t = Wa^T gP + Wb^T gQ [+ gx_part]: the gradient of <gP, Wa x> + <gQ, Wb x> [+ <gx_part, x>] in x."""
    rn = gen(7 * N + res)
    Wa, Wb = rn(L, L) / L ** 0.5, rn(L, L) / L ** 0.5
    x = rn(N, L).requires_grad_(True)
    gP, gQ, gr = rn(N, L), rn(N, L), rn(N, L)
    loss = ((x @ Wa.T) * gP).sum() + ((x @ Wb.T) * gQ).sum() + ((x * gr).sum() if res else 0)
    loss.backward()
    assert rel(gemm_sum2_ref(gP, gQ, Wa.T, Wb.T, gr if res else None), x.grad) < TOL


@pytest.mark.parametrize("N", [1, 17, 300])
def test_decoder_bwd_equals_autograd(N):
    """The decoder (models.py:282-286): y = Wd2 relu(Wd1 x + bd1) + bd2, loss <gy, y>."""
    rn = gen(13 * N)
    Wd1, bd1 = rn(L, L) / L ** 0.5, rn(L) * 0.1
    Wd2, bd2 = (rn(3, L) / L ** 0.5).requires_grad_(True), rn(3).requires_grad_(True)
    x = rn(N, L).requires_grad_(True)
    gy = rn(N, 3)
    z1 = x @ Wd1.T + bd1
    z1.retain_grad()
    a1 = torch.relu(z1)
    ((a1 @ Wd2.T + bd2) * gy).sum().backward()
    r = decoder_bwd_ref(gy, a1, Wd2, Wd1.T)
    assert rel(r.gz1d, z1.grad) < TOL and rel(r.gx, x.grad) < TOL
    assert rel(r.dWd2, Wd2.grad) < TOL and rel(r.dbd2, bd2.grad) < TOL


@pytest.mark.parametrize("N", [1, 17, 300])
def test_mlp2_bwd_equals_autograd(N):
    """The node encoder (models.py:260-274): a1 = relu(W0 x + b0) over the 6 inputs, a2 = relu(W2 a1 + b2),
    LN(a2); loss <gy, LN(a2)>.  gz2, gz1, the LayerNorm's gradients and the narrow first layer's 128 x 6 weight
    gradient and bias gradient."""
    rn = gen(17 * N)
    W0, b0 = (rn(L, 6) / 6 ** 0.5).requires_grad_(True), (rn(L) * 0.1).requires_grad_(True)
    W2, b2 = rn(L, L) / L ** 0.5, rn(L) * 0.1 + 0.1
    gl, bl = (rn(L) * 0.3 + 1.0).requires_grad_(True), (rn(L) * 0.1).requires_grad_(True)
    xn, gy = rn(N, 6), rn(N, L)
    z1 = xn @ W0.T + b0
    a1 = torch.relu(z1)
    z2 = a1 @ W2.T + b2
    a2 = torch.relu(z2)
    for t in (z1, z2):
        t.retain_grad()
    (O.graph_layer_norm(a2, gl, bl) * gy).sum().backward()
    r = mlp2_bwd_ref(gy, a2, a1, gl, W2.T, xn)
    assert rel(r.gz2, z2.grad) < TOL and rel(r.gz1, z1.grad) < TOL
    assert rel(r.dW0, W0.grad) < TOL and rel(r.db0, b0.grad) < TOL
    assert rel(r.ln.col_gy, bl.grad) < TOL and rel(r.ln.col_gyx, gl.grad) < TOL
    assert not hasattr(mlp2_bwd_ref(gy, a2, a1, gl, W2.T), "dW0")


@pytest.mark.parametrize("E", [1, 77, 4099])
def test_node_level_colsums_equal_edge_level_and_autograd(E):
    """The message LayerNorm (models.py:215-222): message = LN(a2m) summed into the nodes, loss <gaggr, aggr>, so
    the upstream gradient of edge k is gaggr[dst_k].  The node-level sums (degree and per-node sums of xhat) equal
    the per-edge ones and autograd's weight / bias gradients, on a graph with a hub, nodes without an incoming
    edge and trailing isolated nodes."""
    rn = gen(19 * E)
    N, _, dst, _, _, _ = hub_graph(E)
    gl, bl = (rn(L) * 0.3 + 1.0).requires_grad_(True), (rn(L) * 0.1).requires_grad_(True)
    a2m, gaggr = torch.relu(rn(E, L)), rn(N, L)
    aggr = torch.zeros(N, L, dtype=torch.float64).index_add(0, dst, O.graph_layer_norm(a2m, gl, bl))
    (aggr * gaggr).sum().backward()
    cn, S1n, S2n = colsums_nodes(gaggr, dst, a2m, gl)
    ce, S1e, S2e = colsums(gaggr[dst], a2m, gl)
    assert rel(cn, ce) < TOL and rel(cn, torch.cat([bl.grad, gl.grad])) < TOL
    assert abs(float(S1n - S1e)) <= TOL * float((gl.detach() * ce[:L]).abs().sum())
    assert abs(float(S2n - S2e)) <= TOL * float((gl.detach() * ce[L:]).abs().sum())


def mid_case(dtype=torch.float32):
    """The GPU suite's mid case (4099 rows) rebuilt on the CPU the way tests/test_gpu_node_bwd.py builds it: the
    consumer LayerNorm's input a2 from a second layer with weights scaled by 2e-4, so that its std (~5e-5) makes
    eps = 1e-5 visible in den = std + eps; another LayerNorm's input a2p with unscaled weights; gy correlated with
    a2 so that S1 / M and S2 / M are O(1); Wn2T scaled by 1e-4, which undoes the 1 / den ~ 2e4 in gz2, so that the
    products in gx_part are of the size of its residual gy and a dropped residual shows."""
    N = 4099
    rn = gen(4099)
    f = lambda t: t.to(dtype)
    W = lambda: f(rn(L, L) / L ** 0.5)
    a1 = f(torch.relu(rn(N, L)))
    W2, b2 = W(), f(rn(L) * 0.1 + 0.1)
    a2 = torch.relu(a1 @ (W2 * 2e-4).T + b2 * 2e-4)
    a2p = torch.relu(f(torch.relu(rn(N, L) * 2.0)) @ W2.T + b2)
    xh = (a2 - a2.mean()) / a2.std(unbiased=False)
    gy = f(rn(N, L)) + 0.5 * xh + 0.3
    return dict(gy=gy, a2n=a2, a1n=a1, ln_g=f(rn(L) * 0.3 + 1.0), Wn2T=W() * 1e-4, Wn1aT=W(), Wn1bT=W()), a2p


def perturbed(kw, a2_other, which):
    """node_bwd_ref with one thing subtly wrong."""
    gy, a2, a1, g = (kw[k].double() for k in ("gy", "a2n", "a1n", "ln_g"))
    W2T, WaT, WbT = (kw[k].double() for k in ("Wn2T", "Wn1aT", "Wn1bT"))
    if which == "swap Wn1aT / Wn1bT":
        WaT, WbT = WbT, WaT
    M = a2.numel()
    stat_src = a2_other.double() if which == "another LayerNorm's statistics" else a2
    mean = stat_src.mean()
    std = (stat_src - mean).pow(2).mean().sqrt()
    den = std + LN_EPS
    xhat = (a2 - mean) / den
    S1, S2 = (g * gy).sum(), (g * gy * xhat).sum()
    ga2 = (g * gy - S1 / M) / den - xhat * (S2 / (M * (den if which == "S2 / (M den)" else std)))
    gz2 = ga2 * (a2 > 0)
    gz1 = gz2 @ W2T.T
    if which != "no [a1n > 0] mask":
        gz1 = gz1 * (a1 > 0)
    out = dict(gz2=gz2, gz1=gz1, gaggr=gz1 @ WaT.T, gx_part=gz1 @ WbT.T + (0 if which == "no + gy" else gy))
    if which == "last row zeroed":
        for v in out.values():
            v[-1] = 0
    return out


PERTURBATIONS = {   # -> the outputs it must show in
    "swap Wn1aT / Wn1bT": ("gaggr", "gx_part"),
    "no + gy": ("gx_part",),
    "no [a1n > 0] mask": ("gz1", "gaggr", "gx_part"),
    "S2 / (M den)": ("gz2", "gz1", "gaggr", "gx_part"),
    "another LayerNorm's statistics": ("gz2", "gz1", "gaggr", "gx_part"),
    "last row zeroed": ("gz2", "gz1", "gaggr", "gx_part"),
}
GPU_TOL, GPU_ROW_FACTOR = 1e-5, 4   # tests/test_gpu_node_bwd.py: TOL_LN and ROW_FACTOR


def test_gpu_suite_constants_are_the_ones_used_here():
    src = open(__file__.replace("test_node_bwd_ref.py", "test_gpu_node_bwd.py")).read()
    assert "TOL_LN = 1e-5" in src and "ROW_FACTOR = 4\n" in src


@pytest.fixture(scope="module")
def mid():
    kw, a2p = mid_case()
    r64 = node_bwd_ref(**kw)
    r32 = node_bwd_ref(**kw, dtype=torch.float32)
    return kw, a2p, r64, r32


def test_unperturbed_restatement_is_the_reference(mid):
    kw, a2p, r64, _ = mid
    same = perturbed(kw, a2p, None)
    for k, v in same.items():
        assert rel(v, getattr(r64, k)) < TOL, k
    # the inputs are what they are meant to be: eps visible in den, S1 / M and S2 / M of order one
    assert 0.05 < LN_EPS / float(r64.ln.std) < 1.0
    assert abs(float(r64.ln.S1)) / r64.ln.count > 0.1 and abs(float(r64.ln.S2)) / r64.ln.count > 0.1
    sp = a2p.double().std(unbiased=False)
    assert abs(float(sp - r64.ln.std)) > 0.1 * float(r64.ln.std)


def test_float32_restatement_is_close_to_float64(mid):
    """The float32 evaluation is the yardstick of the per-row bound: an fp32-accurate evaluation of the chain, not
    something looser that would let a kernel error pass."""
    _, _, r64, r32 = mid
    for k in ("gz2", "gz1", "gaggr", "gx_part"):
        assert getattr(r32, k).dtype == torch.float32
        assert rel(getattr(r32, k), getattr(r64, k)) < 2e-6, k
        assert worst_row(getattr(r32, k), getattr(r64, k)) < 1e-5, k


@pytest.mark.parametrize("which", list(PERTURBATIONS))
def test_reference_tells_right_from_subtly_wrong(mid, which):
    """Each perturbed restatement is at least 1000 x the GPU test's tolerance away from the true one in every output
    it reaches: 1000 x 1e-5 in relative L2, and 1000 x ROW_FACTOR x the fp32 restatement's worst-row error in the
    per-row measure."""
    kw, a2p, r64, r32 = mid
    bad = perturbed(kw, a2p, which)
    for k in PERTURBATIONS[which]:
        ref = getattr(r64, k)
        d, dr = rel(bad[k], ref), worst_row(bad[k], ref)
        row_tol = GPU_ROW_FACTOR * worst_row(getattr(r32, k), ref)
        print(f"{which}: {k} rel {d:.2e} (tol {GPU_TOL:.0e}) worst row {dr:.2e} (tol {row_tol:.2e})")
        assert d >= 1000 * GPU_TOL, (which, k, d)
        assert dr >= 1000 * row_tol, (which, k, dr, row_tol)
    for k in set(bad) - set(PERTURBATIONS[which]):
        assert rel(bad[k], getattr(r64, k)) < TOL, (which, k)


def test_ln_bwd_is_shared_with_the_edge_suite():
    import edge_bwd_ref
    import node_bwd_ref as nb
    assert nb.ln_bwd is edge_bwd_ref.ln_bwd is ln_bwd
