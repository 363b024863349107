"""The fp64 restatement of the per-step edge backward (tests/edge_bwd_ref.py), which the GPU op tests hold
pdg_edge_bwd and pdg_edge_bwd_w2 to, against torch autograd through the model's own graph LayerNorm
(oracle.epd_oracle.graph_layer_norm): the reference is anchored to the model, not to a second derivation."""
import pytest
import torch

from edge_bwd_ref import L, LN_EPS, edge_bwd_ref, hub_graph, worst_row
from oracle import epd_oracle as O


def rel(a, b):
    return float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-300))


def test_eps_is_the_oracles():
    assert LN_EPS == O.LN_EPS


@pytest.mark.parametrize("eu", [True, False])
@pytest.mark.parametrize("E", [1, 17, 300])
def test_closed_form_equals_autograd(E, eu):
    """One step of the edge net as the model runs it (models.py:194-222): C = e Wc^T, z1 = C + the gathered
    P / Q rows, a1 = relu(z1), a2 = relu(a1 W2^T + b2), message = LN(a2m) summed into the nodes, e_next =
    LN(a2e) + e.  The loss <gaggr[dst], message> + <ge_next, e_next> makes autograd deliver every quantity the
    restatement returns; both LayerNorms get their own leaf copy of the shared weight so that their column sums
    can be told apart.  1e-12 relative (fp64 on both sides, the sums in different orders)."""
    g = torch.Generator().manual_seed(11 * E + eu)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    N, _, dst, _, _, _ = hub_graph(E)
    W2 = (rn(L, L) / L ** 0.5).requires_grad_(True)
    b2 = (rn(L) * 0.1 + 0.1).requires_grad_(True)
    Wc = rn(L, L) / L ** 0.5
    ln_g, ln_b = rn(L) * 0.3 + 1.0, rn(L) * 0.1
    e = rn(E, L).requires_grad_(True)
    um, ue = rn(E, L).requires_grad_(True), rn(E, L).requires_grad_(True)
    gaggr, ge_next = rn(N, L), rn(E, L)
    C = e @ Wc.T
    branch = {}
    loss = 0
    for name, u, gy in (("m", um, gaggr[dst]), ("e", ue, ge_next))[: 2 if eu else 1]:
        gl, bl = ln_g.clone().requires_grad_(True), ln_b.clone().requires_grad_(True)
        a1 = torch.relu(C + u)
        z2 = a1 @ W2.T + b2
        a2 = torch.relu(z2)
        a2.retain_grad()
        z2.retain_grad()
        y = O.graph_layer_norm(a2, gl, bl)
        loss = loss + (y * gy).sum() + ((e * gy).sum() if name == "e" else 0)
        branch[name] = (u, a1, z2, a2, gl, bl)
    loss.backward()
    um_, a1m, z2m, a2m, glm, blm = branch["m"]
    a1e = a2e = None
    if eu:
        ue_, a1e, z2e, a2e, gle, ble = branch["e"]
    r = edge_bwd_ref(dst, gaggr, ge_next if eu else None, a2m, a1m, a2e, a1e, ln_g, W2, Wc)
    tol = 1e-12
    assert rel(r.ga2m, a2m.grad) < tol and rel(r.gz2m, z2m.grad) < tol and rel(r.gz1m, um.grad) < tol
    assert rel(r.ln_m.col_gy, blm.grad) < tol and rel(r.ln_m.col_gyx, glm.grad) < tol
    if eu:
        assert rel(r.ga2e, a2e.grad) < tol and rel(r.gz2e, z2e.grad) < tol and rel(r.gz1e, ue.grad) < tol
        assert rel(r.ln_e.col_gy, ble.grad) < tol and rel(r.ln_e.col_gyx, gle.grad) < tol
        assert rel(r.gC, um.grad + ue.grad) < tol
    else:
        assert torch.equal(r.gC, r.gz1m) and not hasattr(r, "gz1e")
    assert rel(r.ge_out, e.grad) < tol
    assert rel(r.dW2, W2.grad) < tol and rel(r.db2, b2.grad) < tol
    # S1 / S2: the g-weighted column sums, i.e. sum over all elements of g * gy and of g * gy * xhat
    for ln, gy, a2 in ((r.ln_m, gaggr[dst], a2m),) + (((r.ln_e, ge_next, a2e),) if eu else ()):
        a2 = a2.detach()
        xhat = (a2 - a2.mean()) / (a2.std(unbiased=False) + O.LN_EPS)
        assert abs(float(ln.S1) - float((ln_g * gy).sum())) <= tol * float((ln_g * gy).abs().sum())
        assert abs(float(ln.S2) - float((ln_g * gy * xhat).sum())) <= tol * float((ln_g * gy * xhat).abs().sum())
        assert float(ln.S1) == float((ln_g * ln.col_gy).sum()) and float(ln.S2) == float((ln_g * ln.col_gyx).sum())
        assert ln.count == E * L and rel(ln.std, a2.std(unbiased=False)) < tol


def test_float32_restatement_is_close_to_float64():
    """The same function in float32 is the yardstick of the GPU tests' per-row bound: it must be an fp32-accurate
    evaluation of the chain (a few 1e-7 from fp64), not something looser that would let a kernel error pass."""
    E = 300
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g)
    N, _, dst, _, _, _ = hub_graph(E)
    a1m, a1e = torch.relu(rn(E, L)), torch.relu(rn(E, L))
    W2, Wc = rn(L, L) / L ** 0.5, rn(L, L) / L ** 0.5
    a2m, a2e = torch.relu(a1m @ W2.T + 0.1), torch.relu(2 * a1e @ W2.T + 0.1)
    args = (dst, rn(N, L), rn(E, L), a2m, a1m, a2e, a1e, rn(L) * 0.3 + 1.0, W2, Wc)
    r64, r32 = edge_bwd_ref(*args), edge_bwd_ref(*args, dtype=torch.float32)
    for k in ("gz1m", "gz1e", "gC", "ge_out", "dW2", "db2"):
        assert getattr(r32, k).dtype == torch.float32
        assert rel(getattr(r32, k), getattr(r64, k)) < 2e-6, k
    assert worst_row(r32.gC, r64.gC) < 1e-5


def test_hub_graph_has_the_shapes_it_promises():
    for E in (1, 15, 77, 4099):
        N, src, dst, rp, rps, perm_src = hub_graph(E)
        assert bool((dst[1:] >= dst[:-1]).all()) and int(rp[-1]) == E == int(rps[-1])
        deg = rp[1:] - rp[:-1]
        assert int(deg.max()) >= min(E, 40)
        assert int((deg[:-3] == 0).sum()) >= 1 and bool((deg[-3:] == 0).all())
        assert bool((src[perm_src][1:] >= src[perm_src][:-1]).all())
        if E >= 4099:
            assert N * 8 < E
