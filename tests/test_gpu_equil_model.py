"""inference.predict_mesh(..., equilibrate=True) on the n = 17 hole plate, as triangles and as its quad twin, with
a seeded random-weight model: the returned field's divergence penalty (the function's own ``divergence=True``
output, whose rows with node type +-1 are zeroed: the interior rows, the ones the projection constrains) falls to
(2 rtol)^2 of the unequilibrated prediction's, the penalty being the mean of the squared row norms over the same n
rows; and without the option the output is bitwise what it was."""
import numpy as np
import pytest
import torch

import equil_ref as R

pytestmark = pytest.mark.gpu

RTOL = 1e-4


@pytest.fixture(scope="module")
def model():
    from gnn_local_stress.models import EncodeProcessDecode
    torch.manual_seed(69)
    stats = {k: torch.tensor(v) for k, v in {"mean_pos": 50.0, "std_pos": 29.0, "mean_mean_stress": 0.0,
                                             "std_mean_stress": 60.0, "mean_local_stress": 0.0,
                                             "std_local_stress": 60.0, "mean_edge_weight": 9.0,
                                             "std_edge_weight": 4.0}.items()}
    m = EncodeProcessDecode(input_edges_features_size=1, message_passing_steps=3, latent_size=128,
                            input_nodes_features_size=6, output_nodes_features_size=3, **stats).to("cuda")
    m.eval()
    return m


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


@pytest.mark.parametrize("name,cells", [("tri17", "triangle"), ("quad17", "quad"), ("quad17", "any")])
def test_predict_mesh_equilibrates(model, name, cells):
    from gnn_local_stress import equilibrate as E
    from gnn_local_stress.inference import predict_mesh
    s = R.mesh(name)
    mesh = (s.pos, s.faces)
    plain, div0 = predict_mesh(model, mesh, s.mean_stress, divergence=True, cells=cells)
    data, div1, info = predict_mesh(model, mesh, s.mean_stress, divergence=True, cells=cells, equilibrate=True,
                                    rtol=RTOL)
    assert info is data.equilibrate_info and info.shape == (1, 4) and info.dtype == torch.float64 and info.is_cuda
    b, res, it, status = info.cpu().numpy()[0]
    ratio = float(np.sqrt(float(div1) / float(div0)))
    print(f"{name} cells={cells}: {int(it)} iterations, penalty {float(div0):.4e} -> {float(div1):.4e}, ratio "
          f"{ratio:.3e}, the solver's own {res / b:.3e}, status {int(status)}")
    assert status == 0 and 0 < it <= 1000
    assert ratio <= 2 * RTOL
    assert data.local_stress.shape == plain.local_stress.shape and data.local_stress.dtype == torch.float32
    assert data.node_area.shape == (s.num_nodes,)
    # it is the module's function on the prediction, with the areas and the operator built with the graph
    want, t = E.equilibrate(plain.local_stress, data, "area", rtol=RTOL, return_info=True)
    assert torch.equal(_bits(data.local_stress), _bits(want)) and torch.equal(_bits(info), _bits(t))
    # projection, then shift
    both, info2 = predict_mesh(model, mesh, s.mean_stress, cells=cells, equilibrate=True, rtol=RTOL,
                               enforce_mean="cell")
    assert torch.equal(_bits(both.local_stress),
                       _bits(E.equilibrate(plain.local_stress, data, "area", rtol=RTOL, mean="cell")))
    assert torch.equal(_bits(info2), _bits(info))


@pytest.mark.parametrize("name,cells", [("tri17", "triangle"), ("quad17", "quad")])
def test_without_the_option_nothing_changes(model, name, cells):
    from gnn_local_stress.inference import predict_mesh
    from pdg.devgraph import convert_mesh_to_graph
    s = R.mesh(name)
    pts = torch.from_numpy(s.pos).cuda()
    fcs = torch.from_numpy(s.faces).cuda()
    with torch.no_grad():
        ref = model(convert_mesh_to_graph(pts, fcs, s.mean_stress, cells=cells)).local_stress
    for kw in ({}, {"equilibrate": False}):
        out = predict_mesh(model, (s.pos, s.faces), s.mean_stress, cells=cells, **kw)
        assert not isinstance(out, tuple) and torch.equal(_bits(out.local_stress), _bits(ref))
        assert out.node_area is None and out.op_div_matrix is None and out.equilibrate_info is None
        data, div = predict_mesh(model, (s.pos, s.faces), s.mean_stress, divergence=True, cells=cells, **kw)
        assert torch.equal(_bits(data.local_stress), _bits(ref)) and torch.isfinite(div).all()
