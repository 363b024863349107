"""The mesh fields reach a minibatch: pdg.devgraph.attach_mesh_fields sets them on a Data from its mesh, and
DeviceGraphStore(..., mesh_fields=True) carries them into every batch bitwise as Batch.from_data_list does; without
the keyword a batch is what it always was."""
import numpy as np
import pytest
import torch

import physloss_ref as R

pytestmark = pytest.mark.gpu

FIELDS = ("node_area", "cell_area", "boundary_vec", "boundary_len")


def _datas(attach=True):
    from pdg import devgraph, graph
    tri, quad = R.cases()
    out = []
    for s in tri[:3] + quad:
        d = graph.sample_to_data(s)
        d.face = torch.from_numpy(np.ascontiguousarray(s.faces.T))
        if attach:
            assert devgraph.attach_mesh_fields(d, "cuda") is d
        out.append(d)
    return out, tri[:3] + quad


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def test_attach_mesh_fields_sets_the_device_results_on_the_data():
    from pdg import devgraph
    datas, samples = _datas()
    for d, s in zip(datas, samples):
        pts, fcs = torch.from_numpy(s.pos).cuda(), torch.from_numpy(s.faces).cuda()
        area = devgraph.nodal_areas(pts, fcs, cells="any")
        bv = devgraph.boundary_vectors(pts, fcs, cells="any")
        n = s.num_nodes
        assert d.node_area.shape == (n,) and d.boundary_vec.shape == (n, 2) and d.boundary_len.shape == (n,)
        assert d.cell_area.shape == (1,) and d.cell_area.dtype == torch.float64
        assert all(d[k].device.type == "cpu" for k in FIELDS)           # kept where the data's pos lives
        assert torch.equal(d.node_area, area.area.cpu()) and torch.equal(d.cell_area, area.cell_area.cpu())
        assert torch.equal(d.boundary_vec, bv.vec.cpu()) and torch.equal(d.boundary_len, bv.length.cpu())
        assert float(d.cell_area) == pytest.approx(1e4, rel=1e-6)


def test_store_batches_carry_the_fields_bitwise():
    from pdg.collate import DeviceGraphStore
    from pdg.graph import Batch
    datas, _ = _datas()
    store = DeviceGraphStore(datas, "cuda", mesh_fields=True)
    plain = DeviceGraphStore(datas, "cuda")
    for idx in ([0, 1, 2, 3], [3, 1], [2]):
        got = store.batch(idx)
        want = Batch.from_data_list([datas[i] for i in idx]).to("cuda")
        old = plain.batch(idx)
        torch.cuda.synchronize()
        for k in FIELDS:
            a, b = got.__dict__[k], want.__dict__[k]
            assert a.is_cuda and a.dtype == b.dtype and a.shape == b.shape, k
            assert torch.equal(_bits(a), _bits(b)), k
            assert k not in old.__dict__, k
        # everything else is what the plain store gives
        assert sorted(set(got.__dict__) - set(FIELDS)) == sorted(old.__dict__)
        for k in ("pos", "mean_stress", "local_stress", "nodes_types", "edge_attr", "edge_index", "ptr"):
            assert torch.equal(got.__dict__[k], old.__dict__[k]), k


def test_store_refuses_graphs_without_the_fields():
    from pdg.collate import DeviceGraphStore
    datas, _ = _datas()
    del datas[2].boundary_len
    with pytest.raises(ValueError, match="graph 2 has no boundary_len"):
        DeviceGraphStore(datas, "cuda", mesh_fields=True)
    bare, _ = _datas(attach=False)
    with pytest.raises(ValueError, match="attach_mesh_fields"):
        DeviceGraphStore(bare, "cuda", mesh_fields=True)
    assert "node_area" not in DeviceGraphStore(bare, "cuda").batch([0, 1]).__dict__
