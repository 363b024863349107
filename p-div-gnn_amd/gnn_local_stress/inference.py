"""Inference I/O of the reference (``scripts/gnn_inference.py``) on the HIP path
(SURVEY §8f row 2): reads a dataset CSV (vtk + npz per sample), loads a
reference checkpoint, runs ``forward(scale_output=True, scale_input=True)``
per minibatch and writes, as the reference does,

* ``fields/hole_plate_mesh_{i}.npz``: a copy of sample i's input ``.npz`` with
  ``stress_field`` replaced by the prediction (gnn_inference.py:34-42, :61-79);
* ``dataset.csv``: the input table with ``data_filename`` pointing at those
  files (:130-131);
* ``normalize_params.json``: the model's ``mean_local_stress`` /
  ``std_local_stress`` (:132-138);
* a copy of the config file (:98).

    python -m gnn_local_stress.inference config_inference.yml
"""
from __future__ import annotations

import json
import shutil
from pathlib import Path

import numpy as np
import torch

from pdg.graph import DataLoader

from . import data_utils, datasets, models


def copy_data_file_and_replace_local_stress_field(original_data_path: str, target_data_path: str,
                                                  local_stress_field: torch.Tensor) -> None:
    """gnn_inference.py:34-42 (arrays loaded without pickle)."""
    with np.load(original_data_path, allow_pickle=False) as f:
        org_data = {k: f[k] for k in f.files}
    org_data["stress_field"] = local_stress_field.numpy()
    np.savez(target_data_path, **org_data)


def predict_and_save(model: models.EncodeProcessDecode, dataloader: DataLoader, results_folder: Path,
                     device) -> list[str]:
    """gnn_inference.py:45-81."""
    fields_folder = Path(results_folder) / "fields"
    fields_folder.mkdir(exist_ok=True, parents=True)
    mesh_id = 0
    names: list[str] = []
    for batch in dataloader:
        batch = batch.to(device)
        with torch.no_grad():
            pred = model.forward(batch, scale_output=True, scale_input=True)
        for field in data_utils.slice_batch_predictions(batch_graph_prediction=pred.local_stress,
                                                        batch_indices=batch.batch):
            path = (fields_folder / f"hole_plate_mesh_{mesh_id}.npz").as_posix()
            original = dataloader.dataset.dataframe.data_filename[mesh_id]
            copy_data_file_and_replace_local_stress_field(original, path, field.cpu())
            mesh_id += 1
            names.append(path)
    return names


@torch.no_grad()
def predict_mesh(model: models.EncodeProcessDecode, mesh, mean_stress, periodic: bool = True,
                 divergence: bool = False, enforce_mean: str | None = None, boundary: bool = False,
                 cells: str = "triangle", *, sample=None, equilibrate: bool = False, rtol: float = 1e-5,
                 max_iter: int = 1000):
    """The reference's published workload (``scripts/benchmark_gnn_fem.py:388-415`` then one
    forward) from a bare mesh: ``mesh`` is a legacy-VTK path or a ``(points, faces)`` pair of
    arrays / tensors, ``mean_stress`` the imposed mean field (3 values).  The graph, the node
    labels and the forward (``scale_output=True``) run on the model's device; no ``.npz`` is
    needed.  Returns the graph ``Data`` with ``local_stress`` (the prediction) and
    ``nodes_types``; with ``divergence`` returns ``(data, div)``, ``div`` the prediction's
    divergence penalty (``losses.compute_divergence`` with the mesh's P1 operator, which is
    kept as ``data.op_div_matrix``).  ``enforce_mean`` = ``"cell"`` or ``"material"`` builds the nodal
    areas with the graph (``data.node_area``, ``data.cell_area``) and returns the prediction shifted so
    that its volume average in that convention equals ``mean_stress``
    (``gnn_local_stress.homogenise.enforce_mean``); None returns the model's output as it is.
    ``boundary`` builds the boundary vectors with the graph (``data.boundary_vec``, ``data.boundary_len``)
    and also returns the boundary residuals of the returned prediction
    (``gnn_local_stress.boundary.boundary_residuals``; the periodic columns with ``periodic``), as the last
    value: ``(data, res)`` or ``(data, div, res)``.  ``cells`` = ``"triangle"`` (the default: (F, 3) faces only, a
    quad array is refused), ``"quad"`` ((F, 4) faces) or ``"any"`` (decided by the faces' width, which is what a VTK
    file's reader returns): a quad mesh gets the four sides of every quad as edges, its labels, the q1 divergence
    operator, the exact Q1 nodal areas and its boundary vectors from the same device builders
    (``pdg.devgraph``).  ``sample`` (keyword only): query points (Q, 2|3); the returned prediction is also evaluated
    there (``gnn_local_stress.sampling``: ``PointLocator(points, faces, cells, periodic)``, so with ``periodic`` a
    point beyond the cell is wrapped into it) and kept as ``data.samples`` (Q, 3), NaN where no cell holds the point,
    with ``data.sample_plan``; what is returned, and the prediction, are otherwise unchanged.  ``equilibrate``
    (keyword only): the prediction is projected onto the fields whose divergence vanishes at the interior nodes
    (``gnn_local_stress.equilibrate.equilibrate`` with the mesh's operator and its nodal areas as weights, both
    built with the graph, to ``rtol`` in at most ``max_iter`` iterations) before ``enforce_mean`` shifts it:
    projection, then shift, which with the areas is the closest field that satisfies both.  The solver's (1, 4)
    fp64 table (``equilibrate.COLUMNS``: defect, true residual, iterations, status bits) is kept as
    ``data.equilibrate_info`` and returned as one more last value, ``(data, info)`` up to
    ``(data, div, res, info)``; it stays on the device and is not read here.  Everything after it (``sample``,
    ``boundary``, ``divergence``) sees the equilibrated field.  False changes nothing."""
    from pdg.devgraph import convert_mesh_to_graph
    from . import boundary as bd, equilibrate as eq, homogenise, losses, sampling, vtk_io
    if enforce_mean is not None:
        homogenise._id(enforce_mean, homogenise.CONVENTIONS, "convention")
    if isinstance(mesh, (str, Path)):
        points, faces = vtk_io.read_legacy_vtk(mesh)
    else:
        points, faces = mesh
    device = next(model.parameters()).device
    points = torch.as_tensor(points).to(device=device, dtype=torch.float32)
    faces = torch.as_tensor(faces).to(device=device, dtype=torch.int64)
    if cells == "triangle" and (faces.dim() != 2 or faces.shape[1] != 3):
        raise ValueError(f"predict_mesh takes triangle meshes only (faces of shape (F, 3)) by default, got "
                         f"{tuple(faces.shape)}: pass cells='quad' or cells='any' for a quad mesh")
    data = convert_mesh_to_graph(points, faces, mean_stress, None, periodic, bool(divergence or equilibrate),
                                 areas=enforce_mean is not None or bool(equilibrate), boundary=bool(boundary),
                                 cells=cells)
    data.local_stress = model.forward(data, scale_output=True, scale_input=True).local_stress
    if equilibrate:
        data.local_stress, data.equilibrate_info = eq.equilibrate(
            data.local_stress, data, "area", rtol, max_iter, mean=enforce_mean, return_info=True)
    elif enforce_mean is not None:
        data.local_stress = homogenise.enforce_mean(data.local_stress, data, convention=enforce_mean)
    if sample is not None:
        xy = torch.as_tensor(sample).to(device=device, dtype=torch.float32)
        data.sample_plan = sampling.PointLocator(points, faces, cells=cells, periodic=bool(periodic)).locate(xy)
        data.samples = sampling.sample_field(data.local_stress, data.sample_plan)
    res = bd.boundary_residuals(data.local_stress, data, periodic=bool(periodic)) if boundary else None
    tail = (data.equilibrate_info,) if equilibrate else ()
    if not divergence:
        return (data, res) + tail if boundary else (data,) + tail if tail else data
    div = losses.compute_divergence(data.local_stress, data.op_div_matrix, data.surfaces_nodes_for_div)
    return ((data, div, res) if boundary else (data, div)) + tail


@torch.no_grad()
def run_inference(dataset_csv, results_folder, model_weights_path, periodic_graph: bool, batch_size: int,
                  latent_size: int, message_passing_steps: int, device, config_path=None) -> None:
    """gnn_inference.py:84-138."""
    import pandas as pd
    dataframe = pd.read_csv(dataset_csv)
    results_folder = Path(results_folder)
    results_folder.mkdir(parents=True, exist_ok=True)
    if config_path is not None:
        shutil.copyfile(config_path, results_folder / Path(config_path).name)
    dataset = datasets.MeshStressFieldDatasetInMemory(dataframe, periodic_graph=periodic_graph)
    loader = DataLoader(dataset, batch_size=batch_size, shuffle=False)   # must not be shuffled
    model = models.EncodeProcessDecode(input_edges_features_size=1, input_nodes_features_size=6,
                                       message_passing_steps=message_passing_steps, latent_size=latent_size,
                                       output_nodes_features_size=3)
    model.to(device)
    models.load_model_checkpoint(model, str(model_weights_path))
    model.to(device)
    model.eval()
    names = predict_and_save(model, loader, results_folder, device)
    dataframe["data_filename"] = names
    dataframe.to_csv((results_folder / "dataset.csv").as_posix(), index=False)
    params = {"mean_local_stress": float(model.mean_local_stress.cpu()),
              "std_local_stress": float(model.std_local_stress.cpu())}
    with open((results_folder / "normalize_params.json").as_posix(), "w") as f:
        json.dump(params, f)


def main(config_path: str) -> None:
    import yaml
    with open(config_path) as f:
        params = yaml.safe_load(f)
    params["config_path"] = Path(config_path)
    run_inference(**params)


if __name__ == "__main__":
    import sys
    main(sys.argv[1])
