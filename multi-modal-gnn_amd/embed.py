"""What the embeddings learned: PCA maps of the node embeddings, the ``visualization.dim_reduction: "pca"`` branch of the
reference's ``create_embedding_visualizations`` (``src/advanced_visualizations.py``) and ``plot_embeddings_umap``
(``src/visualize.py``), without the plotting and over EVERY patient instead of the reference's 1,000-patient sample.

``pca`` has the semantics of ``sklearn.decomposition.PCA`` 1.7: variance ``lambda / (n - 1)``, ratio over all
eigenvalues, each component signed so that its largest-magnitude entry is positive
(``svd_flip(u_based_decision=False)``), negative round-off eigenvalues clamped to 0.

A HIP tensor runs three kernels (``csrc/pca.hip``): the column means and the centred Gram matrix in fp64
(``mmg_centered_gram``, two passes over the rows), then -- after ``numpy.linalg.eigh`` of the at most 256 x 256 matrix
on the host, the one synchronisation -- the projection of every row (``mmg_project_rows``).  The patient density grid is
``mmg_grid2d``.  A host tensor or numpy array runs the same steps in float64 numpy: that path is the checker.  t-SNE and
UMAP stay out of scope.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, Optional

import numpy as np
import pandas as pd
import torch

MAX_D = 256                  # ops.PCA_MAX_D: the widest embedding of csrc/pca.hip (a multiple of 4 in [4, 256])
MAX_K = 8                    # ops.PCA_MAX_K: components per projection call
MAX_GRID = 256               # ops.GRID_MAX
VOCAB_TYPES = ("lab", "diagnosis", "medication")
VARIANCE_COLUMNS = ["node_type", "component", "explained_variance", "explained_variance_ratio", "singular_value"]
DENSITY_COLUMNS = ["ix", "iy", "x_lo", "x_hi", "y_lo", "y_hi", "count", "mean_degree"]

# the reference's panels, in its order: a later panel overwrites an earlier one
PANELS = (
    ("CBC", ("Hct", "Hgb", "RBC", "WBC x 1000", "platelets x 1000", "MCH", "MCHC", "MCV", "RDW", "MPV")),
    ("CMP", ("sodium", "potassium", "chloride", "CO2", "glucose", "BUN", "creatinine", "calcium")),
    ("LFT", ("ALT (SGPT)", "AST (SGOT)", "alkaline phos.", "total bilirubin", "direct bilirubin", "total protein",
             "albumin")),
    ("Coag", ("PT - INR", "PT", "PTT")),
    ("ABG", ("pH", "paCO2", "paO2", "Base Excess", "HCO3")),
)


@dataclass
class PCAResult:
    mean: np.ndarray                         # fp64 [D]
    components: np.ndarray                   # fp64 [k, D]
    explained_variance: np.ndarray           # fp64 [k]
    explained_variance_ratio: np.ndarray     # fp64 [k]
    singular_values: np.ndarray              # fp64 [k]
    projection: object                       # device fp32 [n, k]; float64 numpy [n, k] on the host path


def _is_dev(x) -> bool:
    return torch.is_tensor(x) and x.is_cuda


def spectrum(gram: np.ndarray, n: int, k: int):
    """The PCA tables from the centred Gram matrix (fp64, host): eigh, descending order, negative eigenvalues clamped,
    the sign rule -> (components [k, D], explained_variance, explained_variance_ratio, singular_values)."""
    lam, vec = np.linalg.eigh(np.asarray(gram, np.float64))
    lam = np.maximum(lam[::-1], 0.0)
    comps = np.ascontiguousarray(vec[:, ::-1][:, :k].T)
    lead = np.argmax(np.abs(comps), axis=1)
    sign = np.sign(comps[np.arange(k), lead])
    comps *= np.where(sign == 0, 1.0, sign)[:, None]
    var = lam / (n - 1)
    return comps, var[:k].copy(), var[:k] / var.sum(), np.sqrt(lam[:k])


def _whiten_scale(var: np.ndarray) -> np.ndarray:
    return 1.0 / np.maximum(np.sqrt(var), np.finfo(np.float64).eps)


def pca(x, n_components: int = 2, whiten: bool = False) -> PCAResult:
    """PCA of the rows of ``x`` [n, D] with the semantics of ``sklearn.decomposition.PCA`` (module docstring).  A HIP
    fp32 tensor (unit column stride; the rows may be strided) runs on the device and its ``projection`` stays there; a
    host tensor or numpy array runs in float64 numpy with the same outputs."""
    dev = _is_dev(x)
    if not dev:
        x = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x)
    if x.ndim != 2:
        raise ValueError(f"pca: expected [n, D] rows, got {x.ndim} dimensions")
    n, D, k = int(x.shape[0]), int(x.shape[1]), int(n_components)
    if n < 2:
        raise ValueError(f"pca: n = {n} rows, at least 2 are needed")
    if not 1 <= k <= min(n, D):
        raise ValueError(f"pca: n_components = {k} outside [1, min(n, D) = {min(n, D)}]")
    if dev:
        if D < 4 or D > MAX_D or D % 4:
            raise ValueError(f"pca: D = {D} is not supported on the device: a multiple of 4 in [4, {MAX_D}]")
        if k > MAX_K:
            raise ValueError(f"pca: n_components = {k} exceeds the device limit of {MAX_K}")
        from . import ops
        x = x.detach()
        if x.dtype != torch.float32:
            raise TypeError(f"pca: expected torch.float32 on the device, got {x.dtype}")
        mean_d, gram_d = ops.centered_gram(x)
        mean = mean_d.cpu().numpy()                                   # the one synchronisation
        comps, var, ratio, sv = spectrum(gram_d.cpu().numpy(), n, k)
        scale = torch.from_numpy(_whiten_scale(var)).to(x.device) if whiten else None
        proj = ops.project_rows(x, mean_d, torch.from_numpy(comps).to(x.device), scale)
        return PCAResult(mean, comps, var, ratio, sv, proj)
    x64 = x.astype(np.float64)
    mean = x64.mean(axis=0)
    xc = x64 - mean
    comps, var, ratio, sv = spectrum(xc.T @ xc, n, k)
    proj = xc @ comps.T
    if whiten:
        proj = proj * _whiten_scale(var)
    return PCAResult(mean, comps, var, ratio, sv, proj)


def lab_panels(lab_names) -> Dict[int, str]:
    """The reference's panel of every lab (advanced_visualizations.py:291-306), behaviour kept: a panel entry matches
    every lab whose name CONTAINS it, case-insensitively, and a later panel overwrites an earlier one -- 'pH' also takes
    'phosphate' and 'alkaline phos.', 'PT' also takes 'PTT' (and 'MCH' takes 'MCHC', within one panel).  Labs no entry
    matches are 'Other'.  ``lab_names``: a dict index -> name or a sequence of names."""
    items = list(lab_names.items()) if isinstance(lab_names, dict) else list(enumerate(lab_names))
    out = {int(i): "Other" for i, _ in items}
    for panel, entries in PANELS:
        for entry in entries:
            e = entry.lower()
            for i, name in items:
                if e in str(name).lower():
                    out[int(i)] = panel
    return out


def density_grid(proj, degrees, grid: int = 128):
    """The patient density of the first two components: ``grid + 1`` equally spaced float64 edges from the min to the
    max of each axis (numpy.histogram2d's bin rule), per cell the patients and the sum of their lab-degrees ->
    (ex, ey, count int64 [grid, grid], wsum int64 [grid, grid])."""
    if not 1 <= grid <= MAX_GRID:
        raise ValueError(f"density_grid: grid = {grid} outside [1, {MAX_GRID}]")
    if _is_dev(proj):
        from . import ops
        lo, hi = proj[:, :2].min(dim=0).values.double().cpu().numpy(), proj[:, :2].max(dim=0).values.double().cpu().numpy()
        ex, ey = np.linspace(lo[0], hi[0], grid + 1), np.linspace(lo[1], hi[1], grid + 1)
        count, wsum = ops.grid2d(proj, torch.from_numpy(ex).to(proj.device), torch.from_numpy(ey).to(proj.device),
                                 degrees.to(device=proj.device, dtype=torch.int32).contiguous())
        return ex, ey, count.cpu().numpy(), wsum.cpu().numpy()
    p = np.asarray(proj, np.float64)
    ex, ey = np.linspace(p[:, 0].min(), p[:, 0].max(), grid + 1), np.linspace(p[:, 1].min(), p[:, 1].max(), grid + 1)
    count = np.histogram2d(p[:, 0], p[:, 1], bins=(ex, ey))[0].astype(np.int64)
    wsum = np.histogram2d(p[:, 0], p[:, 1], bins=(ex, ey), weights=np.asarray(degrees, np.float64))[0].astype(np.int64)
    return ex, ey, count, wsum


def density_frame(ex, ey, count, wsum) -> pd.DataFrame:
    gx, gy = count.shape
    ix, iy = np.meshgrid(np.arange(gx), np.arange(gy), indexing="ij")
    ix, iy = ix.reshape(-1), iy.reshape(-1)
    c, s = count.reshape(-1), wsum.reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean_degree = np.where(c > 0, s / c, np.nan)
    return pd.DataFrame({"ix": ix, "iy": iy, "x_lo": ex[ix], "x_hi": ex[ix + 1], "y_lo": ey[iy], "y_hi": ey[iy + 1],
                         "count": c, "mean_degree": mean_degree}, columns=DENSITY_COLUMNS)


def _vocab_frame(node_type, res: PCAResult, names, panels) -> pd.DataFrame:
    p = res.projection.cpu().numpy() if torch.is_tensor(res.projection) else np.asarray(res.projection)
    cols = {"idx": np.arange(p.shape[0], dtype=np.int64),
            "name": [names.get(i, f"{node_type}_{i}") for i in range(p.shape[0])]}
    if panels is not None:
        cols["panel"] = [panels.get(i, "Other") for i in range(p.shape[0])]
    for c in range(p.shape[1]):
        cols[f"pc{c + 1}"] = p[:, c]
    return pd.DataFrame(cols)


def _names_of(graph, node_type, given=None) -> Dict[int, str]:
    if given is not None:
        return dict(given) if isinstance(given, dict) else dict(enumerate(given))
    store = graph[node_type]
    meta = store.metadata if "metadata" in store else None
    return {int(i): m["label"] for i, m in meta.items() if isinstance(m, dict) and "label" in m} if meta else {}


def embedding_maps(model, graph, space: str = "initial", n_components: int = 2, grid: int = 128, output_dir=None,
                   lab_names=None):
    """PCA maps of the model's node embeddings, per node type.  ``space="initial"`` projects ``encode_nodes`` (what the
    reference plots), ``"final"`` the output of ``forward``.  Eval mode, no gradients; the training flag is restored.
    -> {"lab" / "diagnosis" / "medication": frame (idx, name, panel for labs, pc1..pck), "patient": device fp32
    [n_patients, k], "variance": one frame over the types, "density": the patient grid frame (count, mean_degree =
    the cell's mean lab-degree), "edges": (ex, ey)}.  With ``output_dir``: ``lab_embeddings_pca.csv``,
    ``diagnosis_embeddings_pca.csv``, ``medication_embeddings_pca.csv``, ``pca_explained_variance.csv``,
    ``patient_embeddings_pca.npy`` and ``patient_embedding_density.csv``."""
    if getattr(model, "_comm", None) is not None:
        raise NotImplementedError("embedding_maps on a patient-sharded model (dist.shard_model) is not supported: the "
                                  "forward's collectives need every rank; analyse with an unsharded model")
    if space not in ("initial", "final"):
        raise ValueError(f'embedding_maps: space must be "initial" or "final", got {space!r}')
    if n_components < 2:
        raise ValueError("embedding_maps: the density grid needs n_components >= 2")
    from .analysis import patient_degrees
    device = next(model.parameters()).device
    graph_dev = graph.to(device)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            x_dict = model.encode_nodes(graph_dev) if space == "initial" else model(graph_dev)
    finally:
        model.train(was_training)
    out, var_rows = {}, []
    for t in ("patient",) + VOCAB_TYPES:
        if t not in x_dict:
            continue
        res = pca(x_dict[t].detach().float(), n_components)
        for c in range(n_components):
            var_rows.append({"node_type": t, "component": c + 1, "explained_variance": res.explained_variance[c],
                             "explained_variance_ratio": res.explained_variance_ratio[c],
                             "singular_value": res.singular_values[c]})
        if t == "patient":
            out[t] = res.projection
        else:
            names = _names_of(graph, t, lab_names if t == "lab" else None)
            out[t] = _vocab_frame(t, res, names, lab_panels({i: names.get(i, f"lab_{i}") for i in
                                                             range(int(x_dict[t].shape[0]))}) if t == "lab" else None)
    out["variance"] = pd.DataFrame(var_rows, columns=VARIANCE_COLUMNS)
    deg = patient_degrees(graph_dev, device)
    ex, ey, count, wsum = density_grid(out["patient"], deg, grid)
    out["edges"] = (ex, ey)
    out["density"] = density_frame(ex, ey, count, wsum)
    if output_dir is not None:
        d = Path(output_dir)
        d.mkdir(parents=True, exist_ok=True)
        for t in VOCAB_TYPES:
            if t in out:
                out[t].to_csv(d / f"{t}_embeddings_pca.csv", index=False)
        out["variance"].to_csv(d / "pca_explained_variance.csv", index=False)
        np.save(d / "patient_embeddings_pca.npy", out["patient"].cpu().numpy())
        out["density"].to_csv(d / "patient_embedding_density.csv", index=False)
        logging.info(f"  Saved embedding maps to {d}")
    return out
