"""What the embeddings learned: PCA maps of the node embeddings, the ``visualization.dim_reduction: "pca"`` branch of the
reference's ``create_embedding_visualizations`` (``src/advanced_visualizations.py``) and ``plot_embeddings_umap``
(``src/visualize.py``), without the plotting and over EVERY patient instead of the reference's 1,000-patient sample.

``pca`` has the semantics of ``sklearn.decomposition.PCA`` 1.7: variance ``lambda / (n - 1)``, ratio over all
eigenvalues, each component signed so that its largest-magnitude entry is positive
(``svd_flip(u_based_decision=False)``), negative round-off eigenvalues clamped to 0.

A HIP tensor runs three kernels (``csrc/pca.hip``): the column means and the centred Gram matrix in fp64
(``mmg_centered_gram``, two passes over the rows), then -- after ``numpy.linalg.eigh`` of the at most 256 x 256 matrix
on the host, the one synchronisation -- the projection of every row (``mmg_project_rows``).  The patient density grid is
``mmg_grid2d``.  A host tensor or numpy array runs the same steps in float64 numpy: that path is the checker.

``tsne`` is the reference's own choice for its two embedding figures: ``sklearn.manifold.TSNE(method="exact")`` 1.7, the
O(n^2) algorithm, over one n x n fp32 buffer (``csrc/tsne.hip``: ``mmg_tsne_sqdist``, ``mmg_tsne_joint_p``,
``mmg_tsne_step``), with the same float64 numpy restatement as the host path.  Barnes-Hut and UMAP stay out of scope
(DESIGN.md section 7).
"""
from __future__ import annotations

import logging
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, Optional, Union

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


# ============================================================================ exact t-SNE
TSNE_MAX_N = 16384           # ops.TSNE_MAX_N: the n x n buffer of csrc/tsne.hip
TSNE_EPS = float(np.finfo(np.float64).eps)          # sklearn's MACHINE_EPSILON, 2^-52
TSNE_TOL = 1e-5              # _binary_search_perplexity's tolerance on the entropy
TSNE_SEARCH_STEPS = 100
TSNE_EXPLORATION_ITER = 250  # TSNE._EXPLORATION_MAX_ITER: the early-exaggeration stage
TSNE_N_ITER_CHECK = 50       # TSNE._N_ITER_CHECK
TSNE_MIN_GAIN = 0.01
TSNE_SUMMARY_COLUMNS = ["node_type", "n", "perplexity", "learning_rate", "n_iter", "kl_divergence"]


@dataclass
class TSNEResult:
    embedding: object                        # device fp64 [n, 2]; float64 numpy [n, 2] on the host path
    kl_divergence: float                     # the last computed error: the objective at `embedding`
    n_iter: int                              # the last iteration index
    learning_rate: float
    beta: object                             # fp64 [n]: the bandwidth 1 / (2 sigma_i^2) the search found per row


def tsne_sqdist_host(x) -> np.ndarray:
    """A[i, j] = sum_d (x_id - x_jd)^2 in float64 from the widened input, rounded once to fp32 (the first of the two
    places the host path rounds at); exactly symmetric, zero diagonal."""
    x64 = np.asarray(x, np.float64)
    n, D = x64.shape
    out = np.empty((n, n), np.float32)
    rows = max(1, (1 << 23) // max(n * D, 1))
    for i0 in range(0, n, rows):
        df = x64[i0:i0 + rows, None, :] - x64[None, :, :]
        out[i0:i0 + rows] = np.einsum("ijd,ijd->ij", df, df)
    out = np.triu(out, 1)
    return out + out.T


def tsne_search_host(dist, perplexity: float, margins: Optional[list] = None):
    """sklearn's _binary_search_perplexity on fp32 squared distances [n, n], every row in float64 -> (the conditional
    rows rounded to fp32 -- the second rounding place --, beta fp64 [n] of the rows returned, steps int32 [n] = the
    evaluations of H).  margins: a list that receives, per step, | |H - log perplexity| - tolerance | of the rows still
    searching (how far each decision sat from its threshold)."""
    d = np.asarray(dist, np.float32).astype(np.float64)
    n = d.shape[0]
    target = np.log(perplexity)
    beta, lo, hi = np.ones(n), np.full(n, -np.inf), np.full(n, np.inf)
    s_fin, steps = np.ones(n), np.zeros(n, np.int32)
    active = np.arange(n)
    for step in range(1, TSNE_SEARCH_STEPS + 1):
        if active.size == 0:
            break
        dd, b = d[active], beta[active]
        p = np.exp(-b[:, None] * dd)
        p[np.arange(active.size), active] = 0.0
        sp = p.sum(axis=1)
        s = np.where(sp == 0.0, 1e-8, sp)
        diff = np.log(s) + b * (dd * p).sum(axis=1) / s - target
        steps[active], s_fin[active] = step, s
        if margins is not None:
            margins.append(np.abs(np.abs(diff) - TSNE_TOL))
        go = (np.abs(diff) > TSNE_TOL) & (step < TSNE_SEARCH_STEPS)
        up = go & (diff > 0.0)
        dn = go & ~(diff > 0.0)
        a_up, a_dn = active[up], active[dn]
        lo[a_up] = beta[a_up]
        beta[a_up] = np.where(np.isinf(hi[a_up]), beta[a_up] * 2.0, (beta[a_up] + hi[a_up]) / 2.0)
        hi[a_dn] = beta[a_dn]
        beta[a_dn] = np.where(np.isinf(lo[a_dn]), beta[a_dn] / 2.0, (beta[a_dn] + lo[a_dn]) / 2.0)
        active = active[go]
    c = np.exp(-beta[:, None] * d) / s_fin[:, None]
    np.fill_diagonal(c, 0.0)
    return c.astype(np.float32), beta, steps


def tsne_joint_host(cond) -> np.ndarray:
    """P = max((C + C^T) / S, eps) as fp32 with a zero diagonal: the sum in fp32 (as sklearn has it), S = max(sum, eps)
    and the quotient in float64, rounded once."""
    c = np.asarray(cond, np.float32)
    s32 = c + c.T
    total = max(float(s32.sum(dtype=np.float64)), TSNE_EPS)
    p = np.maximum(s32.astype(np.float64) / total, TSNE_EPS).astype(np.float32)
    np.fill_diagonal(p, 0.0)
    return p


def tsne_affinities_host(x, perplexity: float):
    """-> (P fp32 [n, n], beta, steps) of the host path."""
    cond, beta, steps = tsne_search_host(tsne_sqdist_host(x), perplexity)
    return tsne_joint_host(cond), beta, steps


def tsne_objective_host(p, y, exaggeration: float = 1.0, want_kl: bool = True, sums: Optional[dict] = None):
    """sklearn's _kl_divergence at the map y [n, 2] in float64 over P fp32 [n, n] -> (KL or NaN, grad [n, 2], Z).
    sums: a dict that receives the absolute sums the rounding bounds of the tests are stated against ("grad" [n, 2] =
    4 sum_j |term_j|, "kl" = sum |term|, "z" = Z)."""
    y = np.asarray(y, np.float64)
    df = y[:, None, :] - y[None, :, :]
    num = 1.0 / (1.0 + (df[..., 0] * df[..., 0] + df[..., 1] * df[..., 1]))
    np.fill_diagonal(num, 0.0)
    z = float(num.sum())
    q = np.maximum(num / z, TSNE_EPS)
    pe = exaggeration * np.asarray(p, np.float32).astype(np.float64)
    terms = ((pe - q) * num)[:, :, None] * df
    grad = 4.0 * terms.sum(axis=1)
    kl = float("nan")
    klt = None
    if want_kl or sums is not None:
        klt = pe * np.log(np.maximum(pe, TSNE_EPS) / q)
        np.fill_diagonal(klt, 0.0)
        if want_kl:
            kl = float(klt.sum())
    if sums is not None:
        sums.update(grad=4.0 * np.abs(terms).sum(axis=1), kl=float(np.abs(klt).sum()), z=z)
    return kl, grad, z


def tsne_update_host(y, u, g, grad, momentum: float, learning_rate: float, min_gain: float = TSNE_MIN_GAIN,
                     update: bool = True) -> float:
    """The gains / momentum update of sklearn's _gradient_descent on float64 [n, 2] arrays, in place when `update`
    -> the sum of the squared gained gradient."""
    inc = u * grad < 0.0
    gain = np.maximum(np.where(inc, g + 0.2, g * 0.8), min_gain)
    gg = grad * gain
    if update:
        g[...] = gain
        u[...] = momentum * u - learning_rate * gg
        y += u
    return float((gg * gg).sum())


def tsne_descent(step, read, max_iter: int, early_exaggeration: float, n_iter_without_progress: int,
                 min_grad_norm: float):
    """The two stages of TSNE._tsne over sklearn's _gradient_descent.  step(exaggeration, momentum, want_kl, update)
    runs ONE iteration; read() -> (error, sum g^2) of the iteration just run, called after every 50th iteration and after
    a stage's last (on the device: the only host synchronisation).  Iterations 0 .. 249 run at momentum 0.5 on
    P * early_exaggeration with n_iter_without_progress = 250, the rest at 0.8; each stage keeps its own best error and
    breaks on no progress or on grad_norm <= min_grad_norm.  The error _gradient_descent hands back is the objective
    BEFORE its last update; here one more evaluation without an update follows, so that the error returned is the
    objective AT the returned map -> (that error, the last iteration index)."""
    error, it = float(np.finfo(np.float64).max), 0
    stages = ((0, TSNE_EXPLORATION_ITER, 0.5, early_exaggeration, TSNE_EXPLORATION_ITER),
              (None, max_iter, 0.8, 1.0, n_iter_without_progress))
    for first, last, momentum, exaggeration, patience in stages:
        first = it + 1 if first is None else first
        error = best_error = float(np.finfo(np.float64).max)
        best_iter = it = first
        for it in range(first, last):
            check = (it + 1) % TSNE_N_ITER_CHECK == 0
            want = check or it == last - 1
            step(exaggeration, momentum, want, True)
            if want:
                error, g2 = read()
            if check:
                if error < best_error:
                    best_error, best_iter = error, it
                elif it - best_iter > patience:
                    break
                if np.sqrt(g2) <= min_grad_norm:
                    break
    step(1.0, 0.8, True, False)
    return read()[0], it


def tsne(x, n_components: int = 2, perplexity: float = 30.0, early_exaggeration: float = 12.0,
         learning_rate: Union[str, float] = "auto", max_iter: int = 1000, n_iter_without_progress: int = 300,
         min_grad_norm: float = 1e-7, init="pca") -> TSNEResult:
    """Exact t-SNE of the rows of ``x`` [n, D] into 2 dimensions with the semantics of sklearn 1.7
    ``TSNE(method="exact")``: the perplexity search and joint probabilities of ``_joint_probabilities``, the objective
    ``_kl_divergence``, ``_gradient_descent``'s gains, momentum and stopping rules in ``TSNE._tsne``'s two stages
    (``tsne_descent``); ``learning_rate="auto"`` is ``max(n / early_exaggeration / 4, 50)``.  ``init="pca"`` is this
    module's ``pca(x, 2).projection / std(first column) * 1e-4``; an [n, 2] array is taken as it is; ``"random"`` is not
    offered (the draw would have to match numpy's).

    A HIP fp32 tensor (unit column stride, D a multiple of 4 in [4, 256], 4 <= n <= 16384) runs ``csrc/tsne.hip`` over one
    n x n fp32 buffer; ``embedding`` and ``beta`` stay on the device and the host reads two doubles every 50
    iterations.  A host tensor or numpy array runs the same steps in float64 numpy, the n x n matrix rounded to fp32 at
    the same two places (distances, probabilities): that path is the checker.

    ``kl_divergence`` is the last computed error and ``n_iter`` the last iteration index.  Where sklearn differs beyond
    rounding: it keeps the map, the update and the gains in fp32 (here float64); it multiplies P by the exaggeration and
    divides it again in place in fp32 (here P is never changed; the factor is applied in float64 where P is read); and
    its ``kl_divergence_`` is the objective before the last update, where this one is evaluated once more at the
    returned map."""
    if int(n_components) != 2:
        raise ValueError(f"tsne: n_components = {n_components}; the map has 2 components")
    dev = _is_dev(x)
    if not dev:
        x = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x)
    if x.ndim != 2:
        raise ValueError(f"tsne: expected [n, D] rows, got {x.ndim} dimensions")
    n, D = int(x.shape[0]), int(x.shape[1])
    if n < 4:
        raise ValueError(f"tsne: n = {n} rows, at least 4 are needed")
    if not 0.0 < float(perplexity) < n:
        raise ValueError(f"tsne: perplexity = {perplexity} must be positive and less than n = {n}")
    if int(max_iter) < TSNE_EXPLORATION_ITER:
        raise ValueError(f"tsne: max_iter = {max_iter} is below the {TSNE_EXPLORATION_ITER} iterations of the first stage")
    if isinstance(init, str) and init != "pca":
        raise ValueError(f'tsne: init must be "pca" or an [n, 2] array, got {init!r}')
    if not isinstance(init, str) and tuple(init.shape) != (n, 2):
        raise ValueError(f"tsne: init must be [{n}, 2], got {tuple(init.shape)}")
    if isinstance(learning_rate, str):
        if learning_rate != "auto":
            raise ValueError(f'tsne: learning_rate must be "auto" or a number, got {learning_rate!r}')
        lr = max(n / early_exaggeration / 4.0, 50.0)
    else:
        lr = float(learning_rate)
    if dev:
        if n > TSNE_MAX_N:
            raise ValueError(f"tsne: n = {n} exceeds the device limit of {TSNE_MAX_N}")
        if D < 4 or D > MAX_D or D % 4:
            raise ValueError(f"tsne: D = {D} is not supported on the device: a multiple of 4 in [4, {MAX_D}]")
        x = x.detach()
        if x.dtype != torch.float32:
            raise TypeError(f"tsne: expected torch.float32 on the device, got {x.dtype}")
        if not bool(torch.isfinite(x).all()):
            raise ValueError("tsne: x holds non-finite values")
        from . import ops
        if isinstance(init, str):
            proj = pca(x, 2).projection.double()
            y = proj / proj[:, 0].std(unbiased=False) * 1e-4
        else:
            y = torch.as_tensor(init).to(device=x.device, dtype=torch.float64)
        y = y.contiguous().clone()
        a = ops.tsne_sqdist(x)
        beta, _ = ops.tsne_joint_p(a, perplexity)
        u, g = torch.zeros_like(y), torch.ones_like(y)
        stats = torch.empty(3, dtype=torch.float64, device=x.device)

        def step(exaggeration, momentum, want_kl, update):
            ops.tsne_step(a, y, u, g, stats, exaggeration, momentum, lr, TSNE_MIN_GAIN, want_kl, update)

        def read():
            s = stats.cpu().numpy()                                   # the synchronisation: after every 50th iteration
            return float(s[0]), float(s[1])
    else:
        if not np.all(np.isfinite(x)):
            raise ValueError("tsne: x holds non-finite values")
        if isinstance(init, str):
            proj = pca(x, 2).projection
            y = proj / np.std(proj[:, 0]) * 1e-4
        else:
            y = np.asarray(init.detach().cpu().numpy() if torch.is_tensor(init) else init)
        y = np.array(y, np.float64)
        a, beta, _ = tsne_affinities_host(x, perplexity)
        u, g = np.zeros_like(y), np.ones_like(y)
        last = [0.0, 0.0]

        def step(exaggeration, momentum, want_kl, update):
            last[0], grad, _ = tsne_objective_host(a, y, exaggeration, want_kl)
            last[1] = tsne_update_host(y, u, g, grad, momentum, lr, TSNE_MIN_GAIN, update)

        def read():
            return last[0], last[1]
    error, it = tsne_descent(step, read, int(max_iter), float(early_exaggeration), int(n_iter_without_progress),
                             float(min_grad_norm))
    return TSNEResult(y, float(error), int(it), float(lr), beta)


def embedding_tsne(model, graph, space: str = "initial", perplexity: float = 30.0, max_points: int = 1000, seed: int = 42,
                   output_dir=None, lab_names=None):
    """t-SNE maps of the model's node embeddings, per node type: what the reference's
    ``create_embedding_visualizations`` draws, without the drawing.  ``space`` as for ``embedding_maps``; eval mode, no
    gradients; the training flag is restored.  Per type the perplexity is ``min(perplexity, n - 1)``; more than
    ``max_points`` (at most 16384) patients are sampled without replacement by ``numpy.random.RandomState(seed)`` (the
    reference's draw is unseeded).
    -> {"lab" / "diagnosis" / "medication": frame (idx, name, panel for labs, tsne1, tsne2), "patient": frame
    (patient_idx, tsne1, tsne2, lab_degree), "summary": frame (node_type, n, perplexity, learning_rate, n_iter,
    kl_divergence)}.  With ``output_dir``: ``{lab,diagnosis,medication}_embeddings_tsne.csv``,
    ``patient_embeddings_tsne.csv`` and ``tsne_summary.csv``."""
    if getattr(model, "_comm", None) is not None:
        raise NotImplementedError("embedding_tsne on a patient-sharded model (dist.shard_model) is not supported: the "
                                  "forward's collectives need every rank; analyse with an unsharded model")
    if space not in ("initial", "final"):
        raise ValueError(f'embedding_tsne: space must be "initial" or "final", got {space!r}')
    if not 4 <= int(max_points) <= TSNE_MAX_N:
        raise ValueError(f"embedding_tsne: max_points = {max_points} outside [4, {TSNE_MAX_N}]")
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
    out, rows = {}, []
    for t in VOCAB_TYPES + ("patient",):
        if t not in x_dict:
            continue
        x = x_dict[t].detach().float()
        n_all = int(x.shape[0])
        pick = None
        if t == "patient" and n_all > max_points:
            pick = np.random.RandomState(seed).choice(n_all, int(max_points), replace=False)
            x = x[torch.from_numpy(pick).to(x.device)]
        n = int(x.shape[0])
        perp = min(float(perplexity), float(n - 1))
        res = tsne(x.contiguous(), perplexity=perp)
        emb = res.embedding.cpu().numpy() if torch.is_tensor(res.embedding) else np.asarray(res.embedding)
        rows.append({"node_type": t, "n": n, "perplexity": perp, "learning_rate": res.learning_rate, "n_iter": res.n_iter,
                     "kl_divergence": res.kl_divergence})
        if t == "patient":
            idx = np.arange(n_all, dtype=np.int64) if pick is None else pick.astype(np.int64)
            deg = patient_degrees(graph_dev, device if device.type == "cuda" else None)
            deg = deg.cpu().numpy() if torch.is_tensor(deg) else np.asarray(deg)
            out[t] = pd.DataFrame({"patient_idx": idx, "tsne1": emb[:, 0], "tsne2": emb[:, 1],
                                   "lab_degree": deg.astype(np.int64)[idx]})
        else:
            names = _names_of(graph, t, lab_names if t == "lab" else None)
            cols = {"idx": np.arange(n, dtype=np.int64), "name": [names.get(i, f"{t}_{i}") for i in range(n)]}
            if t == "lab":
                panels = lab_panels({i: names.get(i, f"lab_{i}") for i in range(n)})
                cols["panel"] = [panels.get(i, "Other") for i in range(n)]
            cols["tsne1"], cols["tsne2"] = emb[:, 0], emb[:, 1]
            out[t] = pd.DataFrame(cols)
    out["summary"] = pd.DataFrame(rows, columns=TSNE_SUMMARY_COLUMNS)
    if output_dir is not None:
        d = Path(output_dir)
        d.mkdir(parents=True, exist_ok=True)
        for t in VOCAB_TYPES + ("patient",):
            if t in out:
                out[t].to_csv(d / f"{t}_embeddings_tsne.csv", index=False)
        out["summary"].to_csv(d / "tsne_summary.csv", index=False)
        logging.info(f"  Saved t-SNE maps to {d}")
    return out
