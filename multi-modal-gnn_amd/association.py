"""Lab association: which labs are measured together, and how their values move together.

The reference draws a missingness heatmap of 100 patients x 50 labs (``src/visualize.py``, ``plot_missingness_heatmap``)
"to show which labs are commonly ordered together"; no number comes out of it.  This module computes the numbers over
ALL rows: on a patient x lab matrix with NaN for "not measured",

* the co-observation counts ``N = M^T M`` and what follows from them per lab pair -- ``jaccard = nab / (na + nb - nab)``
  and ``lift = nab * n / (na * nb)`` (1: ordered independently; above 1: a panel);
* the pairwise-complete covariance and Pearson correlation of every lab pair over the rows that have BOTH --
  ``pandas.DataFrame.cov(min_periods=)`` / ``.corr(min_periods=)``.

When the matrix holds residuals ``prediction - target`` (``error_association``) the same tables say how correlated a
patient's errors across labs are -- why ``mmgnn.bootstrap`` resamples patients -- and, for values, which lab is worth
offering ``LabStacker`` as an extra predictor.

Definitions (this module's numpy functions are the definition; ``tests/assoc_ref.py`` restates them pair by pair):

* a cell is observed when it is finite.  NaN is "not measured"; an infinite cell is treated as missing by the kernels
  and counted, and the public functions raise ``ValueError`` when there is one.
* with ``m_ia = [X_ia observed]``, ``u_ia = m_ia * (float64(X_ia) - center[a])`` and ``q_ia = u_ia * u_ia`` the four
  planes are ``N = m^T m``, ``SX = u^T m``, ``SXX = q^T m``, ``SXY = u^T u``; ``SY`` and ``SYY`` are the transposes of
  ``SX`` and ``SXX``.  ``center`` defaults to the column means: neither ``cov`` nor ``r`` depends on it, and with the
  means the step ``SXY - SX * SY / nab`` cancels little (a lab with mean 1e4 and std 1 keeps its digits).
* ``cxy = SXY - SX * SY / nab``, ``vx = SXX - SX * SX / nab``, ``vy = SYY - SY * SY / nab``;
  ``cov = cxy / (nab - 1)``, NaN when ``nab < max(min_periods, 2)``; ``r = cxy / sqrt(vx * vy)`` clipped to [-1, 1], NaN
  when ``nab < max(min_periods, 1)`` or ``vx * vy`` is not greater than 0 (a constant lab, one row).

HIP tensors run the kernels of libmmgnn_assoc.so (csrc/assoc.hip): the products on ``v_mfma_f64_16x16x4_f64``, every
fp64 sum in an order fixed by (n, L) alone.  numpy arrays (and CPU tensors) run the float64 restatement of this module,
which is the checker and never a silent substitute for the kernels.  Pearson only: no Spearman or Kendall, no partial
correlation, no panel clustering, no plotting; at most 512 labs.
"""
from __future__ import annotations

import logging
from pathlib import Path
from typing import NamedTuple, Optional

import numpy as np
import pandas as pd
import torch

from .analysis import _is_dev, _lab_name
from .data import LAB_EDGE

MAX_LABS = 512                        # MMG_AS_MAX_LABS
Z95 = 1.959963984540054               # the 97.5 % point of the standard normal
PAIR_COLUMNS = ["lab_a", "lab_b", "n", "jaccard", "lift", "r", "r_lower", "r_upper"]
COVERAGE_COLUMNS = ["lab", "patients", "coverage", "mean", "std"]


class PairMoments(NamedTuple):
    planes: object                    # fp64 [4, L, L]: N, SX, SXX, SXY
    count: object                     # int64 [L]
    center: object                    # fp64 [L]


class LabAssociation(NamedTuple):
    n: object                         # int64 [L, L]: rows that have both labs
    r: object                         # fp64 [L, L]
    cov: object
    jaccard: object
    lift: object
    count: object                     # int64 [L]
    mean: object                      # fp64 [L]
    n_rows: int = 0


# ============================================================================ the numpy restatement
def _host_matrix(X) -> np.ndarray:
    X = np.asarray(X.detach().cpu().numpy() if torch.is_tensor(X) else X)
    if X.ndim != 2:
        raise ValueError(f"X must be a 2-D matrix [patients, labs], got shape {list(X.shape)}")
    return np.ascontiguousarray(X, np.float32)


def host_colstats(X):
    """-> (count int64 [L], mean fp64 [L] -- 0 for a lab nobody has --, number of infinite cells)."""
    X = _host_matrix(X)
    obs = np.isfinite(X)
    count = obs.sum(0).astype(np.int64)
    s = np.where(obs, X.astype(np.float64), 0.0).sum(0)
    mean = np.divide(s, count, out=np.zeros(X.shape[1], np.float64), where=count > 0)
    return count, mean, int(np.isinf(X).sum())


def host_moments(X, center) -> np.ndarray:
    """The planes N, SX, SXX, SXY (fp64 [4, L, L]) of X about `center`."""
    X = _host_matrix(X)
    obs = np.isfinite(X)
    m = obs.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        u = np.where(obs, X.astype(np.float64) - np.asarray(center, np.float64)[None, :], 0.0)
    q = u * u
    return np.stack([m.T @ m, u.T @ m, q.T @ m, u.T @ u])


def host_finish(planes, count, n: int, min_periods: int = 1):
    """planes [4, L, L], count [L] -> (r, cov, jaccard, lift): the arithmetic of mmg_assoc_finish, operation by
    operation."""
    nab, sx, sxx, sxy = (np.asarray(p, np.float64) for p in planes)
    sy, syy = sx.T, sxx.T
    c = np.asarray(count).astype(np.float64)
    ca, cb = c[:, None], c[None, :]
    mp = float(min_periods)
    with np.errstate(all="ignore"):
        cxy = sxy - sx * sy / nab
        vx = sxx - sx * sx / nab
        vy = syy - sy * sy / nab
        cov = np.where(nab >= max(mp, 2.0), cxy / (nab - 1.0), np.nan)
        den = vx * vy
        r = np.clip(cxy / np.sqrt(den), -1.0, 1.0)
        r = np.where((nab >= max(mp, 1.0)) & (den > 0.0), r, np.nan)
        uni = ca + cb - nab
        jaccard = np.where(uni == 0.0, np.nan, nab / uni)
        lift = (nab * float(n)) / (ca * cb)
    return r, cov, jaccard, lift


# ============================================================================ the public functions
def _check_shape(n: int, L: int):
    if not 1 <= L <= MAX_LABS:
        raise ValueError(f"the matrix has {L} labs, outside [1, {MAX_LABS}]")
    if not 1 <= n < 2 ** 31:
        raise ValueError(f"the matrix has {n} patients, outside [1, 2^31)")


def _dev_matrix(X: torch.Tensor) -> torch.Tensor:
    if X.dim() != 2:
        raise ValueError(f"X must be a 2-D matrix [patients, labs], got shape {list(X.shape)}")
    X = X.detach()
    if X.dtype != torch.float32:
        X = X.float()
    return X if X.shape[1] <= 1 or X.stride(1) == 1 else X.contiguous()


def _refuse_inf(n_inf: int):
    if n_inf:
        raise ValueError(f"X holds {n_inf} infinite cells: a lab value is finite, and NaN marks a missing one")


def pairwise_moments(X, center=None) -> PairMoments:
    """The four pairwise-complete moment planes of X [patients, labs] about ``center`` (None: the column means), the
    per-lab counts and the centre used.  A HIP tensor runs the kernels and returns device tensors."""
    if _is_dev(X):
        from . import assoc_ops
        X = _dev_matrix(X)
        _check_shape(*X.shape)
        count, mean, n_inf = assoc_ops.assoc_colstats(X)
        _refuse_inf(int(n_inf.item()))
        if center is not None:
            mean = torch.as_tensor(center, dtype=torch.float64).reshape(-1).to(X.device).contiguous()
        return PairMoments(assoc_ops.assoc_moments(X, mean), count, mean)
    X = _host_matrix(X)
    _check_shape(*X.shape)
    count, mean, n_inf = host_colstats(X)
    _refuse_inf(n_inf)
    if center is not None:
        mean = np.asarray(center.detach().cpu().numpy() if torch.is_tensor(center) else center, np.float64).reshape(-1)
        if mean.size != X.shape[1]:
            raise ValueError(f"center must hold {X.shape[1]} values, got {mean.size}")
    return PairMoments(host_moments(X, mean), count, mean)


def lab_correlation(X, min_periods: int = 1) -> LabAssociation:
    """``pandas.DataFrame(X).corr(min_periods=)`` and ``.cov(min_periods=)`` of the labs, with the co-observation
    counts, Jaccard index and lift of every lab pair."""
    if int(min_periods) < 0:
        raise ValueError(f"min_periods must not be negative, got {min_periods}")
    mom = pairwise_moments(X)
    n = int(X.shape[0]) if hasattr(X, "shape") else len(X)
    if _is_dev(X):
        from . import assoc_ops
        r, cov, jaccard, lift = assoc_ops.assoc_finish(mom.planes, mom.count, n, int(min_periods))
        nab = mom.planes[0].to(torch.int64)
    else:
        r, cov, jaccard, lift = host_finish(mom.planes, mom.count, n, int(min_periods))
        nab = mom.planes[0].astype(np.int64)
    return LabAssociation(nab, r, cov, jaccard, lift, mom.count, mom.center, n)


def lab_matrix(patient_indices, lab_indices, values, n_patients: int, n_labs: int):
    """The dense [n_patients, n_labs] fp32 matrix of (patient, lab, value) triples, NaN where there is none, under the
    checks of ``KNNLabImputer.fit``: indices in range, no NaN value, no duplicate pair.  HIP tensors give a device
    matrix, anything else a numpy array."""
    if not 1 <= int(n_labs) <= MAX_LABS:
        raise ValueError(f"n_labs must be in [1, {MAX_LABS}], got {n_labs}")
    if not 1 <= int(n_patients) < 2 ** 31:
        raise ValueError(f"n_patients must be in [1, 2^31), got {n_patients}")
    n_patients, n_labs = int(n_patients), int(n_labs)
    dev = _is_dev(values)
    if dev:
        as_t = lambda x: x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))           # noqa: E731
    else:
        as_t = lambda x: torch.as_tensor(x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x))   # noqa: E731
    p, lab, v = as_t(patient_indices), as_t(lab_indices), as_t(values).detach()
    for t, name in ((p, "patient_indices"), (lab, "lab_indices")):
        if t.dim() != 1:
            raise ValueError(f"{name} must be 1-D, got shape {list(t.shape)}")
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError(f"{name} must hold integers, got {t.dtype}")
    if v.dim() == 2 and v.shape[1] == 1:
        v = v[:, 0]
    if not (p.numel() == lab.numel() == v.numel()) or v.dim() != 1:
        raise ValueError(f"patient_indices, lab_indices and values must have one entry per cell, got "
                         f"{p.numel()}, {lab.numel()} and shape {list(v.shape)}")
    if not (p.device == lab.device == v.device):
        raise ValueError(f"inputs on different devices: {p.device}, {lab.device}, {v.device}")
    p, lab = p.to(torch.int64), lab.to(torch.int64)
    if p.numel():
        if int(p.min()) < 0 or int(p.max()) >= n_patients:
            raise ValueError(f"patient index outside [0, {n_patients})")
        if int(lab.min()) < 0 or int(lab.max()) >= n_labs:
            raise ValueError(f"lab index outside [0, {n_labs})")
    if bool(torch.isnan(v).any()):
        raise ValueError("values hold NaN: NaN marks a missing cell and cannot be an observation")
    key = p * n_labs + lab
    if torch.unique(key).numel() != key.numel():
        raise ValueError("duplicate (patient, lab) pairs")
    X = torch.full((n_patients, n_labs), float("nan"), dtype=torch.float32, device=v.device)
    X[p, lab] = v.to(torch.float32)
    return X if dev else X.numpy()


def _np(x) -> np.ndarray:
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def fisher_interval(r, n, z: float = Z95):
    """The Fisher-z interval of a correlation r over n rows -> (lower, upper); NaN for n <= 3."""
    r, n = np.asarray(r, np.float64), np.asarray(n, np.float64)
    with np.errstate(all="ignore"):
        zr = np.arctanh(r)
        half = z / np.sqrt(n - 3.0)
        ok = n > 3.0
        return np.where(ok, np.tanh(zr - half), np.nan), np.where(ok, np.tanh(zr + half), np.nan)


def association_pairs(assoc: LabAssociation, names=None, min_periods: int = 30) -> pd.DataFrame:
    """The long form of the tables: one row per lab pair a < b with at least ``min_periods`` common rows -- lab_a,
    lab_b, n, jaccard, lift, r and its 95 % Fisher-z interval (n > 3) --, by ``|r|`` descending (a pair without a
    correlation last), then by (a, b).  Computed on the host over the L x L tables."""
    nab, r, jac, lift = _np(assoc.n), _np(assoc.r), _np(assoc.jaccard), _np(assoc.lift)
    L = nab.shape[0]
    a, b = np.triu_indices(L, 1)
    keep = nab[a, b] >= max(int(min_periods), 0)
    a, b = a[keep], b[keep]
    rr, nn = r[a, b], nab[a, b]
    lower, upper = fisher_interval(rr, nn)
    order = np.lexsort((b, a, -np.where(np.isnan(rr), -1.0, np.abs(rr))))
    frame = pd.DataFrame({"lab_a": [_lab_name(names, int(i)) for i in a], "lab_b": [_lab_name(names, int(i)) for i in b],
                          "n": nn.astype(np.int64), "jaccard": jac[a, b], "lift": lift[a, b], "r": rr, "r_lower": lower,
                          "r_upper": upper}, columns=PAIR_COLUMNS)
    return frame.iloc[order].reset_index(drop=True)


def coverage_frame(assoc: LabAssociation, names=None) -> pd.DataFrame:
    """Per lab: the patients that have it, its coverage, the mean and the std (``sqrt(cov[a, a])``) of its values."""
    count, mean, cov = _np(assoc.count), _np(assoc.mean), _np(assoc.cov)
    with np.errstate(invalid="ignore"):
        std = np.sqrt(np.diagonal(cov))
    return pd.DataFrame({"lab": [_lab_name(names, i) for i in range(count.size)], "patients": count.astype(np.int64),
                         "coverage": count / float(assoc.n_rows), "mean": mean, "std": std}, columns=COVERAGE_COLUMNS)


def _square_frame(table, names) -> pd.DataFrame:
    table = _np(table)
    labels = [_lab_name(names, i) for i in range(table.shape[0])]
    return pd.DataFrame(table, index=labels, columns=labels)


def _graph_names(graph):
    meta = graph["lab"].metadata if "metadata" in graph["lab"] else None
    return {idx: m["label"] for idx, m in meta.items()} if meta else None


def _tables(X, names, min_periods: int, output_dir, files: dict):
    """lab_correlation of X and its frames; `files`: frame name -> file name of those that are written."""
    assoc = lab_correlation(X, min_periods)
    frames = {"comeasurement": _square_frame(assoc.n, names), "correlation": _square_frame(assoc.r, names),
              "pairs": association_pairs(assoc, names, min_periods), "coverage": coverage_frame(assoc, names)}
    if output_dir is not None:
        out = Path(output_dir)
        out.mkdir(parents=True, exist_ok=True)
        for key, fname in files.items():
            frames[key].to_csv(out / fname, index=key in ("comeasurement", "correlation"))
        logging.info(f"  Saved lab association tables to {out}")
    return assoc, frames


def lab_association(graph, output_dir=None, min_periods: int = 30, lab_names=None):
    """The association tables of ALL patients' has_lab edges -> (LabAssociation, {"comeasurement", "correlation",
    "pairs", "coverage": frames}).  A graph on a HIP device runs the kernels, one on the host the numpy restatement.
    With ``output_dir`` writes ``lab_comeasurement.csv`` (the counts), ``lab_correlation.csv``,
    ``lab_association_pairs.csv`` and ``lab_coverage.csv``."""
    ei = graph[LAB_EDGE].edge_index
    X = lab_matrix(ei[0], ei[1], graph[LAB_EDGE].edge_attr.reshape(-1), int(graph["patient"].num_nodes),
                   int(graph["lab"].num_nodes))
    return _tables(X, lab_names if lab_names is not None else _graph_names(graph), min_periods, output_dir,
                   {"comeasurement": "lab_comeasurement.csv", "correlation": "lab_correlation.csv",
                    "pairs": "lab_association_pairs.csv", "coverage": "lab_coverage.csv"})


def residual_matrix(model, graph, masker, split: str = "test"):
    """The dense [patients, labs] matrix of ``prediction - target`` on the split's edges (NaN elsewhere), from one
    ``predict_lab_values`` call in eval mode, on the model's device."""
    from .conformal import _predict_split
    graph_dev, pred, y, pi, li = _predict_split(model, graph, masker, split)
    return lab_matrix(pi, li, pred - y, int(graph["patient"].num_nodes), int(graph["lab"].num_nodes))


def error_association(model, graph, masker, split: str = "test", output_dir=None, min_periods: int = 30,
                      lab_names=None):
    """The same tables for the residuals ``prediction - target`` on the split's edges: how a patient's errors move
    together across labs.  With ``output_dir`` writes ``error_correlation.csv`` and ``error_association_pairs.csv``."""
    X = residual_matrix(model, graph, masker, split)
    return _tables(X, lab_names if lab_names is not None else _graph_names(graph), min_periods, output_dir,
                   {"correlation": "error_correlation.csv", "pairs": "error_association_pairs.csv"})
