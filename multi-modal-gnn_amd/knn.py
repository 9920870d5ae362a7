"""Nearest-neighbour lab imputation: the reference config's third baseline (``evaluation.baselines: nearest_neighbor``,
"predict from most similar patient") with the semantics of ``sklearn.impute.KNNImputer(n_neighbors, weights)``
``.fit_transform(X)`` over the dense patient x lab matrix of observed values (NaN = not observed).

The O(patients^2 x labs) distance and top-k work is one HIP kernel (``mmg_knn_impute``, csrc/knn.hip); this module builds
the matrix on the device and gathers cells.  There is no CPU fallback: host tensors are refused after validation.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib, ops

MAX_LABS = 512
MAX_NEIGHBORS = 32


def _as_index(t, name: str) -> torch.Tensor:
    t = torch.as_tensor(t)
    if t.dim() != 1:
        raise ValueError(f"{name} must be 1-D, got shape {list(t.shape)}")
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"{name} must hold integers, got {t.dtype}")
    return t


def _require_device(*ts):
    for t in ts:
        if not t.is_cuda:
            raise _lib.MmgError(f"KNNLabImputer: expected HIP device tensors, got {t.device} (no CPU fallback)")


class KNNLabImputer:
    """``fit`` the (patient, lab, value) triples, then ``impute_matrix`` / ``predict``: every patient is a donor for every
    other patient; an observed cell is passed through; a lab nobody has stays NaN."""

    def __init__(self, n_neighbors: int = 5, weights: str = "uniform"):
        self.n_neighbors = n_neighbors
        self.weights = weights
        self.X: Optional[torch.Tensor] = None

    def fit(self, patient_indices, lab_indices, values, n_patients: int, n_labs: int) -> "KNNLabImputer":
        if not (isinstance(self.n_neighbors, int) and 1 <= self.n_neighbors <= MAX_NEIGHBORS):
            raise ValueError(f"n_neighbors must be an int in [1, {MAX_NEIGHBORS}], got {self.n_neighbors!r}")
        if self.weights not in ops.KNN_WEIGHTS:
            raise ValueError(f"weights must be 'uniform' or 'distance', got {self.weights!r}")
        if not 1 <= int(n_labs) <= MAX_LABS:
            raise ValueError(f"n_labs must be in [1, {MAX_LABS}], got {n_labs}")
        if not 1 <= int(n_patients) < 2 ** 31:
            raise ValueError(f"n_patients must be in [1, 2^31), got {n_patients}")
        n_patients, n_labs = int(n_patients), int(n_labs)
        p = _as_index(patient_indices, "patient_indices")
        lab = _as_index(lab_indices, "lab_indices")
        v = torch.as_tensor(values)
        if v.dim() == 2 and v.shape[1] == 1:
            v = v[:, 0]
        if not (p.numel() == lab.numel() == v.numel()) or v.dim() != 1:
            raise ValueError(f"patient_indices, lab_indices and values must have one entry per cell, got "
                             f"{p.numel()}, {lab.numel()} and shape {list(v.shape)}")
        if not (p.device == lab.device == v.device):
            raise ValueError(f"inputs on different devices: {p.device}, {lab.device}, {v.device}")
        if p.numel():
            if int(p.min()) < 0 or int(p.max()) >= n_patients:
                raise ValueError(f"patient index outside [0, {n_patients})")
            if int(lab.min()) < 0 or int(lab.max()) >= n_labs:
                raise ValueError(f"lab index outside [0, {n_labs})")
        if bool(torch.isnan(v).any()):
            raise ValueError("values hold NaN: NaN marks a missing cell and cannot be an observation")
        key = p.to(torch.int64) * n_labs + lab.to(torch.int64)
        if torch.unique(key).numel() != key.numel():
            raise ValueError("duplicate (patient, lab) pairs")
        _require_device(p, lab, v)
        X = torch.full((n_patients, n_labs), float("nan"), dtype=torch.float32, device=v.device)
        X[p.to(torch.int64), lab.to(torch.int64)] = v.to(torch.float32)
        self.X = X
        return self

    def _check_fitted(self):
        if self.X is None:
            raise RuntimeError("KNNLabImputer: call fit() first")

    def _rows(self, patient_indices) -> torch.Tensor:
        n_patients = self.X.shape[0]
        if patient_indices is None:
            return torch.arange(n_patients, dtype=torch.int32, device=self.X.device)
        p = _as_index(patient_indices, "patient_indices").to(self.X.device)
        if p.numel() and (int(p.min()) < 0 or int(p.max()) >= n_patients):
            raise ValueError(f"patient index outside [0, {n_patients})")
        return p.to(torch.int32).contiguous()

    def impute_matrix(self, patient_indices=None) -> torch.Tensor:
        """-> fp32 [rows, n_labs]: every lab of every requested patient (default: all, in order)."""
        self._check_fitted()
        return ops.knn_impute(self.X, self._rows(patient_indices), self.n_neighbors, self.weights)

    def predict(self, patient_indices, lab_indices) -> torch.Tensor:
        """-> fp32 [n]: the imputed value of each (patient, lab) cell; one kernel call over the unique patients."""
        self._check_fitted()
        rows = self._rows(patient_indices)
        lab = _as_index(lab_indices, "lab_indices").to(self.X.device).to(torch.int64)
        if lab.numel() != rows.numel():
            raise ValueError(f"{rows.numel()} patients but {lab.numel()} labs")
        if lab.numel() and (int(lab.min()) < 0 or int(lab.max()) >= self.X.shape[1]):
            raise ValueError(f"lab index outside [0, {self.X.shape[1]})")
        uniq, inv = torch.unique(rows, return_inverse=True)
        m = ops.knn_impute(self.X, uniq.to(torch.int32).contiguous(), self.n_neighbors, self.weights)
        return m[inv, lab]
