"""Per-lab stacked recalibration of imputed lab values: the number a clinician sees, corrected out of sample.

The reference's own log asks three times for "per-lab calibration or ensemble with baseline".  ``LabStacker`` is that
step: per lab x patient lab-degree bin (the cells of ``conformal.LabConformal``) a ridge regression of the TARGET on K
predictors -- by convention the GNN prediction first, then baselines such as the per-lab mean -- fitted on a held-out
split and applied to every later prediction:

    y = w_0 + w_1 f_1 + ... + w_K f_K

DIRECTION.  This regresses the target on the predictors (``target ~ w . phi``): applying it moves a prediction toward
the truth.  ``analysis.create_per_lab_calibration_table`` fits the reference's diagnostic line the other way round
(``pred = a * true + b``, on the very pairs it scores) and is never applied to anything.  Neither is a bug; do not
"fix" one into the other.

Definitions (this module's numpy functions are the definition; ``tests/stack_ref.py`` restates them with loops):

* cells, and the pairs dropped (``dropped[4]``: lab out of range, patient out of range, degree in no bin, a NaN in the
  target or any feature, the first that applies) as in ``conformal``.
* folds: ``fold(patient) = mix32(rng_key(seed, ST_SITE) ^ patient) mod folds`` -- the first word of the project's
  counter-based RNG under a site of its own: a function of the patient alone.
* sums per (fold, cell): the upper triangle of ``sum phi phi^T`` (row-major; the (0, 0) entry is the count), ``sum phi t``
  and ``sum t^2`` in fp64, in the fixed order of include/mmgnn_stack.h (a segment's pairs in input order, chunks of
  4096, slot t adds the pairs t, t + 256, .., butterfly over 64 slots, four waves in order, chunks in order).
* solve: three levels (cell, lab, all pairs), ridge toward ``e = (0, 1, 0, ..)``: ``A = G + ridge * diag(G)``,
  ``rhs = h + ridge * diag(G) e``, Cholesky in fp64 without fused multiply-add; a level is usable with
  ``m >= max(min_count, K + 2)`` pairs and pivots above ``1e-10 * A_ii``; a cell takes the first usable level, else ``e``
  (level 3), which leaves ``f_1`` as it is.
* ``folds >= 2`` adds, for every fold j, the coefficients fitted WITHOUT fold j; ``cross_fit_predict`` gives every pair
  the prediction of the coefficients that never saw its patient.

HIP tensors run the kernels of libmmgnn_stack.so (csrc/stack.hip) and EQUAL the numpy path, which serves numpy inputs
and is the checker; it is never a silent fallback for device tensors.  Ridge only, at most four predictors; no isotonic
or quantile recalibration and no plotting.
"""
from __future__ import annotations

import logging
from pathlib import Path
from typing import Optional, Sequence

import numpy as np
import pandas as pd
import torch

from .analysis import _edges, _is_dev, _lab_name, patient_degrees
from .bootstrap import _key, _mix32
from .evaluate import baseline_matrix, baseline_pairs, fit_baselines
from .conformal import (DEFAULT_BINS, DEFAULT_LABELS, _h_f32, _h_idx, _predict_split, _t_f32, _t_idx, host_cells)

ST_SITE = 0x53544B31                  # MMG_ST_SITE, "STK1"
ST_CHUNK = 4096                       # MMG_ST_CHUNK
ST_MAX_FEATURES, ST_MAX_FOLDS = 4, 8
PIVOT_REL = 1e-10                     # MMG_ST_PIVOT_REL
LEVELS = ("cell", "lab", "all", "none")
DROP_KINDS = ("lab_out_of_range", "patient_out_of_range", "degree_in_no_bin", "nan_value")
SCORE_FIELDS = ("n", "abs_raw", "sq_raw", "abs_stacked", "sq_stacked")
SCORE_COLUMNS = ["scope", "key", "n", "mae_raw", "mae_stacked", "rmse_raw", "rmse_stacked"]
_F32, _U32 = np.float32, np.uint32


# ============================================================================ the numpy restatement
def n_fields(n_features: int) -> int:
    k = int(n_features)
    return (k + 1) * (k + 2) // 2 + k + 2


def folds_out(folds: int) -> int:
    return int(folds) + 1 if int(folds) > 1 else 1


def host_folds(patient, folds: int, seed: int = 0) -> np.ndarray:
    """fold of every patient index (int64, in [0, 2^31)) -> int64."""
    p = np.asarray(patient).astype(np.int64)
    if int(folds) <= 1:
        return np.zeros(p.shape, np.int64)
    w0 = _mix32(_U32(_key(seed, ST_SITE)) ^ p.astype(_U32))
    return (w0 % _U32(folds)).astype(np.int64)


def host_fit_terms(feats, target) -> np.ndarray:
    """float64 [n, F]: the additive terms of every pair; each is the exact product of two fp32 values."""
    t = np.asarray(target, _F32).astype(np.float64)
    phi = [np.ones(t.size)] + [np.asarray(f, _F32).astype(np.float64) for f in feats]
    with np.errstate(all="ignore"):
        cols = [phi[a] * phi[b] for a in range(len(phi)) for b in range(a, len(phi))]
        cols += [p * t for p in phi] + [t * t]
    return np.stack(cols, axis=1) if t.size else np.zeros((0, len(cols)))


def host_score_terms(raw, stacked, target) -> np.ndarray:
    t = np.asarray(target, _F32)
    cols = [np.ones(t.size)]
    with np.errstate(all="ignore"):
        for p in (raw, stacked):
            e = t - np.asarray(p, _F32)                              # fp32
            e64 = e.astype(np.float64)
            cols += [np.abs(e).astype(np.float64), e64 * e64]
    return np.stack(cols, axis=1) if t.size else np.zeros((0, len(cols)))


def host_segment_sums(terms, seg, n_seg: int, chunk: int = ST_CHUNK, block: int = 32) -> np.ndarray:
    """float64 [n_seg, F]: per segment the sum of the rows of ``terms`` [n, F] with ``seg`` in [0, n_seg) (every other
    row belongs to none), in the documented order."""
    terms, seg = np.asarray(terms, np.float64), np.asarray(seg).astype(np.int64)
    F = terms.shape[1]
    keep = np.flatnonzero((seg >= 0) & (seg < n_seg))
    order = keep[np.argsort(seg[keep], kind="stable")]
    S = seg[order]
    X = np.concatenate([terms[order], np.zeros((1, F))])            # the last row: the +0 an idle slot holds
    m = S.size
    lo = np.searchsorted(S, np.arange(n_seg), "left")
    hi = np.searchsorted(S, np.arange(n_seg), "right")
    n_chunks = (hi - lo + chunk - 1) // chunk
    first = np.cumsum(n_chunks) - n_chunks                           # a segment's chunks, listed segment after segment
    total = int(n_chunks.sum())
    c_seg = np.repeat(np.arange(n_seg), n_chunks)
    c_j = np.arange(total) - first[c_seg]
    c_begin = lo[c_seg] + c_j * chunk
    c_end = np.minimum(c_begin + chunk, hi[c_seg])
    part = np.zeros((total, F))
    lane = np.arange(64)
    with np.errstate(all="ignore"):
        for c0 in range(0, total, block):
            c1 = min(c0 + block, total)
            pos = c_begin[c0:c1, None] + np.arange(chunk)[None, :]
            pos = np.where(pos < c_end[c0:c1, None], pos, m)
            x = X[pos].reshape(c1 - c0, chunk // 256, 256, F)
            acc = np.zeros((c1 - c0, 256, F))
            for q in range(chunk // 256):                            # slot t: the pairs t, t + 256, ..
                acc = acc + x[:, q]
            v = acc.reshape(c1 - c0, 4, 64, F)
            for o in (32, 16, 8, 4, 2, 1):                           # the butterfly of a wave
                v = v + v[:, :, lane ^ o]
            tot = np.zeros((c1 - c0, F))
            for w in range(4):                                       # the waves in order
                tot = tot + v[:, w, 0]
            part[c0:c1] = tot
        sums = np.zeros((n_seg, F))
        for j in range(int(n_chunks.max()) if n_seg and total else 0):   # the chunks of a segment in order
            sel = np.flatnonzero(n_chunks > j)
            sums[sel] = sums[sel] + part[first[sel] + j]
    return sums


def _host_keep(values, patient, lab, n_labs, deg, edges):
    """-> (cell int64 [n], kind int64 [n]: -1 kept, 0 .. 3 the drop kinds, dropped int64 [4])."""
    cell, kind, _ = host_cells(patient, lab, n_labs, deg, edges)
    nan = np.zeros(cell.shape, bool)
    for v in values:
        nan |= np.isnan(v)
    kind = np.where((kind < 0) & nan, 3, kind)
    return cell, kind, np.bincount(kind[kind >= 0], minlength=4).astype(np.int64)


def host_sums(feats, target, patient, lab, n_labs: int, deg, edges, folds: int = 1, seed: int = 0):
    """mmg_stack_sums in numpy -> (sums float64 [folds, n_cells, F], dropped int64 [4])."""
    feats = [np.asarray(f, _F32).reshape(-1) for f in feats]
    target = np.asarray(target, _F32).reshape(-1)
    n_cells = n_labs * (len(edges) - 1)
    cell, kind, dropped = _host_keep(feats + [target], patient, lab, n_labs, deg, edges)
    seg = np.where(kind < 0, host_folds(np.where(kind < 0, patient, 0), folds, seed) * n_cells + cell, folds * n_cells)
    sums = host_segment_sums(host_fit_terms(feats, target), seg, folds * n_cells)
    return sums.reshape(folds, n_cells, n_fields(len(feats))), dropped


def host_systems(S, n_features: int, ridge: float, min_count: int):
    """The systems of the header over sums S float64 [n_sys, F] -> (w float64 [n_sys, K + 1], usable bool [n_sys], m
    float64 [n_sys]); w of an unusable system is meaningless."""
    S = np.asarray(S, np.float64)
    K, P, n = int(n_features), int(n_features) + 1, S.shape[0]
    A, q = np.zeros((P, P, n)), 0
    for a in range(P):
        for b in range(a, P):
            A[a, b] = A[b, a] = S[:, q]
            q += 1
    r = [S[:, q + a].copy() for a in range(P)]
    m = A[0, 0].copy()
    ridge = np.float64(ridge)
    with np.errstate(all="ignore"):
        ok = m >= float(max(int(min_count), K + 2))
        r[1] = r[1] + ridge * A[1, 1]
        for a in range(P):
            A[a, a] = A[a, a] + ridge * A[a, a]
        L = np.zeros((P, P, n))
        for i in range(P):
            for j in range(i + 1):
                s = A[i, j].copy()
                for k in range(j):
                    s = s - L[i, k] * L[j, k]
                if j < i:
                    L[i, j] = s / L[j, j]
                else:
                    ok = ok & (s > PIVOT_REL * A[i, i])
                    L[i, i] = np.sqrt(s)
        z = [None] * P
        for i in range(P):
            s = r[i]
            for k in range(i):
                s = s - L[i, k] * z[k]
            z[i] = s / L[i, i]
        w = [None] * P
        for i in range(P - 1, -1, -1):
            s = z[i]
            for k in range(i + 1, P):
                s = s - L[k, i] * w[k]
            w[i] = s / L[i, i]
    return np.stack(w, axis=1), ok, m


def host_training_sums(sums):
    """sums [folds, n_cells, F] -> T [folds_out, n_cells, F]: row j the folds but j added in fold order, the last row
    every fold."""
    folds = sums.shape[0]
    rows = []
    with np.errstate(all="ignore"):
        for jo in range(folds_out(folds)):
            t = np.zeros(sums.shape[1:])
            for fo in range(folds):
                if folds == 1 or fo != jo:
                    t = t + sums[fo]
            rows.append(t)
    return np.stack(rows)


def _host_groups(x, gs: int):
    """[.., n_groups * gs, F] -> [.., n_groups, F]: the members of a group added in order from 0."""
    x = x.reshape(x.shape[:-2] + (x.shape[-2] // gs, gs, x.shape[-1]))
    t = np.zeros(x.shape[:-2] + x.shape[-1:])
    with np.errstate(all="ignore"):
        for i in range(gs):
            t = t + x[..., i, :]
    return t


def host_solve(sums, n_labs: int, n_bins: int, n_features: int, ridge: float, min_count: int):
    """mmg_stack_solve in numpy -> (coef float64 [folds_out, n_cells, K + 1], level int32, n_used int32 [folds_out,
    n_cells])."""
    K, n_cells = int(n_features), n_labs * n_bins
    T = host_training_sums(np.asarray(sums, np.float64))
    fo, F = T.shape[0], T.shape[2]
    labs = _host_groups(T, n_bins)                                   # [fo, n_labs, F]
    everything = _host_groups(labs, n_labs)                          # [fo, 1, F]
    lab_of = np.arange(n_cells) // n_bins
    lv = [host_systems(T.reshape(-1, F), K, ridge, min_count), host_systems(labs.reshape(-1, F), K, ridge, min_count),
          host_systems(everything.reshape(-1, F), K, ridge, min_count)]
    w = [lv[0][0].reshape(fo, n_cells, K + 1), lv[1][0].reshape(fo, n_labs, K + 1)[:, lab_of],
         np.broadcast_to(lv[2][0].reshape(fo, 1, K + 1), (fo, n_cells, K + 1))]
    ok = [lv[0][1].reshape(fo, n_cells), lv[1][1].reshape(fo, n_labs)[:, lab_of],
          np.broadcast_to(lv[2][1].reshape(fo, 1), (fo, n_cells))]
    m = [lv[0][2].reshape(fo, n_cells), lv[1][2].reshape(fo, n_labs)[:, lab_of],
         np.broadcast_to(lv[2][2].reshape(fo, 1), (fo, n_cells))]
    level = np.where(ok[0], 0, np.where(ok[1], 1, np.where(ok[2], 2, 3))).astype(np.int32)
    e = np.zeros(K + 1)
    e[1] = 1.0
    coef = np.broadcast_to(e, (fo, n_cells, K + 1)).copy()
    n_used = np.zeros((fo, n_cells), np.int32)
    for k in range(3):
        pick = level == k
        coef[pick] = w[k][pick]
        n_used[pick] = m[k][pick].astype(np.int32)
    return coef, level, n_used


def host_apply_pairs(feats, patient, lab, n_labs: int, deg, edges, coef, seed: int = 0, cross: bool = False):
    """mmg_stack_apply_pairs in numpy -> fp32 [n]."""
    feats = [np.asarray(f, _F32).reshape(-1) for f in feats]
    n_cells = coef.shape[1]
    folds = coef.shape[0] - 1 if coef.shape[0] > 1 else 1
    if cross and folds < 2:
        raise ValueError("out-of-fold coefficients need folds >= 2")
    cell, kind, _ = host_cells(patient, lab, n_labs, deg, edges)
    has = kind < 0
    c = np.where(has, cell, 0)
    row = host_folds(np.where(has, patient, 0), folds, seed) if cross else np.full(c.shape, coef.shape[0] - 1)
    if n_cells == 0 or not c.size:
        return feats[0].copy()
    w = coef[row, c]                                                 # [n, K + 1]
    with np.errstate(all="ignore"):
        y = w[:, 0]
        for k, f in enumerate(feats):
            y = y + w[:, k + 1] * f.astype(np.float64)
        y = y.astype(_F32)
    return np.where(has, y, feats[0]).astype(_F32)


def host_apply_matrix(feats, rows, deg, edges, coef, seed: int = 0, cross: bool = False):
    """mmg_stack_apply_matrix in numpy: feats[0] fp32 [n_rows, n_labs], the others such a matrix or [n_labs]."""
    f0 = np.asarray(feats[0], _F32)
    n_rows, n_labs = f0.shape
    rows = np.arange(n_rows, dtype=np.int64) if rows is None else np.asarray(rows).astype(np.int64)
    flat = [np.ascontiguousarray(np.broadcast_to(np.asarray(f, _F32), (n_rows, n_labs))).reshape(-1) for f in feats]
    out = host_apply_pairs(flat, np.repeat(rows, n_labs), np.tile(np.arange(n_labs, dtype=np.int64), n_rows), n_labs, deg,
                           edges, coef, seed, cross)
    return out.reshape(n_rows, n_labs)


def host_scores(raw, stacked, target, patient, lab, n_labs: int, deg, edges):
    """mmg_stack_scores in numpy -> (scores float64 [n_cells + n_labs + 1, 5], dropped int64 [4])."""
    raw, stacked, target = (np.asarray(x, _F32).reshape(-1) for x in (raw, stacked, target))
    n_bins = len(edges) - 1
    n_cells = n_labs * n_bins
    cell, kind, dropped = _host_keep([raw, stacked, target], patient, lab, n_labs, deg, edges)
    cells = host_segment_sums(host_score_terms(raw, stacked, target), np.where(kind < 0, cell, n_cells), n_cells)
    labs = _host_groups(cells, n_bins)
    return np.concatenate([cells, labs, _host_groups(labs, n_labs)]), dropped


# ============================================================================ the public object
def _feature_seq(features):
    """A sequence or dict of K predictors -> list (a dict in its insertion order)."""
    if torch.is_tensor(features) or isinstance(features, np.ndarray):
        feats = [features]
    else:
        feats = list(features.values()) if isinstance(features, dict) else list(features)
    if not 1 <= len(feats) <= ST_MAX_FEATURES:
        raise ValueError(f"a stacker takes 1 to {ST_MAX_FEATURES} predictors, got {len(feats)}")
    return feats


class LabStacker:
    """Ridge stacking per (lab, patient lab-degree bin): ``fit`` on a held-out split, then ``predict`` /
    ``predict_matrix`` give the recalibrated value and ``scores`` compares before and after on another split.  With
    ``folds >= 2`` ``cross_fit_predict`` gives out-of-fold predictions on the fitting split itself.  HIP tensors run the
    kernels; numpy arrays run the numpy restatement of this module."""

    def __init__(self, bins: Sequence = DEFAULT_BINS, ridge: float = 1e-3, min_count: int = 30, folds: int = 1, seed: int = 0,
                 labels: Optional[Sequence[str]] = None):
        if not (float(ridge) >= 0.0 and np.isfinite(float(ridge))):
            raise ValueError(f"ridge must be finite and not negative, got {ridge}")
        if int(min_count) < 0:
            raise ValueError("min_count must not be negative")
        if not 1 <= int(folds) <= ST_MAX_FOLDS:
            raise ValueError(f"folds must lie in [1, {ST_MAX_FOLDS}], got {folds}")
        if labels is None:
            labels = DEFAULT_LABELS if tuple(bins) == tuple(DEFAULT_BINS) else tuple(
                f"bin{j}" for j in range(len(list(bins)) - 1))
        self.ridge, self.min_count, self.folds, self.seed = float(ridge), int(min_count), int(folds), int(seed)
        self.edges = _edges(bins, labels)
        self.labels = tuple(labels)
        self.n_labs: Optional[int] = None
        self.n_features: Optional[int] = None
        self.feature_names: Optional[tuple] = None
        self._host = None            # (coef, level, n_used, dropped) as numpy
        self._deg = None             # host degrees, int32
        self._dev = {}               # device -> (coef, deg) tensors

    # ---- state
    @property
    def n_bins(self) -> int:
        return len(self.edges) - 1

    @property
    def fitted(self) -> bool:
        return self._host is not None

    def _need(self):
        if not self.fitted:
            raise RuntimeError("LabStacker: call fit() or load_state_dict() first")
        return self._host

    coef = property(lambda self: self._need()[0])          # [folds_out, n_cells, K + 1]; the last row: all pairs
    level = property(lambda self: self._need()[1])
    n_used = property(lambda self: self._need()[2])
    dropped = property(lambda self: self._need()[3])

    def _on(self, dev):
        if dev not in self._dev:
            self._dev[dev] = (torch.from_numpy(self.coef).to(dev), torch.from_numpy(self._deg).to(dev))
        return self._dev[dev]

    def set_degrees(self, graph_or_degrees):
        """The patient degrees ``predict`` / ``scores`` bin by (``fit`` keeps the ones it was given)."""
        self._deg = np.ascontiguousarray(np.asarray(patient_degrees(graph_or_degrees, None)), np.int32)
        self._dev = {}
        return self

    def _features(self, features, dev):
        feats = _feature_seq(features)
        if self.n_features is not None and len(feats) != self.n_features:
            raise ValueError(f"LabStacker: fitted on {self.n_features} predictors, got {len(feats)}")
        if dev is not None:
            return [_t_f32(f, dev) for f in feats]
        return [_h_f32(f) for f in feats]

    @staticmethod
    def _indices(patient_indices, lab_indices, dev):
        if dev is None:
            return _h_idx(patient_indices, "patient_indices"), _h_idx(lab_indices, "lab_indices")
        pi, li = _t_idx(patient_indices, dev), _t_idx(lab_indices, dev)
        if pi.dtype != li.dtype:
            pi, li = pi.to(torch.int64), li.to(torch.int64)
        return pi, li

    # ---- fit
    def fit(self, features, target, lab_indices, patient_indices, graph_or_degrees, n_labs: Optional[int] = None):
        feats = _feature_seq(features)
        dev = feats[0].device if _is_dev(feats[0]) else None
        if n_labs is None:
            try:
                n_labs = int(graph_or_degrees["lab"].num_nodes)
            except (TypeError, KeyError, IndexError, AttributeError, ValueError):
                li = lab_indices
                n_labs = (int(li.max()) + 1) if (li.numel() if torch.is_tensor(li) else np.size(li)) else 1
        self.n_labs, self.n_features = int(n_labs), len(feats)
        self.feature_names = tuple(features) if isinstance(features, dict) else tuple(f"f{k + 1}" for k in range(len(feats)))
        feats = self._features(feats, dev)
        pi, li = self._indices(patient_indices, lab_indices, dev)
        if dev is not None:
            from . import stack_ops as so
            deg = patient_degrees(graph_or_degrees, dev)
            sums, dropped = so.stack_sums(feats, _t_f32(target, dev), pi, li, self.n_labs, deg, self.edges, self.folds,
                                          self.seed)
            coef, level, n_used = so.stack_solve(sums, self.n_labs, self.n_bins, self.n_features, self.ridge, self.min_count)
            self._deg = deg.cpu().numpy().astype(np.int32)
            self._host = (coef.cpu().numpy(), level.cpu().numpy(), n_used.cpu().numpy(), dropped.cpu().numpy())
            self._dev = {dev: (coef, deg)}
        else:
            self.set_degrees(graph_or_degrees)
            sums, dropped = host_sums(feats, _h_f32(target), pi, li, self.n_labs, self._deg, self.edges, self.folds, self.seed)
            self._host = host_solve(sums, self.n_labs, self.n_bins, self.n_features, self.ridge, self.min_count) + (dropped,)
        d = self.dropped
        if int(d.sum()):
            logging.info("  stacker fit: dropped pairs " + ", ".join(f"{k}={int(v)}" for k, v in zip(DROP_KINDS, d)))
        return self

    # ---- apply
    def _apply(self, features, lab_indices, patient_indices, cross: bool):
        self._need()
        feats = _feature_seq(features)
        dev = feats[0].device if _is_dev(feats[0]) else None
        feats = self._features(feats, dev)
        pi, li = self._indices(patient_indices, lab_indices, dev)
        if dev is not None:
            from . import stack_ops as so
            coef, deg = self._on(dev)
            return so.stack_apply_pairs(feats, pi, li, self.n_labs, deg, self.edges, coef, self.seed, cross)
        return host_apply_pairs(feats, pi, li, self.n_labs, self._deg, self.edges, self.coef, self.seed, cross)

    def predict(self, features, lab_indices, patient_indices):
        """The stacked prediction fp32 [n] under the coefficients of all fitting pairs: a tensor on the device of the
        features or a numpy array."""
        return self._apply(features, lab_indices, patient_indices, False)

    def cross_fit_predict(self, features, lab_indices, patient_indices):
        """The out-of-fold prediction: every pair under the coefficients fitted without its own patient's fold -- for
        the pairs ``fit`` saw, a prediction that never saw them.  Needs ``folds >= 2``."""
        if self.folds < 2:
            raise ValueError("cross_fit_predict needs a stacker with folds >= 2")
        return self._apply(features, lab_indices, patient_indices, True)

    def predict_matrix(self, feature_matrices, patient_indices=None):
        """The stacked prediction [n_rows, n_labs] of dense predictions (a row of ``impute_lab_matrix`` per patient).
        The first entry is the matrix; every other entry is such a matrix or a 1-D ``[n_labs]`` vector broadcast over the
        rows (the per-lab mean).  ``patient_indices``: the patient of every row, None: row i is patient i."""
        self._need()
        feats = _feature_seq(feature_matrices)
        if len(feats) != self.n_features:
            raise ValueError(f"LabStacker: fitted on {self.n_features} predictors, got {len(feats)}")
        f0 = feats[0]
        if f0.ndim != 2 or int(f0.shape[1]) != self.n_labs:
            raise ValueError(f"predict_matrix: expected [n_rows, {self.n_labs}], got {tuple(f0.shape)}")
        if _is_dev(f0):
            from . import stack_ops as so
            dev = f0.device
            coef, deg = self._on(dev)
            ms = []
            for f in feats:
                x = (f if torch.is_tensor(f) else torch.from_numpy(np.ascontiguousarray(f))).detach().to(dev)
                if x.dtype != torch.float32 or (x.dim() == 2 and x.shape[1] > 1 and x.stride(1) != 1) or \
                        (x.dim() == 1 and not x.is_contiguous()):
                    x = x.float().contiguous()
                ms.append(x)
            rows = None if patient_indices is None else _t_idx(patient_indices, dev)
            return so.stack_apply_matrix(ms, rows, deg, self.edges, coef, self.seed, False)
        hs = [(f.detach().cpu().numpy() if torch.is_tensor(f) else np.asarray(f)).astype(_F32, copy=False) for f in feats]
        rows = None if patient_indices is None else _h_idx(patient_indices, "patient_indices")
        return host_apply_matrix(hs, rows, self._deg, self.edges, self.coef, self.seed, False)

    # ---- scores
    def score_sums(self, features, target, lab_indices, patient_indices, stacked=None):
        """Per cell, per lab and overall (float64 [n_cells + n_labs + 1, 5]: n, sum |t - f_1|, sum (t - f_1)^2, sum |t -
        y|, sum (t - y)^2) as numpy, and the dropped counts.  ``stacked``: y, default ``predict(features, ..)``."""
        self._need()
        feats = _feature_seq(features)
        dev = feats[0].device if _is_dev(feats[0]) else None
        y = self.predict(features, lab_indices, patient_indices) if stacked is None else stacked
        pi, li = self._indices(patient_indices, lab_indices, dev)
        if dev is not None:
            from . import stack_ops as so
            _, deg = self._on(dev)
            s, d = so.stack_scores(_t_f32(feats[0], dev), _t_f32(y, dev), _t_f32(target, dev), pi, li, self.n_labs, deg,
                                   self.edges)
            return s.cpu().numpy(), d.cpu().numpy()
        return host_scores(_h_f32(feats[0]), _h_f32(y), _h_f32(target), pi, li, self.n_labs, self._deg, self.edges)

    def scores(self, features, target, lab_indices, patient_indices, lab_names=None, stacked=None) -> pd.DataFrame:
        """One row overall, per lab and per cell: n, MAE and RMSE of the raw first predictor and of the stacked value."""
        s, _ = self.score_sums(features, target, lab_indices, patient_indices, stacked)
        return scores_frame(s, self.n_labs, self.labels, lab_names)

    # ---- tables
    def table_frame(self, lab_names=None) -> pd.DataFrame:
        """The coefficients fitted on all pairs: one row per cell."""
        nb = self.n_bins
        cells = np.arange(self.n_labs * nb)
        cols = {"lab_idx": cells // nb,
                "lab_name": [_lab_name(lab_names, int(c // nb)) for c in cells],
                "degree_bin": [self.labels[int(c % nb)] for c in cells],
                "n_used": self.n_used[-1].astype(np.int64),
                "level": [LEVELS[int(v)] for v in self.level[-1]],
                "intercept": self.coef[-1][:, 0]}
        for k, name in enumerate(self.feature_names):
            cols[f"w_{name}"] = self.coef[-1][:, k + 1]
        return pd.DataFrame(cols)

    def state_dict(self) -> dict:
        """The table with what it needs to be applied, as a plain dict of numpy arrays and scalars: it ships with a
        checkpoint."""
        self._need()
        return {"ridge": self.ridge, "min_count": self.min_count, "folds": self.folds, "seed": self.seed,
                "edges": [float(e) for e in self.edges], "labels": list(self.labels), "n_labs": self.n_labs,
                "n_features": self.n_features, "feature_names": list(self.feature_names), "coef": self.coef.copy(),
                "level": self.level.copy(), "n_used": self.n_used.copy(), "dropped": self.dropped.copy(),
                "degrees": self._deg.copy()}

    def load_state_dict(self, state: dict):
        self.__init__(state["edges"], state["ridge"], state["min_count"], state["folds"], state["seed"], state["labels"])
        self.n_labs, self.n_features = int(state["n_labs"]), int(state["n_features"])
        self.feature_names = tuple(state["feature_names"])
        host = tuple(np.ascontiguousarray(np.asarray(state[k]), dt) for k, dt in
                     (("coef", np.float64), ("level", np.int32), ("n_used", np.int32), ("dropped", np.int64)))
        want = (folds_out(self.folds), self.n_labs * self.n_bins, self.n_features + 1)
        if host[0].shape != want:
            raise ValueError(f"load_state_dict: coefficients of shape {host[0].shape}, expected {want}")
        self._host = host
        self._deg = np.ascontiguousarray(np.asarray(state["degrees"]), np.int32)
        return self


def scores_frame(scores, n_labs: int, labels, lab_names=None) -> pd.DataFrame:
    """The rows of ``score_sums`` -> (scope, key, n, mae_raw, mae_stacked, rmse_raw, rmse_stacked): overall, every lab,
    every cell."""
    s, nb = np.asarray(scores), len(labels)
    n_cells = n_labs * nb

    def row(scope, key, v):
        n = float(v[0])
        f = (lambda x: x / n) if n > 0 else (lambda x: np.nan)
        return {"scope": scope, "key": key, "n": int(n), "mae_raw": f(v[1]), "mae_stacked": f(v[3]),
                "rmse_raw": np.sqrt(f(v[2])), "rmse_stacked": np.sqrt(f(v[4]))}

    rows = [row("overall", "all", s[n_cells + n_labs])]
    rows += [row("lab", _lab_name(lab_names, l), s[n_cells + l]) for l in range(n_labs)]
    rows += [row("cell", f"{_lab_name(lab_names, c // nb)}|{labels[c % nb]}", s[c]) for c in range(n_cells)]
    return pd.DataFrame(rows, columns=SCORE_COLUMNS)


# ============================================================================ drivers
def _train_edges(graph_dev, masker, dev):
    tr_ei, tr_v, _, _ = masker.get_masked_data("train", want_mask=False)
    return tr_ei.to(dev), tr_v.to(dev).reshape(-1).float()


def _split_features(model, graph, masker, split: str, fitted: dict):
    """-> (graph on the device, {name: fp32 [n]} with the model's prediction first, y, pi, li)."""
    graph_dev, pred, y, pi, li = _predict_split(model, graph, masker, split)
    feats = {"gnn": pred}
    for name, bm in fitted.items():
        feats[name] = baseline_pairs(bm, pi, li)
    return graph_dev, feats, y, pi, li


def _fit_named_baselines(model, graph, masker, baselines, n_neighbors: int = 5):
    dev = next(model.parameters()).device
    graph_dev = graph.to(dev)
    tr_ei, tr_v = _train_edges(graph_dev, masker, dev)
    return fit_baselines(tuple(baselines), tr_ei, tr_v, int(graph["lab"].num_nodes), int(graph["patient"].num_nodes),
                         n_neighbors)


def fit_stacker(model, graph, masker, split: str = "val", baselines: Sequence[str] = ("per_lab_mean",),
                return_baselines: bool = False, **kw):
    """Predict the pairs of ``split`` (eval mode), fit the named baselines on the TRAIN edges exactly as
    ``evaluate_with_intervals`` does, and fit a ``LabStacker(**kw)`` on (GNN prediction, baselines...) of the split.
    -> the stacker (and, with ``return_baselines``, the fitted baselines ``impute_stacked`` takes)."""
    fitted = _fit_named_baselines(model, graph, masker, baselines)
    graph_dev, feats, y, pi, li = _split_features(model, graph, masker, split, fitted)
    st = LabStacker(**kw).fit(feats, y, li, pi, graph_dev, n_labs=int(graph["lab"].num_nodes))
    return (st, fitted) if return_baselines else st


def stacking_report(model, graph, masker, output_dir=None, calibration: str = "val", evaluation: str = "test",
                    baselines: Sequence[str] = ("per_lab_mean",), replicates: int = 1000, confidence: float = 0.95,
                    lab_names=None, **kw):
    """Fit on one split, evaluate on another -> (LabStacker, table frame, scores frame, comparison frame).  The
    comparison is ``bootstrap_metrics(stacked, .., baseline=raw)``: the paired difference stacked - raw of every metric
    with its patient-cluster bootstrap interval (a negative MAE difference: stacking helped).  With ``output_dir``
    writes ``stacking_table.csv``, ``stacking_scores.csv`` and ``stacking_comparison.csv``."""
    from .bootstrap import bootstrap_metrics
    st, fitted = fit_stacker(model, graph, masker, calibration, baselines, return_baselines=True, **kw)
    graph_dev, feats, y, pi, li = _split_features(model, graph, masker, evaluation, fitted)
    if lab_names is None:
        meta = graph["lab"].metadata if "metadata" in graph["lab"] else None
        if meta:
            lab_names = {idx: m["label"] for idx, m in meta.items()}
    stacked = st.predict(feats, li, pi)
    table = st.table_frame(lab_names)
    scores = st.scores(feats, y, li, pi, lab_names, stacked=stacked)
    comparison = bootstrap_metrics(stacked, y, pi, li, graph_dev, replicates=replicates, confidence=confidence,
                                   seed=st.seed, baseline=feats["gnn"], n_sigma=0.0, lab_names=lab_names).comparison
    if output_dir is not None:
        out = Path(output_dir)
        out.mkdir(parents=True, exist_ok=True)
        table.to_csv(out / "stacking_table.csv", index=False)
        scores.to_csv(out / "stacking_scores.csv", index=False)
        comparison.to_csv(out / "stacking_comparison.csv", index=False)
        logging.info(f"  Saved stacking tables to {out}")
    return st, table, scores, comparison


def impute_stacked(model, data, stacker: LabStacker, baselines: dict, conformal=None,
                   patient_indices: Optional[torch.Tensor] = None):
    """(stacked, raw, observed) -- with ``conformal`` (a ``LabConformal`` fitted on STACKED predictions) (point, lower,
    upper, raw, observed) -- each [n, L], from ONE ``impute_lab_matrix`` forward and the matrix epilogue.  ``baselines``:
    the fitted baselines of ``fit_stacker(.., return_baselines=True)``, in the order the stacker was fitted with."""
    from .inference import impute_missing
    was_training = model.training
    model.eval()                                             # impute_lab_matrix is inference-only
    try:
        raw, observed = impute_missing(model, data, patient_indices)
    finally:
        model.train(was_training)
    rows = None if patient_indices is None else patient_indices.to(raw.device)
    feats = [raw] + [baseline_matrix(bm, rows, int(raw.shape[1])) for bm in baselines.values()]
    stacked = stacker.predict_matrix(feats, patient_indices)
    if conformal is None:
        return stacked, raw, observed
    point, lower, upper = conformal.predict_matrix(stacked, patient_indices)
    return point, lower, upper, raw, observed


def fit_stacker_and_conformal(model, graph, masker, folds: int = 5, split: str = "val",
                              baselines: Sequence[str] = ("per_lab_mean",), alpha: float = 0.1, score: str = "signed",
                              stacker_kw: Optional[dict] = None, conformal_kw: Optional[dict] = None):
    """Both tables from ONE held-out split: the stacker is cross-fitted on ``split`` (``folds`` patient folds), and the
    conformal table is fitted on the OUT-OF-FOLD stacked predictions of the same pairs -- residuals of predictions that
    never saw their own patient.  The intervals then carry the cross-conformal guarantee (Vovk 2015; Barber et al. 2021:
    coverage about 1 - 2 alpha in the worst case, close to 1 - alpha in practice), NOT the exact split-conformal
    theorem: the deployed coefficients are those of all folds, not the ones the residuals were taken under.
    -> (LabStacker, LabConformal, fitted baselines)."""
    from .conformal import LabConformal
    if int(folds) < 2:
        raise ValueError("fit_stacker_and_conformal cross-fits: folds >= 2")
    fitted = _fit_named_baselines(model, graph, masker, baselines)
    graph_dev, feats, y, pi, li = _split_features(model, graph, masker, split, fitted)
    n_labs = int(graph["lab"].num_nodes)
    st = LabStacker(folds=folds, **(stacker_kw or {})).fit(feats, y, li, pi, graph_dev, n_labs=n_labs)
    oof = st.cross_fit_predict(feats, li, pi)
    kw = dict(bins=st.edges, labels=st.labels)
    kw.update(conformal_kw or {})
    cf = LabConformal(alpha=alpha, score=score, **kw).fit(oof, y, li, pi, graph_dev, n_labs=n_labs)
    return st, cf, fitted
