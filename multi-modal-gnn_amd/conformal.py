"""Split-conformal prediction intervals for imputed labs: how far off may ``impute_lab_matrix`` be?

A held-out split (the validation edges of ``EdgeMasker`` / ``PatientHoldoutSplitter``) gives, per lab x patient
lab-degree bin, exact order statistics of the residuals ``target - pred``.  Every imputed cell then gets an interval
``[pred + q_lo, pred + q_hi]`` whose coverage of at least ``1 - alpha`` is a finite-sample theorem -- under
exchangeability of the calibration pairs and the new pair ("Prediction intervals": a lab that was
never measured is not a random holdout, so there the guarantee is only as good as missing-at-random).  The model is not
changed.

Definitions (this module's numpy functions are the definition; ``tests/conformal_ref.py`` restates them with loops):

* key: ``r = target - pred`` in fp32 (``score="signed"``) or ``|r|`` (``score="absolute"``).  A pair is dropped, and
  counted in ``dropped[4]``, under the first of: lab outside [0, n_labs); patient outside [0, n_patients); degree in no
  bin (bins are half open, ``[bins[j], bins[j + 1])``); NaN key.
* segments at three levels: cell = ``lab * n_bins + bin``; lab; all pairs.  With the m keys of a segment ascending,
  signed: ``k_lo = floor((m + 1) * (alpha / 2))``, ``k_hi = ceil((m + 1) * (1 - alpha / 2))``, ``q_lo = x_(k_lo)``,
  ``q_hi = x_(k_hi)``, ``shift`` = the median; absolute: ``k_hi = ceil((m + 1) * (1 - alpha))``, ``q_hi = x_(k_hi)``,
  ``q_lo = -q_hi``, ``shift = 0``.  fp64 rank arithmetic, every operation rounded on its own.  A segment is usable when
  all its ranks exist (``k_lo >= 1``, ``k_hi <= m``) and ``m >= min_count``.
* table: one row per cell from the first usable level of (cell, lab, all); none: ``(-inf, +inf, 0)``, level 3.
* apply: ``lower = p + q_lo``, ``upper = p + q_hi``, ``point = p + shift`` (``point="median"``) or ``p``; a pair
  without a cell takes ``(-inf, +inf, 0)``.

HIP tensors run the kernels of libmmgnn_conformal.so (csrc/conformal.hip) and EQUAL the numpy path, which serves numpy
inputs and is the checker; the only sums (interval widths of ``coverage``) are fixed-order fp64 on the device.
"""
from __future__ import annotations

import logging
from pathlib import Path
from typing import Optional, Sequence

import numpy as np
import pandas as pd
import torch

from .analysis import _edges, _is_dev, _lab_name, patient_degrees
from .train import LAB_EDGE

DEFAULT_BINS = (0, 6, 16, np.inf)          # the model's degree gate (6) and the reference's strata; every degree
DEFAULT_LABELS = ("0-5", "6-15", "16+")
SCORES = ("signed", "absolute")
LEVELS = ("cell", "lab", "all", "none")
DROP_KINDS = ("lab_out_of_range", "patient_out_of_range", "degree_in_no_bin", "nan_key")
COV_FIELDS = ("n", "covered", "below", "above", "infinite", "dropped")
TABLE_COLUMNS = ["lab_idx", "lab_name", "degree_bin", "n_used", "level", "q_lo", "q_hi", "shift"]
COVERAGE_COLUMNS = ["scope", "key", "n", "coverage", "below", "above", "infinite", "mean_width"]
_F32 = np.float32


# ============================================================================ the numpy restatement
def _h_f32(x):
    return np.ascontiguousarray(np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x).reshape(-1), _F32)


def _h_idx(x, what):
    x = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x).reshape(-1)
    if x.size and x.dtype.kind not in "iu":
        raise TypeError(f"{what}: expected integer indices, got {x.dtype}")
    return x.astype(np.int64)


def host_cells(patient, lab, n_labs: int, deg, edges):
    """-> (cell int64 [n], n_cells for a pair without one; kind int64 [n]: -1 a cell, 0 lab out of range, 1 patient out
    of range, 2 degree in no bin; row bin int64 [n], -1 none)."""
    e = np.asarray(edges, np.float64)
    nb = e.size - 1
    okl = (lab >= 0) & (lab < n_labs)
    okp = (patient >= 0) & (patient < deg.size)
    d = np.zeros(patient.shape, np.float64)
    if deg.size:
        d = deg[np.where(okp, patient, 0)].astype(np.float64)
    b = np.searchsorted(e, d, side="right") - 1                    # [e_j, e_j+1)
    okb = okp & (b >= 0) & (b < nb)
    kind = np.where(~okl, 0, np.where(~okp, 1, np.where(~okb, 2, -1))).astype(np.int64)
    cell = np.where(kind < 0, lab * nb + b, n_labs * nb).astype(np.int64)
    return cell, kind, np.where(okb, b, -1).astype(np.int64)


def host_seg_order_stats(keys, seg, n_seg: int, alpha: float, mode: str = "signed", min_count: int = 0):
    """mmg_seg_order_stats in numpy -> (count int32, q_lo, q_hi, shift fp32, usable int32), each [n_seg]."""
    keys, seg = np.asarray(keys, _F32), np.asarray(seg).astype(np.int64)
    ok = (seg >= 0) & (seg < n_seg) & ~np.isnan(keys)
    k, s = keys[ok], seg[ok]
    ks = k[np.lexsort((k, s))]
    count = np.bincount(s, minlength=n_seg).astype(np.int64)
    start = np.cumsum(count) - count
    m1 = (count + 1).astype(np.float64)
    half = alpha / 2
    k_hi = np.ceil(m1 * ((1.0 - half) if mode == "signed" else (1.0 - alpha))).astype(np.int64)
    has_hi = k_hi <= count
    q_hi = np.full(n_seg, np.inf, _F32)
    q_hi[has_hi] = ks[(start + k_hi - 1)[has_hi]]
    shift = np.zeros(n_seg, _F32)
    if mode == "signed":
        k_lo = np.floor(m1 * half).astype(np.int64)
        has_lo = k_lo >= 1
        q_lo = np.full(n_seg, -np.inf, _F32)
        q_lo[has_lo] = ks[(start + k_lo - 1)[has_lo]]
        odd, even = (count & 1) == 1, ((count & 1) == 0) & (count > 0)
        shift[odd] = ks[(start + (count >> 1))[odd]]
        with np.errstate(invalid="ignore", over="ignore"):
            shift[even] = (ks[(start + (count >> 1) - 1)[even]] + ks[(start + (count >> 1))[even]]) * _F32(0.5)
        usable = has_lo & has_hi
    else:
        q_lo = -q_hi
        usable = has_hi
    usable = usable & (count >= min_count)
    return count.astype(np.int32), q_lo, q_hi, shift, usable.astype(np.int32)


def host_fit(pred, target, patient, lab, n_labs: int, deg, edges, alpha: float, mode: str = "signed", min_count: int = 0):
    """mmg_cf_fit in numpy -> (table fp32 [3, n_cells], level int32 [n_cells], n_used int32 [n_cells], dropped int64 [4])."""
    nb = len(edges) - 1
    n_cells = n_labs * nb
    cell, kind, _ = host_cells(patient, lab, n_labs, deg, edges)
    with np.errstate(invalid="ignore", over="ignore"):
        r = target - pred                                          # fp32
    key = r if mode == "signed" else np.abs(r)
    kind = np.where((kind < 0) & np.isnan(key), 3, kind)
    dropped = np.bincount(kind[kind >= 0], minlength=4).astype(np.int64)
    valid = kind < 0
    seg = np.where(valid, cell, n_cells)
    lv = [host_seg_order_stats(key, seg, n_cells, alpha, mode, min_count),
          host_seg_order_stats(key, np.where(valid, seg // nb, n_labs), n_labs, alpha, mode, min_count),
          host_seg_order_stats(key, np.where(valid, 0, 1), 1, alpha, mode, min_count)]
    lab_of = np.arange(n_cells) // nb
    u0, u1, u2 = lv[0][4] != 0, lv[1][4][lab_of] != 0, np.full(n_cells, lv[2][4][0] != 0)
    level = np.where(u0, 0, np.where(u1, 1, np.where(u2, 2, 3))).astype(np.int32)
    none = [np.zeros(n_cells, np.int32), np.full(n_cells, -np.inf, _F32), np.full(n_cells, np.inf, _F32),
            np.zeros(n_cells, _F32)]
    cols = []
    for f in range(4):                                             # count, q_lo, q_hi, shift
        per = [lv[0][f], lv[1][f][lab_of], np.full(n_cells, lv[2][f][0]), none[f]]
        cols.append(np.choose(level, per))
    table = np.stack([cols[1], cols[2], cols[3]]).astype(_F32)
    return table, level, cols[0].astype(np.int32), dropped


def _host_rows(table, cell, n_cells):
    ok = cell < n_cells
    c = np.where(ok, cell, 0)
    if n_cells == 0:
        z = np.zeros(cell.shape, _F32)
        return z - np.inf, z + np.inf, z
    return (np.where(ok, table[0][c], _F32(-np.inf)).astype(_F32), np.where(ok, table[1][c], _F32(np.inf)).astype(_F32),
            np.where(ok, table[2][c], _F32(0)).astype(_F32))


def host_apply_pairs(pred, patient, lab, n_labs: int, deg, edges, table, use_shift: bool = False):
    """mmg_cf_apply_pairs in numpy -> (point, lower, upper) fp32 [n]."""
    cell, _, _ = host_cells(patient, lab, n_labs, deg, edges)
    ql, qh, sh = _host_rows(table, cell, table.shape[1])
    with np.errstate(invalid="ignore", over="ignore"):
        return ((pred + sh) if use_shift else pred.copy()), pred + ql, pred + qh


def host_apply_matrix(pred, rows, deg, edges, table, use_shift: bool = False):
    """mmg_cf_apply_matrix in numpy: pred fp32 [n_rows, n_labs] -> (point, lower, upper)."""
    n_rows, n_labs = pred.shape
    rows = np.arange(n_rows, dtype=np.int64) if rows is None else rows
    p = np.ascontiguousarray(pred, _F32).reshape(-1)
    out = host_apply_pairs(p, np.repeat(rows, n_labs), np.tile(np.arange(n_labs, dtype=np.int64), n_rows), n_labs, deg,
                           edges, table, use_shift)
    return tuple(o.reshape(n_rows, n_labs) for o in out)


def host_coverage(pred, target, patient, lab, n_labs: int, deg, edges, table):
    """mmg_cf_coverage in numpy -> (counts int64 [n_cells + 1, 6], width fp64 [n_cells + 1])."""
    n_cells = table.shape[1]
    cell, _, _ = host_cells(patient, lab, n_labs, deg, edges)
    ql, qh, _ = _host_rows(table, cell, n_cells)
    with np.errstate(invalid="ignore", over="ignore"):
        lower, upper = pred + ql, pred + qh
        has = cell < n_cells
        nan = np.isnan(pred) | np.isnan(target)
        live = has & ~nan
        fin = live & np.isfinite(lower) & np.isfinite(upper)
        w = np.where(fin, upper - lower, _F32(0)).astype(np.float64)
    fields = [live, live & (lower <= target) & (target <= upper), live & (target < lower), live & (target > upper),
              live & ~fin, ~live]
    counts = np.stack([np.bincount(cell[f], minlength=n_cells + 1) for f in fields], axis=1).astype(np.int64)
    width = np.bincount(cell[fin], weights=w[fin], minlength=n_cells + 1)
    return counts, width


# ============================================================================ the public object
def _t_idx(x, dev):
    x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x).reshape(-1)))
    x = x.detach().reshape(-1).to(dev)
    if x.dtype not in (torch.int64, torch.int32):
        if x.dtype.is_floating_point or x.dtype == torch.bool:
            raise TypeError(f"expected integer indices, got {x.dtype}")
        x = x.to(torch.int64)
    return x.contiguous()


def _t_f32(x, dev):
    x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x).reshape(-1)))
    return x.detach().reshape(-1).to(device=dev, dtype=torch.float32).contiguous()


class LabConformal:
    """Split-conformal intervals per (lab, patient lab-degree bin).  ``fit`` on a held-out split, then ``predict`` /
    ``predict_matrix`` give (point, lower, upper) and ``coverage`` scores them on another split.  HIP tensors run the
    kernels; numpy arrays run the numpy restatement of this module."""

    def __init__(self, alpha: float = 0.1, score: str = "signed", bins: Sequence = DEFAULT_BINS,
                 labels: Sequence[str] = DEFAULT_LABELS, min_count: int = 0, point: str = "prediction"):
        if not 0.0 < float(alpha) < 1.0:
            raise ValueError(f"alpha must lie in (0, 1), got {alpha}")
        if score not in SCORES:
            raise ValueError(f"score must be one of {SCORES}, got {score!r}")
        if point not in ("prediction", "median") or (point == "median" and score != "signed"):
            raise ValueError('point must be "prediction" or (with score="signed") "median"')
        if int(min_count) < 0:
            raise ValueError("min_count must not be negative")
        self.alpha, self.score, self.point, self.min_count = float(alpha), score, point, int(min_count)
        self.edges = _edges(bins, labels)
        self.labels = tuple(labels)
        self.n_labs: Optional[int] = None
        self._host = None            # (table, level, n_used, dropped) as numpy
        self._deg = None             # host degrees, int32
        self._dev = {}               # device -> (table, deg) tensors

    # ---- state
    @property
    def n_bins(self) -> int:
        return len(self.edges) - 1

    @property
    def fitted(self) -> bool:
        return self._host is not None

    def _need(self):
        if not self.fitted:
            raise RuntimeError("LabConformal: call fit() or load_state_dict() first")
        return self._host

    table = property(lambda self: self._need()[0])
    level = property(lambda self: self._need()[1])
    n_used = property(lambda self: self._need()[2])
    dropped = property(lambda self: self._need()[3])

    def _on(self, dev):
        if dev not in self._dev:
            self._dev[dev] = (torch.from_numpy(self.table).to(dev), torch.from_numpy(self._deg).to(dev))
        return self._dev[dev]

    def set_degrees(self, graph_or_degrees):
        """The patient degrees ``predict`` / ``coverage`` bin by (``fit`` keeps the ones it was given)."""
        self._deg = np.ascontiguousarray(np.asarray(patient_degrees(graph_or_degrees, None)), np.int32)
        self._dev = {}
        return self

    # ---- fit
    def fit(self, pred, target, lab_indices, patient_indices, graph_or_degrees, n_labs: Optional[int] = None):
        dev = pred.device if _is_dev(pred) else None
        if n_labs is None:
            try:
                n_labs = int(graph_or_degrees["lab"].num_nodes)
            except (TypeError, KeyError, IndexError, AttributeError, ValueError):
                li = lab_indices
                n_labs = (int(li.max()) + 1) if (li.numel() if torch.is_tensor(li) else np.size(li)) else 1
        self.n_labs = int(n_labs)
        if dev is not None:
            from . import conformal_ops as co
            deg = patient_degrees(graph_or_degrees, dev)
            p, t = _t_f32(pred, dev), _t_f32(target, dev)
            pi, li = _t_idx(patient_indices, dev), _t_idx(lab_indices, dev)
            if pi.dtype != li.dtype:
                pi, li = pi.to(torch.int64), li.to(torch.int64)
            table, level, n_used, dropped = co.cf_fit(p, t, pi, li, self.n_labs, deg, self.edges, self.alpha, self.score,
                                                      self.min_count)
            self._deg = deg.cpu().numpy().astype(np.int32)
            self._host = (table.cpu().numpy(), level.cpu().numpy(), n_used.cpu().numpy(), dropped.cpu().numpy())
            self._dev = {dev: (table, deg)}
        else:
            self.set_degrees(graph_or_degrees)
            self._host = host_fit(_h_f32(pred), _h_f32(target), _h_idx(patient_indices, "patient_indices"),
                                  _h_idx(lab_indices, "lab_indices"), self.n_labs, self._deg, self.edges, self.alpha,
                                  self.score, self.min_count)
        d = self.dropped
        if int(d.sum()):
            logging.info("  conformal fit: dropped pairs " + ", ".join(f"{k}={int(v)}" for k, v in zip(DROP_KINDS, d)))
        return self

    # ---- apply
    def predict(self, pred, lab_indices, patient_indices):
        """-> (point, lower, upper), fp32 [n]: tensors on the device of ``pred`` or numpy arrays."""
        self._need()
        shift = self.point == "median"
        if _is_dev(pred):
            from . import conformal_ops as co
            dev = pred.device
            table, deg = self._on(dev)
            pi, li = _t_idx(patient_indices, dev), _t_idx(lab_indices, dev)
            if pi.dtype != li.dtype:
                pi, li = pi.to(torch.int64), li.to(torch.int64)
            return co.cf_apply_pairs(_t_f32(pred, dev), pi, li, self.n_labs, deg, self.edges, table, shift)
        return host_apply_pairs(_h_f32(pred), _h_idx(patient_indices, "patient_indices"), _h_idx(lab_indices, "lab_indices"),
                                self.n_labs, self._deg, self.edges, self.table, shift)

    def predict_matrix(self, pred_matrix, patient_indices=None):
        """(point, lower, upper) [n_rows, n_labs] of a dense prediction matrix (a row of ``impute_lab_matrix`` per
        patient); ``patient_indices``: the patient of every row, None: row i is patient i."""
        self._need()
        shift = self.point == "median"
        if pred_matrix.ndim != 2 or int(pred_matrix.shape[1]) != self.n_labs:
            raise ValueError(f"predict_matrix: expected [n_rows, {self.n_labs}], got {tuple(pred_matrix.shape)}")
        if _is_dev(pred_matrix):
            from . import conformal_ops as co
            dev = pred_matrix.device
            table, deg = self._on(dev)
            x = pred_matrix.detach()
            if x.dtype != torch.float32 or (x.shape[1] > 1 and x.stride(1) != 1):
                x = x.float().contiguous()
            rows = None if patient_indices is None else _t_idx(patient_indices, dev)
            return co.cf_apply_matrix(x, rows, deg, self.edges, table, shift)
        x = pred_matrix.detach().cpu().numpy() if torch.is_tensor(pred_matrix) else np.asarray(pred_matrix)
        rows = None if patient_indices is None else _h_idx(patient_indices, "patient_indices")
        return host_apply_matrix(x.astype(_F32, copy=False), rows, self._deg, self.edges, self.table, shift)

    # ---- coverage
    def coverage_counts(self, pred, target, lab_indices, patient_indices):
        """Per cell (counts int64 [n_cells + 1, 6]: n, covered, below, above, infinite, dropped; width sums fp64
        [n_cells + 1]) as numpy; the last row holds, under dropped, the pairs without a cell."""
        self._need()
        if _is_dev(pred):
            from . import conformal_ops as co
            dev = pred.device
            table, deg = self._on(dev)
            pi, li = _t_idx(patient_indices, dev), _t_idx(lab_indices, dev)
            if pi.dtype != li.dtype:
                pi, li = pi.to(torch.int64), li.to(torch.int64)
            c, w = co.cf_coverage(_t_f32(pred, dev), _t_f32(target, dev), pi, li, self.n_labs, deg, self.edges, table)
            return c.cpu().numpy(), w.cpu().numpy()
        return host_coverage(_h_f32(pred), _h_f32(target), _h_idx(patient_indices, "patient_indices"),
                             _h_idx(lab_indices, "lab_indices"), self.n_labs, self._deg, self.edges, self.table)

    def coverage(self, pred, target, lab_indices, patient_indices, lab_names=None) -> pd.DataFrame:
        """One row overall, per lab and per degree bin: n, coverage = covered / n, the counts below / above / with an
        infinite bound, and the mean width of the finite intervals.  The cells are added in cell order."""
        counts, width = self.coverage_counts(pred, target, lab_indices, patient_indices)
        return coverage_frame(counts, width, self.n_labs, self.labels, lab_names)

    # ---- tables
    def table_frame(self, lab_names=None) -> pd.DataFrame:
        t, nb = self.table, self.n_bins
        cells = np.arange(self.n_labs * nb)
        return pd.DataFrame({
            "lab_idx": cells // nb,
            "lab_name": [_lab_name(lab_names, int(c // nb)) for c in cells],
            "degree_bin": [self.labels[int(c % nb)] for c in cells],
            "n_used": self.n_used.astype(np.int64),
            "level": [LEVELS[int(v)] for v in self.level],
            "q_lo": t[0], "q_hi": t[1], "shift": t[2]}, columns=TABLE_COLUMNS)

    def state_dict(self) -> dict:
        """The table, edges, alpha and score (tensors and plain values): an interval set ships with a checkpoint."""
        self._need()
        return {"alpha": self.alpha, "score": self.score, "point": self.point, "min_count": self.min_count,
                "edges": list(self.edges), "labels": list(self.labels), "n_labs": self.n_labs,
                "table": torch.from_numpy(self.table.copy()), "level": torch.from_numpy(self.level.copy()),
                "n_used": torch.from_numpy(self.n_used.copy()), "dropped": torch.from_numpy(self.dropped.copy()),
                "degrees": torch.from_numpy(self._deg.copy())}

    def load_state_dict(self, state: dict):
        self.__init__(state["alpha"], state["score"], state["edges"], state["labels"], state["min_count"], state["point"])
        self.n_labs = int(state["n_labs"])
        host = tuple(np.ascontiguousarray(state[k].cpu().numpy(), dt) for k, dt in
                     (("table", _F32), ("level", np.int32), ("n_used", np.int32), ("dropped", np.int64)))
        if host[0].shape != (3, self.n_labs * self.n_bins):
            raise ValueError(f"load_state_dict: table of shape {host[0].shape} for {self.n_labs} labs x {self.n_bins} bins")
        self._host = host
        self._deg = np.ascontiguousarray(state["degrees"].cpu().numpy(), np.int32)
        return self


def coverage_frame(counts, width, n_labs: int, labels, lab_names=None) -> pd.DataFrame:
    """The per-cell counts of ``coverage_counts`` -> rows (scope, key): overall, every lab, every degree bin."""
    nb = len(labels)
    c = np.asarray(counts)[:-1].reshape(n_labs, nb, len(COV_FIELDS))
    w = np.asarray(width)[:-1].reshape(n_labs, nb)

    def row(scope, key, cc, ww):
        tot, wsum = np.zeros(len(COV_FIELDS), np.int64), 0.0
        for x, y in zip(cc.reshape(-1, len(COV_FIELDS)), ww.reshape(-1)):        # cell order
            tot, wsum = tot + x, wsum + float(y)
        n, fin = int(tot[0]), int(tot[0] - tot[4])
        return {"scope": scope, "key": key, "n": n, "coverage": (tot[1] / n) if n else np.nan, "below": int(tot[2]),
                "above": int(tot[3]), "infinite": int(tot[4]), "mean_width": (wsum / fin) if fin else np.nan}

    rows = [row("overall", "all", c, w)]
    rows += [row("lab", _lab_name(lab_names, l), c[l], w[l]) for l in range(n_labs)]
    rows += [row("degree_bin", labels[b], c[:, b], w[:, b]) for b in range(nb)]
    return pd.DataFrame(rows, columns=COVERAGE_COLUMNS)


# ============================================================================ drivers
def _split_pairs(graph_dev, masker, split: str):
    mask = {"train": masker.train_mask, "val": masker.val_mask, "test": masker.test_mask}[split]
    ei = graph_dev[LAB_EDGE].edge_index
    mask = mask.to(ei.device)
    y = graph_dev[LAB_EDGE].edge_attr.reshape(-1)[mask].float().contiguous()
    return ei[0][mask].contiguous(), ei[1][mask].contiguous(), y


def _predict_split(model, graph, masker, split: str):
    if getattr(model, "_comm", None) is not None:
        raise NotImplementedError("conformal calibration on a patient-sharded model (dist.shard_model) is not supported: "
                                  "the forward's collectives need every rank; calibrate with an unsharded model")
    device = next(model.parameters()).device
    graph_dev = graph.to(device)
    pi, li, y = _split_pairs(graph_dev, masker, split)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            pred = model.predict_lab_values(graph_dev, pi, li).reshape(-1).float().contiguous()
    finally:
        model.train(was_training)
    return graph_dev, pred, y, pi, li


def fit_conformal(model, graph, masker, split: str = "val", **kw) -> LabConformal:
    """Predict the pairs of ``split`` (eval mode, ``predict_lab_values``) and fit a ``LabConformal(**kw)`` on them.  The
    degrees are the graph's has_lab degrees, as the model's own degree gate sees them."""
    graph_dev, pred, y, pi, li = _predict_split(model, graph, masker, split)
    return LabConformal(**kw).fit(pred, y, li, pi, graph_dev, n_labs=int(graph["lab"].num_nodes))


def conformal_report(model, graph, masker, alpha: float = 0.1, score: str = "signed", calibration: str = "val",
                     evaluation: str = "test", output_dir=None, lab_names=None, **kw):
    """Calibrate on one split, evaluate on another -> (LabConformal, table frame, coverage frame); with ``output_dir``
    writes ``conformal_table.csv`` and ``conformal_coverage.csv``."""
    cf = fit_conformal(model, graph, masker, calibration, alpha=alpha, score=score, **kw)
    graph_dev, pred, y, pi, li = _predict_split(model, graph, masker, evaluation)
    if lab_names is None:
        meta = graph["lab"].metadata if "metadata" in graph["lab"] else None
        if meta:
            lab_names = {idx: m["label"] for idx, m in meta.items()}
    table, cov = cf.table_frame(lab_names), cf.coverage(pred, y, li, pi, lab_names)
    if output_dir is not None:
        write_report(table, cov, output_dir)
    return cf, table, cov


def write_report(table: pd.DataFrame, cov: pd.DataFrame, output_dir):
    out = Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    table.to_csv(out / "conformal_table.csv", index=False)
    cov.to_csv(out / "conformal_coverage.csv", index=False)
    logging.info(f"  Saved conformal tables to {out}")


def impute_intervals(model, data, conformal: LabConformal, patient_indices: Optional[torch.Tensor] = None):
    """(point, lower, upper, observed), each [n, L], from ONE ``impute_lab_matrix`` forward: the dense predictions of the
    requested patients (all when None) with their intervals, and which cells are observed has_lab edges."""
    from .inference import impute_missing
    was_training = model.training
    model.eval()                                             # impute_lab_matrix is inference-only
    try:
        pred, observed = impute_missing(model, data, patient_indices)
    finally:
        model.train(was_training)
    point, lower, upper = conformal.predict_matrix(pred, patient_indices)
    return point, lower, upper, observed
