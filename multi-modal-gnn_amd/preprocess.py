"""Lab-event preprocessing on the device: the lab half of the reference's ``src/preprocess.py`` (:28-164) and the two
helpers of ``src/utils.py`` it rests on (:309-481), with the reference's names, arguments, result columns and edge
cases.  The arithmetic runs in the kernels of ``csrc/prep.hip`` (fp64 throughout; there is no CPU fallback):

* ``preprocess_lab_events``  the tensor-level entry: cohort filter, outlier removal, aggregation and normalisation of
  device tensors of event codes; one stable radix sort of the events, per-lab statistics in a fixed order, one
  segment pass, one element-wise pass.
* ``aggregate_lab_values`` / ``normalize_lab_values``  the reference's frame functions: the key columns are factorised
  with sorted uniques on the host, four columns go to the device, and the frames that come back are what
  ``graph_build.build_heterogeneous_graph`` consumes.
* ``remove_outliers`` and ``LabNormalizer``  on a pandas Series, a numpy array or a device tensor (the same kind comes
  back).  Beyond the reference the normaliser offers ``to_lab_stats()`` (the ``ITEMID, mean, std`` frame
  ``inference.lab_report`` reads) and ``inverse_transform_matrix`` (a whole ``impute_lab_matrix`` result).

Feature-space selection -- which labs, diagnoses and drugs become nodes (``src/io_mimic.py`` filter_labs_for_cohort,
``src/preprocess.py`` process_diagnoses / process_medications / the frame part of preprocess_pipeline).  The counting,
ranking and row selection run in ``csrc/select.hip``:

* ``select_codes``  the tensor-level entry over device tensors of event codes.
* ``filter_labs_for_cohort`` / ``process_diagnoses`` / ``process_medications`` / ``normalize_drug_name``  the
  reference's frame functions.  String work (strip, 3-character collapse, the drug-name rules) runs on the host over
  the UNIQUE values only; the row-sized arrays that go to the device are integer codes.
* ``preprocess_frames``  raw frames -> the frames ``graph_build.build_heterogeneous_graph`` consumes.

Ties.  The reference ranks labs with ``nlargest(keep="first")`` over a sorted index: among equal patient counts the
smaller ITEMID wins, and so it does here.  It ranks diagnoses and drugs with ``value_counts().head(top_k)``, whose order
among equal counts is whatever pandas' unstable sort yields; this module's rule is its own: among equal counts the
smaller code (in sorted key order) wins.  The results differ from the reference's only for a tie exactly at the cut.
"""
from __future__ import annotations

import logging
import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import pandas as pd
import torch

INT64_MAX = np.iinfo(np.int64).max
AGGREGATIONS = ("last", "mean", "median", "min", "max")
NORMALIZATIONS = ("zscore", "minmax", "robust")
OUTLIER_METHODS = ("std", "iqr")


def _ops():
    from . import ops
    return ops


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _to_device_f64(values) -> torch.Tensor:
    if torch.is_tensor(values):
        return values.reshape(-1).to(torch.float64).contiguous()
    arr = values.to_numpy(dtype=np.float64) if isinstance(values, pd.Series) else np.asarray(values, dtype=np.float64)
    return torch.from_numpy(np.ascontiguousarray(arr.reshape(-1))).to(_device())


def _like(values, result: torch.Tensor):
    """The result in the caller's container: Series (its index and name), ndarray, or the device tensor itself."""
    if torch.is_tensor(values):
        return result
    arr = result.cpu().numpy()
    if isinstance(values, pd.Series):
        return pd.Series(arr, index=values.index, name=values.name)
    return arr.reshape(np.shape(values))


def _one_lab_table(v: torch.Tensor, quantiles: bool) -> torch.Tensor:
    """[1, 9] table of one lab's values."""
    ops = _ops()
    lab = torch.zeros(v.numel(), dtype=torch.int64, device=v.device)
    if not quantiles:
        return ops.lab_stats(lab, v, 1, 1)
    _, group, vs = ops.prep_sort(lab, None, v, 1, 1, value=v)
    return ops.lab_quantiles(group, vs, 1, 1, ops.lab_stats(group, vs, 1, 1))


def remove_outliers(values, method: str = "std", threshold: float = 5.0):
    """utils.py:435-481: the values with outliers set to NaN.  "std": outside mean +- threshold * std (NaN-skipping,
    ddof 1); "iqr": outside q25 - threshold * iqr, q75 + threshold * iqr (linear quantiles)."""
    if method not in OUTLIER_METHODS:
        raise ValueError(f"Unknown outlier detection method: {method}")
    v = _to_device_f64(values)
    table = _one_lab_table(v, method == "iqr")
    return _like(values, _ops().lab_outlier_mask(v, None, table, method, threshold))


def _stats_entry(method: str, row: np.ndarray) -> Optional[Dict]:
    ops = _ops()
    if not row[ops.LS_N] > 0:
        return None
    if method == "zscore":
        return {"mean": np.float64(row[ops.LS_MEAN]), "std": np.float64(row[ops.LS_STD])}
    if method == "minmax":
        return {"min": np.float64(row[ops.LS_MIN]), "max": np.float64(row[ops.LS_MAX])}
    return {"median": np.float64(row[ops.LS_MEDIAN]), "q25": np.float64(row[ops.LS_Q25]),
            "q75": np.float64(row[ops.LS_Q75])}


def _table_row(method: str, entry: Optional[Dict]) -> np.ndarray:
    ops = _ops()
    row = np.full(ops.LAB_STAT_FIELDS, np.nan)
    row[ops.LS_N] = row[ops.LS_ROWS] = 0.0
    if entry is not None:
        row[ops.LS_N] = row[ops.LS_ROWS] = 1.0
        for k, f in (("mean", ops.LS_MEAN), ("std", ops.LS_STD), ("min", ops.LS_MIN), ("max", ops.LS_MAX),
                     ("median", ops.LS_MEDIAN), ("q25", ops.LS_Q25), ("q75", ops.LS_Q75)):
            if k in entry:
                row[f] = entry[k]
    return row


class LabNormalizer:
    """utils.py:309-432.  ``stats[lab_id]`` holds the reference's entries ({'mean', 'std'}, {'min', 'max'} or
    {'median', 'q25', 'q75'}; None for a lab without a valid value)."""

    def __init__(self, method: str = "zscore"):
        self.method = method
        self.stats: Dict[str, Optional[Dict]] = {}
        self.lab_ids: List[str] = []          # column order of inverse_transform_matrix (filled by the bulk paths)

    def _check(self):
        if self.method not in NORMALIZATIONS:
            raise ValueError(f"Unknown normalization method: {self.method}")

    @classmethod
    def from_table(cls, method: str, table: np.ndarray, lab_ids: Sequence) -> "LabNormalizer":
        """From a host copy of the [n_labs, 9] device table: one entry per lab that has a row."""
        ops = _ops()
        nz = cls(method)
        nz._check()
        nz.lab_ids = [str(i) for i in lab_ids]
        for row, key in zip(table, nz.lab_ids):
            if row[ops.LS_ROWS] > 0:
                nz.stats[key] = _stats_entry(method, row)
                if nz.stats[key] is None:
                    logging.warning(f"No valid values for lab {key}")
        return nz

    def _table(self, keys: Sequence[str], device) -> torch.Tensor:
        rows = np.stack([_table_row(self.method, self.stats.get(k)) for k in keys])
        return torch.from_numpy(rows).to(device)

    def fit(self, values, lab_id: str) -> None:
        v = _to_device_f64(values)
        row = _one_lab_table(v, self.method == "robust").cpu().numpy()[0]
        if not row[_ops().LS_N] > 0:
            logging.warning(f"No valid values for lab {lab_id}")
            self.stats[lab_id] = None
            return
        self._check()
        self.stats[lab_id] = _stats_entry(self.method, row)

    def transform(self, values, lab_id: str):
        if lab_id not in self.stats or self.stats[lab_id] is None:
            logging.warning(f"No statistics available for lab {lab_id}, returning original values")
            return values
        self._check()
        v = _to_device_f64(values)
        return _like(values, _ops().lab_normalize(v, None, self._table([lab_id], v.device), self.method))

    def fit_transform(self, values, lab_id: str):
        self.fit(values, lab_id)
        return self.transform(values, lab_id)

    def inverse_transform(self, normalized_values, lab_id: str):
        """Back to the lab's own scale.  As in the reference a zero spread is not special-cased.  An fp32 tensor comes
        back as fp32 (formed in fp64, rounded once: what inverse_transform_matrix gives for that column)."""
        if lab_id not in self.stats or self.stats[lab_id] is None:
            return normalized_values
        self._check()
        v = _to_device_f64(normalized_values)
        out = _ops().lab_inverse(v, None, self._table([lab_id], v.device), self.method)
        if torch.is_tensor(normalized_values) and normalized_values.dtype == torch.float32:
            out = out.to(torch.float32)
        return _like(normalized_values, out.reshape(normalized_values.shape) if torch.is_tensor(normalized_values) else out)

    def inverse_transform_matrix(self, pred: torch.Tensor, lab_ids: Optional[Sequence] = None) -> torch.Tensor:
        """The inverse of a dense fp32 [n_rows, n_labs] device matrix (``impute_lab_matrix``'s result); column c is the
        lab ``lab_ids[c]`` (default: the labs this normaliser was fitted on, in key order)."""
        self._check()
        keys = [str(i) for i in lab_ids] if lab_ids is not None else (self.lab_ids or list(self.stats))
        if pred.dim() != 2 or pred.shape[1] != len(keys):
            raise ValueError(f"inverse_transform_matrix: pred must be [n_rows, {len(keys)}], got {tuple(pred.shape)}")
        return _ops().lab_inverse_matrix(pred, self._table(keys, pred.device), self.method)

    def to_lab_stats(self) -> pd.DataFrame:
        """The ``ITEMID, mean, std`` frame ``inference.lab_report`` denormalises with (value * std + mean): the location
        and spread of this method's inverse, so the report is right for every method.  A lab without statistics
        passes through (0, 1)."""
        self._check()
        rows = []
        for key in (self.lab_ids or list(self.stats)):
            e = self.stats.get(key)
            if e is None:
                loc, spread = 0.0, 1.0
            elif self.method == "zscore":
                loc, spread = e["mean"], e["std"]
            elif self.method == "minmax":
                loc, spread = e["min"], e["max"] - e["min"]
            else:
                loc, spread = e["median"], e["q75"] - e["q25"]
            rows.append((key, float(loc), float(spread)))
        return pd.DataFrame(rows, columns=["ITEMID", "mean", "std"])


# ============================================================================ tensor level
def aggregate_lab_events(patient: torch.Tensor, lab: torch.Tensor, value: torch.Tensor, time: Optional[torch.Tensor],
                         n_patients: int, n_labs: int, aggregate: str = "last",
                         outlier_threshold: Optional[float] = 5.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Cohort filter, outlier removal ("std", per lab over all its events) and aggregation of device event tensors
    -> (patient, lab, value) of the pairs in (lab, patient) order.  See preprocess_lab_events for the inputs."""
    if aggregate not in AGGREGATIONS:
        raise ValueError(f"Unknown aggregation method: {aggregate}")
    ops = _ops()
    if aggregate == "last":
        if time is None:
            raise ValueError('aggregate="last" needs the event times')
        secondary = time
    else:
        secondary = value if aggregate == "median" else None
    _, group, vs = ops.prep_sort(lab, patient, secondary, n_patients, n_labs, value=value)
    stats = ops.lab_stats(group, vs, n_patients, n_labs) if outlier_threshold is not None else None
    return ops.lab_aggregate(group, vs, n_patients, n_labs, aggregate, "std" if stats is not None else None,
                             outlier_threshold if stats is not None else 0.0, stats)


def fit_lab_table(lab_sorted: torch.Tensor, value: torch.Tensor, n_labs: int, normalize: str) -> torch.Tensor:
    """The [n_labs, 9] table of values whose lab codes are non-decreasing (the quantiles only for "robust")."""
    ops = _ops()
    stats = ops.lab_stats(lab_sorted, value, 1, n_labs)
    if normalize == "robust":
        _, g2, v2 = ops.prep_sort(lab_sorted, None, value, 1, n_labs, value=value)
        ops.lab_quantiles(g2, v2, 1, n_labs, stats)
    return stats


def preprocess_lab_events(patient: torch.Tensor, lab: torch.Tensor, value: torch.Tensor, time: Optional[torch.Tensor],
                          n_patients: int, n_labs: int, aggregate: str = "last",
                          outlier_threshold: Optional[float] = 5.0, normalize: str = "zscore"):
    """Raw lab events -> normalised (patient, lab) pairs, all on the device.

    patient, lab: int64 codes (code order = key order; a code outside [0, n_patients) / [0, n_labs) drops the event);
    value: fp64; time: int64, INT64_MAX for a missing time (needed for "last" only).  outlier_threshold None: no
    outlier removal (then a pair whose chosen value is NaN is dropped by the normaliser instead).
    -> (patient, lab, value, value_normalized, LabNormalizer), rows in (lab, patient) order, the normaliser's stats keyed
    by str(lab code)."""
    if normalize not in NORMALIZATIONS:
        raise ValueError(f"Unknown normalization method: {normalize}")
    ops = _ops()
    p, l, v = aggregate_lab_events(patient, lab, value, time, n_patients, n_labs, aggregate, outlier_threshold)
    table = fit_lab_table(l, v, n_labs, normalize)
    vn = ops.lab_normalize(v, l, table, normalize)
    keep = ~torch.isnan(vn)                                   # "Drop any remaining NaN" (preprocess.py:150)
    normalizer = LabNormalizer.from_table(normalize, table.cpu().numpy(), range(n_labs))
    return p[keep], l[keep], v[keep], vn[keep], normalizer


# ============================================================================ frame level
def _time_codes(col: pd.Series) -> np.ndarray:
    """CHARTTIME as int64 with INT64_MAX for a missing time: datetime64 (MIMIC) or numeric offsets (eICU)."""
    if pd.api.types.is_datetime64_any_dtype(col):
        t = col.to_numpy(dtype="datetime64[ns]").view(np.int64).copy()
        t[col.isna().to_numpy()] = INT64_MAX
        return t
    arr = col.to_numpy()
    if arr.dtype.kind == "f":
        miss = np.isnan(arr)
        t = np.where(miss, 0, arr).astype(np.int64)
        t[miss] = INT64_MAX
        return t
    if arr.dtype.kind in "iu":
        return arr.astype(np.int64)
    raise TypeError(f"CHARTTIME: expected datetime64 or numeric offsets, got {arr.dtype}")


def _factorize_sorted(col: pd.Series):
    codes, uniques = pd.factorize(col, sort=True)
    return codes.astype(np.int64), np.asarray(uniques)


def aggregate_lab_values(labs: pd.DataFrame, cohort: pd.DataFrame, method: str = "last",
                         remove_outliers_flag: bool = True, outlier_threshold: float = 5.0) -> pd.DataFrame:
    """preprocess.py:28-110: events (SUBJECT_ID, ITEMID, VALUENUM, CHARTTIME) of the cohort's patients -> one VALUE per
    (SUBJECT_ID, ITEMID), rows sorted by (SUBJECT_ID, ITEMID) as the reference's groupby leaves them (fresh index)."""
    logging.info(f"Aggregating lab values using method: {method}")
    if method not in AGGREGATIONS:
        raise ValueError(f"Unknown aggregation method: {method}")
    cohort_ids = np.unique(cohort["SUBJECT_ID"].to_numpy())
    sid = labs["SUBJECT_ID"].to_numpy()
    pos = np.searchsorted(cohort_ids, sid)
    pos_c = np.minimum(pos, max(len(cohort_ids) - 1, 0))
    pcode = np.where(cohort_ids[pos_c] == sid, pos_c, -1).astype(np.int64) if len(cohort_ids) else np.full(len(sid), -1, np.int64)
    lcode, lab_keys = _factorize_sorted(labs["ITEMID"])
    n_labs = max(len(lab_keys), 1)
    dev = _device()
    time = torch.from_numpy(_time_codes(labs["CHARTTIME"])).to(dev) if method == "last" else None
    value = torch.from_numpy(np.ascontiguousarray(labs["VALUENUM"].to_numpy(dtype=np.float64))).to(dev)
    p, l, v = aggregate_lab_events(torch.from_numpy(pcode).to(dev), torch.from_numpy(lcode).to(dev), value, time,
                                   max(len(cohort_ids), 1), n_labs, method,
                                   outlier_threshold if remove_outliers_flag else None)
    p, l, v = p.cpu().numpy(), l.cpu().numpy(), v.cpu().numpy()
    order = np.argsort(p, kind="stable")                      # (lab, patient) -> the reference's (patient, lab) order
    labs_agg = pd.DataFrame({"SUBJECT_ID": cohort_ids[p[order]] if len(p) else np.empty(0, cohort_ids.dtype),
                             "ITEMID": lab_keys[l[order]] if len(l) else lab_keys[:0], "VALUE": v[order]})
    logging.info(f"Aggregated to {len(labs_agg)} patient-lab pairs")
    return labs_agg


def normalize_lab_values(labs_agg: pd.DataFrame, method: str = "zscore") -> Tuple[pd.DataFrame, LabNormalizer]:
    """preprocess.py:113-164: VALUE_NORMALIZED per lab, rows in lab-key order (input order inside a lab), NaN rows
    dropped, SUBJECT_ID int64, ITEMID int64 where it converts."""
    logging.info(f"Normalizing lab values using method: {method}")
    if method not in NORMALIZATIONS:
        raise ValueError(f"Unknown normalization method: {method}")
    ops = _ops()
    lcode, lab_keys = _factorize_sorted(labs_agg["ITEMID"])
    n_labs = max(len(lab_keys), 1)
    dev = _device()
    lab = torch.from_numpy(lcode).to(dev)
    value = torch.from_numpy(np.ascontiguousarray(labs_agg["VALUE"].to_numpy(dtype=np.float64))).to(dev)
    perm, l_sorted, v_sorted = ops.prep_sort(lab, None, None, 1, n_labs, value=value)      # stable: groupby + concat
    table = fit_lab_table(l_sorted, v_sorted, n_labs, method)
    vn = ops.lab_normalize(v_sorted, l_sorted, table, method)
    normalizer = LabNormalizer.from_table(method, table.cpu().numpy(), lab_keys)
    n_keyed = int((lcode >= 0).sum())                         # rows without an ITEMID sort last and leave, as in groupby
    perm, vn = perm.cpu().numpy()[:n_keyed], vn.cpu().numpy()[:n_keyed]
    out = labs_agg.iloc[perm].reset_index(drop=True)
    out["VALUE_NORMALIZED"] = vn
    out = out[out["VALUE_NORMALIZED"].notna()].copy()
    out["SUBJECT_ID"] = out["SUBJECT_ID"].astype("int64")
    try:
        out["ITEMID"] = out["ITEMID"].astype("int64")
    except (ValueError, TypeError):
        pass                                                   # string ids (eICU lab names) stay
    logging.info(f"Normalized {len(out)} lab values")
    return out, normalizer


# ============================================================================ feature-space selection
def select_codes(patient: torch.Tensor, code: torch.Tensor, n_patients: int, n_codes: int, *,
                 valid: Optional[torch.Tensor] = None, min_patient_count: int, top_k: Optional[int] = None,
                 rows: str = "all"):
    """Which codes become nodes and which event rows stay, all on the device.

    patient, code: int64 codes over the event rows (code order = key order; a value outside [0, n_patients) /
    [0, n_codes) drops the row); valid: uint8 / bool, 0 drops the row.  A code is eligible with at least one row and at
    least min_patient_count distinct patients; the eligible codes are ranked by (patients descending, code ascending)
    and the first top_k (None: all) are selected.  rows="all" keeps every counted row of a selected code, "first" the
    first row of each (patient, code) pair.  n_codes is not limited to ops.PREP_MAX_LABS.
    -> (n_patients_per_code int64, n_rows_per_code int64, rank int32 (-1: not eligible), selected uint8, out_rows int32
    ascending)."""
    return _ops().code_select(code, patient, n_patients, n_codes, min_patient_count, top_k, rows, valid)


def _member_codes(col: pd.Series, members) -> Tuple[np.ndarray, np.ndarray]:
    """(position of every value among the sorted unique members, -1 outside; the sorted unique members)."""
    keys = np.unique(np.asarray(pd.Series(members).dropna()))
    v = col.to_numpy()
    if len(keys) == 0 or len(v) == 0:
        return np.full(len(v), -1, np.int64), keys
    try:
        pos = np.searchsorted(keys, v)
        pos_c = np.minimum(pos, len(keys) - 1)
        return np.where(keys[pos_c] == v, pos_c, -1).astype(np.int64), keys
    except TypeError:                                         # ids that do not order against the members: a lookup
        return pd.Index(keys).get_indexer(v).astype(np.int64), keys


def _string_codes(col: pd.Series, rule) -> Tuple[np.ndarray, np.ndarray]:
    """Row codes of rule(str(value).strip()) with sorted unique keys; '' (before or after the rule) gives -1.  The
    strings are formed over the unique values only; a missing value becomes the text pandas' astype(str) gives it
    ('nan', 'None'), as in the reference."""
    c0, u0 = pd.factorize(col)                                # missing -> -1
    texts = pd.Series(u0).astype(str).tolist() if len(u0) else []
    miss = c0 < 0
    if miss.any():
        cm, um = pd.factorize(col[miss].astype(str))
        c0 = c0.copy()
        c0[miss] = len(texts) + cm
        texts += list(um)
    mapped = []
    for t in texts:
        t = t.strip()
        mapped.append(rule(t) if t != "" else "")
    keys = np.array(sorted(set(mapped) - {""}), dtype=object)            # code order = sorted key order
    at = {k: i for i, k in enumerate(keys)}
    of_unique = np.array([at.get(t, -1) for t in mapped], dtype=np.int64)
    return (of_unique[c0] if len(c0) else np.empty(0, np.int64)), keys


def _run_selection(pcode, ccode, valid, n_patients, n_codes, min_patient_count, top_k, rows):
    if top_k is not None and top_k < 0:                       # head(-k) / nlargest(-k) are not a selection rule
        raise ValueError(f"top_k must be None or >= 0, got {top_k}")
    dev = _device()
    out = select_codes(torch.from_numpy(np.ascontiguousarray(pcode)).to(dev),
                       torch.from_numpy(np.ascontiguousarray(ccode)).to(dev), max(int(n_patients), 1),
                       max(int(n_codes), 1),
                       valid=None if valid is None else torch.from_numpy(np.ascontiguousarray(valid, dtype=np.uint8)).to(dev),
                       min_patient_count=int(min_patient_count), top_k=top_k, rows=rows)
    return [t.cpu().numpy() for t in out]


def filter_labs_for_cohort(labevents: pd.DataFrame, cohort: pd.DataFrame, d_labitems: pd.DataFrame,
                           top_k: Optional[int] = None, min_patient_count: int = 10) -> Tuple[pd.DataFrame, pd.DataFrame]:
    """io_mimic.py:442-516: the events of the cohort's patients with a numeric VALUENUM, restricted to the labs that at
    least min_patient_count patients have and, of those, the top_k by NUM_PATIENTS (a tie at the cut goes to the
    smaller ITEMID, integer or string).  -> (labs: the surviving rows in input order with their index,
    selected_labitems: d_labitems' rows of the selected ids with NUM_PATIENTS and NUM_MEASUREMENTS merged on)."""
    logging.info("Filtering lab events for cohort...")
    pcode, cohort_ids = _member_codes(labevents["SUBJECT_ID"], cohort["SUBJECT_ID"])
    lcode, lab_keys = _factorize_sorted(labevents["ITEMID"])
    valid = labevents["VALUENUM"].notna().to_numpy()
    n_pat, n_rows, rank, selected, rows = _run_selection(pcode, lcode, valid, len(cohort_ids), len(lab_keys),
                                                        min_patient_count, top_k, "all")
    sel = np.flatnonzero(selected[:len(lab_keys)])
    if top_k is not None:
        sel = sel[np.argsort(rank[sel], kind="stable")]       # nlargest's order; without a cut the groupby's key order
    lab_counts = pd.DataFrame({"NUM_PATIENTS": n_pat[sel], "NUM_MEASUREMENTS": n_rows[sel]},
                              index=pd.Index(lab_keys[sel], name="ITEMID"))
    logging.info(f"Selected {len(lab_counts)} lab tests")
    labs = labevents.iloc[rows]
    logging.info(f"Final lab events: {len(labs)}")
    selected_labitems = d_labitems[d_labitems["ITEMID"].isin(set(lab_counts.index))].copy()
    selected_labitems = selected_labitems.merge(lab_counts, left_on="ITEMID", right_index=True)
    return labs, selected_labitems


def _select_pairs(frame: pd.DataFrame, cohort: pd.DataFrame, source_col: str, rule, min_patient_count, top_k):
    """The shared part of process_diagnoses / process_medications -> (kept row positions, their code strings, the
    selected keys by rank with their patient counts)."""
    pcode, cohort_ids = _member_codes(frame["SUBJECT_ID"], cohort["SUBJECT_ID"])
    in_adm = frame["HADM_ID"].isin(set(cohort["HADM_ID"])).to_numpy()
    ccode, keys = _string_codes(frame[source_col], rule)
    n_pat, _, rank, selected, rows = _run_selection(pcode, ccode, in_adm, len(cohort_ids), len(keys),
                                                    min_patient_count, top_k, "first")
    sel = np.flatnonzero(selected[:len(keys)])
    sel = sel[np.argsort(rank[sel], kind="stable")]
    counts = pd.Series(n_pat[sel], index=pd.Index(keys[sel], dtype=object), name="count")
    return rows, (keys[ccode[rows]] if len(rows) else np.empty(0, object)), counts


def process_diagnoses(diagnoses: pd.DataFrame, cohort: pd.DataFrame, collapse_to_3digit: bool = True,
                      top_k: Optional[int] = None, min_patient_count: int = 5) -> pd.DataFrame:
    """preprocess.py:171-266.  A row counts if its HADM_ID is one of the cohort's AND its SUBJECT_ID is; the code is
    str(ICD9_CODE).strip() ('' dropped; a missing code is the code 'nan' / 'None', as in the reference), cut to its first
    three characters with collapse_to_3digit.  Kept: the diagnoses of at least min_patient_count patients, the top_k
    most frequent of them -- among equal counts the smaller code (sorted key order) wins, this project's own rule where
    the reference's value_counts() leaves the order of ties to an unstable sort.
    -> the first row of each (patient, code) pair of a kept code, in input order with the original index: SUBJECT_ID,
    ICD3_CODE (collapsed) or ICD9_CODE (not collapsed; then there is no ICD3_CODE column), and DIAGNOSIS_CATEGORY /
    DIAGNOSIS_SUBCATEGORY / DIAGNOSIS_PRIORITY of that first row when present."""
    logging.info("Processing diagnosis codes...")
    col = "ICD3_CODE" if collapse_to_3digit else "ICD9_CODE"
    rule = (lambda t: t[:3]) if collapse_to_3digit else (lambda t: t)
    rows, codes, counts = _select_pairs(diagnoses, cohort, "ICD9_CODE", rule, min_patient_count, top_k)
    logging.info(f"Selected {len(counts)} diagnoses")
    kept = diagnoses.iloc[rows]
    out = pd.DataFrame({"SUBJECT_ID": kept["SUBJECT_ID"], col: pd.Series(codes, index=kept.index, dtype=object)})
    for extra in ("DIAGNOSIS_CATEGORY", "DIAGNOSIS_SUBCATEGORY", "DIAGNOSIS_PRIORITY"):
        if extra in diagnoses.columns:
            out[extra] = kept[extra]
    logging.info(f"Final: {len(out)} patient-diagnosis pairs")
    return out


_DOSAGE = re.compile(r"\d+\.?\d*\s*(mg|mcg|ml|g|%|units?)")
_FORM_WORDS = re.compile(r"\b(tablet|capsule|injection|solution|suspension|syrup|cream|ointment)\b")
_ROUTE_WORDS = re.compile(r"\b(oral|topical|iv|intravenous|subcutaneous)\b")
_PUNCTUATION = re.compile(r"[^\w\s]")


def normalize_drug_name(drug) -> str:
    """preprocess.py:273-312: lower case, dosage patterns ("50mg", "10 ml", "5 %", "3 units"), form words and route
    words removed, punctuation to spaces, the first remaining word ("" for a missing name; a name with no word left
    comes back as what is left, the empty string)."""
    if pd.isna(drug):
        return ""
    text = str(drug).lower()
    for pattern in (_DOSAGE, _FORM_WORDS, _ROUTE_WORDS):
        text = pattern.sub("", text)
    words = _PUNCTUATION.sub(" ", text).split()
    return words[0] if words else ""


def process_medications(prescriptions: pd.DataFrame, cohort: pd.DataFrame, normalize_names: bool = True,
                        top_k: Optional[int] = None, min_patient_count: int = 5) -> pd.DataFrame:
    """preprocess.py:315-412.  The cohort rule of process_diagnoses; the name is str(DRUG).strip() ('' dropped), with
    normalize_names passed through normalize_drug_name (empty results dropped).  Kept: the drugs of at least
    min_patient_count patients, the top_k most frequent of them, among equal counts the smaller name (sorted key order)
    -- this project's own rule, see process_diagnoses.
    -> the first row of each (patient, drug) pair of a kept drug, in input order with the original index: SUBJECT_ID,
    DRUG, and ROUTE / FREQUENCY / PRN / IV_ADMIXTURE of that first row when present."""
    logging.info("Processing medications...")
    rule = normalize_drug_name if normalize_names else (lambda t: t)
    rows, names, counts = _select_pairs(prescriptions, cohort, "DRUG", rule, min_patient_count, top_k)
    logging.info(f"Selected {len(counts)} medications")
    kept = prescriptions.iloc[rows]
    out = pd.DataFrame({"SUBJECT_ID": kept["SUBJECT_ID"], "DRUG": pd.Series(names, index=kept.index, dtype=object)})
    for extra in ("ROUTE", "FREQUENCY", "PRN", "IV_ADMIXTURE"):
        if extra in prescriptions.columns:
            out[extra] = kept[extra]
    logging.info(f"Final: {len(out)} patient-medication pairs")
    return out


def preprocess_frames(labevents: pd.DataFrame, d_labitems: pd.DataFrame, diagnoses: pd.DataFrame,
                      prescriptions: pd.DataFrame, cohort: pd.DataFrame, config: Dict) -> Dict:
    """The frame part of preprocess_pipeline (preprocess.py:553-673), from raw frames to what
    graph_build.build_heterogeneous_graph consumes; the arguments come from config["feature_space"] as the reference
    reads them.  -> {"labitems", "labs" (normalised), "lab_normalizer", "diagnoses", "medications"}.  The loaders, the
    parquet files, the demographic features and the APACHE scores are not part of it."""
    fs = config["feature_space"]
    labs_filtered, selected_labitems = filter_labs_for_cohort(
        labevents, cohort, d_labitems, top_k=fs["labs"]["top_k"], min_patient_count=fs["labs"].get("min_patient_count", 10))
    labs_agg = aggregate_lab_values(labs_filtered, cohort, method=fs["labs"]["aggregate"],
                                    remove_outliers_flag=fs["labs"].get("outlier_std_threshold") is not None,
                                    outlier_threshold=fs["labs"].get("outlier_std_threshold", 5.0))
    labs_normalized, normalizer = normalize_lab_values(labs_agg, method=fs["labs"]["normalize"])
    dx = process_diagnoses(diagnoses, cohort, collapse_to_3digit=fs["diagnoses"]["collapse_to_3digit"],
                           top_k=fs["diagnoses"]["top_k"], min_patient_count=fs["diagnoses"].get("min_patient_count", 5))
    meds = process_medications(prescriptions, cohort, normalize_names=fs["medications"]["normalize_names"],
                               top_k=fs["medications"]["top_k"],
                               min_patient_count=fs["medications"].get("min_patient_count", 5))
    return {"labitems": selected_labitems, "labs": labs_normalized, "lab_normalizer": normalizer, "diagnoses": dx,
            "medications": meds}
