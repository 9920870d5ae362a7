"""Lab imputation reports (reference ``src/inference.py:53-178``, ``predict_for_patient``).

The reference answers "what are this patient's labs" with two whole-graph forwards per patient: ``predict_lab_values``
over the labs the patient has, then again over the ones never measured.  Here one ``HeteroRGCN.impute_lab_matrix``
forward gives every lab of every requested patient (bit for bit the pair path's predictions), and the report of each
patient is assembled on the host from its row of that matrix:

  impute_missing        the dense matrix and which of its cells are observed ``has_lab`` edges
  predict_for_patient   the reference's signature and result dict (measured / masked / truly missing labs)
  predict_for_patients  the same dicts for many patients from one forward
  lab_report            the host-side assembly of one patient's dict (no device, no model)

With ``intervals=`` (a fitted ``conformal.LabConformal``) every predicted entry also carries its split-conformal
interval; without it the dicts are the reference's.  With ``stacker=`` (a fitted ``stacking.LabStacker``) every
predicted entry carries the stacked value and keeps the model's own under ``raw_prediction``.

Printing, config loading and the command line of the reference script (``print_patient_report``, ``run_inference``)
are not part of this module.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .data import LAB_EDGE, ROW_TYPE


def impute_missing(model, data, patient_indices: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (pred [n, L] fp32, observed [n, L] bool) for the requested patients (all when None), in the requested order:
    pred = model.impute_lab_matrix(data, patient_indices); observed[i, l] = patient i has a has_lab edge to lab l."""
    pred = model.impute_lab_matrix(data, patient_indices)
    dev = pred.device
    P = int(data[ROW_TYPE].num_nodes)
    rows = torch.arange(P, device=dev) if patient_indices is None else patient_indices.to(torch.int64)
    observed = torch.zeros(pred.shape, dtype=torch.bool, device=dev)
    if rows.numel() == 0:
        return pred, observed
    ei = data[LAB_EDGE].edge_index.to(dev)
    uniq, inv = torch.unique(rows, return_inverse=True)        # (a request may repeat a patient)
    upos = torch.full((P,), -1, dtype=torch.int64, device=dev)
    upos[uniq] = torch.arange(uniq.numel(), device=dev)
    e_row = upos[ei[0]]
    keep = e_row >= 0
    obs_u = torch.zeros(uniq.numel(), pred.shape[1], dtype=torch.bool, device=dev)
    obs_u[e_row[keep], ei[1][keep]] = True
    return pred, obs_u[inv]


def _lab_stats_rows(lab_stats, names):
    # the reference's own lookup (inference.py:120): the first row of lab_stats whose ITEMID is the lab's name
    return {name: lab_stats[lab_stats['ITEMID'] == name].iloc[0] for name in names}


def lab_report(pred_row: np.ndarray, lab_indices: np.ndarray, values: np.ndarray, in_test: np.ndarray,
               lab_stats, lab_indexer: Dict, stats_rows: Optional[Dict] = None,
               bounds: Optional[Tuple[np.ndarray, np.ndarray]] = None, raw_row: Optional[np.ndarray] = None) -> Dict:
    """One patient's report, reference inference.py:107-178, from host data only.
    pred_row: [L] normalised predictions of every lab (a row of impute_lab_matrix); lab_indices / values / in_test: the
    patient's has_lab edges in edge order -- lab index, normalised value, edge in the test split.  Values are
    denormalised as value * std + mean with the lab's row of lab_stats (columns ITEMID, mean, std).
    bounds: (lower_row, upper_row), [L] normalised interval bounds of every lab (conformal.LabConformal.predict_matrix);
    every entry of masked_labs and truly_missing_labs then also has 'lower', 'upper' (bound * std + mean, as 'predicted'
    is formed), 'normalized_lower' and 'normalized_upper'.
    raw_row: [L] the model's own normalised predictions when pred_row holds stacked ones (stacking.LabStacker); every
    entry of masked_labs and truly_missing_labs then also has 'raw_prediction' (raw * std + mean) and
    'normalized_raw_prediction'.
    -> {'measured_labs', 'masked_labs', 'truly_missing_labs'} with the reference's keys."""

    def interval(lab_idx, lab_stat):
        if bounds is None:
            return {}
        lo, hi = bounds[0][lab_idx], bounds[1][lab_idx]
        return {'lower': float(lo * lab_stat['std'] + lab_stat['mean']), 'upper': float(hi * lab_stat['std'] + lab_stat['mean']),
                'normalized_lower': float(lo), 'normalized_upper': float(hi)}

    def raw(lab_idx, lab_stat):
        if raw_row is None:
            return {}
        r = raw_row[lab_idx]
        return {'raw_prediction': float(r * lab_stat['std'] + lab_stat['mean']), 'normalized_raw_prediction': float(r)}

    lab_idx_to_name = {v: k for k, v in lab_indexer.items()}
    if stats_rows is None:
        stats_rows = _lab_stats_rows(lab_stats, lab_indexer.keys())
    measured_labs, masked_labs = {}, {}
    for lab_idx, actual, test in zip(lab_indices, values, in_test):
        lab_name = lab_idx_to_name[lab_idx]
        pred = pred_row[lab_idx]
        lab_stat = stats_rows[lab_name]
        mean_val = lab_stat['mean']
        std_val = lab_stat['std']
        actual_original = actual * std_val + mean_val
        pred_original = pred * std_val + mean_val
        if test:
            masked_labs[lab_name] = {
                'predicted': float(pred_original),
                'actual': float(actual_original),
                'error': float(abs(pred_original - actual_original)),
                'normalized_predicted': float(pred),
                'normalized_actual': float(actual)
            }
            masked_labs[lab_name].update(interval(lab_idx, lab_stat))
            masked_labs[lab_name].update(raw(lab_idx, lab_stat))
        else:
            measured_labs[lab_name] = {
                'value': float(actual_original),
                'normalized': float(actual)
            }
    patient_lab_names = set(lab_idx_to_name[idx] for idx in lab_indices)
    truly_missing_labs = {}
    for lab_name, lab_idx in lab_indexer.items():
        if lab_name in patient_lab_names:
            continue
        pred = pred_row[lab_idx]
        lab_stat = stats_rows[lab_name]
        pred_original = pred * lab_stat['std'] + lab_stat['mean']
        truly_missing_labs[lab_name] = {
            'predicted': float(pred_original),
            'normalized_predicted': float(pred),
            'note': 'Lab was never measured for this patient'
        }
        truly_missing_labs[lab_name].update(interval(lab_idx, lab_stat))
        truly_missing_labs[lab_name].update(raw(lab_idx, lab_stat))
    return {
        'measured_labs': measured_labs,
        'masked_labs': masked_labs,
        'truly_missing_labs': truly_missing_labs
    }


def predict_for_patients(patient_ids: Sequence, data, model, device, labs_df, lab_stats, masker, patient_indexer: Dict,
                         lab_indexer: Dict, intervals=None, stacker=None, stack_features=None) -> List[Dict]:
    """predict_for_patient for many patients from ONE impute_lab_matrix forward -> one dict per id, in order.
    intervals: a fitted conformal.LabConformal; the bounds of every cell come from one more streaming launch.
    stacker: a fitted stacking.LabStacker; the predictions reported (and handed to ``intervals``, which should then have
    been fitted on stacked predictions) are the stacked ones, the model's own stay under 'raw_prediction'.
    stack_features: the stacker's predictors after the model's own -- the fitted baselines of
    ``stacking.fit_stacker(.., return_baselines=True)`` (a dict), or a sequence of [n, L] / [L] tensors."""
    idx = [patient_indexer[str(pid)] for pid in patient_ids]
    data_device = data.to(device)
    rows = torch.tensor(idx, dtype=torch.int64, device=device)
    pred = model.impute_lab_matrix(data_device, rows)
    lower = upper = raw = None
    if stacker is not None and idx:
        from .evaluate import baseline_matrix
        extra = stack_features if stack_features is not None else ()
        if isinstance(extra, dict):
            extra = [baseline_matrix(bm, rows, int(pred.shape[1])) for bm in extra.values()]
        raw = pred.cpu().numpy()
        pred = stacker.predict_matrix([pred] + list(extra), rows)
    if intervals is not None and idx:
        _, lower, upper = (t.cpu().numpy() if torch.is_tensor(t) else t for t in intervals.predict_matrix(pred, rows))
    pred = pred.cpu().numpy() if torch.is_tensor(pred) else pred
    if not idx:
        return []
    # the requested patients' edges, grouped by patient in edge order (torch.where(edge_index[0] == p) of the reference)
    ei = data_device[LAB_EDGE].edge_index
    attr = data_device[LAB_EDGE].edge_attr.reshape(-1)
    want = torch.zeros(int(data_device[ROW_TYPE].num_nodes), dtype=torch.bool, device=ei.device)
    want[rows.to(ei.device)] = True
    pos = torch.nonzero(want[ei[0]]).squeeze(1)
    e_pat, e_lab, e_val = ei[0][pos].cpu().numpy(), ei[1][pos].cpu().numpy(), attr[pos].cpu().numpy()
    pos = pos.cpu().numpy()
    order = np.argsort(e_pat, kind="stable")
    e_pat, e_lab, e_val, pos = e_pat[order], e_lab[order], e_val[order], pos[order]
    test_mask = masker.test_mask.cpu().numpy()
    stats_rows = _lab_stats_rows(lab_stats, lab_indexer.keys())
    out = []
    for i, p in enumerate(idx):
        lo, hi = np.searchsorted(e_pat, p, "left"), np.searchsorted(e_pat, p, "right")
        out.append(lab_report(pred[i], e_lab[lo:hi], e_val[lo:hi], test_mask[pos[lo:hi]], lab_stats, lab_indexer,
                              stats_rows, None if lower is None else (lower[i], upper[i]),
                              None if raw is None else raw[i]))
    return out


def predict_for_patient(patient_id: int, data, model, device, labs_df, lab_stats, masker, patient_indexer: Dict,
                        lab_indexer: Dict, intervals=None, stacker=None, stack_features=None) -> Dict:
    """Reference inference.py:53-178 (same arguments, same result): the patient's measured labs, the labs held out in
    the test split (predicted vs actual) and the labs never measured (predicted), denormalised through lab_stats --
    from one row of impute_lab_matrix instead of two whole-graph forwards."""
    return predict_for_patients([patient_id], data, model, device, labs_df, lab_stats, masker, patient_indexer,
                                lab_indexer, intervals, stacker, stack_features)[0]
