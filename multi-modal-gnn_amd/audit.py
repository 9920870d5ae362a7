"""Leakage audit and split diagnostics: the counterpart of the reference's ``src/audit_leakage.py`` (same function and
class names, arguments, result keys and strings).

* ``audit_patient_leakage`` / ``audit_masked_value_visibility``: on HIP tensors one pass of ``mmg_split_membership``
  gives the patients of each train / val / test membership class, and every field follows from those integer counts; on
  host tensors a numpy restatement derives the same counts.
* ``PatientHoldoutSplitter``: an ``EdgeMasker`` whose three masks hold out whole patients, bit-identical to the
  reference's for the same seed, built with one vectorised lookup instead of a Python loop per edge and split.
* ``compute_robust_metrics``: numpy input runs the reference's arithmetic on the host; HIP tensors run
  ``mmg_order_stats`` (exact order statistics of |residual|) and ``mmg_robust_sums`` (one fixed-order fp64 pass), and
  only 15 doubles come back.
* ``run_full_audit`` writes ``audit_report.json``; its predictions come from ``predict_lab_values`` (see there).
"""
from __future__ import annotations

import json
import logging
from pathlib import Path
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from .train import LAB_EDGE, EdgeMasker


# ============================================================================ split membership
def _membership_counts(patient: torch.Tensor, train_mask, val_mask, test_mask):
    """-> ([patients per membership class m = 0..7], edges in more than one split, edges in train and val or test)."""
    if patient.is_cuda:
        from . import ops
        pid = patient.contiguous().to(torch.int64)
        masks = [m.reshape(-1).to(device=pid.device, dtype=torch.bool).contiguous() for m in (train_mask, val_mask, test_mask)]
        n_pat = int(pid.max()) + 1 if pid.numel() else 0
        c = ops.split_membership(pid, *masks, n_pat).cpu().tolist()
        return c[:8], c[8], c[9]
    p = patient.cpu().numpy().astype(np.int64)
    ms = [np.asarray(m.cpu().numpy() if torch.is_tensor(m) else m, dtype=bool).reshape(-1) for m in (train_mask, val_mask, test_mask)]
    word_e = ms[0].astype(np.uint8) | (ms[1].astype(np.uint8) << 1) | (ms[2].astype(np.uint8) << 2)
    multi = int(np.count_nonzero(word_e & (word_e - 1)))
    train_other = int(np.count_nonzero((word_e & 1) & ((word_e & 6) != 0)))
    n_pat = int(p.max()) + 1 if p.size else 0
    word = np.zeros(n_pat, np.uint8)
    for bit, m in enumerate(ms):
        word[np.unique(p[m])] |= np.uint8(1 << bit)
    cls = np.bincount(word, minlength=8)
    return [0] + [int(v) for v in cls[1:8]], multi, train_other


def _patient_report(cls) -> Dict:
    def n(bits):
        return sum(cls[m] for m in range(1, 8) if m & bits == bits)
    return {
        "split_type": "edge_level",
        "num_train_patients": n(1),
        "num_val_patients": n(2),
        "num_test_patients": n(4),
        "train_val_overlap": n(3),
        "train_test_overlap": n(5),
        "val_test_overlap": n(6),
        "all_splits_overlap": n(7),
        "total_unique_patients": sum(cls[1:8]),
        "note": "Edge-level splits: patient overlap is EXPECTED and VALID",
    }


def audit_patient_leakage(edge_index: torch.Tensor, train_mask: torch.Tensor, val_mask: torch.Tensor,
                          test_mask: torch.Tensor) -> Dict:
    """audit_leakage.py:29-70: patients per split and their overlaps.  HIP tensors: one mmg_split_membership pass;
    host tensors: the numpy restatement.  Both give the reference's set arithmetic exactly."""
    cls, _, _ = _membership_counts(edge_index[0], train_mask, val_mask, test_mask)
    return _patient_report(cls)


def _store_x(store):
    get = getattr(store, "get", None)
    if get is not None:
        return get("x", None)
    return store.x if "x" in store else None


def audit_masked_value_visibility(data, masker: EdgeMasker) -> Dict:
    """audit_leakage.py:73-119: node features, edge attributes, and whether the train mask overlaps val or test (on HIP
    masks from the counts of mmg_split_membership)."""
    report = {
        "masked_values_in_node_features": False,
        "masked_values_in_other_edges": False,
        "supervision_leak": False,
    }
    if _store_x(data["patient"]) is not None or _store_x(data["lab"]) is not None:
        report["masked_values_in_node_features"] = True
        report["node_feature_leak_details"] = "Raw features detected in nodes"
    else:
        report["node_feature_leak_details"] = "✓ All nodes use learnable embeddings only"
    report["edge_attribute_leak_details"] = "✓ Only patient-lab edges have attributes"
    tm, vm, sm = masker.train_mask, masker.val_mask, masker.test_mask
    if tm.is_cuda:
        _, _, train_other = _membership_counts(masker.edge_index[0], tm, vm, sm)
        leak = train_other > 0
    else:
        leak = bool(torch.any(tm & vm) or torch.any(tm & sm))
    if leak:
        report["supervision_leak"] = True
        report["supervision_leak_details"] = "Train mask overlaps with val/test!"
    else:
        report["supervision_leak_details"] = "✓ Train/val/test masks are mutually exclusive"
    return report


# ============================================================================ patient-holdout split
class PatientHoldoutSplitter(EdgeMasker):
    """audit_leakage.py:126-198: train, validation and test are disjoint sets of PATIENTS (70/15/15 of the patients that
    have a has_lab edge), and every has_lab edge goes to its patient's split.

    Only the three masks differ from ``EdgeMasker``: the supervision draw, ``get_masked_data``, ``to`` and ``shard`` are
    inherited, so ``Trainer`` trains on it unchanged.  The masks are bit-identical to the reference's for the same seed
    (the same CPU ``torch.manual_seed`` / ``np.random.seed`` / ``torch.randperm`` over ``torch.unique(edge_index[0])``
    and the same ``int(split * n)`` boundaries); they are made by one lookup of each edge's patient in a per-patient
    split table instead of the reference's Python loop per edge and split.

    As in the reference, held-out patients keep their has_lab edges in the message-passing graph: the split decides
    which edges are supervised and scored, not which edges the encoder sees."""

    def __init__(self, data, train_split: float = 0.7, val_split: float = 0.15, test_split: float = 0.15,
                 seed: int = 42, mask_fraction: float = 0.2, mask_generator: Optional[torch.Generator] = None):
        super().__init__(data, train_split, val_split, test_split, mask_fraction=mask_fraction, seed=seed,
                         mask_generator=mask_generator)
        logging.info("\nPatient-holdout splits created:")
        logging.info(f"  Train patients: {len(self.train_patients)} ({train_split*100:.1f}%)")
        logging.info(f"  Val patients: {len(self.val_patients)} ({val_split*100:.1f}%)")
        logging.info(f"  Test patients: {len(self.test_patients)} ({test_split*100:.1f}%)")
        assert len(self.train_patients & self.val_patients) == 0
        assert len(self.train_patients & self.test_patients) == 0
        assert len(self.val_patients & self.test_patients) == 0
        logging.info("  ✓ No patient overlap between splits")

    def _create_splits(self):
        patient_indices = self.edge_index[0]
        self.unique_patients = torch.unique(patient_indices.cpu())
        self.num_patients = len(self.unique_patients)
        torch.manual_seed(self.seed)
        np.random.seed(self.seed)
        perm = torch.randperm(self.num_patients)
        n_train = int(self.train_split * self.num_patients)
        n_val = int(self.val_split * self.num_patients)
        parts = (perm[:n_train], perm[n_train:n_train + n_val], perm[n_train + n_val:])
        self.train_patients, self.val_patients, self.test_patients = (set(self.unique_patients[p].tolist()) for p in parts)
        # split of every patient id (3 = no has_lab edge), then one gather over the edges
        n_ids = int(self.unique_patients[-1]) + 1 if self.num_patients else 0
        split_of = torch.full((max(n_ids, 1),), 3, dtype=torch.int8)
        for s, p in enumerate(parts):
            split_of[self.unique_patients[p]] = s
        edge_split = split_of.to(patient_indices.device)[patient_indices]
        return tuple(edge_split == s for s in range(3))


def compare_split_strategies(data, config: Dict) -> Dict:
    """audit_leakage.py:201-261: the patient distribution of the edge-level and of the patient-holdout split."""
    tc = config["train"]
    edge_splitter = EdgeMasker(data, train_split=tc["train_split"], val_split=tc["val_split"],
                               test_split=tc["test_split"], seed=tc["seed"])
    patient_splitter = PatientHoldoutSplitter(data, train_split=tc["train_split"], val_split=tc["val_split"],
                                              test_split=tc["test_split"], seed=tc["seed"])
    ei = data[LAB_EDGE].edge_index
    edge_audit = audit_patient_leakage(ei, edge_splitter.train_mask, edge_splitter.val_mask, edge_splitter.test_mask)
    patient_audit = audit_patient_leakage(ei, patient_splitter.train_mask, patient_splitter.val_mask,
                                          patient_splitter.test_mask)
    patient_audit["split_type"] = "patient_holdout"
    patient_audit["note"] = "Patient-holdout: NO patient overlap (more conservative)"
    return {
        "edge_level_split": edge_audit,
        "patient_holdout_split": patient_audit,
        "recommendation": (
            "Edge-level split is standard for link prediction tasks. "
            "Patient-holdout is more conservative but may underestimate model utility "
            "in settings where we need to impute labs for existing patients."
        ),
    }


# ============================================================================ robust metrics
def percentile_plan(n: int, pct: float):
    """numpy's "linear" percentile of n sorted fp32 values as (i, j, gamma): value = x[i] + (x[j] - x[i]) * gamma, in
    numpy's own fp32 operations (``lerp_f32``).  The virtual index (n - 1) * q is formed in fp32, as numpy does for an
    fp32 array."""
    q = np.float32(pct) / np.float32(100)
    vi = np.float32(n - 1) * q
    if vi >= np.float32(n - 1):
        return n - 1, n - 1, np.float32(0)
    if vi < 0:
        return 0, 0, np.float32(0)
    fl = np.floor(vi)
    return int(fl), int(fl) + 1, np.float32(vi - fl)


def lerp_f32(xi, xj, g):
    """numpy's _lerp on fp32 scalars: every operation rounded on its own."""
    xi, xj, g = np.float32(xi), np.float32(xj), np.float32(g)
    d = np.float32(xj - xi)
    if g >= 0.5:
        return np.float32(xj - np.float32(d * np.float32(np.float32(1) - g)))
    return np.float32(xi + np.float32(d * g))


def _check_pct(winsorize_pct):
    for p in (winsorize_pct, 100 - winsorize_pct):
        if not 0 <= p <= 100:
            raise ValueError("Percentiles must be in the range [0, 100]")


def _robust_host(y_true: np.ndarray, y_pred: np.ndarray, winsorize_pct: float) -> Dict:
    """audit_leakage.py:264-338 as written (numpy, the caller's dtype)."""
    residuals = y_pred - y_true
    abs_residuals = np.abs(residuals)
    mae = np.mean(abs_residuals)
    rmse = np.sqrt(np.mean(residuals ** 2))
    r2 = 1 - (np.sum(residuals ** 2) / np.sum((y_true - np.mean(y_true)) ** 2))
    smape = 100 * np.mean(abs_residuals / (np.abs(y_true) + np.abs(y_pred) + 1e-8))
    wape = 100 * np.sum(abs_residuals) / (np.sum(np.abs(y_true)) + 1e-8)
    lower = np.percentile(abs_residuals, winsorize_pct)
    upper = np.percentile(abs_residuals, 100 - winsorize_pct)
    abs_residuals_winsorized = np.clip(abs_residuals, lower, upper)
    mae_winsorized = np.mean(abs_residuals_winsorized)
    rmse_winsorized = np.sqrt(np.mean(np.clip(residuals, -upper, upper) ** 2))
    return {
        "mae": float(mae),
        "rmse": float(rmse),
        "r2": float(r2),
        "smape": float(smape),
        "wape": float(wape),
        "mae_winsorized": float(mae_winsorized),
        "rmse_winsorized": float(rmse_winsorized),
        "winsorize_percentile": winsorize_pct,
        "num_outliers_capped": int(np.sum((abs_residuals < lower) | (abs_residuals > upper))),
        "outlier_percentage": float(100 * np.mean((abs_residuals < lower) | (abs_residuals > upper))),
        "max_residual": float(np.max(abs_residuals)),
        "p95_residual": float(np.percentile(abs_residuals, 95)),
    }


def robust_metrics_from_sums(s, winsorize_pct: float) -> Dict:
    """The compute_robust_metrics dict from the 15 fp64 fields of mmg_robust_sums (include/mmgnn.h)."""
    s = np.asarray(s, np.float64)
    n = s[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        ss_tot = s[4] - s[3] * s[3] / n
        r2 = 1 - s[2] / ss_tot
    return {
        "mae": float(s[1] / n),
        "rmse": float(np.sqrt(s[2] / n)),
        "r2": float(r2),
        "smape": float(100 * s[5] / n),
        "wape": float(100 * s[1] / (s[6] + 1e-8)),
        "mae_winsorized": float(s[7] / n),
        "rmse_winsorized": float(np.sqrt(s[8] / n)),
        "winsorize_percentile": winsorize_pct,
        "num_outliers_capped": int(s[9]),
        "outlier_percentage": float(100 * s[9] / n),
        "max_residual": float(s[11]),
        "p95_residual": float(s[_lib.MMG_RS_P95]),
    }


def robust_sums_device(y_true: torch.Tensor, y_pred: torch.Tensor, winsorize_pct: float = 5.0) -> torch.Tensor:
    """The device half of compute_robust_metrics: mmg_order_stats of |y_pred - y_true| at the ranks the three
    percentiles need, then mmg_robust_sums.  -> fp64 [15] on the device; nothing synchronises with the host."""
    from . import ops
    yt = y_true.reshape(-1).to(torch.float32).contiguous()
    yp = y_pred.reshape(-1).to(torch.float32).contiguous()
    n = yt.numel()
    if n == 0 or yp.numel() != n:
        raise ValueError(f"compute_robust_metrics: need matching non-empty arrays, got {n} and {yp.numel()} values")
    _check_pct(winsorize_pct)
    plans = [percentile_plan(n, p) for p in (winsorize_pct, 100 - winsorize_pct, 95)]
    ranks = sorted({i for i, j, _ in plans} | {j for i, j, _ in plans})
    xs, nan_count = ops.order_stats(yp, ranks, b=yt)
    at = {r: k for k, r in enumerate(ranks)}
    specs = [(at[i], at[j], float(g)) for i, j, g in plans]
    return ops.robust_sums(yp, yt, xs, nan_count, *specs)


def compute_robust_metrics(y_true, y_pred, winsorize_pct: float = 5.0) -> Dict:
    """audit_leakage.py:264-338: MAE, RMSE, R², SMAPE, WAPE, |residual| winsorised at the winsorize_pct / 100 -
    winsorize_pct percentiles, outlier counts, max and p95 residual.  HIP tensors: computed on the device (exact order
    statistics, fp64 sums in a fixed order; 15 doubles come back in one copy).  Anything else: the reference's numpy
    arithmetic.  The reference's quirks stay: the lower bound also RAISES |residuals| below it, the winsorised RMSE
    clips the signed residuals to +- upper only, and any NaN makes the percentiles NaN.  An empty input raises
    ValueError on both paths."""
    if torch.is_tensor(y_true) and torch.is_tensor(y_pred) and y_true.is_cuda and y_pred.is_cuda:
        return robust_metrics_from_sums(robust_sums_device(y_true, y_pred, winsorize_pct).cpu().numpy(), winsorize_pct)
    yt = y_true.detach().cpu().numpy() if torch.is_tensor(y_true) else np.asarray(y_true)
    yp = y_pred.detach().cpu().numpy() if torch.is_tensor(y_pred) else np.asarray(y_pred)
    if yt.size == 0 or yp.size != yt.size:
        raise ValueError(f"compute_robust_metrics: need matching non-empty arrays, got {yt.size} and {yp.size} values")
    _check_pct(winsorize_pct)
    return _robust_host(yt, yp, winsorize_pct)


# ============================================================================ full audit
def _host_view(graph):
    """A host copy of what the audits read: the patient and lab stores and the has_lab edges."""
    from .data import HeteroGraph
    h = HeteroGraph()
    for nt in ("patient", "lab"):
        for k in ("num_nodes", "x"):
            if k in graph[nt]:
                v = getattr(graph[nt], k)
                setattr(h[nt], k, v.cpu() if torch.is_tensor(v) else v)
    h[LAB_EDGE].edge_index = graph[LAB_EDGE].edge_index.cpu()
    h[LAB_EDGE].edge_attr = graph[LAB_EDGE].edge_attr.cpu()
    return h


def _masks_on(masker: EdgeMasker, device) -> EdgeMasker:
    """A shallow copy of the masker whose edge list and split masks live on `device`."""
    m = object.__new__(type(masker))
    m.__dict__.update(masker.__dict__)
    m.edge_index = masker.edge_index.to(device)
    m.train_mask, m.val_mask, m.test_mask = (t.to(device) for t in (masker.train_mask, masker.val_mask, masker.test_mask))
    return m


def run_full_audit(model, graph, config: Dict, output_dir, masker: Optional[EdgeMasker] = None,
                   device_reducers: bool = True) -> Dict:
    """audit_leakage.py:345-490: leakage check, patient distribution, split comparison and robust test metrics, written
    to ``output_dir / audit_report.json`` with the reference's keys.

    The reference takes the test predictions from ``model(data)`` indexed by the test mask, which cannot run: the
    forward returns a dict of node embeddings, not one prediction per edge.  Here they come from
    ``model.predict_lab_values`` on the test edges, as ``evaluate_model`` takes them.  ``masker``: the edge-level split
    to audit (default: a new ``EdgeMasker`` from the config, as the reference builds it).  ``device_reducers=False``
    copies masks and predictions to the host and runs the numpy restatements instead of the kernels."""
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    tc = config["train"]
    if masker is None:
        masker = EdgeMasker(graph, train_split=tc["train_split"], val_split=tc["val_split"],
                            test_split=tc["test_split"], seed=tc["seed"])
    device = next(model.parameters()).device
    graph_dev = graph.to(device)
    audit_graph = graph_dev if device_reducers else _host_view(graph_dev)
    audit_masker = _masks_on(masker, audit_graph[LAB_EDGE].edge_index.device)

    leakage_report = audit_masked_value_visibility(audit_graph, audit_masker)
    patient_dist = audit_patient_leakage(audit_masker.edge_index, audit_masker.train_mask, audit_masker.val_mask,
                                         audit_masker.test_mask)
    comparison = compare_split_strategies(audit_graph, config)

    model.eval()
    ei = graph_dev[LAB_EDGE].edge_index
    ea = graph_dev[LAB_EDGE].edge_attr
    test_mask = masker.test_mask.to(ei.device)
    pi, li = ei[0][test_mask].contiguous(), ei[1][test_mask].contiguous()
    y_true = ea[test_mask].reshape(-1).float().contiguous()
    with torch.no_grad():
        y_pred = model.predict_lab_values(graph_dev, pi, li).reshape(-1).float()
    if device_reducers:
        robust_metrics = compute_robust_metrics(y_true, y_pred, winsorize_pct=5.0)
    else:
        robust_metrics = compute_robust_metrics(y_true.cpu().numpy(), y_pred.cpu().numpy(), winsorize_pct=5.0)

    audit_report = {
        "leakage_check": leakage_report,
        "patient_distribution": patient_dist,
        "split_comparison": comparison,
        "robust_metrics": robust_metrics,
    }
    with open(output_dir / "audit_report.json", "w") as f:
        json.dump(audit_report, f, indent=2)
    logging.info(f"Full report saved to {output_dir / 'audit_report.json'}")
    return audit_report
