"""Numpy restatement of the reference's audit arithmetic (src/audit_leakage.py), the checker of mmgnn.audit.

* robust_metrics_f32: compute_robust_metrics as the reference writes it, on fp32 arrays (numpy's own operations).
* robust_sums_f64 / robust_metrics_f64: the same elementwise fp32 terms the device forms (r = p - t, |r|, the SMAPE term,
  the clipped values; bounds from numpy's percentile) summed in fp64 -- the fields of mmg_robust_sums.
* patient_sets_report: audit_patient_leakage with Python sets, as the reference does it.
* holdout_masks_loop: PatientHoldoutSplitter's masks by the reference's loop over the edges (slow: sub-samples only).
"""
import numpy as np
import torch


def robust_metrics_f32(y_true, y_pred, winsorize_pct=5.0):
    y_true = np.asarray(y_true, np.float32)
    y_pred = np.asarray(y_pred, np.float32)
    residuals = y_pred - y_true
    abs_residuals = np.abs(residuals)
    with np.errstate(divide="ignore", invalid="ignore"):
        mae = np.mean(abs_residuals)
        rmse = np.sqrt(np.mean(residuals ** 2))
        r2 = 1 - (np.sum(residuals ** 2) / np.sum((y_true - np.mean(y_true)) ** 2))
        smape = 100 * np.mean(abs_residuals / (np.abs(y_true) + np.abs(y_pred) + 1e-8))
        wape = 100 * np.sum(abs_residuals) / (np.sum(np.abs(y_true)) + 1e-8)
    lower = np.percentile(abs_residuals, winsorize_pct)
    upper = np.percentile(abs_residuals, 100 - winsorize_pct)
    mae_w = np.mean(np.clip(abs_residuals, lower, upper))
    rmse_w = np.sqrt(np.mean(np.clip(residuals, -upper, upper) ** 2))
    out = (abs_residuals < lower) | (abs_residuals > upper)
    return {"mae": float(mae), "rmse": float(rmse), "r2": float(r2), "smape": float(smape), "wape": float(wape),
            "mae_winsorized": float(mae_w), "rmse_winsorized": float(rmse_w), "winsorize_percentile": winsorize_pct,
            "num_outliers_capped": int(np.sum(out)), "outlier_percentage": float(100 * np.mean(out)),
            "max_residual": float(np.max(abs_residuals)), "p95_residual": float(np.percentile(abs_residuals, 95))}


def robust_sums_f64(y_true, y_pred, winsorize_pct=5.0):
    """The 15 fields of mmg_robust_sums (include/mmgnn.h), fp32 terms summed in fp64."""
    t = np.asarray(y_true, np.float32).reshape(-1)
    p = np.asarray(y_pred, np.float32).reshape(-1)
    r = p - t
    ar = np.abs(r)
    lo = np.percentile(ar, winsorize_pct)
    hi = np.percentile(ar, 100 - winsorize_pct)
    q95 = np.percentile(ar, 95)
    with np.errstate(divide="ignore", invalid="ignore"):
        sm = ar / (np.abs(t) + np.abs(p) + np.float32(1e-8))
    cw = np.clip(ar, lo, hi)
    cr = np.clip(r, -hi, hi)
    d = lambda x: np.asarray(x, np.float64)  # noqa: E731
    nan = int(np.isnan(ar).sum())
    return np.array([t.size, d(ar).sum(), (d(r) ** 2).sum(), d(t).sum(), (d(t) ** 2).sum(), d(sm).sum(), np.abs(d(t)).sum(),
                     d(cw).sum(), (d(cr) ** 2).sum(), int(((ar < lo) | (ar > hi)).sum()), nan,
                     np.nan if nan else float(np.max(ar)), lo, hi, q95], np.float64)


def robust_metrics_f64(y_true, y_pred, winsorize_pct=5.0):
    """compute_robust_metrics from the fp64 sums, R² from a two-pass fp64 total sum of squares."""
    s = robust_sums_f64(y_true, y_pred, winsorize_pct)
    t = np.asarray(y_true, np.float32).astype(np.float64).reshape(-1)
    n = s[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        r2 = 1 - s[2] / np.sum((t - t.mean()) ** 2)
    return {"mae": s[1] / n, "rmse": float(np.sqrt(s[2] / n)), "r2": float(r2), "smape": 100 * s[5] / n,
            "wape": 100 * s[1] / (s[6] + 1e-8), "mae_winsorized": s[7] / n, "rmse_winsorized": float(np.sqrt(s[8] / n)),
            "winsorize_percentile": winsorize_pct, "num_outliers_capped": int(s[9]),
            "outlier_percentage": 100 * s[9] / n, "max_residual": float(s[11]), "p95_residual": float(s[14])}


def patient_sets_report(edge_index, train_mask, val_mask, test_mask):
    pid = np.asarray(edge_index[0])
    tr, va, te = (set(pid[np.asarray(m, bool)].tolist()) for m in (train_mask, val_mask, test_mask))
    return {"split_type": "edge_level", "num_train_patients": len(tr), "num_val_patients": len(va),
            "num_test_patients": len(te), "train_val_overlap": len(tr & va), "train_test_overlap": len(tr & te),
            "val_test_overlap": len(va & te), "all_splits_overlap": len(tr & va & te),
            "total_unique_patients": len(tr | va | te),
            "note": "Edge-level splits: patient overlap is EXPECTED and VALID"}


def holdout_masks_loop(patient_indices, train_patients, val_patients, test_patients):
    """The reference's mask construction (audit_leakage.py:170-180), literally."""
    patient_indices = torch.as_tensor(patient_indices)
    return tuple(torch.tensor([p.item() in s for p in patient_indices], dtype=torch.bool)
                 for s in (train_patients, val_patients, test_patients))
