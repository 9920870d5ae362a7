"""Where the model is wrong: the three tables of the reference's ``src/advanced_visualizations.py`` (per-lab
calibration, error against patient lab-degree, parity by lab-frequency decile), without the plotting and over EVERY
prediction pair instead of the reference's unseeded 10,000-pair sample.

Every table is a function of a few sums over the pairs (pred, target, patient index, lab index):

* first read (``mmg_pair_analysis``): per lab ``n, sum t, sum p, sum t^2, sum t p, sum |p - t|, sum (p - t)^2, min t,
  max t``; per degree bin ``n, sum |p - t|``;
* second read (``mmg_pair_calibrated_abs``), with the least-squares line of every lab and the mean error of every bin
  from the first: per lab ``sum |(a t + b) - t|``, per bin ``sum (|p - t| - mean_bin)^2``.

HIP tensors run the two kernels (fp64 sums in a fixed order: the tables are bitwise reproducible) and only the small
tables of sums come back; numpy arrays -- and more than 2048 labs -- run the same sums in numpy on the host.  The tables
are assembled from the sums on the host by the same code in both cases.  The elementwise terms are the reference's
(``p - t``, its absolute value and square, ``a * t + b`` with the fp32 line, all formed in fp32 on fp32 inputs); what
differs from the reference is that every reduction and the least-squares solve are fp64.
"""
from __future__ import annotations

import logging
from pathlib import Path
from typing import Dict, Optional, Sequence

import numpy as np
import pandas as pd
import torch

from . import _lib
from .train import LAB_EDGE

DEFAULT_BINS = (0, 1, 6, 16, 50)
DEFAULT_LABELS = ("0-1", "2-5", "6-15", "16+")
CALIBRATION_COLUMNS = ["lab_idx", "lab_name", "n_samples", "a", "b", "mae_before", "mae_after", "delta_mae",
                       "is_calibrated"]
DEGREE_COLUMNS = ["degree_bin", "mean", "std", "count"]
DECILE_COLUMNS = ["decile", "n_labs", "count_min", "count_max", "n_pairs", "mae", "r2"]
# columns of the first read's lab table (MMG_AN_LAB_FIELDS)
N, ST, SP, STT, STP, SAE, SSE, TMIN, TMAX = range(_lib.MMG_AN_LAB_FIELDS)


# ============================================================================ inputs
def _is_dev(x) -> bool:
    return torch.is_tensor(x) and x.is_cuda


def _flat(x, what):
    if torch.is_tensor(x):
        x = x.detach().reshape(-1)
        return x.contiguous() if x.is_cuda else x.cpu().numpy()
    return np.asarray(x).reshape(-1)


def _values(x, what, dev):
    """fp32 values, on the device when the analysis runs there."""
    x = _flat(x, what)
    if dev is not None:
        x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
        return x.to(device=dev, dtype=torch.float32).contiguous()
    return np.asarray(x.cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float32)


def _indices(x, what, dev):
    x = _flat(x, what)
    if dev is not None:
        x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
        x = x.to(dev)
        if x.dtype not in (torch.int64, torch.int32):
            x = x.to(torch.int64)
        return x.contiguous()
    x = np.asarray(x.cpu().numpy() if torch.is_tensor(x) else x)
    if x.dtype.kind not in "iu":
        raise TypeError(f"{what}: expected integer indices, got {x.dtype}")
    return x.astype(np.int64, copy=False)


def _same_length(**arrays):
    sizes = {k: (v.numel() if torch.is_tensor(v) else v.size) for k, v in arrays.items() if v is not None}
    if len(set(sizes.values())) > 1:
        raise ValueError(f"prediction analysis: inputs of different lengths: {sizes}")
    return next(iter(sizes.values()))


def _device_of(*xs):
    for x in xs:
        if _is_dev(x):
            return x.device
    return None


def _to_host(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else x


def _lab_name(lab_names, idx: int) -> str:
    if lab_names is None:
        return f"Lab_{idx}"
    if isinstance(lab_names, dict):
        return lab_names.get(idx, f"Lab_{idx}")
    return lab_names[idx] if 0 <= idx < len(lab_names) else f"Lab_{idx}"


def _edges(bins, labels):
    e = [float(b) for b in bins]
    if len(e) < 2 or any(not (e[i] < e[i + 1]) for i in range(len(e) - 1)):
        raise ValueError("bins must increase monotonically.")
    if len(labels) != len(e) - 1:
        raise ValueError("Bin labels must be one fewer than the number of bin edges")
    return e


def patient_degrees(graph_data, dev=None):
    """The has_lab out-degree of every patient: int32 on the device from the graph plan (mmg_row_degree), a numpy
    bincount on the host.  A tensor or array of degrees passes through."""
    if torch.is_tensor(graph_data) or isinstance(graph_data, np.ndarray):
        d = graph_data
        if dev is not None:
            d = d if torch.is_tensor(d) else torch.from_numpy(np.ascontiguousarray(d))
            return d.to(device=dev, dtype=torch.int32).contiguous()
        return np.asarray(_to_host(d)).astype(np.int64)
    lab_deg = getattr(graph_data, "lab_deg", None)            # a GraphPlan
    if lab_deg is None:
        ei = graph_data[LAB_EDGE].edge_index
        if dev is not None and ei.is_cuda:
            from .data import build_plan
            lab_deg = build_plan(graph_data, ei.device).lab_deg
        else:
            d = np.bincount(ei[0].cpu().numpy(), minlength=int(graph_data["patient"].num_nodes))
            return patient_degrees(d, dev)
    return patient_degrees(lab_deg, dev)


# ============================================================================ the two reads
def _device_fits(n_labs: int, n_bins: int) -> bool:
    return n_labs + n_bins > 0 and _lib.load().mmg_pair_analysis_ws_bytes(1, int(n_labs), int(n_bins)) > 0


def _host_lab_valid(lab, n_labs):
    return (lab >= 0) & (lab < n_labs)


def _first_read_host(pred, target, lab, n_labs, patient, deg, edges):
    r = pred - target                                        # fp32, as the reference forms it
    ae = np.abs(r)
    lab_sums = bin_sums = None
    if lab is not None and n_labs > 0:
        ok = _host_lab_valid(lab, n_labs)
        li = lab[ok]
        t64, p64 = target[ok].astype(np.float64), pred[ok].astype(np.float64)
        terms = [np.ones(li.size), t64, p64, t64 * t64, t64 * p64, ae[ok].astype(np.float64),
                 (r[ok] * r[ok]).astype(np.float64)]
        lab_sums = np.empty((n_labs, 9), np.float64)
        for f, w in enumerate(terms):
            lab_sums[:, f] = np.bincount(li, weights=w, minlength=n_labs)
        lab_sums[:, TMIN], lab_sums[:, TMAX] = np.inf, -np.inf
        np.minimum.at(lab_sums[:, TMIN], li, t64)
        np.maximum.at(lab_sums[:, TMAX], li, t64)
    if patient is not None and edges is not None:
        b, okb = _host_bins(patient, deg, edges)
        nb = len(edges) - 1
        bin_sums = np.stack([np.bincount(b[okb], minlength=nb).astype(np.float64),
                             np.bincount(b[okb], weights=ae[okb].astype(np.float64), minlength=nb)], axis=1)
    return lab_sums, bin_sums


def _host_bins(patient, deg, edges):
    okp = (patient >= 0) & (patient < deg.size)
    d = np.where(okp, deg[np.where(okp, patient, 0)], -1).astype(np.float64)
    e = np.asarray(edges, np.float64)
    b = np.searchsorted(e, d, side="right") - 1              # [e_j, e_j+1)
    ok = okp & (d >= 0) & (b >= 0) & (b < e.size - 1)
    return np.where(ok, b, 0), ok


def _second_read_host(pred, target, lab, a32, b32, patient, deg, edges, bin_mean):
    lab_abs = bin_sq = None
    if lab is not None and a32 is not None:
        n_labs = a32.size
        ok = _host_lab_valid(lab, n_labs)
        li, t = lab[ok], target[ok]
        cal = a32[li] * t + b32[li]                          # fp32 operands: every operation rounded on its own
        lab_abs = np.bincount(li, weights=np.abs(cal - t).astype(np.float64), minlength=n_labs)
    if patient is not None and edges is not None:
        b, okb = _host_bins(patient, deg, edges)
        x = np.abs(pred - target)[okb].astype(np.float64) - np.asarray(bin_mean, np.float64)[b[okb]]
        bin_sq = np.bincount(b[okb], weights=x * x, minlength=len(edges) - 1)
    return lab_abs, bin_sq


def _first_read(pred, target, lab, n_labs, patient, deg, edges):
    """-> (lab sums [n_labs, 9] or None, bin sums [n_bins, 2] or None) as numpy fp64."""
    if _is_dev(pred):
        from . import ops
        ls, bs = ops.pair_analysis(pred, target, lab, n_labs, patient, deg, edges)
        return (None if ls is None else ls.cpu().numpy()), (None if bs is None else bs.cpu().numpy())
    return _first_read_host(pred, target, lab, n_labs, patient, deg, edges)


def _second_read(pred, target, lab, a32, b32, patient, deg, edges, bin_mean):
    if _is_dev(target):
        from . import ops
        dev = target.device
        ta = torch.from_numpy(a32).to(dev) if a32 is not None else None
        tb = torch.from_numpy(b32).to(dev) if b32 is not None else None
        tm = torch.from_numpy(np.ascontiguousarray(bin_mean, np.float64)).to(dev) if bin_mean is not None else None
        la, bq = ops.pair_calibrated_abs(pred, target, lab if ta is not None else None, ta, tb,
                                         patient if tm is not None else None, deg, edges, tm)
        return (None if la is None else la.cpu().numpy()), (None if bq is None else bq.cpu().numpy())
    return _second_read_host(pred, target, lab, a32, b32, patient, deg, edges, bin_mean)


def _prepare(predictions, targets, lab_indices=None, patient_indices=None, n_labs=None, n_bins=0):
    """Flatten and place the inputs: on the device when the predictions are there and the tables fit its kernels."""
    dev = _device_of(predictions, targets)
    pred, target = _flat(predictions, "predictions"), _flat(targets, "targets")
    lab = None if lab_indices is None else _flat(lab_indices, "lab_indices")
    pat = None if patient_indices is None else _flat(patient_indices, "patient_indices")
    n = _same_length(predictions=pred, targets=target, lab_indices=lab, patient_indices=pat)
    if lab is not None and n_labs is None:
        n_labs = (int(lab.max()) + 1) if n else 0
    if dev is not None and n == 0:
        dev = None                                           # nothing to read: the (empty) tables come from the host code
    if dev is not None and not _device_fits(n_labs or 0, n_bins):
        logging.info(f"prediction analysis: {n_labs} labs / {n_bins} bins exceed the device tables, using the host arithmetic")
        dev = None
    pred, target = _values(pred, "predictions", dev), _values(target, "targets", dev)
    lab = None if lab is None else _indices(lab, "lab_indices", dev)
    pat = None if pat is None else _indices(pat, "patient_indices", dev)
    if dev is not None and lab is not None and pat is not None and lab.dtype != pat.dtype:
        lab, pat = lab.to(torch.int64), pat.to(torch.int64)
    return dev, n, pred, target, lab, pat, int(n_labs or 0)


# ============================================================================ tables from the sums
def calibration_line(lab_sums: np.ndarray):
    """Least-squares pred = a * true + b of every lab from its sums (fp64).  A lab whose targets are all equal has no
    slope: a = 0, b = mean(pred), as sklearn's LinearRegression returns.  Labs without a pair: NaN."""
    s = np.asarray(lab_sums, np.float64)
    n = s[:, N]
    with np.errstate(divide="ignore", invalid="ignore"):
        sxx = s[:, STT] - s[:, ST] * s[:, ST] / n
        sxy = s[:, STP] - s[:, ST] * s[:, SP] / n
        flat = s[:, TMIN] == s[:, TMAX]
        a = np.where(flat, 0.0, sxy / sxx)
        b = (s[:, SP] - a * s[:, ST]) / n
    return a, b


def calibration_frame(lab_sums, lab_abs, a, b, lab_names) -> pd.DataFrame:
    s = np.asarray(lab_sums, np.float64)
    keep = np.nonzero(s[:, N] >= 2)[0]                       # fewer than 2 pairs: left out
    n = s[keep, N]
    mae_before = s[keep, SAE] / n
    mae_after = np.asarray(lab_abs, np.float64)[keep] / n
    df = pd.DataFrame({
        "lab_idx": keep.astype(np.int64),
        "lab_name": [_lab_name(lab_names, int(i)) for i in keep],
        "n_samples": n.astype(np.int64),
        "a": a[keep], "b": b[keep],
        "mae_before": mae_before, "mae_after": mae_after, "delta_mae": mae_after - mae_before,
        "is_calibrated": (np.abs(a[keep] - 1.0) < 0.1) & (np.abs(b[keep]) < 0.1),
    }, columns=CALIBRATION_COLUMNS)
    return df.sort_values("mae_before", ascending=False)


def degree_frame(bin_sums, bin_sq, labels) -> pd.DataFrame:
    s = np.asarray(bin_sums, np.float64)
    n = s[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(n > 0, s[:, 1] / n, np.nan)
        std = np.where(n > 1, np.sqrt(np.asarray(bin_sq, np.float64) / (n - 1)), np.nan)      # ddof = 1
    return pd.DataFrame({"degree_bin": pd.Categorical(list(labels), categories=list(labels), ordered=True),
                         "mean": mean, "std": std, "count": n.astype(np.int64)}, columns=DEGREE_COLUMNS)


def bin_means(bin_sums):
    s = np.asarray(bin_sums, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s[:, 0] > 0, s[:, 1] / s[:, 0], 0.0)


def decile_frame(lab_sums) -> pd.DataFrame:
    s = np.asarray(lab_sums, np.float64)
    present = np.nonzero(s[:, N] > 0)[0]
    if present.size == 0:
        return pd.DataFrame({c: pd.Series(dtype=np.float64 if c in ("mae", "r2") else np.int64) for c in DECILE_COLUMNS})
    counts = s[present, N].astype(np.int64)
    order = np.argsort(counts, kind="stable")
    present, counts = present[order], counts[order]
    dec = np.asarray(pd.qcut(pd.Series(counts), q=10, labels=False, duplicates="drop"))
    rows = []
    for d in sorted(set(int(v) for v in dec if v == v)):     # (one distinct count: qcut forms no decile at all)
        m = dec == d
        t = s[present[m]]
        n = t[:, N].sum()
        st, stt = t[:, ST].sum(), t[:, STT].sum()
        flat = t[:, TMIN].min() == t[:, TMAX].max()
        ss_tot = 0.0 if flat else stt - st * st / n
        with np.errstate(divide="ignore", invalid="ignore"):
            r2 = float(1.0 - np.float64(t[:, SSE].sum()) / np.float64(ss_tot))      # bare 1 - SS_res / SS_tot
        rows.append({"decile": d, "n_labs": int(m.sum()), "count_min": int(counts[m].min()),
                     "count_max": int(counts[m].max()), "n_pairs": int(n), "mae": float(t[:, SAE].sum() / n), "r2": r2})
    return pd.DataFrame(rows, columns=DECILE_COLUMNS)


# ============================================================================ the reference's three functions
def create_per_lab_calibration_table(predictions, targets, lab_indices, lab_names, output_dir=None) -> pd.DataFrame:
    """advanced_visualizations.py:169-267 without the plot: per lab the least-squares line ``pred = a * true + b``, the
    MAE before and after applying it, their difference and ``is_calibrated = |a - 1| < 0.1 and |b| < 0.1``.  Labs with
    fewer than 2 pairs are left out; rows are sorted by ``mae_before``, descending; a lab whose targets are all equal
    gets ``a = 0, b = mean(pred)``.  Written as ``per_lab_calibration.csv`` (``%.4f``) when ``output_dir`` is given."""
    _, n, pred, target, lab, _, n_labs = _prepare(predictions, targets, lab_indices)
    if n == 0 or n_labs == 0:
        df = pd.DataFrame({c: [] for c in CALIBRATION_COLUMNS})
    else:
        lab_sums, _ = _first_read(pred, target, lab, n_labs, None, None, None)
        a, b = calibration_line(lab_sums)
        lab_abs, _ = _second_read(None, target, lab, *_line32(a, b), None, None, None, None)
        df = calibration_frame(lab_sums, lab_abs, a, b, lab_names)
    if output_dir is not None:
        _write_calibration(df, output_dir)
    return df


def _line32(a, b):
    """The line as the reference holds it (fp32 coefficients); labs without a pair get 0."""
    return (np.nan_to_num(a, nan=0.0, posinf=0.0, neginf=0.0).astype(np.float32),
            np.nan_to_num(b, nan=0.0, posinf=0.0, neginf=0.0).astype(np.float32))


def _write_calibration(df, output_dir):
    out = Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    df.to_csv(out / "per_lab_calibration.csv", index=False, float_format="%.4f")
    logging.info(f"  Saved calibration table to {out / 'per_lab_calibration.csv'}")


def create_error_vs_degree_table(predictions, targets, patient_indices, graph_data, bins: Sequence = DEFAULT_BINS,
                                 labels: Sequence[str] = DEFAULT_LABELS) -> pd.DataFrame:
    """advanced_visualizations.py:105-166 without the plot: mean, standard deviation (``ddof=1``: NaN for one sample) and
    count of ``|pred - true|`` per bin of the patient's has_lab degree, one row per bin, empty ones included
    (``NaN, NaN, 0``).  Bins are half open, ``[bins[j], bins[j + 1])``, as ``pd.cut(..., right=False)`` makes them.

    The reference's quirk is kept under the default arguments: the last edge is 50, so every pair of a patient with 50
    or more labs falls into NO bin and is dropped (on the x1 synthetic graph 194 patients and 9,700 of 61,484 pairs).
    Pass ``bins=(0, 1, 6, 16, np.inf)`` to keep them.  The number of pairs no bin took is logged at INFO.

    ``graph_data``: the graph (its has_lab edges give the degrees), a ``GraphPlan``, or the degrees themselves."""
    edges = _edges(bins, labels)
    _, n, pred, target, _, pat, _ = _prepare(predictions, targets, None, patient_indices, n_bins=len(edges) - 1)
    deg = patient_degrees(graph_data, pred.device if _is_dev(pred) else None)
    _, bin_sums = _first_read(pred, target, None, 0, pat, deg, edges)
    _, bin_sq = _second_read(pred, target, None, None, None, pat, deg, edges, bin_means(bin_sums))
    _log_dropped(n, bin_sums)
    return degree_frame(bin_sums, bin_sq, labels)


def _log_dropped(n, bin_sums):
    dropped = int(n - np.asarray(bin_sums)[:, 0].sum())
    logging.info(f"  error vs degree: {dropped} of {n} pairs fall into no degree bin")
    return dropped


def parity_by_frequency_decile(predictions, targets, lab_indices, lab_names=None) -> pd.DataFrame:
    """advanced_visualizations.py:32-102 without the scatter plots: the labs present in the pairs are cut into deciles of
    their pair count by ``pd.qcut(counts, 10, labels=False, duplicates='drop')``; one row per decile formed with the
    number of labs, the smallest and largest count, the pairs, their MAE and the reference's bare
    ``R^2 = 1 - SS_res / SS_tot`` (``-inf`` / ``nan`` for a decile of constant targets, as numpy gives)."""
    _, n, pred, target, lab, _, n_labs = _prepare(predictions, targets, lab_indices)
    if n == 0 or n_labs == 0:
        return decile_frame(np.zeros((0, 9)))
    lab_sums, _ = _first_read(pred, target, lab, n_labs, None, None, None)
    return decile_frame(lab_sums)


# ============================================================================ the driver
def analysis_tables(predictions, targets, patient_indices, lab_indices, graph_data, lab_names=None, n_labs=None,
                    bins: Sequence = DEFAULT_BINS, labels: Sequence[str] = DEFAULT_LABELS) -> Dict[str, pd.DataFrame]:
    """The three tables from ONE first and ONE second read of the pairs -> {"calibration", "error_vs_degree",
    "parity_by_decile"}."""
    edges = _edges(bins, labels)
    _, n, pred, target, lab, pat, n_labs = _prepare(predictions, targets, lab_indices, patient_indices, n_labs,
                                                    len(edges) - 1)
    deg = patient_degrees(graph_data, pred.device if _is_dev(pred) else None)
    if n_labs == 0:
        n_labs = 1                                           # no pair and no lab count given: one empty lab row, so that
        #                                                      the three (empty) frames come out of the usual assembly
    lab_sums, bin_sums = _first_read(pred, target, lab, n_labs, pat, deg, edges)
    a, b = calibration_line(lab_sums)
    lab_abs, bin_sq = _second_read(pred, target, lab, *_line32(a, b), pat, deg, edges, bin_means(bin_sums))
    _log_dropped(n, bin_sums)
    return {"calibration": calibration_frame(lab_sums, lab_abs, a, b, lab_names),
            "error_vs_degree": degree_frame(bin_sums, bin_sq, labels),
            "parity_by_decile": decile_frame(lab_sums)}


def run_analysis(model, graph, pairs=None, output_dir=None, lab_names=None):
    """What a driver of the reference's ``advanced_visualizations.main()`` calls instead: predicts the given pairs
    ``(patient_indices, lab_indices, targets)`` -- default: every has_lab edge with its ``edge_attr``, as the reference
    does, but WITHOUT its 10,000-pair sample --, runs the three tables from one first and one second read, writes
    ``per_lab_calibration.csv``, ``error_vs_degree.csv`` and ``parity_by_frequency_decile.csv`` into ``output_dir``
    (when given) and returns the three frames (calibration, error vs degree, parity by decile)."""
    if getattr(model, "_comm", None) is not None:
        raise NotImplementedError("run_analysis on a patient-sharded model (dist.shard_model) is not supported: the "
                                  "forward's collectives need every rank; analyse with an unsharded model")
    device = next(model.parameters()).device
    graph_dev = graph.to(device)
    if pairs is None:
        ei = graph_dev[LAB_EDGE].edge_index
        pi, li = ei[0].contiguous(), ei[1].contiguous()
        y = graph_dev[LAB_EDGE].edge_attr.reshape(-1).float().contiguous()
    else:
        pi, li, y = (torch.as_tensor(t).to(device).reshape(-1).contiguous() for t in pairs)
        y = y.float()
    if lab_names is None:
        meta = graph["lab"].metadata if "metadata" in graph["lab"] else None
        if meta:
            lab_names = {idx: m["label"] for idx, m in meta.items()}
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            pred = model.predict_lab_values(graph_dev, pi, li).reshape(-1).float().contiguous()
    finally:
        model.train(was_training)
    t = analysis_tables(pred, y, pi, li, graph_dev, lab_names, n_labs=int(graph["lab"].num_nodes))
    if output_dir is not None:
        out = Path(output_dir)
        _write_calibration(t["calibration"], out)
        t["error_vs_degree"].to_csv(out / "error_vs_degree.csv", index=False)
        t["parity_by_decile"].to_csv(out / "parity_by_frequency_decile.csv", index=False)
    return t["calibration"], t["error_vs_degree"], t["parity_by_decile"]
