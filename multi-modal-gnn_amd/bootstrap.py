"""Patient-cluster bootstrap intervals for the evaluation metrics: is "the GNN beats the per-lab mean by so much"
outside the noise, and for which labs?

``evaluate_model`` reports MAE / RMSE / R^2 / MAPE as bare point values.  A patient contributes about 33 correlated
pairs, so the resampling unit is the patient, not the pair (``cluster="pair"`` is the iid bootstrap, kept for comparison).
Replicate ``b`` multiplies every pair of unit ``u`` by an integer weight; the metrics of a replicate are those of the
weighted sample; the interval is the percentile interval of the replicates.  DESIGN.md section 5, "Metric intervals".

Definitions (this module's numpy functions are the definition; ``tests/boot_ref.py`` restates them with loops):

* weights: ``k_b = key(seed, SITE_BOOT + b)``, ``w0`` = the first word of the project's counter-based RNG group hash of
  ``(k_b, u >> 1)``, ``field = w0 >> 16 if u & 1 else w0 & 0xFFFF``, ``w = #{j: field >= T[j]}`` with
  ``T[j] = round(65536 * PoissonCDF(j; 1))``: Poisson(1) on a 16-bit grid, mean exactly 1.  Replicate 0 is the sample
  itself (every weight 1).
* sums: per replicate and segment the sum of ``w * term`` over the seven additive terms of ``ops.seg_sums`` (ten with a
  second predictor on the same pairs), each term formed as ``k_seg_metrics`` forms it.  A pair is left out of every
  replicate, and counted, under the first of: segment out of range, unit out of range, a NaN value.  Every weighted term is
  exact in float64; the order of the additions is fixed: pairs in segment order (stable), cut into chunks of
  ``BOOT_CHUNK`` sorted pairs, left to right from 0 inside a chunk, chunk partials in chunk order.
* metrics: ``evaluate.metrics_from_sums`` per (replicate, segment) and for all segments together (sums added in segment
  order); with a second predictor also its four metrics and the paired differences.
* summary: over the finite replicates 1 .. B: mean, standard deviation (ddof = 1), numpy's "linear" percentiles at
  ``100 * (1 -+ confidence) / 2``, their number, the share below zero.

HIP tensors run the kernels of libmmgnn_boot.so (csrc/boot.hip); numpy inputs run the float64 restatement below, which is
the checker and never a silent substitute for the kernels.
"""
from __future__ import annotations

import json
import logging
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, Optional, Sequence

import numpy as np
import pandas as pd
import torch

SITE_BOOT = 0x424F4F54
THRESHOLDS = (24109, 48219, 60273, 64292, 65296, 65497, 65531, 65535)       # round(65536 * PoissonCDF(j; 1))
BOOT_CHUNK = 4096                     # MMG_BOOT_CHUNK of include/mmgnn_boot.h (tests check the two against each other)
MAX_REPLICATES = 4096
MAX_SEGMENTS = 2048
FIELDS = ("n", "sum_abs", "sum_sq", "sum_t", "sum_t2", "sum_ape", "n_nonzero")
FIELDS_B = FIELDS + ("sum_abs_b", "sum_sq_b", "sum_ape_b")
METRICS = ("mae", "rmse", "r2", "mape")
SUMMARY_FIELDS = ("estimate", "mean", "std_error", "lower", "upper", "n_finite", "p_below_zero")
DROP_KINDS = ("segment_out_of_range", "unit_out_of_range", "nan_value")
COLUMNS = ["metric", "estimate", "lower", "upper", "std_error", "n_finite"]
_U32 = np.uint32
_M32, _M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def _is_dev(x) -> bool:
    return torch.is_tensor(x) and x.is_cuda


def _host(x):
    return np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x)


# ============================================================================ the numpy restatement
def _mix32_int(h: int) -> int:
    h &= _M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & _M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def _mix32(h):
    h = h ^ (h >> _U32(16))
    h = h * _U32(0x85EBCA6B)
    h = h ^ (h >> _U32(13))
    h = h * _U32(0xC2B2AE35)
    return h ^ (h >> _U32(16))


def _key(seed: int, site: int) -> int:
    """mmg_rng_key of csrc/common.h."""
    seed, site = int(seed) & _M64, int(site) & _M32
    h = _mix32_int((seed & _M32) ^ 0x9E3779B9)
    return _mix32_int(h ^ (seed >> 32) ^ ((site * 0x632BE5AB) & _M32))


def poisson_weights(seed: int, n_units: int, replicates: int, first: int = 0) -> np.ndarray:
    """The bootstrap weights, int8 [replicates + 1, n_units]: row 0 is the sample itself, row b replicate b.
    first > 0: rows first .. replicates only (the host sums walk the replicates in blocks)."""
    n_units, replicates = int(n_units), int(replicates)
    if not 0 <= n_units < 2 ** 31:
        raise ValueError(f"poisson_weights: {n_units} units outside [0, 2^31)")
    return _weights_at(seed, np.arange(n_units, dtype=_U32), int(first), replicates)


def _weights_at(seed: int, units: np.ndarray, first: int, last: int) -> np.ndarray:
    """int8 [last - first + 1, len(units)]: the weights replicates first .. last give the listed units (below 2^31, so
    the high half of the 64-bit group index u >> 1 is 0)."""
    units = np.asarray(units).astype(_U32)
    rows = range(int(first), int(last) + 1)
    out = np.ones((len(rows), units.size), np.int8)
    grp, shift = units >> _U32(1), (units & _U32(1)) * _U32(16)
    T = np.asarray(THRESHOLDS, _U32)
    for i, b in enumerate(rows):
        if b == 0:
            continue
        w0 = _mix32(_U32(_key(seed, SITE_BOOT + b)) ^ grp)
        out[i] = np.searchsorted(T, (w0 >> shift) & _U32(0xFFFF), side="right").astype(np.int8)     # #{j: field >= T[j]}
    return out


def host_terms(pred, target, pred_b=None) -> np.ndarray:
    """float64 [n, F]: the additive terms of every pair, formed as k_seg_metrics forms them."""
    p, t = np.asarray(pred, np.float32).reshape(-1), np.asarray(target, np.float32).reshape(-1)
    nz = t != 0
    t64 = t.astype(np.float64)
    cols = [np.ones(t.size), None, None, t64, t64 * t64, None, nz.astype(np.float64)]

    def three(q):
        with np.errstate(all="ignore"):
            e = t - q                                             # fp32
            ape = np.where(nz, np.abs(e / np.where(nz, t, np.float32(1))), np.float32(0))
        e64 = e.astype(np.float64)
        return np.abs(e).astype(np.float64), e64 * e64, ape.astype(np.float64)

    cols[1], cols[2], cols[5] = three(p)
    if pred_b is not None:
        cols += list(three(np.asarray(pred_b, np.float32).reshape(-1)))
    return np.stack(cols, axis=1) if t.size else np.zeros((0, len(cols)))


def host_sums(pred, target, unit, seg, n_units: int, n_seg: int, replicates: int, seed: int = 0, pred_b=None,
              chunk: int = BOOT_CHUNK, rep_block: int = 64):
    """mmg_boot_sums in numpy -> (sums float64 [replicates + 1, n_seg, F], dropped int64 [3]), in the documented order."""
    _check_shape(n_seg, replicates)
    terms = host_terms(pred, target, pred_b)
    n, F = terms.shape
    unit, seg = _host(unit).reshape(-1).astype(np.int64), _host(seg).reshape(-1).astype(np.int64)
    if unit.size != n or seg.size != n:
        raise ValueError("host_sums: pred, target, unit and seg need the same length")
    bad_s = (seg < 0) | (seg >= n_seg)
    bad_u = (unit < 0) | (unit >= n_units)
    bad_v = np.isnan(terms[:, 1]) | np.isnan(terms[:, 3]) | (np.isnan(terms[:, 7]) if F > 7 else False)
    dropped = np.array([bad_s.sum(), (~bad_s & bad_u).sum(), (~bad_s & ~bad_u & bad_v).sum()], np.int64)
    keep = np.flatnonzero(~(bad_s | bad_u | bad_v))
    order = keep[np.argsort(seg[keep], kind="stable")]
    K, X = seg[order], terms[order]
    present, U = np.unique(unit[order], return_inverse=True)      # the weights of the units that occur, no others
    m = K.size
    cuts = np.flatnonzero(np.concatenate(([True], K[1:] != K[:-1]))) if m else np.empty(0, np.int64)
    cuts = np.union1d(cuts, np.arange(0, m, chunk)).astype(np.int64)
    ends = np.concatenate((cuts[1:], [m])).astype(np.int64)
    sums = np.zeros((replicates + 1, n_seg, F))
    for r0 in range(0, replicates + 1, rep_block):
        r1 = min(r0 + rep_block, replicates + 1)
        W = _weights_at(seed, present, r0, r1 - 1)
        for a, b in zip(cuts.tolist(), ends.tolist()):
            wt = W[:, U[a:b]].astype(np.float64)[:, :, None] * X[None, a:b, :]         # every product exact
            sums[r0:r1, K[a]] = sums[r0:r1, K[a]] + np.cumsum(wt, axis=1)[:, -1]       # left to right, chunk after chunk
    return sums, dropped


def host_metrics(sums) -> np.ndarray:
    """mmg_boot_metrics in numpy: evaluate.metrics_from_sums per (replicate, row); row n_seg is all segments together."""
    sums = np.asarray(sums, np.float64)
    F = sums.shape[2]
    total = (np.cumsum(sums, axis=1)[:, -1:] + 0.0) if sums.shape[1] else np.zeros((sums.shape[0], 1, F))
    s = np.concatenate((sums, total), axis=1)

    def four(n, s_abs, s_sq, s_t, s_t2, s_ape, n_nz):
        with np.errstate(all="ignore"):
            ok = n > 0
            ss_tot = s_t2 - s_t * s_t / n
            r2 = np.where(ss_tot > 1e-12 * np.maximum(s_t2, 1e-300), 1.0 - s_sq / ss_tot, 0.0)
            r2 = np.where(s_sq == 0, 1.0, r2)
            r2 = np.where(n < 2, np.nan, r2)
            mape = np.where(n_nz > 0, s_ape / n_nz * 100.0, np.nan)
            out = np.stack([s_abs / n, np.sqrt(s_sq / n), r2, mape], axis=-1)
        return np.where(ok[..., None], out, np.nan)

    m = four(*(s[..., i] for i in range(7)))
    if F == len(FIELDS):
        return m
    mb = four(s[..., 0], s[..., 7], s[..., 8], s[..., 3], s[..., 4], s[..., 9], s[..., 6])
    with np.errstate(all="ignore"):
        return np.concatenate((m, mb, m - mb), axis=-1)


def _quantiles(confidence: float):
    if not 0.0 < float(confidence) < 1.0:
        raise ValueError(f"confidence {confidence} outside (0, 1)")
    c = float(confidence)
    return (1.0 - c) / 2.0 * 100.0, (1.0 + c) / 2.0 * 100.0             # the p of numpy.percentile(x, p)


def host_percentile(xs: np.ndarray, p: float) -> float:
    """numpy.percentile(x, p) under the "linear" rule for ascending xs, in the form mmg_boot_summary documents."""
    m, q = xs.size, p / 100.0
    v = (m - 1) * q
    if v >= m - 1:
        return float(xs[m - 1])
    if v < 0:
        return float(xs[0])
    i = int(np.floor(v))
    g, a, b = v - i, float(xs[i]), float(xs[i + 1])
    d = b - a
    return b - d * (1.0 - g) if g >= 0.5 else a + d * g


def host_summary(metrics, confidence: float = 0.95) -> np.ndarray:
    """mmg_boot_summary in numpy -> float64 [rows, M, 7] (SUMMARY_FIELDS).  The mean and the standard deviation are
    numpy's: their summation order is not the device's, which agrees within (B + 8) ulp-sums (tests)."""
    metrics = np.asarray(metrics, np.float64)
    p_lo, p_hi = _quantiles(confidence)
    _, rows, M = metrics.shape
    out = np.full((rows, M, len(SUMMARY_FIELDS)), np.nan)
    for r in range(rows):
        for k in range(M):
            x = metrics[1:, r, k]
            x = x[np.isfinite(x)]
            out[r, k, 0], out[r, k, 5] = metrics[0, r, k], x.size
            if x.size:
                out[r, k, 1] = x.mean()
                out[r, k, 2] = x.std(ddof=1) if x.size > 1 else np.nan
                x = np.sort(x)
                out[r, k, 3], out[r, k, 4] = host_percentile(x, p_lo), host_percentile(x, p_hi)
                out[r, k, 6] = np.count_nonzero(x < 0) / x.size
    return out


def _check_shape(n_seg: int, replicates: int):
    if not 1 <= int(replicates) <= MAX_REPLICATES:
        raise ValueError(f"{replicates} replicates outside [1, {MAX_REPLICATES}]")
    if not 1 <= int(n_seg) <= MAX_SEGMENTS:
        raise ValueError(f"{n_seg} segments outside [1, {MAX_SEGMENTS}]")


# ============================================================================ the three steps, device or host
def bootstrap_sums(pred, target, unit, seg, n_units: int, n_seg: int, replicates: int = 1000, seed: int = 0, pred_b=None):
    """-> (sums float64 [replicates + 1, n_seg, 7 or 10], dropped int64 [3]).  HIP tensors: mmg_boot_sums (unit and seg
    both int64 or both int32); numpy arrays: the restatement.  Mixing the two is refused."""
    given = [x for x in (pred, target, unit, seg, pred_b) if x is not None]
    if any(_is_dev(x) for x in given):
        if not all(_is_dev(x) for x in given):
            raise TypeError("bootstrap_sums: every input on the HIP device, or none (no silent host fallback)")
        from . import boot_ops
        f32 = lambda x: x.reshape(-1).to(torch.float32).contiguous()      # noqa: E731
        return boot_ops.boot_sums(f32(pred), f32(target), unit.reshape(-1).contiguous(), seg.reshape(-1).contiguous(),
                                  n_units, n_seg, replicates, seed, None if pred_b is None else f32(pred_b))
    return host_sums(_host(pred), _host(target), unit, seg, n_units, n_seg, replicates, seed,
                     None if pred_b is None else _host(pred_b))


def bootstrap_metrics_from_sums(sums):
    """sums -> metrics float64 [replicates + 1, n_seg + 1, 4 or 12]; row n_seg: all segments together."""
    if _is_dev(sums):
        from . import boot_ops
        return boot_ops.boot_metrics(sums.contiguous())
    return host_metrics(_host(sums))


def bootstrap_summary(metrics, confidence: float = 0.95):
    """metrics -> summary float64 [n_seg + 1, M, 7]: SUMMARY_FIELDS."""
    if _is_dev(metrics):
        from . import boot_ops
        return boot_ops.boot_summary(metrics.contiguous(), confidence)
    return host_summary(_host(metrics), confidence)


# ============================================================================ the report
@dataclass
class BootstrapResult:
    overall: pd.DataFrame
    per_lab: pd.DataFrame
    strata: pd.DataFrame
    comparison: Optional[pd.DataFrame]
    replicates: int
    confidence: float
    seed: int
    cluster: str
    num_capped: int = 0
    dropped: Dict[str, int] = field(default_factory=dict)


def _rows(summary_row, names=METRICS, extra=None, offset=0, with_p=False):
    out = []
    for k, name in enumerate(names):
        est, _, se, lo, hi, nf, pb = (float(v) for v in summary_row[offset + k])
        row = dict(extra or {}, metric=name, estimate=est, lower=lo, upper=hi, std_error=se, n_finite=int(nf))
        if with_p:
            row["p_below_zero"] = pb
        out.append(row)
    return out


def _degree_segments(patient_indices, lab_indices, graph, dev):
    """The two stratifications of evaluate.device_evaluate as segment ids (int64; -1: in no group) and their labels."""
    ei = graph["patient", "has_lab", "lab"].edge_index
    n_labs = int(graph["lab"].num_nodes)
    if dev is not None:
        deg = torch.bincount(ei[0].to(dev), minlength=int(graph["patient"].num_nodes))[patient_indices]
        s_deg = torch.full_like(deg, -1)
        s_deg[(deg >= 1) & (deg <= 5)] = 0
        s_deg[(deg >= 6) & (deg <= 15)] = 1
        s_deg[deg >= 16] = 2
        counts = torch.bincount(ei[1].to(dev), minlength=n_labs)
        cn = counts.cpu().numpy()
        q25, q75 = np.percentile(cn[cn > 0], 25), np.percentile(cn[cn > 0], 75)
        f = counts[lab_indices].double()
        s_frq = torch.ones_like(lab_indices)
        s_frq[f < q25] = 0
        s_frq[f > q75] = 2
    else:
        e = _host(ei)
        deg = np.bincount(e[0], minlength=int(graph["patient"].num_nodes))[patient_indices]
        s_deg = np.where((deg >= 1) & (deg <= 5), 0, np.where((deg >= 6) & (deg <= 15), 1, np.where(deg >= 16, 2, -1)))
        cn = np.bincount(e[1], minlength=n_labs)
        q25, q75 = np.percentile(cn[cn > 0], 25), np.percentile(cn[cn > 0], 75)
        f = cn[lab_indices].astype(np.float64)
        s_frq = np.where(f < q25, 0, np.where(f > q75, 2, 1))
    return {"num_labs": ("by_patient_degree", s_deg, ("low (1-5 labs)", "medium (6-15 labs)", "high (16+ labs)")),
            "lab_frequency": ("by_lab_frequency", s_frq, ("rare (bottom 25%)", "common (middle 50%)",
                                                          "very common (top 25%)"))}


def bootstrap_metrics(predictions, targets, patient_indices, lab_indices, graph, replicates: int = 1000,
                      confidence: float = 0.95, seed: int = 0, cluster: str = "patient", baseline=None,
                      stratify: Sequence[str] = (), n_sigma: float = 3.0, lab_names=None) -> BootstrapResult:
    """Percentile bootstrap intervals of everything ``evaluate.device_evaluate`` reports: ``overall``, ``per_lab`` (labs
    with at least two pairs) and ``strata`` (``stratify``: "num_labs", "lab_frequency"; same labels), each with the
    columns ``metric, estimate, lower, upper, std_error, n_finite``; with ``baseline`` (a second predictor on the same
    pairs) also ``comparison``: the paired differences ``model - baseline`` overall and per lab, with ``p_below_zero``,
    the share of replicates in which the model's metric is the smaller one.

    cluster="patient" resamples patients (the pairs of one patient are not independent), "pair" is the iid bootstrap.
    The per-lab +-``n_sigma`` winsorisation of the model's residuals is applied ONCE, on the full sample
    (``ops.seg_sums(..., want_adjusted=True)``, as evaluate_model applies it); its bounds are NOT re-drawn per replicate, so
    the intervals are conditional on them.  The baseline is not winsorised, as in ``evaluate_baselines``.
    HIP tensors run the kernels; numpy arrays the float64 restatement."""
    from .analysis import _lab_name
    if cluster not in ("patient", "pair"):
        raise ValueError(f"cluster must be 'patient' or 'pair', got {cluster!r}")
    _quantiles(confidence)
    n_labs, n_pat = int(graph["lab"].num_nodes), int(graph["patient"].num_nodes)
    dev = predictions.device if _is_dev(predictions) else None
    num_capped = 0
    if dev is not None:
        from . import ops
        pred = predictions.reshape(-1).to(torch.float32).contiguous()
        tgt = targets.to(dev).reshape(-1).to(torch.float32).contiguous()
        pi = patient_indices.to(dev).reshape(-1).to(torch.int64).contiguous()
        li = lab_indices.to(dev).reshape(-1).to(torch.int64).contiguous()
        base = None if baseline is None else torch.as_tensor(baseline).to(dev).reshape(-1).to(torch.float32).contiguous()
        if n_sigma > 0:
            s8, pred = ops.seg_sums(pred, tgt, li, n_labs, n_sigma, want_adjusted=True)
            num_capped = int(round(float(s8[:, 7].sum())))
        unit = pi if cluster == "patient" else torch.arange(pred.numel(), dtype=torch.int64, device=dev)
    else:
        from .evaluate import winsorize_residuals
        pred, tgt = _host(predictions).reshape(-1).astype(np.float32), _host(targets).reshape(-1).astype(np.float32)
        pi, li = _host(patient_indices).reshape(-1).astype(np.int64), _host(lab_indices).reshape(-1).astype(np.int64)
        base = None if baseline is None else _host(baseline).reshape(-1).astype(np.float32)
        if n_sigma > 0:
            pred, num_capped = winsorize_residuals(pred, tgt, li, n_sigma)
        unit = pi if cluster == "patient" else np.arange(pred.size, dtype=np.int64)
    n_units = n_pat if cluster == "patient" else int(pred.shape[0])

    def run(seg, n_seg):
        sums, dropped = bootstrap_sums(pred, tgt, unit, seg, n_units, n_seg, replicates, seed, base)
        summary = bootstrap_summary(bootstrap_metrics_from_sums(sums), confidence)
        return _host(sums[0]), _host(summary), _host(dropped)

    s0, summ, dropped = run(li, n_labs)
    overall = pd.DataFrame(_rows(summ[n_labs]), columns=COLUMNS)
    lab_rows, cmp_rows = [], []
    if base is not None:
        cmp_rows += _rows(summ[n_labs], extra={"scope": "overall", "lab_index": -1}, offset=8, with_p=True)
    for j in range(n_labs):
        if s0[j, 0] < 2:
            continue
        extra = {"lab_index": j, "lab_name": _lab_name(lab_names, j), "num_samples": int(s0[j, 0])}
        lab_rows += _rows(summ[j], extra=extra)
        if base is not None:
            cmp_rows += _rows(summ[j], extra={"scope": extra["lab_name"], "lab_index": j}, offset=8, with_p=True)
    per_lab = pd.DataFrame(lab_rows, columns=["lab_index", "lab_name", "num_samples"] + COLUMNS)
    strata_rows = []
    if stratify:
        table = _degree_segments(pi, li, graph, dev)
        for name in stratify:
            if name not in table:
                continue
            title, seg, labels = table[name]
            g0, gs, _ = run(seg if dev is None else seg.contiguous(), 3)
            for i, label in enumerate(labels):
                if g0[i, 0] > 0:
                    strata_rows += _rows(gs[i], extra={"stratification": title, "group": label,
                                                       "num_samples": int(g0[i, 0])})
    strata = pd.DataFrame(strata_rows, columns=["stratification", "group", "num_samples"] + COLUMNS)
    comparison = None
    if base is not None:
        comparison = pd.DataFrame(cmp_rows, columns=["scope", "lab_index"] + COLUMNS + ["p_below_zero"])
    return BootstrapResult(overall, per_lab, strata, comparison, int(replicates), float(confidence), int(seed), cluster,
                           num_capped, {k: int(v) for k, v in zip(DROP_KINDS, dropped.tolist())})


@torch.no_grad()
def evaluate_with_intervals(model, graph, masker, config: Dict, output_dir, split: str = "test", replicates: int = 1000,
                            baselines: Sequence[str] = ("global_mean", "per_lab_mean"), confidence: float = 0.95,
                            seed: int = 0) -> Dict:
    """Predict the ``split`` pairs of ``masker``, fit the named baselines ("global_mean", "per_lab_mean",
    "nearest_neighbor": mmgnn.knn.KNNLabImputer, "chained_equations": mmgnn.chained.ChainedLabImputer) on its train
    edges and bootstrap the model's metrics and every paired
    difference ``model - baseline`` over patients.  Writes ``evaluation_intervals.json``, ``per_lab_metrics_ci.csv`` and
    ``baseline_comparison.csv`` (one row per baseline x metric x scope) into ``output_dir``; ``evaluate_model`` and its
    files are untouched."""
    from .evaluate import BASELINES, baseline_pairs, fit_baselines
    for b in baselines:
        if b not in BASELINES:
            raise ValueError(f"unknown baseline {b!r}: one of {BASELINES}")
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    model.eval()
    dev = next(model.parameters()).device
    graph = graph.to(dev)
    tr_ei, tr_v, _, _ = masker.get_masked_data("train", want_mask=False)
    ev_ei, ev_v, _, _ = masker.get_masked_data(split, want_mask=False)
    tr_ei, tr_v, ev_ei = tr_ei.to(dev), tr_v.to(dev).reshape(-1).float(), ev_ei.to(dev)
    ev_v = ev_v.to(dev).reshape(-1).float()
    pi, li = ev_ei[0].contiguous(), ev_ei[1].contiguous()
    n_labs, n_pat = int(graph["lab"].num_nodes), int(graph["patient"].num_nodes)
    pred = model.predict_lab_values(graph, pi, li)
    lab_store = graph["lab"]
    meta = getattr(lab_store, "metadata", None) if "metadata" in lab_store else None
    lab_names = {idx: m["label"] for idx, m in meta.items()} if meta else None
    stratify = tuple((config.get("evaluation") or {}).get("stratify_by") or ())

    nn = (config.get("evaluation") or {}).get("n_neighbors", 5)
    models = fit_baselines(tuple(baselines), tr_ei, tr_v, n_labs, n_pat, nn)
    fitted = {b: baseline_pairs(m, pi, li) for b, m in models.items()}

    kw = dict(replicates=replicates, confidence=confidence, seed=seed, cluster="patient", lab_names=lab_names)
    res = bootstrap_metrics(pred, ev_v, pi, li, graph, stratify=stratify, **kw)
    frames = []
    for b, bp in fitted.items():
        c = bootstrap_metrics(pred, ev_v, pi, li, graph, baseline=bp, **kw).comparison
        c.insert(0, "baseline", b)
        frames.append(c)
    comparison = pd.concat(frames, ignore_index=True) if frames else pd.DataFrame(
        columns=["baseline", "scope", "lab_index"] + COLUMNS + ["p_below_zero"])
    res.per_lab.to_csv(output_dir / "per_lab_metrics_ci.csv", index=False)
    comparison.to_csv(output_dir / "baseline_comparison.csv", index=False)

    def records(df):
        return json.loads(df.to_json(orient="records"))
    out = {"split": split, "num_samples": int(pred.numel()), "replicates": int(replicates), "confidence": float(confidence),
           "seed": int(seed), "cluster": "patient", "num_capped": res.num_capped, "dropped": res.dropped,
           "overall": records(res.overall), "strata": records(res.strata),
           "baseline_comparison": records(comparison[comparison["scope"] == "overall"])}
    with open(output_dir / "evaluation_intervals.json", "w") as f:
        json.dump(out, f, indent=2)
    mae = res.overall.set_index("metric").loc["mae"]
    logging.info(f"MAE {mae['estimate']:.4f} [{mae['lower']:.4f}, {mae['upper']:.4f}] ({replicates} patient replicates)")
    return out
