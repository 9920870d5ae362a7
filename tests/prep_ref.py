"""numpy / pandas restatement of the lab preprocessing semantics (the checker of mmgnn.preprocess, as audit_ref.py is
the audit's), plus the high-precision evaluation the sum-type results are judged against.

Semantics (reference src/preprocess.py:28-164, src/utils.py:309-481):
  cohort filter -> per-lab outlier removal over all remaining events -> rows with NaN dropped (only with removal on)
  -> one value per (patient, lab) -> per-lab normalisation -> NaN rows dropped -> rows in (lab, patient) order.
Per-lab statistics use the same pandas Series reductions the reference calls, so that on one machine the restatement
and the reference agree to the bit; the device path is compared with tolerances only where sums are involved.
"""
import decimal

import numpy as np
import pandas as pd

AGGS = ("last", "mean", "median", "min", "max")
NORMS = ("zscore", "minmax", "robust")


# ------------------------------------------------------------------------------------------ restatement
def outlier_bounds(values: pd.Series, method: str, threshold: float):
    if method == "std":
        mean, std = values.mean(), values.std()
        return mean - threshold * std, mean + threshold * std
    if method == "iqr":
        q25, q75 = values.quantile(0.25), values.quantile(0.75)
        iqr = q75 - q25
        return q25 - threshold * iqr, q75 + threshold * iqr
    raise ValueError(f"Unknown outlier detection method: {method}")


def remove_outliers(values, method="std", threshold=5.0) -> np.ndarray:
    s = pd.Series(np.asarray(values, dtype=np.float64))
    lo, hi = outlier_bounds(s, method, threshold)
    out = s.to_numpy().copy()
    with np.errstate(invalid="ignore"):
        out[(out < lo) | (out > hi)] = np.nan
    return out


def bound_margin(values, method="std", threshold=5.0) -> float:
    """Smallest |v - bound| / |bound| over the finite values and both bounds (inf when the bounds are NaN)."""
    s = pd.Series(np.asarray(values, dtype=np.float64))
    lo, hi = outlier_bounds(s, method, threshold)
    v = s.to_numpy()
    v = v[np.isfinite(v)]
    if not (np.isfinite(lo) and np.isfinite(hi)) or v.size == 0:
        return np.inf
    return float(min(np.min(np.abs(v - lo)) / max(abs(lo), 1e-300), np.min(np.abs(v - hi)) / max(abs(hi), 1e-300)))


def clean_events(labs: pd.DataFrame, cohort_ids, remove: bool, threshold: float = 5.0) -> pd.DataFrame:
    """Cohort filter and outlier removal; the surviving rows in input order."""
    labs = labs[labs["SUBJECT_ID"].isin(np.asarray(cohort_ids))].copy()
    if not remove:
        return labs
    v = labs["VALUENUM"].to_numpy(dtype=np.float64).copy()
    for _, idx in labs.groupby("ITEMID").indices.items():
        v[idx] = remove_outliers(v[idx], "std", threshold)
    labs["VALUENUM"] = v
    return labs[~np.isnan(v)]


def _time_key(col: pd.Series) -> np.ndarray:
    if pd.api.types.is_datetime64_any_dtype(col):
        t = col.to_numpy(dtype="datetime64[ns]").view(np.int64).astype(np.float64)
        t[col.isna().to_numpy()] = np.inf
        return t
    t = col.to_numpy(dtype=np.float64).copy()
    t[np.isnan(t)] = np.inf                                    # a missing time sorts after every time
    return t


def aggregate(labs: pd.DataFrame, cohort: pd.DataFrame, method="last", remove=True, threshold=5.0) -> pd.DataFrame:
    """-> SUBJECT_ID, ITEMID, VALUE sorted by (SUBJECT_ID, ITEMID), fresh index."""
    if method not in AGGS:
        raise ValueError(f"Unknown aggregation method: {method}")
    ev = clean_events(labs, cohort["SUBJECT_ID"].unique(), remove, threshold)
    if method == "last":
        pc, _ = pd.factorize(ev["SUBJECT_ID"], sort=True)
        lc, _ = pd.factorize(ev["ITEMID"], sort=True)
        order = np.lexsort((_time_key(ev["CHARTTIME"]), lc, pc))            # stable: ties keep the input order
        s = ev.iloc[order]
        pcs, lcs = pc[order], lc[order]
        last = np.ones(len(s), bool)
        last[:-1] = (pcs[1:] != pcs[:-1]) | (lcs[1:] != lcs[:-1])
        out = s.loc[last, ["SUBJECT_ID", "ITEMID", "VALUENUM"]]
    else:
        out = ev.groupby(["SUBJECT_ID", "ITEMID"])["VALUENUM"].agg(method).reset_index()
    return out.rename(columns={"VALUENUM": "VALUE"}).reset_index(drop=True)


def fit_stats(values: pd.Series, method: str):
    clean = values.dropna()
    if len(clean) == 0:
        return None
    if method == "zscore":
        return {"mean": clean.mean(), "std": clean.std()}
    if method == "minmax":
        return {"min": clean.min(), "max": clean.max()}
    if method == "robust":
        return {"median": clean.median(), "q25": clean.quantile(0.25), "q75": clean.quantile(0.75)}
    raise ValueError(f"Unknown normalization method: {method}")


def location_spread(st, method):
    if method == "zscore":
        return st["mean"], st["std"]
    if method == "minmax":
        return st["min"], st["max"] - st["min"]
    return st["median"], st["q75"] - st["q25"]


def transform(v: np.ndarray, st, method: str) -> np.ndarray:
    if st is None:
        return v
    loc, spread = location_spread(st, method)
    degenerate = spread == 0 or np.isnan(spread)
    if method == "minmax":
        return v * 0 if degenerate else (v - loc) / spread
    return v - loc if degenerate else (v - loc) / spread


def inverse(v: np.ndarray, st, method: str) -> np.ndarray:
    if st is None:
        return v
    loc, spread = location_spread(st, method)
    return v * spread + loc


def normalize(labs_agg: pd.DataFrame, method="zscore"):
    """-> (frame with VALUE_NORMALIZED, rows by lab key then input order, NaN rows dropped; stats dict by str(lab))."""
    if method not in NORMS:
        raise ValueError(f"Unknown normalization method: {method}")
    lc, keys = pd.factorize(labs_agg["ITEMID"], sort=True)
    order = np.argsort(lc, kind="stable")
    order = order[lc[order] >= 0]
    out = labs_agg.iloc[order].reset_index(drop=True)
    v = out["VALUE"].to_numpy(dtype=np.float64)
    vn = np.empty_like(v)
    stats = {}
    lcs = lc[order]
    starts = np.searchsorted(lcs, np.arange(len(keys) + 1))
    for k, key in enumerate(keys):
        a, b = starts[k], starts[k + 1]
        st = fit_stats(pd.Series(v[a:b]), method)
        stats[str(key)] = st
        vn[a:b] = transform(v[a:b], st, method)
    out["VALUE_NORMALIZED"] = vn
    out = out[~np.isnan(vn)].copy()
    out["SUBJECT_ID"] = out["SUBJECT_ID"].astype("int64")
    try:
        out["ITEMID"] = out["ITEMID"].astype("int64")
    except (ValueError, TypeError):
        pass
    return out, stats


# ------------------------------------------------------------------------------------------ high-precision evaluation
# The "exact" side of the tolerance: the same formulas in a precision whose own error is far below fp64's.  With an
# 80-bit long double (x86) every operation carries 11 more bits than fp64 and the pairwise sums stay ~1e-3 of an fp64
# ulp for the sizes used here; elsewhere the evaluation falls back to 60-digit decimals.
_LD = np.longdouble
_HAVE_LD = np.finfo(_LD).nmant >= 63


def exact_mean_std(values: np.ndarray):
    """(mean, std ddof 1) of the non-NaN values, as high-precision numbers (std NaN for fewer than two)."""
    v = np.asarray(values, dtype=np.float64)
    v = v[~np.isnan(v)]
    n = len(v)
    if n == 0:
        return _LD("nan"), _LD("nan")
    if _HAVE_LD:
        x = v.astype(_LD)
        mean = x.sum() / _LD(n)
        if n < 2:
            return mean, _LD("nan")
        d = x - mean
        return mean, np.sqrt((d * d).sum() / _LD(n - 1))
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        x = [decimal.Decimal(float(t)) for t in v]
        mean = sum(x) / n
        if n < 2:
            return _LD(float(mean)), _LD("nan")
        var = sum((t - mean) ** 2 for t in x) / (n - 1)
        return _LD(float(mean)), _LD(float(var.sqrt()))


def sum_deviations(lab_codes: np.ndarray, values: np.ndarray, got_mean=None, got_std=None, got_z=None) -> float:
    """Largest condition-scaled deviation of per-lab zscore results from the high-precision evaluation.

    lab_codes / values: the aggregated pairs (values finite or NaN); got_mean / got_std: per lab code (dict);
    got_z: per pair.  Scales: a mean's error is relative to the largest |summand| (a sum's rounding error does not
    shrink when the terms cancel); a std's to the std; a z-score z = (v - mean) / std inherits the mean's error
    divided by std and the std's error times |z|, so it is scaled by max|v| / std + |z| (by max|v| when the spread is
    degenerate and z = v - mean)."""
    worst = 0.0
    for k in np.unique(lab_codes):
        sel = lab_codes == k
        v = values[sel]
        ok = ~np.isnan(v)
        if not ok.any():
            continue
        mean, std = exact_mean_std(v)
        vmax = float(np.max(np.abs(v[ok]))) or 1.0
        if got_mean is not None:
            worst = max(worst, float(abs(_LD(got_mean[k]) - mean)) / vmax)
        if got_std is not None and np.isfinite(float(std)) and float(std) > 0:
            worst = max(worst, float(abs(_LD(got_std[k]) - std) / std))
        if got_z is not None:
            z = got_z[sel][ok]
            x = v[ok].astype(_LD)
            if np.isfinite(float(std)) and float(std) > 0:
                zx = (x - mean) / std
                scale = _LD(vmax) / std + np.abs(zx)
            else:
                zx = x - mean
                scale = _LD(vmax)
            worst = max(worst, float(np.max(np.abs(z.astype(_LD) - zx) / scale)))
    return worst


def mean_agg_deviation(ev: pd.DataFrame, agg: pd.DataFrame) -> float:
    """Largest deviation of a "mean" aggregation from the high-precision mean of each pair's surviving values,
    relative to the pair's largest |value|.  ev: clean_events' rows; agg: SUBJECT_ID, ITEMID, VALUE."""
    if len(ev) == 0:
        return 0.0
    pk = np.unique(ev["SUBJECT_ID"].to_numpy())
    lc, lk = pd.factorize(ev["ITEMID"], sort=True)
    code = np.searchsorted(pk, ev["SUBJECT_ID"].to_numpy()) * len(lk) + lc
    order = np.argsort(code, kind="stable")
    code = code[order]
    v = ev["VALUENUM"].to_numpy(dtype=np.float64)[order]
    ok = ~np.isnan(v)
    heads = np.flatnonzero(np.r_[True, code[1:] != code[:-1]])
    x = np.where(ok, v, 0.0).astype(_LD if _HAVE_LD else np.float64)
    cnt = np.add.reduceat(ok.astype(np.int64), heads)
    sums = np.add.reduceat(x, heads)
    vmax = np.maximum.reduceat(np.where(ok, np.abs(v), 0.0), heads)
    acode = np.searchsorted(pk, agg["SUBJECT_ID"].to_numpy()) * len(lk) + pd.Index(lk).get_indexer(agg["ITEMID"])
    at = np.searchsorted(code[heads], acode)
    assert np.array_equal(code[heads][at], acode)
    have = cnt[at] > 0
    mean = sums[at][have] / cnt[at][have]
    got = agg["VALUE"].to_numpy(dtype=np.float64)[have].astype(x.dtype)
    scale = np.where(vmax[at][have] > 0, vmax[at][have], 1.0)
    return float(np.max(np.abs(got - mean) / scale)) if have.any() else 0.0


# ------------------------------------------------------------------------------------------ golden file access
def golden_events(d, kind: str):
    """(labs, cohort) frames of table `kind` ("int" / "str") of tests/golden/prep_small.npz."""
    item = d[f"{kind}_ev_item"]
    labs = pd.DataFrame({"SUBJECT_ID": d[f"{kind}_ev_sid"], "ITEMID": item if kind == "int" else item.astype(object),
                         "VALUENUM": d[f"{kind}_ev_value"], "CHARTTIME": d[f"{kind}_ev_time"]})
    return labs, pd.DataFrame({"SUBJECT_ID": d[f"{kind}_cohort"]})


def golden_frame(d, prefix: str, kind: str) -> pd.DataFrame:
    item = d[f"{prefix}_item"]
    f = pd.DataFrame({"SUBJECT_ID": d[f"{prefix}_sid"], "ITEMID": item if kind == "int" else item.astype(object),
                      "VALUE": d[f"{prefix}_value"]})
    if f"{prefix}_norm" in d:
        f["VALUE_NORMALIZED"] = d[f"{prefix}_norm"]
    return f


def same_bits(a, b) -> bool:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))
