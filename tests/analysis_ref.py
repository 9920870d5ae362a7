"""Checkers of the prediction analysis (mmgnn/analysis.py), written from the behaviour of the reference's
src/advanced_visualizations.py with plain numpy / pandas (a loop per lab, a boolean mask per decile, pandas' own cut /
qcut / groupby).

* ``*_f64``: the float64 evaluation of the reference's formulas.  The elementwise terms are the ones numpy forms on the
  reference's fp32 arrays (pred - true, its absolute value and square; a * true + b with the fp32 line); every reduction
  (mean, standard deviation, sums, the least-squares solve, R^2) is float64.
* ``*_mixed``: the reference's own recipe -- sklearn's LinearRegression on fp32 inputs (an fp32 solve), np.mean of fp32
  arrays (fp32 pairwise sums), fp32 R^2, pandas' groupby of an fp32 column (accumulated in float64 but RETURNED in fp32:
  the degree table of the reference is not exact to float64 either).  calibration_mixed needs sklearn.
* ``*_hp``: the same float64 formulas with exactly rounded sums (math.fsum).

Bounds.  A device (or host-path) table may be no further from the float64 evaluation than the reference's own recipe
is: per column, BOUNDS holds max over the rows of |mixed - f64| on the named input, and where that distance is zero,
8 x max |f64 - hp| (no column of these inputs needs that second rule).  The figures were measured on the CPU with the
recipes of this file (numpy 2.x, pandas 2.x, scikit-learn 1.7) on ``inputs(make_graph(scale, seed=0))``; tests/test_analysis_cpu.py measures them again
and fails if they moved.
"""
import math

import numpy as np
import pandas as pd

BINS = (0, 1, 6, 16, 50)
LABELS = ("0-1", "2-5", "6-15", "16+")
CAL_FLOAT = ["a", "b", "mae_before", "mae_after", "delta_mae"]
DEG_FLOAT = ["mean", "std"]
DEC_FLOAT = ["mae", "r2"]

# input ("x1" / "x100": inputs(make_graph(scale, seed=0)) under the default bins) -> column -> the allowed absolute
# distance from the float64 evaluation: measure_bounds() on that input, rounded up to three digits.  Every figure is
# the first rule's (the reference recipe's own distance); the is_calibrated thresholds are at least 0.017 away from
# every lab's a and b on both inputs.
BOUNDS = {
    "x1": {
        "calibration.a": 3.34e-07,
        "calibration.b": 4.36e-08,
        "calibration.mae_before": 3.72e-08,
        "calibration.mae_after": 2.06e-07,
        "calibration.delta_mae": 2.06e-07,
        "decile.mae": 2.42e-08,
        "decile.r2": 2.93e-08,
        "degree.mean": 2.31e-08,
        "degree.std": 5.55e-09,
    },
    "x100": {
        "calibration.a": 5.75e-07,
        "calibration.b": 6.19e-08,
        "calibration.mae_before": 4.92e-08,
        "calibration.mae_after": 1.94e-07,
        "calibration.delta_mae": 2.02e-07,
        "decile.mae": 8.15e-08,
        "decile.r2": 6.45e-08,
        "degree.mean": 7.84e-09,
        "degree.std": 5.99e-09,
    },
}


def inputs(graph, seed=1, noise=0.2):
    """Predictions with structure and known answers on a synthetic graph's has_lab pairs:
    pred = target * s_lab + o_lab + noise, slope and offset per lab drawn once from a seeded generator.
    -> (pred fp32, target fp32, patient int64, lab int64, slope, offset) as numpy arrays."""
    ei = graph["patient", "has_lab", "lab"].edge_index.cpu().numpy()
    t = graph["patient", "has_lab", "lab"].edge_attr.cpu().numpy().reshape(-1).astype(np.float32)
    n_labs = int(graph["lab"].num_nodes)
    rng = np.random.default_rng(seed)
    # slopes and offsets keep clear of the is_calibrated thresholds (|a - 1| = 0.1, |b| = 0.1) by 0.02
    slope = np.where(rng.random(n_labs) < 0.5, rng.uniform(0.93, 1.07, n_labs),
                     np.where(rng.random(n_labs) < 0.5, rng.uniform(0.6, 0.87, n_labs), rng.uniform(1.13, 1.4, n_labs)))
    offset = np.where(rng.random(n_labs) < 0.5, rng.uniform(-0.07, 0.07, n_labs),
                      rng.choice([-1.0, 1.0], n_labs) * rng.uniform(0.13, 0.5, n_labs))
    li = ei[1]
    p = (t.astype(np.float64) * slope[li] + offset[li] + noise * rng.standard_normal(t.size)).astype(np.float32)
    return p, t, ei[0].astype(np.int64), li.astype(np.int64), slope, offset


def degrees(graph):
    ei = graph["patient", "has_lab", "lab"].edge_index.cpu().numpy()
    return np.bincount(ei[0], minlength=int(graph["patient"].num_nodes))


# ------------------------------------------------------------------------------------------ calibration
def _cal_frame(rows):
    cols = ["lab_idx", "lab_name", "n_samples", "a", "b", "mae_before", "mae_after", "delta_mae", "is_calibrated"]
    if not rows:
        return pd.DataFrame({c: [] for c in cols})
    return pd.DataFrame(rows, columns=cols).sort_values("mae_before", ascending=False)


def _names(lab_names, i):
    return (lab_names or {}).get(i, f"Lab_{i}")


def calibration_f64(pred, target, lab, lab_names=None, mean=np.mean, total=np.sum):
    pred, target = np.asarray(pred, np.float32), np.asarray(target, np.float32)
    rows = []
    for i in np.unique(lab):
        m = lab == i
        if m.sum() < 2:
            continue
        t, p = target[m], pred[m]
        t64, p64 = t.astype(np.float64), p.astype(np.float64)
        if t.min() == t.max():
            a, b = 0.0, float(mean(p64))
        else:
            tm, pm = mean(t64), mean(p64)
            tc = t64 - tm
            a = float(total(tc * (p64 - pm)) / total(tc * tc))
            b = float(pm - a * tm)
        before = float(mean(np.abs(p - t).astype(np.float64)))
        cal = np.float32(a) * t + np.float32(b)
        after = float(mean(np.abs(cal - t).astype(np.float64)))
        rows.append([int(i), _names(lab_names, int(i)), int(m.sum()), a, b, before, after, after - before,
                     abs(a - 1.0) < 0.1 and abs(b) < 0.1])
    return _cal_frame(rows)


def _fsum_mean(x):
    return math.fsum(x.tolist()) / x.size


def _fsum(x):
    return math.fsum(np.asarray(x).tolist())


def calibration_hp(pred, target, lab, lab_names=None):
    return calibration_f64(pred, target, lab, lab_names, mean=_fsum_mean, total=_fsum)


def calibration_mixed(pred, target, lab, lab_names=None):
    from sklearn.linear_model import LinearRegression
    pred, target = np.asarray(pred, np.float32), np.asarray(target, np.float32)
    rows = []
    for i in np.unique(lab):
        m = lab == i
        if m.sum() < 2:
            continue
        t, p = target[m], pred[m]
        lr = LinearRegression()
        lr.fit(t.reshape(-1, 1), p)
        a, b = lr.coef_[0], lr.intercept_
        before = np.mean(np.abs(p - t))
        after = np.mean(np.abs(a * t + b - t))
        rows.append([int(i), _names(lab_names, int(i)), int(m.sum()), a, b, before, after, after - before,
                     bool(abs(a - 1.0) < 0.1 and abs(b) < 0.1)])
    return _cal_frame(rows)


# ------------------------------------------------------------------------------------------ error vs degree
def degree_f64(pred, target, patient, deg, bins=BINS, labels=LABELS, dtype=np.float64):
    """pandas' own cut / groupby over the fp32 errors held as float64."""
    err = np.abs(np.asarray(pred, np.float32) - np.asarray(target, np.float32)).astype(dtype)
    df = pd.DataFrame({"degree": np.asarray(deg)[patient], "error": err})
    df["degree_bin"] = pd.cut(df["degree"], bins=list(bins), labels=list(labels), right=False)
    return df.groupby("degree_bin", observed=False)["error"].agg(["mean", "std", "count"]).reset_index()


def degree_mixed(pred, target, patient, deg, bins=BINS, labels=LABELS):
    """as the reference runs it: an fp32 error column, whose group means and deviations pandas returns in fp32"""
    return degree_f64(pred, target, patient, deg, bins, labels, dtype=np.float32)


def degree_hp(pred, target, patient, deg, bins=BINS, labels=LABELS):
    err = np.abs(np.asarray(pred, np.float32) - np.asarray(target, np.float32)).astype(np.float64)
    d = np.asarray(deg)[patient].astype(np.float64)
    rows = []
    for j, name in enumerate(labels):
        e = err[(d >= bins[j]) & (d < bins[j + 1])]
        n = e.size
        mean = _fsum_mean(e) if n else float("nan")
        # the exactly rounded mean is itself rounded: sum (e - mean)^2 with a longdouble mean correction
        if n > 1:
            dev = e.astype(np.longdouble) - np.longdouble(math.fsum(e.tolist())) / np.longdouble(n)
            std = float(np.sqrt(np.sum(dev * dev) / np.longdouble(n - 1)))
        else:
            std = float("nan")
        rows.append([name, mean, std, n])
    return pd.DataFrame(rows, columns=["degree_bin", "mean", "std", "count"])


# ------------------------------------------------------------------------------------------ parity by decile
def _deciles(lab):
    labs, counts = np.unique(lab, return_counts=True)
    f = pd.DataFrame({"lab_idx": labs, "count": counts}).sort_values("count")
    f["decile"] = pd.qcut(f["count"], q=10, labels=False, duplicates="drop")
    return f


def _decile_rows(pred, target, lab, metric):
    pred, target = np.asarray(pred, np.float32), np.asarray(target, np.float32)
    cols = ["decile", "n_labs", "count_min", "count_max", "n_pairs", "mae", "r2"]
    if np.asarray(lab).size == 0:
        return pd.DataFrame({c: [] for c in cols})
    f = _deciles(lab)
    rows = []
    for d in sorted(f["decile"].dropna().unique()):
        g = f[f["decile"] == d]
        m = np.isin(lab, g["lab_idx"].values)
        mae, r2 = metric(pred[m], target[m])
        rows.append([int(d), len(g), int(g["count"].min()), int(g["count"].max()), int(m.sum()), mae, r2])
    return pd.DataFrame(rows, columns=cols)


def _metric_f64(p, t):
    with np.errstate(divide="ignore", invalid="ignore"):
        mae = float(np.mean(np.abs(p - t).astype(np.float64)))
        d = t - p
        t64 = t.astype(np.float64)
        r2 = float(1 - np.sum((d * d).astype(np.float64)) / np.sum((t64 - t64.mean()) ** 2))
    return mae, r2


def _metric_hp(p, t):
    with np.errstate(divide="ignore", invalid="ignore"):
        mae = _fsum_mean(np.abs(p - t).astype(np.float64))
        d = t - p
        t64 = t.astype(np.float64)
        tc = t64 - _fsum_mean(t64)
        r2 = float(1 - np.float64(_fsum((d * d).astype(np.float64))) / np.float64(_fsum(tc * tc)))
    return mae, r2


def _metric_mixed(p, t):
    with np.errstate(divide="ignore", invalid="ignore"):
        mae = np.mean(np.abs(p - t))
        r2 = 1 - np.sum((t - p) ** 2) / np.sum((t - t.mean()) ** 2)
    return float(mae), float(r2)


def deciles_f64(pred, target, lab):
    return _decile_rows(pred, target, lab, _metric_f64)


def deciles_hp(pred, target, lab):
    return _decile_rows(pred, target, lab, _metric_hp)


def deciles_mixed(pred, target, lab):
    return _decile_rows(pred, target, lab, _metric_mixed)


# ------------------------------------------------------------------------------------------ distances
def distance(a: pd.DataFrame, b: pd.DataFrame, col: str, key=None) -> float:
    """max over the rows of |a[col] - b[col]|; cells that are NaN / inf in both and equal as such count 0, a NaN or
    inf on one side only is an infinite distance.  No row is dropped."""
    if key is not None:
        a, b = a.sort_values(key), b.sort_values(key)
    x, y = np.asarray(a[col], np.float64), np.asarray(b[col], np.float64)
    assert x.shape == y.shape, (col, x.shape, y.shape)
    same = (np.isnan(x) & np.isnan(y)) | (np.isinf(x) & (x == y))
    with np.errstate(invalid="ignore"):
        d = np.where(same, 0.0, np.abs(x - y))
    d = np.where(np.isnan(d), np.inf, d)
    return float(d.max()) if d.size else 0.0


def measure_bounds(pred, target, patient, lab, deg):
    """column -> allowed distance on this input (the rule of the module docstring), with its two ingredients."""
    out = {}

    def rule(name, cols, f64, mixed, hp, key=None):
        for c in cols:
            d = distance(mixed, f64, c, key)
            out[name + "." + c] = d if d > 0 else 8.0 * distance(f64, hp(), c, key)

    rule("calibration", CAL_FLOAT, calibration_f64(pred, target, lab), calibration_mixed(pred, target, lab),
         lambda: calibration_hp(pred, target, lab), "lab_idx")
    rule("decile", DEC_FLOAT, deciles_f64(pred, target, lab), deciles_mixed(pred, target, lab),
         lambda: deciles_hp(pred, target, lab))
    rule("degree", DEG_FLOAT, degree_f64(pred, target, patient, deg), degree_mixed(pred, target, patient, deg),
         lambda: degree_hp(pred, target, patient, deg))
    return out
