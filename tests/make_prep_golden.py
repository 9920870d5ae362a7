#!/usr/bin/env python3
"""Generate tests/golden/prep_small.npz by running the REFERENCE's own preprocess / utils functions.

Runs only where a checkout of the reference exists (its root in MMGNN_REFERENCE); nothing of it is copied.  Stored
(data only), for two fixed event tables ("int": integer ITEMIDs, "str": string ITEMIDs):
  the events and the cohort; for each of 5 aggregations x outlier removal on / off the aggregated frame; for each of
  those x 3 normalisers the normalised frame (rows kept, VALUE, VALUE_NORMALIZED) and every normalizer.stats entry;
  remove_outliers("std" / "iqr") on bare arrays;
  the largest deviation of the reference's sum-type results (means, stds, "mean" aggregation, z-scores) from the
  high-precision evaluation of prep_ref.py -- the measured margin the device path is allowed 8x of.
The generator asserts that the tables contain every edge case the tests rely on, and that no value lies within 1e-9
(relative) of an outlier bound.

Usage:  MMGNN_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/make_prep_golden.py
"""
import json
import logging
import os
import sys

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.environ["MMGNN_REFERENCE"]
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REF, "src"))
logging.disable(logging.CRITICAL)

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

import preprocess as ref_prep  # noqa: E402
import utils as ref_utils  # noqa: E402
import prep_ref  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "prep_small.npz")
AGGS = ("last", "mean", "median", "min", "max")
NORMS = ("zscore", "minmax", "robust")
THRESHOLD = 5.0
N_PAT, N_LAB = 40, 8                      # bulk labs 0..7; special labs 8..10


def make_table(seed: int):
    """Events over 40 cohort patients (ids 1000..1039) + 3 outside, 8 bulk labs and 3 special ones (integer codes)."""
    rng = np.random.default_rng(seed)
    rows = []                                               # (patient, lab, value, time)
    loc = 10.0 ** np.linspace(0, 2, N_LAB)
    for p in range(N_PAT):
        for lab in rng.choice(N_LAB, size=rng.integers(3, N_LAB + 1), replace=False):
            k = 1 + rng.poisson(3.0)
            t = rng.integers(0, 6, k) * 60.0                # hours: many ties inside a pair
            v = loc[lab] * (1 + 0.2 * rng.standard_normal(k))
            rows += [(1000 + p, int(lab), float(a), float(b)) for a, b in zip(v, t)]
    rows += [(2000 + int(rng.integers(0, 3)), int(rng.integers(0, N_LAB)), float(rng.normal(5, 1)), 60.0) for _ in range(25)]
    # hand-made cases on cohort patients
    rows += [(1001, 0, 9999.0, 100000.0)]                   # gross outlier with the pair's greatest time
    rows += [(1002, 1, float("nan"), 30.0), (1002, 1, 2.5, float("nan")), (1002, 1, 3.5, 99999.0)]   # missing time wins
    rows += [(1003, 2, float("nan"), 10.0), (1003, 2, float("nan"), 20.0)]
    rows = [r for r in rows if not (r[0] == 1003 and r[1] == 2 and r[2] == r[2])]   # pair (1003, 2): all NaN
    rows += [(1004, 3, 7.25, 5.0), (1004, 3, 7.75, 5.0), (1004, 3, 6.5, 5.0)]        # three-way time tie: the last wins
    rows += [(1005, 8, 42.0, 1.0)]                          # lab 8: one value
    rows += [(1000 + p, 9, 7.5, float(p)) for p in range(12)]                        # lab 9: all equal (exact sums)
    rows += [(1006, 10, float("nan"), 1.0), (1007, 10, float("nan"), 2.0)]           # lab 10: no valid value
    rows += [(1008, 4, float("nan"), 1e6)]                  # a NaN as the last event of a pair
    order = rng.permutation(len(rows))
    a = np.array(rows, dtype=np.float64)[order]
    return pd.DataFrame({"SUBJECT_ID": a[:, 0].astype(np.int64), "ITEMID": a[:, 1].astype(np.int64), "VALUENUM": a[:, 2],
                         "CHARTTIME": a[:, 3]})


def check_table(labs, cohort):
    """Every edge case the tests rely on is in the table."""
    inc = labs[labs["SUBJECT_ID"].isin(cohort["SUBJECT_ID"])]
    assert len(inc) < len(labs), "patients outside the cohort"
    pairs = inc.groupby(["SUBJECT_ID", "ITEMID"])
    assert (pairs["CHARTTIME"].apply(lambda t: t.dropna().duplicated().any())).any(), "time ties inside a pair"
    assert inc["CHARTTIME"].isna().any(), "a missing time"
    assert pairs["VALUENUM"].apply(lambda v: v.isna().all()).any(), "a pair whose values are all NaN"
    sizes = pairs.size()
    assert (sizes == 1).any() and (sizes % 2 == 0).any() and ((sizes % 2 == 1) & (sizes > 1)).any(), "pair sizes"
    per_lab = inc.groupby("ITEMID")["VALUENUM"]
    assert (per_lab.count() == 1).any(), "a lab with one value"
    assert ((per_lab.nunique() == 1) & (per_lab.count() > 1)).any(), "a lab whose values are all equal"
    assert (per_lab.count() == 0).any(), "a lab with no valid value"
    # a gross outlier that is removed and would otherwise have been the "last" value
    on = ref_prep.aggregate_lab_values(labs, cohort, "last", True, THRESHOLD)
    off = ref_prep.aggregate_lab_values(labs, cohort, "last", False, THRESHOLD)
    m = on.merge(off, on=["SUBJECT_ID", "ITEMID"], suffixes=("_on", "_off"))
    assert ((m["VALUE_off"] == 9999.0) & (m["VALUE_on"] != 9999.0)).any(), "removed outlier that was the last value"
    for _, g in inc.groupby("ITEMID"):
        v = g["VALUENUM"].dropna()
        if len(v) > 1 and v.nunique() == 1 and float(v.iloc[0]) * 1024 == int(float(v.iloc[0]) * 1024):
            # the all-equal lab: std is 0 and both bounds ARE the value.  Its sums are exact in any order (a short
            # binary fraction times a small count), so mean = value and std = 0 to the bit on every path, and the strict
            # comparisons remove nothing: this decision does not hang on rounding either.
            assert v.std() == 0.0 and v.mean() == v.iloc[0]
            continue
        assert prep_ref.bound_margin(g["VALUENUM"], "std", THRESHOLD) > 1e-9, "a value within 1e-9 of an outlier bound"


def frame_arrays(prefix, df, arrays, itemid_kind):
    arrays[f"{prefix}_sid"] = df["SUBJECT_ID"].to_numpy(dtype=np.int64)
    arrays[f"{prefix}_item"] = df["ITEMID"].to_numpy(dtype=np.int64) if itemid_kind == "int" else df["ITEMID"].to_numpy(dtype="U16")
    arrays[f"{prefix}_value"] = df["VALUE"].to_numpy(dtype=np.float64)
    if "VALUE_NORMALIZED" in df:
        arrays[f"{prefix}_norm"] = df["VALUE_NORMALIZED"].to_numpy(dtype=np.float64)


def jsonable(stats):
    return {k: (None if v is None else {f: float(x) for f, x in v.items()}) for k, v in stats.items()}


def main():
    arrays, meta = {}, {"threshold": THRESHOLD, "tables": {}, "stats": {}, "outliers": {}}
    worst = 0.0
    for kind, seed in (("int", 11), ("str", 12)):
        labs = make_table(seed)
        if kind == "str":
            labs["ITEMID"] = labs["ITEMID"].map(lambda i: f"lab_{i:02d}")
        cohort = pd.DataFrame({"SUBJECT_ID": np.arange(1000, 1000 + N_PAT, dtype=np.int64)[::-1].copy()})
        check_table(labs, cohort)
        arrays[f"{kind}_ev_sid"] = labs["SUBJECT_ID"].to_numpy()
        arrays[f"{kind}_ev_item"] = labs["ITEMID"].to_numpy() if kind == "int" else labs["ITEMID"].to_numpy(dtype="U16")
        arrays[f"{kind}_ev_value"] = labs["VALUENUM"].to_numpy()
        arrays[f"{kind}_ev_time"] = labs["CHARTTIME"].to_numpy()
        arrays[f"{kind}_cohort"] = cohort["SUBJECT_ID"].to_numpy()
        meta["tables"][kind] = {"events": len(labs)}
        for agg in AGGS:
            for remove in (True, False):
                tag = f"{kind}_{agg}_{'on' if remove else 'off'}"
                la = ref_prep.aggregate_lab_values(labs, cohort, agg, remove, THRESHOLD)
                frame_arrays(f"{tag}_agg", la, arrays, kind)
                if agg == "mean":
                    ev = prep_ref.clean_events(labs, cohort["SUBJECT_ID"], remove, THRESHOLD)
                    worst = max(worst, prep_ref.mean_agg_deviation(ev, la))
                for norm in NORMS:
                    ln, nz = ref_prep.normalize_lab_values(la, norm)
                    frame_arrays(f"{tag}_{norm}", ln, arrays, kind)
                    meta["stats"][f"{tag}_{norm}"] = jsonable(nz.stats)
                    if norm == "zscore":
                        lc, keys = pd.factorize(la["ITEMID"], sort=True)
                        gm = {k: nz.stats[str(key)]["mean"] for k, key in enumerate(keys) if nz.stats[str(key)]}
                        gs = {k: nz.stats[str(key)]["std"] for k, key in enumerate(keys) if nz.stats[str(key)]}
                        full = la.copy()                     # z of every pair, NaN rows included, in la's order
                        z = np.full(len(la), np.nan)
                        for k, key in enumerate(keys):
                            sel = lc == k
                            z[sel] = nz.transform(la["VALUE"][sel], str(key)).to_numpy()
                        ok = np.isin(lc, list(gm))
                        worst = max(worst, prep_ref.sum_deviations(lc[ok], full["VALUE"].to_numpy()[ok], gm, gs, z[ok]))
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.normal(50, 4, 400), [9999.0, -500.0, np.nan, 71.0, 29.5]])
    rng.shuffle(x)
    for name, arr, method, thr in (("std5", x, "std", 5.0), ("iqr15", x, "iqr", 1.5), ("iqr3", x[:64], "iqr", 3.0),
                                   ("one", np.array([3.0]), "std", 5.0), ("nan", np.array([np.nan, np.nan]), "iqr", 1.5)):
        assert prep_ref.bound_margin(arr, method, thr) > 1e-9
        arrays[f"out_{name}_in"] = arr
        arrays[f"out_{name}_out"] = ref_utils.remove_outliers(pd.Series(arr), method, thr).to_numpy()
        meta["outliers"][name] = {"method": method, "threshold": thr}
    meta["sum_rel_dev_max"] = worst
    meta["long_double_mantissa_bits"] = int(np.finfo(np.longdouble).nmant)
    np.savez_compressed(OUT, __meta__=np.array(json.dumps(meta)), **arrays)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1024:.1f} KiB, reference deviation from exact {worst:.3e}")


if __name__ == "__main__":
    main()
