"""numpy / pandas restatement of the feature-space selection (the checker of mmgnn.preprocess' select_codes,
filter_labs_for_cohort, process_diagnoses, process_medications and normalize_drug_name, as prep_ref.py is for the lab
half), plus the reader / writer of tests/golden/select_small.npz.

Semantics (reference src/io_mimic.py:442-516, src/preprocess.py:171-412):
  cohort filter -> distinct patients per code -> codes with >= min_patient_count patients -> the top_k most frequent
  -> every surviving row (labs) or the first row of each (patient, code) pair (diagnoses, medications), in input order
  with the original index.
Ties: among equal patient counts the smaller code wins (sorted key order).  For labs that is the reference's
nlargest(keep="first") over the groupby's sorted index; for diagnoses and medications the reference's value_counts()
leaves the order of ties to an unstable sort, and this is the project's own rule.
"""
import re

import numpy as np
import pandas as pd


# ------------------------------------------------------------------------------------------ tensor level
def select_codes(patient, code, n_patients, n_codes, valid=None, min_patient_count=1, top_k=None, rows="all"):
    """numpy arrays in -> (n_patients_per_code int64, n_rows_per_code int64, rank int32, selected uint8, out_rows int32)."""
    patient, code = np.asarray(patient, np.int64), np.asarray(code, np.int64)
    ok = (code >= 0) & (code < n_codes) & (patient >= 0) & (patient < n_patients)
    if valid is not None:
        ok &= np.asarray(valid) != 0
    idx = np.flatnonzero(ok)
    c, p = code[idx], patient[idx]
    n_rows = np.bincount(c, minlength=n_codes).astype(np.int64)
    pair, first = np.unique(c * np.int64(n_patients) + p, return_index=True)      # first occurrence of every pair
    pair_code = pair // np.int64(n_patients)
    n_pat = np.bincount(pair_code, minlength=n_codes).astype(np.int64)
    eligible = np.flatnonzero((n_rows > 0) & (n_pat >= min_patient_count))
    order = eligible[np.argsort(-n_pat[eligible], kind="stable")]                 # patients descending, code ascending
    rank = np.full(n_codes, -1, np.int32)
    rank[order] = np.arange(len(order), dtype=np.int32)
    selected = (rank >= 0) & ((top_k is None) | (rank < (0 if top_k is None else top_k)))
    if rows == "all":
        out = idx[selected[c]]
    elif rows == "first":
        out = np.sort(idx[first[selected[pair_code]]])
    else:
        raise ValueError(rows)
    return n_pat, n_rows, rank, selected.astype(np.uint8), out.astype(np.int32)


# ------------------------------------------------------------------------------------------ frame level
def _ranked(counts: pd.Series, min_patient_count, top_k) -> pd.Series:
    """counts indexed by sorted keys -> the kept ones, most frequent first, the smaller key first among equals."""
    counts = counts[counts >= min_patient_count]
    counts = counts.sort_values(ascending=False, kind="stable")
    return counts if top_k is None else counts.head(top_k)


def filter_labs(labevents, cohort, d_labitems, top_k=None, min_patient_count=10):
    labs = labevents[labevents["SUBJECT_ID"].isin(set(cohort["SUBJECT_ID"]))]
    labs = labs[labs["VALUENUM"].notna()]
    g = labs.groupby("ITEMID")
    counts = pd.DataFrame({"NUM_PATIENTS": g["SUBJECT_ID"].nunique(), "NUM_MEASUREMENTS": g["VALUENUM"].count()})
    counts = counts[counts["NUM_PATIENTS"] >= min_patient_count]
    if top_k is not None:
        counts = counts.loc[_ranked(counts["NUM_PATIENTS"], min_patient_count, top_k).index]
    labs = labs[labs["ITEMID"].isin(set(counts.index))]
    items = d_labitems[d_labitems["ITEMID"].isin(set(counts.index))].copy()
    return labs, items.merge(counts, left_on="ITEMID", right_index=True)


def _pairs(frame, cohort, source_col, out_col, rule, extras, min_patient_count, top_k):
    f = frame[frame["HADM_ID"].isin(set(cohort["HADM_ID"])) & frame["SUBJECT_ID"].isin(set(cohort["SUBJECT_ID"]))]
    text = f[source_col].astype(str).str.strip()
    f, text = f[text != ""], text[text != ""]
    text = text.map(rule)
    f, text = f[text != ""], text[text != ""]
    out = pd.DataFrame({"SUBJECT_ID": f["SUBJECT_ID"], out_col: text.astype(object)})
    for c in extras:
        if c in f.columns:
            out[c] = f[c]
    out = out.drop_duplicates(subset=["SUBJECT_ID", out_col])
    keep = _ranked(out.groupby(out_col).size(), min_patient_count, top_k)
    return out[out[out_col].isin(set(keep.index))], keep


def diagnoses(dx, cohort, collapse_to_3digit=True, top_k=None, min_patient_count=5):
    col = "ICD3_CODE" if collapse_to_3digit else "ICD9_CODE"
    rule = (lambda t: t[:3]) if collapse_to_3digit else (lambda t: t)
    return _pairs(dx, cohort, "ICD9_CODE", col, rule, ("DIAGNOSIS_CATEGORY", "DIAGNOSIS_SUBCATEGORY", "DIAGNOSIS_PRIORITY"),
                  min_patient_count, top_k)[0]


def drug_name(drug) -> str:
    if pd.isna(drug):
        return ""
    d = str(drug).lower()
    d = re.sub(r"\d+\.?\d*\s*(mg|mcg|ml|g|%|units?)", "", d)
    d = re.sub(r"\b(tablet|capsule|injection|solution|suspension|syrup|cream|ointment)\b", "", d)
    d = re.sub(r"\b(oral|topical|iv|intravenous|subcutaneous)\b", "", d)
    d = re.sub(r"[^\w\s]", " ", d).split()
    return d[0] if d else ""


def medications(rx, cohort, normalize_names=True, top_k=None, min_patient_count=5):
    rule = drug_name if normalize_names else (lambda t: t)
    return _pairs(rx, cohort, "DRUG", "DRUG", rule, ("ROUTE", "FREQUENCY", "PRN", "IV_ADMIXTURE"), min_patient_count,
                  top_k)[0]


def frames(labevents, d_labitems, dx, rx, cohort, config):
    """The selection half of preprocess_frames: (labs_filtered, labitems, diagnoses, medications)."""
    fs = config["feature_space"]
    labs, items = filter_labs(labevents, cohort, d_labitems, fs["labs"]["top_k"], fs["labs"].get("min_patient_count", 10))
    return (labs, items,
            diagnoses(dx, cohort, fs["diagnoses"]["collapse_to_3digit"], fs["diagnoses"]["top_k"],
                      fs["diagnoses"].get("min_patient_count", 5)),
            medications(rx, cohort, fs["medications"]["normalize_names"], fs["medications"]["top_k"],
                        fs["medications"].get("min_patient_count", 5)))


# ------------------------------------------------------------------------------------------ golden file access
_NAN, _NONE = 1, 2


def pack_frame(prefix: str, df: pd.DataFrame, arrays: dict, meta: dict) -> None:
    """A frame as plain arrays (no pickle): numeric columns as they are; object columns as fixed-width text plus a
    marker array (1 = NaN, 2 = None); the index as int64."""
    cols = []
    arrays[f"{prefix}/index"] = df.index.to_numpy(dtype=np.int64)
    for c in df.columns:
        v = df[c].to_numpy()
        if v.dtype == object:
            mark = np.array([_NONE if x is None else _NAN if (isinstance(x, float) and x != x) else 0 for x in v], np.uint8)
            assert all(isinstance(x, str) for x, m in zip(v, mark) if m == 0), (prefix, c)
            arrays[f"{prefix}/{c}"] = np.array([x if m == 0 else "" for x, m in zip(v, mark)], dtype="U64")
            arrays[f"{prefix}/{c}/na"] = mark
            cols.append([c, "object"])
        else:
            assert v.dtype.kind in "iuf", (prefix, c, v.dtype)
            arrays[f"{prefix}/{c}"] = v
            cols.append([c, str(v.dtype)])
    meta["frames"][prefix] = cols


def unpack_frame(d, meta: dict, prefix: str) -> pd.DataFrame:
    data = {}
    for c, kind in meta["frames"][prefix]:
        v = d[f"{prefix}/{c}"]
        if kind == "object":
            mark = d[f"{prefix}/{c}/na"]
            o = v.astype(object)
            o[mark == _NAN] = np.nan
            o[mark == _NONE] = None
            v = o
        data[c] = v
    return pd.DataFrame(data, index=pd.Index(d[f"{prefix}/index"]), columns=[c for c, _ in meta["frames"][prefix]])


def _cells(col: pd.Series):
    return [("<NaN>" if (isinstance(x, float) and x != x) else "<None>" if x is None else x) for x in col.tolist()]


def same_frame(got: pd.DataFrame, want: pd.DataFrame) -> bool:
    """Columns, index, dtypes' kinds and every cell (NaN equals NaN, None only None)."""
    if list(got.columns) != list(want.columns) or not np.array_equal(got.index.to_numpy(), want.index.to_numpy()):
        return False
    for c in want.columns:
        g, w = got[c], want[c]
        if (g.dtype == object) != (w.dtype == object):
            return False
        if w.dtype != object and (g.dtype.kind != w.dtype.kind or not np.array_equal(g.to_numpy(), w.to_numpy(), equal_nan=w.dtype.kind == "f")):
            return False
        if w.dtype == object and _cells(g) != _cells(w):
            return False
    return True
