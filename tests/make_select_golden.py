#!/usr/bin/env python3
"""Generate tests/golden/select_small.npz by running the REFERENCE's own filter_labs_for_cohort, process_diagnoses,
process_medications and normalize_drug_name.

Runs only where a checkout of the reference exists (its root in MMGNN_REFERENCE); nothing of it is copied.  Stored (data
only): the small fixed tables (a cohort of 40 patients and a few outside; lab events with integer and with string
ITEMIDs and the lab dictionary; diagnoses; prescriptions) and, for every argument combination listed in CASES, the
frames the reference returned -- columns, values and index.  The generator asserts that the tables contain every edge
case the tests rely on and that, for diagnoses and medications, the count just inside every top_k cut is strictly greater
than the one just outside (the reference's order among equal counts is that of an unstable sort and is kept out of the
fixture).

Usage:  MMGNN_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/make_select_golden.py
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

import io_mimic as ref_io  # noqa: E402
import preprocess as ref_prep  # noqa: E402
import select_ref  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "select_small.npz")
N_PAT = 40
LAB_MIN, DX_MIN, RX_MIN = 10, 5, 5
CASES = {"labs": [None, 5, 2, 0], "dx": [(True, None), (True, 6), (False, None), (False, 4)],
         "rx": [(True, None), (True, 5), (False, None), (False, 2)]}


def sid(p):
    return 1000 + p


def hadm(p):
    return 5000 + p


def make_cohort():
    p = np.arange(N_PAT)[::-1]
    return pd.DataFrame({"SUBJECT_ID": sid(p).astype(np.int64), "HADM_ID": hadm(p).astype(np.int64)})


def shuffled(rows, columns, seed, first_index):
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(rows))
    df = pd.DataFrame([rows[i] for i in order], columns=columns)
    df.index = pd.Index(np.arange(first_index, first_index + len(df), dtype=np.int64)[::-1].copy())   # not a RangeIndex
    return df


def make_labs(seed):
    """16 labs, patient counts 38 35 35 30 30 30 25 20 15 12 10 9 5 3, one lab whose NaN-only patients pull it below the
    minimum, one lab that only patients outside the cohort have.  The ids are not in count order."""
    counts = [38, 35, 35, 30, 30, 30, 25, 20, 15, 12, 10, 9, 5, 3]
    ids = [50820, 50811, 50807, 50816, 50803, 50809, 50801, 50802, 50804, 50805, 50806, 50808, 50810, 50812]
    rng = np.random.default_rng(seed)
    rows = []
    for lab, cnt in zip(ids, counts):
        for p in rng.choice(N_PAT, size=cnt, replace=False):
            k = 1 + int(rng.integers(0, 4))
            rows += [(sid(p), lab, float(rng.normal(10, 2)), 60.0 * t) for t in range(k)]
            if rng.random() < 0.3:
                rows.append((sid(p), lab, float("nan"), 999.0))
    for p in range(11):                                       # lab 50813: 11 patients with rows, 2 of them NaN only
        rows.append((sid(p), 50813, float("nan") if p < 2 else 1.5 + p, 5.0))
    rows += [(sid(0), 50820, 7.0, 1000.0 + t) for t in range(12)]                  # one pair many times
    rows += [(2000 + q, 50814, 3.0 + q, 1.0) for q in range(3)]                    # outside the cohort only
    rows += [(2000 + q % 3, 50806, 3.0, 1.0) for q in range(6)]                    # would lift lab 50806 over its rank
    return shuffled(rows, ["SUBJECT_ID", "ITEMID", "VALUENUM", "CHARTTIME"], seed + 1, 700)


def make_labitems(ids):
    rows = [(i, f"label {i}", "Blood" if i % 2 else "Urine", "Chemistry") for i in ids]
    df = pd.DataFrame(rows, columns=["ITEMID", "LABEL", "FLUID", "CATEGORY"])
    return df.iloc[np.random.default_rng(3).permutation(len(df))].copy()          # shuffled, its index kept


def make_dx():
    """Patient sets per ICD-9 code; 4280 and 4281 share patients 24..27 and collapse to 428."""
    plan = {"4280": range(0, 28), "4281": range(24, 30), "25000": range(5, 30), "4019": range(10, 32), "5849": range(20, 39),
            "2724": range(0, 16), "41401": range(27, 40), "2859": range(3, 13), "53081": range(33, 40),
            "V5861": range(15, 20), "E8788": range(36, 40), "99591": range(1, 4), "0389": range(8, 10), "486": range(39, 40)}
    rng = np.random.default_rng(21)
    rows, serial = [], 0
    for code, pats in plan.items():
        for p in pats:
            for _ in range(1 + int(rng.integers(0, 3))):
                text = code if rng.random() < 0.7 else f" {code}  "             # whitespace-padded
                rows.append((sid(p), hadm(p), text, f"cat{serial % 5}" if serial % 11 else None, serial))
                serial += 1
    rows += [(sid(2), hadm(2), "4280", "many", 9000 + t) for t in range(9)]       # one pair many times
    rows += [(sid(p), hadm(p), np.nan, "nan-code", 9100 + p) for p in range(6)]   # missing codes: 'nan' reaches the minimum
    rows += [(sid(7), hadm(7), None, "none-code", 9200), (sid(8), hadm(8), "", "empty", 9201),
             (sid(9), hadm(9), "   ", "blank", 9202)]
    rows += [(sid(39), 9999, "5849", "adm-outside", 9300)]                        # patient inside, admission outside
    rows += [(2000, hadm(3), "4019", "pat-outside", 9301)]                        # admission inside, patient outside
    rows += [(2001, 9998, "4019", "both-outside", 9302)]
    return shuffled(rows, ["SUBJECT_ID", "HADM_ID", "ICD9_CODE", "DIAGNOSIS_CATEGORY", "DIAGNOSIS_PRIORITY"], 22, 300)


DRUGS = {   # generic -> (patients, raw spellings)
    "aspirin": (range(0, 30), ["Aspirin 81mg Tablet", "aspirin EC", "ASPIRIN (Oral)", " Aspirin 325 mg "]),
    "metoprolol": (range(3, 30), ["Metoprolol Tartrate 25mg", "Metoprolol-Succinate XL", "metoprolol 5 mg/5 ml injection"]),
    "heparin": (range(10, 34), ["Heparin 5000 units", "Heparin (porcine) 1 unit", "heparin IV"]),
    "insulin": (range(15, 36), ["Insulin Subcutaneous", "Insulin, Regular", "INSULIN 100 units/ml"]),
    "furosemide": (range(22, 40), ["Furosemide 40 mg Oral Solution", "furosemide"]),
    "potassium": (range(0, 15), ["Potassium Chloride 20 mEq", "Potassium Chl. 10% syrup"]),
    "acetaminophen": (range(28, 40), ["Acetaminophen 500mg Capsule", "acetaminophen 650 mg"]),
    "morphine": (range(5, 14), ["Morphine Sulfate 2.5 mg Intravenous", "morphine 0.5mg"]),
    "lorazepam": (range(30, 37), ["Lorazepam 1 mg", "lorazepam Topical Cream"]),
    "vancomycin": (range(17, 22), ["Vancomycin 1 g", "vancomycin 250 mcg suspension"]),
    "ondansetron": (range(1, 5), ["Ondansetron 4mg ointment"]),
    "dextrose": (range(36, 39), ["5% Dextrose", "50 % dextrose"]),
    "d5w": (range(12, 14), ["D5W"]),
}
EMPTY_DRUGS = ["5 mg", "IV", "Oral Solution", "10%", "--- / ---", "20 units Subcutaneous Injection"]


def make_rx():
    rng = np.random.default_rng(31)
    rows, serial = [], 0
    for _, (pats, names) in DRUGS.items():
        for p in pats:
            for _ in range(1 + int(rng.integers(0, 3))):
                rows.append((sid(p), hadm(p), names[int(rng.integers(0, len(names)))], ("PO", "IV", None)[serial % 3],
                             "Y" if serial % 4 == 0 else "N"))
                serial += 1
    rows += [(sid(4), hadm(4), "Aspirin 81mg Tablet", "many", "N") for _ in range(8)]
    rows += [(sid(p), hadm(p), name, "empty-name", "N") for p, name in enumerate(EMPTY_DRUGS)]
    rows += [(sid(p), hadm(p), np.nan, "nan-name", "N") for p in range(5)]
    rows += [(sid(6), hadm(6), None, "none-name", "N"), (sid(7), hadm(7), "", "empty", "N"), (sid(8), hadm(8), "  ", "blank", "N")]
    rows += [(sid(38), 9999, "furosemide", "adm-outside", "N"), (2000, hadm(3), "heparin IV", "pat-outside", "N")]
    return shuffled(rows, ["SUBJECT_ID", "HADM_ID", "DRUG", "ROUTE", "PRN"], 32, 100)


# ------------------------------------------------------------------------------------------ the cases are present
def check_labs(labs, cohort):
    inc = labs[labs["SUBJECT_ID"].isin(cohort["SUBJECT_ID"])]
    assert len(inc) < len(labs), "rows outside the cohort"
    assert inc.groupby(["SUBJECT_ID", "ITEMID"]).size().max() >= 10, "a pair many times"
    num = inc[inc["VALUENUM"].notna()]
    with_rows = inc.groupby("ITEMID")["SUBJECT_ID"].nunique()
    counted = num.groupby("ITEMID")["SUBJECT_ID"].nunique().reindex(with_rows.index, fill_value=0)
    assert ((with_rows >= LAB_MIN) & (counted < LAB_MIN)).any(), "a lab that NaN-only patients pull below the minimum"
    assert (counted == LAB_MIN).any() and (counted == LAB_MIN - 1).any(), "labs at and just below the minimum"
    ranked = counted[counted >= LAB_MIN].sort_values(ascending=False, kind="stable")
    for k in CASES["labs"]:
        if k:
            assert ranked.iloc[k - 1] == ranked.iloc[k], f"a tie at the top-{k} cut"
            tied = ranked[ranked == ranked.iloc[k]].index
            assert list(tied) == sorted(tied) and ranked.index[k - 1] in tied
    outside_only = set(labs["ITEMID"]) - set(inc["ITEMID"])
    assert outside_only, "a lab only patients outside the cohort have"


def check_pairs(frame, cohort, col, min_count, top_ks, what):
    in_s, in_h = frame["SUBJECT_ID"].isin(cohort["SUBJECT_ID"]), frame["HADM_ID"].isin(cohort["HADM_ID"])
    assert (in_s & ~in_h).any() and (~in_s & in_h).any(), f"{what}: a row with only one of patient / admission inside"
    raw = frame[col]
    assert raw.map(lambda x: isinstance(x, float) and x != x).any() and raw.map(lambda x: x is None).any(), f"{what}: NaN and None"
    assert (raw == "").any() and raw.map(lambda x: isinstance(x, str) and x != "" and x.strip() == "").any(), f"{what}: '' and blanks"
    assert raw.map(lambda x: isinstance(x, str) and x.strip() != "" and x != x.strip()).any(), f"{what}: padded codes"
    inc = frame[in_s & in_h]
    assert inc.groupby(["SUBJECT_ID", col], dropna=False).size().max() >= 8, f"{what}: a pair many times"
    for n_rule, (rule, ks) in enumerate(top_ks):
        text = inc[col].astype(str).str.strip()
        text = text[text != ""].map(rule)
        text = text[text != ""]
        counts = pd.DataFrame({"p": inc.loc[text.index, "SUBJECT_ID"], "c": text}).drop_duplicates().groupby("c").size()
        if n_rule == 0:
            assert (counts == min_count).any() and (counts == min_count - 1).any(), f"{what}: codes at and just below the minimum"
        ranked = counts[counts >= min_count].sort_values(ascending=False, kind="stable")
        for k in ks:
            if k is not None and k < len(ranked):
                assert ranked.iloc[k - 1] > ranked.iloc[k], f"{what}: equal counts across the top-{k} cut ({ranked.tolist()})"
            assert k is None or k < len(ranked), f"{what}: top_k {k} does not cut"


def check_dx(dx, cohort):
    check_pairs(dx, cohort, "ICD9_CODE", DX_MIN, [(lambda t: t[:3], [k for c, k in CASES["dx"] if c]),
                                                 (lambda t: t, [k for c, k in CASES["dx"] if not c])], "diagnoses")
    inc = dx[dx["SUBJECT_ID"].isin(cohort["SUBJECT_ID"]) & dx["HADM_ID"].isin(cohort["HADM_ID"])].copy()
    inc["c9"] = inc["ICD9_CODE"].astype(str).str.strip()
    inc["c3"] = inc["c9"].str[:3]
    per = inc.groupby(["SUBJECT_ID", "c3"])["c9"].nunique()
    assert (per > 1).any(), "two ICD-9 codes of one patient under one 3-digit code"
    # ... and somewhere the LATER code's first row differs in metadata from the pair's first row
    first = inc.drop_duplicates(["SUBJECT_ID", "c3"])
    first9 = inc.drop_duplicates(["SUBJECT_ID", "c9"])
    later = first9[~first9.index.isin(first.index)]
    m = later.merge(first[["SUBJECT_ID", "c3", "DIAGNOSIS_PRIORITY"]], on=["SUBJECT_ID", "c3"], suffixes=("", "_first"))
    assert len(m) and (m["DIAGNOSIS_PRIORITY"] != m["DIAGNOSIS_PRIORITY_first"]).all(), "metadata of the earlier row"


def check_rx(rx, cohort):
    check_pairs(rx, cohort, "DRUG", RX_MIN, [(ref_prep.normalize_drug_name, [k for c, k in CASES["rx"] if c]),
                                             (lambda t: t, [k for c, k in CASES["rx"] if not c])], "medications")
    names = [n for _, (_, ns) in DRUGS.items() for n in ns]
    low = " ".join(names).lower()
    for token in ("mg", "mcg", "ml", " g", "%", "unit", "units", "tablet", "capsule", "injection", "solution", "suspension",
                  "syrup", "cream", "ointment", "oral", "topical", "iv", "intravenous", "subcutaneous", "(", "-", ",", "/", "."):
        assert token in low, f"no drug name with {token!r}"
    assert all(ref_prep.normalize_drug_name(n) == "" for n in EMPTY_DRUGS), "names that normalise to nothing"
    for generic, (_, ns) in DRUGS.items():
        assert {ref_prep.normalize_drug_name(n) for n in ns} == {generic}, generic


def main():
    arrays, meta = {}, {"frames": {}, "cases": CASES, "min": {"labs": LAB_MIN, "dx": DX_MIN, "rx": RX_MIN}}
    cohort = make_cohort()
    select_ref.pack_frame("cohort", cohort, arrays, meta)
    for kind, seed in (("int", 41), ("str", 42)):
        labs = make_labs(seed)
        items = make_labitems(sorted(set(labs["ITEMID"])) + [50990, 50991])
        if kind == "str":
            labs["ITEMID"] = labs["ITEMID"].map(lambda i: f"lab_{i}")
            items["ITEMID"] = items["ITEMID"].map(lambda i: f"lab_{i}")
        check_labs(labs, cohort)
        select_ref.pack_frame(f"{kind}/labevents", labs, arrays, meta)
        select_ref.pack_frame(f"{kind}/d_labitems", items, arrays, meta)
        for k in CASES["labs"]:
            got, sel = ref_io.filter_labs_for_cohort(labs, cohort, items, top_k=k, min_patient_count=LAB_MIN)
            assert len(sel) == (k if k is not None else len(sel))
            select_ref.pack_frame(f"{kind}/labs_top{k}", got, arrays, meta)
            select_ref.pack_frame(f"{kind}/labitems_top{k}", sel, arrays, meta)
    dx = make_dx()
    check_dx(dx, cohort)
    select_ref.pack_frame("dx/in", dx, arrays, meta)
    for collapse, k in CASES["dx"]:
        select_ref.pack_frame(f"dx/out_{int(collapse)}_top{k}", ref_prep.process_diagnoses(dx, cohort, collapse, k, DX_MIN),
                              arrays, meta)
    select_ref.pack_frame("dx/out_bare", ref_prep.process_diagnoses(dx[["SUBJECT_ID", "HADM_ID", "ICD9_CODE"]], cohort, True,
                                                                   None, DX_MIN), arrays, meta)
    rx = make_rx()
    check_rx(rx, cohort)
    select_ref.pack_frame("rx/in", rx, arrays, meta)
    for norm, k in CASES["rx"]:
        select_ref.pack_frame(f"rx/out_{int(norm)}_top{k}", ref_prep.process_medications(rx, cohort, norm, k, RX_MIN), arrays,
                              meta)
    raw = sorted({n for _, (_, ns) in DRUGS.items() for n in ns} | set(EMPTY_DRUGS) | {"nan", "None", "Heparin Sodium 25,000 units in 0.45% NaCl"})
    arrays["drug/raw"] = np.array(raw, dtype="U64")
    arrays["drug/normalized"] = np.array([ref_prep.normalize_drug_name(n) for n in raw], dtype="U64")
    meta["drug_missing"] = [ref_prep.normalize_drug_name(np.nan), ref_prep.normalize_drug_name(None)]
    np.savez_compressed(OUT, __meta__=np.array(json.dumps(meta)), **arrays)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1024:.1f} KiB, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
