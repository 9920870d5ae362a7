"""Feature-space selection timings on the synthetic tables, per scale and per table (labs: synth.make_lab_events with
valid = the value is not NaN, rows="all", 50 codes; diagnoses / medications: synth.make_code_events, rows="first",
2,162 / 2,148 codes):
  select_ms     mmgnn.preprocess.select_codes on device tensors -- host clock around a call that ends in the device
                synchronise the entry point itself does (its row count comes back); median over --reps after --warmup;
  lab_prep_ms   (labs only) preprocess_lab_events on the SAME events in the same run (last / outlier removal / zscore),
                and select_over_lab_prep = select_ms / lab_prep_ms;
  host          what a user has without the kernel: the device-to-host copy of the columns + the reference-equivalent
                pandas of tests/select_ref.py (filter_labs / diagnoses / medications on frames of the same rows) on the
                same box.  Above --host-max-rows rows the pandas runs on the first --host-max-rows rows (the rows are
                shuffled: a uniform sample) and the figure is EXTRAPOLATED linearly in the row count (marked in the JSON);
                the copy is always timed in full.
The top_k / min_patient_count are the reference configuration's (labs 50 -> 30 at >= 10 patients; diagnoses top 100,
medications top 80 at >= 5 patients).

  python profiles/probes/select_time.py --scales 1 10 100 --out profiles/select_time_x1_x10_x100.json
"""
import argparse
import json
import os
import platform
import statistics
import sys
import time

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import mmgnn  # noqa: E402,F401
from mmgnn import preprocess  # noqa: E402
from mmgnn.synth import make_code_events, make_lab_events  # noqa: E402
import select_ref  # noqa: E402

SETTINGS = {"lab": dict(top_k=30, min_patient_count=10, rows="all"),
            "diagnosis": dict(top_k=100, min_patient_count=5, rows="first"),
            "medication": dict(top_k=80, min_patient_count=5, rows="first")}


def host_clock(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


def pandas_ms(kind, patient, code, valid, n_patients, m, reps):
    """The pandas path on the first m rows (ids are the codes; one admission per patient)."""
    sid = patient[:m]
    cohort = pd.DataFrame({"SUBJECT_ID": np.arange(n_patients, dtype=np.int64),
                           "HADM_ID": np.arange(n_patients, dtype=np.int64) + 10 ** 9})
    s = SETTINGS[kind]
    if kind == "lab":
        frame = pd.DataFrame({"SUBJECT_ID": sid, "ITEMID": code[:m], "VALUENUM": np.where(valid[:m] != 0, 1.0, np.nan)})
        items = pd.DataFrame({"ITEMID": np.unique(code[:m])})
        fn = lambda: select_ref.filter_labs(frame, cohort, items, s["top_k"], s["min_patient_count"])   # noqa: E731
    else:
        col = "ICD9_CODE" if kind == "diagnosis" else "DRUG"
        names = np.array([f"c{c:07d}" for c in range(int(code.max()) + 1)], dtype=object)              # no collapse, no rules:
        frame = pd.DataFrame({"SUBJECT_ID": sid, "HADM_ID": sid + 10 ** 9, col: names[code[:m]]})       # the counting alone
        if kind == "diagnosis":
            fn = lambda: select_ref.diagnoses(frame, cohort, False, s["top_k"], s["min_patient_count"])    # noqa: E731
        else:
            fn = lambda: select_ref.medications(frame, cohort, False, s["top_k"], s["min_patient_count"])  # noqa: E731
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="+", default=[1, 10, 100])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--host-max-rows", type=int, default=4_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "numpy": np.__version__, "pandas": pd.__version__, "settings": SETTINGS, "scales": {}}
    for s in a.scales:
        res["scales"][str(s)] = {}
        for kind in ("lab", "diagnosis", "medication"):
            if kind == "lab":
                ev = make_lab_events(s, seed=0, device=dev)
                patient, code, n_codes = ev["patient"], ev["lab"], ev["n_labs"]
                valid = (~torch.isnan(ev["value"])).to(torch.uint8)
            else:
                ev = make_code_events(s, seed=0, device=dev, kind=kind)
                patient, code, n_codes, valid = ev["patient"], ev["code"], ev["n_codes"], None
            P, n = ev["n_patients"], int(patient.numel())
            st = SETTINGS[kind]
            call = lambda: preprocess.select_codes(patient, code, P, n_codes, valid=valid, **st)   # noqa: E731
            out = call()
            r = {"rows": n, "patients": P, "codes": n_codes, "selected": int(out[3].sum()), "kept_rows": int(out[4].numel())}
            r["select_ms"], r["select_all_ms"] = host_clock(call, a.reps, a.warmup)
            if kind == "lab":
                args = (ev["patient"], ev["lab"], ev["value"], ev["time"], P, n_codes)
                r["lab_prep_ms"], r["lab_prep_all_ms"] = host_clock(lambda: preprocess.preprocess_lab_events(*args), a.reps,
                                                                     a.warmup)
                r["select_over_lab_prep"] = r["select_ms"] / r["lab_prep_ms"]
            cols = [patient, code] + ([valid] if valid is not None else [])
            copy_ms, copy_all = host_clock(lambda: [x.cpu() for x in cols], a.host_reps, 1)
            hp, hc = patient.cpu().numpy(), code.cpu().numpy()
            hv = valid.cpu().numpy() if valid is not None else None
            m = min(n, a.host_max_rows)
            t = pandas_ms(kind, hp, hc, hv, P, m, a.host_reps)
            r["host"] = {"copy_ms": copy_ms, "copy_all_ms": copy_all, "pandas_ms": t * (n / m), "pandas_rows_timed": m,
                         "pandas_EXTRAPOLATED": m < n, "copy_plus_pandas_ms": copy_ms + t * (n / m)}
            r["speedup"] = r["host"]["copy_plus_pandas_ms"] / r["select_ms"]
            res["scales"][str(s)][kind] = r
            print(json.dumps({s: {kind: r}}), flush=True)
            del ev, patient, code, valid, hp, hc, hv, out
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
