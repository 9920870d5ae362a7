"""Lab-preprocessing timings on synth.make_lab_events, per scale:
  tensor_ms   preprocess_lab_events on device tensors (last / outlier removal on / zscore), host clock around a device
              synchronise, median over --reps after --warmup calls;
  frame_ms    aggregate_lab_values + normalize_lab_values on the frames (host factorisation and copies included),
              with host_prep_ms = the factorisation / conversion of the key and time columns alone;
  kernels     per-kernel totals of ONE tensor-level call from a `rocprofv3 --kernel-trace --stats` child run;
  reference   the pandas path (tests/prep_ref.py: the reference's own Series reductions, 16 host threads) on the same
              box, measured up to --ref-max-scale and EXTRAPOLATED linearly in the events above it.
Every GPU step is a child process under its own `timeout`; a failed step ends the run.

  python profiles/probes/prep_time.py --scales 1 10 100 --out profiles/prep_time_x1_x10_x100.json
"""
import argparse
import csv
import glob
import json
import os
import platform
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "tests"))


def clock(fn, reps, warmup):
    import torch
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


def measure(scale, reps, warmup, with_ref):
    import torch
    import mmgnn  # noqa: F401
    from mmgnn import preprocess
    from mmgnn.synth import lab_event_frames, make_lab_events
    import prep_ref
    ev = make_lab_events(scale, seed=0, device="cuda:0")
    args = (ev["patient"], ev["lab"], ev["value"], ev["time"], ev["n_patients"], ev["n_labs"])
    out = preprocess.preprocess_lab_events(*args)
    r = {"events": int(ev["patient"].numel()), "pairs": int(out[0].numel())}
    r["tensor_ms"], r["tensor_all_ms"] = clock(lambda: preprocess.preprocess_lab_events(*args), reps, warmup)
    labs, cohort = lab_event_frames(ev)

    def frames():
        return preprocess.normalize_lab_values(preprocess.aggregate_lab_values(labs, cohort, "last", True, 5.0), "zscore")
    r["frame_ms"], r["frame_all_ms"] = clock(frames, max(reps // 3, 2), 1)

    def host_prep():
        import numpy as np
        ids = np.unique(cohort["SUBJECT_ID"].to_numpy())
        np.searchsorted(ids, labs["SUBJECT_ID"].to_numpy())
        preprocess._factorize_sorted(labs["ITEMID"])
        preprocess._time_codes(labs["CHARTTIME"])
    t0 = time.perf_counter()
    host_prep()
    r["host_prep_ms"] = (time.perf_counter() - t0) * 1e3
    if with_ref:
        torch.set_num_threads(16)
        ts = []
        for _ in range(2):
            t0 = time.perf_counter()
            prep_ref.normalize(prep_ref.aggregate(labs, cohort, "last", True, 5.0), "zscore")
            ts.append(time.perf_counter() - t0)
        r["reference_s"] = min(ts)
    return r


def one_call(scale):
    import torch
    import mmgnn  # noqa: F401
    from mmgnn import preprocess
    from mmgnn.synth import make_lab_events
    ev = make_lab_events(scale, seed=0, device="cuda:0")
    preprocess.preprocess_lab_events(ev["patient"], ev["lab"], ev["value"], ev["time"], ev["n_patients"], ev["n_labs"])
    torch.cuda.synchronize()


def kernel_stats(scale, limit):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d,
               "--", sys.executable, os.path.abspath(__file__), "--one-call", str(scale)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        rows = {}
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                name = row["Name"].split("(anonymous namespace)::")[-1].split("(")[0]
                if name.startswith(("k_ps_", "k_radix_", "k_ls_", "k_lq", "k_lt", "k_ag_", "k_lab_ptr", "k_scan", "mmg_k_zero")):
                    e = rows.setdefault(name, {"calls": 0, "total_us": 0.0})
                    e["calls"] += int(row["Calls"])
                    e["total_us"] += int(row["TotalDurationNs"]) / 1e3
        return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="+", default=[1, 10, 100])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ref-max-scale", type=int, default=10)
    ap.add_argument("--step-limit", type=int, default=420)
    ap.add_argument("--out", default=None)
    ap.add_argument("--measure", type=int, default=None)
    ap.add_argument("--one-call", type=int, default=None)
    a = ap.parse_args()
    if a.one_call is not None:
        return one_call(a.one_call)
    if a.measure is not None:
        print("RESULT " + json.dumps(measure(a.measure, a.reps, a.warmup, a.measure <= a.ref_max_scale)), flush=True)
        return
    res = {"host": platform.node(), "config": "aggregate=last, outlier_threshold=5.0, normalize=zscore", "scales": {}}
    for s in a.scales:
        cmd = ["timeout", "-k", "10", str(a.step_limit), sys.executable, os.path.abspath(__file__), "--measure", str(s),
               "--reps", str(a.reps), "--warmup", str(a.warmup), "--ref-max-scale", str(a.ref_max_scale)]
        p = subprocess.run(cmd, check=True, capture_output=True, text=True)
        r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        r["kernels"] = kernel_stats(s, a.step_limit)
        res["scales"][str(s)] = r
        print(json.dumps({s: r}), flush=True)
    measured = [(int(k), v) for k, v in res["scales"].items() if "reference_s" in v]
    if measured:
        k, v = max(measured)
        for s, r in res["scales"].items():
            if "reference_s" not in r:
                r["reference_s_EXTRAPOLATED"] = v["reference_s"] * r["events"] / v["events"]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
