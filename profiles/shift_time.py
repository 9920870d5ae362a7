"""Cohort-shift timings at the eICU shape (synth.make_graph): the patients are split 70 / 15 / 15 by a seeded permutation
on the device, cohort A is the has_lab pairs of the train patients, cohort B those of the test patients (the validation
patients' pairs are left out beforehand), the unit is the patient, everything already on the device.
  two_sample   mmgnn.shift.two_sample end to end (host clock around a device synchronise): thresholds, statistics, finish,
               summary, the read-back and the frame
  kernels      the four calls alone between device events.  mmg_shift_stats is held against an INTEGER ISSUE bound: one
               hash per kept pair, replicate and pass (two passes: counting and statistics), a hash counted as its two
               v_mul_lo_u32 at quarter rate (8 issue slots) and the 7 xors and shifts around them (15 slots), on
               256 CUs x 4 SIMDs x 16 lanes at the data sheet's 2.4 GHz
  host         the copy of the pairs to the host plus the float64 restatement of the same module (numpy, this machine's
               CPUs) on --host-replicates replicates; scaled to the full count and marked EXTRAPOLATED when that is fewer
Medians over --reps after --warmup calls.

  python profiles/shift_time.py --scales 1 100 1000 --out profiles/shift_time.json
"""
import argparse
import json
import os
import platform
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import mmgnn  # noqa: E402,F401
from mmgnn import shift as sh  # noqa: E402
from mmgnn import shift_ops as so  # noqa: E402
from mmgnn.synth import make_graph  # noqa: E402
from mmgnn.train import LAB_EDGE  # noqa: E402

LANES, CLOCK_HZ, HASH_SLOTS, PASSES = 256 * 4 * 16, 2.4e9, 15, 2


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


def event_clock(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="+", default=[1, 100, 1000])
    ap.add_argument("--replicates", type=int, default=1000)
    ap.add_argument("--host-replicates", type=int, nargs="+", default=[63, 7, 1], help="one per scale")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    R = a.replicates
    res = {"device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "numpy": np.__version__, "replicates": R, "unit": "patient", "chunk": so.SHIFT_CHUNK,
           "replicates_per_workgroup": so.SHIFT_RB,
           "integer_issue_bound": {"lanes": LANES, "clock_hz": CLOCK_HZ, "slots_per_hash": HASH_SLOTS, "passes": PASSES},
           "host_threads": {"torch": torch.get_num_threads(), "OMP_NUM_THREADS": os.environ.get("OMP_NUM_THREADS")},
           "scales": {}}
    for s, host_r in zip(a.scales, a.host_replicates):
        g = make_graph(s, seed=0, device=dev)
        ei = g[LAB_EDGE].edge_index
        y = g[LAB_EDGE].edge_attr.reshape(-1).float()
        L, P = int(g["lab"].num_nodes), int(g["patient"].num_nodes)
        gen = torch.Generator(dev).manual_seed(1)
        perm = torch.randperm(P, device=dev, generator=gen)
        group = torch.full((P,), 2, dtype=torch.uint8, device=dev)
        group[perm[:int(0.7 * P)]] = 1
        group[perm[int(0.85 * P):]] = 0
        sel = group[ei[0]] <= 1
        pi, li, v = ei[0][sel].contiguous(), ei[1][sel].contiguous(), y[sel].contiguous()
        n = int(v.numel())
        r = {"pairs": n, "patients": P, "labs": L, "index_bytes": 8}
        print(f"x{s}: {n} pairs, {P} patients, {L} labs", flush=True)

        ms, allms = host_clock(lambda: sh.two_sample(v, li, pi, group, L, replicates=R), a.reps, a.warmup)
        r["two_sample"] = {"ms": ms, "all_ms": allms}
        out = sh.two_sample(v, li, pi, group, L, replicates=R)
        r["overall"] = {k: out.overall[k] for k in ("max_z", "p", "n_units", "n_units_a", "dropped")}
        r["labs_with_p_adjusted_at_most_0.05"] = len(out.overall["shifted_labs"])

        k = {}
        T, cohort = so.shift_thresholds(group, R, 0)
        ms, allms = event_clock(lambda: so.shift_thresholds(group, R, 0, out=(T, cohort)), a.reps, a.warmup)
        k["thresholds"] = {"ms": ms, "all_ms": allms, "hashes": 8 * R * int(cohort[0])}
        tabs = so.shift_stats(v, li, pi, group, L, T, 0)
        ms, allms = event_clock(lambda: so.shift_stats(v, li, pi, group, L, T, 0, out=tabs), a.reps, a.warmup)
        hashes = n * (R + 1) * PASSES
        bound_ms = hashes * HASH_SLOTS / (LANES * CLOCK_HZ) * 1e3
        k["stats"] = {"ms": ms, "all_ms": allms, "label_evaluations": hashes, "integer_issue_bound_ms": bound_ms,
                      "fraction_of_bound": bound_ms / ms,
                      "workspace_bytes": int(so.load().mmg_shift_stats_ws_bytes(n, L, R))}
        stats = so.shift_finish(tabs[0], tabs[1], cohort)
        ms, allms = event_clock(lambda: so.shift_finish(tabs[0], tabs[1], cohort, out=stats), a.reps, a.warmup)
        k["finish"] = {"ms": ms, "all_ms": allms}
        summary = so.shift_summary(stats)
        ms, allms = event_clock(lambda: so.shift_summary(stats, out=summary), a.reps, a.warmup)
        k["summary"] = {"ms": ms, "all_ms": allms}
        r["kernels"] = k
        print(json.dumps({s: r}), flush=True)

        # the copy to the host and the host path of the same module on the same pairs, fewer replicates
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hv, hl, hp, hg = (x.cpu().numpy() for x in (v, li, pi, group))
        copy_sec = time.perf_counter() - t0
        t0 = time.perf_counter()
        ht = sh.shift_tables(hv, hl, hp, hg, L, host_r, 0)
        sec = time.perf_counter() - t0
        d = so.shift_stats(v, li, pi, group, L, so.shift_thresholds(group, host_r, 0)[0], 0)
        assert np.array_equal(d[0].cpu().numpy(), ht["counts"])
        r["host"] = {"replicates_timed": host_r, "copy_seconds": copy_sec, "seconds": sec,
                     "seconds_at_full_replicates": copy_sec + sec * (R + 1) / (host_r + 1), "EXTRAPOLATED": host_r < R,
                     "sums_bitwise_equal_to_device": bool(np.array_equal(d[1].cpu().numpy(), ht["sums"]))}
        res["scales"][str(s)] = r
        print(json.dumps({s: r["host"]}), flush=True)
        del g, ei, y, pi, li, v, tabs, stats, summary, d, T
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
