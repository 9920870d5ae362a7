"""Split-conformal timings at the eICU shape (synth.make_graph): the validation / test pairs are a seeded 15 % / 15 % of
the has_lab edges, the predictions synthetic (target * slope_lab + offset_lab + noise: the arithmetic does not depend on
their origin), already on the device.
  fit             mmgnn.conformal.LabConformal.fit on the validation pairs -- the mmg_cf_fit call alone (device events)
                  and the method end to end (host clock: with the small copies of the table)
  predict_matrix  mmg_cf_apply_matrix on the dense [N_P, 50] prediction matrix (device events) and its fraction of the
                  8 TB/s HBM roofline on 16 algorithmic bytes per cell, beside mmg_lab_inverse_matrix on the same matrix
                  in the same run (8 bytes per cell, the same access pattern)
  coverage        mmg_cf_coverage on the test pairs (device events)
Each beside what a user has without the kernels: the copy of the inputs to the host + the numpy path of this module.
Medians over --reps after --warmup calls; host figures over --host-reps.

  python profiles/probes/conformal_time.py --scales 100 1000 --out <dir>/conformal_time.json
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

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import mmgnn  # noqa: E402,F401
from mmgnn import conformal as cf  # noqa: E402
from mmgnn import conformal_ops as co  # noqa: E402
from mmgnn import ops  # noqa: E402
from mmgnn.data import build_plan  # noqa: E402
from mmgnn.synth import make_graph  # noqa: E402
from mmgnn.train import LAB_EDGE  # noqa: E402

HBM_BYTES_PER_S = 8e12


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
    ap.add_argument("--scales", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--matrix-scales", type=int, nargs="+", default=[100])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    edges = [float(e) for e in cf.DEFAULT_BINS]
    res = {"device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "numpy": np.__version__, "hbm_roofline_bytes_per_s": HBM_BYTES_PER_S, "alpha": 0.1, "score": "signed",
           "bins": [str(e) for e in edges], "scales": {}}
    for s in a.scales:
        g = make_graph(s, seed=0, device=dev)
        ei = g[LAB_EDGE].edge_index
        t_all = g[LAB_EDGE].edge_attr.reshape(-1)
        L, P, E = int(g["lab"].num_nodes), int(g["patient"].num_nodes), int(t_all.numel())
        gen = torch.Generator(dev).manual_seed(1)
        perm = torch.randperm(E, device=dev, generator=gen)
        n_split = int(0.15 * E)
        slope = 0.7 + 0.6 * torch.rand(L, device=dev, generator=gen)
        offset = 0.3 * torch.randn(L, device=dev, generator=gen)
        deg = build_plan(g, dev).lab_deg
        split = {}
        for name, idx in (("val", perm[:n_split]), ("test", perm[n_split:2 * n_split])):
            idx = idx.sort().values
            pi, li, t = ei[0][idx].contiguous(), ei[1][idx].contiguous(), t_all[idx].contiguous()
            p = (t * slope[li] + offset[li] + 0.2 * torch.randn(t.numel(), device=dev, generator=gen)).contiguous()
            split[name] = (p, t, pi, li)
        del perm
        r = {"pairs_per_split": n_split, "patients": P, "labs": L, "cells": L * (len(edges) - 1), "index_bytes": 8}

        p, t, pi, li = split["val"]
        ms, allms = event_clock(lambda: co.cf_fit(p, t, pi, li, L, deg, edges, 0.1, "signed", 0), a.reps, a.warmup)
        r["fit_kernels"] = {"ms": ms, "all_ms": allms}
        e2e, e2e_all = host_clock(lambda: cf.LabConformal().fit(p, t, li, pi, deg, n_labs=L), a.reps, a.warmup)
        r["fit_end_to_end_ms"], r["fit_end_to_end_all_ms"] = e2e, e2e_all
        obj = cf.LabConformal().fit(p, t, li, pi, deg, n_labs=L)
        copy_ms, _ = host_clock(lambda: [x.cpu() for x in (p, t, pi, li)], a.host_reps, 1)
        hp, ht, hpi, hli = (x.cpu().numpy() for x in (p, t, pi, li))
        hdeg = deg.cpu().numpy()
        ts = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            host = cf.LabConformal().fit(hp, ht, hli, hpi, hdeg, n_labs=L)
            ts.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(host.table, obj.table, equal_nan=True) and np.array_equal(host.level, obj.level)
        r["fit_host"] = {"copy_ms": copy_ms, "numpy_ms": statistics.median(ts), "copy_plus_numpy_ms": copy_ms + statistics.median(ts)}
        r["fit_speedup_end_to_end"] = r["fit_host"]["copy_plus_numpy_ms"] / e2e
        r["levels"] = {cf.LEVELS[k]: int((obj.level == k).sum()) for k in range(4)}

        p, t, pi, li = split["test"]
        table = obj._on(dev)[0]
        ms, allms = event_clock(lambda: co.cf_coverage(p, t, pi, li, L, deg, edges, table), a.reps, a.warmup)
        r["coverage_kernels"] = {"ms": ms, "all_ms": allms}
        copy_ms, _ = host_clock(lambda: [x.cpu() for x in (p, t, pi, li)], a.host_reps, 1)
        hp, ht, hpi, hli = (x.cpu().numpy() for x in (p, t, pi, li))
        ts = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            hc = host.coverage_counts(hp, ht, hli, hpi)
            ts.append((time.perf_counter() - t0) * 1e3)
        dc = obj.coverage_counts(p, t, li, pi)
        assert np.array_equal(hc[0], dc[0])
        r["coverage_host"] = {"copy_ms": copy_ms, "numpy_ms": statistics.median(ts), "copy_plus_numpy_ms": copy_ms + statistics.median(ts)}
        r["coverage_overall"] = float(dc[0][:-1, 1].sum() / dc[0][:-1, 0].sum())

        if s in a.matrix_scales:
            gen2 = torch.Generator(dev).manual_seed(2)
            m = torch.randn(P, L, device=dev, generator=gen2)
            outs = tuple(torch.empty_like(m) for _ in range(3))
            cells = P * L
            ms, allms = event_clock(lambda: co.cf_apply_matrix(m, None, deg, edges, table, False, out=outs), a.reps, a.warmup)
            r["predict_matrix"] = {"rows": P, "ms": ms, "all_ms": allms, "algorithmic_bytes": 16 * cells,
                                   "roofline_fraction": 16 * cells / (ms * 1e-3) / HBM_BYTES_PER_S}
            stats = torch.zeros(L, ops.LAB_STAT_FIELDS, dtype=torch.float64, device=dev)
            stats[:, 1], stats[:, 2] = 1.5, 2.0
            inv = torch.empty_like(m)
            ms, allms = event_clock(lambda: ops.lab_inverse_matrix(m, stats, "zscore", out=inv), a.reps, a.warmup)
            r["lab_inverse_matrix"] = {"ms": ms, "all_ms": allms, "algorithmic_bytes": 8 * cells,
                                       "roofline_fraction": 8 * cells / (ms * 1e-3) / HBM_BYTES_PER_S}
            copy_ms, _ = host_clock(lambda: m.cpu(), a.host_reps, 1)
            hm = m.cpu().numpy()
            ts = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter()
                hw = host.predict_matrix(hm)
                ts.append((time.perf_counter() - t0) * 1e3)
            assert all(np.array_equal(o.cpu().numpy(), w, equal_nan=True) for o, w in zip(outs, hw))
            r["predict_matrix_host"] = {"copy_ms": copy_ms, "numpy_ms": statistics.median(ts),
                                        "copy_plus_numpy_ms": copy_ms + statistics.median(ts)}
            del m, outs, inv, hm, hw
        res["scales"][str(s)] = r
        print(json.dumps({s: r}), flush=True)
        del g, ei, t_all, split, p, t, pi, li, deg
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
