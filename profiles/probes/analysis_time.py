"""Prediction-analysis timings at the eICU shape (synth.make_graph), over ALL has_lab pairs with the predictions already
on the device (synthetic: target * slope_lab + offset_lab + noise; the arithmetic does not depend on their origin):
  (a) the device path end to end (mmgnn.analysis.analysis_tables: two launches, the small copies, the host assembly of
      the three tables) -- host clock around work that ends in a device synchronise;
  (b) each kernel alone (device events around the one entry point) and its fraction of the 8 TB/s HBM roofline on
      ALGORITHMIC bytes: n * (8 + 2 * index bytes) for the pairs + 4 * N_P for the degrees, each counted once (both
      reads touch every column when labs and bins are requested together);
      The synthetic has_lab edges are lab-major (what the reference's parquet yields): a lane's run of equal labs is
      long and flushes are rare.  The same two kernels are timed again on a seeded SHUFFLE of the pairs, where every
      pair flushes and the lanes take turns per lab ("shuffled_order" in the JSON; mmg_seg_metrics too);
  (c) mmg_seg_metrics on the same pred / target / lab in the same run, on its own algorithmic bytes (n * 16);
  (d) what a user has without the kernels: copy pred, target, patient, lab to the host + the float64 tables of
      tests/analysis_ref.py.  Above --host-max-pairs pairs the host tables run on every k-th pair (all labs and bins
      stay present) and the figure is EXTRAPOLATED linearly in the pair count (marked in the JSON); the copy is always
      timed in full.
Medians over --reps after --warmup calls.

  python profiles/probes/analysis_time.py --scales 1 100 1000 --out <dir>/analysis_time.json
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
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import mmgnn  # noqa: E402,F401
from mmgnn import analysis, ops  # noqa: E402
from mmgnn.data import build_plan  # noqa: E402
from mmgnn.synth import make_graph  # noqa: E402
from mmgnn.train import LAB_EDGE  # noqa: E402
import analysis_ref  # noqa: E402

HBM_BYTES_PER_S = 8e12
EDGES = (0.0, 1.0, 6.0, 16.0, 50.0)


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--host-max-pairs", type=int, default=8_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "numpy": np.__version__, "hbm_roofline_bytes_per_s": HBM_BYTES_PER_S, "scales": {}}
    for s in a.scales:
        g = make_graph(s, seed=0, device=dev)
        ei = g[LAB_EDGE].edge_index
        pi, li = ei[0].contiguous(), ei[1].contiguous()
        t = g[LAB_EDGE].edge_attr.reshape(-1).contiguous()
        L, P, n = int(g["lab"].num_nodes), int(g["patient"].num_nodes), int(t.numel())
        gen = torch.Generator(dev).manual_seed(1)
        slope = 0.7 + 0.6 * torch.rand(L, device=dev, generator=gen)
        offset = 0.3 * torch.randn(L, device=dev, generator=gen)
        p = (t * slope[li] + offset[li] + 0.2 * torch.randn(n, device=dev, generator=gen)).contiguous()
        deg = build_plan(g, dev).lab_deg
        r = {"pairs": n, "patients": P, "labs": L, "index_bytes": 8}

        e2e_ms, e2e_all = host_clock(lambda: analysis.analysis_tables(p, t, pi, li, deg, n_labs=L), a.reps, a.warmup)
        r["device_end_to_end_ms"], r["device_end_to_end_all_ms"] = e2e_ms, e2e_all

        ls, bs = ops.pair_analysis(p, t, li, L, pi, deg, EDGES)
        ca, cb = analysis._line32(*analysis.calibration_line(ls.cpu().numpy()))
        ca, cb = torch.from_numpy(ca).to(dev), torch.from_numpy(cb).to(dev)
        bm = torch.from_numpy(analysis.bin_means(bs.cpu().numpy())).to(dev)
        algo = n * (8 + 2 * 8) + 4 * P
        for name, fn in (("pass1_pair_analysis", lambda: ops.pair_analysis(p, t, li, L, pi, deg, EDGES)),
                         ("pass2_pair_calibrated_abs",
                          lambda: ops.pair_calibrated_abs(p, t, li, ca, cb, pi, deg, EDGES, bm))):
            ms, allms = event_clock(fn, a.reps, a.warmup)
            r[name] = {"ms": ms, "all_ms": allms, "algorithmic_bytes": algo,
                       "roofline_fraction": algo / (ms * 1e-3) / HBM_BYTES_PER_S}
        ms, allms = event_clock(lambda: ops.seg_sums(p, t, li, L), a.reps, a.warmup)
        r["seg_metrics"] = {"ms": ms, "all_ms": allms, "algorithmic_bytes": n * 16,
                            "roofline_fraction": n * 16 / (ms * 1e-3) / HBM_BYTES_PER_S}
        r["pass1_fraction_over_seg_metrics_fraction"] = (r["pass1_pair_analysis"]["roofline_fraction"] /
                                                         r["seg_metrics"]["roofline_fraction"])

        perm = torch.randperm(n, device=dev, generator=gen)
        qp, qt, qpi, qli = (x[perm].contiguous() for x in (p, t, pi, li))
        del perm
        sh = {}
        for name, fn, nbytes in (("pass1_pair_analysis", lambda: ops.pair_analysis(qp, qt, qli, L, qpi, deg, EDGES), algo),
                                 ("pass2_pair_calibrated_abs",
                                  lambda: ops.pair_calibrated_abs(qp, qt, qli, ca, cb, qpi, deg, EDGES, bm), algo),
                                 ("seg_metrics", lambda: ops.seg_sums(qp, qt, qli, L), n * 16)):
            ms, allms = event_clock(fn, a.reps, a.warmup)
            sh[name] = {"ms": ms, "all_ms": allms, "algorithmic_bytes": nbytes,
                        "roofline_fraction": nbytes / (ms * 1e-3) / HBM_BYTES_PER_S}
        sh["pass1_fraction_over_seg_metrics_fraction"] = (sh["pass1_pair_analysis"]["roofline_fraction"] /
                                                          sh["seg_metrics"]["roofline_fraction"])
        r["shuffled_order"] = sh
        del qp, qt, qpi, qli

        copy_ms, copy_all = host_clock(lambda: [x.cpu() for x in (p, t, pi, li)], a.host_reps, 1)
        hp, ht, hpi, hli = (x.cpu().numpy() for x in (p, t, pi, li))
        hdeg = deg.cpu().numpy()
        k = -(-n // a.host_max_pairs)
        sp, st, spi, sli = (np.ascontiguousarray(x[::k]) for x in (hp, ht, hpi, hli))
        m = int(sp.size)

        def host_tables():
            analysis_ref.calibration_f64(sp, st, sli)
            analysis_ref.degree_f64(sp, st, spi, hdeg)
            analysis_ref.deciles_f64(sp, st, sli)
        ts = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            host_tables()
            ts.append((time.perf_counter() - t0) * 1e3)
        tab_ms = statistics.median(ts) * (n / m)
        r["host"] = {"copy_ms": copy_ms, "copy_all_ms": copy_all, "tables_ms": tab_ms, "tables_pairs_timed": m,
                     "tables_EXTRAPOLATED": m < n, "copy_plus_tables_ms": copy_ms + tab_ms}
        r["speedup_end_to_end"] = (copy_ms + tab_ms) / e2e_ms
        res["scales"][str(s)] = r
        print(json.dumps({s: r}), flush=True)
        del g, ei, pi, li, t, p, deg, hp, ht, hpi, hli
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
