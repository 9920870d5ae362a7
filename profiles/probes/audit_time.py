"""Leakage-audit timings at the eICU shape (synth.make_graph, the test split of an EdgeMasker), per scale:
  (a) compute_robust_metrics on the device (mmg_order_stats + mmg_robust_sums + the copy of 15 doubles) against the
      copy of (y_true, y_pred) to the host + the reference's numpy arithmetic, over the test pairs (the predictions are
      synthetic: target + noise, the arithmetic does not depend on where they come from);
  (b) PatientHoldoutSplitter (one vectorised lookup) against the reference's loop `p.item() in set` per edge and split,
      timed on a sub-sample of --loop-sample edges and EXTRAPOLATED linearly to all edges x 3 masks;
  (c) audit_patient_leakage on the device (mmg_split_membership) against the reference's Python sets (x100 and below).
Device times: host clock around work that ends in a device synchronise (the robust metrics end in a host copy anyway);
medians over --reps after --warmup calls.

  python profiles/probes/audit_time.py --scales 100 1000 --out <dir>/audit_time.json
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
from mmgnn import audit  # noqa: E402
from mmgnn.synth import make_graph  # noqa: E402
from mmgnn.train import LAB_EDGE, EdgeMasker  # noqa: E402
import audit_ref  # noqa: E402


def clock(fn, reps, warmup, sync=True):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--loop-sample", type=int, default=200_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "numpy": np.__version__, "scales": {}}
    for s in a.scales:
        g = make_graph(s, seed=0, device=dev)
        ei = g[LAB_EDGE].edge_index
        em = EdgeMasker(g, 0.7, 0.15, 0.15, 0.2, 42)
        yt = g[LAB_EDGE].edge_attr.reshape(-1)[em.test_mask].contiguous()
        yp = (yt + 0.3 * torch.randn(yt.numel(), device=dev, generator=torch.Generator(dev).manual_seed(1))).contiguous()
        r = {"edges": int(ei.shape[1]), "test_pairs": int(yt.numel()), "patients": int(g["patient"].num_nodes)}

        dev_ms, dev_all = clock(lambda: audit.compute_robust_metrics(yt, yp), a.reps, a.warmup)

        def host():
            audit_ref.robust_metrics_f32(yt.cpu().numpy(), yp.cpu().numpy())
        host_ms, host_all = clock(host, a.host_reps, 1)
        r["robust_metrics"] = {"device_ms": dev_ms, "device_all_ms": dev_all, "copy_plus_numpy_ms": host_ms,
                               "copy_plus_numpy_all_ms": host_all, "speedup": host_ms / dev_ms}

        vec_ms, vec_all = clock(lambda: audit.PatientHoldoutSplitter(g, 0.7, 0.15, 0.15, seed=42), a.host_reps, 1)
        hs = audit.PatientHoldoutSplitter(g, 0.7, 0.15, 0.15, seed=42)
        k = min(a.loop_sample, int(ei.shape[1]))
        sub = ei[0][:k].cpu()
        t0 = time.perf_counter()
        audit_ref.holdout_masks_loop(sub, hs.train_patients, hs.val_patients, hs.test_patients)
        loop_s = time.perf_counter() - t0
        per_check_us = loop_s / (3 * k) * 1e6
        r["holdout_split"] = {"vectorised_ms": vec_ms, "vectorised_all_ms": vec_all, "loop_sample_edges": k,
                              "loop_sample_s": loop_s, "loop_us_per_check": per_check_us,
                              "loop_all_edges_s_EXTRAPOLATED": per_check_us * 3 * int(ei.shape[1]) / 1e6}

        m = (em.train_mask, em.val_mask, em.test_mask)
        pl_ms, pl_all = clock(lambda: audit.audit_patient_leakage(ei, *m), a.reps, a.warmup)
        r["patient_leakage"] = {"device_ms": pl_ms, "device_all_ms": pl_all}
        if s <= 100:                 # the sets of ~40 M Python ints at x1000 would need tens of GB of host memory
            ei_np = ei.cpu().numpy()
            m_np = [t.cpu().numpy() for t in m]
            t0 = time.perf_counter()
            audit_ref.patient_sets_report(ei_np, *m_np)
            r["patient_leakage"]["python_sets_s"] = time.perf_counter() - t0
        res["scales"][str(s)] = r
        print(json.dumps({s: r}), flush=True)
        del g, ei, em, yt, yp, hs
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
