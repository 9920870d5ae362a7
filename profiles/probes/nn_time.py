"""Neighbour search and map-quality timings (mmgnn.neighbors, csrc/nn.hip) for 128-wide fp32 rows already on the device.
Synthetic rows: five L2-normalised clusters, tests/tsne_ref.make_case's recipe (unit norm, as the initial patient
embeddings are); the map scored is the rows' 2-component PCA projection (mmgnn.embed.pca).
  (a) nearest_neighbors, self mode, k = 10, at the patient counts of the x1, x10 and x100 graphs (1,834 / 18,340 /
      183,400 rows): a host clock around the call and a device synchronise, the search kernel alone from the library's
      probe, and that kernel's fraction of the fp64 vector issue bound;
  (b) trustworthiness (k = 5) at n = 1,000, 16,384 and the x100 count: the search in the map, the rank pass in the
      128-wide space and the read of the penalty, end to end; the rank kernel alone and its fraction of the bound;
  (c) beside those, on the same box and its thread limit: sklearn NearestNeighbors(algorithm="brute").kneighbors() and
      sklearn.manifold.trustworthiness.  Above --sklearn-nn-max / --sklearn-trust-max rows sklearn is not run: its figure
      is EXTRAPOLATED from the largest n that was run by (n / n_run)^2 (both are n^2 D work; the argsort's log n is left
      out, so the extrapolation flatters sklearn) and labelled so.
The bound: 2 fp64 lane-operations (a subtraction and an fma) per pair and column.  MI355X_MICROARCH.md gives the fp32 vector
peak as 157.3 TFLOPS = 256 CUs x 4 SIMDs x 2.4 GHz x 64 FLOP per clock, i.e. 32 fp32 fma lanes per SIMD and clock; the
fp64 vector rate of CDNA4 is half of it (78.6 TFLOPS in AMD's specification), 16 lane-operations per SIMD and clock:
256 x 4 x 16 x 2.4e9 = 3.93e13 lane-operations per second.
Medians over --reps after --warmup calls.  Reported figures, not thresholds.

  python profiles/probes/nn_time.py --out profiles/nn_time.json
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

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mmgnn  # noqa: E402,F401
from mmgnn import embed, neighbors as nb, nn_ops, ops  # noqa: E402
import tsne_ref as tr  # noqa: E402

FP64_LANE_OPS_PER_S = 256 * 4 * 16 * 2.4e9
PATIENTS_X1 = 1834


def wall_ms(fn, reps, warmup):
    ts = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


def kernel_ms(fn, n_launches, reps):
    """-> {kernel symbol: median ms} from the library's probe (each launch carries its own event pair)."""
    rows = {}
    for _ in range(reps):
        torch.cuda.synchronize()
        ops.probe_arm(n_launches)
        fn()
        torch.cuda.synchronize()
        for ms, _, _, _, _, flags, sym in ops.probe_read():
            rows.setdefault(sym, []).append(ms)
    ops.probe_arm(0)
    return {k: statistics.median(v) for k, v in rows.items()}


def of_bound(n, D, ms):
    return 2.0 * n * n * D / (ms * 1e-3) / FP64_LANE_OPS_PER_S


def host_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="+", default=[1, 10, 100])
    ap.add_argument("--trust-sizes", type=int, nargs="+", default=[1000, 16384, 100 * PATIENTS_X1])
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--trust-k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sklearn-nn-max", type=int, default=10 * PATIENTS_X1, help="0: skip the sklearn runs")
    ap.add_argument("--sklearn-trust-max", type=int, default=16384)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    D = a.dim
    res = {"device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "numpy": np.__version__, "D": D, "fp64_lane_ops_per_s_bound": FP64_LANE_OPS_PER_S,
           "threads": torch.get_num_threads(), "OMP_NUM_THREADS": os.environ.get("OMP_NUM_THREADS"),
           "nearest_neighbors": {}, "trustworthiness": {}}
    sk_nn, sk_tr = None, None                                      # (n, ms) of the largest sklearn run
    for scale in a.scales:
        n = scale * PATIENTS_X1
        xh = tr.make_case(n, D)
        x = torch.from_numpy(xh).to(dev)
        r = {"n": n, "k": a.k, "plan_ranges_items_workgroups": nn_ops.nn_plan(n)}
        r["ms"], r["all_ms"] = wall_ms(lambda: nb.nearest_neighbors(x, a.k), a.reps, a.warmup)
        kt = kernel_ms(lambda: nn_ops.nn_search(x, a.k), 2, a.reps)
        r["kernels_ms"] = kt
        ks = next(v for s, v in kt.items() if "k_nn_search" in s)
        r["search_kernel"] = {"ms": ks, "fraction_of_fp64_issue_bound": of_bound(n, D, ks), "label": "measured"}
        if a.sklearn_nn_max and n <= a.sklearn_nn_max:
            from sklearn.neighbors import NearestNeighbors
            x64 = xh.astype(np.float64)
            ms = host_ms(lambda: NearestNeighbors(n_neighbors=a.k, algorithm="brute").fit(x64).kneighbors())
            sk_nn = (n, ms)
            r["sklearn_brute"] = {"ms": ms, "label": "measured"}
        elif sk_nn:
            r["sklearn_brute"] = {"ms": sk_nn[1] * (n / sk_nn[0]) ** 2,
                                  "label": f"extrapolated from n = {sk_nn[0]} by (n / n_run)^2"}
        res["nearest_neighbors"][f"x{scale}"] = r
        print(json.dumps({f"nn x{scale}": r}), flush=True)
        del x
        torch.cuda.empty_cache()
    for n in a.trust_sizes:
        xh = tr.make_case(n, D)
        x = torch.from_numpy(xh).to(dev)
        y = embed.pca(x, 2).projection.contiguous()
        k = a.trust_k
        r = {"n": n, "k": k, "map": "pca, 2 components"}
        val = [None]

        def run():
            val[0] = nb.trustworthiness(x, y, k)
        r["ms"], r["all_ms"] = wall_ms(run, a.reps, a.warmup)
        r["value"] = val[0]
        idx = nb.nearest_neighbors(y, k).indices
        kt = kernel_ms(lambda: nn_ops.nn_rank(x, idx, False, True), 1, a.reps)
        kr = next(v for s, v in kt.items() if "k_nn_rank" in s)
        r["rank_kernel"] = {"ms": kr, "fraction_of_fp64_issue_bound": of_bound(n, D, kr), "label": "measured"}
        if a.sklearn_trust_max and n <= a.sklearn_trust_max:
            from sklearn.manifold import trustworthiness
            x64, y64 = xh.astype(np.float64), y.cpu().numpy().astype(np.float64)
            out = [None]

            def sk():
                out[0] = trustworthiness(x64, y64, n_neighbors=k)
            ms = host_ms(sk)
            sk_tr = (n, ms)
            r["sklearn"] = {"ms": ms, "value": float(out[0]), "difference": float(val[0] - out[0]), "label": "measured"}
        elif sk_tr:
            r["sklearn"] = {"ms": sk_tr[1] * (n / sk_tr[0]) ** 2,
                            "label": f"extrapolated from n = {sk_tr[0]} by (n / n_run)^2: the n x n float64 matrix and its "
                                     f"argsort ({16 * n * n / 2 ** 30:.0f} GiB) are not formed"}
        res["trustworthiness"][str(n)] = r
        print(json.dumps({f"trustworthiness {n}": r}), flush=True)
        del x, y, idx
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
