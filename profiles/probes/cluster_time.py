"""K-means and silhouette timings (mmgnn.cluster, csrc/cluster.hip) for 128-wide fp32 rows already on the device.
Synthetic rows: 16 Gaussian blobs (unit noise around centres of spread 4), made on the device from a seed.
  (a) kmeans with k = 8 and k = 64 at 1,834 / 183,400 / 1,834,000 rows (the patient counts of the x1, x100 and x1000
      graphs) from a fixed init (k rows of x), tol = 0 and max_iter = --iters, so that every run is the same number of
      iterations unless the labels stop changing: a host clock around the call and a device synchronise -> time per run
      and per iteration (run / n_iter; the run also holds the column statistics, the final assignment and the scores);
      the kernels of ONE assign + update step from the library's probe, each against its bound:
        assignment  fp64 vector issue: n k D fma lane-operations (the subtraction in front of every fma doubles the
                    lane-operations actually issued; the fraction is stated against the fma count, as the plan was);
        sums        HBM: one read of X, n D 4 bytes;
  (b) beside it, on the same box and its thread limit: sklearn KMeans(algorithm="lloyd", n_init=1) from the same init,
      tol and max_iter on the float64 copy of the rows;
  (c) silhouette_score over ALL rows at n = 16,384 and 183,400 (k = 8): wall time, the kernel alone and its fraction of
      the issue bound 2 n^2 D lane-operations (a subtraction and an fma per pair and column); sklearn's
      silhouette_score where its chunked n x n pass is run (--sklearn-sil-max), EXTRAPOLATED by (n / n_run)^2 above.
Peaks: fp64 vector 256 CUs x 4 SIMDs x 16 lane-operations x 2.4 GHz = 3.93e13 per second (profiles/probes/nn_time.py);
HBM 8.0e12 bytes per second (specification; 6.29e12 measured by a float4 copy).
Medians over --reps after --warmup calls.  Reported figures, not thresholds.

  python profiles/probes/cluster_time.py --out profiles/cluster_time.json
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
import mmgnn  # noqa: E402,F401
from mmgnn import cluster, cluster_ops, ops  # noqa: E402

FP64_LANE_OPS_PER_S = 256 * 4 * 16 * 2.4e9
HBM_BYTES_PER_S = 8.0e12
PATIENTS_X1 = 1834


def make_rows(n, D, dev, seed=0, blobs=16):
    g = torch.Generator(device=dev).manual_seed(seed)
    centers = torch.randn(blobs, D, generator=g, device=dev) * 4.0
    which = torch.randint(0, blobs, (n,), generator=g, device=dev)
    return (centers[which] + torch.randn(n, D, generator=g, device=dev)).contiguous()


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


def host_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="+", default=[1, 100, 1000])
    ap.add_argument("--ks", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--sil-sizes", type=int, nargs="+", default=[16384, 100 * PATIENTS_X1])
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sklearn-max", type=int, default=1000 * PATIENTS_X1, help="0: skip the sklearn KMeans runs")
    ap.add_argument("--sklearn-sil-max", type=int, default=16384)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    D = a.dim
    res = {"device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "numpy": np.__version__, "D": D, "fp64_lane_ops_per_s_bound": FP64_LANE_OPS_PER_S,
           "hbm_bytes_per_s_bound": HBM_BYTES_PER_S, "threads": torch.get_num_threads(),
           "OMP_NUM_THREADS": os.environ.get("OMP_NUM_THREADS"), "max_iter": a.iters, "kmeans": {}, "silhouette": {}}
    for scale in a.scales:
        n = scale * PATIENTS_X1
        x = make_rows(n, D, dev)
        x64 = x.cpu().numpy().astype(np.float64) if a.sklearn_max and n <= a.sklearn_max else None
        for k in a.ks:
            pick = np.random.RandomState(1).choice(n, k, replace=False)
            init = x[torch.from_numpy(pick).to(dev)].double().cpu().numpy()
            r = {"n": n, "k": k, "plan_ranges_rows_workgroups": cluster_ops.km_plan(n)}
            out = [None]

            def run():
                out[0] = cluster.kmeans(x, k, init=init, max_iter=a.iters, tol=0.0)
            r["run_ms"], r["all_run_ms"] = wall_ms(run, a.reps, a.warmup)
            r["n_iter"], r["inertia"] = out[0].n_iter, out[0].inertia
            r["ms_per_iteration"] = r["run_ms"] / out[0].n_iter
            cen = torch.from_numpy(init).to(dev)
            labels, min_s = cluster_ops.km_assign(x, cen)
            changed = torch.zeros(1, dtype=torch.int64, device=dev)

            def step():
                cluster_ops.km_assign(x, cen, labels, labels, min_s, changed)
                cluster_ops.km_update(x, labels, min_s, cen, None, None, changed)
            kt = kernel_ms(step, 5, a.reps)
            r["kernels_ms"] = kt
            ka = next(v for s, v in kt.items() if "k_km_assign" in s)
            ks = next(v for s, v in kt.items() if "k_km_sums" in s)
            r["step_kernels_ms"] = sum(kt.values())
            r["assign_kernel"] = {"ms": ka, "fraction_of_fp64_issue_bound": n * k * D / (ka * 1e-3) / FP64_LANE_OPS_PER_S,
                                  "fraction_of_hbm_bound": n * D * 4 / (ka * 1e-3) / HBM_BYTES_PER_S, "label": "measured"}
            r["sums_kernel"] = {"ms": ks, "fraction_of_hbm_bound": n * D * 4 / (ks * 1e-3) / HBM_BYTES_PER_S,
                                "label": "measured"}
            if x64 is not None:
                from sklearn.cluster import KMeans
                km = [None]

                def sk():
                    km[0] = KMeans(k, init=init, n_init=1, algorithm="lloyd", max_iter=a.iters, tol=0.0).fit(x64)
                import warnings
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    ms = host_ms(sk)
                r["sklearn_lloyd"] = {"run_ms": ms, "n_iter": int(km[0].n_iter_), "ms_per_iteration": ms / int(km[0].n_iter_),
                                      "inertia": float(km[0].inertia_),
                                      "labels_equal": bool(np.array_equal(km[0].labels_, out[0].labels.cpu().numpy())),
                                      "label": "measured"}
            res["kmeans"][f"x{scale}_k{k}"] = r
            print(json.dumps({f"kmeans x{scale} k={k}": r}), flush=True)
        del x, x64
        torch.cuda.empty_cache()
    sk_sil = None
    for n in a.sil_sizes:
        x = make_rows(n, D, dev)
        k = 8
        pick = np.random.RandomState(1).choice(n, k, replace=False)
        fit = cluster.kmeans(x, k, init=x[torch.from_numpy(pick).to(dev)].double().cpu().numpy(), max_iter=a.iters)
        r = {"n": n, "k": k, "plan_ranges_items_workgroups": cluster_ops.km_sil_plan(n)}
        val = [None]

        def run():
            val[0] = cluster.silhouette_score(x, fit.labels)
        r["ms"], r["all_ms"] = wall_ms(run, a.reps, a.warmup)
        r["value"] = val[0]
        counts = torch.bincount(fit.labels.long(), minlength=k).to(torch.int32)
        kt = kernel_ms(lambda: cluster_ops.km_silhouette(x, fit.labels, counts), 3, 1)
        r["kernels_ms"] = kt
        kk = next(v for s, v in kt.items() if "k_km_sil" in s and "fin" not in s)
        r["silhouette_kernel"] = {"ms": kk, "fraction_of_fp64_issue_bound": 2.0 * n * n * D / (kk * 1e-3) / FP64_LANE_OPS_PER_S,
                                  "label": "measured"}
        if a.sklearn_sil_max and n <= a.sklearn_sil_max:
            from sklearn.metrics import silhouette_score
            x64, lab = x.cpu().numpy().astype(np.float64), fit.labels.cpu().numpy()
            o = [None]

            def sk():
                o[0] = silhouette_score(x64, lab)
            ms = host_ms(sk)
            sk_sil = (n, ms)
            r["sklearn"] = {"ms": ms, "value": float(o[0]), "difference": float(val[0] - o[0]), "label": "measured"}
        elif sk_sil:
            r["sklearn"] = {"ms": sk_sil[1] * (n / sk_sil[0]) ** 2,
                            "label": f"extrapolated from n = {sk_sil[0]} by (n / n_run)^2"}
        res["silhouette"][str(n)] = r
        print(json.dumps({f"silhouette {n}": r}), flush=True)
        del x
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
