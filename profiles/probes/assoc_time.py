"""Lab-association timings: the x100 eICU-shaped lab matrix (synth.make_graph(100): 183,400 patients x 50 labs, about
two thirds of the cells observed) and a synthetic 183,400 x 512 matrix with about 30 % of the cells observed.
  kernels         k_as_colsum, k_as_colfin, k_as_moments, k_as_sum, k_as_finish one by one (the library's launch probe:
                  HIP events on the kernel itself), medians over --reps probed calls after --warmup
  moments         mmg_assoc_moments as a call (device events around both of its kernels): its fraction of ONE read of X
                  at the 8 TB/s HBM data-sheet rate (4 n L bytes), and of the fp64 matrix-issue bound for the six products
                  over the triangle, 2 * 6 * n * L^2 / 2 flops against FP64_MATRIX_FLOPS, the vendor's published peak
  lab_correlation mmgnn.association.lab_correlation end to end on the device matrix (host clock; includes the one
                  synchronising read of n_inf)
  host            the copy of X to the host + pandas.DataFrame.corr(min_periods=1) on the same box; at 512 labs pandas
                  runs on --pandas-rows rows and the figure is EXTRAPOLATED linearly in the rows (flagged)
  scaling         k_as_moments at 50 labs over 18,340 / 183,400 / 1,834,000 rows (synthetic): whether one block pair
                  with parallelism only over the slabs is bound by latency (time flat in n) or by throughput (linear)

  python profiles/probes/assoc_time.py --out <dir>/assoc_time.json
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
import mmgnn  # noqa: E402,F401
from mmgnn import assoc_ops as ao  # noqa: E402
from mmgnn import association as asc  # noqa: E402
from mmgnn import ops  # noqa: E402
from mmgnn.synth import make_graph  # noqa: E402

HBM_BYTES_PER_S = 8e12
FP64_MATRIX_FLOPS = 78.6e12          # published peak of the MI355X (data sheet), not measured


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


def probed(fn, reps, warmup):
    """-> {kernel: median ms} of the kernels fn launches."""
    for _ in range(warmup):
        fn()
    seen = {}
    for _ in range(reps):
        torch.cuda.synchronize()
        ops.probe_arm(16)
        fn()
        torch.cuda.synchronize()
        for ms, _, _, _, _, _, sym in ops.probe_read():
            seen.setdefault(sym.split("(")[0].strip(), []).append(ms)
        ops.probe_arm(0)
    return {k: statistics.median(v) for k, v in seen.items()}


def measure(X, a, pandas_rows=None):
    n, L = X.shape
    count, mean, _ = ao.assoc_colstats(X)
    rows, slabs = ao.assoc_plan(n, L)
    nb = (L + ao.AS_TILE - 1) // ao.AS_TILE
    r = {"rows": n, "labs": L, "observed_fraction": float(count.sum().item()) / (n * L), "rows_per_slab": rows,
         "slabs": slabs, "block_pairs": nb * (nb + 1) // 2,
         "workspace_bytes": int(ao.load().mmg_assoc_moments_ws_bytes(n, L))}

    def kernels():
        c, m, _ = ao.assoc_colstats(X)
        ao.assoc_finish(ao.assoc_moments(X, m), c, n, 1)

    r["kernels_ms"] = probed(kernels, a.reps, a.warmup)
    ms, allms = event_clock(lambda: ao.assoc_moments(X, mean), a.reps, a.warmup)
    flops = 6 * n * L * L
    r["moments"] = {"ms": ms, "all_ms": allms, "x_bytes": 4 * n * L,
                    "fraction_of_one_hbm_read": 4 * n * L / (ms * 1e-3) / HBM_BYTES_PER_S,
                    "flops_six_products_triangle": flops,
                    "fraction_of_fp64_matrix_bound": flops / (ms * 1e-3) / FP64_MATRIX_FLOPS}
    ms, allms = host_clock(lambda: asc.lab_correlation(X, 1), a.reps, a.warmup)
    r["lab_correlation_end_to_end"] = {"ms": ms, "all_ms": allms}
    copy_ms, _ = host_clock(lambda: X.cpu(), a.host_reps, 1)
    Xh = X.cpu().numpy()
    m = n if pandas_rows is None else min(pandas_rows, n)
    frame = pd.DataFrame(Xh[:m].astype(np.float64))
    ts = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        want = frame.corr(min_periods=1)
        ts.append((time.perf_counter() - t0) * 1e3)
    pms = statistics.median(ts) * (n / m)
    r["host"] = {"copy_ms": copy_ms, "pandas_corr_ms": pms, "pandas_rows": m, "EXTRAPOLATED": m != n,
                 "copy_plus_pandas_ms": copy_ms + pms}
    r["speedup_end_to_end"] = r["host"]["copy_plus_pandas_ms"] / r["lab_correlation_end_to_end"]["ms"]
    if m == n:
        got = asc.lab_correlation(X, 1).r.cpu().numpy()
        w = want.to_numpy()
        assert np.array_equal(np.isnan(got), np.isnan(w))
        r["max_abs_r_difference_from_pandas"] = float(np.nanmax(np.abs(got - w)))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=100)
    ap.add_argument("--wide-labs", type=int, default=512)
    ap.add_argument("--pandas-rows", type=int, default=8000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "numpy": np.__version__, "pandas": pd.__version__, "hbm_bytes_per_s_DATA_SHEET": HBM_BYTES_PER_S,
           "fp64_matrix_flops_per_s_DATA_SHEET_NOT_MEASURED": FP64_MATRIX_FLOPS,
           "host_threads": {"torch": torch.get_num_threads(), "OMP_NUM_THREADS": os.environ.get("OMP_NUM_THREADS")},
           "reps": a.reps, "warmup": a.warmup, "shapes": {}}

    def dump():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    g = make_graph(a.scale, seed=0, device=dev)
    ei = g[asc.LAB_EDGE].edge_index
    P, L = int(g["patient"].num_nodes), int(g["lab"].num_nodes)
    X = asc.lab_matrix(ei[0], ei[1], g[asc.LAB_EDGE].edge_attr.reshape(-1), P, L)
    del g, ei
    res["shapes"][f"x{a.scale}_{P}x{L}"] = measure(X, a)
    print(json.dumps(res["shapes"]), flush=True)
    dump()
    gen = torch.Generator(dev).manual_seed(1)
    W = torch.randn(P, a.wide_labs, device=dev, generator=gen)
    W[torch.rand(P, a.wide_labs, device=dev, generator=gen) >= 0.3] = float("nan")
    res["shapes"][f"synthetic_{P}x{a.wide_labs}"] = measure(W, a, a.pandas_rows)
    print(json.dumps(res["shapes"][f"synthetic_{P}x{a.wide_labs}"]), flush=True)
    dump()
    del W
    scaling = {}
    for n in (P // 10, P, P * 10):
        S = torch.randn(n, L, device=dev, generator=gen)
        S[torch.rand(n, L, device=dev, generator=gen) >= 0.67] = float("nan")
        mean = ao.assoc_colstats(S)[1]
        k = probed(lambda: ao.assoc_moments(S, mean), a.reps, a.warmup)
        rows, slabs = ao.assoc_plan(n, L)
        scaling[str(n)] = {"rows_per_slab": rows, "slabs": slabs, "kernels_ms": k}
        del S
    res["scaling_50_labs"] = scaling
    print(json.dumps(scaling), flush=True)
    dump()


if __name__ == "__main__":
    main()
