"""Embedding-map timings at the eICU patient counts (1,834 x scale rows) for 128- and 256-wide fp32 embeddings already on
the device (synthetic: a planted spectrum plus an offset, tests/embed_ref.make_case's recipe drawn on the device; the
arithmetic does not depend on their origin):
  (a) mmgnn.embed.pca end to end (Gram, the copy of the D x D matrix, numpy.linalg.eigh on the host, projection) and
      with the density grid on top -- host clock around work that ends in a device synchronise;
  (b) each kernel alone, from the library's own probe (the kernel's begin / end timestamps): column sums, mean, Gram
      slabs, Gram sum, projection, grid.  For the Gram kernel its fraction of two bounds:
        fp64 issue: the MFMA flops it ISSUES (2 * 256 * 4 per v_mfma_f64_16x16x4_f64, every 16 x 16 tile on or above
                    the diagonal, rows padded to the chunk) against FP64_MATRIX_FLOPS, the vendor's published peak for
                    the part -- a figure taken from the data sheet, not measured here;
        bytes:      4 n D (one read of X; the block pairs re-read it through the cache) against 8 TB/s;
  (c) what a user has without the kernels: copy X to the host + float64 numpy (centre, X.T @ X, eigh, project).  Above
      --host-max-rows rows the host arithmetic runs on the first rows only and the figure is EXTRAPOLATED linearly in the
      row count (marked in the JSON); the copy is always timed in full.
Medians over --reps after --warmup calls.

  python profiles/probes/embed_time.py --scales 1 100 1000 --out <dir>/embed_time.json
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
from mmgnn import embed, ops  # noqa: E402

HBM_BYTES_PER_S = 8e12
FP64_MATRIX_FLOPS = 78.6e12          # published peak of the MI355X (data sheet), not measured
PATIENTS_X1 = 1834


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


def make_rows(n, D, dev, seed=0):
    gen = torch.Generator(dev).manual_seed(seed)
    sv = torch.tensor([8.0, 4.0, 2.0, 1.0], device=dev)
    z = torch.randn(n, 4, device=dev, generator=gen) * sv
    v = torch.linalg.qr(torch.randn(D, 4, device=dev, generator=gen))[0]
    return (z @ v.T + 0.05 * torch.randn(n, D, device=dev, generator=gen) + 3.0).contiguous()


def kernel_times(fn, n_launches, reps, warmup):
    """-> {kernel symbol: median ms} from the library's probe (each launch carries its own event pair)."""
    for _ in range(warmup):
        fn()
    rows = {}
    for _ in range(reps):
        torch.cuda.synchronize()
        ops.probe_arm(n_launches)
        fn()
        torch.cuda.synchronize()
        for ms, _, _, _, _, _, sym in ops.probe_read():
            rows.setdefault(sym, []).append(ms)
    ops.probe_arm(0)
    return {k: {"ms": statistics.median(v), "all_ms": v} for k, v in rows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="+", default=[1, 100, 1000])
    ap.add_argument("--dims", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--host-max-rows", type=int, default=400_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "numpy": np.__version__, "hbm_roofline_bytes_per_s": HBM_BYTES_PER_S,
           "fp64_matrix_flops_per_s_DATA_SHEET_NOT_MEASURED": FP64_MATRIX_FLOPS, "scales": {}}
    for s in a.scales:
        n = PATIENTS_X1 * s
        res["scales"][str(s)] = {}
        for D in a.dims:
            x = make_rows(n, D, dev)
            deg = torch.randint(0, 60, (n,), device=dev, dtype=torch.int32)
            r = {"rows": n, "D": D}
            r["pca_end_to_end_ms"], r["pca_end_to_end_all_ms"] = host_clock(lambda: embed.pca(x, 2), a.reps, a.warmup)
            pr = embed.pca(x, 2)
            r["pca_plus_grid_end_to_end_ms"], _ = host_clock(
                lambda: embed.density_grid(embed.pca(x, 2).projection, deg, 128), a.reps, a.warmup)
            mean_d, gram_d = ops.centered_gram(x)
            comps_d = torch.from_numpy(pr.components).to(dev)
            lo, hi = pr.projection.min(dim=0).values.double().cpu().numpy(), pr.projection.max(dim=0).values.double().cpu().numpy()
            ex = torch.from_numpy(np.linspace(lo[0], hi[0], 129)).to(dev)
            ey = torch.from_numpy(np.linspace(lo[1], hi[1], 129)).to(dev)

            def kernels():
                ops.centered_gram(x)
                ops.project_rows(x, mean_d, comps_d)
                ops.grid2d(pr.projection, ex, ey, deg)
            kt = kernel_times(kernels, 6, a.reps, a.warmup)
            r["kernels"] = kt
            gram_ms = next(v["ms"] for k, v in kt.items() if "k_pca_gram" in k and "sum" not in k)
            tiles = (D // 16) * (D // 16 + 1) // 2 if D % 16 == 0 else None
            rows_issued = -(-n // 32) * 32
            issued = 2.0 * 256 * rows_issued * tiles
            r["gram"] = {"ms": gram_ms, "mfma_flops_issued": issued, "useful_flops": float(n) * D * (D + 1),
                         "fraction_of_fp64_issue_bound": issued / (gram_ms * 1e-3) / FP64_MATRIX_FLOPS,
                         "algorithmic_bytes": 4 * n * D,
                         "fraction_of_byte_bound": 4 * n * D / (gram_ms * 1e-3) / HBM_BYTES_PER_S}

            copy_ms, copy_all = host_clock(lambda: x.cpu(), a.host_reps, 1)
            hx = x.cpu().numpy()
            m = min(n, a.host_max_rows)
            sub = hx[:m]

            def host_pca():
                x64 = sub.astype(np.float64)
                xc = x64 - x64.mean(axis=0)
                lam, vec = np.linalg.eigh(xc.T @ xc)
                return xc @ vec[:, ::-1][:, :2]
            ts = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter()
                host_pca()
                ts.append((time.perf_counter() - t0) * 1e3)
            host_ms = statistics.median(ts) * (n / m)
            r["host"] = {"copy_ms": copy_ms, "copy_all_ms": copy_all, "numpy_ms": host_ms, "numpy_rows_timed": m,
                         "numpy_EXTRAPOLATED": m < n, "copy_plus_numpy_ms": copy_ms + host_ms,
                         "threads": torch.get_num_threads()}
            r["speedup_end_to_end"] = (copy_ms + host_ms) / r["pca_end_to_end_ms"]
            res["scales"][str(s)][str(D)] = r
            print(json.dumps({s: {D: r}}), flush=True)
            del x, hx, sub, pr, deg
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
