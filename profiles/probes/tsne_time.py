"""Exact t-SNE timings (mmgnn.embed.tsne, csrc/tsne.hip) for 128-wide fp32 embeddings already on the device, at
n = 50 (the reference's labs), 1,000 (its patient sample), 4,096 and 16,384 (the n x n buffer's limit).  Synthetic rows:
five L2-normalised clusters, tests/tsne_ref.make_case's recipe; the arithmetic does not depend on their origin.
  (a) the affinities (mmg_tsne_sqdist + mmg_tsne_joint_p) and one iteration (mmg_tsne_step, mean over --iters eager
      iterations without the error), between device events; mmgnn.embed.tsne end to end (max_iter = 1000, PCA init,
      a host clock around work that ends in a device synchronise), with the iterations it ran;
  (b) each kernel alone, from the library's own probe (the kernel's begin / end timestamps); for the gradient kernel the
      bytes of A it reads per iteration (4 n^2) against the 8 TB/s roofline;
  (c) beside those, on the same box and its thread limit: sklearn TSNE(method="exact") and sklearn's default
      barnes_hut (what the reference runs) at n = 1,000 from the same PCA start, max_iter = 1000.
Medians over --reps after --warmup calls.  Reported figures, not thresholds.

  python profiles/probes/tsne_time.py --out profiles/tsne_time.json
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
from mmgnn import embed, ops  # noqa: E402
import tsne_ref as tr  # noqa: E402

HBM_BYTES_PER_S = 8e12


def event_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), ts


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
        for ms, _, _, _, _, flags, sym in ops.probe_read():
            rows.setdefault(f"{sym}#{flags}", []).append(ms)
    ops.probe_arm(0)
    return {k: {"ms": statistics.median(v), "all_ms": v} for k, v in rows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[50, 1000, 4096, 16384])
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sklearn-n", type=int, default=1000, help="0: skip the sklearn runs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "numpy": np.__version__, "hbm_roofline_bytes_per_s": HBM_BYTES_PER_S, "D": a.dim, "sizes": {}}
    for n in a.sizes:
        x = torch.from_numpy(tr.make_case(n, a.dim)).to(dev)
        perp = tr.default_perplexity(n)
        lr = max(n / 12.0 / 4.0, 50.0)
        buf = torch.empty(n, n, device=dev)
        r = {"n": n, "perplexity": perp}

        def affinities():
            ops.tsne_sqdist(x, out=buf)
            ops.tsne_joint_p(buf, perp)
        r["affinities_ms"], r["affinities_all_ms"] = event_ms(affinities, a.reps, a.warmup)
        r["affinity_kernels"] = kernel_times(affinities, 5, a.reps, 1)
        proj = embed.pca(x, 2).projection.double()
        y0 = (proj / proj[:, 0].std(unbiased=False) * 1e-4).contiguous()
        y, u, g = y0.clone(), torch.zeros_like(y0), torch.ones_like(y0)
        stats = torch.empty(3, dtype=torch.float64, device=dev)

        def iterations(want_kl=False):
            y.copy_(y0)
            u.zero_()
            g.fill_(1.0)
            for _ in range(a.iters):
                ops.tsne_step(buf, y, u, g, stats, 12.0, 0.5, lr, 0.01, want_kl, True)
        ms, all_ms = event_ms(iterations, a.reps, a.warmup)
        r["iteration_ms"], r["iteration_all_ms"] = ms / a.iters, [t / a.iters for t in all_ms]
        ms, _ = event_ms(lambda: iterations(True), a.reps, 1)
        r["iteration_with_error_ms"] = ms / a.iters
        kt = kernel_times(lambda: ops.tsne_step(buf, y, u, g, stats, 12.0, 0.5, lr, 0.01, False, True), 3, a.reps, 1)
        r["step_kernels"] = kt
        grad_ms = next(v["ms"] for k, v in kt.items() if "k_tsne_pairs" in k and k.endswith("#1"))
        r["gradient_pass"] = {"ms": grad_ms, "bytes_of_A_read": 4 * n * n,
                              "fraction_of_hbm_roofline": 4 * n * n / (grad_ms * 1e-3) / HBM_BYTES_PER_S,
                              "pairs_per_s": n * (n - 1) / (grad_ms * 1e-3)}
        ts, its = [], []
        for i in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = embed.tsne(x, perplexity=perp)
            torch.cuda.synchronize()
            if i >= a.warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
                its.append(out.n_iter + 1)
        r["end_to_end_ms"], r["end_to_end_all_ms"], r["end_to_end_iterations"] = statistics.median(ts), ts, its
        r["end_to_end_kl"] = out.kl_divergence
        res["sizes"][str(n)] = r
        print(json.dumps({n: r}), flush=True)
        del x, buf, y, u, g, y0, proj
        torch.cuda.empty_cache()
    if a.sklearn_n:
        from sklearn.manifold import TSNE
        n = a.sklearn_n
        x = tr.make_case(n, a.dim)
        y0 = tr.golden_starts(x)[0].astype(np.float32)
        sk = {"n": n, "threads": torch.get_num_threads(), "OMP_NUM_THREADS": os.environ.get("OMP_NUM_THREADS")}
        for method in ("exact", "barnes_hut"):
            t0 = time.perf_counter()
            m = TSNE(method=method, init=y0, perplexity=tr.default_perplexity(n), max_iter=1000).fit(x)
            sk[method] = {"ms": (time.perf_counter() - t0) * 1e3, "n_iter": int(m.n_iter_), "kl": float(m.kl_divergence_)}
        res["sklearn"] = sk
        print(json.dumps({"sklearn": sk}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
