"""Bootstrap timings at the eICU shape (synth.make_graph): the test pairs are a seeded 15 % of the has_lab edges, the
predictions synthetic (target * slope_lab + offset_lab + noise: the arithmetic does not depend on their origin), the
baseline the per-lab mean, everything already on the device.
  bootstrap_metrics   mmgnn.bootstrap.bootstrap_metrics end to end (host clock around a device synchronise): the per-lab
                      winsorisation, mmg_boot_sums / _metrics / _summary over the labs, the frames; without and with a
                      baseline
  kernels             the three calls alone between device events, on the lab segments, F = 7 and F = 10.  mmg_boot_sums
                      is held against the fp64 FMA issue bound: kept pairs x (replicates + 1) x (F - 2) fused
                      multiply-adds at FP64_VECTOR_FLOPS / 2 per second
  host                the float64 restatement of the same module (numpy, this machine's CPUs, torch and numpy threads as
                      the environment sets them) on --host-replicates replicates; scaled to the full count and marked
                      EXTRAPOLATED when that is fewer
Medians over --reps after --warmup calls.

  python profiles/probes/boot_time.py --scales 100 1000 --out <dir>/boot_time.json
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
from mmgnn import boot_ops as bo  # noqa: E402
from mmgnn import bootstrap as bt  # noqa: E402
from mmgnn.synth import make_graph  # noqa: E402
from mmgnn.train import LAB_EDGE  # noqa: E402

FP64_VECTOR_FLOPS = 78.6e12          # MI355X data sheet: peak FP64 vector, 2 FLOP per fused multiply-add


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
    ap.add_argument("--replicates", type=int, default=1000)
    ap.add_argument("--host-replicates", type=int, nargs="+", default=[64, 8], help="one per scale")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B = a.replicates
    res = {"device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "numpy": np.__version__, "replicates": B, "confidence": 0.95, "cluster": "patient",
           "fp64_vector_flops": FP64_VECTOR_FLOPS, "chunk": bo.BOOT_CHUNK, "replicates_per_workgroup": bo.BOOT_RB,
           "host_threads": {"torch": torch.get_num_threads(), "OMP_NUM_THREADS": os.environ.get("OMP_NUM_THREADS")},
           "scales": {}}
    for s, host_b in zip(a.scales, a.host_replicates):
        g = make_graph(s, seed=0, device=dev)
        ei = g[LAB_EDGE].edge_index
        t_all = g[LAB_EDGE].edge_attr.reshape(-1)
        L, P, E = int(g["lab"].num_nodes), int(g["patient"].num_nodes), int(t_all.numel())
        gen = torch.Generator(dev).manual_seed(1)
        idx = torch.randperm(E, device=dev, generator=gen)[:int(0.15 * E)].sort().values
        slope = 0.7 + 0.6 * torch.rand(L, device=dev, generator=gen)
        offset = 0.3 * torch.randn(L, device=dev, generator=gen)
        pi, li, t = ei[0][idx].contiguous(), ei[1][idx].contiguous(), t_all[idx].float().contiguous()
        p = (t * slope[li] + offset[li] + 0.2 * torch.randn(t.numel(), device=dev, generator=gen)).contiguous()
        cnt = torch.bincount(li, minlength=L).double()
        base = (torch.zeros(L, dtype=torch.float64, device=dev).index_add_(0, li, t.double()) / cnt.clamp(min=1)).float()[li]
        base = base.contiguous()
        n = int(t.numel())
        r = {"pairs": n, "patients": P, "labs": L, "index_bytes": 8}

        for name, bl in (("bootstrap_metrics", None), ("bootstrap_metrics_with_baseline", base)):
            ms, allms = host_clock(lambda: bt.bootstrap_metrics(p, t, pi, li, g, replicates=B, baseline=bl), a.reps, a.warmup)
            r[name] = {"ms": ms, "all_ms": allms}
        out = bt.bootstrap_metrics(p, t, pi, li, g, replicates=B, baseline=base)
        r["overall"] = json.loads(out.overall.to_json(orient="records"))
        r["comparison_overall"] = json.loads(out.comparison[out.comparison["scope"] == "overall"].to_json(orient="records"))

        for F, bl in ((bo.BOOT_FIELDS, None), (bo.BOOT_FIELDS_B, base)):
            k = {}
            sums, dropped = bo.boot_sums(p, t, pi, li, P, L, B, 0, bl)
            ms, allms = event_clock(lambda: bo.boot_sums(p, t, pi, li, P, L, B, 0, bl, out=(sums, dropped)), a.reps, a.warmup)
            fma = n * (B + 1) * (F - 2)
            bound_ms = fma / (FP64_VECTOR_FLOPS / 2) * 1e3
            k["sums"] = {"ms": ms, "all_ms": allms, "weighted_updates": n * (B + 1), "fp64_fma": fma,
                         "fp64_fma_bound_ms": bound_ms, "fraction_of_bound": bound_ms / ms,
                         "workspace_bytes": int(bo.load().mmg_boot_sums_ws_bytes(n, L, B, 1 if bl is not None else 0))}
            metrics = bo.boot_metrics(sums)
            ms, allms = event_clock(lambda: bo.boot_metrics(sums, out=metrics), a.reps, a.warmup)
            k["metrics"] = {"ms": ms, "all_ms": allms}
            summary = bo.boot_summary(metrics, 0.95)
            ms, allms = event_clock(lambda: bo.boot_summary(metrics, 0.95, out=summary), a.reps, a.warmup)
            k["summary"] = {"ms": ms, "all_ms": allms}
            r[f"kernels_F{F}"] = k
            del sums, metrics, summary

        # the host path of the same module on the same pairs, fewer replicates
        hp, ht, hpi, hli, hb = (x.cpu().numpy() for x in (p, t, pi, li, base))
        t0 = time.perf_counter()
        hs, _ = bt.host_sums(hp, ht, hpi, hli, P, L, host_b, 0)
        hm = bt.host_metrics(hs)
        bt.host_summary(hm, 0.95)
        sec = time.perf_counter() - t0
        dsums = bo.boot_sums(p, t, pi, li, P, L, host_b, 0)[0].cpu().numpy()
        assert np.array_equal(dsums[..., 0], hs[..., 0]) and np.allclose(dsums, hs, rtol=1e-12, atol=0)
        r["host"] = {"replicates_timed": host_b, "seconds": sec,
                     "seconds_at_full_replicates": sec * (B + 1) / (host_b + 1),
                     "EXTRAPOLATED": host_b < B, "sums_bitwise_equal_to_device": bool(np.array_equal(dsums, hs))}
        res["scales"][str(s)] = r
        print(json.dumps({s: r}), flush=True)
        del g, ei, t_all, p, t, pi, li, base
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
