"""Stacked-recalibration timings at the eICU shape (synth.make_graph): the validation pairs are a seeded 15 % of the
has_lab edges, the two predictors synthetic (a flat, per-lab offset "GNN": 0.3 target + offset_lab + noise; the per-lab
mean), already on the device.
  fit             mmg_stack_sums + mmg_stack_solve alone (device events), mmg_stack_sums alone with its fraction of the
                  8 TB/s HBM roofline on its algorithmic bytes ((K + 1) fp32 values and two indices per pair), and
                  mmgnn.stacking.LabStacker.fit end to end (host clock: with the small copies of the table); K = 2, three
                  bins, folds 1 and 5
  predict_matrix  mmg_stack_apply_matrix on the dense [N_P, 50] prediction matrix with a broadcast per-lab feature (device
                  events; 8 algorithmic bytes per cell), beside mmg_cf_apply_matrix on the same matrix in the same run (16)
  model           (--model-steps > 0) a model trained that many steps on the x1 graph: stacking_report's before / after test
                  scores and the bootstrap comparison stacked - raw with its interval
Each fit beside what a user has without the kernels: the copy of the inputs to the host + the numpy path of the module.
Medians over --reps after --warmup calls; host figures over --host-reps.

  python profiles/probes/stack_time.py --scales 100 1000 --out <dir>/stack_time.json
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
from mmgnn import stack_ops as so  # noqa: E402
from mmgnn import stacking as st  # noqa: E402
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


def model_effect(steps, replicates):
    from mmgnn.model import build_model
    from mmgnn.train import EdgeMasker
    dev = torch.device("cuda:0")
    g = make_graph(1, seed=0).to(dev)
    cfg = {"model": {"architecture": "RGCN", "hidden_dim": 64, "num_layers": 2, "dropout": 0.0,
                     "use_batch_norm": True, "activation": "relu"}}
    torch.manual_seed(0)
    model = build_model(cfg, (g.node_types, g.edge_types), None).to(dev)
    model._init_embeddings(g)
    masker = EdgeMasker(g)
    pi, li, y = cf._split_pairs(g, masker, "train")
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    model.train()
    for _ in range(steps):
        opt.zero_grad()
        (model.predict_lab_values(g, pi, li).reshape(-1) - y).abs().mean().backward()
        opt.step()
    obj, table, scores, comparison = st.stacking_report(model, g, masker, replicates=replicates)
    top = scores.iloc[0]
    cmp_ = comparison[comparison.scope == "overall"]
    return {"train_steps": steps, "test_pairs": int(top["n"]), "replicates": replicates,
            "levels": table.level.value_counts().to_dict(),
            "mae_raw": float(top["mae_raw"]), "mae_stacked": float(top["mae_stacked"]),
            "rmse_raw": float(top["rmse_raw"]), "rmse_stacked": float(top["rmse_stacked"]),
            "stacked_minus_raw": {r["metric"]: {"estimate": r["estimate"], "lower": r["lower"], "upper": r["upper"],
                                                "p_below_zero": r["p_below_zero"]} for _, r in cmp_.iterrows()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--matrix-scales", type=int, nargs="+", default=[100])
    ap.add_argument("--folds", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--model-steps", type=int, default=0)
    ap.add_argument("--replicates", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    edges = [float(e) for e in st.DEFAULT_BINS]
    res = {"device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "numpy": np.__version__, "hbm_roofline_bytes_per_s": HBM_BYTES_PER_S, "features": 2, "ridge": 1e-3,
           "min_count": 30, "bins": [str(e) for e in edges], "scales": {}}

    def dump():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    if a.model_steps > 0:
        res["model"] = model_effect(a.model_steps, a.replicates)
        print(json.dumps({"model": res["model"]}), flush=True)
        dump()
    for s in a.scales:
        g = make_graph(s, seed=0, device=dev)
        ei = g[LAB_EDGE].edge_index
        t_all = g[LAB_EDGE].edge_attr.reshape(-1)
        L, P, E = int(g["lab"].num_nodes), int(g["patient"].num_nodes), int(t_all.numel())
        gen = torch.Generator(dev).manual_seed(1)
        idx = torch.randperm(E, device=dev, generator=gen)[:int(0.15 * E)].sort().values
        offset = 0.3 * torch.randn(L, device=dev, generator=gen)
        deg = build_plan(g, dev).lab_deg
        pi, li, t = ei[0][idx].contiguous(), ei[1][idx].contiguous(), t_all[idx].contiguous()
        n = int(t.numel())
        f1 = (0.3 * t + offset[li] + 0.2 * torch.randn(n, device=dev, generator=gen)).contiguous()
        lab_mean = torch.zeros(L, device=dev).index_add_(0, li, t) / torch.bincount(li, minlength=L).clamp(min=1)
        f2 = lab_mean[li].contiguous()
        del idx
        r = {"pairs": n, "patients": P, "labs": L, "cells": L * (len(edges) - 1), "index_bytes": 8, "folds": {}}
        copy_ms, _ = host_clock(lambda: [x.cpu() for x in (f1, f2, t, pi, li)], a.host_reps, 1)
        hf1, hf2, ht, hpi, hli = (x.cpu().numpy() for x in (f1, f2, t, pi, li))
        hdeg = deg.cpu().numpy()
        alg = n * (3 * 4 + 2 * 8)
        for J in a.folds:
            q = {}
            ms, allms = event_clock(lambda: so.stack_sums([f1, f2], t, pi, li, L, deg, edges, J, 0), a.reps, a.warmup)
            q["sums_kernels"] = {"ms": ms, "all_ms": allms, "algorithmic_bytes": alg,
                                 "roofline_fraction": alg / (ms * 1e-3) / HBM_BYTES_PER_S}

            def fit_kernels():
                sums, _ = so.stack_sums([f1, f2], t, pi, li, L, deg, edges, J, 0)
                so.stack_solve(sums, L, len(edges) - 1, 2, 1e-3, 30)

            ms, allms = event_clock(fit_kernels, a.reps, a.warmup)
            q["fit_kernels"] = {"ms": ms, "all_ms": allms}
            e2e, e2e_all = host_clock(lambda: st.LabStacker(folds=J).fit([f1, f2], t, li, pi, deg, n_labs=L), a.reps, a.warmup)
            q["fit_end_to_end_ms"], q["fit_end_to_end_all_ms"] = e2e, e2e_all
            obj = st.LabStacker(folds=J).fit([f1, f2], t, li, pi, deg, n_labs=L)
            ts = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter()
                host = st.LabStacker(folds=J).fit([hf1, hf2], ht, hli, hpi, hdeg, n_labs=L)
                ts.append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(host.coef, obj.coef, equal_nan=True) and np.array_equal(host.level, obj.level)
            q["fit_host"] = {"copy_ms": copy_ms, "numpy_ms": statistics.median(ts),
                             "copy_plus_numpy_ms": copy_ms + statistics.median(ts)}
            q["fit_speedup_end_to_end"] = q["fit_host"]["copy_plus_numpy_ms"] / e2e
            q["levels"] = {st.LEVELS[k]: int((obj.level[-1] == k).sum()) for k in range(4)}
            y = obj.predict([f1, f2], li, pi)
            q["mse_raw"], q["mse_stacked"] = float(((t - f1) ** 2).mean()), float(((t - y) ** 2).mean())
            r["folds"][str(J)] = q
            del host
        if s in a.matrix_scales:
            gen2 = torch.Generator(dev).manual_seed(2)
            m = torch.randn(P, L, device=dev, generator=gen2)
            coef = obj._on(dev)[0]
            out = torch.empty_like(m)
            cells = P * L
            ms, allms = event_clock(lambda: so.stack_apply_matrix([m, lab_mean], None, deg, edges, coef, out=out), a.reps,
                                    a.warmup)
            r["predict_matrix"] = {"rows": P, "ms": ms, "all_ms": allms, "algorithmic_bytes": 8 * cells,
                                   "roofline_fraction": 8 * cells / (ms * 1e-3) / HBM_BYTES_PER_S}
            table = torch.zeros(3, L * (len(edges) - 1), device=dev)
            outs = tuple(torch.empty_like(m) for _ in range(3))
            ms, allms = event_clock(lambda: co.cf_apply_matrix(m, None, deg, edges, table, False, out=outs), a.reps, a.warmup)
            r["cf_apply_matrix"] = {"ms": ms, "all_ms": allms, "algorithmic_bytes": 16 * cells,
                                    "roofline_fraction": 16 * cells / (ms * 1e-3) / HBM_BYTES_PER_S}
            hw = obj.predict_matrix([m.cpu().numpy(), lab_mean.cpu().numpy()])
            assert np.array_equal(out.cpu().numpy(), hw, equal_nan=True)
            del m, out, outs, hw
        res["scales"][str(s)] = r
        print(json.dumps({s: r}), flush=True)
        dump()
        del g, ei, t_all, pi, li, t, f1, f2, deg, hf1, hf2, ht, hpi, hli
        torch.cuda.empty_cache()
    dump()


if __name__ == "__main__":
    main()
