"""Measurement-propensity timings at the eICU shape (synth.make_graph), kind="codes" with 128 features, everything
already on the device.
  fit        LabPropensity(C=1, max_iter=25, tol=1e-8).fit end to end (host clock around a device synchronise): column
             statistics, counts, the one read, max_iter + 1 rounds of link, moments, solve, update, the read-back
  kernels    mmg_prop_moments and mmg_prop_link alone between device events, every lab of the first batch live; the
             moments' useful flops are the cells a <= b of the (D + 2)-wide table, a multiply and an add per row
  sklearn    LogisticRegression(solver="newton-cholesky", tol=1e-8) lab by lab on this machine's CPUs (OMP_NUM_THREADS as
             set), every lab that is not degenerate; the largest coefficient difference to the fit
Medians over 5 fits at x1 and 3 above, after one warm-up fit.

  python profiles/prop_time.py --scales 1 100 --out profiles/prop_time.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import mmgnn  # noqa: E402,F401
from mmgnn import missingness as ms  # noqa: E402
from mmgnn import prop_ops as po  # noqa: E402
from mmgnn.association import lab_matrix  # noqa: E402
from mmgnn.synth import make_graph  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scales", type=int, nargs="+", default=[1, 100])
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "prop_time.json"))
args = ap.parse_args()

DEV = torch.device("cuda:0")
out = {"device": torch.cuda.get_device_name(0), "threads": int(os.environ.get("OMP_NUM_THREADS", "0")), "cases": []}


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return ts


for scale in args.scales:
    t0 = time.perf_counter()
    g = make_graph(scale, seed=0, device=DEV) if scale > 1 else make_graph(scale, seed=0).to(DEV)
    F, names = ms.measurement_features(g, "codes", 128)
    ei = g["patient", "has_lab", "lab"].edge_index
    P, L = int(g["patient"].num_nodes), int(g["lab"].num_nodes)
    X = lab_matrix(ei[0], ei[1], torch.ones(ei.shape[1], dtype=torch.float32, device=DEV), P, L)
    Y = po.prop_indicator(X)
    torch.cuda.synchronize()
    D = int(F.shape[1])
    case = {"scale": scale, "n": P, "L": L, "D": D, "setup_s": round(time.perf_counter() - t0, 2),
            "plan": po.prop_plan(P, D), "batch": po.prop_batch(P, D)}
    print(case, flush=True)
    fit = None

    def run():
        global fit
        fit = ms.LabPropensity(C=1.0, max_iter=25, tol=1e-8).fit(F, Y)

    run()                                                    # warm-up: workspaces, the LDS attribute
    ts = timed(run, 3 if scale > 1 else 5)
    case["fit_ms"] = [round(t, 2) for t in ts]
    case["fit_ms_median"] = round(statistics.median(ts), 2)
    case["n_iter_max"] = int(fit.n_iter_.max())
    case["n_iter"] = [int(v) for v in fit.n_iter_]
    case["converged"] = int(fit.converged_.sum())
    case["degenerate"] = int(fit.degenerate_.sum())
    print("fit", case["fit_ms"], "n_iter max", case["n_iter_max"], flush=True)
    # moments alone, every lab live, at the start point
    count = po.prop_count(Y).cpu().numpy()
    trial, state, _ = ms.start_point(count, P, D)
    df = ms._DeviceFit(F, torch.from_numpy(fit._st["mean"]).to(DEV), Y, trial, state, 1.0, 1e-8 * P, 25)
    j0, nb = df.batches[0]
    sr, lossp, H, gg, delta, dec = df.views(nb)
    po.prop_link(df.X, df.mean, df.Y, j0, nb, df.beta, None, sr, lossp)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(12)]
    po.prop_moments(df.X, df.mean, sr, L, j0, nb, None, H, gg)
    for i in range(0, 12, 2):
        ev[i].record()
        po.prop_moments(df.X, df.mean, sr, L, j0, nb, None, H, gg)
        ev[i + 1].record()
    torch.cuda.synchronize()
    mm = [ev[i].elapsed_time(ev[i + 1]) for i in range(0, 12, 2)]
    T = D + 2
    flops = 2.0 * P * (T * (T + 1) / 2) * nb                 # the cells a <= b, a multiply and an add each
    case["moments_ms"] = [round(t, 3) for t in mm]
    case["moments_ms_median"] = round(statistics.median(mm), 3)
    case["moments_labs"] = nb
    case["moments_useful_tflops"] = round(flops / (statistics.median(mm) * 1e-3) / 1e12, 3)
    lk = []
    for i in range(0, 12, 2):
        ev[i].record()
        po.prop_link(df.X, df.mean, df.Y, j0, nb, df.beta, None, sr, lossp)
        ev[i + 1].record()
    torch.cuda.synchronize()
    case["link_ms_median"] = round(statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(0, 12, 2)), 3)
    print("moments", case["moments_ms"], case["moments_useful_tflops"], "link", case["link_ms_median"], flush=True)
    # sklearn on this box
    from sklearn.linear_model import LogisticRegression
    Fh, Yh = F.cpu().numpy().astype(np.float64), Y.cpu().numpy()
    labs = [j for j in range(L) if 0 < Yh[:, j].sum() < P]
    t = time.perf_counter()
    worst = 0.0
    for j in labs:
        sk = LogisticRegression(C=1.0, solver="newton-cholesky", tol=1e-8, max_iter=100).fit(Fh, Yh[:, j])
        worst = max(worst, float(np.abs(sk.coef_[0] - fit.coef_[j]).max()))
    case["sklearn_newton_cholesky_s"] = round(time.perf_counter() - t, 3)
    case["sklearn_labs"] = len(labs)
    case["sklearn_max_coef_difference"] = worst
    print("sklearn", case["sklearn_newton_cholesky_s"], len(labs), worst, flush=True)
    out["cases"].append(case)
    json.dump(out, open(args.out, "w"), indent=1)
    # the weighted error sums over every has_lab pair, the propensities of the fit
    prob = fit.predict_proba(F)
    pred = torch.randn(ei.shape[1], device=DEV)
    target = torch.randn(ei.shape[1], device=DEV)
    pi, li = ei[0].contiguous(), ei[1].contiguous()
    ms.ipw_metrics(pred, target, pi, li, prob)
    ts = timed(lambda: ms.ipw_metrics(pred, target, pi, li, prob), 5)
    case["pairs"] = int(ei.shape[1])
    case["ipw_metrics_ms_median"] = round(statistics.median(ts), 3)
    cov = torch.from_numpy(fit.coverage_).to(DEV)
    for i in range(0, 12, 2):
        ev[i].record()
        po.prop_pair_sums(pred, target, pi, li, prob, cov, 0.02, True)
        ev[i + 1].record()
    torch.cuda.synchronize()
    case["pair_sums_ms_median"] = round(statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(0, 12, 2)), 3)
    print("ipw", case["ipw_metrics_ms_median"], case["pair_sums_ms_median"], flush=True)
    json.dump(out, open(args.out, "w"), indent=1)
    del g, F, X, Y, fit, df
    torch.cuda.empty_cache()
