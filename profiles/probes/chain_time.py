"""Chained-equations imputation timings: the x1 and x100 eICU-shaped lab matrices (synth.make_graph: 1,834 and 183,400
patients x 50 labs, about two thirds of the train cells observed) and a synthetic 183,400 x 128 matrix with about 30 % of
the cells observed.
  kernels   k_ch_moments, k_ch_sum, k_ch_solve, k_ch_apply, k_ch_maxfin one by one over ONE round (the library's launch
            probe: HIP events on the kernel itself), medians over the round's steps; k_ch_moments against the fp64
            matrix-issue bound (2 n_j L^2 / 2 flops over the triangle against FP64_MATRIX_FLOPS, the vendor's published
            peak) and against one read of W at the 8 TB/s HBM data-sheet rate (8 n L bytes); k_ch_apply against one read
            of the rows it rewrites
  fit       ChainedLabImputer(max_iter=--rounds, tol=0).fit_matrix end to end (host clock; one read at the end)
  round     one round eager (device events) against one replay of the same round captured into a hipGraph
  sklearn   IterativeImputer(Ridge(1.0), skip_complete=False) on the same box and host threads: all rounds at x1; ONE round
            elsewhere, on --sklearn-rows rows at 128 labs, EXTRAPOLATED linearly in rounds and rows (flagged)
  accuracy  the test-split MAE of chained_equations beside per_lab_mean and nearest_neighbor on the x1 graph

  python profiles/probes/chain_time.py --out <dir>/chain_time.json
"""
import argparse
import json
import os
import platform
import statistics
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import mmgnn  # noqa: E402,F401
from mmgnn import assoc_ops  # noqa: E402
from mmgnn import association as asc  # noqa: E402
from mmgnn import chain_ops as co  # noqa: E402
from mmgnn import chained as ch  # noqa: E402
from mmgnn import evaluate as ev  # noqa: E402
from mmgnn import ops  # noqa: E402
from mmgnn.synth import make_graph  # noqa: E402
from mmgnn.train import EdgeMasker  # noqa: E402

HBM_BYTES_PER_S = 8e12
FP64_MATRIX_FLOPS = 78.6e12          # published peak of the MI355X (data sheet), not measured


def new_chain(X, rounds=1):
    count, center, _ = assoc_ops.assoc_colstats(X)
    n, L = X.shape
    order = ch.visit_order(count.cpu().numpy(), n)
    return ch._DeviceChain(X, count, center, order, 1.0, np.full(L, -np.inf), np.full(L, np.inf), rounds), count


def measure(X, a, sklearn_rows=None, sklearn_all_rounds=False):
    n, L = (int(v) for v in X.shape)
    rows, slabs = co.chain_plan(n, L)
    nb = (L + co.CH_TILE - 1) // co.CH_TILE
    chain, count = new_chain(X)
    r = {"rows": n, "labs": L, "observed_fraction": float(count.sum().item()) / (n * L), "rows_per_slab": rows,
         "slabs": slabs, "block_pairs": nb * (nb + 1) // 2,
         "workspace_bytes": int(co.load().mmg_chain_moments_ws_bytes(n, L)), "steps_per_round": len(chain.order)}
    chain.round(0)                                            # warm-up
    torch.cuda.synchronize()
    ops.probe_arm(8 * L + 16)
    chain.round(0)
    torch.cuda.synchronize()
    seen = {}
    for ms, _, _, _, _, _, sym in ops.probe_read():
        seen.setdefault(sym.split("(")[0].strip(), []).append(ms)
    ops.probe_arm(0)
    r["kernels_ms_median_of_a_round"] = {k: statistics.median(v) for k, v in seen.items()}
    r["kernels_ms_sum_of_a_round"] = {k: sum(v) for k, v in seen.items()}
    nj = float(count.double().mean().item())
    mom = r["kernels_ms_median_of_a_round"].get("k_ch_moments")
    if mom:
        flops = nj * L * L
        r["k_ch_moments"] = {"flops_triangle_mean_step": flops, "fraction_of_fp64_matrix_bound": flops / (mom * 1e-3) / FP64_MATRIX_FLOPS,
                             "w_bytes": 8 * n * L, "fraction_of_one_hbm_read_of_W": 8 * n * L / (mom * 1e-3) / HBM_BYTES_PER_S}
    app = r["kernels_ms_median_of_a_round"].get("k_ch_apply")
    if app:
        b = 8 * (n - nj) * L
        r["k_ch_apply"] = {"bytes_rows_rewritten_mean_step": b, "fraction_of_hbm_rate": b / (app * 1e-3) / HBM_BYTES_PER_S}
    # one round: eager against a captured replay
    ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        chain.round(0)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    r["round_eager"] = {"ms": statistics.median(ts), "all_ms": ts}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        chain.round(0)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain.round(0)
    ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    r["round_graph_replay"] = {"ms": statistics.median(ts), "all_ms": ts}
    del graph, chain
    ts = []
    for _ in range(a.fit_reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        imp = ch.ChainedLabImputer(max_iter=a.rounds, tol=0).fit_matrix(X)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    r["fit_end_to_end"] = {"rounds": a.rounds, "ms": statistics.median(ts[1:]), "all_ms_first_is_warmup": ts}
    # sklearn on the host
    from sklearn.experimental import enable_iterative_imputer  # noqa: F401
    from sklearn.impute import IterativeImputer
    from sklearn.linear_model import Ridge
    t0 = time.perf_counter()
    Xh = X.cpu().numpy()
    copy_ms = (time.perf_counter() - t0) * 1e3
    m = n if sklearn_rows is None else min(sklearn_rows, n)
    sk_rounds = a.rounds if sklearn_all_rounds else 1
    sk = IterativeImputer(Ridge(alpha=1.0), max_iter=sk_rounds, tol=0, skip_complete=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t0 = time.perf_counter()
        S = sk.fit_transform(Xh[:m].astype(np.float64))
        sk_ms = (time.perf_counter() - t0) * 1e3
    full = sk_ms * (a.rounds / sk_rounds) * (n / m)
    r["host"] = {"copy_ms": copy_ms, "sklearn_measured_ms": sk_ms, "sklearn_rounds": sk_rounds, "sklearn_rows": m,
                 "sklearn_ms_for_the_fit": full, "EXTRAPOLATED": sk_rounds != a.rounds or m != n}
    r["speedup_end_to_end"] = (copy_ms + full) / r["fit_end_to_end"]["ms"]
    if m == n and sk_rounds == a.rounds and S.shape == (n, L):
        r["max_abs_difference_from_sklearn"] = float(np.abs(imp.imputed64_.cpu().numpy() - S).max())
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wide-labs", type=int, default=128)
    ap.add_argument("--sklearn-rows", type=int, default=20000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fit-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "numpy": np.__version__, "hbm_bytes_per_s_DATA_SHEET": HBM_BYTES_PER_S,
           "fp64_matrix_flops_per_s_DATA_SHEET_NOT_MEASURED": FP64_MATRIX_FLOPS,
           "host_threads": {"torch": torch.get_num_threads(), "OMP_NUM_THREADS": os.environ.get("OMP_NUM_THREADS")},
           "reps": a.reps, "rounds": a.rounds, "shapes": {}}

    def dump():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    P = 0
    for scale in (1, 100):
        g = make_graph(scale, seed=0, device=dev)
        masker = EdgeMasker(g)
        tr_ei, tr_v, _, _ = masker.get_masked_data("train", want_mask=False)
        P, L = int(g["patient"].num_nodes), int(g["lab"].num_nodes)
        X = asc.lab_matrix(tr_ei[0].to(dev), tr_ei[1].to(dev), tr_v.to(dev).reshape(-1), P, L)
        key = f"x{scale}_{P}x{L}_train_edges"
        res["shapes"][key] = measure(X, a, sklearn_all_rounds=scale == 1)
        print(json.dumps({key: res["shapes"][key]}), flush=True)
        if scale == 1:
            te_ei, te_v, _, _ = masker.get_masked_data("test", want_mask=False)
            tv, ti = tr_v.cpu().numpy().reshape(-1), tr_ei.cpu().numpy()
            acc = ev.evaluate_baselines((tv, ti[1]), (te_v.cpu().numpy().reshape(-1), te_ei.cpu().numpy()[1], None))
            acc.update(ev.evaluate_nearest_neighbor_baseline(g, masker, "test"))
            acc.update(ev.evaluate_chained_baseline(g, masker, "test"))
            res["accuracy_x1_test_split_NOT_ASSERTED"] = {k: v["mae"] for k, v in acc.items()}
            print(json.dumps(res["accuracy_x1_test_split_NOT_ASSERTED"]), flush=True)
        dump()
        del g, masker, X
    gen = torch.Generator(dev).manual_seed(1)
    f = torch.randn(P, 1, device=dev, generator=gen)
    W = f * torch.rand(1, a.wide_labs, device=dev, generator=gen) + torch.randn(P, a.wide_labs, device=dev, generator=gen)
    W[torch.rand(P, a.wide_labs, device=dev, generator=gen) >= 0.3] = float("nan")
    key = f"synthetic_{P}x{a.wide_labs}"
    res["shapes"][key] = measure(W, a, a.sklearn_rows)
    print(json.dumps({key: res["shapes"][key]}), flush=True)
    dump()


if __name__ == "__main__":
    main()
