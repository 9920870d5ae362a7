"""Nearest-neighbour imputation (mmg_knn_impute) at the eICU shape (synth.make_graph, train split of an EdgeMasker),
k = 5, uniform weights, in one process, per scale:
  (a) the test-split cells: KNNLabImputer.predict over the test pairs (one kernel call over the unique test patients)
  (b) impute_matrix over all patients
Each with the kernel time (the launches' own event pairs, ops.probe_*: column means + the main kernel) and the call time
(device events around the call).  Medians over --reps after --warmup calls.  The bound is the distance arithmetic alone:
receivers x donors x the receivers' mean observed labs x 3 VALU ops over 1024 SIMDs x 32 lanes x 2.4 GHz.
--sklearn adds sklearn KNNImputer.fit_transform of the x1 matrix on the host (threads: OMP_NUM_THREADS).
--x1000 adds a sampled-receiver figure at x1000 (kernel time of --sample receivers against all donors).

  python profiles/probes/knn_time.py --scales 1 10 100 --sklearn --x1000 --out <dir>/knn_time.json
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
from mmgnn import ops  # noqa: E402
from mmgnn.knn import KNNLabImputer  # noqa: E402
from mmgnn.synth import make_graph  # noqa: E402
from mmgnn.train import EdgeMasker  # noqa: E402

LANE_OPS_PER_S = 1024 * 32 * 2.4e9


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def kernel_ms(fn):
    ops.probe_arm(1 << 10)
    fn()
    torch.cuda.synchronize()
    return sum(r[0] for r in ops.probe_read() if r[1] == "knn_impute")


def measure(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    call = [timed(fn) for _ in range(reps)]
    kern = [kernel_ms(fn) for _ in range(reps)]
    return dict(kernel_ms=round(statistics.median(kern), 4), call_ms=round(statistics.median(call), 4),
                kernel_ms_min=round(min(kern), 4), kernel_ms_max=round(max(kern), 4))


def bound_ms(X, rows):
    obs = (~torch.isnan(X[rows.long()])).sum(1).double().mean().item()
    return rows.numel() * X.shape[0] * obs * 3 / LANE_OPS_PER_S * 1e3, obs


def fitted(scale, dev, k):
    g = make_graph(scale, seed=0, device=dev)
    m = EdgeMasker(g)
    ei, ev, _, _ = m.get_masked_data("train", want_mask=False)
    imp = KNNLabImputer(k, "uniform").fit(ei[0], ei[1], ev, g["patient"].num_nodes, g["lab"].num_nodes)
    te, _, _, _ = m.get_masked_data("test", want_mask=False)
    return imp, te


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="+", default=[1, 10, 100])
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--x1000", action="store_true")
    ap.add_argument("--sample", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), k=a.k, weights="uniform", reps=a.reps, warmup=a.warmup,
               scales={})
    for s in a.scales:
        imp, te = fitted(s, dev, a.k)
        X = imp.X
        uniq = torch.unique(te[0]).to(torch.int32)
        allr = torch.arange(X.shape[0], dtype=torch.int32, device=dev)
        ba, obs_a = bound_ms(X, uniq)
        bb, obs_b = bound_ms(X, allr)
        r = dict(patients=X.shape[0], labs=X.shape[1], train_cells=int((~torch.isnan(X)).sum()),
                 test_pairs=int(te.shape[1]), test_patients=int(uniq.numel()))
        r["a_test_cells"] = dict(measure(lambda: imp.predict(te[0], te[1]), a.reps, a.warmup), receivers=int(uniq.numel()),
                                 mean_observed_labs=round(obs_a, 2), bound_ms=round(ba, 4))
        r["b_impute_matrix"] = dict(measure(lambda: imp.impute_matrix(), a.reps, a.warmup), receivers=X.shape[0],
                                    mean_observed_labs=round(obs_b, 2), bound_ms=round(bb, 4))
        for m in ("a_test_cells", "b_impute_matrix"):
            r[m]["kernel_over_bound"] = round(r[m]["kernel_ms"] / r[m]["bound_ms"], 2)
        res["scales"][f"x{s}"] = r
        print(json.dumps({f"x{s}": r}), flush=True)
        if s == 1 and a.sklearn:
            try:
                from sklearn.impute import KNNImputer
            except ImportError:
                res["sklearn_x1"] = "sklearn not installed"
            else:
                Xh = X.cpu().numpy()
                t = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    KNNImputer(n_neighbors=a.k).fit_transform(Xh)
                    t.append((time.perf_counter() - t0) * 1e3)
                cpu = next((ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")), "?")
                res["sklearn_x1"] = dict(ms=round(statistics.median(t), 1), runs=len(t), host=platform.node(), cpu=cpu,
                                         threads=os.environ.get("OMP_NUM_THREADS", "unset"),
                                         sklearn=__import__("sklearn").__version__)
                print(json.dumps({"sklearn_x1": res["sklearn_x1"]}), flush=True)
        del imp, X
        torch.cuda.empty_cache()
    if a.x1000:
        imp, _ = fitted(1000, dev, a.k)
        X = imp.X
        rows = torch.from_numpy(np.sort(np.random.default_rng(0).choice(X.shape[0], a.sample, replace=False))).to(
            device=dev, dtype=torch.int32)
        b, obs = bound_ms(X, rows)
        r = dict(measure(lambda: ops.knn_impute(X, rows, a.k), 2, 1), patients=X.shape[0], receivers=a.sample,
                 mean_observed_labs=round(obs, 2), bound_ms=round(b, 4))
        r["kernel_over_bound"] = round(r["kernel_ms"] / r["bound_ms"], 2)
        res["x1000_sampled"] = r
        print(json.dumps({"x1000_sampled": r}), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
