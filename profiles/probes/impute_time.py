"""Dense imputation against the pair path at the eICU shape (synth.make_graph), eval mode, in one process:
  (a) k_pair_dense_fwd alone, both heads over all patients   (kernel time: the launches' own event pairs, ops.probe_*)
  (b) HeteroRGCN.impute_lab_matrix end to end                (device events around the call)
  (c) predict_lab_values over the explicit P x L pair list, its _pairs build (sort, head lists) included
  (d) k_pair_fwd_mfma alone over that list                   (kernel time, as (a))
and, with --x1000, (a) and (b) at x1000.  Medians over --reps after --warmup calls; one JSON object on stdout (and in
--out).  The matrix-issue bound is tiles x 24 v_mfma_f32_32x32x16_bf16 x 32 cycles over 1024 SIMDs at 2.4 GHz.

  python profiles/probes/impute_time.py --dim 128 --reps 10 --x1000 --out <dir>/impute_time.json
  rocprofv3 --kernel-trace --stats -d <dir> -o impute -- python profiles/probes/impute_time.py --once
  python profiles/probes/impute_time.py --table <dir>/impute_results.db profiles/<name>
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import mmgnn  # noqa: E402,F401
from mmgnn import ops  # noqa: E402
from mmgnn.model import build_model  # noqa: E402
from mmgnn.synth import make_graph  # noqa: E402

SIMDS, CLOCK_HZ, MFMA_PER_TILE, MFMA_CYCLES = 1024, 2.4e9, 24, 32


def issue_bound_us(cells):
    return (cells + 31) // 32 * MFMA_PER_TILE * MFMA_CYCLES / SIMDS / CLOCK_HZ * 1e6


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def kernel_ms(fn, family):
    """Sum of the durations of the launches of one kernel family inside fn()."""
    ops.probe_arm(1 << 15)
    fn()
    torch.cuda.synchronize()
    rows = ops.probe_read()
    return sum(r[0] for r in rows if r[1] == family), sum(r[2] for r in rows if r[1] == family)


def med(xs):
    return statistics.median(xs)


def eval_model(scale, dim, dev):
    """bench.py's workload: synth.make_graph(scale, seed 0) and the model built after torch.manual_seed(42), in eval."""
    g = make_graph(scale, seed=0, device=dev)
    torch.manual_seed(42)
    cfg = {"model": {"architecture": "RGCN", "hidden_dim": dim, "num_layers": 2, "dropout": 0.2,
                     "use_batch_norm": True, "activation": "relu"}}
    model = build_model(cfg, (g.node_types, g.edge_types), None).to(dev)
    model._init_embeddings(g)
    model.eval()
    return g, model


def run_scale(scale, dim, reps, warmup, pairs, dev):
    g, model = eval_model(scale, dim, dev)
    P, L = int(g["patient"].num_nodes), int(g["lab"].num_nodes)
    cells = P * L
    rec = dict(scale=scale, dim=dim, patients=P, labs=L, cells=cells, reps=reps, warmup=warmup)
    with torch.no_grad():
        imp = lambda: model.impute_lab_matrix(g)                        # noqa: E731
        for _ in range(warmup):
            dense = imp()
        a, b = [], []
        for _ in range(reps):
            ms, n = kernel_ms(imp, "pair_head_dense_fwd")
            assert n == cells, (n, cells)
            a.append(ms)
            b.append(timed(imp)[0])
        rec.update(a_dense_kernel_ms=med(a), b_impute_ms=med(b), a_runs_ms=a, b_runs_ms=b,
                   dense_issue_bound_us=issue_bound_us(cells),
                   dense_issue_share=issue_bound_us(cells) / 1e3 / med(a), dense_ns_per_cell=med(a) * 1e6 / cells)
        if pairs:
            pi = torch.arange(P, device=dev).repeat_interleave(L)
            li = torch.arange(L, device=dev).repeat(P)

            def pred():
                model._pair_cache.clear()                # the _pairs build (sort + head lists) is part of every call
                return model.predict_lab_values(g, pi, li)
            for _ in range(warmup):
                p = pred()
            c, d = [], []
            for _ in range(reps):
                ms, n = kernel_ms(pred, "pair_head_fwd")
                assert n == cells, (n, cells)            # (each head launch is bounded by its own list)
                d.append(ms)
                c.append(timed(pred)[0])
            rec.update(c_predict_pairs_ms=med(c), d_pair_kernel_ms=med(d), c_runs_ms=c, d_runs_ms=d,
                       pair_ns_per_pair=med(d) * 1e6 / cells,
                       dense_equals_pairs=bool(torch.equal(dense.view(-1), p)))
    del g, model
    torch.cuda.empty_cache()
    return rec


def table(db, prefix):
    """Per-kernel totals of the dispatches behind the warm-up call: the second half of the k_pair_dense_fwd launches
    belongs to the measured call, which starts right after the last launch of the first half (no GPU needed)."""
    import csv
    import sqlite3
    rows = sqlite3.connect(db).execute("select name, start, end from kernels order by start").fetchall()
    dense = [r for r in rows if "k_pair_dense_fwd" in r[0]]
    cut = dense[len(dense) // 2 - 1][2]
    mine = [r for r in rows if r[1] > cut]
    agg = {}
    for name, t0, t1 in mine:
        a = agg.setdefault(name, [0, 0])
        a[0] += 1
        a[1] += t1 - t0
    tot = sum(a[1] for a in agg.values())
    span = mine[-1][2] - mine[0][1]
    order = sorted(agg.items(), key=lambda kv: -kv[1][1])
    with open(prefix + ".csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage"])
        for name, (n, ns) in order:
            w.writerow([name, n, ns, ns / n, round(100 * ns / tot, 2)])
    with open(prefix + ".txt", "w") as f:
        f.write(f"one impute_lab_matrix call (x100, 128-d, eval): {len(mine)} kernels, {tot / 1e6:.3f} ms of kernel time, "
                f"{span / 1e6:.3f} ms first start -> last end\n")
        for name, (n, ns) in order:
            f.write(f"{ns / 1e6:9.3f} ms {100 * ns / tot:5.1f}%  calls {n:5d}  avg {ns / n / 1e3:8.1f} us  {name[:120]}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--x1000", action="store_true", help="also (a) and (b) at x1000")
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true",
                    help="a warm-up and one impute_lab_matrix call at x100, nothing else (for rocprofv3 --kernel-trace)")
    ap.add_argument("--table", nargs=2, metavar=("DB", "PREFIX"),
                    help="kernel table (PREFIX.csv / .txt) of the last call of a --once trace (rocprofv3 database)")
    args = ap.parse_args()
    if args.table:
        table(*args.table)
        return
    if not torch.cuda.is_available():
        raise SystemExit("impute_time: needs a GPU (no CPU timing)")
    dev = torch.device("cuda:0")
    if args.once:
        g, model = eval_model(100, args.dim, dev)
        with torch.no_grad():
            model.impute_lab_matrix(g)               # warm-up: graph plan, code objects (cut off by --table)
            torch.cuda.synchronize()
            out = model.impute_lab_matrix(g)
        torch.cuda.synchronize()
        print(json.dumps(dict(once=list(out.shape))))
        return
    res = dict(device=torch.cuda.get_device_name(0), x100=run_scale(100, args.dim, args.reps, args.warmup, True, dev))
    if args.x1000:
        res["x1000"] = run_scale(1000, args.dim, max(3, args.reps // 2), 2, False, dev)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
