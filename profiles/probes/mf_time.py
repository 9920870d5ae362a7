"""Low-rank (ALS) imputation timings on the train edges of the eICU-shaped synthetic graphs (synth.make_graph: x1 1,834,
x100 183,400, x1000 1,834,000 patients x 50 labs).
  half-sweeps   the patient and the lab half-sweep one by one (device events around mmg_mf_half_sweep, medians), each as
                a fraction of its fp64 issue bound -- pairs (r (r + 1) / 2 + r) fused multiply-adds at the vendor's
                published vector rate -- and of one read of its pairs, the other side's factors and its own output at the
                8 TB/s data-sheet rate; the kernels inside them from the library's launch probe
  round         one round eager against one replay of the round captured into a hipGraph
  fit           LowRankLabImputer(rank, max_iter=--rounds, tol=0).fit end to end (host clock; one read at the end)
  numpy         the restatement of the same module on the same box: all rounds at x1; ONE round elsewhere, EXTRAPOLATED
                linearly in rounds (flagged); scales past --numpy-scale are extrapolated linearly in pairs from the last
                measured one (flagged)
  accuracy      the test-split MAE of low_rank beside per_lab_mean, chained_equations and a briefly trained GNN on the x1
                graph: a plumbing figure (the synthetic labs are independent by construction), not a ranking

  python profiles/probes/mf_time.py --scales 1 100 1000 --out <dir>/mf_time.json
"""
import argparse
import json
import os
import platform
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import mmgnn  # noqa: E402,F401
from mmgnn import evaluate as ev  # noqa: E402
from mmgnn import lowrank as lr  # noqa: E402
from mmgnn import mf_ops as mo  # noqa: E402
from mmgnn import ops  # noqa: E402
from mmgnn.lowrank import LowRankLabImputer  # noqa: E402
from mmgnn.synth import make_graph  # noqa: E402
from mmgnn.train import EdgeMasker  # noqa: E402

HBM_BYTES_PER_S = 8e12
FP64_VECTOR_FLOPS = 78.6e12          # published peak of the MI355X (data sheet), not measured


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"ms": statistics.median(ts), "all_ms": ts}


def half_sweep_bounds(ms, pairs, segments, m, r):
    fma = pairs * (r * (r + 1) // 2 + r)
    nbytes = pairs * 12 + 8 * r * (m + segments) + 8 * (segments + 1)
    return {"ms": ms, "pairs": pairs, "segments": segments, "fused_multiply_adds": fma,
            "fraction_of_fp64_issue_bound": 2 * fma / (ms * 1e-3) / FP64_VECTOR_FLOPS,
            "bytes_one_read": nbytes, "fraction_of_one_hbm_read": nbytes / (ms * 1e-3) / HBM_BYTES_PER_S}


def measure(p, lab, v, P, L, a, numpy_rounds):
    r = a.rank
    t0 = time.perf_counter()
    ix = mo.mf_index(p, lab, v, P, L)
    torch.cuda.synchronize()
    res = {"patients": P, "labs": L, "pairs": ix.nnz, "rank": r, "index_first_call_ms": (time.perf_counter() - t0) * 1e3,
           "index": timed(lambda: mo.mf_index(p, lab, v, P, L), a.reps),
           "longest_lab": int(ix.count.max().item()), "lab_jobs_of_the_split_path": int(
               sum(-(-int(c) // mo.MF_CHUNK) for c in ix.count.tolist() if c > mo.MF_SPLIT)),
           "workspace_bytes": {"patient": int(mo.load().mmg_mf_half_sweep_ws_bytes(P, ix.nnz, r)),
                               "lab": int(mo.load().mmg_mf_half_sweep_ws_bytes(L, ix.nnz, r))}}
    V0 = torch.from_numpy(np.random.default_rng(0).standard_normal((L, r)) * 0.1).to(p.device)
    als = lr._DeviceALS(ix, V0.clone(), 1.0, 1)
    als.round(0)                                              # warm-up
    torch.cuda.synchronize()
    ops.probe_arm(64)
    als.round(0)
    torch.cuda.synchronize()
    res["kernels_ms_of_a_round_in_launch_order"] = [(sym.split("(")[0].strip(), ms) for ms, _, _, _, _, _, sym in ops.probe_read()]
    ops.probe_arm(0)
    res["patient_half_sweep"] = half_sweep_bounds(timed(als.patient_half, a.reps)["ms"], ix.nnz, P, L, r)
    res["lab_half_sweep"] = half_sweep_bounds(timed(als.lab_half, a.reps)["ms"], ix.nnz, L, P, r)
    res["objective"] = timed(lambda: mo.mf_objective(ix, als.U, als.V, als.obj[0]), a.reps)
    res["round_eager"] = timed(lambda: als.round(0), a.reps)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        als.round(0)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        als.round(0)
    res["round_graph_replay"] = timed(graph.replay, a.reps)
    del graph, als
    ts = []
    for _ in range(a.fit_reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        imp = LowRankLabImputer(rank=r, max_iter=a.rounds, tol=0).fit(p, lab, v, P, L)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    res["fit_end_to_end"] = {"rounds": a.rounds, "ms": statistics.median(ts[1:]), "all_ms_first_is_warmup": ts,
                             "objective_first_and_last_round": [imp.history_[0], imp.history_[-1]]}
    if numpy_rounds:
        t0 = time.perf_counter()
        ph, lh, vh = p.cpu().numpy(), lab.cpu().numpy(), v.cpu().numpy()
        copy_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        host = LowRankLabImputer(rank=r, max_iter=numpy_rounds, tol=0).fit(ph, lh, vh, P, L)
        np_ms = (time.perf_counter() - t0) * 1e3
        full = np_ms * a.rounds / numpy_rounds
        res["host"] = {"copy_ms": copy_ms, "numpy_measured_ms": np_ms, "numpy_rounds": numpy_rounds,
                       "numpy_ms_for_the_fit": full, "EXTRAPOLATED": numpy_rounds != a.rounds}
        res["speedup_end_to_end"] = (copy_ms + full) / res["fit_end_to_end"]["ms"]
        if numpy_rounds == a.rounds:
            res["max_abs_difference_of_the_lab_factors"] = float(np.abs(imp.lab_factors_.cpu().numpy() - host.lab_factors_).max())
    return res


def gnn_mae(g, masker, dev, epochs):
    from mmgnn.model import build_model
    from mmgnn.train import Trainer
    cfg = {"model": {"architecture": "RGCN", "hidden_dim": 64, "num_layers": 2, "dropout": 0.0, "use_batch_norm": True,
                     "activation": "relu"},
           "train": {"optimizer": {"type": "adam", "lr": 1e-2, "weight_decay": 1e-5}, "lr_scheduler": {"enabled": False},
                     "loss": "mae", "epochs": epochs, "early_stopping_patience": epochs, "train_split": 0.7, "val_split": 0.15,
                     "test_split": 0.15, "mask_fraction": 0.2, "seed": 42, "device": "cuda"},
           "logging": {"save_checkpoints": False}}
    torch.manual_seed(0)
    model = build_model(cfg, (g.node_types, g.edge_types), None)
    trainer = Trainer(model, g, masker, cfg, dev)
    with tempfile.TemporaryDirectory() as d:
        hist = trainer.train(d)
    te_ei, te_v, _, _ = masker.get_masked_data("test", want_mask=False)
    model.eval()
    with torch.no_grad():
        pred = model.predict_lab_values(trainer.data, te_ei[0].to(dev), te_ei[1].to(dev))
    m = ev.compute_regression_metrics(pred.float().cpu().numpy().reshape(-1), te_v.cpu().numpy().reshape(-1))
    return {"mae": m["mae"], "epochs": len(hist["train_loss"]), "last_val_loss": hist["val_loss"][-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="+", default=[1, 100, 1000])
    ap.add_argument("--numpy-scale", type=int, default=100, help="the largest scale at which the numpy path is run")
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fit-reps", type=int, default=2)
    ap.add_argument("--gnn-epochs", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "numpy": np.__version__, "hbm_bytes_per_s_DATA_SHEET": HBM_BYTES_PER_S,
           "fp64_vector_flops_per_s_DATA_SHEET_NOT_MEASURED": FP64_VECTOR_FLOPS,
           "host_threads": {"torch": torch.get_num_threads(), "OMP_NUM_THREADS": os.environ.get("OMP_NUM_THREADS")},
           "chunk": mo.MF_CHUNK, "split": mo.MF_SPLIT, "reps": a.reps, "rounds": a.rounds, "shapes": {}}

    def dump():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    last_numpy = None
    for scale in a.scales:
        g = make_graph(scale, seed=0, device=dev)
        masker = EdgeMasker(g)
        tr_ei, tr_v, _, _ = masker.get_masked_data("train", want_mask=False)
        P, L = int(g["patient"].num_nodes), int(g["lab"].num_nodes)
        p, lab, v = tr_ei[0].to(dev).contiguous(), tr_ei[1].to(dev).contiguous(), tr_v.to(dev).reshape(-1).float().contiguous()
        key = f"x{scale}_{P}x{L}_train_edges"
        numpy_rounds = (a.rounds if scale == 1 else 1) if scale <= a.numpy_scale else 0
        r = measure(p, lab, v, P, L, a, numpy_rounds)
        if numpy_rounds:
            last_numpy = (r["pairs"], r["host"]["numpy_ms_for_the_fit"])
        elif last_numpy:
            full = last_numpy[1] * r["pairs"] / last_numpy[0]
            r["host"] = {"numpy_ms_for_the_fit": full, "EXTRAPOLATED": True, "from_pairs": last_numpy[0]}
            r["speedup_end_to_end"] = full / r["fit_end_to_end"]["ms"]
        res["shapes"][key] = r
        print(json.dumps({key: r}), flush=True)
        dump()
        if scale == 1:
            te_ei, te_v, _, _ = masker.get_masked_data("test", want_mask=False)
            tv, ti = tr_v.cpu().numpy().reshape(-1), tr_ei.cpu().numpy()
            acc = ev.evaluate_baselines((tv, ti[1]), (te_v.cpu().numpy().reshape(-1), te_ei.cpu().numpy()[1], None))
            acc.update(ev.evaluate_chained_baseline(g, masker, "test"))
            acc.update(ev.evaluate_lowrank_baseline(g, masker, "test"))                 # the defaults: rank 8, reg 1
            acc[f"low_rank_rank{a.rank}_{a.rounds}_rounds"] = ev.evaluate_lowrank_baseline(
                g, masker, "test", rank=a.rank, max_iter=a.rounds, tol=0.0)["low_rank"]
            out = {k: m["mae"] for k, m in acc.items()}
            out["low_rank_sweep_val_split"] = ev.lowrank_sweep(g, masker).to_dict("records")
            try:
                out["gnn_briefly_trained"] = gnn_mae(g, masker, dev, a.gnn_epochs)
            except Exception as e:                                                      # the timings above stand
                out["gnn_briefly_trained"] = {"error": repr(e)}
            res["accuracy_x1_test_split_NOT_ASSERTED"] = out
            print(json.dumps(out), flush=True)
            dump()
        del g, masker, p, lab, v, tr_ei, tr_v
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
