"""Device graph build timings on the events of synth.make_graph(scale): all three relations, both directions.
  device_ms      mmgnn.graph_build.build_graph_from_events, device event tensors in, HeteroGraph on the device out -- host
                 clock around the call, which ends in the device synchronise the entry points themselves do (their counts
                 come back) and includes validate_graph; median over --reps after --warmup;
  kernels_ms     the four mmg_first_seen_index and three mmg_edge_build calls of that build alone (ops level, same clock);
  roofline       the builder's ALGORITHMIC bytes -- every event column read once (16 bytes a row, 24 with the lab value;
                 the item column a second time for the first-seen pass: 8 more), the cohort read once, every output
                 written once (32 bytes an edge for both directions, 4 for the lab value, 4 per code and 8 per node of the
                 tables) -- over device_ms, as a fraction of 8 TB/s;
  host           what a user has without the kernels, on the same box in the same run: the copy of the event tensors to
                 the host (copy_ms) and build_heterogeneous_graph on the equivalent frames (frames_ms; the ids are the
                 integer codes, so the pandas factorisation is at its cheapest).
No time is asserted anywhere.

  python profiles/probes/graph_time.py --scales 1 10 100 --out profiles/graph_time_x1_x10_x100.json
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
from mmgnn import graph_build as gb, ops  # noqa: E402
from mmgnn.synth import make_graph  # noqa: E402

HBM_BYTES_PER_S = 8e12
CFG = {"graph": {"edge_types": {k: {"enabled": True, "bidirectional": True}
                                for k in ("patient_lab", "patient_diagnosis", "patient_medication")}}}
RELS = (("has_lab", "lab"), ("has_diagnosis", "diagnosis"), ("has_medication", "medication"))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="+", default=[1, 10, 100])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "numpy": np.__version__, "pandas": pd.__version__, "hbm_roofline_bytes_per_s": HBM_BYTES_PER_S, "scales": {}}
    for s in a.scales:
        src = make_graph(s, seed=3, device=dev, with_reverse=False)
        n_codes = {t: int(src[t].num_nodes) for t in ("patient", "lab", "diagnosis", "medication")}
        cohort = torch.arange(n_codes["patient"], device=dev)
        cols = []
        for rel, node in RELS:
            ei = src["patient", rel, node].edge_index
            cols.append((ei[0].contiguous(), ei[1].contiguous()))
        value = src["patient", "has_lab", "lab"].edge_attr.squeeze(-1).double().contiguous()
        labs = (cols[0][0], cols[0][1], value)

        build = lambda: gb.build_graph_from_events(cohort, labs, cols[1], cols[2], n_codes, CFG)   # noqa: E731
        g = build()
        rows = {node: int(c[0].numel()) for (_, node), c in zip(RELS, cols)}
        edges = {node: int(g["patient", rel, node].edge_index.shape[1]) for rel, node in RELS}
        assert edges == rows and torch.equal(g["patient", "has_lab", "lab"].edge_index, src["patient", "has_lab", "lab"].edge_index)
        n_rows, n_edges = sum(rows.values()), sum(edges.values())
        algo = (16 + 8) * n_rows + 8 * rows["lab"] + 8 * n_codes["patient"] + 32 * n_edges + 4 * edges["lab"] + \
            sum(4 * n_codes[t] + 8 * int(g[t].num_nodes) for t in n_codes)
        r = {"rows": rows, "patients": n_codes["patient"], "directed_edges": 2 * n_edges, "algorithmic_bytes": algo}
        r["device_ms"], r["device_all_ms"] = host_clock(build, a.reps, a.warmup)
        r["roofline_fraction"] = algo / (r["device_ms"] * 1e-3) / HBM_BYTES_PER_S

        def kernels():
            index = {"patient": ops.first_seen_index(cohort, n_codes["patient"])[0]}
            for (_, node), c in zip(RELS, cols):
                index[node] = ops.first_seen_index(c[1], n_codes[node])[0]
            for (_, node), c in zip(RELS, cols):
                ops.edge_build(c[0], c[1], index["patient"], index[node], value if node == "lab" else None)

        r["kernels_ms"], r["kernels_all_ms"] = host_clock(kernels, a.reps, a.warmup)

        flat = [cohort, value] + [x for c in cols for x in c]
        copy_ms, copy_all = host_clock(lambda: [x.cpu() for x in flat], a.host_reps, 1)
        frames = [pd.DataFrame({"SUBJECT_ID": cohort.cpu().numpy()}),
                  pd.DataFrame({"SUBJECT_ID": cols[0][0].cpu().numpy(), "ITEMID": cols[0][1].cpu().numpy(),
                                "VALUE_NORMALIZED": value.cpu().numpy()}),
                  pd.DataFrame({"SUBJECT_ID": cols[1][0].cpu().numpy(), "ICD3_CODE": cols[1][1].cpu().numpy()}),
                  pd.DataFrame({"SUBJECT_ID": cols[2][0].cpu().numpy(), "DRUG": cols[2][1].cpu().numpy()})]
        labitems = pd.DataFrame({"ITEMID": np.arange(n_codes["lab"])})
        ts = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            h = gb.build_heterogeneous_graph(frames[0], frames[1], frames[2], frames[3], frames[0], labitems, CFG)
            ts.append((time.perf_counter() - t0) * 1e3)
        assert torch.equal(h["patient", "has_lab", "lab"].edge_index, g["patient", "has_lab", "lab"].edge_index.cpu())
        r["host"] = {"copy_ms": copy_ms, "copy_all_ms": copy_all, "frames_ms": statistics.median(ts), "frames_all_ms": ts,
                     "copy_plus_frames_ms": copy_ms + statistics.median(ts)}
        r["speedup"] = r["host"]["copy_plus_frames_ms"] / r["device_ms"]
        res["scales"][str(s)] = r
        print(json.dumps({s: r}), flush=True)
        del src, g, h, frames, cols, labs, value, cohort, flat
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
