"""The fp64 Cholesky solve (csrc/chol64.h) inside its three users, timed against ANOTHER build of the libraries -- the
parent commit's -- in the same call, so that the noise of a shared host is measured beside the difference.
  chain   mmg_chain_solve at L = 50 and L = 128 (every lab active, one target)
  prop    mmg_prop_solve at D = 128 with 50 live labs in the batch
  mf      mmg_mf_half_sweep, the patient side and the lab side, over all has_lab pairs of the x1 and x100 synthetic graphs
          (synth.make_graph) at rank 8 and rank 32
A measurement is one fresh process per (build, round): after a warm-up it times windows of calls between two device
events, each window sized to run about --window-ms, and keeps the per-call time of the fastest of three windows.  The
driver alternates the two builds --rounds times each and never opens the device itself.  A case PASSES when the new
build's median over the rounds is at most the reference's median plus the reference's own range (max - min over its
rounds): the reference is the other build, never this one.

  python profiles/solve_time.py REFERENCE_LIB_DIR [--new LIB_DIR] [--rounds 5] [--out profiles/solve_time.json]

A LIB_DIR holds libmmgnn.so and its satellites as `make -C multi-modal-gnn_amd/csrc` leaves them beside the package.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PACKAGE = os.path.join(ROOT, "multi-modal-gnn_amd")


def measure(lib_dir, window_ms):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import mmgnn  # noqa: F401
    from mmgnn import _lib, chain_ops, mf_ops, prop_ops
    from mmgnn.synth import make_graph
    _lib.LIB_PATH = os.path.join(lib_dir, "libmmgnn.so")          # before the first load
    for mod, stem in ((chain_ops, "chain"), (mf_ops, "mf"), (prop_ops, "prop")):
        mod.BINDING.lib_path = os.path.join(lib_dir, f"libmmgnn_{stem}.so")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    out = {}

    def timed(name, fn):
        def window(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / reps
        window(3)                                                 # warm-up: workspaces, the LDS attribute
        reps = max(3, int(window_ms / max(window(3), 1e-3)))
        out[name] = {"reps": reps, "ms": min(window(reps) for _ in range(3))}
        print(name, out[name], file=sys.stderr, flush=True)

    for L in (50, 128):
        u = rng.standard_normal((4 * L, L))
        G, s = to(u.T @ u), to(u.sum(0))
        n_j = torch.full((1,), 4 * L, dtype=torch.int64, device=dev)
        count = torch.full((L,), 4 * L, dtype=torch.int64, device=dev)
        w, mu = torch.empty(L, dtype=torch.float64, device=dev), torch.empty(L, dtype=torch.float64, device=dev)
        bad = torch.zeros(1, dtype=torch.int64, device=dev)
        timed(f"chain_solve_L{L}", lambda: chain_ops.chain_solve(G, s, n_j, count, L // 2, 1.0, w, mu, bad))
        assert int(bad.item()) == 0 and bool(torch.isfinite(w).all())

    D, nb = 128, 50
    M = D + 1
    ut = np.concatenate([rng.standard_normal((nb, 4 * M, D)), np.ones((nb, 4 * M, 1))], axis=2)
    H = np.einsum("kia,kib->kab", ut * 0.25, ut)
    H, g = to(np.triu(H) + np.triu(H, 1).transpose(0, 2, 1)), to(rng.standard_normal((nb, M)))
    trial = to(rng.standard_normal((nb, M)) * 0.1)
    state = torch.zeros(nb, prop_ops.PR_STATE, dtype=torch.int32, device=dev)
    state[:, prop_ops.DEFINES["MMG_PR_ACTIVE"]] = 1
    delta, dec = torch.empty(nb, M, dtype=torch.float64, device=dev), torch.empty(nb, dtype=torch.float64, device=dev)
    timed(f"prop_solve_D{D}_labs{nb}", lambda: prop_ops.prop_solve(H, g, trial, 0, 1.0, state, delta, dec))
    assert int(state[:, prop_ops.DEFINES["MMG_PR_BAD"]].sum().item()) == 0 and bool(torch.isfinite(delta).all())

    for scale in (1, 100):
        gr = make_graph(scale, seed=0, device=dev) if scale > 1 else make_graph(scale, seed=0).to(dev)
        ei = gr["patient", "has_lab", "lab"].edge_index
        v = gr["patient", "has_lab", "lab"].edge_attr.reshape(-1).float().contiguous()
        P, L = int(gr["patient"].num_nodes), int(gr["lab"].num_nodes)
        ix = mf_ops.mf_index(ei[0].contiguous(), ei[1].contiguous(), v, P, L)
        for r in (8, 32):
            V0 = to(rng.standard_normal((L, r)) * 0.1)
            U, V = torch.zeros(P, r, dtype=torch.float64, device=dev), torch.zeros(L, r, dtype=torch.float64, device=dev)
            bad = torch.zeros(1, dtype=torch.int64, device=dev)
            timed(f"mf_half_sweep_patients_x{scale}_r{r}",
                  lambda: mf_ops.mf_half_sweep(ix.p_ptr, ix.p_idx, ix.p_y, V0, 1.0, U, bad))
            timed(f"mf_half_sweep_labs_x{scale}_r{r}",
                  lambda: mf_ops.mf_half_sweep(ix.l_ptr, ix.l_idx, ix.l_y, U, 1.0, V, bad))
            assert int(bad.item()) == 0 and bool(torch.isfinite(V).all())
        del gr, ix
        torch.cuda.empty_cache()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "cases": out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="the directory of the libraries to compare against (the parent commit's build)")
    ap.add_argument("--new", default=PACKAGE, help="the directory of the libraries under test")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(HERE, "solve_time.json"))
    ap.add_argument("--measure", action="store_true", help="(the driver's child) measure `reference` and print one JSON line")
    a = ap.parse_args()
    if a.measure:
        return measure(os.path.abspath(a.reference), a.window_ms)
    dirs = {"reference": os.path.abspath(a.reference), "new": os.path.abspath(a.new)}
    runs, device = {"reference": [], "new": []}, None
    for rnd in range(a.rounds):
        for which in ("reference", "new"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), dirs[which], "--measure", "--window-ms",
                                str(a.window_ms)], stdout=subprocess.PIPE, text=True, timeout=a.child_timeout)
            if p.returncode != 0:                                 # nothing more is started on the device
                sys.exit(f"round {rnd}, {which}: the measuring process ended with {p.returncode}")
            res = json.loads(p.stdout.strip().splitlines()[-1])
            device = res["device"]
            runs[which].append(res["cases"])
            print(rnd, which, {k: round(c["ms"], 4) for k, c in res["cases"].items()}, flush=True)
    out = {"device": device, "rounds": a.rounds, "window_ms": a.window_ms,
           "rule": "new median <= reference median + (reference max - reference min)", "cases": {}}
    for name in runs["reference"][0]:
        ref, new = ([r[name]["ms"] for r in runs[w]] for w in ("reference", "new"))
        rm, rr, nm = statistics.median(ref), max(ref) - min(ref), statistics.median(new)
        out["cases"][name] = {"reference_ms": ref, "new_ms": new, "reference_median_ms": rm, "reference_range_ms": rr,
                              "new_median_ms": nm, "new_over_reference": nm / rm, "passes": nm <= rm + rr,
                              "calls_per_window": runs["new"][0][name]["reps"]}
        print(f"{name:36s} ref {rm:9.4f} ms (range {rr:7.4f})  new {nm:9.4f} ms  {nm / rm:6.3f}  "
              f"{'ok' if nm <= rm + rr else 'OUTSIDE'}", flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
