"""The entry points that run on the sorted pair list (csrc/segsort.h), timed against ANOTHER build of the libraries -- the
parent commit's -- in the same call, so that the noise of a shared host is measured beside the difference.  The inputs
are those of probes/boot_time.py, shift_time.py, probes/stack_time.py, probes/conformal_time.py and prop_time.py at the
x100 shape (synth.make_graph): a seeded 15 % of the has_lab pairs (the patients of two cohorts for shift), 1,000
replicates, int64 indices.
  boot_sums        F = 7 and F = 10 (the case that pays for the third in-kernel search of k_boot_combine)
  shift_stats      keys, sort, bounds, both walks, both combines
  stack_sums       K = 2 at 1 and 5 folds;   stack_scores
  cf_fit           the three segmented order statistics;   cf_coverage
  prop_pair_sums   stabilised weights
A measurement is one fresh process per (build, round): after a warm-up it times windows of calls between two device
events, each window sized to run about --window-ms, and keeps the per-call time of the fastest of three windows.  The
driver alternates the two builds --rounds times each and never opens the device itself.  A case PASSES when the new
build's median over the rounds is at most the reference's median plus the reference's own range (max - min over its
rounds): the reference is the other build, never this one.

  python profiles/segsort_time.py REFERENCE_LIB_DIR [--new LIB_DIR] [--rounds 5] [--out profiles/segsort_time.json]

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
EDGES = [1.0, 6.0, 16.0, float("inf")]


def measure(lib_dir, window_ms, scale, replicates):
    import torch
    sys.path.insert(0, ROOT)
    import mmgnn  # noqa: F401
    from mmgnn import _lib, boot_ops, conformal_ops, prop_ops, shift_ops, stack_ops
    from mmgnn.synth import make_graph
    from mmgnn.train import LAB_EDGE
    _lib.LIB_PATH = os.path.join(lib_dir, "libmmgnn.so")          # before the first load
    for mod, stem in ((boot_ops, "boot"), (conformal_ops, "conformal"), (prop_ops, "prop"), (shift_ops, "shift"),
                      (stack_ops, "stack")):
        mod.BINDING.lib_path = os.path.join(lib_dir, f"libmmgnn_{stem}.so")
    dev = torch.device("cuda:0")
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
        window(3)                                                 # warm-up: workspaces
        reps = max(3, int(window_ms / max(window(3), 1e-3)))
        out[name] = {"reps": reps, "ms": min(window(reps) for _ in range(3))}
        print(name, out[name], file=sys.stderr, flush=True)

    g = make_graph(scale, seed=0, device=dev)
    ei = g[LAB_EDGE].edge_index
    y = g[LAB_EDGE].edge_attr.reshape(-1).float()
    L, P, E = int(g["lab"].num_nodes), int(g["patient"].num_nodes), int(y.numel())
    R = replicates
    gen = torch.Generator(dev).manual_seed(1)
    idx = torch.randperm(E, device=dev, generator=gen)[:int(0.15 * E)].sort().values
    pi, li, t = ei[0][idx].contiguous(), ei[1][idx].contiguous(), y[idx].contiguous()
    p = (t * 0.9 + 0.2 * torch.randn(t.numel(), device=dev, generator=gen)).contiguous()
    base = (t * 0.5 + 0.4 * torch.randn(t.numel(), device=dev, generator=gen)).contiguous()
    deg = torch.bincount(ei[0], minlength=P).to(torch.int32)

    for name, bl in (("boot_sums_F7", None), ("boot_sums_F10", base)):
        o = boot_ops.boot_sums(p, t, pi, li, P, L, R, 0, bl)
        timed(name, lambda: boot_ops.boot_sums(p, t, pi, li, P, L, R, 0, bl, out=o))

    perm = torch.randperm(P, device=dev, generator=gen)
    group = torch.full((P,), 2, dtype=torch.uint8, device=dev)
    group[perm[:int(0.7 * P)]] = 1
    group[perm[int(0.85 * P):]] = 0
    sel = group[ei[0]] <= 1
    spi, sli, sv = ei[0][sel].contiguous(), ei[1][sel].contiguous(), y[sel].contiguous()
    T, _ = shift_ops.shift_thresholds(group, R, 0)
    tabs = shift_ops.shift_stats(sv, sli, spi, group, L, T, 0)
    timed("shift_stats", lambda: shift_ops.shift_stats(sv, sli, spi, group, L, T, 0, out=tabs))
    del spi, sli, sv, tabs

    for folds in (1, 5):
        timed(f"stack_sums_K2_folds{folds}", lambda: stack_ops.stack_sums([p, base], t, pi, li, L, deg, EDGES, folds, 0))
    timed("stack_scores", lambda: stack_ops.stack_scores(base, p, t, pi, li, L, deg, EDGES))
    timed("cf_fit_signed", lambda: conformal_ops.cf_fit(p, t, pi, li, L, deg, EDGES, 0.1, "signed", 30))
    table = conformal_ops.cf_fit(p, t, pi, li, L, deg, EDGES, 0.1, "signed", 30)[0]
    timed("cf_coverage", lambda: conformal_ops.cf_coverage(p, t, pi, li, L, deg, EDGES, table))
    prob = torch.rand(P, L, device=dev, generator=gen).clamp_(0.01, 1.0).contiguous()
    cov = prob.double().mean(0).contiguous()
    timed("prop_pair_sums", lambda: prop_ops.prop_pair_sums(p, t, pi, li, prob, cov, 0.01, True))
    print(json.dumps({"device": torch.cuda.get_device_name(0), "pairs": int(t.numel()), "patients": P, "labs": L,
                      "cases": out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="the directory of the libraries to compare against (the parent commit's build)")
    ap.add_argument("--new", default=PACKAGE, help="the directory of the libraries under test")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--scale", type=int, default=100)
    ap.add_argument("--replicates", type=int, default=1000)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(HERE, "segsort_time.json"))
    ap.add_argument("--measure", action="store_true", help="(the driver's child) measure `reference` and print one JSON line")
    a = ap.parse_args()
    if a.measure:
        return measure(os.path.abspath(a.reference), a.window_ms, a.scale, a.replicates)
    dirs = {"reference": os.path.abspath(a.reference), "new": os.path.abspath(a.new)}
    runs, shape = {"reference": [], "new": []}, None
    for rnd in range(a.rounds):
        for which in ("reference", "new"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), dirs[which], "--measure", "--window-ms",
                                str(a.window_ms), "--scale", str(a.scale), "--replicates", str(a.replicates)],
                               stdout=subprocess.PIPE, text=True, timeout=a.child_timeout)
            if p.returncode != 0:                                 # nothing more is started on the device
                sys.exit(f"round {rnd}, {which}: the measuring process ended with {p.returncode}")
            res = json.loads(p.stdout.strip().splitlines()[-1])
            shape = {k: res[k] for k in ("device", "pairs", "patients", "labs")}
            runs[which].append(res["cases"])
            print(rnd, which, {k: round(c["ms"], 4) for k, c in res["cases"].items()}, flush=True)
    out = dict(shape, scale=a.scale, replicates=a.replicates, rounds=a.rounds, window_ms=a.window_ms,
               rule="new median <= reference median + (reference max - reference min)", cases={})
    for name in runs["reference"][0]:
        ref, new = ([r[name]["ms"] for r in runs[w]] for w in ("reference", "new"))
        rm, rr, nm = statistics.median(ref), max(ref) - min(ref), statistics.median(new)
        out["cases"][name] = {"reference_ms": ref, "new_ms": new, "reference_median_ms": rm, "reference_range_ms": rr,
                              "new_median_ms": nm, "new_over_reference": nm / rm, "passes": nm <= rm + rr,
                              "calls_per_window": runs["new"][0][name]["reps"]}
        print(f"{name:28s} ref {rm:9.4f} ms (range {rr:7.4f})  new {nm:9.4f} ms  {nm / rm:6.3f}  "
              f"{'ok' if nm <= rm + rr else 'OUTSIDE'}", flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
