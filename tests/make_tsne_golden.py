"""Writes tests/golden/tsne_kl.json: the final KL of mmgnn.embed.tsne's host path (float64 numpy, max_iter = 1000) over
five starts per case of tsne_ref.GOLDEN_CASES -- the PCA init, and the PCA init times 1 +- 1e-3 per coordinate under
seeds 1 .. 4.  The spread of the five is what a correct run may land in: test_tsne_gpu.py and test_tsne_cpu.py hold a
finished map against max + (max - min).

    python tests/make_tsne_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import mmgnn  # noqa: E402,F401
from mmgnn import embed  # noqa: E402
import tsne_ref as tr  # noqa: E402


def main():
    out = {}
    for n, D in tr.GOLDEN_CASES:
        x = tr.make_case(n, D)
        runs = [embed.tsne(x, perplexity=tr.default_perplexity(n), max_iter=1000, init=y0) for y0 in tr.golden_starts(x)]
        out[f"{n}x{D}"] = {"n": n, "D": D, "seed": 0, "perplexity": tr.default_perplexity(n),
                           "kl": [r.kl_divergence for r in runs], "n_iter": [r.n_iter for r in runs]}
        print(f"{n} x {D}: KL {out[f'{n}x{D}']['kl']}")
    path = os.path.join(HERE, "golden", "tsne_kl.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
