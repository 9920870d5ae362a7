"""One SHA-256 per output of the three fp64 slab-Gram users (csrc/gram64.h) on the GENERIC data of their GPU tests' shapes:
  centered_gram   mean and S at every embed_ref.GRAM_CASES shape (D up to 256)
  assoc_moments   the planes N, SX, SXX, SXY at test_association_gpu's (L, n)
  chain_moments   n_j, s and G at targets 0 and L - 1 at test_chained_gpu's (L, n)
Two builds whose listings are identical line for line add the same terms in the same order: the lattice tests cannot
tell a changed summation order (their sums are exact in any order) and the bound tests allow one.

  python profiles/probes/gram_outputs.py > <listing>
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import mmgnn  # noqa: E402,F401
from mmgnn import assoc_ops as ao  # noqa: E402
from mmgnn import chain_ops as co  # noqa: E402
from mmgnn import ops  # noqa: E402
from mmgnn.association import host_colstats  # noqa: E402
import assoc_ref  # noqa: E402
import chain_ref  # noqa: E402
import embed_ref  # noqa: E402

DEV = torch.device("cuda:0")


def dv(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def show(name, t):
    print(f"{name}  {hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()}", flush=True)


def row_counts(plan, chunk, L):
    rows, _ = plan(1, L)
    return [1, chunk - 1, chunk + 1, rows, rows + 1, 2 * rows + 77]


def main():
    for n, D, ld in embed_ref.GRAM_CASES:
        x = embed_ref.gram_case_x(n, D, ld)
        mean, gram = ops.centered_gram(dv(x.base)[:, :D])
        show(f"centered_gram n {n} D {D} ld {ld} mean", mean)
        show(f"centered_gram n {n} D {D} ld {ld} S", gram)
    for L in (1, 3, 16, 17, 50, 64, 65, 130):
        for n in row_counts(ao.assoc_plan, ao.AS_CHUNK, L):
            X = assoc_ref.make_matrix(n, L, seed=L * 1000 + n, density=0.6)
            mom = ao.assoc_moments(dv(X), dv(host_colstats(X)[1]))
            for k, plane in enumerate(("N", "SX", "SXX", "SXY")):
                show(f"assoc_moments L {L} n {n} {plane}", mom[k])
    for L in (1, 2, 3, 16, 17, 50, 64, 65, 128):
        for n in row_counts(co.chain_plan, co.CH_CHUNK, L):
            X = chain_ref.make_matrix(n, L, seed=L * 1000 + n, density=0.6)
            if L > 2:
                X[:, 1] = np.nan
            center = host_colstats(X)[1]
            fill = np.random.default_rng(L + n).standard_normal((n, L)) * 2.0 + center[None, :]
            W = np.where(np.isfinite(X), X.astype(np.float64), fill)
            Xd, Wd, cd = dv(X), dv(W), dv(center)
            for j in sorted({0, L - 1}):
                for name, t in zip(("n_j", "s", "G"), co.chain_moments(Wd, Xd, j, cd)):
                    show(f"chain_moments L {L} n {n} target {j} {name}", t)


if __name__ == "__main__":
    main()
