"""Helpers of the t-SNE tests (test_tsne_cpu.py, test_tsne_gpu.py, make_tsne_golden.py): the case generator, the margin
of the perplexity search's decisions, the rounding bounds of one objective evaluation, the plain host iteration and its
reversed-order twin.  The reference arithmetic itself is mmgnn.embed's host path (tsne_*_host): float64 numpy, the n x n
matrix rounded to fp32 at the same two places as the device."""
import numpy as np

from mmgnn import embed

EPS = embed.TSNE_EPS
U24 = 2.0 ** -24                     # the unit round-off of fp32
U53 = 2.0 ** -53                     # ... of fp64
MARGIN = 1e-10                       # no decision of the search may sit this close to its tolerance
# (n, D) the margin was checked at on the host: >= 2.7e-9, the searches take 8 .. 26 steps
MARGIN_CASES = ((5, 4), (63, 8), (65, 64), (200, 32), (513, 128), (1100, 128))


def make_case(n, D, seed=0):
    """5 centres N(0, 4), rows centre + N(0, 1), L2-normalised, fp32 [n, D]."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 2.0, (5, D))
    x = centres[rng.integers(0, 5, n)] + rng.normal(0.0, 1.0, (n, D))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


def default_perplexity(n):
    return float(min(30, n - 1))


def search_margin(dist, perplexity):
    """-> (the smallest | |H - log perplexity| - 1e-5 | over every row and every visited step of the host search on the
    fp32 distances, (conditional fp32, beta, steps) of that search)."""
    margins = []
    out = embed.tsne_search_host(dist, perplexity, margins)
    return float(min(m.min() for m in margins if m.size)), out


def objective_bounds(p, y, exaggeration, n):
    """One evaluation of the host objective and what a device evaluation may differ from it by: every component of the
    gradient, Z and KL are sums of n terms, each term a handful of correctly rounded fp64 operations; (n + 8) 2^-53
    times the sum of the absolute terms covers any summation order (n 2^-53, first order) and eight roundings per
    term.  -> (kl, grad, z, bound_kl, bound_grad [n, 2], bound_z)."""
    sums = {}
    kl, grad, z = embed.tsne_objective_host(p, y, exaggeration, True, sums)
    c = (n + 8) * U53
    return kl, grad, z, c * sums["kl"], c * sums["grad"], c * sums["z"]


def run_host(p, y0, iters, learning_rate, early_exaggeration=12.0, momentum=0.5):
    """`iters` iterations of the host path from y0 over P (the first stage's settings) -> Y."""
    y = np.array(y0, np.float64)
    u, g = np.zeros_like(y), np.ones_like(y)
    for _ in range(iters):
        _, grad, _ = embed.tsne_objective_host(p, y, early_exaggeration, False)
        embed.tsne_update_host(y, u, g, grad, momentum, learning_rate)
    return y


def run_host_reversed(p, y0, iters, learning_rate, early_exaggeration=12.0, momentum=0.5):
    """The same run with the points in reversed order (rows and columns of P and the rows of y0 permuted, the result
    unpermuted): the same arithmetic, every sum taken in another order."""
    p = np.ascontiguousarray(np.asarray(p)[::-1, ::-1])
    return run_host(p, np.asarray(y0)[::-1], iters, learning_rate, early_exaggeration, momentum)[::-1]


def extent(y):
    return float(np.ptp(np.asarray(y), axis=0).max())


def golden_starts(x):
    """The five starts of tests/golden/tsne_kl.json: the PCA init, and the PCA init times 1 +- 1e-3 per coordinate
    under seeds 1 .. 4."""
    proj = embed.pca(np.asarray(x), 2).projection
    y0 = proj / np.std(proj[:, 0]) * 1e-4
    starts = [y0]
    for seed in (1, 2, 3, 4):
        sign = np.random.default_rng(seed).choice([-1.0, 1.0], y0.shape)
        starts.append(y0 * (1.0 + 1e-3 * sign))
    return starts


GOLDEN_CASES = ((60, 16), (200, 32))         # (n, D) of test 7, generator seed 0, the default perplexity
