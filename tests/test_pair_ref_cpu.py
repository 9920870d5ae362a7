"""tests/pair_ref.py against torch.autograd, and the properties of its case builder -- no GPU needed.

The fp64 gradients of head_ref are hand-written; here the same forward formula is differentiated by autograd (masks from
tests/rng_ref.py, applied as constants) and the two agree to 1e-12 of each tensor's largest element.  The scales are
checked for what they promise: zero exactly where nothing arrived, never below the value they scale."""
import pytest
import torch

import pair_ref as PR
import rng_ref as R

SWEEP = PR.SWEEP                 # the lab counts of tests/test_pair_lab_edges_gpu.py


def params(L, P, seed=7):
    g = torch.Generator().manual_seed(seed + L)
    r = lambda *s: torch.randn(*s, generator=g)
    return r(P, 64), r(L, 64), r(32, 64) / 8, r(32) * 0.1, r(32) / 5, r(1)


def masks(ids, p, seed):
    if p == 0:
        return 1.0, 1.0
    e = ids.numpy().astype("uint64")
    ik = float(R.inv_keep(p))
    k1 = R.keep_at(seed, R.SITE_H1, e[:, None] * 64 + torch.arange(64).numpy().astype("uint64"), p)
    k2 = R.keep_at(seed, R.SITE_H2, e[:, None] * 32 + torch.arange(32).numpy().astype("uint64"), p)
    return torch.from_numpy(k1).double() * ik, torch.from_numpy(k2).double() * ik


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("L", [2, 50, 129])
def test_fp64_gradients_equal_autograd(L, p):
    c = PR.pair_case(L, 700, seed=3, P=120)
    par = PR.settle_b2(params(L, c.P), c.pi, c.li, c.pair_id, p)
    visited = c.deg[c.pi] >= c.thr
    dpred = (c.dpred * visited).double()
    pred, grads, S_pred, S, margin = PR.head_ref(par, c.pi, c.li, c.pair_id, p, dpred, scales=True)
    assert margin >= PR.TIE_TOL
    leaves = [t.double().requires_grad_() for t in par]
    A, B, W2, b2, W3, b3 = leaves
    d1, d2 = masks(c.pair_id, p, PR.SEED)
    h1 = torch.relu(A[c.pi] + B[c.li]) * d1
    h2 = torch.relu(h1 @ W2.t() + b2) * d2
    out = h2 @ W3 + b3
    assert float((out.detach() - pred).abs().max()) <= 1e-12 * float(pred.abs().max())
    out.backward(dpred)
    for name, t, g, s in zip("A B W2 b2 W3 b3".split(), leaves, grads, S):
        assert float((t.grad - g).abs().max()) <= 1e-12 * float(g.abs().max()), name
        assert bool((s >= g.abs() * (1 - 1e-12)).all()), name                 # a sum of absolute terms bounds the sum
        assert bool((g[s == 0] == 0).all()), name
    assert bool((S_pred >= pred.abs() * (1 - 1e-12)).all())
    # a row of dA / dB has scale 0 exactly when no visited pair with dpred != 0 names it
    live = dpred != 0
    for s, idx, rows in ((S[0], c.pi, c.P), (S[1], c.li, L)):
        hit = torch.zeros(rows, dtype=torch.bool)
        hit[idx[live]] = True
        assert bool(((s.amax(1) > 0) <= hit).all())
        assert bool((s[~hit] == 0).all())


def test_fp32_restatement_is_the_same_formula():
    """dtype=torch.float32 differs from fp64 by rounding only: a few 1e-7 of the row scales (PR.scaled_err)."""
    L, p = 50, 0.2
    c = PR.pair_case(L, 700, seed=4, P=120)
    par = PR.settle_b2(params(L, c.P), c.pi, c.li, c.pair_id, p)
    dpred = c.dpred * (c.deg[c.pi] < c.thr)
    pred, grads, S_pred, S, _ = PR.head_ref(par, c.pi, c.li, c.pair_id, p, dpred, scales=True)
    pred32, grads32 = PR.head_ref(par, c.pi, c.li, c.pair_id, p, dpred, dtype=torch.float32)
    assert pred32.dtype == torch.float32 and all(g.dtype == torch.float32 for g in grads32)
    assert PR.scaled_err(pred32, pred, S_pred) <= 1e-5
    for name, g32, g, s in zip("A B W2 b2 W3 b3".split(), grads32, grads, S):
        e = PR.scaled_err(g32, g, s, name)
        assert 0 < e <= 1e-5, (name, e)
    # a lost contribution to a rare row is an error of the order of that row's scale
    lost = grads32[1].clone()
    lost[L - 1] = 0
    assert PR.scaled_err(lost, grads[1], S[1]) >= 0.05


@pytest.mark.parametrize("L", SWEEP)
def test_builder_properties_hold_at_every_lab_count_of_the_sweep(L):
    c = PR.pair_case(L, 2531, seed=L)                   # (asserts its own properties: check_case)
    assert c.n == 2531 and c.P == 300 and c.L == L
    assert c.rare == sorted((set(range(31, L, 32)) | {L - 1}) - {0})
    count = torch.bincount(c.li, minlength=L)
    assert int(count.min()) >= 1
    for r in c.rare:
        assert int(count[r]) == 2
    first = torch.full((c.P,), c.n, dtype=torch.long).scatter_reduce(0, c.pi, torch.arange(c.n), "amin")
    last = torch.full((c.P,), -1, dtype=torch.long).scatter_reduce(0, c.pi, torch.arange(c.n), "amax")
    assert int((last // 32 - first // 32).max()) >= 2                           # a run over three tiles of 32 pairs
    d = PR.pair_case(L, 2531, seed=L)
    assert torch.equal(c.li, d.li) and torch.equal(c.pi, d.pi) and torch.equal(c.dpred, d.dpred)      # deterministic


@pytest.mark.parametrize("n", [1, 31, 32, 33])
@pytest.mark.parametrize("L", [50, 100, 205])
def test_builder_tiny_cases(L, n):
    c = PR.pair_case(L, n, seed=n)
    assert c.pi.numel() == n and int(c.li[-1]) == L - 1
