"""One reference for the degree-gated pair head (csrc/pairs.hip), and the case builder of the lab-count sweep.

  z1 = A[pi] + B[li]          h1 = relu(z1) * d1          d1 / d2: dropout's factor, inv_keep where kept else 0, masks
  z2 = h1 . W2^T + b2         h2 = relu(z2) * d2          restated by tests/rng_ref.py from the pair ids (64 / 32 per pair)
  pred = h2 . W3 + b3

head_ref(..., dtype=torch.float64) is the reference.  The same formula in dtype=torch.float32 (plain torch on the CPU, in
whatever order torch sums) is the RESTATEMENT: its error against fp64 sizes the bar of tests/test_pair_lab_edges_gpu.py.

With scales=True every output comes with the sum of the absolute values of the terms it was summed from -- the scale an
error of it is measured by (scaled_err: a matrix row by the largest of its element scales, since the 32 terms of ONE
element of dz1 may cancel).  A row whose scale is 0 received nothing and has to be exactly 0.

The ReLU of layer 2 makes the gradients discontinuous in z2: a kernel whose fp32 z2 lands on the other side of 0 than the
fp64 one is not wrong, yet differs by a whole term.  settle_b2() therefore moves b2 (per case, by a few 1e-4) until no
pair of the case has a z2 closer to 0 than 2^-16 of its scale |b2| + sum |W2 h1| -- four times the worst-case bound
64 * 2^-24 of a 64-deep fp32 FMA chain -- so reference, restatement and kernels take the same masks.  (z1 = A + B is one
fp32 addition: its sign is exact in every precision.)
"""
import types

import numpy as np
import torch

import rng_ref as R

SEED = 2 ** 40 + 99
TIE_TOL = 2.0 ** -16


def _layers(par, a, l, ids, p, seed):
    """The forward of the pairs (a, l) in the dtype of par -> (z1, d1, h1, z2, d2, h2)."""
    A, B, W2, b2, W3, b3 = par
    z1 = A[a] + B[l]
    d1 = d2 = 1.0
    if p > 0:
        ik = float(R.inv_keep(p))
        thr = np.uint32(R.threshold(p))
        e = ids.numpy().astype(np.uint64)
        k1 = R.fields_at(R.key(seed, R.SITE_H1), e[:, None] * np.uint64(64) + np.arange(64, dtype=np.uint64)) >= thr
        k2 = R.fields_at(R.key(seed, R.SITE_H2), e[:, None] * np.uint64(32) + np.arange(32, dtype=np.uint64)) >= thr
        d1, d2 = torch.from_numpy(k1).to(A.dtype) * ik, torch.from_numpy(k2).to(A.dtype) * ik
    h1 = z1.clamp(min=0) * d1
    z2 = h1 @ W2.t() + b2
    h2 = z2.clamp(min=0) * d2
    return z1, d1, h1, z2, d2, h2


def head_ref(params, pi, li, ids, p, dpred=None, chunk=65536, dtype=torch.float64, seed=SEED, scales=False):
    """The head in `dtype`, in chunks of 64k pairs: pred, and with dpred (zero where a pair is not visited) the six
    gradients (dA, dB, dW2, db2, dW3, db3).  ids: the pair ids the dropout streams are indexed by.
    scales=True: -> (pred, grads, S_pred, S_grads, margin) with
      S_pred[k] = |b3| + sum_u |W3[u] h2[k, u]|;
      S_grads: per element, the sum of the absolute values of the terms (dA / dB: index_add_ of |dz1|; dW2: |dz2|^T |h1|;
               db2: sum |dz2|; dW3: h2^T |dpred|; db3: sum |dpred|);
      margin:  min |z2| / (|b2| + |h1| . |W2|^T) over the units of the pairs with dpred != 0 (see settle_b2)."""
    A, B, W2, b2, W3, b3 = par = [t.to(dtype) for t in params]
    n = pi.numel()
    pred = torch.empty(n, dtype=dtype)
    grads = [torch.zeros_like(t) for t in par] if dpred is not None else None
    S_pred = torch.empty(n, dtype=dtype) if scales else None
    S = [torch.zeros_like(t) for t in par] if scales and dpred is not None else None
    margin = float("inf")
    for i in range(0, n, chunk):
        sl = slice(i, i + chunk)
        a, l = pi[sl], li[sl]
        z1, d1, h1, z2, d2, h2 = _layers(par, a, l, ids[sl], p, seed)
        pred[sl] = h2 @ W3 + b3
        if scales:
            S_pred[sl] = b3.abs() + h2.abs() @ W3.abs()
        if dpred is not None:
            gp = dpred[sl].to(dtype)
            grads[4] += h2.t() @ gp
            grads[5] += gp.sum()
            dz2 = gp[:, None] * W3[None, :] * d2 * (z2 > 0)
            grads[2] += dz2.t() @ h1
            grads[3] += dz2.sum(0)
            dz1 = (dz2 @ W2) * d1 * (z1 > 0)
            grads[0].index_add_(0, a, dz1)
            grads[1].index_add_(0, l, dz1)
            if scales:
                S[0].index_add_(0, a, dz1.abs())
                S[1].index_add_(0, l, dz1.abs())
                S[2] += dz2.abs().t() @ h1.abs()
                S[3] += dz2.abs().sum(0)
                S[4] += h2.abs().t() @ gp.abs()
                S[5] += gp.abs().sum()
                live = gp != 0
                if bool(live.any()):
                    rel = z2.abs() / (b2.abs() + h1.abs() @ W2.abs().t())
                    margin = min(margin, float(rel[live].min()))
    if scales:
        return pred, grads, S_pred, S, margin
    return pred, grads


def scaled_err(got, ref, S, what=""):
    """The scaled error of `got` against the fp64 `ref`: e = max |got - ref| / S per ROW -- of a matrix: its largest
    element error over its largest element scale (one element's terms may cancel, a row's do not all), of a vector: per
    element.  Nothing is excluded: a row with S = 0 received nothing and has to be exactly 0 (asserted).
    -> the worst e over the rows with S > 0 (0.0 if there is none)."""
    got, ref, S = got.detach().double().cpu().reshape(ref.shape), ref.double(), S.double()
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    err = (got - ref).abs()
    if ref.dim() == 2:
        err, S, nz = err.amax(1), S.amax(1), got.abs().amax(1)
    else:
        err, S, nz = err.reshape(-1), S.reshape(-1), got.abs().reshape(-1)
    dead = S == 0
    assert bool((nz[dead] == 0).all()), f"{what}: row {int((dead & (nz != 0)).nonzero()[0])} received nothing and is not 0"
    return float((err[~dead] / S[~dead]).max()) if bool((~dead).any()) else 0.0


def settle_b2(params, pi, li, ids, p, seed=SEED, tol=TIE_TOL):
    """params with b2 moved, unit by unit and by the smallest multiple of the clearance that does it, until every pair of
    the case keeps |z2| >= tol * (|b2| + sum |W2 h1|) in fp64 (asserted) -> the new params (fp32 tensors)."""
    A, B, W2, b2, W3, b3 = params
    par = [t.double() for t in params]
    _, _, h1, z2, _, _ = _layers(par, pi, li, ids, p, seed)
    scale = par[3].abs() + h1.abs() @ par[2].abs().t()
    clear = 2.0 * tol * float(scale.max()) + 1e-3 * tol          # (b2 itself enters the scale: leave room for its move)
    new = b2.clone()
    for u in range(32):
        for j in range(400):
            delta = ((j + 1) // 2) * (1 if j % 2 else -1) * 2.0 * clear
            if float((z2[:, u] + delta).abs().min()) >= clear:
                new[u] = float(b2[u]) + delta
                break
        else:
            raise AssertionError(f"unit {u}: no clear offset of b2")
    out = (A, B, W2, new, W3, b3)
    par = [t.double() for t in out]
    _, _, h1, z2, _, _ = _layers(par, pi, li, ids, p, seed)
    rel = z2.abs() / (par[3].abs() + h1.abs() @ par[2].abs().t())
    assert float(rel.min()) >= tol, float(rel.min())
    return out


# ------------------------------------------------------------------------------------------ the case builder
SWEEP = (1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 204, 205, 256, 257, 300)      # both sides of every lab-count switch
RUNS = (1, 2, 31, 32, 33, 75)          # patient run lengths every full case holds: one tile and its neighbours, three tiles
FULL = 512                             # from this many pairs on a case has every property below


def rare_rows(L):
    """The last row of every 32-lab tile present and row L - 1 -- without row 0, which is the hot row."""
    return sorted((set(range(31, L, 32)) | {L - 1}) - {0})


def pair_case(L, n, seed, P=300, thr=6):
    """A pair set over L labs and P patients -> namespace(pi sorted, li, deg, pair_id, dpred, thr, P, L, n, rare, runs).

    n >= FULL (asserted here, every property):
      - lab frequencies are skewed, not uniform: lab 0, the hot row, holds about 30 % of the pairs (all pairs that are
        not on a rare row where there is no third kind of lab: L <= 2); the labs in between follow 1 / rank;
      - every lab row < L is hit (n >= L);
      - the rare rows -- rare_rows(L) -- hold exactly two pairs each, one of a patient below the degree threshold and
        one of a patient at or above it, both with dpred != 0: ONE contribution per row and gate;
      - the patient runs include lengths 1, 2, 31, 32, 33 and 75, some patients have no pair;
      - degrees fall on both sides of the threshold; about 30 % of dpred is exactly 0.
    n < FULL (the tiny launches): random labs with lab 0 on the first and lab L - 1 on the last pair."""
    gen = torch.Generator().manual_seed(seed * 1000003 + L * 4099 + n)
    deg = torch.randint(0, 2 * thr, (P,), generator=gen)
    full = n >= FULL
    # patients and their runs
    order = torch.randperm(P, generator=gen)
    if full:
        n_with = (P * 17) // 20
        assert n - sum(RUNS) >= n_with - len(RUNS)
        rest = n_with - len(RUNS)
        extra = torch.bincount(torch.randint(0, rest, (n - sum(RUNS) - rest,), generator=gen), minlength=rest) + 1
        lens = torch.cat([torch.tensor(RUNS), extra])
    else:
        n_with = max(1, min(P, n // 8))
        lens = torch.bincount(torch.randint(0, n_with, (n - n_with,), generator=gen), minlength=n_with) + 1
    run = torch.zeros(P, dtype=torch.long)
    run[order[:n_with]] = lens
    pi = torch.repeat_interleave(torch.arange(P), run)
    assert pi.numel() == n
    low = deg[pi] < thr
    # labs
    rare = rare_rows(L) if full else []
    li = torch.full((n,), -1, dtype=torch.long)
    dpred = torch.randn(n, generator=gen) * (torch.rand(n, generator=gen) < 0.7)
    if full:
        lo_pos = low.nonzero().flatten()
        hi_pos = (~low).nonzero().flatten()
        lo_pos = lo_pos[torch.randperm(lo_pos.numel(), generator=gen)][:len(rare)]
        hi_pos = hi_pos[torch.randperm(hi_pos.numel(), generator=gen)][:len(rare)]
        assert lo_pos.numel() == len(rare) and hi_pos.numel() == len(rare)
        for r, a, b in zip(rare, lo_pos.tolist(), hi_pos.tolist()):
            li[a] = li[b] = r
            for q in (a, b):
                if dpred[q] == 0:
                    dpred[q] = 0.5 + float(torch.rand((), generator=gen))
        free = (li < 0).nonzero().flatten()
        free = free[torch.randperm(free.numel(), generator=gen)]
        common = torch.tensor(sorted(set(range(1, L)) - set(rare)), dtype=torch.long)
        assert free.numel() >= common.numel()
        li[free[:common.numel()]] = common[torch.randperm(common.numel(), generator=gen)]     # every row is hit
        free = free[common.numel():]
        if common.numel():
            n_hot = int(round(0.3 * n))
            hot = free[:n_hot]
            li[hot] = 0
            w = 1.0 / torch.arange(1, common.numel() + 1, dtype=torch.float64)                # Zipf-like: 1 / rank
            ranks = common[torch.randperm(common.numel(), generator=gen)]
            draw = torch.multinomial(w, free.numel() - hot.numel(), replacement=True, generator=gen)
            li[free[n_hot:]] = ranks[draw]
        else:
            li[free] = 0
    else:
        li = torch.randint(0, L, (n,), generator=gen)
        li[0], li[-1] = 0, L - 1
    pair_id = torch.randperm(n, generator=gen) + 12345
    c = types.SimpleNamespace(pi=pi, li=li, deg=deg, pair_id=pair_id, dpred=dpred, thr=thr, P=P, L=L, n=n, rare=rare,
                              runs=run)
    check_case(c)
    return c


def check_case(c):
    """The properties pair_case promises, asserted."""
    L, n, pi, li = c.L, c.n, c.pi, c.li
    assert pi.numel() == li.numel() == c.dpred.numel() == c.pair_id.numel() == n
    assert bool((pi[1:] >= pi[:-1]).all()) and 0 <= int(pi.min()) and int(pi.max()) < c.P
    assert 0 <= int(li.min()) and int(li.max()) < L
    assert c.pair_id.unique().numel() == n
    if n < FULL:
        assert int(li[-1]) == L - 1 and (n == 1 or int(li[0]) == 0)
        return
    low = c.deg[pi] < c.thr
    assert 0.2 <= float((c.deg < c.thr).float().mean()) <= 0.8 and 0.2 <= float(low.float().mean()) <= 0.8
    count = torch.bincount(li, minlength=L)
    assert n < L or int(count.min()) >= 1                                      # every row that can be hit is hit
    assert c.rare == rare_rows(L)
    for r in c.rare:
        at = (li == r).nonzero().flatten()
        assert at.numel() == 2 and bool((c.dpred[at] != 0).all()), r
        assert int(low[at].sum()) == 1, r                                      # one per gate
    if L - len(c.rare) > 1:
        assert 0.27 <= int(count[0]) / n <= 0.36, int(count[0]) / n            # the hot row
        assert L < 31 or int(count[0]) == int(count.max())
    else:
        assert int(count[0]) == n - 2 * len(c.rare)
    lens = set(c.runs.tolist())
    assert set(RUNS) <= lens and 0 in lens and max(lens) >= 70
    zero = float((c.dpred == 0).float().mean())
    assert 0.25 <= zero <= 0.35, zero
