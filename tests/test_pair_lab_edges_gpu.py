"""The pair heads (csrc/pairs.hip) at every lab count where the host picks another kernel or moves a table.

  64 | 65     backward k_pair_bwd_duo6<2, ...> -> k_pair_bwd_duo<4, ...>; slab of 2 -> 4 lab tiles; saved state used -> ignored
  128 | 129   matrix-core backward -> fp32 k_pair_bwd; the workspace drops to 256 B
  204 | 205   k_pair_bwd keeps dB in LDS -> adds dB with global atomics (lds_db)
  256 | 257   forward and dense forward: lab table in LDS -> read through the buffer descriptor
  k * 32      one lab tile of the one-hot dB product; EpiPairFlush's guard behind the last row of the table

Shapes: n = 2,531 pairs over 300 patients (80 tiles of 32, the last one with 3 pairs; 10 tiles of 256 for k_pair_bwd) from
pair_ref.pair_case: Zipf-like lab frequencies with a hot row 0 (30 % of the pairs) and RARE rows -- the last row of every
lab tile and row L - 1 -- that receive exactly one contribution per gate.  The many-tile regime is
tests/test_steady_state_gpu.py's.

The bar.  Scaled error of a row or pair: e = max |got - ref64| / S with S the sum of the absolute terms (pair_ref.head_ref,
pair_ref.scaled_err: a matrix row is judged by its largest element scale).  Nothing is excluded; a row with S = 0 has to
be exactly 0.  Per tensor and case the bar is 8 x max(worst e of the fp32 restatement on the same inputs, 2^-24),
computed here, never taken from a kernel: the restatement rounds the same FMA chains (64-deep, 32-deep, the row sums), the
kernels add at most 3 * 2^-25 |x||w| per product for the dropped split terms (csrc/mma.h) and sum slabs and atomics in
another order -- three octaves cover the order.  A lost or misplaced contribution to a rare row is an error of 1.0 of that
row's scale.  The global max-norm bars of the older tests (1e-5 predictions, 2e-5 gradients) are asserted beside it.

The probe names the kernel instance of every launch; it cannot see lds_db.  204 | 205 restated: k_pair_bwd's fixed LDS is
OFF_DB = 2048 (W2) + 32 (b2) + 32 (W3) + 64 * 260 (T1t) + 32 * 260 (T2t) + 256 (pi) + 256 (li) + 4 * 68 (RED) = 27,856
floats = 111,424 B; dB needs 256 B per lab; 111,424 + 256 L <= 163,840 (160 KB) <=> L <= 204.75.  204 labs ask for
163,648 B, 192 B under the ceiling; 205 labs would need 163,904 B and take the global-atomics path.

saved= beyond 64 labs ("recomputed"): the state is not read.  Where the summation order of a tensor is fixed (the slab sums
of k_pair_bwd_duo<4>: dB, dW2, db2, dW3, db3; everywhere: a row with at most two addends) passing it changes no bit; where
fp32 atomics arrive in free order (dA rows over three tiles; every tensor of k_pair_bwd) two launches of the SAME arguments
do not agree to the bit -- measured at 129 labs: 97 .. 245 elements of dB, 457 .. 870 of dW2, 6 .. 22 of db2, 5 .. 15 of dW3
differ between two launches, with the state, with a poisoned state or without alike; at 65 / 128 labs 0 .. 18 elements of
dA -- so those are held to 1e-6 of each other and to the bar, and the launch is repeated with poisoned state (NaN
activations, all sign bits set), which must not show.

Measured worst scaled errors, kernel (restatement), MI355X, over all cases of this file; no case came closer to its own
bar than a factor 3.0 (k_pair_bwd, dW3 of a tiny launch: 2.2e-6 under a bar of 6.8e-6; predictions: 3.5).  No defect found.
                            pred              dA                dB                dW2               db2               dW3               db3
  k_pair_fwd_mfma<true, *>  2.7e-7 (3.1e-7)
  k_pair_fwd_mfma<false, *> 2.4e-7 (1.9e-7)
  k_pair_dense_fwd<true>    2.7e-7 (2.2e-7)
  k_pair_dense_fwd<false>   1.3e-7 (1.3e-7)
  k_pair_bwd_duo6<2, .., *>                   2.6e-7 (2.7e-7)   2.9e-7 (2.7e-7)   1.5e-7 (1.4e-7)   8.6e-8 (1.0e-7)   2.5e-6 (2.9e-6)   2.4e-8 (8.5e-8)
  k_pair_bwd_duo<4, true>                     1.9e-7 (2.2e-7)   2.3e-7 (2.1e-7)   2.0e-7 (2.0e-7)   8.7e-8 (9.9e-8)   1.5e-6 (5.8e-6)   1.9e-8 (6.2e-8)
  k_pair_bwd                                  2.5e-7 (2.5e-7)   3.5e-7 (3.5e-7)   1.7e-7 (1.7e-7)   1.2e-7 (1.2e-7)   2.9e-5 (9.6e-5)   2.2e-8 (2.2e-8)
  ... into the prefilled flat buffer (scale S + |prefill|): at most 2.1e-7 (2.1e-7), every kernel and tensor
(saved and recomputing duo6 give the same figures: the same bits but for dA's atomics.  The worst cases are the tiny
launches, where k_pair_bwd's sequential FMA chains and the restatement's round alike.  dW3's scale sum |dpred| h2 is small
for a unit whose z2 is negative on most pairs, while its error follows the scale of z2: kernel and restatement show it
alike, and the bar moves with the restatement.)  The whole file takes 4.2 s, its slowest case 0.3 s.
"""
import functools
import types

import pytest
import torch

import pair_ref as PR
from test_steady_state_gpu import launch_of, probed, rel, tf

pytestmark = pytest.mark.gpu

SEED = PR.SEED
N, P, THR = 2531, 300, 6
SWEEP = PR.SWEEP
CANARY = 123.0
EPS = 2.0 ** -24
NAMES = "dA dB dW2 db2 dW3 db3".split()
WORST = {}                       # (kernel instance, tensor) -> [worst e of the kernel, worst e of the restatement]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    import mmgnn  # noqa: F401
    from mmgnn import ops as o
    return o


def note(instance, tensor, e, e32):
    w = WORST.setdefault((instance, tensor), [0.0, 0.0])
    w[0], w[1] = max(w[0], e), max(w[1], e32)
    print(f"[lab edges] {instance} {tensor}: kernel e = {e:.3e}, restatement e = {e32:.3e}, bar {8 * max(e32, EPS):.3e}")


def bwd_instance(L, saved=False):
    """What the host launches for L labs with pair ids given (AUX)."""
    if L <= 64:
        return f"k_pair_bwd_duo6<2, true, {tf(saved)}>"
    return "k_pair_bwd_duo<4, true>" if L <= 128 else "k_pair_bwd"


def ran(recs, want, n):
    sym, M, grid, block = launch_of(recs, want.split("<")[0])
    assert (sym == want if "<" not in want else want in sym) and M == n, (sym, want, M, n)
    return sym


# ------------------------------------------------------------------------------------------ host side: cases, references
def head_params(L, P_=P, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + L)
    r = lambda *s: torch.randn(*s, generator=g)
    return r(P_, 64), r(L, 64), r(32, 64) / 8, r(32) * 0.1, r(32) / 5, r(1)


def gate_ref(par, c, p, want_low):
    """fp64 reference and fp32 restatement of one gate -> namespace(visited, pred, S_pred, grads, S, e32_pred, e32)."""
    visited = (c.deg[c.pi] < c.thr) == want_low
    dp = c.dpred * visited
    pred, grads, S_pred, S, margin = PR.head_ref(par, c.pi, c.li, c.pair_id, p, dp, seed=SEED, scales=True)
    assert margin >= PR.TIE_TOL
    pred32, grads32 = PR.head_ref(par, c.pi, c.li, c.pair_id, p, dp, dtype=torch.float32, seed=SEED)
    e32_pred = PR.scaled_err(pred32[visited], pred[visited], S_pred[visited]) if bool(visited.any()) else 0.0
    e32 = [PR.scaled_err(a, b, s, nm) for nm, a, b, s in zip(NAMES, grads32, grads, S)]
    return types.SimpleNamespace(visited=visited, dp=dp, pred=pred, S_pred=S_pred, grads=grads, S=S, e32_pred=e32_pred,
                                 e32=e32, grads32=grads32)


@functools.lru_cache(maxsize=None)
def case_data(L, n, p, one_lab=False, seed=0):
    """The pair case, the settled head parameters and both gates' references, once per (labs, pairs, p)."""
    c = PR.pair_case(L, n, seed=L)                                   # (seed: another head's parameters, the same pairs)
    if one_lab:
        c.li = torch.full_like(c.li, L - 1)
    par = PR.settle_b2(head_params(L, seed=seed), c.pi, c.li, c.pair_id, p, seed=SEED)
    return types.SimpleNamespace(case=c, par=par, gate={wl: gate_ref(par, c, p, wl) for wl in (False, True)})


def padded(t, extra, fill, dev):
    """t as the leading rows of a tensor with `extra` more rows of `fill` -> (the view, the whole tensor)."""
    whole = torch.full((t.shape[0] + extra,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
    whole[:t.shape[0]] = t
    whole = whole.to(dev)
    return whole[:t.shape[0]], whole


def dev_head(ops, dev, par):
    """A and B with 3 / 5 rows of NaN behind them: a read past a table shows."""
    A, B, W2, b2, W3, b3 = par
    return ops.Head(padded(A, 3, float("nan"), dev)[0], padded(B, 5, float("nan"), dev)[0], *[t.to(dev) for t in (W2, b2, W3, b3)])


def grad_bufs(ops, dev, L, tail_b=5):
    """Zero gradients; dA / dB are the leading rows of tensors with a canary tail -> (ops.Head, dA whole, dB whole)."""
    a, aw = padded(torch.zeros(P, 64), 3, CANARY, dev)
    b, bw = padded(torch.zeros(L, 64), tail_b, CANARY, dev)
    z = lambda *s: torch.zeros(*s, device=dev)
    return ops.Head(a, b, z(32, 64), z(32), z(32), z(1)), aw, bw


def dev_case(c, dev):
    i32 = lambda t: t.to(torch.int32).to(dev)
    return i32(c.pi), i32(c.li), i32(c.deg), c.pair_id.to(dev)


def tails_kept(aw, bw, L):
    assert bool((aw[P:] == CANARY).all()), "dA: rows behind the table were written"
    assert bool((bw[L:] == CANARY).all()), "dB: rows behind the table were written"


def check_grads(g, r, instance):
    for nm, got, ref, S, e32 in zip(NAMES, (g.A, g.B, g.W2, g.b2, g.W3, g.b3), r.grads, r.S, r.e32):
        e = PR.scaled_err(got, ref, S, f"{instance} {nm}")
        note(instance, nm, e, e32)
        assert e <= 8 * max(e32, EPS), (instance, nm, e, e32)
        assert rel(got, ref.reshape(got.shape)) <= 2e-5, (instance, nm)


def forward(ops, dev, d, L, p, want_low, save):
    """One forward launch into pred with a tail -> (pred view on the host side checks, saved buffers)."""
    c, r = d.case, d.gate[want_low]
    n = c.n
    pi, li, deg, pid = dev_case(c, dev)
    head = dev_head(ops, dev, d.par)
    whole = torch.full((n + 7,), CANARY, device=dev)
    sv = ops.pair_saved_alloc(n, dev) if save else None
    _, recs = probed(ops, lambda: ops.pair_head_fwd(head, pi, li, deg, THR, want_low, p, SEED, pid, whole[:n], save=sv))
    sym = ran(recs, f"k_pair_fwd_mfma<{tf(L <= 256)}, {tf(save)}>", n)
    pred = whole[:n].cpu()
    assert bool((whole[n:] == CANARY).all()), "pred: slots behind the pairs were written"
    assert bool((pred[~r.visited] == CANARY).all()), "pred: an unvisited pair was written"
    if bool(r.visited.any()):
        e = PR.scaled_err(pred[r.visited], r.pred[r.visited], r.S_pred[r.visited], sym)
        note(sym, "pred", e, r.e32_pred)
        assert e <= 8 * max(r.e32_pred, EPS), (sym, e, r.e32_pred)
        assert rel(pred[r.visited], r.pred[r.visited]) <= 1e-5
    return whole[:n], sv


def backward(ops, dev, d, L, p, want_low, saved=None, tail_b=5):
    c = d.case
    pi, li, deg, pid = dev_case(c, dev)
    head = dev_head(ops, dev, d.par)
    g, aw, bw = grad_bufs(ops, dev, L, tail_b)
    _, recs = probed(ops, lambda: ops.pair_head_bwd(head, g, pi, li, deg, THR, want_low, L, p, SEED, pid, c.dpred.to(dev),
                                                    saved=saved))
    sym = ran(recs, bwd_instance(L, saved is not None), c.n)
    tails_kept(aw, bw, L)
    return g, sym


# ------------------------------------------------------------------------------------------ the lab sweep
GATES = pytest.mark.parametrize("want_low", [False, True], ids=["high", "low"])


@GATES
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("L", SWEEP)
def test_forward_at_lab_count(ops, dev, L, p, want_low):
    """k_pair_fwd_mfma<L <= 256, save>, plain and saving: every visited prediction per pair against fp64, unvisited slots
    and the tail untouched, saving changes no bit."""
    d = case_data(L, N, p)
    plain, _ = forward(ops, dev, d, L, p, want_low, False)
    saving, _ = forward(ops, dev, d, L, p, want_low, True)
    assert torch.equal(plain, saving)


@GATES
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("L", SWEEP)
def test_backward_at_lab_count(ops, dev, L, p, want_low):
    """duo6<2> up to 64 labs, duo<4> up to 128, k_pair_bwd beyond (dB in LDS up to 204, global atomics from 205): the six
    gradients per row against fp64, rows that received nothing bitwise zero, the tails behind dA / dB untouched."""
    d = case_data(L, N, p)
    g, sym = backward(ops, dev, d, L, p, want_low)
    check_grads(g, d.gate[want_low], sym)


def tile_span(c, T):
    """Per patient: over how many T-pair tiles of the launch its run lies, minus one."""
    first = torch.full((P,), c.n, dtype=torch.long).scatter_reduce(0, c.pi, torch.arange(c.n), "amin")
    last = torch.full((P,), -1, dtype=torch.long).scatter_reduce(0, c.pi, torch.arange(c.n), "amax")
    return last // T - first // T


@GATES
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("L", [1, 2, 31, 32, 33, 63, 64])
def test_backward_from_saved_state_up_to_64_labs(ops, dev, L, p, want_low):
    """saved= from the forward: k_pair_bwd_duo6<2, true, true>; the bits of the recomputing kernel in dB, dW2, db2, dW3, db3
    (fixed-order slab sums).  dA as tests/test_steady_state_gpu.py states it: the same run sums per tile, added by atomics
    -- bitwise where a patient's pairs lie in at most two tiles, else to the rounding of two fp32 additions."""
    d = case_data(L, N, p)
    _, sv = forward(ops, dev, d, L, p, want_low, True)
    g0, _ = backward(ops, dev, d, L, p, want_low)
    g1, sym = backward(ops, dev, d, L, p, want_low, saved=sv)
    check_grads(g1, d.gate[want_low], sym)
    for nm in "B W2 b2 W3 b3".split():
        assert torch.equal(getattr(g0, nm), getattr(g1, nm)), nm
    two = (tile_span(d.case, 32) <= 1).to(dev)
    assert int(two.sum()) > 50 and int((~two).sum()) >= 1
    assert torch.equal(g0.A[two], g1.A[two])
    assert rel(g0.A, g1.A) <= 1e-6


@GATES
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("L", [65, 128, 129])
def test_saved_state_is_ignored_beyond_64_labs(ops, dev, L, p, want_low):
    """"beyond: recomputed".  The same instance runs with saved=, the forward's state and a poisoned one alike; no bit
    changes where the order of the sums is fixed (module docstring), the rest agrees to 1e-6 and meets the bar."""
    d = case_data(L, N, p)
    c, r = d.case, d.gate[want_low]
    _, sv = forward(ops, dev, d, L, p, want_low, True)
    poison = (torch.full_like(sv[0], -1), torch.full_like(sv[1], float("nan")))
    g0, sym = backward(ops, dev, d, L, p, want_low)
    fixed = "B W2 b2 W3 b3".split() if L <= 128 else []
    two = (tile_span(c, 32 if L <= 128 else 64) <= 1).to(dev)       # k_pair_bwd: a wave pre-sums runs over its 64 pairs
    single = torch.zeros(L, dtype=torch.bool)
    single[c.rare] = True                                           # one addend per gate (a zero dpred adds +0)
    assert int(two.sum()) > 50
    for what, state in (("forward's", sv), ("poisoned", poison)):
        g1, sym1 = backward(ops, dev, d, L, p, want_low, saved=state)
        assert sym1 == sym == bwd_instance(L)
        check_grads(g1, r, sym1)
        for nm in fixed:
            assert torch.equal(getattr(g0, nm), getattr(g1, nm)), (what, nm)
        assert torch.equal(g0.A[two], g1.A[two]), what
        assert torch.equal(g0.B[single.to(dev)], g1.B[single.to(dev)]), what
        diff = {nm: int((getattr(g0, nm) != getattr(g1, nm)).sum()) for nm in "A B W2 b2 W3 b3".split()}
        print(f"[lab edges] {sym}, {what} saved state: elements that differ from the launch without: {diff}")
        for nm in "A B W2 b2 W3 b3".split():
            assert rel(getattr(g1, nm), getattr(g0, nm)) <= 1e-6, (what, nm)


@GATES
def test_lab_id_inside_the_lab_tile_outside_the_table_L50(ops, dev, want_low):
    """50 labs, lab id 60 on a few pairs: inside the second lab tile (rows 32 .. 63 of the slab), outside the table.
    EpiPairFlush's row guard has something to protect: dB is the leading 50 rows of a 64-row tensor, so a flushed row 60
    would land in the canary.  Every other gradient stays finite."""
    L, p = 50, 0.2
    d = case_data(L, N, p)
    c = types.SimpleNamespace(**vars(d.case))
    c.li = c.li.clone()
    at = torch.arange(40, c.n, 211)
    c.li[at] = 60
    r = d.gate[want_low]
    assert bool((r.dp[at] != 0).any())                               # pairs of this gate with a gradient name lab 60
    g, sym = backward(ops, dev, types.SimpleNamespace(case=c, par=d.par), L, p, want_low, tail_b=14)
    for nm in "A B W2 b2 W3 b3".split():
        assert bool(torch.isfinite(getattr(g, nm)).all()), nm
    # the pairs that name a lab of the table are untouched by the others in dB: rows of labs no such pair of this gate names
    keep = torch.ones(c.n, dtype=torch.bool)
    keep[at] = False
    sub = (d.par, c.pi[keep], c.li[keep], c.pair_id[keep], p, r.dp[keep])
    _, grads, _, S, _ = PR.head_ref(*sub, seed=SEED, scales=True)
    _, grads32 = PR.head_ref(*sub, seed=SEED, dtype=torch.float32)
    e, e32 = PR.scaled_err(g.B, grads[1], S[1], "dB"), PR.scaled_err(grads32[1], grads[1], S[1])
    note(sym + " lab 60", "dB", e, e32)
    assert e <= 8 * max(e32, EPS), (e, e32)


# ------------------------------------------------------------------------------------------ tiny launches
@GATES
@pytest.mark.parametrize("n", [1, 31, 32, 33])
@pytest.mark.parametrize("L", [50, 100, 205])
def test_tiny_launch(ops, dev, L, n, want_low):
    """One pair, one tile minus one, one tile, one tile plus one -- through duo6<2>, duo<4> and k_pair_bwd without dB in
    LDS; the assertions of the sweep (p = 0.2)."""
    p = 0.2
    d = case_data(L, n, p)
    plain, _ = forward(ops, dev, d, L, p, want_low, False)
    saving, sv = forward(ops, dev, d, L, p, want_low, True)
    assert torch.equal(plain, saving)
    g, sym = backward(ops, dev, d, L, p, want_low)
    check_grads(g, d.gate[want_low], sym)
    if L <= 64:
        g1, sym1 = backward(ops, dev, d, L, p, want_low, saved=sv)
        check_grads(g1, d.gate[want_low], sym1)
        for nm in "A B W2 b2 W3 b3".split():                         # (n <= 33: no run over three tiles)
            assert torch.equal(getattr(g, nm), getattr(g1, nm)), nm


# ------------------------------------------------------------------------------------------ one lab holds every pair
@GATES
@pytest.mark.parametrize("L", [64, 128, 129, 205])
def test_one_lab_holds_every_pair(ops, dev, L, want_low):
    """li == L - 1 on 4,096 pairs: the last row of the last lab tile (64, 128), the first row past a switch (129, 205)
    takes every contribution; every other row of dB is bitwise zero (scaled_err: S = 0)."""
    p = 0.2
    d = case_data(L, 4096, p, one_lab=True)
    r = d.gate[want_low]
    assert bool((r.S[1][:L - 1] == 0).all()) and float(r.S[1][L - 1].max()) > 0
    g, sym = backward(ops, dev, d, L, p, want_low)
    check_grads(g, r, sym + " one lab")
    assert bool((g.B[:L - 1] == 0).all())


# ------------------------------------------------------------------------------------------ production layout and +=
@pytest.mark.parametrize("L", [50, 64, 65, 200, 205])
def test_production_layout_accumulates_L(ops, dev, L):
    """The flat gradient buffer of model.heads_bwd: dB of both heads first, then W2, b2, W3, b3 of head one and of head
    two, padding to 64 floats, then the two dA tables -- prefilled with random values.  mmg_head_grad_t says +=: each view
    ends as prefill + gradient (scale: S + |prefill|, restatement: the fp32 sum of prefill and the fp32 gradient), rows
    that received nothing keep the prefill's bits, the padding is untouched.  The second head's dW2 starts 2 * 64 L + 2113
    floats in: 4 B off 16-byte alignment under EpiPairFlush's f32x4 read-modify-write."""
    p = 0.2
    heads = [(case_data(L, N, p, seed=0), False), (case_data(L, N, p, seed=1), True)]      # gate high, then low
    shapes = [(L, 64), (32, 64), (32,), (32,), (1,)]
    numel = [a * (b[0] if b else 1) for a, *b in shapes]
    n_b = 2 * numel[0]
    n_small = 2 * sum(numel)
    n_small_pad = (n_small + 63) & ~63
    assert n_small_pad > n_small                                     # there IS padding: 2 * 2113 floats are no multiple of 64
    pre = torch.randn(n_small_pad + 2 * P * 64, generator=torch.Generator().manual_seed(L)) * 0.1
    flat = pre.to(dev)
    views, pviews, ob, o, oa = [], [], 0, n_b, n_small_pad
    for _ in heads:
        spans = [(ob, numel[0])]
        ob += numel[0]
        for k in numel[1:]:
            spans.append((o, k))
            o += k
        spans.insert(0, (oa, P * 64))
        oa += P * 64
        shp = [(P, 64)] + shapes
        views.append([flat[s:s + k].view(sh) for (s, k), sh in zip(spans, shp)])
        pviews.append([pre[s:s + k].view(sh) for (s, k), sh in zip(spans, shp)])
    assert o == n_small and oa == flat.numel()
    assert views[1][2].data_ptr() % 16 == 4                          # the second head's dW2
    for (d, want_low), v in zip(heads, views):
        c = d.case
        pi, li, deg, pid = dev_case(c, dev)
        head = dev_head(ops, dev, d.par)
        _, recs = probed(ops, lambda: ops.pair_head_bwd(head, ops.Head(*v), pi, li, deg, THR, want_low, L, p, SEED, pid,
                                                        c.dpred.to(dev)))
        ran(recs, bwd_instance(L), c.n)
    assert torch.equal(flat[n_small:n_small_pad].cpu(), pre[n_small:n_small_pad]), "the padding was written"
    for (d, want_low), v, pv in zip(heads, views, pviews):
        r = d.gate[want_low]
        sym = bwd_instance(L) + " +="
        for nm, got, pr, ref, S, g32 in zip(NAMES, v, pv, r.grads, r.S, r.grads32):
            got = got.cpu()
            want = pr.double() + ref.reshape(pr.shape)
            scale = S.reshape(pr.shape) + pr.double().abs()
            dead = (S.reshape(pr.shape) == 0)
            dead = dead.all(1) if dead.dim() == 2 else dead
            assert torch.equal(got[dead], pr[dead]), f"{nm}: a row that received nothing lost the prefill's bits"
            e = PR.scaled_err(got, want, scale, nm)
            e32 = PR.scaled_err(pr + g32.reshape(pr.shape), want, scale, nm)
            note(sym, nm, e, e32)
            assert e <= 8 * max(e32, EPS), (L, want_low, nm, e, e32)


# ------------------------------------------------------------------------------------------ dense forward
@pytest.mark.parametrize("L", [1, 2, 3, 31, 32, 33, 64, 256, 257])
def test_dense_forward_at_lab_count(ops, dev, L):
    """mmg_pair_head_dense_fwd over 67 rows (with repeats) into a permutation of 72 output rows, ld = L + 3: a 32-cell tile
    spans up to 33 patient rows at L = 1 and the k / n_labs row split is at its extremes.  Bitwise pair_head_fwd's
    predictions for the same pairs at p = 0 (the contract), per pair against fp64, unlisted rows and the padding columns
    untouched."""
    n_rows, n_out = 67, 72
    gen = torch.Generator().manual_seed(900 + L)
    par = head_params(L, seed=2)
    rows = torch.randint(0, P, (n_rows,), generator=gen)
    rows[5], rows[66] = rows[4], rows[0]                             # repeats, adjacent and far apart
    out_rows = torch.randperm(n_out, generator=gen)[:n_rows]
    head = dev_head(ops, dev, par)
    out = torch.full((n_out, L + 3), CANARY, device=dev)
    i32 = lambda t: t.to(torch.int32).to(dev)
    _, recs = probed(ops, lambda: ops.pair_head_dense_fwd(head, i32(rows), i32(out_rows), out))
    sym = ran(recs, f"k_pair_dense_fwd<{tf(L <= 256)}>", n_rows * L)
    pi, li = rows.repeat_interleave(L), torch.arange(L).repeat(n_rows)
    pred = torch.empty(n_rows * L, device=dev)
    deg = torch.full((P,), 9, dtype=torch.int32, device=dev)
    _, recs = probed(ops, lambda: ops.pair_head_fwd(head, i32(pi), i32(li), deg, THR, False, 0.0, SEED, None, pred))
    ran(recs, f"k_pair_fwd_mfma<{tf(L <= 256)}, false>", n_rows * L)
    cells = out.cpu()[out_rows, :L]
    assert torch.equal(cells, pred.cpu().view(n_rows, L))
    ids = torch.arange(n_rows * L)
    ref, _, S_pred, _, _ = PR.head_ref(par, pi, li, ids, 0.0, seed=SEED, scales=True)
    ref32, _ = PR.head_ref(par, pi, li, ids, 0.0, dtype=torch.float32, seed=SEED)
    e, e32 = PR.scaled_err(cells.reshape(-1), ref, S_pred, sym), PR.scaled_err(ref32, ref, S_pred)
    note(sym, "pred", e, e32)
    assert e <= 8 * max(e32, EPS), (sym, e, e32)
    assert rel(cells.reshape(-1), ref) <= 1e-5
    listed = torch.zeros(n_out, dtype=torch.bool)
    listed[out_rows] = True
    assert bool((out.cpu()[~listed] == CANARY).all()), "an unlisted output row was written"
    assert bool((out[:, L:] == CANARY).all()), "a padding column was written"


def test_zz_worst_scaled_errors():
    """Prints what the module docstring and DESIGN.md quote (run last: the cases above fill the table)."""
    for (instance, tensor), (e, e32) in sorted(WORST.items()):
        print(f"[lab edges] worst scaled error, {instance} {tensor}: kernel {e:.3e}, restatement {e32:.3e}")
