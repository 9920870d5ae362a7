"""The device's dropout RNG against tests/rng_ref.py, the host restatement: the generator's own entry points, and every
kernel that draws a mask, at element indices on both sides of 2^32, of 2^34 (the RNG group's high word turns non-zero)
and at 2^51 (the high word's 16-bit rotate matters).

Every comparison of a mask is exact equality.  Where a kernel's output is a sum over masked elements it is held against
an fp64 sum over the restated mask at the bar the kernel's own parity test uses (tests/test_ops_gpu.py,
tests/test_bnbwd_wgrad_gpu.py): one wrong keep decision moves such a sum by a whole element, orders of magnitude above
any of those bars.  Inputs are ones, or positive and different in every row, so that rows cannot swap unnoticed.
"""
import functools

import numpy as np
import pytest
import torch

import rng_ref as R

pytestmark = pytest.mark.gpu

P = 0.3
SEED = 2 ** 63 + 0x1234567                      # both words of the seed in use
IK = R.inv_keep(P)                              # float32: what a kept element is multiplied by
OFFS = ["0", "r32", "r34", "r50"]
MS = (300, 2049)                                # the small-M kernels / the matrix-core kernels + a partial tile


def row_offset(width, name):
    """Row offsets at which the rows of a tile straddle element 2^32 and element 2^34, and one whose elements start at
    2^51 (width 128: 2^25 - 7, 2^27 - 5, 2^44)."""
    return {"0": 0, "r32": 2 ** 32 // width - 7, "r34": 2 ** 34 // width - 5, "r50": 2 ** 51 // width}[name]


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


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@functools.lru_cache(maxsize=None)
def _mask_np(site, M, N, off):
    return R.mask2d(SEED, site, M, N, P, off)


def mask(site, M, N, off):
    """The restated keep-mask, bool [M, N] on the host (computed once per shape and offset, never written to)."""
    return torch.from_numpy(_mask_np(site, M, N, off))


def dropped_ones(site, M, N, off):
    """dropout(ones): float32 [M, N], exactly inv_keep where kept."""
    return torch.from_numpy(np.where(_mask_np(site, M, N, off), IK, np.float32(0.0)).astype(np.float32))


def pro_of(ops, site, off, relu=0, fold=None):
    return ops.Pro(fold.scale if fold else None, fold.shift if fold else None, relu, P, seed=SEED, site=site, row_offset=off)


def identity_fold(ops, dev, M, N):
    """A BatchNorm fold that changes nothing: scale 1, shift 0, mean 0, rstd 1 (xhat = y)."""
    one, zero = torch.ones(N, device=dev), torch.zeros(N, device=dev)
    return ops.BNFold(one, zero, zero.clone(), one.clone(), M, True)


def positive(gen, *shape):
    return torch.rand(*shape, generator=gen) + 0.5


def some_rows(M):
    rows = torch.arange(0, M, 7)
    return torch.cat([rows, torch.tensor([M - 2, M - 1])]).unique()


def as_i64(v):
    """A 64-bit pattern as the int64 a device tensor holds."""
    v &= R.M64
    return v - 2 ** 64 if v >= 2 ** 63 else v


# ------------------------------------------------------------------------------------------ a. the mask kernel itself
SUP = R.SITE_SUP
A_SITES = [0, 1, 39, 64, 65, SUP, 2 ** 32 - 1]
A_FIRSTS = [0, 3, 2 ** 32 - 40, 2 ** 34 - 40, 2 ** 51 - 40]
A_PS = [0.0, 1e-6, 0.2, 0.3, 0.5, 0.99999, 1.0]


@pytest.mark.parametrize("seed", [0, 1, 2 ** 32, 2 ** 63 + 5, 2 ** 64 - 1])
def test_dropout_mask_equals_the_restatement(ops, dev, seed):
    n = 4099
    got = {}
    for site in A_SITES:
        for first in A_FIRSTS:
            for p in A_PS:               # width 1: row_offset IS the first element
                got[site, first, p] = ops.dropout_mask(seed, site, n, 1, p, dev, row_offset=first)
    bad = []
    for (site, first, p), m in got.items():
        if not np.array_equal(m.cpu().numpy().ravel() != 0, R.keep(seed, site, first, n, p)):
            bad.append((site, first, p))
    assert not bad, bad


def test_dropout_mask_reads_the_seed_from_the_device(ops, dev):
    n = 4099
    for seed in (2 ** 63 + 5, 77):
        seed_dev = torch.tensor([as_i64(seed)], dtype=torch.int64, device=dev)
        for first in A_FIRSTS:
            m = ops.dropout_mask(123, 39, n, 1, 0.3, dev, row_offset=first, seed_dev=seed_dev)     # the argument is overridden
            assert np.array_equal(m.cpu().numpy().ravel() != 0, R.keep(seed, 39, first, n, 0.3)), (seed, first)


# ------------------------------------------------------------------------------------------ b. the supervision subset
@pytest.mark.parametrize("fraction", [0.2, 0.5])
def test_sup_mask_draw_equals_the_restatement(ops, dev, fraction):
    n = 4099
    keep_p = np.float32(1.0) - np.float32(fraction)          # the kernel's keep probability, formed in float
    for seed in (0, 2 ** 63 + 5):
        for start in (None, 0, 2 ** 32 - 3, 2 ** 40):
            ids = None if start is None else (start + torch.arange(n, dtype=torch.int64)).to(dev)
            sup, count, inv_den = ops.sup_mask_draw(n, fraction, dev, seed=seed, ids=ids)
            want = R.keep(seed, SUP, start or 0, n, keep_p)
            assert np.array_equal(sup.cpu().numpy(), want.astype(np.float32)), (seed, start)
            assert float(count) == float(want.sum()) and float(inv_den) == 1.0 / max(float(want.sum()), 1.0)
        seed_dev = torch.tensor([as_i64(seed)], dtype=torch.int64, device=dev)
        _, c2, _ = ops.sup_mask_draw(n, fraction, dev, seed=99, seed_dev=seed_dev, count_only=True)
        assert float(c2) == float(R.keep(seed, SUP, 0, n, keep_p).sum())


# ------------------------------------------------------------------------------------------ c. the seed stream
def test_seed_advance_equals_splitmix(ops, dev):
    wraps = 2 ** 64 - 0x9E3779B97F4A7C15 + 3                 # the next position is 3: the addition wraps 2^64
    for pos in (0, 123456789, wraps):
        state = (0, pos)
        t = torch.tensor([0, as_i64(pos)], dtype=torch.int64, device=dev)
        for step in range(5):
            state = R.splitmix(state)
            ops.seed_advance(t)
            got = [int(v) & R.M64 for v in t.cpu().tolist()]
            assert got == [state[0], state[1]], (pos, step)
    assert R.splitmix((0, wraps))[1] == 3


# ------------------------------------------------------------------------------------------ d. every mask-drawing kernel
@pytest.mark.parametrize("off", OFFS)
def test_affine_act_drop_and_affine_act_drop_rows(ops, dev, off):
    for N in (64, 128, 256):
        for M in MS:
            o = row_offset(N, off)
            pro = pro_of(ops, 3, o)
            y = torch.ones(M, N, device=dev)
            want = dropped_ones(3, M, N, o)
            assert torch.equal(ops.affine_act_drop(y, pro).cpu(), want), (N, M)
            rows = some_rows(M)
            assert torch.equal(ops.affine_act_drop_rows(y, pro, rows.to(dev)).cpu(), want[rows]), (N, M)


@pytest.mark.parametrize("off", OFFS)
def test_linear_fwd_prologue(ops, dev, off):
    """Identity weights: the output is dropout(ones).  K = N = 256 at M = 2049 is the three-product kernel; N != K runs
    the other tile widths."""
    for K, N in ((64, 64), (128, 128), (256, 256), (256, 64), (128, 64), (64, 128)):
        for M in MS:
            o = row_offset(K, off)
            W = torch.eye(N, K, device=dev)
            y = ops.linear_fwd(torch.ones(M, K, device=dev), W, None, pro=pro_of(ops, 1, o)).cpu()
            want = torch.zeros(M, N)
            c = min(N, K)
            want[:, :c] = dropped_ones(1, M, K, o)[:, :c]
            assert torch.equal(y != 0, want != 0), (K, N, M)
            assert rel(y, want) <= 1e-5, (K, N, M)


@pytest.mark.parametrize("off", OFFS)
def test_linear_fwd_prologue_l2_epilogue(ops, dev, off):
    M = 2049
    for K, N in ((64, 64), (128, 128), (128, 64)):
        assert ops._lib.load().mmg_linear_fwd_supported(ops.EPI_L2, M, N, K)
        o = row_offset(K, off)
        out, rn = ops.linear_l2norm_fwd(torch.ones(M, K, device=dev), torch.eye(N, K, device=dev), None, pro_of(ops, 1, o))
        m = mask(1, M, K, o)[:, :N].double()
        norm = m.sum(1).sqrt()                                     # of the row (kept, kept, ...) in units of inv_keep
        assert torch.equal(out.cpu() != 0, m != 0), (K, N)
        e_out, e_rn = rel(out, m / norm[:, None]), rel(rn, 1.0 / (norm * float(IK)))
        print(f"l2 epilogue K={K} N={N} {off}: out {e_out:.2e} rn {e_rn:.2e}")
        assert e_out <= 5e-7 and e_rn <= 5e-7, (K, N)


@pytest.mark.parametrize("off", OFFS)
def test_linear_wgrad_prologue_and_deferred(ops, dev, off):
    """dY[r, r % N] = 1: row n of dW is the sum of the dropped rows r = n (mod N) of x."""
    gen = torch.Generator().manual_seed(7)
    for N, K in ((64, 64), (128, 128), (64, 128), (128, 64), (256, 256)):
        for M in MS:
            o = row_offset(K, off)
            x = positive(gen, M, K)
            dy = torch.zeros(M, N)
            dy[torch.arange(M), torch.arange(M) % N] = 1.0
            xp = x.double() * mask(2, M, K, o).double() * float(IK)
            ref = dy.double().t() @ xp
            pro = pro_of(ops, 2, o)
            dW = ops.linear_wgrad(dy.to(dev), x.to(dev), pro)
            assert rel(dW, ref) <= 1e-5, (N, K, M)
            jobs = []
            dWd = ops.linear_wgrad(dy.to(dev), x.to(dev), pro, defer=jobs)
            ops.wgrad_reduce_flush(jobs)
            assert torch.equal(dWd, dW), (N, K, M)
            ones = torch.zeros(M, N)
            ones[:, 0] = 1.0                                        # a column of ones: row 0 = the column sums
            dW1 = ops.linear_wgrad(ones.to(dev), x.to(dev), pro)
            assert rel(dW1[0], xp.sum(0)) <= 1e-5 and float(dW1[1:].abs().max()) == 0.0, (N, K, M)


@pytest.mark.parametrize("off", OFFS)
def test_bn_bwd_stats_stats2_and_stats_rows(ops, dev, off):
    gen = torch.Generator().manual_seed(8)
    for N in (64, 128, 256):
        for M in MS:
            o = row_offset(N, off)
            fold = identity_fold(ops, dev, M, N)
            pro, pro2 = pro_of(ops, 17, o, 1, fold), pro_of(ops, 19, o, 1, fold)
            g, g2, y = positive(gen, M, N), positive(gen, M, N), positive(gen, M, N)
            ga = g.double() * mask(17, M, N, o).double() * float(IK)
            gb = g2.double() * mask(19, M, N, o).double() * float(IK)
            s = ops.bn_bwd_stats(g.to(dev), y.to(dev), pro, fold)
            assert rel(s[0], ga.sum(0)) <= 1e-6 and rel(s[1], (ga * y.double()).sum(0)) <= 1e-5, (N, M)
            s2 = ops.bn_bwd_stats2(g.to(dev), g2.to(dev), y.to(dev), pro, pro2, fold)
            assert rel(s2[0], (ga + gb).sum(0)) <= 1e-6 and rel(s2[1], ((ga + gb) * y.double()).sum(0)) <= 1e-5, (N, M)
            rows = some_rows(M)
            sr = ops.bn_bwd_stats_rows(g[rows].contiguous().to(dev), y.to(dev), rows.to(dev), pro, fold)
            assert rel(sr[0], ga[rows].sum(0)) <= 1e-6 and rel(sr[1], (ga * y.double())[rows].sum(0)) <= 1e-5, (N, M)


@pytest.mark.parametrize("off", OFFS)
def test_bn_bwd_apply_apply2_and_apply_rows(ops, dev, off):
    """An identity fold and no batch statistics: dy is the masked upstream gradient itself."""
    for N in (64, 128, 256):
        for M in MS:
            o = row_offset(N, off)
            fold = identity_fold(ops, dev, M, N)
            one = torch.ones(M, N, device=dev)
            for f in (fold, None):                                   # BatchNorm in eval mode / no BatchNorm at all
                pro = pro_of(ops, 17, o, 1, f)
                assert torch.equal(ops.bn_bwd_apply(one, one, pro, f).cpu(), dropped_ones(17, M, N, o)), (N, M)
            pro, pro2 = pro_of(ops, 17, o, 1, fold), pro_of(ops, 19, o, 1, fold)
            zsum = torch.zeros(2, N, dtype=torch.float64, device=dev)
            dy2 = ops.bn_bwd_apply2(one, one, one, pro, pro2, fold, zsum, M)
            assert torch.equal(dy2.cpu(), dropped_ones(17, M, N, o) + dropped_ones(19, M, N, o)), (N, M)
            rows = some_rows(M)
            dyr = torch.zeros(M, N, device=dev)
            ops.bn_bwd_apply_rows(torch.ones(rows.numel(), N, device=dev), one, rows.to(dev), pro, dyr)
            want = torch.zeros(M, N)
            want[rows] = dropped_ones(17, M, N, o)[rows]
            assert torch.equal(dyr.cpu(), want), (N, M)


BNBWD_M = 2049                                  # (the fused data-gradient GEMMs start above 512 rows)


@pytest.mark.parametrize("off", OFFS)
def test_linear_bnbwd_bnbwd2_bnbwd_rows_and_fused_wgrad(ops, dev, off):
    """No BatchNorm: dZ is dropout(ones) exactly; dX = dZ @ W; the fused weight gradient multiplies two masked tensors."""
    gen = torch.Generator().manual_seed(9)
    M = BNBWD_M
    for K, N in ((128, 64), (64, 128), (64, 64), (128, 128)):             # (the last one's tensors serve the rest)
        o = row_offset(K, off)
        one = torch.ones(M, K, device=dev)
        W = (torch.randn(K, N, generator=gen) / K ** 0.5).to(dev)
        assert ops.linear_bnbwd_supported(M, N, K)
        dz, dx = ops.linear_bnbwd(one, one, pro_of(ops, 39, o, 1), None, W)
        want = dropped_ones(39, M, K, o)
        assert torch.equal(dz.cpu(), want), (K, N)
        assert rel(dx, want.double() @ W.cpu().double()) <= 2e-6, (K, N)
    K = N = 128
    o = row_offset(K, off)
    fold = identity_fold(ops, dev, M, K)
    pro, pro2 = pro_of(ops, 39, o, 1, fold), pro_of(ops, 41, o, 1, fold)
    zsum = torch.zeros(2, K, dtype=torch.float64, device=dev)
    dz2, dx2 = ops.linear_bnbwd2(one, one, one, pro, pro2, fold, W, zsum, M)
    want2 = dropped_ones(39, M, K, o) + dropped_ones(41, M, K, o)
    assert torch.equal(dz2.cpu(), want2) and rel(dx2, want2.double() @ W.cpu().double()) <= 2e-6
    rows = some_rows(M)
    row_pos = torch.full((M,), -1, dtype=torch.int32, device=dev)
    row_pos[rows.to(dev)] = torch.arange(rows.numel(), dtype=torch.int32, device=dev)
    dzr, dxr = ops.linear_bnbwd_rows(torch.ones(rows.numel(), K, device=dev), row_pos, one, pro, fold, W, zsum, M)
    wantr = torch.zeros(M, K)
    wantr[rows] = want[rows]
    assert torch.equal(dzr.cpu(), wantr) and rel(dxr, wantr.double() @ W.cpu().double()) <= 2e-6
    # the weight gradient in the same launch: dW [K, N] = dZ^T @ dropout(x), x with a mask of its own
    assert ops.linear_bnbwd_wgrad_supported(M, N, K)
    x = positive(gen, M, N)
    xp = x.double() * mask(43, M, N, o).double() * float(IK)
    fw = ops.FusedWgrad(x.to(dev), pro_of(ops, 43, o))
    dzf, dxf = ops.linear_bnbwd(one, one, pro_of(ops, 39, o, 1), None, W, wgrad=fw)
    assert torch.equal(dzf.cpu(), want) and torch.equal(dxf, dx)
    assert rel(fw.dW, want.double().t() @ xp) <= 1e-5
    fw2 = ops.FusedWgrad(x.to(dev), pro_of(ops, 43, o))
    ops.linear_bnbwd2(one, one, one, pro, pro2, fold, W, zsum, M, wgrad=fw2)
    assert rel(fw2.dW, want2.double().t() @ xp) <= 1e-5
    fw3 = ops.FusedWgrad(x.to(dev), pro_of(ops, 43, o))
    ops.linear_bnbwd_rows(torch.ones(rows.numel(), K, device=dev), row_pos, one, pro, fold, W, zsum, M, wgrad=fw3)
    assert rel(fw3.dW, wantr.double().t() @ xp) <= 1e-5
    outn, rn = ops.l2norm_fwd(torch.randn(M, K, generator=gen).to(dev))          # the L2 backward: only x is masked
    fw4 = ops.FusedWgrad(x.to(dev), pro_of(ops, 43, o))
    dz4, _ = ops.linear_l2bwd(torch.randn(M, K, generator=gen).to(dev), outn, rn, W, wgrad=fw4)
    assert rel(fw4.dW, dz4.double().cpu().t() @ xp) <= 1e-5


# ---- the statistics of the NEXT BatchNorm's backward, summed in a producer's epilogue (the DPP quad path)
def _next_bn_want(out, y, site, o):
    """(sum g', sum g' * xhat) of g' = dropout(out) under an identity fold: xhat = y."""
    M, N = out.shape
    gp = out.double().cpu() * mask(site, M, N, o).double() * float(IK)
    return gp.sum(0), (gp * y.double().cpu()).sum(0)


def _next_bn(ops, dev, gen, M, N, site, o):
    y = positive(gen, M, N).to(dev)
    fold = identity_fold(ops, dev, M, N)
    return y, ops.NextBN(y, pro_of(ops, site, o, 1, fold), fold)


def _stats_are(sums, out, y, site, o, what):
    w0, w1 = _next_bn_want(out, y, site, o)
    e0, e1 = rel(sums[0], w0), rel(sums[1], w1)
    print(f"{what}: {e0:.2e} {e1:.2e}")
    assert e0 <= 1e-6 and e1 <= 1e-6, what


@pytest.mark.parametrize("off", OFFS)
def test_next_bn_statistics_from_the_linear_epilogue(ops, dev, off):
    gen = torch.Generator().manual_seed(10)
    for M, N, K in ((2049, 128, 64), (2049, 256, 64), (2049, 128, 128), (300, 128, 64)):
        o = row_offset(N, off)
        W = torch.zeros(K, N, device=dev)
        W[0] = 1.0                                                   # out = ones
        y, nb = _next_bn(ops, dev, gen, M, N, 23, o)
        out, sums = ops.linear_fwd(torch.ones(M, K, device=dev), W, w_kn=True, next_bn=nb)
        assert torch.equal(out.cpu(), torch.ones(M, N))
        _stats_are(sums, out, y, 23, o, f"linear epilogue M={M} N={N} K={K} {off}")
        xr = positive(gen, M, K).to(dev)                             # and a gradient that differs in every row
        out, sums = ops.linear_fwd(xr, W, w_kn=True, next_bn=nb)
        _stats_are(sums, out, y, 23, o, f"linear epilogue, rows differ, M={M} N={N} K={K} {off}")


@pytest.mark.parametrize("off", OFFS)
def test_next_bn_statistics_from_the_l2bwd_and_bnbwd_gemms(ops, dev, off):
    gen = torch.Generator().manual_seed(11)
    M, K, N = BNBWD_M, 128, 128
    o = row_offset(N, off)
    W = (torch.randn(K, N, generator=gen) / K ** 0.5).to(dev)
    y, nb = _next_bn(ops, dev, gen, M, N, 23, o)
    outn, rn = ops.l2norm_fwd(torch.randn(M, K, generator=gen).to(dev))
    g = torch.randn(M, K, generator=gen).to(dev)
    _, dx, s = ops.linear_l2bwd(g, outn, rn, W, next_bn=nb)
    _stats_are(s, dx, y, 23, o, f"l2bwd {off}")
    one = torch.ones(M, K, device=dev)
    dz, dx, s = ops.linear_bnbwd(one, one, pro_of(ops, 39, o, 1), None, W, next_bn=nb)
    assert torch.equal(dz.cpu(), dropped_ones(39, M, K, o))
    _stats_are(s, dx, y, 23, o, f"bnbwd {off}")
    fold = identity_fold(ops, dev, M, K)
    rows = some_rows(M)
    row_pos = torch.full((M,), -1, dtype=torch.int32, device=dev)
    row_pos[rows.to(dev)] = torch.arange(rows.numel(), dtype=torch.int32, device=dev)
    zsum = torch.zeros(2, K, dtype=torch.float64, device=dev)
    _, dx, s = ops.linear_bnbwd_rows(torch.ones(rows.numel(), K, device=dev), row_pos, one, pro_of(ops, 39, o, 1, fold), fold,
                                     W, zsum, M, next_bn=nb)
    _stats_are(s, dx, y, 23, o, f"bnbwd_rows {off}")


def _simple_edges(gen, n_rows, n_cols, max_deg):
    """Edges without duplicate (row, col) pairs and with ragged degrees (some rows empty)."""
    order = torch.rand(n_rows, n_cols, generator=gen).argsort(1)
    deg = torch.randint(0, min(max_deg, n_cols) + 1, (n_rows,), generator=gen)
    deg[::7] = 0
    r, k = torch.nonzero(torch.arange(n_cols)[None, :] < deg[:, None], as_tuple=True)
    ei = torch.stack([r, order[r, k]])
    return ei[:, torch.randperm(ei.shape[1], generator=gen)].contiguous()


@pytest.mark.parametrize("off", OFFS)
def test_next_bn_statistics_from_the_gather_epilogue(ops, dev, off):
    gen = torch.Generator().manual_seed(12)
    for D, n_rows in ((128, 2049), (256, 2049), (128, 300)):
        o = row_offset(D, off)
        rels = []
        for nc, md in zip([50, 114, 100], [50, 9, 25]):
            rp, col, _ = ops.csr_build(_simple_edges(gen, n_rows, nc, md).to(dev), n_rows, 0)
            _, inv = ops.row_degree(rp)
            _, cinv = ops.col_degree(col, nc)
            _, mask_r = ops.rel_mask_build(rp, col, nc)
            rels.append(ops.Rel(rp, col, nc, rowscale=inv, colscale=cinv, table=(positive(gen, nc, D) * 2).to(dev),
                                simple=True, mask_r=mask_r))
        y, nb = _next_bn(ops, dev, gen, n_rows, D, 23, o)
        for use in (rels[:1], rels):
            for acc in (True, False):
                out = positive(gen, n_rows, D).to(dev)
                _, sums = ops.gather_rows(use, n_rows, D, out, accumulate=acc, next_bn=nb)
                _stats_are(sums, out, y, 23, o, f"gather D={D} rows={n_rows} rels={len(use)} acc={acc} {off}")


@pytest.mark.parametrize("off", OFFS)
def test_small_bn_act_group_and_small_bn_bwd_group(ops, dev, off):
    for N in (64, 128, 256):
        o = row_offset(N, off)
        Ms = [300, 2049, 50, 2]
        items = [(torch.ones(M, N, device=dev), None, ops.Pro(None, None, 1, P, SEED, 16 + i, o + 3 * i))
                 for i, M in enumerate(Ms)]
        res = ops.small_bn_act_group(items, True)
        for i, (M, (out, fold)) in enumerate(zip(Ms, res)):
            assert fold is None and torch.equal(out.cpu(), dropped_ones(16 + i, M, N, o + 3 * i)), (N, M)
        back = ops.small_bn_bwd_group([(y, y, pro, None) for y, _, pro in items])
        for i, (M, (dy, dbeta, dgamma)) in enumerate(zip(Ms, back)):
            assert dbeta is None and torch.equal(dy.cpu(), dropped_ones(16 + i, M, N, o + 3 * i)), (N, M)


# ------------------------------------------------------------------------------------------ the pair heads
PAIR_N = 4096
# pair ids in blocks: from 0; across layer-1 element 2^32 (id 2^26); across layer-2 element 2^32 (id 2^27); across the
# id's own high word (2^32); far beyond (2^40)
PAIR_STARTS = [0, 2 ** 26 - 3, 2 ** 27 - 3, 2 ** 32 - 3, 2 ** 40]


def _pair_ids(gen, n, starts):
    per = -(-n // len(starts))
    ids = torch.cat([s + torch.arange(per, dtype=torch.int64) for s in starts])[:n]
    return ids[torch.randperm(n, generator=gen)]


def _pair_masks(pid, seed=SEED, p=P):
    pid = pid.numpy().astype(np.uint64)
    m1 = R.keep_at(seed, R.SITE_H1, pid[:, None] * np.uint64(64) + np.arange(64, dtype=np.uint64), p)
    m2 = R.keep_at(seed, R.SITE_H2, pid[:, None] * np.uint64(32) + np.arange(32, dtype=np.uint64), p)
    return torch.from_numpy(m1), torch.from_numpy(m2)


@functools.lru_cache(maxsize=None)
def _pair_problem(L):
    """Inputs and the fp64 reference (predictions, the six gradients, per gate) with the restated masks, once per L."""
    gen = torch.Generator().manual_seed(31 + L)
    Pn, n = 400, PAIR_N
    A, B = torch.randn(Pn, 64, generator=gen), torch.randn(L, 64, generator=gen)
    W2, b2 = torch.randn(32, 64, generator=gen) / 8, torch.randn(32, generator=gen) * 0.1
    W3, b3 = torch.randn(32, generator=gen) / 5, torch.randn(1, generator=gen)
    pi = torch.randint(0, Pn, (n,), generator=gen).sort().values
    li = torch.randint(0, L, (n,), generator=gen)
    deg = torch.randint(0, 12, (Pn,), generator=gen)
    pid = _pair_ids(gen, n, PAIR_STARTS)
    dpred = torch.randn(n, generator=gen) * (torch.rand(n, generator=gen) < 0.7)
    m1, m2 = _pair_masks(pid)
    refs = {}
    for want_low in (False, True):
        sel = (deg[pi] < 6) == want_low
        leaf = [t.double().requires_grad_(True) for t in (A, B, W2, b2, W3, b3)]
        h1 = torch.relu(leaf[0][pi] + leaf[1][li]) * m1.double() / (1 - P)
        h2 = torch.relu(h1 @ leaf[2].t() + leaf[3]) * m2.double() / (1 - P)
        pred = h2 @ leaf[4] + leaf[5]
        (pred * dpred.double() * sel.double()).sum().backward()
        refs[want_low] = (sel, pred.detach(), [t.grad for t in leaf])
    return dict(weights=(A, B, W2, b2, W3, b3), pi=pi, li=li, deg=deg, pid=pid, dpred=dpred, refs=refs, L=L)


@pytest.mark.parametrize("variant", ["fwd_bwd", "fwd_save_bwd_saved", "listed_fwd_save_bwd_saved", "listed_fwd_bwd"])
@pytest.mark.parametrize("L", [50, 100, 200])
def test_pair_head_masks_at_large_pair_ids(ops, dev, L, variant):
    """L = 50 / 100 / 200: the three backward kernels.  Predictions and the six gradients against fp64 with restated masks,
    at the bars of test_pair_head_fwd_bwd."""
    pb = _pair_problem(L)
    n = PAIR_N
    head = ops.Head(*[t.to(dev) for t in pb["weights"]])
    i32 = lambda t: t.to(torch.int32).to(dev)            # noqa: E731
    pi, li, deg, pid, dpred = i32(pb["pi"]), i32(pb["li"]), i32(pb["deg"]), pb["pid"].to(dev), pb["dpred"].to(dev)
    listed, saving = variant.startswith("listed"), "save" in variant
    for want_low in (False, True):
        sel, ref_pred, ref_grads = pb["refs"][want_low]
        save = ops.pair_saved_alloc(n, dev) if saving else None
        fsel = bsel = {}
        if listed:
            lo, hi, cnt = ops.pair_select(pi, deg, 6, None)
            blo, bhi, bcnt = ops.pair_select(pi, deg, 6, dpred)
            fsel = dict(sel=lo if want_low else hi, n_sel=cnt[0:1] if want_low else cnt[1:2], n_bound=n)
            bsel = dict(sel=blo if want_low else bhi, n_sel=bcnt[0:1] if want_low else bcnt[1:2], n_bound=n)
        pred = torch.full((n,), 123.0, device=dev)
        ops.pair_head_fwd(head, pi, li, deg, 6, want_low, P, SEED, pid, pred, save=save, **fsel)
        e = rel(pred[sel.to(dev)], ref_pred[sel])
        print(f"pair head L={L} {variant} low={want_low}: pred {e:.2e}")
        assert e <= 1e-5, want_low
        assert bool((pred[(~sel).to(dev)] == 123.0).all())
        g = ops.Head(*[torch.zeros_like(t, device=dev) for t in pb["weights"]])
        ops.pair_head_bwd(head, g, pi, li, deg, 6, want_low, L, P, SEED, pid, dpred, saved=save, **bsel)
        for name, got, want in zip("A B W2 b2 W3 b3".split(), (g.A, g.B, g.W2, g.b2, g.W3, g.b3), ref_grads):
            e = rel(got, want)
            print(f"pair head L={L} {variant} low={want_low}: d{name} {e:.2e}")
            assert e <= 2e-5, (name, want_low)


# ------------------------------------------------------------------------------------------ e. forward == backward
def test_dense_forward_and_backward_draw_the_same_mask(ops, dev):
    M, K = 2049, 128
    o = row_offset(K, "r34")
    pro = pro_of(ops, 1, o, 1)
    one = torch.ones(M, K, device=dev)
    fwd = ops.linear_fwd(one, torch.eye(K, device=dev), None, pro=pro) != 0
    dz, _ = ops.linear_bnbwd(one, one, pro, None, torch.eye(K, device=dev))
    assert torch.equal(fwd, dz != 0)
    assert torch.equal(fwd.cpu(), mask(1, M, K, o))


def test_pair_head_forward_and_backward_draw_the_same_masks(ops, dev):
    """One patient per pair, positive first-layer sums, W2[i, j] = [j % 32 == i], positive biases: the state the forward
    saves IS its two masks, and dA[k, j] of the recomputing backward is non-zero exactly where layer-1 unit j and
    layer-2 unit j % 32 of pair k were both kept."""
    gen = torch.Generator().manual_seed(77)
    n, L = PAIR_N, 50
    half = torch.full((n, 64), 0.5)
    W2 = torch.zeros(32, 64)
    W2[torch.arange(64) % 32, torch.arange(64)] = 1.0
    weights = (half, torch.full((L, 64), 0.5), W2, torch.ones(32), torch.ones(32), torch.zeros(1))
    head = ops.Head(*[t.to(dev) for t in weights])
    pid = _pair_ids(gen, n, [2 ** 28 - 5, 2 ** 29 - 5])             # layer-1 / layer-2 element 2^34
    m1, m2 = _pair_masks(pid)
    pi = torch.arange(n, dtype=torch.int32, device=dev)
    li = torch.randint(0, L, (n,), generator=gen).to(torch.int32).to(dev)
    deg = torch.zeros(n, dtype=torch.int32, device=dev)
    save = ops.pair_saved_alloc(n, dev)
    pred = torch.zeros(n, device=dev)
    ops.pair_head_fwd(head, pi, li, deg, 6, True, P, SEED, pid.to(dev), pred, save=save)
    bits = save[0].cpu().numpy().view(np.uint32)                    # [n, 2]
    f1 = torch.from_numpy(((bits[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(n, 64).astype(bool))
    f2 = save[1].cpu() != 0
    for saved in (None, save):
        g = ops.Head(*[torch.zeros_like(t, device=dev) for t in weights])
        ops.pair_head_bwd(head, g, pi, li, deg, 6, True, L, P, SEED, pid.to(dev), torch.ones(n, device=dev), saved=saved)
        assert torch.equal(g.A.cpu() != 0, f1 & f2.repeat(1, 2)), "recomputed" if saved is None else "saved"
    assert torch.equal(f1, m1) and torch.equal(f2, m2)
