"""The persistent kernels past their first tile per workgroup.

A fixed grid of workgroups (or waves) walks tiles t0, t0 + R, t0 + 2R, ... and keeps state across them: double-buffered
LDS planes, two tiles of X in registers, a peeled first tile pair, fp64 statistics partials, dB / dW2 accumulators, the
front / back hand-off buffers of the pair backward.  The shapes of tests/test_ops_gpu.py give every workgroup ONE tile.
Here every case runs n = T * (3R + R // 2) + 5 rows (T = tile height): half of the row sets take 4 tiles and half take 3
-- both parities of the loop, the call on a tile past the end -- and the last tile holds 5 rows.

R is never assumed: it is read from the probe (ops.probe_grids) of a launch of the same kernel family at a large size, and
every case then asserts FROM THE PROBE OF ITS OWN LAUNCH that the expected kernel instance ran and that its row sets took
3 and 4 tiles.  A retuned grid constant moves n with it; a case that lands in another regime fails, it does not skip.

Two kinds of check:
 (a) slice invariance, bit for bit: where an output row depends on its own input row only, the many-tile launch must
     equal separate launches over contiguous 1,024-row blocks (each in the single-tile regime of the same kernel) that
     straddle the boundary between ordinal j and j + 1 of the row sets, plus the block that ends at row n.  Dropout uses
     row_offset + block start (pair heads: the same pair ids), so the masks are the same by contract.
 (b) an fp64 reference on the host at the bars of the single-tile tests: dense outputs PER ROW, max|err| / max|ref row|
     <= 2e-6 (the header's stated accuracy of the split kernels; plain fp32 addmm sits at 5.5e-7 .. 9.5e-7 on these
     shapes); statistics 1e-6 against fp64 sums of the device output; weight gradients 1e-5, bias 2e-6; pair gradients
     2e-5; gather 1e-5.  Dropout masks of the references come from tests/rng_ref.py, never from the library.

Measured worst per-row error of the dense families (MI355X, these shapes and seeds; bar 2e-6):
  k_linear_fwd_x6, K <= 128 ........ 1.09e-06 (K = 128, N = 64, accumulating)
  k_linear_fwd_x6, K = 256 ......... 9.8e-07
  k_linear_fwd_h3_k256 ............. 4.3e-07
  k_linear_bnbwd_x6, dX ............ 1.02e-06
"""
import functools

import pytest
import torch

import pair_ref
import rng_ref as R
from dense_plan_ref import fwd_symbol, tf

pytestmark = pytest.mark.gpu

SEED = 2 ** 40 + 99
BIG = 200_000                  # "any large size": where the grid rule of every dense kernel has saturated
WORST = {}                     # family -> worst per-row error seen (printed by the last test of the module)


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


# ------------------------------------------------------------------------------------------ the regime, from the probe
def probed(ops, fn):
    """fn() under an armed probe -> (its result, [(kernel symbol, M, grid xyz, block x)] of the launches it made)."""
    ops.probe_arm(64)
    out = fn()
    torch.cuda.synchronize()
    rows = ops.probe_read()
    grids = ops.probe_grids()
    assert len(rows) == len(grids)
    return out, [(r[6], r[2], g, b) for r, (g, b) in zip(rows, grids)]


def launch_of(recs, want):
    hit = [r for r in recs if want in r[0]]
    assert len(hit) == 1, f"expected one launch of {want!r}, the probe saw {[r[0] for r in recs]}"
    return hit[0]


def walkers(sym, grid, block):
    """-> (R, T): how many tile walkers the launch had along its tile axis, and the tile height.  The dense kernels put the
    row sets on grid.y, the gathers on grid.x; in the pair kernels a wave (forward) or a front / back wave pair (backward)
    owns a 32-pair tile; k_pair_bwd (fp32, more than 128 labs) gives a 256-thread workgroup a 256-pair tile."""
    if sym.startswith("k_linear_"):
        return grid[1], 32
    if sym.startswith("k_gather_"):
        return grid[0], 32
    if sym.startswith("k_pair_fwd_mfma") or sym.startswith("k_pair_dense_fwd"):
        return grid[0] * (block // 64), 32
    if sym.startswith("k_pair_bwd_duo"):
        return grid[0] * (block // 128), 32
    if sym == "k_pair_bwd":
        return grid[0], 256
    raise AssertionError(f"no tile rule for {sym}")


_R_BIG = {}


def steady_n(ops, key, want, big_launch, launch_at=None):
    """The shape rule: R of `want` from one launch at a large size (cached per key) -> n = T * (3R + R // 2) + 5.
    launch_at(n): for a kernel whose grid still moves with n below the large size (the weight gradient rounds its row
    ranges to whole stages, so its n_split is not a constant): the rule is applied again to the R of a launch at the n it
    gave, until a launch at n is in the regime -- every R on the way is a probed one."""
    if key not in _R_BIG:
        _, recs = probed(ops, big_launch)
        sym, M, grid, block = launch_of(recs, want)
        Rw, T = walkers(sym, grid, block)
        assert (M + T - 1) // T >= 4 * Rw, f"{sym}: {M} rows do not saturate a grid of {Rw}"
        for _ in range(8 if launch_at is not None else 0):
            n = T * (3 * Rw + Rw // 2) + 5
            _, recs = probed(ops, lambda: launch_at(n))
            sym, M, grid, block = launch_of(recs, want)
            R_n = walkers(sym, grid, block)[0]
            lo, more = divmod((n + T - 1) // T, R_n)
            if lo == 3 and 0 < more < R_n:
                break
            Rw = R_n
        _R_BIG[key] = (Rw, T)
    Rw, T = _R_BIG[key]
    return T * (3 * Rw + Rw // 2) + 5


def regime(recs, want, n):
    """Asserts from the probe of the case's own launch: the instance `want` ran over n rows and its row sets took 3 and 4
    tiles each.  -> (symbol, R, T, histogram text)."""
    sym, M, grid, block = launch_of(recs, want)
    Rw, T = walkers(sym, grid, block)
    tiles = (n + T - 1) // T
    assert M == n, (sym, M, n)
    lo, more = divmod(tiles, Rw)
    assert lo == 3 and 0 < more < Rw, f"{sym}: {tiles} tiles over R = {Rw}: {more} x {lo + 1}, {Rw - more} x {lo}"
    return sym, Rw, T, f"{more} x 4, {Rw - more} x 3"


def blocks(n, Rw, T=32):
    """Row blocks of the slice-invariance check: 32 tiles from tile j * R + R - 16 (the last 16 row sets of ordinal j and the
    first 16 of ordinal j + 1), j = 0..3 while inside the tensor, and the block that ends at row n."""
    out = []
    for j in range(4):
        s = (j * Rw + Rw - 16) * T
        if s + 32 * T <= n:
            out.append((s, s + 32 * T))
    out.append(((n - 1024) // 32 * 32, n))
    return out


def same_rows(full, part, b0, Rw, T, what):
    got = full[b0:b0 + part.shape[0]]
    if torch.equal(got, part):
        return
    bad = int((got != part).reshape(part.shape[0], -1).any(1).nonzero()[0])
    row = b0 + bad
    pytest.fail(f"{what}: row {row} of the many-tile launch differs from its block launch "
                f"(row set {(row // T) % Rw}, ordinal {(row // T) // Rw})")


def row_err(y, ref):
    """Worst per-row error: max|err| / max|ref row| (a small row cannot hide behind a large one)."""
    y = y.double().cpu()
    assert bool(torch.isfinite(y).all())
    e = (y - ref).abs().amax(1) / ref.abs().amax(1).clamp(min=1e-300)
    return float(e.max())


def note(family, err):
    WORST[family] = max(WORST.get(family, 0.0), err)
    print(f"[steady] {family}: worst per-row error {err:.3e}")


# ------------------------------------------------------------------------------------------ host side: inputs, prologue
@functools.lru_cache(maxsize=None)
def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def _keep(site, n_rows, width, p, row_offset):
    return R.mask2d(SEED, site, n_rows, width, p, row_offset)


def keep_f64(site, n_rows, width, p, row_offset=0):
    """dropout's factor per element in fp64: inv_keep (the float32 the kernels multiply by) where kept, else 0."""
    if p == 0:
        return None
    return torch.from_numpy(_keep(site, n_rows, width, p, row_offset)).double() * float(R.inv_keep(p))


class HostPro:
    """A prologue kept on the host (fp32 tensors) beside the ops.Pro the kernels get."""

    def __init__(self, K, relu=True, p=0.0, site=3, row_offset=40, affine=True, seed=5):
        self.scale = _randn(seed, K).abs() * 0.5 + 0.5 if affine else None
        self.shift = _randn(seed + 1, K) * 0.3 if affine else None
        self.relu, self.p, self.site, self.row_offset = relu, p, site, row_offset

    def dev(self, ops, dev, b0=0, fold=None):
        sc = fold.scale if fold is not None else (self.scale.to(dev) if self.scale is not None else None)
        sh = fold.shift if fold is not None else (self.shift.to(dev) if self.shift is not None else None)
        return ops.Pro(sc, sh, self.relu, self.p, seed=SEED, site=self.site, row_offset=self.row_offset + b0)

    def apply(self, x, scale=None, shift=None):
        """dropout(relu(x * scale + shift)) in fp64 with the restated mask."""
        scale = self.scale if scale is None else scale
        shift = self.shift if shift is None else shift
        v = x.double()
        if scale is not None:
            v = v * scale.double() + shift.double()
        if self.relu:
            v = v.clamp(min=0)
        k = keep_f64(self.site, x.shape[0], x.shape[1], self.p, self.row_offset)
        return v if k is None else v * k

    def gate(self, y, scale, shift):
        """The factor the backward multiplies an upstream gradient by: keep / (1 - p) * [y * scale + shift > 0]."""
        v = y.double()
        if scale is not None:
            v = v * scale.double() + shift.double()
        g = (v > 0).double() if self.relu else torch.ones_like(v)
        k = keep_f64(self.site, y.shape[0], y.shape[1], self.p, self.row_offset)
        return g if k is None else g * k


def mm64(a, b_t, bias=None, chunk=16384):
    """a [M, K] (any float dtype) @ b_t[N, K]^T + bias in fp64, in row chunks."""
    bt = b_t.double().t().contiguous()
    out = torch.empty(a.shape[0], bt.shape[1], dtype=torch.float64)
    for i in range(0, a.shape[0], chunk):
        out[i:i + chunk] = a[i:i + chunk].double() @ bt
    return out if bias is None else out + bias.double()


def host_next_bn_sums(out, y, hp, fold):
    """What mmg_bn_bwd_stats(G = out, y, pro, mean, rstd) sums, in fp64 over the restated mask."""
    g = out.double().cpu() * hp.gate(y.cpu(), fold.scale.cpu(), fold.shift.cpu())
    xhat = (y.double().cpu() - fold.mean.double().cpu()) * fold.rstd.double().cpu()
    return torch.stack([g.sum(0), (g * xhat).sum(0)])


def bn_below(ops, dev, M, N, p, seed=71, site=23, row_offset=10):
    """A BatchNorm + ReLU + dropout 'below' a producer -> (y on the device, HostPro, BNFold, ops.Pro)."""
    y = (_randn(seed, M, N) * 1.5 + 0.2).to(dev)
    gamma, beta = (_randn(seed + 1, N).abs() * 0.5 + 0.5).to(dev), (_randn(seed + 2, N) * 0.2).to(dev)
    fold = ops.bn_finalize(ops.col_reduce2(y), M, gamma, beta, None, None, True)
    hp = HostPro(N, True, p, site=site, row_offset=row_offset, affine=False)
    return y, hp, fold, hp.dev(ops, dev, fold=fold)


# ------------------------------------------------------------------------------------------ mmg_linear_fwd
def fwd_family(K, N):
    return "h3" if K == 256 and N % 256 == 0 else ("x6 K = 256" if K == 256 else "x6 K <= 128")


def fwd_n(ops, dev, K, N):
    return steady_n(ops, ("fwd", K, N), "k_linear_fwd_",
                    lambda: ops.linear_fwd(torch.zeros(BIG, K, device=dev), torch.zeros(N, K, device=dev)))


def fwd_inputs(K, N, n):
    return _randn(K + N, n, K), _randn(K * N, N, K) / K ** 0.5, _randn(K * N + 1, N)


FWD_VARIANTS = {"plain": (False, False), "pro": (True, False), "acc": (False, True), "pro_acc": (True, True)}


def run_fwd_case(ops, dev, K, N, variant, p=0.2, with_stats=False):
    """One forward case: regime from the probe, slice invariance of Y, per-row fp64 bar; -> (Y, extras, sym, R, hist)."""
    pro, acc = FWD_VARIANTS[variant]
    n = fwd_n(ops, dev, K, N)
    x, W, b = fwd_inputs(K, N, n)
    xd, Wd, bd = x.to(dev), W.to(dev), b.to(dev)
    hp = HostPro(K, True, p) if pro else None
    base = _randn(7, n, N) if acc else None
    kw = dict(with_stats=True) if with_stats else {}

    def launch(b0, b1):
        out = base[b0:b1].to(dev) if acc else None
        return ops.linear_fwd(xd[b0:b1], Wd, bd, pro=hp.dev(ops, dev, b0) if pro else None, out=out, accumulate=acc, **kw)

    res, recs = probed(ops, lambda: launch(0, n))
    y, extra = (res[0], res[1:]) if with_stats else (res, ())
    sym, Rw, T, hist = regime(recs, fwd_symbol(K, N, pro, acc, stats=with_stats, p=p), n)
    print(f"[steady] {sym}: R = {Rw}, tiles per row set {hist}")
    for b0, b1 in blocks(n, Rw):
        part = launch(b0, b1)
        same_rows(y, part[0] if with_stats else part, b0, Rw, T, sym)
    ref = mm64(hp.apply(x) if pro else x, W, b)
    if acc:
        ref = ref + base.double()
    err = row_err(y, ref)
    note(fwd_family(K, N), err)
    assert err <= 2e-6, (sym, err)
    return y, extra, sym, Rw, hist


@pytest.mark.parametrize("variant", ["plain", "pro", "acc", "pro_acc", "w_kn"])
@pytest.mark.parametrize("K,N", [(64, 64), (128, 64), (64, 128), (128, 128)])
def test_linear_fwd_many_tiles(ops, dev, K, N, variant):
    """plain + bias, prologue (scale / shift, relu, p = 0.2, row_offset 40), accumulate, both, and the weight stored [K, N]
    (same arithmetic, same bits as the plain launch)."""
    if variant != "w_kn":
        run_fwd_case(ops, dev, K, N, variant)
        return
    n = fwd_n(ops, dev, K, N)
    x, W, b = fwd_inputs(K, N, n)
    xd, bd = x.to(dev), b.to(dev)
    y, recs = probed(ops, lambda: ops.linear_fwd(xd, W.t().contiguous().to(dev), bd, w_kn=True))
    regime(recs, fwd_symbol(K, N), n)
    err = row_err(y, mm64(x, W, b))
    note(fwd_family(K, N), err)
    assert err <= 2e-6
    assert torch.equal(y, ops.linear_fwd(xd, W.to(dev), bd))


@pytest.mark.parametrize("pro", [False, True])
@pytest.mark.parametrize("K,N", [(64, 64), (128, 128)])
def test_l2_epilogue_many_tiles(ops, dev, K, N, pro):
    """MMG_EPI_L2: Y = y / max(|y|, eps) and rnorm, slice-invariant bit for bit and against F.normalize of an fp64 product.
    rnorm: relative 2e-6 per row -- the row's elements carry at most the dense bar each and their errors do not line up, the
    32-lane tree sum of the squares adds a few 6e-8."""
    n = fwd_n(ops, dev, K, N)
    x, W, b = fwd_inputs(K, N, n)
    xd, Wd, bd = x.to(dev), W.to(dev), b.to(dev)
    hp = HostPro(K, True, 0.25, site=4, row_offset=77) if pro else None

    def launch(b0, b1):
        return ops.linear_l2norm_fwd(xd[b0:b1], Wd, bd, hp.dev(ops, dev, b0) if pro else None)

    (out, rn), recs = probed(ops, lambda: launch(0, n))
    sym, Rw, T, hist = regime(recs, fwd_symbol(K, N, pro, False, l2=True), n)
    for b0, b1 in blocks(n, Rw):
        o, r = launch(b0, b1)
        same_rows(out, o, b0, Rw, T, sym + " Y")
        same_rows(rn, r, b0, Rw, T, sym + " rnorm")
    z = mm64(hp.apply(x) if pro else x, W, b)
    nrm = z.norm(dim=1).clamp(min=ops.L2_EPS)
    err = row_err(out, z / nrm[:, None])
    note("x6 K <= 128", err)
    assert err <= 2e-6, err
    e_rn = float(((rn.double().cpu() - 1 / nrm).abs() * nrm).max())
    assert e_rn <= 2e-6, e_rn


@pytest.mark.parametrize("K,N", [(64, 64), (128, 64), (64, 128), (128, 128)])
def test_forward_statistics_and_fold_many_tiles(ops, dev, K, N):
    """with_stats: the fp64 partials of a workgroup sum over ALL of its tiles (1e-6 against fp64 sums of the device output);
    bn = ...: the fold of the same launch == with_stats + bn_finalize, bit for bit."""
    y, (sums,), sym, Rw, hist = run_fwd_case(ops, dev, K, N, "plain", with_stats=True)
    yd = y.double().cpu()
    assert rel(sums[0], yd.sum(0)) <= 1e-6 and rel(sums[1], (yd * yd).sum(0)) <= 1e-6
    n = y.shape[0]
    x, W, b = fwd_inputs(K, N, n)
    gamma, beta = (_randn(1, N).abs() + 0.5).to(dev), (_randn(2, N) * 0.2).to(dev)
    rm0, rv0 = torch.zeros(N, device=dev), torch.ones(N, device=dev)
    rm1, rv1 = rm0.clone(), rv0.clone()
    f0 = ops.bn_finalize(sums, n, gamma, beta, rm0, rv0, True, 2)
    (y1, s1, f1), recs = probed(ops, lambda: ops.linear_fwd(x.to(dev), W.to(dev), b.to(dev), bn=(gamma, beta, rm1, rv1, 2)))
    regime(recs, fwd_symbol(K, N), n)
    assert torch.equal(y1, y) and torch.equal(s1, sums)
    for a, c in ((f0.scale, f1.scale), (f0.shift, f1.shift), (f0.mean, f1.mean), (f0.rstd, f1.rstd), (rm0, rm1), (rv0, rv1)):
        assert torch.equal(a, c)


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("K", [64, 128])
def test_next_bn_epilogue_of_the_forward_many_tiles(ops, dev, K, p):
    """MMG_EPI_NEXT_BN at N = 128: the output is the plain launch's, the statistics are mmg_bn_bwd_stats of it -- summed on
    the host in fp64 over the restated mask, bar 1e-6."""
    N = 128
    n = fwd_n(ops, dev, K, N)
    dy, W = _randn(K + 5, n, K).to(dev), (_randn(K + 6, K, N) / K ** 0.5).to(dev)
    y, hp, fold, pro = bn_below(ops, dev, n, N, p)
    (out, sums), recs = probed(ops, lambda: ops.linear_fwd(dy, W, w_kn=True, next_bn=ops.NextBN(y, pro, fold)))
    sym, Rw, T, hist = regime(recs, fwd_symbol(K, N, nbn=True), n)
    assert torch.equal(out, ops.linear_fwd(dy, W, w_kn=True))
    want = host_next_bn_sums(out, y, hp, fold)
    assert rel(sums[0], want[0]) <= 1e-6 and rel(sums[1], want[1]) <= 1e-6, (rel(sums[0], want[0]), rel(sums[1], want[1]))


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("variant,p", [("plain", 0.0), ("pro", 0.0), ("pro", 0.2)])
def test_k256_three_f16_products_many_tiles(ops, dev, variant, p, acc):
    """k_linear_fwd_h3_k256: all three prologue instances x accumulate, with the forward statistics."""
    v = variant + ("_acc" if acc else "") if variant == "pro" else ("acc" if acc else "plain")
    y, (sums,), sym, Rw, hist = run_fwd_case(ops, dev, 256, 256, v, p=p, with_stats=True)
    yd = y.double().cpu()
    assert rel(sums[0], yd.sum(0)) <= 1e-6 and rel(sums[1], (yd * yd).sum(0)) <= 1e-6


@pytest.mark.parametrize("variant", ["plain", "pro"])
@pytest.mark.parametrize("N", [64, 128])
def test_k256_woven_staging_many_tiles(ops, dev, N, variant):
    """k_linear_fwd_x6<256, ...>: the staging of the next tile is dealt out between the k-steps of this one."""
    run_fwd_case(ops, dev, 256, N, variant)


@pytest.mark.parametrize("variant", ["plain", "pro"])
@pytest.mark.parametrize("K,N", [(128, 256), (256, 512)])
def test_multi_slice_shapes_many_tiles(ops, dev, K, N, variant):
    """More than one column slice: the only shapes where xcd_tile_map is not the identity."""
    run_fwd_case(ops, dev, K, N, variant)


# ------------------------------------------------------------------------------------------ mmg_linear_bnbwd (no fused wgrad)
def bnbwd_n(ops, dev, K, N):
    def big():
        z = torch.zeros(BIG, K, device=dev)
        return ops.linear_bnbwd(z, z, ops.Pro(None, None, True, 0.0), None, torch.zeros(K, N, device=dev))
    return steady_n(ops, ("bnbwd", K, N), "k_linear_bnbwd_x6", big)


def bnbwd_symbol(K, N, mode, nbn=False):
    return f"k_linear_bnbwd_x6<{K}, {N // 32}, {mode}, {tf(nbn)}>"


def check_dx(dx, dz, W, sym):
    err = row_err(dx, mm64(dz.cpu(), W.t()))
    note("bnbwd dX", err)
    assert err <= 2e-6, (sym, err)


@pytest.mark.parametrize("p,mode", [(0.0, "train"), (0.3, "train"), (0.3, "eval"), (0.3, "nobn")])
@pytest.mark.parametrize("K,N", [(128, 128), (64, 128), (128, 64), (64, 64)])
def test_bn_backward_gemm_many_tiles(ops, dev, K, N, p, mode):
    """mmg_linear_bnbwd, mode BN: dZ / dX slice-invariant given the same sums; dZ == mmg_bn_bwd_apply bit for bit and within
    2e-5 of the fp64 formula over the restated mask (the bar of the elementwise kernel); dX per row against dZ . W."""
    n = bnbwd_n(ops, dev, K, N)
    y, g = (_randn(K, n, K) * 1.5 + 0.2).to(dev), _randn(K + 1, n, K).to(dev)
    W = _randn(K * N + 3, K, N) / K ** 0.5
    Wd = W.to(dev)
    hp = HostPro(K, True, p, site=3, row_offset=1000, affine=False)
    fold = sums = None
    if mode != "nobn":
        gamma, beta = (_randn(11, K).abs() * 0.5 + 0.5).to(dev), (_randn(12, K) * 0.2).to(dev)
        rm, rv = torch.zeros(K, device=dev), torch.ones(K, device=dev)
        fold = ops.bn_finalize(ops.col_reduce2(y) if mode == "train" else None, n, gamma, beta, rm, rv, mode == "train")
        if mode == "train":
            sums = ops.bn_bwd_stats(g, y, hp.dev(ops, dev, fold=fold), fold)
    d0, d1 = torch.zeros(2, K, device=dev), torch.zeros(2, K, device=dev)

    def launch(b0, b1, dbg=None):
        pro = hp.dev(ops, dev, b0, fold=fold)
        if sums is not None:
            return ops.linear_bnbwd(g[b0:b1], y[b0:b1], pro, fold, Wd, sums, n, *(dbg if dbg is not None else (None, None)))
        return ops.linear_bnbwd(g[b0:b1], y[b0:b1], pro, fold, Wd)

    (dz, dx), recs = probed(ops, lambda: launch(0, n, (d1[0], d1[1])))
    sym, Rw, T, hist = regime(recs, bnbwd_symbol(K, N, 0), n)
    print(f"[steady] {sym}: R = {Rw}, tiles per row set {hist}")
    for b0, b1 in blocks(n, Rw):
        z, xx = launch(b0, b1)
        same_rows(dz, z, b0, Rw, T, sym + " dZ")
        same_rows(dx, xx, b0, Rw, T, sym + " dX")
    pro = hp.dev(ops, dev, fold=fold)
    if sums is not None:
        dz_ref = ops.bn_bwd_apply(g, y, pro, fold, sums, n, d0[0], d0[1])
    else:
        dz_ref = ops.bn_bwd_apply(g, y, pro, fold)
    assert torch.equal(dz, dz_ref) and torch.equal(d0, d1)
    # the fp64 formula: dy = scale * (g_out - c0 - xhat * c1)
    sc, sh = (fold.scale.cpu(), fold.shift.cpu()) if fold is not None else (None, None)
    want = g.double().cpu() * hp.gate(y.cpu(), sc, sh)
    if fold is not None:
        if sums is not None:
            xhat = (y.double().cpu() - fold.mean.double().cpu()) * fold.rstd.double().cpu()
            want = want - sums[0].cpu() / n - xhat * (sums[1].cpu() / n)
        want = want * sc.double()
    assert rel(dz, want) <= 2e-5, rel(dz, want)
    check_dx(dx, dz, W, sym)


@pytest.mark.parametrize("K,N", [(128, 128), (64, 128), (128, 64), (64, 64)])
def test_l2_backward_gemm_many_tiles(ops, dev, K, N):
    """mode L2: dZ = rn * (G - out <G, out>) within 2e-6 of fp64 (the single-tile bar), dX per row, both slice-invariant."""
    n = bnbwd_n(ops, dev, K, N)
    z = _randn(K + 2, n, K).clone()
    z[7] = 0.0
    g = _randn(K + 1, n, K).to(dev)
    W = _randn(K * N + 3, K, N) / K ** 0.5
    Wd = W.to(dev)
    out, rn = ops.l2norm_fwd(z.to(dev))
    (dz, dx), recs = probed(ops, lambda: ops.linear_l2bwd(g, out, rn, Wd))
    sym, Rw, T, hist = regime(recs, bnbwd_symbol(K, N, 1), n)
    for b0, b1 in blocks(n, Rw):
        zz, xx = ops.linear_l2bwd(g[b0:b1], out[b0:b1], rn[b0:b1], Wd)
        same_rows(dz, zz, b0, Rw, T, sym + " dZ")
        same_rows(dx, xx, b0, Rw, T, sym + " dX")
    o64, g64, r64 = out.double().cpu(), g.double().cpu(), rn.double().cpu()
    want = r64[:, None] * (g64 - o64 * (g64 * o64).sum(1, keepdim=True))
    keep = torch.ones(n, dtype=torch.bool)
    keep[7] = False                                                      # the clamped row: dz = g / eps, compared exactly
    assert rel(dz.cpu()[keep], want[keep]) <= 2e-6
    assert torch.equal(dz[7], ops.l2norm_bwd(g[:32], out[:32], rn[:32])[7])
    check_dx(dx[keep.to(dev)], dz[keep.to(dev)], W, sym)


def test_joint_bn_backward_gemm_many_tiles(ops, dev):
    """mode BN2 at 128 / 128 == mmg_bn_bwd_apply2 + mmg_linear_fwd(W_KN) bit for bit; slice-invariant; dX per row."""
    K = N = 128
    n = bnbwd_n(ops, dev, K, N)
    y, g, g2 = (_randn(K, n, K) * 1.5 + 0.2).to(dev), _randn(K + 1, n, K).to(dev), _randn(K + 4, n, K).to(dev)
    W = _randn(K * N + 3, K, N) / K ** 0.5
    Wd = W.to(dev)
    gamma, beta = (_randn(11, K).abs() * 0.5 + 0.5).to(dev), (_randn(12, K) * 0.2).to(dev)
    fold = ops.bn_finalize(ops.col_reduce2(y), n, gamma, beta, None, None, True)
    pa = lambda b0: ops.Pro(fold.scale, fold.shift, True, 0.3, seed=SEED, site=0, row_offset=10 + b0)
    pb = lambda b0: ops.Pro(fold.scale, fold.shift, True, 0.3, seed=SEED, site=2, row_offset=10 + b0)
    sums = ops.bn_bwd_stats2(g, g2, y, pa(0), pb(0), fold)
    d0, d1 = torch.zeros(2, K, device=dev), torch.zeros(2, K, device=dev)
    (dz, dx), recs = probed(ops, lambda: ops.linear_bnbwd2(g, g2, y, pa(0), pb(0), fold, Wd, sums, n, d1[0], d1[1]))
    sym, Rw, T, hist = regime(recs, bnbwd_symbol(K, N, 2), n)
    for b0, b1 in blocks(n, Rw):
        zz, xx = ops.linear_bnbwd2(g[b0:b1], g2[b0:b1], y[b0:b1], pa(b0), pb(b0), fold, Wd, sums, n)
        same_rows(dz, zz, b0, Rw, T, sym + " dZ")
        same_rows(dx, xx, b0, Rw, T, sym + " dX")
    dz_ref = ops.bn_bwd_apply2(g, g2, y, pa(0), pb(0), fold, sums, n, d0[0], d0[1])
    assert torch.equal(dz, dz_ref) and torch.equal(d0, d1)
    assert torch.equal(dx, ops.linear_fwd(dz_ref, Wd, w_kn=True))
    check_dx(dx, dz, W, sym)


@pytest.mark.parametrize("n_sel,nbn", [(157, False), (0, False), (157, True)])
def test_row_list_bn_backward_gemm_many_tiles(ops, dev, n_sel, nbn):
    """mode ROWS at 128 / 128: 157 listed rows spread so that every ordinal of the row sets holds some (the last row among
    them), and an empty list; with nbn the statistics of the next BatchNorm backward on top (host fp64, 1e-6)."""
    K = N = 128
    n = bnbwd_n(ops, dev, K, N)
    y = (_randn(K, n, K) * 1.5 + 0.2).to(dev)
    W = _randn(K * N + 3, K, N) / K ** 0.5
    Wd = W.to(dev)
    rows = torch.linspace(0, n - 1, n_sel).round().long().unique().to(dev) if n_sel else torch.zeros(0, dtype=torch.long, device=dev)
    g_rows = _randn(K + 9, max(n_sel, 1), K)[:rows.numel()].to(dev)
    row_pos = torch.full((n,), -1, dtype=torch.int32, device=dev)
    row_pos[rows] = torch.arange(rows.numel(), dtype=torch.int32, device=dev)
    gamma, beta = (_randn(11, K).abs() * 0.5 + 0.5).to(dev), (_randn(12, K) * 0.2).to(dev)
    fold = ops.bn_finalize(ops.col_reduce2(y), n, gamma, beta, None, None, True)
    pro = lambda b0: ops.Pro(fold.scale, fold.shift, True, 0.3, seed=SEED, site=1, row_offset=10 + b0)
    sums = ops.bn_bwd_stats_rows(g_rows, y, rows, pro(0), fold) if rows.numel() else torch.zeros(2, K, dtype=torch.float64, device=dev)
    d0, d1 = torch.zeros(2, K, device=dev), torch.zeros(2, K, device=dev)
    nb = {}
    if nbn:
        yb, hpb, fold_b, pro_b = bn_below(ops, dev, n, N, 0.3)
        nb = dict(next_bn=ops.NextBN(yb, pro_b, fold_b))
    res, recs = probed(ops, lambda: ops.linear_bnbwd_rows(g_rows, row_pos, y, pro(0), fold, Wd, sums, n, d1[0], d1[1], **nb))
    dz, dx = res[0], res[1]
    sym, Rw, T, hist = regime(recs, bnbwd_symbol(K, N, 3, nbn), n)
    if rows.numel():
        ordinals = set(((rows.cpu() // T) // Rw).tolist())
        assert ordinals == {0, 1, 2, 3}, ordinals
    for b0, b1 in blocks(n, Rw):
        zz, xx = ops.linear_bnbwd_rows(g_rows, row_pos[b0:b1].contiguous(), y[b0:b1], pro(b0), fold, Wd, sums, n)
        same_rows(dz, zz, b0, Rw, T, sym + " dZ")
        same_rows(dx, xx, b0, Rw, T, sym + " dX")
    dz_ref = ops.bn_bwd_apply(None, y, pro(0), fold, sums, n, d0[0], d0[1])
    if rows.numel():
        ops.bn_bwd_apply_rows(g_rows, y, rows, pro(0), dz_ref)
    assert torch.equal(d0, d1)
    rest = torch.ones(n, dtype=torch.bool, device=dev)
    rest[rows] = False
    assert torch.equal(dz[rest], dz_ref[rest]) and rel(dz, dz_ref) <= 1e-6
    check_dx(dx, dz, W, sym)
    if nbn:
        want = host_next_bn_sums(dx, yb, hpb, fold_b)
        assert rel(res[2][0], want[0]) <= 1e-6 and rel(res[2][1], want[1]) <= 1e-6


def test_next_bn_statistics_of_the_bn_backward_gemm_many_tiles(ops, dev):
    """mode BN with the next BatchNorm's statistics in the epilogue: dZ / dX unchanged, the sums against host fp64 (1e-6)."""
    K = N = 128
    n = bnbwd_n(ops, dev, K, N)
    y, g = (_randn(K, n, K) * 1.5 + 0.2).to(dev), _randn(K + 1, n, K).to(dev)
    Wd = (_randn(K * N + 3, K, N) / K ** 0.5).to(dev)
    gamma, beta = (_randn(11, K).abs() * 0.5 + 0.5).to(dev), (_randn(12, K) * 0.2).to(dev)
    fold = ops.bn_finalize(ops.col_reduce2(y), n, gamma, beta, None, None, True)
    pro = ops.Pro(fold.scale, fold.shift, True, 0.3, seed=SEED, site=31, row_offset=10)
    sums = ops.bn_bwd_stats(g, y, pro, fold)
    yb, hpb, fold_b, pro_b = bn_below(ops, dev, n, N, 0.3)
    (dz, dx, got), recs = probed(ops, lambda: ops.linear_bnbwd(g, y, pro, fold, Wd, sums, n, next_bn=ops.NextBN(yb, pro_b, fold_b)))
    regime(recs, bnbwd_symbol(K, N, 0, True), n)
    dz0, dx0 = ops.linear_bnbwd(g, y, pro, fold, Wd, sums, n)
    assert torch.equal(dz, dz0) and torch.equal(dx, dx0)
    want = host_next_bn_sums(dx, yb, hpb, fold_b)
    assert rel(got[0], want[0]) <= 1e-6 and rel(got[1], want[1]) <= 1e-6


# ------------------------------------------------------------------------------------------ mmg_linear_wgrad
@pytest.mark.parametrize("N,K,pro", [(128, 128, False), (128, 128, True), (64, 128, False), (128, 64, True), (64, 64, False)])
def test_linear_wgrad_many_stages(ops, dev, N, K, pro):
    """R = n_split (grid.y): every workgroup reduces 3 or 4 stages of 32 rows into its slab.  fp64 reference 1e-5, bias 2e-6;
    with the bias, accumulating, and deferred + wgrad_reduce_flush (the same slabs, the same sums: bit for bit).  n_split
    still moves with n at these sizes, so steady_n re-applies the rule to probed launches (today: R = 225 at 28,677 rows,
    222 workgroups with 4 stages and 3 with 3)."""
    if N == 128 and K == 128 and not pro:
        want = "k_linear_wgrad_ws"                   # the role-specialised kernel of the plain 128 x 128 case
    else:
        want = f"k_linear_wgrad_x6<{N}, {K}, {N // 32}, {2 if N == 128 else K // 32}, {tf(pro)}>"
    at = lambda m: ops.linear_wgrad(torch.zeros(m, N, device=dev), torch.zeros(m, K, device=dev))
    n = steady_n(ops, ("wgrad", N, K), "k_linear_wgrad_", lambda: at(BIG), at)
    dy, x = _randn(N + 1, n, N), _randn(K + N, n, K)
    dyd, xd = dy.to(dev), x.to(dev)
    hp = HostPro(K, True, 0.2) if pro else None
    prd = hp.dev(ops, dev) if pro else None
    (dW, db), recs = probed(ops, lambda: ops.linear_wgrad(dyd, xd, prd, with_bias=True))
    sym, Rw, T, hist = regime(recs, want, n)
    print(f"[steady] {sym}: R = {Rw}, stages per workgroup {hist}")
    ref = mm64(dy.t(), (hp.apply(x) if pro else x.double()).t())
    assert rel(dW, ref) <= 1e-5, rel(dW, ref)
    assert rel(db, dy.double().sum(0)) <= 2e-6
    assert torch.equal(ops.linear_wgrad(dyd, xd, prd), dW)                    # without the bias: the same slabs
    acc = dW.clone()
    ops.linear_wgrad(dyd, xd, prd, out=acc, accumulate=True)
    assert rel(acc, 2 * ref) <= 1e-5
    jobs, later = [], torch.empty_like(dW)
    _, db2 = ops.linear_wgrad(dyd, xd, prd, out=later, with_bias=True, defer=jobs)
    ops.wgrad_reduce_flush(jobs)
    assert torch.equal(later, dW) and torch.equal(db2, db)


# ------------------------------------------------------------------------------------------ mmg_gather_rows
def simple_edges(gen, n_rows, n_cols, max_deg):
    """Edges without duplicate (row, col) pairs and with ragged degrees (some rows empty) -- as tests/test_ops_gpu.py."""
    order = torch.rand(n_rows, n_cols, generator=gen).argsort(1)
    deg = torch.randint(0, min(max_deg, n_cols) + 1, (n_rows,), generator=gen)
    deg[::7] = 0
    keep = torch.arange(n_cols)[None, :] < deg[:, None]
    r, k = torch.nonzero(keep, as_tuple=True)
    ei = torch.stack([r, order[r, k]])
    return ei[:, torch.randperm(ei.shape[1], generator=gen)].contiguous()


_GRAPHS = {}


def graph(ops, dev, n_rows, sizes):
    """[(edge_index on the host, rowptr, col, 1 / row degree, 1 / col degree, mask_r)] per relation, built once."""
    key = (n_rows, tuple(sizes))
    if key not in _GRAPHS:
        gen = torch.Generator().manual_seed(n_rows + sum(sizes))
        out = []
        for nc, md in zip(sizes, [50, 9, 25]):
            ei = simple_edges(gen, n_rows, nc, md)
            rp, col, _ = ops.csr_build(ei.to(dev), n_rows, 0)
            _, inv = ops.row_degree(rp)
            _, cinv = ops.col_degree(col, nc)
            _, mask_r = ops.rel_mask_build(rp, col, nc)
            out.append((ei, rp, col, inv, cinv, mask_r))
        _GRAPHS[key] = out
    return _GRAPHS[key]


def gather_case(ops, dev, n_rows, sizes, D, n_rel):
    """-> (rels, fp64 reference [n_rows, D])."""
    rels, ref = [], torch.zeros(n_rows, D, dtype=torch.float64)
    for k, ((ei, rp, col, inv, cinv, mask_r), nc) in enumerate(zip(graph(ops, dev, n_rows, sizes)[:n_rel], sizes)):
        tab = _randn(100 + k + D, nc, D) * 2
        rels.append(ops.Rel(rp, col, nc, rowscale=inv, colscale=cinv, table=tab.to(dev), simple=True, mask_r=mask_r))
        src = tab.double() * cinv.cpu().double()[:, None]
        s = torch.zeros(n_rows, D, dtype=torch.float64).index_add_(0, ei[0], src[ei[1]])
        ref += s * inv.cpu().double()[:, None]
    return rels, ref


EICU = (50, 114, 100)            # 64 | 128 | 128 padded items: the layout with a static bit-plane instance


def gather_n(ops, dev, D, sizes, want):
    def big():
        rels, _ = gather_case(ops, dev, 40_000, sizes, D, len(sizes))
        return ops.gather_rows(rels, 40_000, D, torch.empty(40_000, D, device=dev), accumulate=False)
    return steady_n(ops, ("gather", D, sizes), want, big)


@pytest.mark.parametrize("what", ["plain", "acc", "stats", "nbn0", "nbn3"])
@pytest.mark.parametrize("n_rel", [3, 1])
@pytest.mark.parametrize("D", [128, 256])
def test_gather_bit_planes_many_tiles(ops, dev, D, n_rel, what):
    """k_gather_bits over the eICU vocabulary and over its first relation alone: plain, accumulate, the forward statistics,
    the next BatchNorm's statistics (p = 0 / 0.3) -- 1e-5 against fp64, statistics 1e-6 against fp64 sums over the device
    output."""
    n = gather_n(ops, dev, D, EICU, "k_gather_bits")
    rels, ref = gather_case(ops, dev, n, EICU, D, n_rel)
    base = _randn(D + 3, n, D)
    acc = what == "acc"
    out = base.to(dev).clone() if acc else torch.full((n, D), 7.0, device=dev)
    kw = {}
    if what == "stats":
        kw = dict(with_stats=True)
    elif what.startswith("nbn"):
        y, hp, fold, pro = bn_below(ops, dev, n, D, 0.3 if what == "nbn3" else 0.0)
        kw = dict(next_bn=ops.NextBN(y, pro, fold))
    res, recs = probed(ops, lambda: ops.gather_rows(rels, n, D, out, accumulate=acc, **kw))
    nk = "20, 4, 12" if n_rel == 3 else "4, 4, 4"
    sym, Rw, T, hist = regime(recs, f"k_gather_bits<{nk}, {tf(acc)}, {tf(what.startswith('nbn'))}>", n)
    print(f"[steady] {sym}: R = {Rw}, tiles per row set {hist}")
    assert rel(out, ref + base.double() if acc else ref) <= 1e-5
    od = out.double().cpu()
    if what == "stats":
        assert rel(res[1][0], od.sum(0)) <= 1e-6 and rel(res[1][1], (od * od).sum(0)) <= 1e-6
    elif kw:
        want = host_next_bn_sums(out, y, hp, fold)
        assert rel(res[1][0], want[0]) <= 1e-6 and rel(res[1][1], want[1]) <= 1e-6


@pytest.mark.parametrize("what", ["plain", "acc", "stats"])
def test_gather_units_many_tiles(ops, dev, what):
    """A vocabulary without a static bit-plane instance (50 / 200 / 100 items, the MIMIC caps): one unit of at most 128
    items per wave, k_gather_units."""
    D, sizes = 128, (50, 200, 100)
    n = gather_n(ops, dev, D, sizes, "k_gather_units")
    rels, ref = gather_case(ops, dev, n, sizes, D, 3)
    base = _randn(D + 3, n, D)
    acc = what == "acc"
    out = base.to(dev).clone() if acc else torch.full((n, D), 7.0, device=dev)
    res, recs = probed(ops, lambda: ops.gather_rows(rels, n, D, out, accumulate=acc, with_stats=what == "stats"))
    regime(recs, f"k_gather_units<{tf(acc)}>", n)
    assert rel(out, ref + base.double() if acc else ref) <= 1e-5
    if what == "stats":
        od = out.double().cpu()
        assert rel(res[1][0], od.sum(0)) <= 1e-6 and rel(res[1][1], (od * od).sum(0)) <= 1e-6


# ------------------------------------------------------------------------------------------ pair heads
P_PAT = 3000


def head_params(L):
    A, B = _randn(31, P_PAT, 64), _randn(32 + L, L, 64)
    W2, b2 = _randn(33, 32, 64) / 8, _randn(34, 32) * 0.1
    W3, b3 = _randn(35, 32) / 5, _randn(36, 1)
    return A, B, W2, b2, W3, b3


head_ref = functools.partial(pair_ref.head_ref, seed=SEED)      # the head in fp64 (tests/pair_ref.py), on this file's streams


def pair_fwd_n(ops, dev):
    def big():
        n = 1 << 21
        z = torch.zeros(n, dtype=torch.int32, device=dev)
        head = ops.Head(*[t.to(dev) for t in head_params(50)])
        return ops.pair_head_fwd(head, z, z, torch.zeros(P_PAT, dtype=torch.int32, device=dev), 6, False, 0.0, SEED, None,
                                 torch.empty(n, device=dev))
    return steady_n(ops, ("pair_fwd",), "k_pair_fwd_mfma", big)


_PAIR_FWD = {}


def pair_fwd_data(ops, dev, L, p, listed):
    """Pair arrays and the fp64 predictions of the visited pairs, once per (labs, p, listed).  Full sweep: n pairs, mixed
    degrees, the high-degree head visits its share and leaves the rest alone.  Listed: n + n // 3 pairs of which exactly
    n belong to the high-degree head -- the compacted list is then n long."""
    key = (L, p, listed)
    if key not in _PAIR_FWD:
        n = pair_fwd_n(ops, dev)
        gen = torch.Generator().manual_seed(L + int(listed))
        deg = torch.randint(0, 12, (P_PAT,), generator=gen)
        if listed:
            deg[:P_PAT // 2], deg[P_PAT // 2:] = 3, 9
            pi = torch.cat([torch.randint(P_PAT // 2, P_PAT, (n,), generator=gen), torch.randint(0, P_PAT // 2, (n // 3,), generator=gen)])
            pi = pi[torch.randperm(pi.numel(), generator=gen)]
        else:
            pi = torch.randint(0, P_PAT, (n,), generator=gen)
        li = torch.randint(0, L, (pi.numel(),), generator=gen)
        pid = torch.randperm(pi.numel(), generator=gen) + 12345
        params = head_params(L)
        ref, _ = head_ref(params, pi, li, pid, p)
        _PAIR_FWD[key] = (n, params, pi, li, deg, pid, ref)
    return _PAIR_FWD[key]


@pytest.mark.parametrize("listed", [False, True])
@pytest.mark.parametrize("save", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("L", [50, 300])
def test_pair_head_forward_many_tiles(ops, dev, L, p, save, listed):
    """k_pair_fwd_mfma, lab table in LDS (50 labs) and not (300): every wave walks 3 or 4 tiles of 32 pairs.  Predictions
    1e-5 against fp64 (the single-tile bar); unvisited pairs untouched; full sweep: predictions and the saved state equal
    block launches over the same pair ids bit for bit; saving changes nothing in the predictions."""
    n, params, pi, li, deg, pid, ref = pair_fwd_data(ops, dev, L, p, listed)
    head = ops.Head(*[t.to(dev) for t in params])
    i32 = lambda t: t.to(torch.int32).to(dev)
    pi_d, li_d, deg_d, pid_d = i32(pi), i32(li), i32(deg), pid.to(dev)
    n_total = pi.numel()
    visited = deg[pi] >= 6
    kw = {}
    if listed:
        lo, hi, cnt = ops.pair_select(pi_d, deg_d, 6)
        assert int(cnt[1]) == n
        kw = dict(sel=hi, n_sel=cnt[1:2], n_bound=n)
    sv = ops.pair_saved_alloc(n_total, dev) if save else None
    pred = torch.full((n_total,), 123.0, device=dev)
    _, recs = probed(ops, lambda: ops.pair_head_fwd(head, pi_d, li_d, deg_d, 6, False, p, SEED, pid_d, pred, save=sv, **kw))
    sym, Rw, T, hist = regime(recs, f"k_pair_fwd_mfma<{tf(L <= 256)}, {tf(save)}>", n)
    print(f"[steady] {sym}: R = {Rw} waves, tiles per wave {hist}")
    assert rel(pred[visited.to(dev)], ref[visited]) <= 1e-5
    assert bool((pred[(~visited).to(dev)] == 123.0).all())
    if save:
        plain = torch.full((n_total,), 123.0, device=dev)
        ops.pair_head_fwd(head, pi_d, li_d, deg_d, 6, False, p, SEED, pid_d, plain, **kw)
        assert torch.equal(plain, pred)
    if not listed:
        for b0, b1 in blocks(n, Rw):
            part = torch.full((b1 - b0,), 123.0, device=dev)
            svp = ops.pair_saved_alloc(b1 - b0, dev) if save else None
            if save:
                svp[0].copy_(sv[0][b0:b1]); svp[1].copy_(sv[1][b0:b1])      # entries of unvisited pairs: left as they are
            ops.pair_head_fwd(head, pi_d[b0:b1], li_d[b0:b1], deg_d, 6, False, p, SEED, pid_d[b0:b1], part, save=svp)
            same_rows(pred, part, b0, Rw, T, sym + " pred")
            if save:
                v = visited[b0:b1].to(dev)
                same_rows(sv[0][b0:b1][v], svp[0][v], 0, Rw, T, sym + " saved bits")
                same_rows(sv[1][b0:b1][v], svp[1][v], 0, Rw, T, sym + " saved h2")


@pytest.mark.parametrize("L", [50, 300])
def test_pair_head_dense_forward_many_tiles(ops, dev, L):
    """mmg_pair_head_dense_fwd with 3 and 4 tiles of 32 cells per wave: bitwise what the pair forward gives for the same
    (patient row, lab) pairs with p = 0 -- itself in the many-tile regime."""
    n = pair_fwd_n(ops, dev)
    n_rows = (n + L - 1) // L
    params = head_params(L)
    head = ops.Head(*[t.to(dev) for t in params])
    gen = torch.Generator().manual_seed(L)
    rows = torch.randint(0, P_PAT, (n_rows,), generator=gen).to(torch.int32).to(dev)
    out_rows = torch.randperm(n_rows, generator=gen).to(torch.int32).to(dev)
    out = torch.full((n_rows, L + 3), -7.0, device=dev)
    _, recs = probed(ops, lambda: ops.pair_head_dense_fwd(head, rows, out_rows, out))
    regime(recs, f"k_pair_dense_fwd<{tf(L <= 256)}>", n_rows * L)
    pi = rows.repeat_interleave(L)
    li = torch.arange(L, dtype=torch.int32, device=dev).repeat(n_rows)
    pred = torch.empty(n_rows * L, device=dev)
    deg = torch.full((P_PAT,), 9, dtype=torch.int32, device=dev)
    _, recs = probed(ops, lambda: ops.pair_head_fwd(head, pi, li, deg, 6, False, 0.0, SEED, None, pred))
    regime(recs, f"k_pair_fwd_mfma<{tf(L <= 256)}, false>", n_rows * L)
    assert torch.equal(out[out_rows.long(), :L], pred.view(n_rows, L))
    assert bool((out[:, L:] == -7.0).all())


def pair_bwd_case(ops, dev, L, want, T_big=1 << 20):
    def big():
        z = torch.zeros(T_big, dtype=torch.int32, device=dev)
        head = ops.Head(*[t.to(dev) for t in head_params(L)])
        g = ops.Head(*[torch.zeros_like(t) for t in (head.A, head.B, head.W2, head.b2, head.W3, head.b3)])
        return ops.pair_head_bwd(head, g, z, z, torch.zeros(P_PAT, dtype=torch.int32, device=dev), 6, False, L, 0.0, SEED, None,
                                 torch.zeros(T_big, device=dev))
    n = steady_n(ops, ("pair_bwd", L), want, big)
    gen = torch.Generator().manual_seed(57 + L)
    pi = torch.randint(0, P_PAT, (n,), generator=gen).sort().values        # a patient's run straddles tiles and iterations
    li = torch.randint(0, L, (n,), generator=gen)
    deg = torch.randint(0, 12, (P_PAT,), generator=gen)
    dpred = _randn(58, n) * (torch.rand(n, generator=gen) < 0.6)
    return n, pi, li, deg, dpred


def zero_grads(ops, head):
    return ops.Head(*[torch.zeros_like(t) for t in (head.A, head.B, head.W2, head.b2, head.W3, head.b3)])


def check_grads(g, want, tag):
    for name, got, w in zip("A B W2 b2 W3 b3".split(), (g.A, g.B, g.W2, g.b2, g.W3, g.b3), want):
        assert rel(got, w.reshape(got.shape)) <= 2e-5, (tag, name, rel(got, w.reshape(got.shape)))


@pytest.mark.parametrize("aux", [False, True])
def test_pair_head_backward_50_labs_many_tiles(ops, dev, aux):
    """k_pair_bwd_duo6 over n_iter = 3 and 4: the dB / dW2 accumulators and the front / back hand-off across iterations,
    recomputing and from the state the forward saved (bitwise equal to each other up to the order of dA's atomics, see
    below), without and with pair_id / io_perm; 2e-5 against fp64."""
    L, p = 50, 0.2
    n, pi, li, deg, dpred = pair_bwd_case(ops, dev, L, "k_pair_bwd_duo6")
    params = head_params(L)
    head = ops.Head(*[t.to(dev) for t in params])
    i32 = lambda t: t.to(torch.int32).to(dev)
    pi_d, li_d, deg_d = i32(pi), i32(li), i32(deg)
    gen = torch.Generator().manual_seed(3)
    pid = torch.randperm(n, generator=gen) + 777 if aux else torch.arange(n)
    io = torch.randperm(n, generator=gen) if aux else None
    pid_d, io_d = (pid.to(dev), io.to(dev)) if aux else (None, None)
    dp_caller = torch.empty(n)
    if aux:
        dp_caller[io] = dpred                                               # pair k reads dpred[io_perm[k]]
    else:
        dp_caller = dpred
    dp_d = dp_caller.to(dev)
    sel = deg[pi] >= 6
    _, want = head_ref(params, pi, li, pid, p, dpred * sel)
    sv = ops.pair_saved_alloc(n, dev)
    pred = torch.zeros(n, device=dev)
    ops.pair_head_fwd(head, pi_d, li_d, deg_d, 6, False, p, SEED, pid_d, pred, io_perm=io_d, save=sv)
    g0, g1 = zero_grads(ops, head), zero_grads(ops, head)
    _, r0 = probed(ops, lambda: ops.pair_head_bwd(head, g0, pi_d, li_d, deg_d, 6, False, L, p, SEED, pid_d, dp_d, io_perm=io_d))
    _, r1 = probed(ops, lambda: ops.pair_head_bwd(head, g1, pi_d, li_d, deg_d, 6, False, L, p, SEED, pid_d, dp_d, io_perm=io_d,
                                                  saved=sv))
    sym, Rw, T, hist = regime(r0, f"k_pair_bwd_duo6<2, {tf(aux)}, false>", n)
    print(f"[steady] {sym}: R = {Rw} wave pairs, iterations per wave pair {hist}")
    regime(r1, f"k_pair_bwd_duo6<2, {tf(aux)}, true>", n)
    check_grads(g0, want, "recomputing")
    check_grads(g1, want, "saved")
    # what the recomputing kernel recomputes IS what the forward saved: dB, dW2, db2, dW3, db3 (fixed-order slab sums) bit
    # for bit.  dA: the same run sums per tile, added by atomics -- a + b either way where a patient's pairs lie in at
    # most two tiles, but THREE partial sums (a run of more than 32 pairs: most patients here) in whatever order the wave
    # pairs arrive, so those rows agree to the rounding of two fp32 additions, not to the bit
    for name in "B W2 b2 W3 b3".split():
        assert torch.equal(getattr(g0, name), getattr(g1, name)), name
    first = torch.full((P_PAT,), n, dtype=torch.long).scatter_reduce(0, pi, torch.arange(n), "amin")
    last = torch.full((P_PAT,), -1, dtype=torch.long).scatter_reduce(0, pi, torch.arange(n), "amax")
    two = ((last // T - first // T) <= 1).to(dev)
    assert int(two.sum()) > 50
    differ = int((g0.A != g1.A).any(1).sum())
    print(f"[steady] dA rows that differ between saved and recomputing: {differ} of {P_PAT} ({int((~two).sum())} span 3+ tiles)")
    assert torch.equal(g0.A[two], g1.A[two])
    assert rel(g0.A, g1.A) <= 1e-6


@pytest.mark.parametrize("L,want", [(100, "k_pair_bwd_duo<4, true>"), (200, "k_pair_bwd")])
def test_pair_head_backward_wide_lab_tables_many_tiles(ops, dev, L, want):
    """100 labs: k_pair_bwd_duo<4> (four lab tiles of dB in the back wave); 200 labs: k_pair_bwd, the fp32 kernel, whose
    workgroups walk 256-pair tiles (its grid, min(ceil(n / 256), 512), is read from the probe like the others)."""
    p = 0.2
    n, pi, li, deg, dpred = pair_bwd_case(ops, dev, L, want.split("<")[0])
    params = head_params(L)
    head = ops.Head(*[t.to(dev) for t in params])
    i32 = lambda t: t.to(torch.int32).to(dev)
    pid = torch.randperm(n, generator=torch.Generator().manual_seed(4)) + 777
    sel = deg[pi] >= 6
    _, ref = head_ref(params, pi, li, pid, p, dpred * sel)
    g = zero_grads(ops, head)
    _, recs = probed(ops, lambda: ops.pair_head_bwd(head, g, i32(pi), i32(li), i32(deg), 6, False, L, p, SEED, pid.to(dev),
                                                    dpred.to(dev)))
    sym, Rw, T, hist = regime(recs, want, n)
    if sym == "k_pair_bwd":
        assert T == 256
    print(f"[steady] {sym}: R = {Rw}, tiles per walker {hist}")
    check_grads(g, ref, sym)


def test_zz_worst_per_row_errors_of_the_dense_families():
    """Prints what the module docstring quotes (run last: the cases above fill the table)."""
    for family, err in sorted(WORST.items()):
        print(f"[steady] worst per-row error, {family}: {err:.3e}")
        assert err <= 2e-6
