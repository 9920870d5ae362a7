"""The rider of the encoder's third linear (mmg_linear_fwd_rider, ops.FwdRider, mmgnn.model.set_enc_tail_rider): the compact
tail of pass A -- affine_act_drop_rows + the L2 launch on the listed rows -- inside pass B's dense L2 launch of the same W.

The yardstick is the library's own separate launches; every comparison is on the bits (nothing is re-associated).

a. the entry point against the separate launches: dense x0 / rn, the rider's act / x0 / rn -- dense M where a workgroup walks
   one, two and three tiles (513: 17 tiles on 17 workgroups; 8,193: 257 tiles on 257; 16,389: 513 tiles on 512, so the rider's
   first tile lands on workgroup 1 as its SECOND tile and the others as first-and-only rider tiles behind one dense tile), list
   lengths around the tile size above the 512 rows from which the compact launch is the matrix-core kernel (513, 543, 544, 545),
   a list that holds row 0 and row M - 1, all M rows, p = 0.2 and 0.5, row offset 1000, the seed by value and by pointer.
b. lists of 0, 1, 31, 32, 33 rows and of 1.5 % of the rows: the dense launch alone (0), else the separate launches (the
   compact launch is then the fp32 kernel of the small tables, which the query leaves out): ops-level equality of what the
   model's two paths compute.
c. the support query, the refusals (nothing launched), the probe row.
e. the backward entry point (mmg_linear_bnbwd_rider, ops.BwdRider) against linear_l2bwd dense + linear_l2bwd compact +
   bn_bwd_stats_rows: dense dZ / dX and the next BatchNorm's sums, the rider's dZ3_A / dX_A and the sums of its listed rows --
   the same M and list lengths, with and without the next-BatchNorm epilogue on the dense part, a gradient with zeros,
   negatives and one infinity, a row whose norm was clamped at eps; k_partial_sum with two jobs against two launches.
d. captured training steps with the switch on and off: the same steps, one launch for three; 256-d, eval and lists of up to
   512 rows keep today's launches."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = N = 128
SEED = 0x1234_5678_9ABC
OFF = 1000
RIDER_FLAGS = 4 | 32 | 32768


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


def same(a, b):
    """bit for bit: an infinity or a NaN equals itself, +0 differs from -0"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Case:
    """Both passes' third linear on fixed inputs: B dense with its prologue, A on a row list with its own."""

    def __init__(self, ops, dev, M, n_sel, p=0.2, byptr=False, ends=False):
        gen = torch.Generator().manual_seed(M + n_sel + int(p * 100) + 7 * byptr)
        r = lambda *s: torch.randn(*s, generator=gen)                     # noqa: E731
        self.ops, self.M = ops, M
        self.W, self.b = (r(N, K) / K ** 0.5).to(dev), (0.1 * r(N)).to(dev)
        self.z2_b, self.z2_a = r(M, K).to(dev), r(M, K).to(dev)
        rows = torch.randperm(M, generator=gen)[:n_sel]
        if ends and n_sel >= 2:                  # row 0 and row M - 1 are listed
            rows = rows[(rows != 0) & (rows != M - 1)][: n_sel - 2]
            rows = torch.cat([torch.tensor([M - 1]), rows, torch.tensor([0])])
        self.rows = rows.to(dev)
        seed_dev = torch.tensor([SEED], dtype=torch.int64, device=dev) if byptr else None
        pro = lambda site: ops.Pro((1 + 0.1 * r(K)).to(dev), (0.1 * r(K)).to(dev), True, p,        # noqa: E731
                                   seed=0 if byptr else SEED, site=site, row_offset=OFF, seed_dev=seed_dev)
        self.pro_a, self.pro_b = pro(1), pro(3)

    def separate(self):
        o = self.ops
        act = o.affine_act_drop_rows(self.z2_a, self.pro_a, self.rows)
        x0_a, rn_a = o.linear_l2norm_fwd(act, self.W, self.b)
        x0_b, rn_b = o.linear_l2norm_fwd(self.z2_b, self.W, self.b, pro=self.pro_b)
        return x0_b, rn_b, act, x0_a, rn_a

    def ridden(self):
        o = self.ops
        rider = o.FwdRider()
        act, x0_a, rn_a = rider.park_rows(self.z2_a, self.pro_a, self.rows, self.W, self.b)
        x0_b, rn_b = o.linear_l2norm_fwd_rider(self.z2_b, self.W, self.b, self.pro_b, rider)
        rider.require_consumed()
        return x0_b, rn_b, act, x0_a, rn_a


NAMES = ("dense x0", "dense rn", "act_A", "x0_A", "rn_A")
CASES = [(M, n, 0.2, False, False) for M in (8193, 16389) for n in (513, 543, 544, 545)] + \
        [(M, 600, p, byptr, True) for M in (8193, 16389) for p in (0.2, 0.5) for byptr in (False, True)] + \
        [(513, 513, 0.2, False, False), (8193, 8193, 0.5, True, False), (16389, 16389, 0.2, False, False)]


@pytest.mark.parametrize("M,n_sel,p,byptr,ends", CASES)
def test_rider_against_the_separate_launches(ops, dev, M, n_sel, p, byptr, ends):
    c = Case(ops, dev, M, n_sel, p, byptr, ends)
    assert ops.linear_fwd_rider_supported(M, N, K, n_sel)
    if ends:
        assert int(c.rows[0]) == M - 1 and int(c.rows[-1]) == 0 and c.rows.unique().numel() == n_sel
    want = c.separate()
    assert all(torch.isfinite(t).all() for t in want)
    drop = float((want[2] == 0).float().mean())           # ReLU and dropout: between p and p + (1 - p) * ~0.6
    assert p < drop < p + (1 - p) * 0.7 and float(want[3].abs().max()) > 0
    got = c.ridden()
    for name, g, w in zip(NAMES, got, want):
        assert same(g, w), name
    again = c.ridden()                                     # the same call twice: the same bits
    for name, g, w in zip(NAMES, again, got):
        assert same(g, w), name


@pytest.mark.parametrize("M", [513, 8193, 16389])
@pytest.mark.parametrize("n_sel", [0, 1, 31, 32, 33, "1.5%"])
def test_short_lists_keep_the_separate_launches(ops, dev, M, n_sel):
    """b. what model._Run.enc_fwd does with these lists: no rider below 513 rows (the compact launch is then the fp32 kernel),
    and n_sel = 0 through the entry point is the dense launch alone."""
    n = max(2, int(0.015 * M)) if n_sel == "1.5%" else n_sel
    c = Case(ops, dev, M, n, ends=n_sel == "1.5%")
    assert ops.linear_fwd_rider_supported(M, N, K, n) == (n == 0)
    want = c.separate()
    if n:
        with pytest.raises(ValueError, match="no rider"):
            ops.FwdRider().park_rows(c.z2_a, c.pro_a, c.rows, c.W, c.b)
        return
    got = c.ridden()
    for name, g, w in zip(NAMES, got, want):
        assert same(g, w), name
    assert got[2].shape == (0, K) and got[3].shape == (0, N)


def test_support_query_refusals_and_the_probe_row(ops, dev):
    sup = ops.linear_fwd_rider_supported
    assert sup(513, 128, 128, 513) and sup(183400, 128, 128, 2750) and sup(183400, 128, 128, 0) and sup(600, 128, 128, 600)
    assert not sup(512, 128, 128, 0) and not sup(5000, 256, 256, 600) and not sup(5000, 64, 128, 600)
    assert not sup(5000, 128, 64, 600) and not sup(5000, 128, 128, 512) and not sup(5000, 128, 128, 5001)
    assert not sup(5000, 128, 128, -1)
    c = Case(ops, dev, 8193, 600)
    o = ops

    def call(x=None, W=None, b="same", pro="same", park=None):
        rider = o.FwdRider()
        act, x0, rn = rider.park_rows(*(park or (c.z2_a, c.pro_a, c.rows, c.W, c.b)))
        return rider, o.linear_l2norm_fwd_rider(c.z2_b if x is None else x, c.W if W is None else W, c.b if b == "same" else b,
                                                c.pro_b if pro == "same" else pro, rider)

    ops.probe_arm(64)
    try:
        with pytest.raises(RuntimeError, match="another W or bias"):
            call(W=c.W.clone())
        with pytest.raises(RuntimeError, match="another W or bias"):
            call(b=c.b.clone())
        with pytest.raises(RuntimeError, match="another W or bias"):
            call(b=None)
        with pytest.raises(RuntimeError, match="nothing is parked"):
            o.linear_l2norm_fwd_rider(c.z2_b, c.W, c.b, c.pro_b, o.FwdRider())
        with pytest.raises(Exception, match="needs a prologue"):            # an identity prologue is another kernel instance
            call(pro=o.Pro(None, None, False, 0.0))
        with pytest.raises(ValueError, match="another shape"):
            call(x=c.z2_b[:8000].contiguous())
        rider = o.FwdRider()
        rider.park_rows(c.z2_a, c.pro_a, c.rows, c.W, c.b)
        with pytest.raises(RuntimeError, match="already holds"):
            rider.park_rows(c.z2_a, c.pro_a, c.rows, c.W, c.b)
        with pytest.raises(RuntimeError, match="never launched"):
            rider.require_consumed()
        # the C entry point itself: a rider output that aliases the dense output, another W in the descriptor
        import ctypes as C
        out, rn = torch.empty(c.M, N, device=dev), torch.empty(c.M, device=dev)
        act, rn_a = torch.empty(600, K, device=dev), torch.empty(600, device=dev)
        epi = o.FwdEpiT(o.EPI_L2, rnorm=o._p(rn), eps=o.L2_EPS)
        rp = c.pro_a.c()

        def raw(W_r, y_r):
            epi_a = o.FwdEpiT(o.EPI_L2, rnorm=o._p(rn_a), eps=o.L2_EPS)
            o._call("mmg_linear_fwd_rider", c.z2_b, o._pro(c.pro_b), c.W, c.b, out, c.M, N, K, C.byref(epi), c.z2_a, C.byref(rp),
                    c.rows, 600, W_r, c.b, act, y_r, C.byref(epi_a))

        with pytest.raises(Exception, match="aliases"):
            raw(c.W, out[100:700])
        with pytest.raises(Exception, match="dense launch's W and bias"):
            raw(c.W.clone(), torch.empty(600, N, device=dev))
        torch.cuda.synchronize()
    finally:
        rows = ops.probe_read()
    assert [r for r in rows if r[1] == "linear_fwd"] == []
    ops.probe_arm(64)
    c.ridden()
    torch.cuda.synchronize()
    rows = [r for r in ops.probe_read() if r[1] == "linear_fwd"]
    assert [(r[2], r[3], r[4], r[5]) for r in rows] == [(8193, 128, 128, RIDER_FLAGS)]
    assert rows[0][6] == "k_linear_fwd_x6<128, 4, true, false, true, false, true>"


class BCase:
    """Both passes' L2 backward of the third linear: B dense, A compact on a row list, A's BatchNorm-backward statistics."""

    def __init__(self, ops, dev, M, n_sel, p=0.2, byptr=False, ends=False):
        gen = torch.Generator().manual_seed(3 * M + n_sel + int(p * 100) + 7 * byptr)
        r = lambda *s: torch.randn(*s, generator=gen)                     # noqa: E731
        self.ops, self.M, self.n = ops, M, n_sel
        self.W = (r(K, N) / K ** 0.5).to(dev)

        def normed(m):
            z = r(m, K)
            z[m // 3] = 0.0                                             # a row whose norm was clamped at eps
            rn = 1.0 / z.norm(dim=1).clamp_min(ops.L2_EPS)
            return (z * rn[:, None]).to(dev), rn.to(dev)

        self.x0_b, self.rn_b = normed(M)
        self.x0_a, self.rn_a = normed(n_sel) if n_sel else (torch.empty(0, K, device=dev), torch.empty(0, device=dev))

        def grad(m):
            g = r(m, K)
            g[torch.rand(m, K, generator=gen) < 0.1] = 0.0              # zeros and negatives
            return g.to(dev)

        self.g_b, self.g_a = grad(M), grad(n_sel)
        rows = torch.randperm(M, generator=gen)[:n_sel]
        if ends and n_sel >= 2:
            rows = rows[(rows != 0) & (rows != M - 1)][: n_sel - 2]
            rows = torch.cat([torch.tensor([M - 1]), rows, torch.tensor([0])])
        self.rows = rows.to(dev)
        self.z2_b, self.z2_a = r(M, N).to(dev), r(M, N).to(dev)
        seed_dev = torch.tensor([SEED], dtype=torch.int64, device=dev) if byptr else None

        def fold_pro(site):
            f = ops.BNFold((1 + 0.1 * r(N)).to(dev), (0.1 * r(N)).to(dev), (0.1 * r(N)).to(dev), (1 + 0.1 * r(N)).abs().to(dev),
                           M, True)
            return f, ops.Pro(f.scale, f.shift, True, p, seed=0 if byptr else SEED, site=site, row_offset=OFF, seed_dev=seed_dev)

        (self.f_a, self.pro_a), (self.f_b, self.pro_b) = fold_pro(1), fold_pro(3)

    def next_bn(self):
        return self.ops.NextBN(self.z2_b, self.pro_b, self.f_b)

    def separate(self, g_b, g_a, nbn):
        o = self.ops
        out_b = o.linear_l2bwd(g_b, self.x0_b, self.rn_b, self.W, next_bn=self.next_bn() if nbn else None)
        dz_a, dx_a = o.linear_l2bwd(g_a, self.x0_a, self.rn_a, self.W)
        sums_a = o.bn_bwd_stats_rows(dx_a, self.z2_a, self.rows, self.pro_a, self.f_a)
        return tuple(out_b) + (dz_a, dx_a, sums_a)

    def ridden(self, g_b, g_a, nbn, stats=True):
        o = self.ops
        rider = o.BwdRider()
        dz_a, dx_a, sums_a = rider.park(g_a, self.x0_a, self.rn_a, self.W, self.M,
                                        stats=(self.z2_a, self.rows, self.pro_a, self.f_a) if stats else None)
        out_b = o.linear_l2bwd(g_b, self.x0_b, self.rn_b, self.W, next_bn=self.next_bn() if nbn else None, rider=rider)
        rider.require_consumed()
        return tuple(out_b) + (dz_a, dx_a, sums_a)


def bsame(a, b):
    """same() for fp32 and fp64 tensors"""
    it = torch.int32 if a.dtype == torch.float32 else torch.int64
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def bnames(nbn):
    return ("dense dZ", "dense dX") + (("dense next-BatchNorm sums",) if nbn else ()) + ("dZ3_A", "dX_A", "sums_A")


BCASES = [(M, n, 0.2, False, False, nbn) for M in (8193, 16389) for n in (513, 543, 544, 545) for nbn in (True, False)] + \
         [(M, 600, p, byptr, True, True) for M in (8193, 16389) for p in (0.2, 0.5) for byptr in (False, True)] + \
         [(513, 513, 0.2, False, False, True), (8193, 8193, 0.5, True, False, False), (16389, 16389, 0.2, False, False, True)]


@pytest.mark.parametrize("M,n_sel,p,byptr,ends,nbn", BCASES)
def test_backward_rider_against_the_separate_launches(ops, dev, M, n_sel, p, byptr, ends, nbn):
    c = BCase(ops, dev, M, n_sel, p, byptr, ends)
    assert ops.linear_bnbwd_rider_supported(M, N, K, n_sel)
    want = c.separate(c.g_b, c.g_a, nbn)
    assert all(torch.isfinite(t).all() for t in want) and all(float(t.abs().max()) > 0 for t in want)
    got = c.ridden(c.g_b, c.g_a, nbn)
    for name, g, w in zip(bnames(nbn), got, want):
        assert bsame(g, w), name
    # one infinity in each gradient
    g_b, g_a = c.g_b.clone(), c.g_a.clone()
    g_b[M // 2, 5] = float("inf")
    g_a[n_sel // 2, 7] = float("-inf")
    want = c.separate(g_b, g_a, nbn)
    assert not torch.isfinite(want[1][M // 2]).all() and not torch.isfinite(want[-2][n_sel // 2]).all()
    for name, g, w in zip(bnames(nbn), c.ridden(g_b, g_a, nbn), want):
        assert bsame(g, w), name
    # without the statistics of the listed rows: the two L2 backwards alone
    got = c.ridden(c.g_b, c.g_a, nbn, stats=False)
    want = c.separate(c.g_b, c.g_a, nbn)
    assert got[-1] is None
    for name, g, w in zip(bnames(nbn)[:-1], got[:-1], want[:-1]):
        assert bsame(g, w), name


@pytest.mark.parametrize("M", [513, 8193, 16389])
@pytest.mark.parametrize("n_sel", [0, 1, 31, 32, 33, "1.5%"])
def test_backward_short_lists_keep_the_separate_launches(ops, dev, M, n_sel):
    n = max(2, int(0.015 * M)) if n_sel == "1.5%" else n_sel
    assert ops.linear_bnbwd_rider_supported(M, N, K, n) == (n == 0)
    c = BCase(ops, dev, M, n, ends=n_sel == "1.5%")
    if n:
        with pytest.raises(ValueError, match="no rider"):
            ops.BwdRider().park(c.g_a, c.x0_a, c.rn_a, c.W, M)
        return
    want = c.ops.linear_l2bwd(c.g_b, c.x0_b, c.rn_b, c.W, next_bn=c.next_bn())
    got = c.ridden(c.g_b, c.g_a, True)
    for name, g, w in zip(bnames(True)[:3], got[:3], want):
        assert bsame(g, w), name
    assert got[3].shape == (0, K) and got[4].shape == (0, N) and float(got[5].abs().max()) == 0.0


def test_backward_refusals_and_the_probe_row(ops, dev):
    sup = ops.linear_bnbwd_rider_supported
    assert sup(513, 128, 128, 513) and sup(183400, 128, 128, 2750) and sup(183400, 128, 128, 0)
    assert not sup(512, 128, 128, 0) and not sup(5000, 256, 256, 600) and not sup(5000, 64, 128, 600)
    assert not sup(5000, 128, 64, 600) and not sup(5000, 128, 128, 512) and not sup(5000, 128, 128, 5001)
    c = BCase(ops, dev, 8193, 600)
    o = ops
    ops.probe_arm(64)
    try:
        rider = o.BwdRider()
        rider.park(c.g_a, c.x0_a, c.rn_a, c.W, c.M)
        with pytest.raises(RuntimeError, match="another W"):
            o.linear_l2bwd(c.g_b, c.x0_b, c.rn_b, c.W.clone(), rider=rider)
        with pytest.raises(ValueError, match="excludes the fused weight gradient"):
            o.linear_l2bwd(c.g_b, c.x0_b, c.rn_b, c.W, wgrad=o.FusedWgrad(c.z2_b, c.pro_b), rider=rider)
        with pytest.raises(ValueError, match="another size"):
            o.linear_l2bwd(c.g_b[:8000].contiguous(), c.x0_b[:8000].contiguous(), c.rn_b[:8000].contiguous(), c.W, rider=rider)
        with pytest.raises(RuntimeError, match="already holds"):
            rider.park(c.g_a, c.x0_a, c.rn_a, c.W, c.M)
        with pytest.raises(RuntimeError, match="never launched"):
            rider.require_consumed()
        with pytest.raises(RuntimeError, match="nothing is parked"):
            o.linear_l2bwd(c.g_b, c.x0_b, c.rn_b, c.W, rider=o.BwdRider())
        # the C entry point itself: a rider output that aliases the dense dX, another W in the descriptor, another mode
        import ctypes as C
        dz, dx = torch.empty(c.M, K, device=dev), torch.empty(c.M, N, device=dev)
        dz_a = torch.empty(600, K, device=dev)

        def raw(W_r, dx_r, mode_a=o.BNBWD_L2):
            d = lambda mode, g, y, rn: o.BnBwdT(mode, o._p(g), None, None, 0, o._p(y), None, None, None, None, None, 1.0,      # noqa: E731
                                                None, None, o._p(rn), o.L2_EPS)
            db, da = d(o.BNBWD_L2, c.g_b, c.x0_b, c.rn_b), d(mode_a, c.g_a, c.x0_a, c.rn_a)
            o._call("mmg_linear_bnbwd_rider", C.byref(db), c.W, dz, dx, c.M, N, K, None, C.byref(da), W_r, dz_a, dx_r, 600, None,
                    None)

        with pytest.raises(Exception, match="aliases"):
            raw(c.W, dx[100:700])
        with pytest.raises(Exception, match="dense launch's W"):
            raw(c.W.clone(), torch.empty(600, N, device=dev))
        with pytest.raises(Exception, match="MMG_BNBWD_L2"):
            raw(c.W, torch.empty(600, N, device=dev), mode_a=o.BNBWD_BN)
        # the listed rows' statistics in the workspace that holds the next BatchNorm's partial rows
        nbt, _ = o._next_bn(c.next_bn(), c.M, N)
        d = lambda g, y, rn: o.BnBwdT(o.BNBWD_L2, o._p(g), None, None, 0, o._p(y), None, None, None, None, None, 1.0,      # noqa: E731
                                      None, None, o._p(rn), o.L2_EPS)
        db, da, pc = d(c.g_b, c.x0_b, c.rn_b), d(c.g_a, c.x0_a, c.rn_a), c.pro_a.c()
        sums_a = torch.empty(2, N, dtype=torch.float64, device=dev)
        nbt_a = o.NextBnT(o._p(c.z2_a), C.pointer(pc), o._p(c.f_a.mean), o._p(c.f_a.rstd), o._p(sums_a, torch.float64), 0, nbt.ws,
                          nbt.ws_bytes)
        with pytest.raises(Exception, match="share the next BatchNorm's workspace"):
            o._call("mmg_linear_bnbwd_rider", C.byref(db), c.W, dz, dx, c.M, N, K, C.byref(nbt), C.byref(da), c.W, dz_a,
                    torch.empty(600, N, device=dev), 600, c.rows, C.byref(nbt_a))
        torch.cuda.synchronize()
    finally:
        rows = ops.probe_read()
    assert [r for r in rows if r[1] == "linear_fwd"] == []
    for nbn, flags, sym in ((True, 64 | 512 | 32768, "k_linear_bnbwd_x6<128, 4, 1, true, false, 0, true>"),
                            (False, 64 | 32768, "k_linear_bnbwd_x6<128, 4, 1, false, false, 0, true>")):
        ops.probe_arm(64)
        c.ridden(c.g_b, c.g_a, nbn)
        torch.cuda.synchronize()
        rows = [r for r in ops.probe_read() if r[1] == "linear_fwd"]
        assert [(r[2], r[3], r[4], r[5], r[6]) for r in rows] == [(8193, 128, 128, flags, sym)]


def test_partial_sum_with_two_jobs_against_two_launches(dev):
    """k_partial_sum_jobs (job = blockIdx.y) against one k_partial_sum launch per job: 512 partial rows of 256 sums (a
    next-BatchNorm epilogue's) with an `add`, and 76 rows (the listed rows' blocks) without; and the jobs swapped."""
    import ctypes as C
    from mmgnn import _lib
    lib = _lib.load()

    class Job(C.Structure):
        _fields_ = [("partial", C.c_void_p), ("out", C.c_void_p), ("n", C.c_int), ("n_rows", C.c_int), ("add", C.c_void_p)]

    lib.mmg_partial_sum_jobs.argtypes = [C.POINTER(Job), C.POINTER(Job), C.c_void_p]
    lib.mmg_partial_sum_add.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    gen = torch.Generator().manual_seed(5)
    pa = (torch.randn(512, 256, generator=gen, dtype=torch.float64) * 1e3).to(dev)
    pb = torch.randn(76, 256, generator=gen, dtype=torch.float64).to(dev)
    add = torch.randn(256, generator=gen, dtype=torch.float64).to(dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    want_a, want_b = torch.empty(256, dtype=torch.float64, device=dev), torch.empty(256, dtype=torch.float64, device=dev)
    assert lib.mmg_partial_sum_add(pa.data_ptr(), want_a.data_ptr(), 256, 512, add.data_ptr(), st) == 0
    assert lib.mmg_partial_sum_add(pb.data_ptr(), want_b.data_ptr(), 256, 76, None, st) == 0
    for swap in (False, True):
        got_a, got_b = torch.full_like(want_a, float("nan")), torch.full_like(want_b, float("nan"))
        ja = Job(pa.data_ptr(), got_a.data_ptr(), 256, 512, add.data_ptr())
        jb = Job(pb.data_ptr(), got_b.data_ptr(), 256, 76, None)
        first, second = (jb, ja) if swap else (ja, jb)
        assert lib.mmg_partial_sum_jobs(C.byref(first), C.byref(second), st) == 0
        torch.cuda.synchronize()
        assert bsame(got_a, want_a) and bsame(got_b, want_b)
    assert float((want_a - (pa.sum(0) + add)).abs().max()) < 1e-7 and float((want_b - pb.sum(0)).abs().max()) < 1e-10


TAIL_CALLS = ("mmg_linear_fwd_rider", "mmg_affine_act_drop_rows", "mmg_linear_bnbwd_rider", "mmg_bn_bwd_stats_rows")


def _steps(dev, hidden, n_steps, thr=None, train=True):
    """n_steps captured training steps (or one eval prediction) per setting of set_enc_tail_rider (on, off) on
    synth.make_graph(1) -- (1834, 50, 114, 100) -- with the tabular head's degree threshold at thr
    -> [(losses, pred, state, gradients, which of TAIL_CALLS were made)]"""
    import mmgnn  # noqa: F401
    import mmgnn.model as mm
    from mmgnn import ops as o
    from mmgnn.data import build_plan
    from mmgnn.model import build_model
    from mmgnn.optim import Adam
    from mmgnn.synth import make_graph
    from mmgnn.train import PiecewiseGraphedTrainStep
    cfg = {"model": {"architecture": "RGCN", "hidden_dim": hidden, "num_layers": 2, "dropout": 0.2, "use_batch_norm": True,
                     "activation": "relu"}}
    LAB = ("patient", "has_lab", "lab")
    res, calls, real = [], [], o._call

    def counted(name, *a, **kw):
        if name in TAIL_CALLS:
            calls.append(name)
        return real(name, *a, **kw)

    o._call = counted
    try:
        for flag in (True, False):
            mm.set_enc_tail_rider(flag)
            g = make_graph(1, seed=0, device=dev)
            torch.manual_seed(42)
            model = build_model(cfg, (g.node_types, g.edge_types), None).to(dev)
            model._init_embeddings(g)
            if thr is not None:
                model.degree_threshold = thr
            ei = g[LAB].edge_index
            E = ei.shape[1]
            tr = torch.randperm(E, generator=torch.Generator(device=dev).manual_seed(42), device=dev)[: int(0.7 * E)].sort().values
            pi, li = ei[0][tr].contiguous(), ei[1][tr].contiguous()
            n_before = len(calls)
            if not train:
                model.eval()
                with torch.no_grad():
                    pred = model.predict_lab_values(g, pi, li)
                res.append(([0.0], pred.clone(), {}, {}, calls[n_before:]))
                continue
            y = g[LAB].edge_attr[tr].squeeze(-1).contiguous()
            sup = torch.rand(tr.numel(), generator=torch.Generator(device=dev).manual_seed(1234), device=dev) < 0.2
            wlab = torch.ones(int(g["lab"].num_nodes), device=dev)
            opt = Adam([q for k, q in model.named_parameters() if not k.startswith("embeddings.")], lr=1e-2)
            step = PiecewiseGraphedTrainStep(model, build_plan(g, dev, use_cache=False), pi, li, y, wlab, opt, sup, None)
            losses = [float(step.step()) for _ in range(n_steps)]
            grads = {k: q.grad.clone() for k, q in model.named_parameters() if q.grad is not None}
            res.append((losses, step.pred.clone(), {k: v.clone() for k, v in model.state_dict().items()}, grads,
                        calls[n_before:]))
    finally:
        mm.set_enc_tail_rider(True)
        o._call = real
    return res


def _same_steps(a, b):
    assert a[0] == b[0] and np.isfinite(a[0]).all() and same(a[1], b[1])
    assert set(a[2]) == set(b[2]) and set(a[3]) == set(b[3])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    for k in a[3]:
        assert same(a[3][k], b[3][k]), k


def test_graphed_training_steps_with_and_without_the_rider(dev):
    """d. two captured training steps, 128-d, the degree threshold raised to 30 so that the tabular head's list is longer
    than 512 rows: loss, pred, every parameter, buffer and gradient; with the switch on a recorded forward makes ONE rider
    call where it made affine_act_drop_rows (+ two L2 launches) before, and a recorded backward ONE where it made two
    linear_l2bwd calls and bn_bwd_stats_rows (five launches for nine)."""
    import mmgnn.model as mm
    assert mm.ENC_TAIL_RIDER is True
    on, off = _steps(dev, 128, 2, thr=30)
    assert len(on[4]) >= 2 and set(on[4]) == {"mmg_linear_fwd_rider", "mmg_linear_bnbwd_rider"}
    assert sorted(off[4]) == sorted({"mmg_linear_fwd_rider": "mmg_affine_act_drop_rows",
                                     "mmg_linear_bnbwd_rider": "mmg_bn_bwd_stats_rows"}[c] for c in on[4])
    _same_steps(on, off)
    assert mm.ENC_TAIL_RIDER is True


@pytest.mark.parametrize("what", ["short-list", "d256", "eval"])
def test_shapes_without_the_rider_take_the_launches_they_took(dev, what):
    """d. the model's own threshold (a list of ~27 rows), 256-d and eval mode: no rider call whatever the switch says."""
    hidden, thr, train = (256, 30, True) if what == "d256" else (128, None if what == "short-list" else 30, what != "eval")
    on, off = _steps(dev, hidden, 1, thr=thr, train=train)
    assert not [c for c in on[4] + off[4] if c.endswith("_rider")] and on[4] == off[4]
    _same_steps(on, off)
