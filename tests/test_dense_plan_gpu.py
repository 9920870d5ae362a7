"""The dense GEMMs at the shapes where their launch plan switches.

plan_wgrad, fwd_x6_rows, fwd_k256_rows, linear_fwd_launch and xcd_tile_map (csrc/gemm.hip) choose kernel, grid and the
block -> (tile, row set) map on the host.  The shapes here come from tests/dense_plan_ref.py, the plain-Python restatement
of that plan (tests/test_dense_plan_cpu.py holds it against the library and asserts what every shape is for): the direct /
split switch of the weight gradient at M = 256 | 257, the XCD remap with 2, 3, 4, 5 and 9 output tiles, ragged last stages,
more than one turn of the 4-stage ring, the forward switch at M = 512 | 513, three and more column slices, the widest N the
ABI accepts.  EVERY case asserts from the probe of its own launch that the restated symbol, grid and block ran.

References are fp64 on the host (dropout masks from tests/rng_ref.py through HostPro of tests/test_steady_state_gpu.py);
inputs are randn of a seeded generator, W scaled by K ** -0.5.  Bars, as max|err| / max|ref| over the tensor, are the ones
the project already holds these kernels to: weight gradient 1e-5, bias gradient 2e-6, forward 2e-6, epilogue statistics
1e-6 (against fp64 sums of the device output).  Every weight-gradient case runs twice and must give the same bits.
"""
import functools

import pytest
import torch

import dense_plan_ref as D
from test_steady_state_gpu import HostPro, _randn, launch_of, mm64, probed

pytestmark = pytest.mark.gpu

WORST = {}


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
    assert bool(torch.isfinite(a).all())
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def note(family, err, bar):
    WORST[family] = max(WORST.get(family, 0.0), err)
    print(f"[plan] {family}: {err:.3e} (bar {bar:.0e})")


def sid(s):
    return "x".join(map(str, s))


def ran_as_planned(recs, plan, M, prefix):
    """The one launch of the family in the probe records IS the restated plan's."""
    sym, m, grid, block = launch_of(recs, prefix)
    assert (sym, m, grid, block) == (plan.symbol, M, plan.grid, plan.block), \
        f"probe: {sym} M = {m} grid {grid} block {block}; plan: {plan.symbol} grid {plan.grid} block {plan.block}"
    print(f"[plan] {sid((plan.M, plan.N, plan.K))}: {sym} grid {grid} block {block}")


# ------------------------------------------------------------------------------------------ mmg_linear_wgrad
WG_PRO = dict(relu=True, p=0.2)                       # BatchNorm fold + ReLU + dropout in front of x


@functools.lru_cache(maxsize=4)
def wgrad_inputs(M, N, K):
    return _randn(3 * M + N, M, N), _randn(3 * M + K + 1, M, K), _randn(N + K, N, K), _randn(N + K + 1, N)


@functools.lru_cache(maxsize=None)
def wgrad_ref(M, N, K, pro):
    """-> (dy^T pro(x), column sums of dy) in fp64."""
    dy, x, _, _ = wgrad_inputs(M, N, K)
    xp = HostPro(K, **WG_PRO).apply(x) if pro else x.double()
    return dy.double().t() @ xp, dy.double().sum(0)


WG_VARIANTS = ("plain", "bias", "acc", "pro", "pro_acc", "defer")


def run_wgrad(ops, dev, M, N, K, variant):
    dy, x, out0, b0 = wgrad_inputs(M, N, K)
    dyd, xd = dy.to(dev), x.to(dev)
    pro = variant.startswith("pro")
    acc = variant.endswith("acc")
    hp = HostPro(K, **WG_PRO) if pro else None
    plan = D.plan_wgrad(M, N, K, pro)

    def call(defer=None):
        kw = dict(pro=hp.dev(ops, dev)) if pro else {}
        if acc:
            kw.update(out=out0.to(dev), accumulate=True, bias_out=b0.to(dev))
        if defer is not None:
            kw.update(defer=defer)
        return ops.linear_wgrad(dyd, xd, with_bias=variant != "plain", **kw)

    res, recs = probed(ops, call)
    ran_as_planned(recs, plan, M, "k_linear_wgrad")
    # the slab sum follows a split launch and only a split launch
    assert any("reduce_slabs" in r[0] for r in recs) == (not plan.direct), [r[0] for r in recs]
    dW, db = (res, None) if variant == "plain" else res
    again = call()
    assert torch.equal(dW, again if variant == "plain" else again[0]), "the same call twice: other bits"
    if db is not None:
        assert torch.equal(db, again[1])
    ref_w, ref_b = wgrad_ref(M, N, K, pro)
    if acc:
        ref_w, ref_b = ref_w + out0.double(), ref_b + b0.double()
    fam = "wgrad direct" if plan.direct else ("wgrad remap" if plan.remap else "wgrad split")
    e = rel(dW, ref_w)
    note(f"{fam} dW", e, 1e-5)
    assert e <= 1e-5, (plan, variant, e)
    if db is not None:
        eb = rel(db, ref_b)
        note(f"{fam} dbias", eb, 2e-6)
        assert eb <= 2e-6, (plan, variant, eb)
    if variant == "defer":
        jobs = []
        (gW, gb), recs = probed(ops, lambda: call(jobs))
        ran_as_planned(recs, plan, M, "k_linear_wgrad")
        assert len(jobs) == 1
        ops.wgrad_reduce_flush(jobs)
        assert not jobs and torch.equal(gW, dW) and torch.equal(gb, db)


# (the top decorator varies fastest: a shape's variants run back to back and share its cached inputs and references)
@pytest.mark.parametrize("variant", WG_VARIANTS)
@pytest.mark.parametrize("shape", D.wgrad_shapes(), ids=sid)
def test_weight_gradient_at_the_plan_switches(ops, dev, shape, variant):
    """plain; with the bias gradient; accumulating into a random out / bias_out (direct shapes: direct_accumulate == 2);
    BatchNorm fold + ReLU + dropout(0.2) prologue, also accumulating; deferred slab sum == the immediate call, bit for
    bit."""
    run_wgrad(ops, dev, *shape, variant)


# ------------------------------------------------------------------------------------------ mmg_linear_fwd
@functools.lru_cache(maxsize=4)
def fwd_inputs(M, N, K):
    return _randn(5 * M + K, M, K), _randn(N * K + 2, N, K) * K ** -0.5, _randn(N * K + 3, N), _randn(M + N, M, N)


@functools.lru_cache(maxsize=None)
def fwd_ref(M, N, K, pro):
    x, W, b, _ = fwd_inputs(M, N, K)
    return mm64(HostPro(K, True, 0.2).apply(x) if pro else x, W, b)


FWD_VARIANTS = ("plain", "pro", "acc", "w_kn", "stats")


def run_fwd(ops, dev, M, N, K, variant, slices=False):
    x, W, b, base = fwd_inputs(M, N, K)
    xd, Wd, bd = x.to(dev), W.to(dev), b.to(dev)
    pro, acc, stats = variant == "pro", variant == "acc", variant == "stats"
    plan = D.plan_fwd(M, N, K, pro=pro, acc=acc, stats=stats, p=0.2 if pro else 0.0)

    def call():
        if variant == "w_kn":
            return ops.linear_fwd(xd, Wd.t().contiguous(), bd, w_kn=True)
        return ops.linear_fwd(xd, Wd, bd, pro=HostPro(K, True, 0.2).dev(ops, dev) if pro else None,
                              out=base.to(dev) if acc else None, accumulate=acc, with_stats=stats)

    res, recs = probed(ops, call)
    ran_as_planned(recs, plan, M, "k_linear_")
    y, sums = res if stats else (res, None)
    ref = fwd_ref(M, N, K, pro)
    if acc:
        ref = ref + base.double()
    e = rel(y, ref)
    note(f"fwd {plan.family}", e, 2e-6)
    assert e <= 2e-6, (plan, variant, e)
    if variant in ("w_kn", "stats"):
        assert torch.equal(y, ops.linear_fwd(xd, Wd, bd)), f"{variant}: other bits than the plain launch"
    if stats:
        yd = y.double().cpu()
        e1, e2 = rel(sums[0], yd.sum(0)), rel(sums[1], (yd * yd).sum(0))
        note(f"fwd {plan.family} statistics", max(e1, e2), 1e-6)
        assert e1 <= 1e-6 and e2 <= 1e-6, (plan, e1, e2)
    if slices and variant == "plain":
        # a column's products do not depend on its slice: every slice == the single-slice launch of its W rows, the same
        # kernel instance with grid.x = 1 (no remap)
        for s in range(plan.n_slices):
            c0, c1 = s * plan.BN, (s + 1) * plan.BN
            if s == 0:
                ys, recs = probed(ops, lambda: ops.linear_fwd(xd, Wd[c0:c1], bd[c0:c1]))
                one = D.plan_fwd(M, plan.BN, K)
                ran_as_planned(recs, one, M, "k_linear_")
                assert one.symbol == plan.symbol and one.grid[0] == 1 and not one.remap
            else:
                ys = ops.linear_fwd(xd, Wd[c0:c1], bd[c0:c1])
            assert torch.equal(y[:, c0:c1], ys), f"slice {s} of {plan.n_slices} differs from its single-slice launch"
    return y


@pytest.mark.parametrize("variant", FWD_VARIANTS + ("l2",))
@pytest.mark.parametrize("M", [512, 513])
@pytest.mark.parametrize("K,N", D.FWD_SWITCH_KN)
def test_forward_on_both_sides_of_the_kernel_switch(ops, dev, K, N, M, variant):
    """M = 512: k_linear_small; M = 513: the split kernels with 17 row sets, the last tile of one row."""
    if variant != "l2":
        run_fwd(ops, dev, M, N, K, variant)
        return
    from mmgnn import _lib
    fused = bool(_lib.load().mmg_linear_fwd_supported(ops.EPI_L2, M, N, K))
    assert fused == (M > 512 and N in (64, 128) and K in (64, 128))
    x, W, b, _ = fwd_inputs(M, N, K)
    (out, rn), recs = probed(ops, lambda: ops.linear_l2norm_fwd(x.to(dev), W.to(dev), b.to(dev)))
    ran_as_planned(recs, D.plan_fwd(M, N, K, l2=fused), M, "k_linear_")
    z = fwd_ref(M, N, K, False)
    nrm = z.norm(dim=1).clamp(min=ops.L2_EPS)
    e = rel(out, z / nrm[:, None])
    note("fwd l2", e, 2e-6)
    assert e <= 2e-6, e
    e_rn = float(((rn.double().cpu() - 1 / nrm).abs() * nrm).max())
    assert e_rn <= 2e-6, e_rn


@pytest.mark.parametrize("variant", FWD_VARIANTS)
@pytest.mark.parametrize("shape", list(D.FWD_CASES), ids=sid)
def test_forward_with_three_and_more_column_slices(ops, dev, shape, variant):
    """Three to 63 column slices, with and without the remap, up to the widest N the ABI accepts; the plain case also
    holds every slice to the bits of its single-slice launch."""
    run_fwd(ops, dev, *shape, variant, slices=True)


def test_forward_refuses_what_lies_past_the_widest_output(ops, dev):
    from mmgnn import _lib
    x, W = torch.zeros(520, 128, device=dev), torch.zeros(4160, 128, device=dev)
    with pytest.raises(_lib.MmgError, match=r"rc=-1\).*unsupported"):
        ops.linear_fwd(x, W)


def test_report():
    for k in sorted(WORST):
        print(f"[plan] worst {k}: {WORST[k]:.3e}")
