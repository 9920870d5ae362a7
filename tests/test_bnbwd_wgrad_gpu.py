"""The weight gradient inside the BatchNorm-backward data-gradient GEMMs (mmg_linear_bnbwd with a mmg_bnbwd_wgrad_t, every
mode) against the plain GEMM followed by mmg_linear_wgrad.

dZ, dX and d beta / d gamma bit for bit; dW and db bit for bit what mmg_linear_wgrad computes (the fused kernel takes
its sums over the same row sets in the same order), and within the bars of test_ops_gpu.py::test_linear_wgrad_shapes
against fp64; the next BatchNorm's statistics (always the separate pass here) within fp64 re-association."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fixtures as fx
from oracle import model as om
from oracle import train as ot


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


def _bn(ops, dev, gen, M, K, p, site):
    y = (torch.randn(M, K, generator=gen) * 1.5 + 0.2).to(dev)
    gamma, beta = (torch.rand(K, generator=gen) + 0.5).to(dev), (torch.randn(K, generator=gen) * 0.2).to(dev)
    fold = ops.bn_finalize(ops.col_reduce2(y), M, gamma, beta, None, None, True)
    return y, ops.Pro(fold.scale, fold.shift, True, p, seed=9, site=site, row_offset=10), fold


def _problem(ops, dev, mode, M, p, seed):
    """-> run(next_bn, wgrad) calling the mode's entry point on fixed inputs (returns what the ops function returns)."""
    gen = torch.Generator().manual_seed(seed)
    K = N = 128
    W = (torch.randn(K, N, generator=gen) / K ** 0.5).to(dev)
    if mode == 1:
        z = torch.randn(M, K, generator=gen)
        z[min(7, M - 1)] = 0.0
        out, rn = ops.l2norm_fwd(z.to(dev))
        g = torch.randn(M, K, generator=gen).to(dev)
        run = lambda nb, fw, dbg: ops.linear_l2bwd(g, out, rn, W, next_bn=nb, wgrad=fw)      # noqa: E731
        run.W = W
        return run
    y, pro, fold = _bn(ops, dev, gen, M, K, p, site=3)
    if mode == 0:
        g = torch.randn(M, K, generator=gen).to(dev)
        sums = ops.bn_bwd_stats(g, y, pro, fold)
        run = lambda nb, fw, dbg: ops.linear_bnbwd(g, y, pro, fold, W, sums, M, dbg[0], dbg[1], next_bn=nb, wgrad=fw)  # noqa: E731
        run.W = W
        return run
    if mode == 2:
        g, g2 = torch.randn(M, K, generator=gen).to(dev), torch.randn(M, K, generator=gen).to(dev)
        pro2 = ops.Pro(fold.scale, fold.shift, True, p, seed=9, site=5, row_offset=10)
        sums = ops.bn_bwd_stats2(g, g2, y, pro, pro2, fold)
        run = lambda nb, fw, dbg: ops.linear_bnbwd2(g, g2, y, pro, pro2, fold, W, sums, M, dbg[0], dbg[1], wgrad=fw)  # noqa: E731
        run.W = W
        return run
    rows = torch.randperm(M, generator=gen)[:max(1, M // 30)].sort().values
    rows[-1] = M - 1                                                     # a row of the tail tile
    rows = rows.unique().to(dev)
    g_rows = torch.randn(rows.numel(), K, generator=gen).to(dev)
    row_pos = torch.full((M,), -1, dtype=torch.int32, device=dev)
    row_pos[rows] = torch.arange(rows.numel(), dtype=torch.int32, device=dev)
    sums = ops.bn_bwd_stats_rows(g_rows, y, rows, pro, fold)
    run = lambda nb, fw, dbg: ops.linear_bnbwd_rows(g_rows, row_pos, y, pro, fold, W, sums, M, dbg[0], dbg[1],  # noqa: E731
                                                    next_bn=nb, wgrad=fw)
    run.W = W
    return run


def same_dx(mode, dx_fused, dx_plain, dz, W, ops):
    """dX of the fused launch against the plain one: bit for bit, except MODE 1 (the L2 backward), whose plain instance
    rounds its products differently from mmg_linear_fwd by an ulp (test_ops_gpu.py holds it to 2e-6); the fused one
    equals mmg_linear_fwd(dz) there."""
    if mode != 1:
        return torch.equal(dx_fused, dx_plain)
    return rel(dx_fused, dx_plain) <= 2e-6 and torch.equal(dx_fused, ops.linear_fwd(dz, W, w_kn=True))


def db_err(db, dz):
    """error of a column sum of dz against fp64, relative to the column's sum of magnitudes (the BatchNorm backward makes
    the column sums of dz nearly cancel, so a bar relative to the sums themselves would measure the cancellation)"""
    dz = dz.double().cpu()
    return float(((db.double().cpu() - dz.sum(0)).abs() / dz.abs().sum(0).clamp_min(1e-30)).max())


def _x(ops, dev, M, with_pro, p, seed):
    gen = torch.Generator().manual_seed(seed + 1)
    x = (torch.randn(M, 128, generator=gen) * 1.3 + 0.1).to(dev)
    if not with_pro:
        return x, None, x
    sc, sh = (torch.rand(128, generator=gen) + 0.5).to(dev), (torch.randn(128, generator=gen) * 0.3).to(dev)
    pro = ops.Pro(sc, sh, True, p, seed=21, site=6, row_offset=33)
    return x, pro, ops.affine_act_drop(x, pro)


@pytest.mark.parametrize("M", [513, 600, 1001, 5003, 183400])
@pytest.mark.parametrize("with_pro", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_fused_weight_gradient_matches_the_two_kernels(ops, dev, mode, with_pro, M):
    p = 0.3 if with_pro else 0.0
    seed = 1000 * mode + M + with_pro
    run = _problem(ops, dev, mode, M, p, seed)
    x, xpro, xp = _x(ops, dev, M, with_pro, 0.25, seed)
    assert ops.linear_bnbwd_wgrad_supported(M, 128, 128)
    d0, d1 = torch.zeros(2, 128, device=dev), torch.zeros(2, 128, device=dev)
    dz0, dx0 = run(None, None, d0)
    dW0, db0 = ops.linear_wgrad(dz0, x, xpro, with_bias=True)
    fw = ops.FusedWgrad(x, xpro, with_bias=True, keep_dz=True)
    dz1, dx1 = run(None, fw, d1)
    assert torch.equal(dz1, dz0) and same_dx(mode, dx1, dx0, dz0, run.W, ops) and torch.equal(d1, d0)
    ref = dz0.double().t() @ xp.double()
    assert rel(fw.dW, ref) <= 1e-5 and db_err(fw.db, dz0) <= 2e-6
    assert torch.equal(fw.dW, dW0) and torch.equal(fw.db, db0)          # the separate kernel's bits
    # dz not written, the same dX and weight gradient; the same call twice: the same bits
    fw2 = ops.FusedWgrad(x, xpro, with_bias=True, keep_dz=False)
    dz2, dx2 = run(None, fw2, d1)
    assert dz2 is None and torch.equal(dx2, dx1)
    assert torch.equal(fw2.dW, fw.dW) and torch.equal(fw2.db, fw.db)
    # accumulate, deferred to the grouped slab sum
    jobs = []
    acc_w, acc_b = fw.dW.clone(), fw.db.clone()
    fw3 = ops.FusedWgrad(x, xpro, out=acc_w, accumulate=True, with_bias=True, bias_out=acc_b, defer=jobs, keep_dz=False)
    run(None, fw3, d1)
    assert len(jobs) == 1
    ops.wgrad_reduce_flush(jobs)
    assert fw3.dW is acc_w and fw3.db is acc_b
    assert rel(acc_w, 2 * ref) <= 1e-5 and db_err(acc_b, 2 * dz0) <= 2e-6
    jobs2 = []
    acc_w2, acc_b2 = ops.linear_wgrad(dz0, x, xpro, out=dW0.clone(), accumulate=True, with_bias=True, bias_out=db0.clone(),
                                      defer=jobs2)
    ops.wgrad_reduce_flush(jobs2)
    assert torch.equal(acc_w, acc_w2) and torch.equal(acc_b, acc_b2)
    # no bias slot
    fw4 = ops.FusedWgrad(x, xpro, keep_dz=False)
    run(None, fw4, d1)
    assert torch.equal(fw4.dW, fw.dW) and fw4.db is None


@pytest.mark.parametrize("mode", [0, 1, 3])
@pytest.mark.parametrize("M", [1001, 5003])
def test_fused_weight_gradient_with_next_bn_statistics(ops, dev, mode, M):
    """next_bn with the fused weight gradient: the statistics come from the separate pass over dX (the fused kernel has
    no statistics epilogue), so they equal mmg_bn_bwd_stats of dX and the NBN epilogue's up to fp64 re-association."""
    seed = 77 * mode + M
    run = _problem(ops, dev, mode, M, 0.3, seed)
    x, xpro, xp = _x(ops, dev, M, True, 0.25, seed)
    gen = torch.Generator().manual_seed(seed + 5)
    yb, pro_b, fold_b = _bn(ops, dev, gen, M, 128, 0.3, site=41)
    d0, d1 = torch.zeros(2, 128, device=dev), torch.zeros(2, 128, device=dev)
    dz0, dx0, s0 = run(ops.NextBN(yb, pro_b, fold_b), None, d0)
    fw = ops.FusedWgrad(x, xpro, with_bias=True, keep_dz=False)
    dz1, dx1, s1 = run(ops.NextBN(yb, pro_b, fold_b), fw, d1)
    assert dz1 is None and same_dx(mode, dx1, dx0, dz0, run.W, ops) and torch.equal(d1, d0)
    assert rel(s1[0], s0[0]) <= 1e-6 and rel(s1[1], s0[1]) <= 1e-6
    want = ops.bn_bwd_stats(dx1, yb, pro_b, fold_b)
    assert rel(s1[0], want[0]) <= 1e-12 and rel(s1[1], want[1]) <= 1e-12
    assert rel(fw.dW, dz0.double().t() @ xp.double()) <= 1e-5
    dW0, db0 = ops.linear_wgrad(dz0, x, xpro, with_bias=True)
    assert torch.equal(fw.dW, dW0) and torch.equal(fw.db, db0)


def test_fused_weight_gradient_support(ops, dev):
    """K = N = 128 and the data-gradient GEMM's own M > 512 only: smaller M (a tile or less, below 512 rows) and other
    widths keep the two kernels."""
    assert not ops.linear_bnbwd_wgrad_supported(20, 128, 128) and not ops.linear_bnbwd_wgrad_supported(512, 128, 128)
    assert not ops.linear_bnbwd_wgrad_supported(5000, 64, 128) and not ops.linear_bnbwd_wgrad_supported(5000, 128, 64)
    assert ops.linear_bnbwd_wgrad_supported(513, 128, 128)
    with pytest.raises(Exception):
        x = torch.zeros(300, 128, device=dev)
        ops.linear_l2bwd(x, x, torch.ones(300, device=dev), torch.zeros(128, 128, device=dev), wgrad=ops.FusedWgrad(x))


def _config(hidden=128, dropout=0.2):
    return {"model": {"architecture": "RGCN", "hidden_dim": hidden, "num_layers": 2, "dropout": dropout,
                      "use_batch_norm": True, "activation": "relu"}}


def test_graphed_training_step_fused_against_separate_weight_gradients(dev, monkeypatch):
    """mmgnn.model.FUSED_WGRAD: captured training steps with the weight gradients inside the BatchNorm-backward GEMMs and
    with the separate kernels are the SAME steps: losses, predictions and every parameter / buffer after two Adam steps
    bit for bit (the fused sums are the separate kernels' sums)."""
    import mmgnn  # noqa: F401
    import mmgnn.model as mm
    from mmgnn.data import build_plan
    from mmgnn.model import build_model
    from mmgnn.optim import Adam
    from mmgnn.train import PiecewiseGraphedTrainStep
    n = (1500, 20, 25, 18)
    cfg = _config()
    g0 = fx.graph_from_frames(fx.det_frames(*n))
    gv = om.GraphView(g0)
    sd = fx.det_state(gv.num_nodes, 128)
    ei, ea = g0["patient", "has_lab", "lab"].edge_index, g0["patient", "has_lab", "lab"].edge_attr
    tr, _, _ = ot.edge_splits(ei.shape[1])
    pi, li, y = ei[0][tr].to(dev), ei[1][tr].to(dev), ea[tr].squeeze(-1).to(dev)
    w = ot.lab_weights(ei[1][tr], ea[tr].squeeze(-1), gv.num_nodes["lab"]).to(dev)
    sup = (torch.rand(int(tr.sum()), generator=torch.Generator().manual_seed(3)) < 0.2).to(dev)
    res = []
    for flag in (False, True):
        monkeypatch.setattr(mm, "FUSED_WGRAD", flag)
        torch.manual_seed(99)
        g = fx.graph_from_frames(fx.det_frames(*n)).to(dev)
        model = build_model(cfg, (g.node_types, g.edge_types), None).to(dev)
        model._init_embeddings(g)
        model.load_state_dict(sd)
        opt = Adam([q for k, q in model.named_parameters() if not k.startswith("embeddings.")], lr=1e-2)
        step = PiecewiseGraphedTrainStep(model, build_plan(g, dev, use_cache=False), pi, li, y, w, opt, sup, None)
        losses = [float(step.step()) for _ in range(2)]
        res.append((losses, step.pred.clone(), {k: v.clone() for k, v in model.state_dict().items()}))
    (l0, p0, s0), (l1, p1, s1) = res
    assert l0 == l1 and torch.equal(p0, p1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
