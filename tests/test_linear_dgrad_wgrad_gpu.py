"""mmg_linear_dgrad_wgrad -- the data gradient and the weight gradient of a pair head's first layer in ONE launch --
against the two calls it replaces, ops.linear_fwd(dA, W, w_kn=True[, next_bn=...]) and ops.linear_wgrad(dA, X, pro): gP and
dW bit for bit, the next BatchNorm's statistics by the bar of tests/test_ops_gpu.py (_stats_close: relative 1e-6 against
ops.bn_bwd_stats over the finished output) and bitwise repeatable; accumulation; the refusals; captured training steps
with and without it.

Shapes (dA [M, 64], W [64, 128], X [M, 128]; 32-row stages dealt round-robin over plan_wgrad(M, 64, 128).n_split
workgroups): M = 513 -> 17 stages over 17 workgroups, the last of one row; 1,056 -> 33 stages, one per workgroup;
16,389 -> 513 stages over 171 workgroups: three per workgroup (the peeled pair, then a loop pass whose second tile lies
past the end), a short (5-row) last tile; 49,157 -> 1,537 stages over 220 workgroups: seven per workgroup (six for the
last three), so the loop runs three times and both register slots and both LDS buffers wrap, a 5-row last tile."""
import pytest
import torch

pytestmark = pytest.mark.gpu

K, N = 64, 128


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
    """bit for bit (NaN payloads and signed zeros included)"""
    view = {torch.float32: torch.int32, torch.float64: torch.int64}[a.dtype]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _stats_close(ops, got, out, y, pro, fold, bar=1e-6):
    """tests/test_ops_gpu.py::_stats_close; a column that holds the non-finite value of X must be non-finite in the same
    way in both (its position and kind), the bar holds over the other columns."""
    want = ops.bn_bwd_stats(out, y, pro, fold)          # the separate pass (fp64 per element) over the finished output
    fin = torch.isfinite(want)
    assert torch.equal(torch.isfinite(got), fin)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got[~fin & ~torch.isnan(want)], want[~fin & ~torch.isnan(want)])
    z = torch.zeros((), dtype=got.dtype, device=got.device)
    g, w = torch.where(fin, got, z), torch.where(fin, want, z)
    r0, r1 = rel(g[0], w[0]), rel(g[1], w[1])
    print(f"next-BN statistics vs bn_bwd_stats: rel {r0:.3e} {r1:.3e}")
    assert r0 <= bar and r1 <= bar, (r0, r1)


def _inputs(ops, dev, M, seed, specials):
    """dA with exact zeros; X ~45 % negative behind the affine (the ReLU gate) with exact zeros and, with `specials`, one
    infinity; the BatchNorm 'below' (fold from the finite X, as a step would have it)."""
    gen = torch.Generator().manual_seed(seed)
    dA = torch.randn(M, K, generator=gen)
    dA[torch.rand(M, K, generator=gen) < 0.05] = 0.0
    W = torch.randn(K, N, generator=gen) / K ** 0.5
    X = torch.randn(M, N, generator=gen) * 1.5 + 0.2
    X[torch.rand(M, N, generator=gen) < 0.05] = 0.0
    gamma, beta = torch.rand(N, generator=gen) + 0.5, torch.randn(N, generator=gen) * 0.2
    dA, W, X, gamma, beta = (t.to(dev) for t in (dA, W, X, gamma, beta))
    fold = ops.bn_finalize(ops.col_reduce2(X), M, gamma, beta, None, None, True)
    if specials:
        X[M // 2, 17] = float("inf")
    return dA, W, X, fold


CASES = [(M, epi, pro, M in (513, 16389)) for M in (513, 1056, 16389, 49157)
         for epi, pro in ((True, True), (False, True), (False, False))]


@pytest.mark.parametrize("M, epi, with_pro, specials", CASES)
def test_fused_launch_is_the_two_launches(ops, dev, M, epi, with_pro, specials):
    """gP and dW bit for bit; the statistics to the project's bar and the same bits on a second call; accumulate."""
    dA, W, X, fold = _inputs(ops, dev, M, 11 * M + 2 * int(epi) + int(with_pro), specials)
    pro = ops.Pro(fold.scale, fold.shift, True) if with_pro else None
    assert ops.linear_dgrad_wgrad_supported(M, N, K)
    nbn = (lambda: ops.NextBN(X, pro, fold)) if epi else (lambda: None)
    ref = ops.linear_fwd(dA, W, w_kn=True, next_bn=nbn())
    gP_ref = ref[0] if epi else ref
    dW_ref = ops.linear_wgrad(dA, X, pro)
    fw = ops.FusedWgrad(X, pro=pro)
    got = ops.linear_dgrad_wgrad(dA, W, fw, next_bn=nbn())
    gP = got[0] if epi else got
    assert same(gP, gP_ref), "gP"
    assert same(fw.dW, dW_ref), "dW"
    assert tuple(fw.dW.shape) == (K, N)
    if not specials:
        assert bool(torch.isfinite(gP).all()) and bool(torch.isfinite(fw.dW).all())
    if epi:
        _stats_close(ops, got[1], gP, X, pro, fold)
        print(f"fused vs linear_fwd epilogue statistics: rel {rel(torch.nan_to_num(got[1], 0, 0, 0), torch.nan_to_num(ref[1], 0, 0, 0)):.3e}")
        fw2 = ops.FusedWgrad(X, pro=pro)
        again = ops.linear_dgrad_wgrad(dA, W, fw2, next_bn=nbn())
        assert same(again[1], got[1]) and same(again[0], gP) and same(fw2.dW, fw.dW)      # fixed summation order
    # accumulate into an existing dW: bitwise the separate call
    base = torch.randn(K, N, generator=torch.Generator().manual_seed(M)).to(dev)
    acc_ref, acc = base.clone(), base.clone()
    ops.linear_wgrad(dA, X, pro, out=acc_ref, accumulate=True)
    ops.linear_dgrad_wgrad(dA, W, ops.FusedWgrad(X, pro=pro, out=acc, accumulate=True))
    assert same(acc, acc_ref) and not same(acc, base)
    # deferred slab sum: the grouped reduce finishes the same gradient
    jobs, dfw = [], None
    dfw = ops.FusedWgrad(X, pro=pro, defer=jobs)
    ops.linear_dgrad_wgrad(dA, W, dfw)
    assert len(jobs) == 1
    ops.wgrad_reduce_flush(jobs)
    assert same(dfw.dW, dW_ref)


def test_refusals_launch_nothing_and_write_nothing(ops, dev):
    """M = 512, output width 256, dY width 128, drop_p > 0 and wg->X != next->y: MMG_E_ARG, no launch, outputs untouched."""
    from mmgnn import _lib
    import ctypes as C
    M = 600
    dA, W, X, fold = _inputs(ops, dev, M, 5, False)
    pro = ops.Pro(fold.scale, fold.shift, True)
    sup = ops.linear_dgrad_wgrad_supported
    assert sup(513, 128, 64) and not sup(512, 128, 64) and not sup(600, 256, 64) and not sup(600, 128, 128)
    assert not sup(600, 64, 64) and not sup(600, 128, 64, 0.2)
    gen = torch.Generator().manual_seed(9)
    W256, dA128, W128 = torch.randn(K, 256, generator=gen).to(dev), torch.randn(M, 128, generator=gen).to(dev), torch.randn(128, N, generator=gen).to(dev)
    X256 = torch.randn(M, 256, generator=gen).to(dev)
    marker = 12345.0
    dW = torch.full((K, N), marker, device=dev)
    lib = _lib.load()
    bad = [
        (dA[:512], W, ops.FusedWgrad(X[:512], pro=pro, out=dW), None, "unsupported"),
        (dA, W256, ops.FusedWgrad(X256, out=torch.full((K, 256), marker, device=dev)), None, "unsupported"),
        (dA128, W128, ops.FusedWgrad(X, pro=pro, out=torch.full((128, N), marker, device=dev)), None, "unsupported"),
        (dA, W, ops.FusedWgrad(X, pro=ops.Pro(fold.scale, fold.shift, True, 0.2, seed=3, site=1), out=dW), None, "drop_p"),
        (dA, W, ops.FusedWgrad(X, pro=pro, out=dW), ops.NextBN(X, ops.Pro(fold.scale, fold.shift, True, 0.2, seed=3, site=1), fold), "drop_p"),
        (dA, W, ops.FusedWgrad(X.clone(), pro=pro, out=dW), ops.NextBN(X, pro, fold), "wg->X"),
        (dA, W, ops.FusedWgrad(X, pro=ops.Pro(fold.scale, fold.shift, False), out=dW), ops.NextBN(X, pro, fold), "must agree"),
        (dA, W, ops.FusedWgrad(X, pro=None, out=dW), ops.NextBN(X, pro, fold), "must agree"),
    ]
    ops.probe_arm(64)
    try:
        for dy, Wm, fw, nbn, text in bad:
            # through the library itself, with every output pre-filled: a write would show
            Mb, Kb, Nb = dy.shape[0], dy.shape[1], Wm.shape[1]
            gP = torch.full((Mb, Nb), marker, device=dev)
            nbt, sums = ops._next_bn(nbn, Mb, Nb) if nbn is not None else (None, None)
            if sums is not None:
                sums.fill_(marker)
            wt = ops._fused_wgrad(fw, Mb, Nb, Kb)
            rc = lib.mmg_linear_dgrad_wgrad(dy.data_ptr(), Wm.data_ptr(), gP.data_ptr(), Mb, Nb, Kb,
                                            C.byref(nbt) if nbt is not None else None, C.byref(wt), None)
            err = lib.mmg_last_error().decode()
            assert rc == -1 and "linear_dgrad_wgrad" in err and text in err, (rc, err)
            torch.cuda.synchronize()
            assert bool((gP == marker).all()) and bool((fw.dW == marker).all())
            assert sums is None or bool((sums == marker).all())
            with pytest.raises(_lib.MmgError, match=r"rc=-1\).*linear_dgrad_wgrad"):          # and through the wrapper
                ops.linear_dgrad_wgrad(dy, Wm, fw, next_bn=nbn)
            assert bool((fw.dW == marker).all())
    finally:
        rows = ops.probe_read()
    assert rows == []
    assert bool((dW == marker).all())
    # a bias gradient is not this entry's: refused by the wrapper and by the library
    with pytest.raises(ValueError, match="bias"):
        ops.linear_dgrad_wgrad(dA, W, ops.FusedWgrad(X, pro=pro, with_bias=True))
    ws = torch.empty(lib.mmg_linear_dgrad_wgrad_ws_bytes(M, N, K), dtype=torch.uint8, device=dev)
    db = torch.full((K,), marker, device=dev)
    gP = torch.full((M, N), marker, device=dev)
    wt = _lib.BnBwdWgradT(X.data_ptr(), None, dW.data_ptr(), db.data_ptr(), 0, ws.data_ptr(), ws.numel(), None)
    rc = lib.mmg_linear_dgrad_wgrad(dA.data_ptr(), W.data_ptr(), gP.data_ptr(), M, N, K, None, C.byref(wt), None)
    assert rc == -1 and b"dbias" in lib.mmg_last_error()
    torch.cuda.synchronize()
    assert bool((gP == marker).all()) and bool((db == marker).all()) and bool((dW == marker).all())
    # (and the accepted call is probed as the data gradient's row with the new flag, followed by the slab sum)
    ops.probe_arm(64)
    ops.linear_dgrad_wgrad(dA, W, ops.FusedWgrad(X, pro=pro), next_bn=ops.NextBN(X, pro, fold))
    ops.linear_dgrad_wgrad(dA, W, ops.FusedWgrad(X))
    rows = ops.probe_read()
    fwd = [r for r in rows if r[1] == "linear_fwd"]
    assert [r[2:6] for r in fwd] == [(M, N, K, 4 | 512 | 4096), (M, N, K, 4096)]
    assert all("k_linear_dgrad_wgrad_x6" in r[6] for r in fwd)
    assert [r[2:5] for r in rows if r[1] == "linear_wgrad_reduce"] == [(M, K, N)] * 2
    assert not [r for r in rows if r[1] == "linear_wgrad"]


# ------------------------------------------------------------------------------------------ captured training steps
CFG = {"model": {"architecture": "RGCN", "hidden_dim": 128, "num_layers": 2, "dropout": 0.2, "use_batch_norm": True,
                 "activation": "relu"}}
LAB = ("patient", "has_lab", "lab")
_RUNS = {}


def _run(dev, fused, heads):
    """Two captured training steps on synth.make_graph(1) (1,834 patients) + one probed eager step -> (losses, pred,
    gradients, state, probe rows); computed once per (switch, "heads" among the next-BatchNorm sites)."""
    if (fused, heads) in _RUNS:
        return _RUNS[(fused, heads)]
    import mmgnn  # noqa: F401
    import mmgnn.model as mm
    from mmgnn import ops as o
    from mmgnn.data import build_plan
    from mmgnn.model import build_model
    from mmgnn.optim import Adam
    from mmgnn.synth import make_graph
    from mmgnn.train import PiecewiseGraphedTrainStep
    sites = mm.NEXT_BN_SITES
    mm.set_fused_head_wgrad(fused)
    mm.set_next_bn(sites if heads else sites - {"heads"})
    try:
        g = make_graph(1, seed=0, device=dev)
        torch.manual_seed(42)
        model = build_model(CFG, (g.node_types, g.edge_types), None).to(dev)
        model._init_embeddings(g)
        ei = g[LAB].edge_index
        E = ei.shape[1]
        tr = torch.randperm(E, generator=torch.Generator(device=dev).manual_seed(42), device=dev)[: int(0.7 * E)].sort().values
        pi, li = ei[0][tr].contiguous(), ei[1][tr].contiguous()
        y = g[LAB].edge_attr[tr].squeeze(-1).contiguous()
        sup = torch.rand(tr.numel(), generator=torch.Generator(device=dev).manual_seed(1234), device=dev) < 0.2
        wlab = torch.ones(int(g["lab"].num_nodes), device=dev)
        opt = Adam([q for k, q in model.named_parameters() if not k.startswith("embeddings.")], lr=1e-2)
        plan = build_plan(g, dev, use_cache=False)
        step = PiecewiseGraphedTrainStep(model, plan, pi, li, y, wlab, opt, sup, None)
        losses = [float(step.step()) for _ in range(2)]
        torch.cuda.synchronize()
        grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
        state = {k: v.clone() for k, v in model.state_dict().items()}
        pred = step.pred.clone()
        # the launches of one step, eagerly and probed (a captured launch carries no events)
        model._seed_dev = None
        model.train()
        model.zero_grad(set_to_none=True)
        o.probe_arm(1 << 12)
        try:
            p = model.predict_lab_values(plan, pi, li)
            supf = sup.float()
            o.weighted_pair_loss(p, y, wlab[li], supf, 1.0 / max(float(supf.sum()), 1.0), "mae").backward()
            torch.cuda.synchronize()
        finally:
            rows = o.probe_read()
    finally:
        mm.set_fused_head_wgrad(True)
        mm.set_next_bn(sites)
    _RUNS[(fused, heads)] = (losses, pred, grads, state, rows, int(plan.n_rows))
    return _RUNS[(fused, heads)]


def _head_rows(rows, P):
    fused = [r for r in rows if r[1] == "linear_fwd" and r[5] & 4096]
    plain_fwd = [r for r in rows if r[1] == "linear_fwd" and r[2:5] == (P, N, K) and not r[5] & 4096]
    plain_wg = [r for r in rows if r[1] == "linear_wgrad" and r[2:5] == (P, K, N)]
    return fused, plain_fwd, plain_wg


def test_training_steps_without_the_heads_site_are_bitwise_the_same(dev):
    """set_fused_head_wgrad with "heads" taken out of the next-BatchNorm sites: the statistics come from the separate
    pass over a bit-identical gP, so loss, predictions, every gradient and every updated parameter are the same bits;
    the probed step shows the fused row (no epilogue flag) in place of the two launches."""
    (l1, p1, g1, s1, rows1, P), (l0, p0, g0, s0, rows0, _) = _run(dev, True, False), _run(dev, False, False)
    assert P == 1834
    assert l0 == l1 and same(p0, p1)
    assert set(g0) == set(g1) and set(s0) == set(s1)
    for k in g0:
        assert same(g0[k], g1[k]), k
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
    f1, pf1, pw1 = _head_rows(rows1, P)
    f0, pf0, pw0 = _head_rows(rows0, P)
    assert any(r[2:5] == (P, N, K) and not r[5] & 512 for r in f1) and not pf1 and not pw1
    assert not f0 and len(pf0) == 1 and len(pw0) == 1


def test_training_steps_with_the_default_sites_agree_like_the_parent_paths(dev):
    """Default sites: the statistics' fp64 summation order is the only change.  Over loss, predictions, gradients and
    updated parameters, the largest relative difference (max |a - b| / max |b| per array) between switch on and off must
    be within twice the one the parent path shows between "heads" on and off -- one more perturbation of the same kind."""
    on, off, off_nh = _run(dev, True, True), _run(dev, False, True), _run(dev, False, False)

    def diff(a, b):
        d = abs(a[0][1] - b[0][1]) / abs(b[0][1])
        d = max(d, rel(a[1], b[1]))
        for part in (2, 3):
            assert set(a[part]) == set(b[part])
            for k in a[part]:
                if a[part][k].is_floating_point():
                    d = max(d, rel(a[part][k], b[part][k]))
                else:
                    assert torch.equal(a[part][k], b[part][k]), k
        return d

    new, ref = diff(on, off), diff(off, off_nh)
    print(f"fused on vs off (default sites): {new:.3e}; parent heads on vs off: {ref:.3e}")
    assert new <= 2 * ref, (new, ref)
    P = on[5]
    f1, pf1, pw1 = _head_rows(on[4], P)
    f0, pf0, pw0 = _head_rows(off[4], P)
    assert any(r[2:5] == (P, N, K) and r[5] & 512 for r in f1) and not pf1 and not pw1
    assert not f0 and len(pf0) == 1 and pf0[0][5] & 512 and len(pw0) == 1
