"""mmg_linear_fwd_dual -- the encoder's second linear under the two dropout masks of a training step in ONE launch --
against the two mmg_linear_fwd calls it replaces: both outputs, both sets of column statistics, both BatchNorm folds and
the running statistics (advanced once per pass, pass 0 first) bit for bit; the masks against tests/rng_ref.py; the
refusals; and captured training steps with and without it.

Shapes (K = N = 128, 32-row tiles, row sets = min(512, tiles)): M = 513 -> 17 tiles, the last of one row; 1,056 -> 33
tiles, one per row set; 16,389 -> 513 tiles, one row set gets a second tile, short last tile; 49,157 -> 1,537 tiles, every
row set runs the peeled pair and enters the loop, row sets of 3 and of 4 tiles."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rng_ref as R  # noqa: E402

K = N = 128


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


def _inputs(dev, M, seed, with_scale, specials):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=gen) * 1.5 + 0.2        # ~45 % negative behind the affine: the ReLU gate
    x[torch.rand(M, K, generator=gen) < 0.05] = 0.0           # exact zeros
    if specials:
        x[M // 2, 17] = float("inf")                          # one non-finite value
    W = torch.randn(N, K, generator=gen) / K ** 0.5
    b = torch.randn(N, generator=gen)
    scale = shift = None
    if with_scale:
        scale, shift = torch.rand(K, generator=gen) + 0.5, torch.randn(K, generator=gen) * 0.3
    gamma, beta = torch.rand(N, generator=gen) + 0.5, torch.randn(N, generator=gen) * 0.2
    rm, rv = torch.randn(N, generator=gen) * 0.1, torch.rand(N, generator=gen) + 0.5
    to = lambda t: None if t is None else t.to(dev)      # noqa: E731
    return tuple(to(t) for t in (x, W, b, scale, shift, gamma, beta, rm, rv))


def _pros(ops, dev, scale, shift, p, seed, by_ptr, row_offset, sites=(0, 2)):
    sd = torch.tensor([seed], dtype=torch.int64, device=dev) if by_ptr else None
    # with a device seed the value in the descriptor is not the one that counts
    return [ops.Pro(scale, shift, True, p, seed=(12345 if by_ptr else seed), site=s, row_offset=row_offset, seed_dev=sd)
            for s in sites]


CASES = [
    # M,     p,   scale, seed by pointer, row_offset, non-finite value
    (513,    0.2, True,  False, 0,        True),
    (1056,   0.5, False, True,  1_000_003, False),
    (16389,  0.2, True,  True,  183_400,  True),
    (49157,  0.5, True,  False, 0,        False),
    (49157,  0.2, False, False, 77,       False),
]


@pytest.mark.parametrize("M, p, with_scale, by_ptr, row_offset, specials", CASES)
def test_dual_launch_is_the_two_launches_bit_for_bit(ops, dev, M, p, with_scale, by_ptr, row_offset, specials):
    x, W, b, scale, shift, gamma, beta, rm, rv = _inputs(dev, M, 7 * M + int(100 * p), with_scale, specials)
    pros = _pros(ops, dev, scale, shift, p, 0x1234_5678_9ABC + M, by_ptr, row_offset)
    assert ops.linear_fwd_dual_supported(M, N, K)
    # folded: (out, sums, BNFold) per pass, the running statistics advanced by pass 0, then by pass 1
    rm_a, rv_a, rm_b, rv_b = rm.clone(), rv.clone(), rm.clone(), rv.clone()
    want = [ops.linear_fwd(x, W, b, pro=pr, bn=(gamma, beta, rm_a, rv_a, 1)) for pr in pros]
    got = ops.linear_fwd_dual(x, W, b, pros[0], pros[1], bn0=(gamma, beta, rm_b, rv_b, 1), bn1=(gamma, beta, rm_b, rv_b, 1))
    for c in (0, 1):
        (y, s, f), (yw, sw, fw) = got[c], want[c]
        assert same(y, yw), f"Y{c}"
        assert same(s, sw), f"column sums of pass {c}"
        for name in ("scale", "shift", "mean", "rstd"):
            assert same(getattr(f, name), getattr(fw, name)), f"{name} of pass {c}"
    assert same(rm_b, rm_a) and same(rv_b, rv_a)
    assert not same(rm_a, rm)                                   # (they did move)
    assert not same(got[0][0], got[1][0])                        # two masks, two outputs
    if not specials:
        assert bool(torch.isfinite(got[0][0]).all()) and bool(torch.isfinite(got[1][0]).all())
    # unfolded (the patient-sharded contract): (out, sums) per pass
    want = [ops.linear_fwd(x, W, b, pro=pr, with_stats=True) for pr in pros]
    got = ops.linear_fwd_dual(x, W, b, pros[0], pros[1])
    for c in (0, 1):
        assert len(got[c]) == 2 and same(got[c][0], want[c][0]) and same(got[c][1], want[c][1])


@pytest.mark.parametrize("p", [0.2, 0.5])
def test_each_pass_draws_the_mask_of_its_own_site(ops, dev, p):
    """Pass c is (relu(bn(x)) * mask_c / (1 - p)) @ W^T + b with mask_c the host restatement's mask of site c's stream:
    the bar of test_ops_gpu.py::test_linear_fwd for the six-term product (2e-6 of an fp64 reference)."""
    M, seed, row_offset, sites = 513, 0xFEED_5EED, 4097, (0, 2)
    x, W, b, scale, shift, *_ = _inputs(dev, M, 31 + int(100 * p), True, False)
    pros = _pros(ops, dev, scale, shift, p, seed, False, row_offset, sites)
    got = ops.linear_fwd_dual(x, W, b, pros[0], pros[1])
    act = torch.relu(x.cpu() * scale.cpu() + shift.cpu()).double()
    masks = []
    for c, site in enumerate(sites):
        mask = torch.from_numpy(R.mask2d(seed, site, M, K, p, row_offset).astype("bool"))
        masks.append(mask)
        ref = (act * mask / (1.0 - p)) @ W.double().cpu().t() + b.double().cpu()
        assert rel(got[c][0], ref) <= 2e-6, f"pass {c}"
    assert not torch.equal(masks[0], masks[1])


def test_refusals_launch_nothing(ops, dev):
    """Prologues that differ in more than the site, p = 0 and unsupported shapes: the argument error, no launch."""
    from mmgnn import _lib
    M = 600
    x, W, b, scale, shift, *_ = _inputs(dev, M, 5, True, False)
    ok = dict(scale=scale, shift=shift, relu=True, p=0.2, seed=11, site=2, row_offset=0, seed_dev=None)
    pro0 = ops.Pro(scale, shift, True, 0.2, seed=11, site=0)
    sd = torch.tensor([11], dtype=torch.int64, device=dev)
    bad = [dict(ok, scale=scale.clone()), dict(ok, shift=shift.clone()), dict(ok, scale=None, shift=None), dict(ok, relu=False),
           dict(ok, p=0.5), dict(ok, seed=12), dict(ok, row_offset=32), dict(ok, seed_dev=sd), dict(ok, site=0)]
    assert not ops.linear_fwd_dual_supported(512, 128, 128) and not ops.linear_fwd_dual_supported(600, 64, 128)
    assert not ops.linear_fwd_dual_supported(600, 128, 64) and not ops.linear_fwd_dual_supported(600, 256, 256)
    assert ops.linear_fwd_dual_supported(513, 128, 128)
    ops.probe_arm(64)
    try:
        for kw in bad:
            with pytest.raises(_lib.MmgError, match=r"rc=-1\).*linear_fwd_dual"):
                ops.linear_fwd_dual(x, W, b, pro0, ops.Pro(**kw))
        with pytest.raises(_lib.MmgError, match=r"rc=-1\).*drop_p"):                            # p = 0 in both
            ops.linear_fwd_dual(x, W, b, ops.Pro(scale, shift, True, 0.0, seed=11, site=0), ops.Pro(**dict(ok, p=0.0)))
        for xs, Ws in ((x[:512], W), (x[:, :64].contiguous(), W[:, :64].contiguous()), (x, W[:64].contiguous())):
            with pytest.raises(_lib.MmgError, match=r"rc=-1\).*unsupported"):
                ops.linear_fwd_dual(xs, Ws, b[:Ws.shape[0]].contiguous(),
                                    ops.Pro(None, None, True, 0.2, seed=11, site=0), ops.Pro(None, None, True, 0.2, seed=11, site=2))
    finally:
        rows = ops.probe_read()
    assert rows == []
    # (and the accepted call is probed as one launch: N reported as 2 * 128, flag 2048)
    ops.probe_arm(64)
    ops.linear_fwd_dual(x, W, b, pro0, ops.Pro(**ok))
    rows = ops.probe_read()
    dual = [r for r in rows if r[1] == "linear_fwd"]
    assert len(dual) == 1 and dual[0][2:5] == (M, 256, 128) and dual[0][5] & 2048 and not dual[0][5] & (16 | 64)


def test_graphed_training_steps_with_and_without_the_dual_launch(dev):
    """mmgnn.model.set_dual_enc: two captured training steps on synth.make_graph(1) (1,834 patients: M > 512 takes the
    dual launch) are the SAME steps with the one launch and with the two: loss, pred and every parameter / buffer."""
    import mmgnn  # noqa: F401
    import mmgnn.model as mm
    from mmgnn import ops as o
    from mmgnn.data import build_plan
    from mmgnn.model import build_model
    from mmgnn.optim import Adam
    from mmgnn.synth import make_graph
    from mmgnn.train import PiecewiseGraphedTrainStep
    cfg = {"model": {"architecture": "RGCN", "hidden_dim": 128, "num_layers": 2, "dropout": 0.2, "use_batch_norm": True,
                     "activation": "relu"}}
    LAB = ("patient", "has_lab", "lab")
    res, calls, real = [], [], o.linear_fwd_dual

    def counted(x, W, *a, **kw):
        calls.append((x.shape[0], W.shape[0], W.shape[1]))
        return real(x, W, *a, **kw)

    o.linear_fwd_dual = counted
    try:
        for flag in (True, False):
            mm.set_dual_enc(flag)
            g = make_graph(1, seed=0, device=dev)
            torch.manual_seed(42)
            model = build_model(cfg, (g.node_types, g.edge_types), None).to(dev)
            model._init_embeddings(g)
            ei = g[LAB].edge_index
            E = ei.shape[1]
            tr = torch.randperm(E, generator=torch.Generator(device=dev).manual_seed(42), device=dev)[: int(0.7 * E)].sort().values
            pi, li = ei[0][tr].contiguous(), ei[1][tr].contiguous()
            y = g[LAB].edge_attr[tr].squeeze(-1).contiguous()
            sup = torch.rand(tr.numel(), generator=torch.Generator(device=dev).manual_seed(1234), device=dev) < 0.2
            wlab = torch.ones(int(g["lab"].num_nodes), device=dev)
            opt = Adam([q for k, q in model.named_parameters() if not k.startswith("embeddings.")], lr=1e-2)
            n_before = len(calls)
            step = PiecewiseGraphedTrainStep(model, build_plan(g, dev, use_cache=False), pi, li, y, wlab, opt, sup, None)
            losses = [float(step.step()) for _ in range(2)]
            res.append((losses, step.pred.clone(), {k: v.clone() for k, v in model.state_dict().items()}, len(calls) - n_before))
    finally:
        mm.set_dual_enc(True)
        o.linear_fwd_dual = real
    (l1, p1, s1, n1), (l0, p0, s0, n0) = res
    assert n1 >= 1 and n0 == 0              # the switch switches (a captured step calls it once, while it is recorded)
    assert calls[0][:3] == (1834, 128, 128)
    assert l0 == l1 and same(p0, p1)
    assert set(s0) == set(s1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
