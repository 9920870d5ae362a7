"""The dual backward launch of the encoder's second linear (mmg_linear_bnbwd_dual, ops.DualBwd, mmgnn.model.set_dual_enc_bwd):
pass B's masked write and pass A's masked accumulate of tests/test_enc_masked_handdown_gpu.py as ONE launch.

The yardstick is that pair of launches, which the file named above holds against fp32 torch and tests/rng_ref.py; every
comparison here is on the bits.

a. the dual launch against write + accumulate: Gs, the slab-summed dW and db of each pass, d beta / d gamma of each pass, and
   (once) the dZ of each pass -- at the shapes where the kernel's control flow changes, p = 0.2 and 0.5, row offset 1000,
   the seed by value and by pointer, a gradient with zeros, negatives and one infinity, a row list of ~1.5 % with row 0 and
   row M - 1, and an empty row list.
b. the support query, the refusals (nothing launched) and the probe row of an accepted launch.
c. two captured training steps with the switch on and off: the same steps; which entry points the recorded backward called.
d. 256-d and 512 patient rows: today's path.

Shapes (M) as in the file above (checked there against the launch plan): 513 one tile per workgroup with a one-row last tile,
8,193 two tiles and one, 16,389 three tiles each, 24,601 four and three mixed.  In the dual kernel a workgroup runs two
bodies per tile -- no empty trailing tile -- so the odd counts exercise the loop's exit after a pass-A body."""
import numpy as np
import pytest
import torch

import test_enc_masked_handdown_gpu as H

pytestmark = pytest.mark.gpu

K = N = 128
DUAL_FLAGS = 16 | 128 | 1024 | 8192 | 16384


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


same = H.same


def both_passes(c, g, dual, keep_dz=False, x_a=None, pro1_a=None):
    """Pass B's masked write, then pass A's masked accumulate -- with one holder (dual) or without
    -> (Gs, (dz, dW, db, d beta, d gamma) of B, the same of A)"""
    o = c.ops
    pair = o.DualBwd() if dual else None
    db_, da_ = torch.zeros(2, K, device=g.device), torch.zeros(2, K, device=g.device)
    fb = o.FusedWgrad(c.z1, c.pro1_b, with_bias=True, keep_dz=keep_dz)
    fa = o.FusedWgrad(c.z1 if x_a is None else x_a, c.pro1_a if pro1_a is None else pro1_a, with_bias=True, keep_dz=keep_dz)
    dz_b, gs = o.linear_bnbwd(g, c.z2, c.pro2_b, c.f2, c.W, c.sums_b, c.M, db_[0], db_[1], wgrad=fb,
                              masked=o.MaskedDx(c.pro1_b, pair=pair))
    dz_a, gs2 = o.linear_bnbwd_rows(c.g_rows, c.row_pos, c.z2, c.pro2_a, c.f2, c.W, c.sums_a, c.M, da_[0], da_[1], wgrad=fa,
                                    masked=o.MaskedDx(fa.pro, into=gs, pair=pair))
    assert gs2 is gs and (dz_b is None) == (not keep_dz) and (dz_a is None) == (not keep_dz)
    if pair is not None:
        pair.require_consumed()
    return gs, (dz_b, fb.dW, fb.db, db_[0], db_[1]), (dz_a, fa.dW, fa.db, da_[0], da_[1])


def assert_same_outputs(got, want):
    assert same(got[0], want[0]), "Gs"
    for which, g, w in (("B", got[1], want[1]), ("A", got[2], want[2])):
        for name, x, y in zip(("dz", "dW", "db", "dbeta", "dgamma"), g, w):
            assert (x is None and y is None) or same(x, y), f"pass {which}: {name}"


@pytest.mark.parametrize("M,p,byptr,sel", H.CASES)
def test_dual_launch_against_write_and_accumulate(ops, dev, M, p, byptr, sel):
    c = H.Case(ops, dev, M, p, byptr, sel)
    assert ops.linear_bnbwd_dual_supported(M, N, K)
    want = both_passes(c, c.g_b, False)
    assert torch.isfinite(want[0]).all() and float(want[0].abs().max()) > 0
    # (an empty row list: pass A's upstream gradient and its statistics are zero, and so are its dZ and dW)
    assert float(want[1][1].abs().max()) > 0 and (float(want[2][1].abs().max()) > 0) == (sel == "listed")
    assert not same(want[1][1], want[2][1])
    assert_same_outputs(both_passes(c, c.g_b, True), want)
    # one infinity in pass B's gradient, where it reaches dX (the activation is on, the element kept)
    act = (c.z2 * c.f2.scale + c.f2.shift > 0) & torch.from_numpy(H.R.mask2d(H.SEED, 7, M, K, p, H.OFF)).to(dev)
    r, col = [int(v) for v in act.nonzero()[act.sum() // 2]]
    g_inf = c.g_b.clone()
    g_inf[r, col] = float("inf")
    want = both_passes(c, g_inf, False)
    assert not torch.isfinite(want[0][r]).all()
    assert_same_outputs(both_passes(c, g_inf, True), want)


@pytest.mark.parametrize("M", [513, 16389])
def test_dz_of_each_pass_where_it_is_kept(ops, dev, M):
    c = H.Case(ops, dev, M, 0.2, True, "listed")
    want = both_passes(c, c.g_b, False, keep_dz=True)
    got = both_passes(c, c.g_b, True, keep_dz=True)
    assert float(want[1][0].abs().max()) > 0 and float(want[2][0].abs().max()) > 0
    assert_same_outputs(got, want)
    assert_same_outputs(both_passes(c, c.g_b, True, keep_dz=True), got)      # the same call twice: the same bits


def test_support_query_refusals_and_the_probe_row(ops, dev):
    sup = ops.linear_bnbwd_dual_supported
    assert sup(513, 128, 128) and sup(183400, 128, 128)
    assert not sup(512, 128, 128) and not sup(5000, 256, 256) and not sup(5000, 64, 128) and not sup(5000, 128, 64)
    c = H.Case(ops, dev, 513, 0.2, False, "listed")
    small = H.Case(ops, dev, 512, 0.2, False, "listed")
    pro = lambda **kw: ops.Pro(c.f1.scale, c.f1.shift, True, kw.pop("p", 0.2), seed=H.SEED, site=H.SITE_A,      # noqa: E731
                               row_offset=kw.pop("row_offset", H.OFF))
    ops.probe_arm(64)
    try:
        with pytest.raises(Exception, match="does not cover"):                       # M = 512
            both_passes(small, small.g_b, True)
        with pytest.raises(Exception, match="pairs a linear_bnbwd write"):           # swapped modes: a rows call that writes
            fw = ops.FusedWgrad(c.z1, c.pro1_a, with_bias=True, keep_dz=False)
            ops.linear_bnbwd_rows(c.g_rows, c.row_pos, c.z2, c.pro2_a, c.f2, c.W, c.sums_a, c.M, wgrad=fw,
                                  masked=ops.MaskedDx(c.pro1_a, pair=ops.DualBwd()))
        with pytest.raises(Exception, match="pairs a linear_bnbwd write"):           # ... and a dense call that accumulates
            fw = ops.FusedWgrad(c.z1, c.pro1_b, with_bias=True, keep_dz=False)
            ops.linear_bnbwd(c.g_b, c.z2, c.pro2_b, c.f2, c.W, c.sums_b, c.M, wgrad=fw,
                             masked=ops.MaskedDx(c.pro1_b, into=torch.zeros(c.M, N, device=dev), pair=ops.DualBwd()))
        with pytest.raises(Exception, match="different X"):
            both_passes(c, c.g_b, True, x_a=c.z1.clone())
        with pytest.raises(Exception, match="differ in more than the dropout site"):
            both_passes(c, c.g_b, True, pro1_a=pro(p=0.3))
        with pytest.raises(Exception, match="differ in more than the dropout site"):
            both_passes(c, c.g_b, True, pro1_a=pro(row_offset=H.OFF + 1))
        # a holder consumed with a foreign `into`, an empty holder, and a parked write that is never launched
        pair = ops.DualBwd()
        fb = ops.FusedWgrad(c.z1, c.pro1_b, with_bias=True, keep_dz=False)
        ops.linear_bnbwd(c.g_b, c.z2, c.pro2_b, c.f2, c.W, c.sums_b, c.M, wgrad=fb, masked=ops.MaskedDx(c.pro1_b, pair=pair))
        fa = ops.FusedWgrad(c.z1, c.pro1_a, with_bias=True, keep_dz=False)
        with pytest.raises(Exception, match="not that of the parked write"):
            ops.linear_bnbwd_rows(c.g_rows, c.row_pos, c.z2, c.pro2_a, c.f2, c.W, c.sums_a, c.M, wgrad=fa,
                                  masked=ops.MaskedDx(c.pro1_a, into=torch.zeros(c.M, N, device=dev), pair=pair))
        with pytest.raises(RuntimeError, match="never launched"):
            pair.require_consumed()
        with pytest.raises(RuntimeError, match="no parked write"):
            ops.linear_bnbwd_rows(c.g_rows, c.row_pos, c.z2, c.pro2_a, c.f2, c.W, c.sums_a, c.M, wgrad=fa,
                                  masked=ops.MaskedDx(c.pro1_a, into=torch.zeros(c.M, N, device=dev), pair=ops.DualBwd()))
        torch.cuda.synchronize()
    finally:
        rows = ops.probe_read()
    assert [r for r in rows if r[1] == "linear_fwd"] == []
    ops.probe_arm(64)
    both_passes(c, c.g_b, True)
    torch.cuda.synchronize()
    rows = [r for r in ops.probe_read() if r[1] == "linear_fwd"]
    assert [(r[2], r[3], r[4], r[5]) for r in rows] == [(513, 128, 128, DUAL_FLAGS)]


def _steps(dev, hidden, make, n_steps):
    """n_steps captured training steps per setting of set_dual_enc_bwd (on, off)
    -> [(losses, pred, state, the BatchNorm-backward entry points the recorded backward called)]"""
    import mmgnn  # noqa: F401
    import mmgnn.model as mm
    from mmgnn import ops as o
    from mmgnn.data import build_plan
    from mmgnn.model import build_model
    from mmgnn.optim import Adam
    from mmgnn.train import PiecewiseGraphedTrainStep
    cfg = {"model": {"architecture": "RGCN", "hidden_dim": hidden, "num_layers": 2, "dropout": 0.2, "use_batch_norm": True,
                     "activation": "relu"}}
    LAB = ("patient", "has_lab", "lab")
    res, calls, real = [], [], o._call

    def counted(name, *a, **kw):
        if name in ("mmg_linear_bnbwd_dual", "mmg_linear_bnbwd_masked"):
            calls.append(name)
        return real(name, *a, **kw)

    o._call = counted
    try:
        for flag in (True, False):
            mm.set_dual_enc_bwd(flag)
            g = make(dev)
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
            losses = [float(step.step()) for _ in range(n_steps)]
            res.append((losses, step.pred.clone(), {k: v.clone() for k, v in model.state_dict().items()}, calls[n_before:]))
    finally:
        mm.set_dual_enc_bwd(True)
        o._call = real
    return res


def _same_steps(a, b):
    assert a[0] == b[0] and np.isfinite(a[0]).all() and torch.equal(a[1], b[1])
    assert set(a[2]) == set(b[2])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def test_graphed_training_steps_with_and_without_the_dual_launch(dev):
    """c. two captured training steps on synth.make_graph(1) (1,834 patients, 128-d): loss, pred, every parameter and buffer;
    with the switch on every recorded backward makes ONE dual call and no masked call, with it off the two masked calls."""
    import mmgnn.model as mm
    from mmgnn.synth import make_graph
    assert mm.DUAL_ENC_BWD is True
    on, off = _steps(dev, 128, lambda d: make_graph(1, seed=0, device=d), 2)
    assert len(on[3]) >= 1 and set(on[3]) == {"mmg_linear_bnbwd_dual"}
    assert len(off[3]) == 2 * len(on[3]) and set(off[3]) == {"mmg_linear_bnbwd_masked"}
    _same_steps(on, off)
    assert mm.DUAL_ENC_BWD is True


@pytest.mark.parametrize("what", ["d256", "m512"])
def test_shapes_without_the_dual_form_take_the_launches_they_took(dev, what):
    """d. 256-d and 512 patient rows: no dual launch whatever the switch says, and the same step."""
    from mmgnn.synth import EICU, make_graph
    if what == "d256":
        hidden, make = 256, lambda d: make_graph(1, seed=0, device=d)
    else:
        hidden, make = 128, lambda d: make_graph(1, seed=0, device=d, shape=dict(EICU, patients=512, e_lab=512 * 33, e_dx=512 * 4,
                                                                                  e_med=512 * 8))
    on, off = _steps(dev, hidden, make, 1)
    assert on[3] == [] and off[3] == []
    _same_steps(on, off)
