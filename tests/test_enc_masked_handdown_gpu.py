"""The masked dX store of the fused BatchNorm-backward + weight-gradient GEMM (mmg_linear_bnbwd_masked) and the one
gradient it lets the two encoder passes of a training step hand to the first BatchNorm they share.

a. producer: after the dense pass's masked WRITE and the listed-rows pass's masked ACCUMULATE, DX holds
   where(keepB, dX_B * inv, 0) + where(keepA, dX_A * inv, 0) bit for bit -- dX_B / dX_A from the unmasked launches, the keep
   masks from tests/rng_ref.py, the expression formed in fp32 torch; summed dW, db, d beta, d gamma are the unmasked launch's.
b. consumers: mmg_bn_bwd_stats(Gs, p = 0) == mmg_bn_bwd_stats2(dX_B, dX_A), and the MODE 0 launch on Gs == the MODE 2 launch on
   the pair in dE, dW, db, d beta, d gamma.
c. two captured training steps with mmgnn.model.set_masked_handdown on and off: the same steps.
d. the support query, the refusals (nothing launched) and the shapes that keep the two tensors.

Shapes (M): one tile per workgroup with a one-row last tile; both peeled tiles real with a ragged end; three tiles each (the
loop entered, its second body on an empty tile); four and three tiles mixed -- recomputed below from the launch plan."""
import numpy as np
import pytest
import torch

import dense_plan_ref as D
import rng_ref as R

pytestmark = pytest.mark.gpu

K = N = 128
# M -> (32-row tiles, workgroups, tiles per workgroup) as the issue states them; checked against plan_wgrad below
SHAPES = {513: (17, 17, {1}), 8193: (257, 129, {2, 1}), 16389: (513, 171, {3}), 24601: (769, 193, {4, 3})}
SEED = 0x1234_5678_9ABC
OFF = 1000                     # row offset of every mask (a shard's first row)
SITE_B, SITE_A = 3, 5          # the first dropout of pass B / pass A (the masks handed down)


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


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same(a, b):
    """bit for bit: an infinity or a NaN equals itself, +0 differs from -0"""
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def test_shapes_are_what_the_launch_plan_makes_of_them():
    for M, (tiles, wgs, per) in SHAPES.items():
        p = D.plan_wgrad(M, K, N)
        assert (D.cdiv(M, 32), p.n_split) == (tiles, wgs), M
        assert {len(D.wgrad_stages(M, p.n_split, y)) for y in range(p.n_split)} == per, M
    assert D.last_stage_rows(513) == 1 and all(M % 32 for M in SHAPES)


class Case:
    """Both passes' second-linear backward on fixed inputs: B dense (MODE 0), A on listed rows (MODE 3)."""

    def __init__(self, ops, dev, M, p, byptr, sel):
        gen = torch.Generator().manual_seed(M + int(p * 100) + 7 * byptr)
        self.ops, self.M, self.p = ops, M, p
        r = lambda *s: torch.randn(*s, generator=gen)                     # noqa: E731
        self.W = (r(K, N) / K ** 0.5).to(dev)
        self.W0 = (r(K, N) / K ** 0.5).to(dev)
        self.z2, self.z1, self.E = (r(M, K) * 1.5 + 0.2).to(dev), (r(M, N) * 1.3 + 0.1).to(dev), r(M, N).to(dev)
        fin = lambda y: ops.bn_finalize(ops.col_reduce2(y), M, (torch.rand(K, generator=gen) + 0.5).to(dev),   # noqa: E731
                                        (r(K) * 0.2).to(dev), None, None, True)
        self.f2, self.f1 = fin(self.z2), fin(self.z1)
        seed_dev = torch.tensor([SEED], dtype=torch.int64, device=dev) if byptr else None
        sd = dict(seed=123 if byptr else SEED, row_offset=OFF, seed_dev=seed_dev)     # by pointer: the value is overridden
        pro = lambda f, site, pp=p: ops.Pro(f.scale, f.shift, True, pp, site=site, **sd)          # noqa: E731
        self.pro2_b, self.pro2_a = pro(self.f2, 7), pro(self.f2, 9)
        self.pro1_b, self.pro1_a = pro(self.f1, SITE_B), pro(self.f1, SITE_A)
        self.pro1_nodrop = pro(self.f1, SITE_B, 0.0)
        g = r(M, K)
        g[torch.rand(M, K, generator=gen) < 0.1] = 0.0                     # zeros; negatives come with randn
        self.g_b = g.to(dev)
        if sel == "empty":
            rows = torch.zeros(0, dtype=torch.int64)
        else:                                                              # ~1.5 % of the rows, with row 0 and row M - 1
            rows = torch.cat([torch.tensor([0, M - 1]), torch.randperm(M, generator=gen)[:max(1, int(0.015 * M))]]).unique()
        self.rows = rows.to(dev)
        self.g_rows = r(rows.numel(), K).to(dev)
        self.row_pos = torch.full((M,), -1, dtype=torch.int32, device=dev)
        self.row_pos[self.rows] = torch.arange(rows.numel(), dtype=torch.int32, device=dev)
        dense_a = torch.zeros(M, K, device=dev)
        dense_a[self.rows] = self.g_rows
        # the statistics are inputs of the launches: those of the finite gradients throughout
        self.sums_b = ops.bn_bwd_stats(self.g_b, self.z2, self.pro2_b, self.f2)
        self.sums_a = ops.bn_bwd_stats(dense_a, self.z2, self.pro2_a, self.f2)
        inv = torch.tensor(float(R.inv_keep(p)), dtype=torch.float32, device=dev)
        assert float(inv) == float(R.inv_keep(p))
        self.inv = inv
        self.keep_b = torch.from_numpy(R.mask2d(SEED, SITE_B, M, N, p, OFF)).to(dev)
        self.keep_a = torch.from_numpy(R.mask2d(SEED, SITE_A, M, N, p, OFF)).to(dev)

    def pass_b(self, g, masked=None):
        """-> (dx, dW, db, d beta, d gamma)"""
        o, d = self.ops, torch.zeros(2, K, device=g.device)
        fw = o.FusedWgrad(self.z1, self.pro1_b, with_bias=True, keep_dz=False)
        dz, dx = o.linear_bnbwd(g, self.z2, self.pro2_b, self.f2, self.W, self.sums_b, self.M, d[0], d[1], wgrad=fw,
                                **(dict(masked=masked) if masked is not None else {}))
        assert dz is None
        return dx, fw.dW, fw.db, d[0], d[1]

    def pass_a(self, masked=None):
        o, d = self.ops, torch.zeros(2, K, device=self.z1.device)
        fw = o.FusedWgrad(self.z1, self.pro1_a, with_bias=True, keep_dz=False)
        dz, dx = o.linear_bnbwd_rows(self.g_rows, self.row_pos, self.z2, self.pro2_a, self.f2, self.W, self.sums_a, self.M,
                                     d[0], d[1], wgrad=fw, **(dict(masked=masked) if masked is not None else {}))
        assert dz is None
        return dx, fw.dW, fw.db, d[0], d[1]

    def handed_down(self, g):
        """masked write by pass B, masked accumulate by pass A -> (Gs, B's outputs, A's outputs)"""
        o = self.ops
        b = self.pass_b(g, o.MaskedDx(self.pro1_b))
        a = self.pass_a(o.MaskedDx(self.pro1_a, into=b[0]))
        assert a[0] is b[0]
        return b[0], b, a

    def expected(self, dx_b, dx_a):
        zero = torch.zeros((), device=dx_b.device)
        return torch.where(self.keep_b, dx_b * self.inv, zero) + torch.where(self.keep_a, dx_a * self.inv, zero)


CASES = [(M, p, byptr, "listed") for M in SHAPES for p in (0.2, 0.5) for byptr in (False, True)] + \
        [(M, 0.2, False, "empty") for M in SHAPES]


@pytest.mark.parametrize("M,p,byptr,sel", CASES)
def test_masked_write_and_accumulate_then_the_consumers(ops, dev, M, p, byptr, sel):
    c = Case(ops, dev, M, p, byptr, sel)
    assert ops.linear_bnbwd_masked_supported(M, N, K, ops.BNBWD_BN) and ops.linear_bnbwd_masked_supported(M, N, K, ops.BNBWD_ROWS)
    assert 0.5 * (1 - p) < float(c.keep_b.float().mean()) < 1 - 0.5 * p and not torch.equal(c.keep_a, c.keep_b)
    # ---- a. producer, finite gradients
    ub, ua = c.pass_b(c.g_b), c.pass_a()
    gs, mb, ma = c.handed_down(c.g_b)
    want = c.expected(ub[0], ua[0])
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    assert same(gs, want)
    for got, ref in ((mb, ub), (ma, ua)):               # dW, db, d beta, d gamma: untouched by the option
        assert all(same(x, y) for x, y in zip(got[1:], ref[1:]))
    if sel == "empty":                                  # nothing listed: pass A adds its dense part alone
        assert int(c.rows.numel()) == 0
    # ---- b. consumers of the one tensor against today's consumers of the pair
    s1 = ops.bn_bwd_stats(gs, c.z1, c.pro1_nodrop, c.f1)
    s2 = ops.bn_bwd_stats2(ub[0], ua[0], c.z1, c.pro1_b, c.pro1_a, c.f1)
    assert torch.equal(s1, s2)
    d1, d2 = torch.zeros(2, K, device=dev), torch.zeros(2, K, device=dev)
    f1, f2 = (ops.FusedWgrad(c.E, None, with_bias=True, keep_dz=False) for _ in range(2))
    _, de1 = ops.linear_bnbwd(gs, c.z1, c.pro1_nodrop, c.f1, c.W0, s1, M, d1[0], d1[1], wgrad=f1)
    _, de2 = ops.linear_bnbwd2(ub[0], ua[0], c.z1, c.pro1_b, c.pro1_a, c.f1, c.W0, s2, M, d2[0], d2[1], wgrad=f2)
    assert torch.equal(de1, de2) and torch.equal(f1.dW, f2.dW) and torch.equal(f1.db, f2.db) and torch.equal(d1, d2)
    # ---- a. again with ONE infinity in pass B's gradient, where it reaches dX (the activation is on, the element kept)
    act = (c.z2 * c.f2.scale + c.f2.shift > 0) & torch.from_numpy(R.mask2d(SEED, 7, M, K, p, OFF)).to(dev)
    r, col = [int(v) for v in act.nonzero()[act.sum() // 2]]
    g_inf = c.g_b.clone()
    g_inf[r, col] = float("inf")
    ub = c.pass_b(g_inf)
    gs, mb, _ = c.handed_down(g_inf)
    assert not torch.isfinite(ub[0][r]).any() and torch.isfinite(ub[0][r - 1 if r else 1]).all()
    assert same(gs, c.expected(ub[0], ua[0]))
    assert all(same(x, y) for x, y in zip(mb[1:], ub[1:]))


def test_the_same_call_twice_and_a_mask_without_dropout(ops, dev):
    """Repeatable bits; and with p = 0 in the X prologue and the mask the store is the plain / the accumulating one."""
    c = Case(ops, dev, 8193, 0.2, False, "listed")
    g1, _, _ = c.handed_down(c.g_b)
    g2, _, _ = c.handed_down(c.g_b)
    assert same(g1, g2)
    c.pro1_b, c.pro1_a = c.pro1_nodrop, c.pro1_nodrop
    ub, ua = c.pass_b(c.g_b), c.pass_a()
    gs, _, _ = c.handed_down(c.g_b)
    assert same(gs, ub[0] * 1.0 + ua[0] * 1.0)


def test_support_query_and_refusals_launch_nothing(ops, dev):
    sup = ops.linear_bnbwd_masked_supported
    assert sup(513, 128, 128, ops.BNBWD_BN) and sup(513, 128, 128, ops.BNBWD_ROWS)
    assert not sup(512, 128, 128, ops.BNBWD_BN) and not sup(512, 128, 128, ops.BNBWD_ROWS)
    assert not sup(5000, 256, 256, ops.BNBWD_BN) and not sup(5000, 64, 128, ops.BNBWD_ROWS) and not sup(5000, 128, 64, ops.BNBWD_BN)
    assert not sup(5000, 128, 128, ops.BNBWD_BN2) and not sup(5000, 128, 128, ops.BNBWD_L2)
    assert not sup(5000, 128, 128, ops.BNBWD_BN, wgrad=False)
    c = Case(ops, dev, 513, 0.2, False, "listed")
    other = [ops.Pro(c.f1.scale, c.f1.shift, True, 0.2, seed=SEED, site=SITE_B + 1, row_offset=OFF),      # another site
             ops.Pro(c.f1.scale, c.f1.shift, True, 0.2, seed=SEED + 1, site=SITE_B, row_offset=OFF),      # another seed
             ops.Pro(c.f1.scale, c.f1.shift, True, 0.2, seed=SEED, site=SITE_B, row_offset=OFF + 1),      # another offset
             ops.Pro(c.f1.scale, c.f1.shift, True, 0.3, seed=SEED, site=SITE_B, row_offset=OFF),          # another p
             ops.Pro(c.f1.scale, c.f1.shift, True, 0.2, seed=SEED, site=SITE_B, row_offset=OFF,
                     seed_dev=torch.tensor([SEED], dtype=torch.int64, device=dev))]                      # by pointer
    small = Case(ops, dev, 512, 0.2, False, "listed")
    ops.probe_arm(64)
    try:
        for m in other:
            with pytest.raises(Exception, match="not the dropout of the X prologue"):
                c.pass_b(c.g_b, ops.MaskedDx(m))
        with pytest.raises(Exception):                 # no weight gradient in the launch
            ops.linear_bnbwd(c.g_b, c.z2, c.pro2_b, c.f2, c.W, c.sums_b, 513, masked=ops.MaskedDx(c.pro1_b))
        with pytest.raises(Exception, match="unsupported"):       # M = 512: the fused launch does not exist
            small.pass_b(small.g_b, ops.MaskedDx(small.pro1_b))
    finally:
        rows = ops.probe_read()
    assert [r for r in rows if r[1] == "linear_fwd"] == []
    # an accepted launch: the family and the mode's bits, + 1024 (weight gradient) + 8192 (masked)
    ops.probe_arm(64)
    c.handed_down(c.g_b)
    fl = [r[5] for r in ops.probe_read() if r[1] == "linear_fwd"]
    assert fl == [16 | 1024 | 8192, 16 | 256 | 1024 | 8192]


def _steps(dev, hidden, make, n_steps, flags=(True, False)):
    """n_steps captured training steps per setting of set_masked_handdown -> [(losses, pred, state, masked calls)]"""
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
    res, calls, real = [], [], (o.linear_bnbwd, o.linear_bnbwd_rows)

    def counted(fn):
        def f(*a, **kw):
            if kw.get("masked") is not None:
                calls.append((fn.__name__, kw["masked"].into is not None))
            return fn(*a, **kw)
        return f

    o.linear_bnbwd, o.linear_bnbwd_rows = counted(real[0]), counted(real[1])
    try:
        for flag in flags:
            mm.set_masked_handdown(flag)
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
        mm.set_masked_handdown(True)
        o.linear_bnbwd, o.linear_bnbwd_rows = real
    return res


def _same_steps(a, b):
    assert a[0] == b[0] and np.isfinite(a[0]).all() and torch.equal(a[1], b[1])
    assert set(a[2]) == set(b[2])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def test_graphed_training_steps_with_and_without_the_masked_handdown(dev):
    """c. two captured training steps on synth.make_graph(1) (1,834 patients, 128-d): loss, pred, every parameter and buffer."""
    from mmgnn.synth import make_graph
    on, off = _steps(dev, 128, lambda d: make_graph(1, seed=0, device=d), 2)
    # the switch switches: pass B writes, pass A accumulates, once per recorded backward
    assert len(on[3]) >= 2 and set(on[3]) == {("linear_bnbwd", False), ("linear_bnbwd_rows", True)} and off[3] == []
    _same_steps(on, off)


@pytest.mark.parametrize("what", ["d256", "m512"])
def test_shapes_without_the_masked_form_keep_the_two_tensors(dev, what):
    """d. 256-d and 512 patient rows: no masked launch is asked for, and the step is the one the switch-off path takes."""
    from mmgnn.synth import EICU, make_graph
    if what == "d256":
        hidden, make = 256, lambda d: make_graph(1, seed=0, device=d)
    else:
        hidden, make = 128, lambda d: make_graph(1, seed=0, device=d, shape=dict(EICU, patients=512, e_lab=512 * 33, e_dx=512 * 4,
                                                                                  e_med=512 * 8))
    on, off = _steps(dev, hidden, make, 1)
    assert on[3] == [] and off[3] == []
    _same_steps(on, off)
