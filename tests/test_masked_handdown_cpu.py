"""The host side of the masked hand-down (mmgnn.model.MASKED_HANDDOWN): the decision of _Run.masked_handdown_applies, the
glue of the two-pass branch of run_backward's helpers with the ops entry points replaced by recorders, and the shape
rules of mmg_linear_bnbwd_masked_supported -- no GPU."""
from dataclasses import replace

import pytest
import torch

M, D = 600, 128
PT = "patient_transform"


def make(mm, ops, **over):
    """-> (run, pass B, state B, pass A, state A) for which the hand-down applies; `over` changes one thing."""
    fold = lambda tr=True: ops.BNFold(torch.ones(D), torch.zeros(D), torch.zeros(D), torch.ones(D), M, tr)     # noqa: E731
    z1, z2, E = torch.zeros(M, D), torch.zeros(M, D), torch.zeros(M, D)
    pro = lambda site: ops.Pro(torch.ones(D), torch.zeros(D), over.get("act", 1), 0.2, 1, site)                  # noqa: E731
    f1, f2 = fold(over.get("training", True)), fold()
    rows = torch.tensor([0, 5, M - 1])
    row_pos = torch.full((M,), -1, dtype=torch.int32)
    row_pos[rows] = torch.arange(3, dtype=torch.int32)
    enc_b = mm._EncPass(E, z1, z2, z2, torch.ones(M), f1, f2, pro(3), pro(7))
    enc_a = mm._EncPass(E, z1, z2, z2, torch.ones(M), f1, f2, pro(5), pro(9), rows, torch.zeros(3, D), row_pos)
    if over.get("dense_a"):
        enc_a = replace(enc_a, rows=None, act=None, row_pos=None)
    run = object.__new__(mm._Run)
    run.masked_handdown = over.get("switch", True)
    run.fused_wgrad = over.get("fused_wgrad", True)
    run.next_bn_sites = frozenset(over.get("sites", {"heads", "conv", "enc2"}))
    d = over.get("dim", D)
    ename = f"embeddings.{mm.ROW_TYPE}.weight"
    run.params = {f"{PT}.4.weight": torch.nn.Parameter(torch.zeros(d, d)), f"{PT}.0.weight": torch.nn.Parameter(torch.zeros(d, d)),
                  ename: torch.nn.Parameter(torch.zeros(M, d), requires_grad=over.get("emb_grad", True))}
    run.grads, run.comm = ({ename: torch.zeros(M, d)} if over.get("emb_taken") else {}), None
    state = (torch.zeros(M, D), torch.zeros(2, D, dtype=torch.float64))
    return run, enc_b, state, enc_a, (torch.zeros(3, D), state[1])


@pytest.fixture()
def mods():
    import mmgnn  # noqa: F401
    from mmgnn import model as mm, ops
    return mm, ops


def test_the_query_follows_the_fused_launch(mods):
    mm, ops = mods
    sup = ops.linear_bnbwd_masked_supported
    assert sup(513, 128, 128, ops.BNBWD_BN) and sup(183400, 128, 128, ops.BNBWD_ROWS)
    assert not sup(512, 128, 128, ops.BNBWD_BN) and not sup(5000, 256, 256, ops.BNBWD_ROWS) and not sup(5000, 64, 128, ops.BNBWD_BN)
    assert not sup(5000, 128, 128, ops.BNBWD_BN2) and not sup(5000, 128, 128, ops.BNBWD_L2) and not sup(5000, 128, 128, 4)
    assert not sup(5000, 128, 128, ops.BNBWD_BN, wgrad=False)


@pytest.mark.parametrize("over,want", [
    ({}, True),
    ({"switch": False}, False),
    ({"fused_wgrad": False}, False),                       # a producer that is not the fused launch
    ({"sites": {"heads", "conv", "enc2", "enc1"}}, False),  # the "enc1" next-BN site requested
    ({"act": 2}, False),                                   # an activation other than none or ReLU
    ({"act": 0}, True),
    ({"training": False}, False),                          # the row-list kernel has the training form only
    ({"dense_a": True}, False),                            # pass A dense: not the (MODE 0 write, MODE 3 accumulate) pair
    ({"dim": 256}, False),
    ({"emb_grad": False}, False),                          # the consumer would not be the fused launch
    ({"emb_taken": True}, False),
])
def test_masked_handdown_applies(mods, over, want):
    mm, ops = mods
    run, enc_b, sb, enc_a, sa = make(mm, ops, **over)
    assert run.masked_handdown_applies(enc_b, sb, enc_a, sa) is want
    if want:                                               # only one pass live: today's path
        assert run.masked_handdown_applies(enc_b, None, enc_a, sa) is False
        assert run.masked_handdown_applies(enc_b, sb, enc_a, None) is False


def test_the_switch_is_read_from_the_module(mods):
    mm, _ = mods
    assert mm.MASKED_HANDDOWN is True
    mm.set_masked_handdown(False)
    try:
        assert mm.MASKED_HANDDOWN is False
    finally:
        mm.set_masked_handdown(True)


def test_producers_and_consumer_as_the_two_pass_branch_calls_them(mods, monkeypatch):
    """pass B: linear_bnbwd with MaskedDx(pro1 of B); pass A: linear_bnbwd_rows with MaskedDx(pro1 of A, into = B's tensor);
    then bn_bwd_stats and linear_bnbwd on that ONE tensor with B's first prologue at p = 0."""
    mm, ops = mods
    run, enc_b, sb, enc_a, sa = make(mm, ops)
    run.pending, run.partial, run.wgrad_jobs = {}, set(), []
    calls = []

    def bnbwd(name):
        def f(*a, **kw):
            calls.append((name, a, kw))
            fw, mk = kw["wgrad"], kw.get("masked")
            fw.dW, fw.db = torch.zeros(D, D), torch.zeros(D)
            a[-2].fill_(1.0), a[-1].fill_(2.0)
            return None, (mk.into if mk is not None and mk.into is not None else torch.zeros(M, D))
        return f

    monkeypatch.setattr(ops, "linear_bnbwd", bnbwd("linear_bnbwd"))
    monkeypatch.setattr(ops, "linear_bnbwd_rows", bnbwd("linear_bnbwd_rows"))
    monkeypatch.setattr(ops, "bn_bwd_stats", lambda g, y, pro, fold: (calls.append(("bn_bwd_stats", (g, y, pro, fold), {})),
                                                                      torch.zeros(2, D, dtype=torch.float64))[1])
    run.params.update({f"{PT}.{i}.{w}": torch.nn.Parameter(torch.zeros(D)) for i in (1, 5) for w in ("weight", "bias")})
    gs = run.enc_bwd_b(enc_b, sb, masked=ops.MaskedDx(enc_b.pro1))
    gs2 = run.enc_bwd_b(enc_a, sa, masked=ops.MaskedDx(enc_a.pro1, into=gs))
    assert gs2 is gs
    run.enc_bwd_shared_masked(enc_b, gs)
    assert [c[0] for c in calls] == ["linear_bnbwd", "linear_bnbwd_rows", "bn_bwd_stats", "linear_bnbwd"]
    mb, ma = calls[0][2]["masked"], calls[1][2]["masked"]
    assert mb.pro is enc_b.pro1 and mb.into is None and ma.pro is enc_a.pro1 and ma.into is gs
    assert calls[0][2]["wgrad"].pro is enc_b.pro1 and calls[1][2]["wgrad"].pro is enc_a.pro1       # the mask IS the X prologue's
    assert calls[0][2].get("next_bn") is None and calls[1][2].get("next_bn") is None
    g, y, pro, fold = calls[2][1]
    assert g is gs and y is enc_b.z1 and fold is enc_b.f1
    assert pro.p == 0.0 and pro.relu == enc_b.pro1.relu and pro.scale is enc_b.pro1.scale and pro.shift is enc_b.pro1.shift
    last = calls[3]
    assert last[1][0] is gs and last[1][1] is enc_b.z1 and last[1][2].p == 0.0 and "masked" not in last[2]
    assert last[2]["wgrad"].x is enc_b.E and last[2]["wgrad"].pro is None
    assert f"embeddings.{mm.ROW_TYPE}.weight" in run.grads and f"{PT}.0.weight" in run.grads and f"{PT}.4.weight" in run.grads
    # a producer without the fused weight gradient is an error, not a quiet fall-back to an unmasked tensor
    run.fused_wgrad = False
    with pytest.raises(RuntimeError):
        run.enc_bwd_b(enc_b, sb, masked=ops.MaskedDx(enc_b.pro1))
