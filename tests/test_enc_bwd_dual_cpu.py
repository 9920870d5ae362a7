"""The host side of the dual backward launch (mmgnn.model.DUAL_ENC_BWD, ops.DualBwd): the holder protocol of
ops._linear_bnbwd with the library call replaced by a recorder, the decision of _Run.dual_enc_bwd_applies under each
switch and support combination, the switch and the support query -- no GPU."""
import pytest
import torch

import test_masked_handdown_cpu as H

M, D, PT = H.M, H.D, H.PT


@pytest.fixture()
def mods():
    import mmgnn  # noqa: F401
    from mmgnn import model as mm, ops
    return mm, ops


def test_the_query_follows_the_masked_launches(mods):
    _, ops = mods
    sup = ops.linear_bnbwd_dual_supported
    assert sup(513, 128, 128) and sup(183400, 128, 128)
    assert not sup(512, 128, 128) and not sup(5000, 256, 256) and not sup(5000, 64, 128) and not sup(5000, 128, 64)


def test_the_switch_is_read_from_the_module(mods):
    mm, _ = mods
    assert mm.DUAL_ENC_BWD is True
    mm.set_dual_enc_bwd(False)
    try:
        assert mm.DUAL_ENC_BWD is False
    finally:
        mm.set_dual_enc_bwd(True)


@pytest.mark.parametrize("switch,dim,rows,want", [(True, D, M, True), (False, D, M, False), (True, 256, M, False),
                                                  (True, D, 512, False)])
def test_dual_enc_bwd_applies(mods, switch, dim, rows, want):
    mm, ops = mods
    run, enc_b, _, _, _ = H.make(mm, ops, dim=dim)
    run.dual_enc_bwd = switch
    if rows != M:
        enc_b = H.replace(enc_b, z2=torch.zeros(rows, D))
    assert run.dual_enc_bwd_applies(enc_b) is want


@pytest.fixture()
def stubbed(mods, monkeypatch):
    """ops with device pointers and the library call replaced: -> (ops, the recorded calls, inputs of one layer)"""
    _, ops = mods
    calls = []
    monkeypatch.setattr(ops, "_p", lambda t, *a, **kw: None)
    monkeypatch.setattr(ops, "_call", lambda name, *a, **kw: calls.append((name, a)))
    fold = ops.BNFold(torch.ones(D), torch.zeros(D), torch.zeros(D), torch.ones(D), M, True)
    pro = lambda site: ops.Pro(torch.ones(D), torch.zeros(D), 1, 0.2, 1, site)            # noqa: E731
    t = dict(g=torch.zeros(M, D), y=torch.zeros(M, D), x=torch.zeros(M, D), W=torch.zeros(D, D), fold=fold,
             sums=torch.zeros(2, D, dtype=torch.float64), g_rows=torch.zeros(3, D),
             row_pos=torch.full((M,), -1, dtype=torch.int32), pro2=(pro(7), pro(9)), pro1=(pro(3), pro(5)))
    return ops, calls, t


def write(ops, t, pair, defer=None, W=None):
    fw = ops.FusedWgrad(t["x"], t["pro1"][0], with_bias=True, keep_dz=False, defer=defer)
    return ops.linear_bnbwd(t["g"], t["y"], t["pro2"][0], t["fold"], t["W"] if W is None else W, t["sums"], M, wgrad=fw,
                            masked=ops.MaskedDx(t["pro1"][0], pair=pair)), fw


def accumulate(ops, t, pair, into, defer=None, W=None):
    fw = ops.FusedWgrad(t["x"], t["pro1"][1], with_bias=True, keep_dz=False, defer=defer)
    return ops.linear_bnbwd_rows(t["g_rows"], t["row_pos"], t["y"], t["pro2"][1], t["fold"], t["W"] if W is None else W,
                                 t["sums"], M, wgrad=fw, masked=ops.MaskedDx(t["pro1"][1], into=into, pair=pair)), fw


def test_the_write_parks_and_the_accumulate_launches_both(stubbed):
    ops, calls, t = stubbed
    pair, jobs = ops.DualBwd(), []
    (dz, dx), fb = write(ops, t, pair, jobs)
    assert calls == [] and dz is None and tuple(dx.shape) == (M, D) and pair.parked is not None
    assert fb.dW is not None and fb.db is not None and len(jobs) == 1 and jobs[0][2] is fb.dW      # B's job in its usual place
    (dz2, dx2), fa = accumulate(ops, t, pair, dx, jobs)
    assert dx2 is dx and dz2 is None and pair.parked is None
    assert [c[0] for c in calls] == ["mmg_linear_bnbwd_dual"] and len(calls[0][1]) == 11
    assert len(jobs) == 2 and jobs[1][2] is fa.dW and jobs[0][0] is not jobs[1][0]                 # B's series before A's
    pair.require_consumed()
    # a holder serves the next step's pair as well
    (_, dx3), _ = write(ops, t, pair)
    accumulate(ops, t, pair, dx3)
    assert [c[0] for c in calls] == ["mmg_linear_bnbwd_dual"] * 2


def test_without_a_holder_both_calls_are_the_masked_launches(stubbed):
    ops, calls, t = stubbed
    (_, dx), _ = write(ops, t, None)
    (_, dx2), _ = accumulate(ops, t, None, dx)
    assert dx2 is dx and [c[0] for c in calls] == ["mmg_linear_bnbwd_masked"] * 2
    assert [c[1][-2] for c in calls] == [0, 1]                       # write, accumulate


def test_the_holder_never_falls_back(stubbed):
    ops, calls, t = stubbed
    pair = ops.DualBwd()
    with pytest.raises(RuntimeError, match="no parked write"):
        accumulate(ops, t, pair, torch.zeros(M, D))
    (_, dx), _ = write(ops, t, pair)
    with pytest.raises(RuntimeError, match="never launched"):
        pair.require_consumed()
    with pytest.raises(RuntimeError, match="never launched"):        # a second write on a holder that still holds one
        write(ops, t, pair)
    with pytest.raises(ValueError, match="not that of the parked write"):
        accumulate(ops, t, pair, torch.zeros(M, D))
    with pytest.raises(ValueError, match="not that of the parked write"):
        accumulate(ops, t, pair, dx, W=torch.zeros(D, D))
    with pytest.raises(ValueError, match="pairs a linear_bnbwd write"):                  # the modes swapped
        fw = ops.FusedWgrad(t["x"], t["pro1"][0], with_bias=True, keep_dz=False)
        ops.linear_bnbwd(t["g"], t["y"], t["pro2"][0], t["fold"], t["W"], t["sums"], M, wgrad=fw,
                         masked=ops.MaskedDx(t["pro1"][0], into=dx, pair=pair))
    assert calls == []
    small = ops.DualBwd()
    with pytest.raises(ValueError, match="does not cover"):
        fw = ops.FusedWgrad(t["x"][:512], t["pro1"][0], with_bias=True, keep_dz=False)
        ops.linear_bnbwd(t["g"][:512], t["y"][:512], t["pro2"][0], t["fold"], t["W"], t["sums"], 512, wgrad=fw,
                         masked=ops.MaskedDx(t["pro1"][0], pair=small))
    assert calls == [] and small.parked is None
    accumulate(ops, t, pair, dx)                                     # the right call still goes through
    assert [c[0] for c in calls] == ["mmg_linear_bnbwd_dual"]
