"""The host side of the encoder-tail rider (mmgnn.model.ENC_TAIL_RIDER, ops.FwdRider): the holder protocol with the library
call replaced by a recorder, the decision of _Run.enc_tail_rider_applies, the switch and the support query -- no GPU."""
import types

import pytest
import torch

M, D = 1000, 128


@pytest.fixture()
def mods():
    import mmgnn  # noqa: F401
    from mmgnn import model as mm, ops
    return mm, ops


def test_the_query(mods):
    _, ops = mods
    sup = ops.linear_fwd_rider_supported
    assert sup(513, 128, 128, 0) and sup(513, 128, 128, 513) and sup(183400, 128, 128, 2750)
    assert not sup(512, 128, 128, 0) and not sup(5000, 256, 256, 600) and not sup(5000, 64, 128, 600)
    assert not sup(5000, 128, 128, 512) and not sup(5000, 128, 128, 1) and not sup(5000, 128, 128, 5001)


def test_the_header_documents_the_probe_flag_and_adds_no_struct(mods):
    from mmgnn import _lib
    assert "32768" in open(_lib.HEADER_PATH).read()
    assert [p[0] for p in _lib.PARAMS["mmg_linear_fwd_rider"]][-10:] == ["X_a", "pro_a", "rows", "n_sel", "W_a", "bias_a", "act_a",
                                                                        "Y_a", "epi_a", "stream"]
    assert [p[0] for p in _lib.PARAMS["mmg_linear_bnbwd_rider"]][-9:] == ["next", "a", "W_a", "dZ_a", "dX_a", "n_sel", "rows",
                                                                         "next_a", "stream"]


def test_the_switch_is_read_from_the_module(mods):
    mm, _ = mods
    assert mm.ENC_TAIL_RIDER is True
    mm.set_enc_tail_rider(False)
    try:
        assert mm.ENC_TAIL_RIDER is False
    finally:
        mm.set_enc_tail_rider(True)


@pytest.mark.parametrize("switch,train,p,dim,n_rows,n_sel,want", [
    (True, True, 0.2, 128, 5000, 600, True), (False, True, 0.2, 128, 5000, 600, False), (True, False, 0.2, 128, 5000, 600, False),
    (True, True, 0.0, 128, 5000, 600, False), (True, True, 0.2, 256, 5000, 600, False), (True, True, 0.2, 128, 512, 512, False),
    (True, True, 0.2, 128, 5000, 27, False), (True, True, 0.2, 128, 5000, None, False), (True, True, 0.2, 128, 5000, 0, True)])
def test_enc_tail_rider_applies(mods, switch, train, p, dim, n_rows, n_sel, want):
    mm, _ = mods
    lin = types.SimpleNamespace(weight=torch.zeros(dim, dim))
    run = types.SimpleNamespace(enc_tail_rider=switch, T=train, p=p, m=types.SimpleNamespace(patient_transform={8: lin}))
    rows = None if n_sel is None else torch.zeros(n_sel, dtype=torch.int64)
    assert mm._Run.enc_tail_rider_applies(run, n_rows, rows) is want


@pytest.fixture()
def stubbed(mods, monkeypatch):
    _, ops = mods
    calls = []
    monkeypatch.setattr(ops, "_p", lambda t, *a, **kw: None)
    monkeypatch.setattr(ops, "_call", lambda name, *a, **kw: calls.append((name, a)))
    pro = lambda site: ops.Pro(torch.ones(D), torch.zeros(D), 1, 0.2, 1, site)            # noqa: E731
    t = dict(za=torch.zeros(M, D), zb=torch.zeros(M, D), W=torch.zeros(D, D), b=torch.zeros(D),
             rows=torch.arange(600, dtype=torch.int64), pa=pro(1), pb=pro(3))
    return ops, calls, t


def test_the_tail_parks_and_the_dense_call_launches_both(stubbed):
    ops, calls, t = stubbed
    rider = ops.FwdRider()
    act, x0, rn = rider.park_rows(t["za"], t["pa"], t["rows"], t["W"], t["b"])
    assert calls == [] and tuple(act.shape) == (600, D) and tuple(x0.shape) == (600, D) and tuple(rn.shape) == (600,)
    out, rn_b = ops.linear_l2norm_fwd_rider(t["zb"], t["W"], t["b"], t["pb"], rider)
    assert [c[0] for c in calls] == ["mmg_linear_fwd_rider"] and len(calls[0][1]) == 18
    assert tuple(out.shape) == (M, D) and tuple(rn_b.shape) == (M,) and rider.parked is None
    rider.require_consumed()
    rider.park_rows(t["za"], t["pa"], t["rows"], t["W"], t["b"])          # a holder serves the next step as well
    ops.linear_l2norm_fwd_rider(t["zb"], t["W"], t["b"], t["pb"], rider)
    assert [c[0] for c in calls] == ["mmg_linear_fwd_rider"] * 2


def test_the_holder_never_falls_back(stubbed):
    ops, calls, t = stubbed
    rider = ops.FwdRider()
    with pytest.raises(RuntimeError, match="nothing is parked"):
        ops.linear_l2norm_fwd_rider(t["zb"], t["W"], t["b"], t["pb"], rider)
    with pytest.raises(ValueError, match="no rider"):
        rider.park_rows(t["za"], t["pa"], t["rows"][:33], t["W"], t["b"])
    assert rider.parked is None
    rider.park_rows(t["za"], t["pa"], t["rows"], t["W"], t["b"])
    with pytest.raises(RuntimeError, match="never launched"):
        rider.require_consumed()
    with pytest.raises(RuntimeError, match="already holds"):
        rider.park_rows(t["za"], t["pa"], t["rows"], t["W"], t["b"])
    with pytest.raises(RuntimeError, match="another W or bias"):
        ops.linear_l2norm_fwd_rider(t["zb"], torch.zeros(D, D), t["b"], t["pb"], rider)
    with pytest.raises(RuntimeError, match="another W or bias"):
        ops.linear_l2norm_fwd_rider(t["zb"], t["W"], None, t["pb"], rider)
    with pytest.raises(ValueError, match="another shape"):
        ops.linear_l2norm_fwd_rider(torch.zeros(M + 1, D), t["W"], t["b"], t["pb"], rider)
    assert calls == []
    ops.linear_l2norm_fwd_rider(t["zb"], t["W"], t["b"], t["pb"], rider)             # the right call still goes through
    assert [c[0] for c in calls] == ["mmg_linear_fwd_rider"]


def test_the_backward_parks_and_the_dense_call_launches_both(stubbed):
    ops, calls, t = stubbed
    fold = ops.BNFold(torch.ones(D), torch.zeros(D), torch.zeros(D), torch.ones(D), M, True)
    g, out, rn = torch.zeros(M, D), torch.zeros(M, D), torch.ones(M)
    g_a, out_a, rn_a = torch.zeros(600, D), torch.zeros(600, D), torch.ones(600)
    rider = ops.BwdRider()
    with pytest.raises(RuntimeError, match="nothing is parked"):
        ops.linear_l2bwd(g, out, rn, t["W"], rider=rider)
    with pytest.raises(ValueError, match="no rider"):
        rider.park(g_a[:33], out_a[:33], rn_a[:33], t["W"], M)
    dz_a, dx_a, sums_a = rider.park(g_a, out_a, rn_a, t["W"], M, stats=(t["za"], t["rows"], t["pa"], fold))
    assert calls == [] and tuple(dz_a.shape) == (600, D) and tuple(dx_a.shape) == (600, D) and tuple(sums_a.shape) == (2, D)
    with pytest.raises(RuntimeError, match="never launched"):
        rider.require_consumed()
    with pytest.raises(RuntimeError, match="already holds"):
        rider.park(g_a, out_a, rn_a, t["W"], M)
    with pytest.raises(RuntimeError, match="another W"):
        ops.linear_l2bwd(g, out, rn, torch.zeros(D, D), rider=rider)
    with pytest.raises(ValueError, match="excludes the fused weight gradient"):
        ops.linear_l2bwd(g, out, rn, t["W"], wgrad=ops.FusedWgrad(t["zb"], t["pb"]), rider=rider)
    assert calls == []
    dz, dx = ops.linear_l2bwd(g, out, rn, t["W"], rider=rider)
    assert [c[0] for c in calls] == ["mmg_linear_bnbwd_rider"] and len(calls[0][1]) == 15 and rider.parked is None
    assert tuple(dz.shape) == (M, D) and tuple(dx.shape) == (M, D)
    rider.require_consumed()


def test_the_query_of_the_backward(mods):
    _, ops = mods
    sup = ops.linear_bnbwd_rider_supported
    assert sup(513, 128, 128, 0) and sup(513, 128, 128, 513) and sup(183400, 128, 128, 2750)
    assert not sup(512, 128, 128, 0) and not sup(5000, 256, 256, 600) and not sup(5000, 128, 128, 512)


@pytest.mark.parametrize("switch,train,sites,fused,dim,n_rows,n_sel,live,want", [
    (True, True, ("enc2",), True, 128, 5000, 600, True, True), (False, True, ("enc2",), True, 128, 5000, 600, True, False),
    (True, False, ("enc2",), True, 128, 5000, 600, True, False), (True, True, (), True, 128, 5000, 600, True, False),
    (True, True, (), False, 128, 5000, 600, True, True), (True, True, ("enc2",), True, 256, 5000, 600, True, False),
    (True, True, ("enc2",), True, 128, 512, 512, True, False), (True, True, ("enc2",), True, 128, 5000, 27, True, False),
    (True, True, ("enc2",), True, 128, 5000, 600, False, False)])
def test_enc_tail_bwd_rider_applies(mods, switch, train, sites, fused, dim, n_rows, n_sel, live, want):
    """the dense launch must be the one without the fused weight gradient: the "enc2" site rides, or the fused form is off"""
    mm, _ = mods
    run = types.SimpleNamespace(enc_tail_rider=switch, T=train, next_bn_sites=sites, fused_wgrad=fused,
                                W=lambda name: torch.zeros(dim, dim))
    enc_b = types.SimpleNamespace(rows=None, z2=torch.zeros(n_rows, dim))
    enc_a = types.SimpleNamespace(rows=torch.zeros(n_sel, dtype=torch.int64), act=torch.zeros(n_sel, dim))
    g = torch.zeros(1) if live else None
    assert mm._Run.enc_tail_bwd_rider_applies(run, enc_b, g, enc_a, (enc_a.rows, g)) is want
    assert mm._Run.enc_tail_bwd_rider_applies(run, enc_a, g, enc_a, (enc_a.rows, g)) is False      # a compact pass B
