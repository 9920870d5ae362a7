"""The decision table of _Run.bn_lin_bwd -- the backward of "BatchNorm, then the linear in front of it" that the encoder
and the GNN self-loop share -- and of the BatchNorm step counters, on the host: a _Run made with object.__new__, CPU
tensors, the ops entry points replaced by recorders that return tensors of the right shapes."""
import itertools
from types import SimpleNamespace

import pytest
import torch

M, N, K = 6, 4, 3            # dz is [M, K], the linear maps N -> K: W is [K, N]
FORMS = {"plain": "linear_bnbwd", "rows": "linear_bnbwd_rows", "two": "linear_bnbwd2", "l2": "linear_l2bwd"}


class Recorder:
    """Stand-ins for the ops entry points bn_lin_bwd can reach; .calls = [(name, args, kwargs)] in call order."""

    def __init__(self, monkeypatch, ops, form_ok, wgrad_ok):
        self.calls = []
        for name in FORMS.values():
            monkeypatch.setattr(ops, name, lambda *a, _n=name, **kw: self.bnbwd(_n, a, kw))
        monkeypatch.setattr(ops, "linear_wgrad", self.linear_wgrad)
        monkeypatch.setattr(ops, "bn_bwd_stats", self.bn_bwd_stats)
        monkeypatch.setattr(ops, "linear_bnbwd_supported",
                            lambda m, n, k, mode=ops.BNBWD_BN, wgrad=False: (m, n, k) == (M, N, K) and (wgrad_ok if wgrad else form_ok))

    def names(self):
        return [c[0] for c in self.calls]

    def bnbwd(self, name, a, kw):
        self.calls.append((name, a, kw))
        if name != "linear_l2bwd":                 # (..., fold, W, sums, count, dbeta, dgamma): the kernel writes the last two
            dbeta, dgamma = a[-2], a[-1]
            if dbeta is not None:
                dbeta.fill_(1.0), dgamma.fill_(2.0)
        fw = kw.get("wgrad")
        if fw is not None:                         # what ops._fused_wgrad leaves on the descriptor
            acc = fw.accumulate and fw.out is not None
            fw.dW = fw.out if fw.out is not None else torch.zeros(K, N)
            fw.db = (fw.bias_out if fw.bias_out is not None and acc else torch.zeros(K)) if fw.with_bias else None
        dz = torch.zeros(M, K) if fw is None or fw.keep_dz else None
        out = (dz, torch.zeros(M, N))
        return out + (torch.full((2, N), 7.0, dtype=torch.float64),) if kw.get("next_bn") is not None else out

    def linear_wgrad(self, dy, x, pro=None, out=None, accumulate=False, with_bias=False, bias_out=None, defer=None):
        self.calls.append(("linear_wgrad", (dy, x, pro), dict(out=out, accumulate=accumulate, with_bias=with_bias,
                                                              bias_out=bias_out, defer=defer)))
        dW = out if out is not None else torch.zeros(K, N)
        return (dW, bias_out if bias_out is not None else torch.zeros(K)) if with_bias else dW

    def bn_bwd_stats(self, g, y, pro, fold):
        self.calls.append(("bn_bwd_stats", (g, y, pro, fold), {}))
        return torch.full((2, y.shape[1]), 5.0, dtype=torch.float64)


def make_run(mm, fused_wgrad=True):
    run = object.__new__(mm._Run)
    run.grads, run.pending, run.partial, run.wgrad_jobs = {}, {}, set(), []
    run.fused_wgrad, run.comm = fused_wgrad, None
    run.acc_log = []
    real_acc = mm._Run.acc.__get__(run)

    def acc(name, g, partial=False):
        if not isinstance(name, tuple):
            run.acc_log.append((name, partial))
        real_acc(name, g, partial)

    run.acc = acc
    return run


def fold_of(ops, kind):
    if kind == "none":
        return None
    return ops.BNFold(torch.ones(K), torch.zeros(K), torch.zeros(K), torch.ones(K), M, kind == "train")


def block_args(ops, form, fold, sums):
    g, y, ypro = torch.ones(M, K), torch.ones(M, K), ops.Pro(None, None, True, 0.2, 1, 3)
    if form == "plain":
        return g, y, ypro, fold, sums, False
    if form == "rows":
        return torch.ones(2, K), y, ypro, fold, sums, torch.tensor([0, -1, -1, 1, -1, -1], dtype=torch.int32)
    if form == "two":
        return g, y, ypro, fold, sums, torch.ones(M, K), ops.Pro(None, None, True, 0.2, 1, 5)
    return g, y, torch.ones(M)                     # l2: (g, normalised output, reciprocal norms)


FOLDS = {"plain": ("train", "eval", "none"), "rows": ("train", "eval"), "two": ("train", "eval"), "l2": ("none",)}
CASES = [(form, offer, fold, present)
         for form, offer, present in itertools.product(FORMS, ("offered", "unsupported", "switched_off", "next_bn"),
                                                       ("absent", "both", "weight_only"))
         for fold in FOLDS[form] if not (form == "two" and offer == "next_bn")]     # (that kernel has no such epilogue)


@pytest.mark.parametrize("form,offer,fold_kind,present", CASES)
def test_bn_lin_bwd_decisions(monkeypatch, form, offer, fold_kind, present):
    import mmgnn  # noqa: F401
    from mmgnn import model as mm, ops
    rec = Recorder(monkeypatch, ops, form_ok=True, wgrad_ok=offer != "unsupported")
    run = make_run(mm, fused_wgrad=offer != "switched_off")
    fold = fold_of(ops, fold_kind)
    sums = torch.tensor([[1.0] * K, [3.0] * K], dtype=torch.float64) if fold is not None else None
    x, pro, W = torch.ones(M, N), ops.Pro(None, None, True, 0.2, 1, 2), torch.ones(K, N)
    gw0, gb0 = torch.zeros(K, N), torch.zeros(K)
    if present != "absent":
        run.grads["lin.weight"] = gw0
    if present == "both":
        run.grads["lin.bias"] = gb0
    below = mm._NextStats(torch.ones(M, N), ops.BNFold(*[torch.ones(N)] * 4, M, True)) if offer == "next_bn" else None
    bn_prefix = "bn" if fold is not None else None
    res = run.bn_lin_bwd(form, block_args(ops, form, fold, sums), bn_prefix, x, pro, "lin.weight", "lin.bias", W,
                         next_bn=below, keep_dz=False)
    if form == "rows" and fold_kind == "eval":         # the row-list kernel only has the training-statistics form
        assert res is None and rec.calls == [] and run.acc_log == []
        return
    fused = offer == "offered"
    # ---- which ops functions ran, and how often
    assert rec.names() == [FORMS[form]] + ([] if fused else ["linear_wgrad"])
    name, a, kw = rec.calls[0]
    # ---- the fused weight gradient, as fused_wgrad_for decides it
    fw = kw["wgrad"]
    both = present == "both"
    if fused:
        assert fw.x is x and fw.pro is pro and fw.with_bias and fw.defer is run.wgrad_jobs and fw.keep_dz is False
        assert fw.out is (gw0 if both else None) and fw.accumulate is both and fw.bias_out is (gb0 if both else None)
        assert res[0] is None                          # dz is not written
    else:
        assert fw is None and res[0] is not None
        _, (dy, wx, wpro), wkw = rec.calls[1]          # lin_bwd(dz, x, pro, ..., need_dx=False): the same rule, one launch later
        assert dy is res[0] and wx is x and wpro is pro and wkw["with_bias"] and wkw["defer"] is run.wgrad_jobs
        assert wkw["out"] is (gw0 if both else None) and wkw["accumulate"] is both and wkw["bias_out"] is (gb0 if both else None)
    assert res[1].shape == (M, N)
    # ---- the next BatchNorm's statistics ride along, with the linear's own prologue
    if below is not None:
        nb = kw["next_bn"]
        assert nb.y is below.y and nb.pro is pro and nb.fold is below.fold and nb.sums is None
        assert below.n == 1 and float(below.sums[0, 0]) == 7.0
    else:
        assert kw.get("next_bn") is None
    # ---- parameter gradients: the BatchNorm's (whole), then the linear's (per-shard partial sums)
    bn_names = [("bn.bias", False), ("bn.weight", False)] if fold is not None else []
    assert run.acc_log == bn_names + [("lin.weight", True), ("lin.bias", True)]
    assert run.partial == {"lin.weight", "lin.bias"}
    if form != "l2":
        k_sums, k_count, k_dbeta, k_dgamma = a[-4:]
        if fold_kind == "train":                       # the kernel converts the sums and writes d beta / d gamma
            assert k_sums is sums and k_count == M and k_dbeta is not None
            assert torch.equal(run.grads["bn.bias"], torch.full((K,), 1.0)) and \
                torch.equal(run.grads["bn.weight"], torch.full((K,), 2.0))
        else:
            assert k_sums is None and k_count == 1.0 and k_dbeta is None and k_dgamma is None
        if fold_kind == "eval":                        # running statistics: the sums ARE the gradients
            assert torch.equal(run.grads["bn.bias"], sums[0].float()) and torch.equal(run.grads["bn.weight"], sums[1].float())
    if present == "weight_only":                       # a fresh gradient beside an existing one is summed at the end
        assert [g.shape for g in run.pending["lin.weight"]] == [(K, N)] and "lin.bias" not in run.pending
    else:
        assert run.pending == {}


@pytest.mark.parametrize("form,why", [("plain", "shape"), ("rows", "shape"), ("two", "shape"), ("plain", "no_gradient"),
                                      ("plain", "activation"), ("rows", "no_positions")])
def test_bn_lin_bwd_returns_none_before_any_call(monkeypatch, form, why):
    import mmgnn  # noqa: F401
    from mmgnn import _lib, model as mm, ops
    rec = Recorder(monkeypatch, ops, form_ok=why != "shape", wgrad_ok=True)
    run = make_run(mm)
    fold = fold_of(ops, "train")
    args = list(block_args(ops, form, fold, torch.ones(2, K, dtype=torch.float64)))
    if why == "no_gradient":
        args[0] = None
    if why == "activation":                            # the fused kernels stage ReLU only
        args[2] = ops.Pro(None, None, _lib.MMG_ACT_ELU, 0.0, 1, 3)
    if why == "no_positions":
        args[5] = None
    below = mm._NextStats(torch.ones(M, N), ops.BNFold(*[torch.ones(N)] * 4, M, True)) if form != "two" else None
    res = run.bn_lin_bwd(form, tuple(args), "bn", torch.ones(M, N), None, "lin.weight", "lin.bias", torch.ones(K, N),
                         next_bn=below)
    assert res is None and rec.calls == [] and run.acc_log == [] and run.grads == {}
    assert below is None or (below.n == 0 and below.sums is None)


def test_bn_lin_bwd_takes_missing_statistics_itself(monkeypatch):
    """plain form without sums: the statistics pass runs first; a next-BatchNorm holder that does not ride (ride=False)
    gets the separate pass over dx right behind the kernel, before the weight gradient; names given as a tuple share
    the gradient."""
    import mmgnn  # noqa: F401
    from mmgnn import model as mm, ops
    rec = Recorder(monkeypatch, ops, form_ok=True, wgrad_ok=False)
    run = make_run(mm)
    fold = fold_of(ops, "train")
    below = mm._NextStats(torch.ones(M, N), ops.BNFold(*[torch.ones(N)] * 4, M, True), ride=False)
    g, y, ypro = torch.ones(M, K), torch.ones(M, K), ops.Pro(None, None, True)
    dz, dx = run.bn_lin_bwd("plain", (g, y, ypro, fold, None, True), "bn", torch.ones(M, N), None, ("a.w", "b.w"),
                            ("a.b", "b.b"), torch.ones(K, N), next_bn=below, keep_dz=True)
    assert rec.names() == ["bn_bwd_stats", "linear_bnbwd", "bn_bwd_stats", "linear_wgrad"]
    assert rec.calls[0][1][0] is g and rec.calls[0][1][1] is y and rec.calls[1][2]["next_bn"] is None
    assert rec.calls[2][1][0] is dx and rec.calls[2][1][1] is below.y and below.n == 1 and float(below.sums[0, 0]) == 5.0
    assert run.acc_log == [("bn.bias", False), ("bn.weight", False), ("a.w", True), ("b.w", True), ("a.b", True), ("b.b", True)]
    assert run.grads["a.w"] is run.grads["b.w"] and run.grads["a.b"] is run.grads["b.b"] and run.pending == {}


def test_count_bn_is_the_one_place_that_advances_the_step_counters(monkeypatch):
    """Two bn_fold calls (one whose producer already folded, one that folds here) and one grouped small-vocab epilogue on
    the same BatchNorm module leave ONE _nbt entry whose increment is the sum, all through count_bn."""
    import mmgnn  # noqa: F401
    from mmgnn import model as mm, ops
    D, n_lab = 4, 3
    mod = torch.nn.BatchNorm1d(D)
    folded = ops.BNFold(*[torch.ones(D)] * 4, 5, True)
    monkeypatch.setattr(ops, "col_reduce2", lambda y: torch.zeros(2, y.shape[1], dtype=torch.float64))
    monkeypatch.setattr(ops, "bn_finalize", lambda *a: folded)
    monkeypatch.setattr(ops, "scatter_rows", lambda *a: None)
    monkeypatch.setattr(ops, "small_fwd_group", lambda probs, grouped=True: [p.out for p in probs])
    monkeypatch.setattr(ops, "small_bn_act_group", lambda items, training: [(torch.zeros_like(y), folded) for y, _, _ in items])
    et = ("patient", "has_lab", "lab")
    rel = SimpleNamespace(other="lab", edge_type=et, n_cols=n_lab, rowptr=None, col=None, inv_col=None, simple=True, mask_t=None)
    run = object.__new__(mm._Run)
    run.plan = SimpleNamespace(n_rows=5, node_types=["patient", "lab"], row_offset=0, rels_into_patient=lambda: [],
                               rels_from_patient=lambda: [rel])
    run.m = SimpleNamespace(num_layers=2, use_batch_norm=True, batch_norms=[{"lab": mod}], _act_code=1)
    run.T, run.p, run.seed, run.seed_dev, run.D, run.dev = True, 0.2, 1, None, D, torch.device("cpu")
    run.comm, run.overlap, run.lazy_final, run._nbt = None, False, False, {}
    conv = f"convs.0.convs.{mm._mangle(et)}"
    run.params = {f"{conv}.{n}": torch.nn.Parameter(torch.zeros(D, D) if n.endswith("weight") else torch.zeros(D))
                  for n in ("lin_l.weight", "lin_l.bias", "lin_r.weight")}
    counted = []
    real = mm._Run.count_bn.__get__(run)
    run.count_bn = lambda m, n: (counted.append(n), real(m, n))[1]
    assert run.bn_fold(torch.zeros(5, D), mod, n_updates=2, sums=folded) is folded
    assert run.bn_fold(torch.zeros(5, D), mod, n_updates=2) is folded
    out, rec = run.layer_fwd(0, {"patient": torch.zeros(5, D), "lab": torch.zeros(n_lab, D)})
    assert list(out) == ["lab"] and rec.folds["lab"] is folded
    assert counted == [2, 2, 1]
    assert list(run._nbt) == [id(mod)] and run._nbt[id(mod)][0] is mod.num_batches_tracked and run._nbt[id(mod)][1] == 5
