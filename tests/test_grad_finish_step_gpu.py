"""The training step with the gradient-finish launch (model.set_grad_finish) and the one-launch state advance
(train.set_step_advance) switched on and off: everything a step leaves behind must be the same BITS -- every parameter,
both Adam moment buckets, loss, predictions, the step counter, both words of the seed state, every num_batches_tracked and
every BatchNorm running statistic (the last three are in the model's state_dict)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = {"model": {"architecture": "RGCN", "hidden_dim": 128, "num_layers": 2, "dropout": 0.2, "use_batch_norm": True,
                 "activation": "relu"}}
LAB = ("patient", "has_lab", "lab")
_SETUP, _RUNS = {}, {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _setup(dev):
    """The graph, its plan and the pair set: built once, never changed."""
    if not _SETUP:
        import mmgnn  # noqa: F401
        from mmgnn.data import build_plan
        from mmgnn.synth import make_graph
        g = make_graph(1, seed=0, device=dev)
        ei = g[LAB].edge_index
        E = ei.shape[1]
        tr = torch.randperm(E, generator=torch.Generator(device=dev).manual_seed(42), device=dev)[: int(0.7 * E)].sort().values
        pi, li = ei[0][tr].contiguous(), ei[1][tr].contiguous()
        y = g[LAB].edge_attr[tr].squeeze(-1).contiguous()
        sup = torch.rand(tr.numel(), generator=torch.Generator(device=dev).manual_seed(1234), device=dev) < 0.2
        _SETUP.update(g=g, plan=build_plan(g, dev, use_cache=False), pi=pi, li=li, y=y, sup=sup,
                      wlab=torch.ones(int(g["lab"].num_nodes), device=dev))
    return _SETUP


def _steps(dev, on, sites=None, threshold=None, step_advance=None):
    """Two captured training steps -> everything they leave behind.  on: set_grad_finish, and set_step_advance unless
    step_advance says otherwise."""
    import mmgnn.model as mm
    import mmgnn.train as mt
    from mmgnn.model import build_model
    from mmgnn.optim import Adam
    key = (on, sites, threshold, step_advance)
    if key in _RUNS:                         # (the switched-off reference serves two tests)
        return _RUNS[key]
    s = _setup(dev)
    keep = mm.NEXT_BN_SITES
    mm.set_grad_finish(on)
    mt.set_step_advance(on if step_advance is None else step_advance)
    if sites is not None:
        mm.set_next_bn(sites)
    try:
        torch.manual_seed(42)
        model = build_model(CFG, (s["g"].node_types, s["g"].edge_types), None).to(dev)
        model._init_embeddings(s["g"])
        if threshold is not None:
            model.degree_threshold = threshold
        opt = Adam([q for k, q in model.named_parameters() if not k.startswith("embeddings.")], lr=1e-2)
        step = mt.PiecewiseGraphedTrainStep(model, s["plan"], s["pi"], s["li"], s["y"], s["wlab"], opt, s["sup"], None)
        losses = [step.step().clone() for _ in range(2)]
        torch.cuda.synchronize()
        out = {f"state.{k}": v.clone() for k, v in model.state_dict().items()}
        out.update({f"grad.{k}": p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
        fl = opt._flat[0]
        out.update(adam_m=fl["m"].clone(), adam_v=fl["v"].clone(), adam_step=fl["step"].clone(), params=fl["p"].clone(),
                   seed=model._seed_dev.clone(), pred=step.pred.clone(), loss0=losses[0], loss1=losses[1])
        _RUNS[key] = out
        return out
    finally:
        mm.set_grad_finish(True)
        mt.set_step_advance(True)
        mm.set_next_bn(keep)


def _check(a, b):
    assert set(a) == set(b)
    for k in a:
        assert same(a[k], b[k]), k
    assert float(a["adam_step"]) == 2.0 and any(k.endswith("num_batches_tracked") for k in a)
    assert all(int(v) > 0 for k, v in a.items() if k.endswith("num_batches_tracked"))


def test_two_training_steps_are_bitwise_the_same_with_the_default_sites(dev):
    _check(_steps(dev, True), _steps(dev, False))


@pytest.mark.parametrize("sites", [(), ("heads", "conv", "enc2", "enc1")])
def test_two_training_steps_are_bitwise_the_same_without_and_with_every_next_bn_site(dev, sites):
    _check(_steps(dev, True, sites=sites), _steps(dev, False, sites=sites))


def test_two_training_steps_with_a_low_head_of_more_than_512_rows(dev):
    """degree_threshold 30: about 40 % of the 1,834 patients feed the tabular head, so its first layer takes the fused
    data + weight gradient launch (M > 512) and its dW1a slabs are deferred like the high head's."""
    s = _setup(dev)
    assert int((s["plan"].lab_deg < 30).sum()) > 512
    _check(_steps(dev, True, threshold=30), _steps(dev, False, threshold=30))


def test_each_switch_alone(dev):
    ref = _steps(dev, False)
    _check(_steps(dev, True, step_advance=False), ref)
    _check(_steps(dev, False, step_advance=True), ref)


def test_eager_backward_gives_the_same_gradients(dev):
    """One eager predict_lab_values(...).backward(): the same .grad for every parameter both ways, embeddings included."""
    import mmgnn.model as mm
    from mmgnn import ops
    from mmgnn.model import build_model
    s = _setup(dev)
    res, reds = [], []
    for on in (True, False):
        mm.set_grad_finish(on)
        try:
            torch.manual_seed(42)
            model = build_model(CFG, (s["g"].node_types, s["g"].edge_types), None).to(dev)
            model._init_embeddings(s["g"])
            model._dropout_seed = 99
            model.train()
            ops.probe_arm(1 << 12)
            try:
                p = model.predict_lab_values(s["plan"], s["pi"], s["li"])
                supf = s["sup"].float()
                ops.weighted_pair_loss(p, s["y"], s["wlab"][s["li"]], supf, 1.0 / max(float(supf.sum()), 1.0), "mae").backward()
                torch.cuda.synchronize()
            finally:
                rows = ops.probe_read()
            res.append({k: q.grad.clone() for k, q in model.named_parameters() if q.grad is not None})
            reds.append([r for r in rows if r[1] == "linear_wgrad_reduce"])
        finally:
            mm.set_grad_finish(True)
    # the slab sums of the step, as probed: finish launches alone (logged as the grouped reduce is, shape 0 / 0 / 0; at
    # this size a small accumulating launch forces one in the middle of the backward, as it forces a grouped reduce
    # there without the switch) against the heads' own sum and the grouped launches, which are more
    assert reds[0] and all(r[2:5] == (0, 0, 0) and "k_grad_finish_group" in r[6] for r in reds[0]), reds[0]
    assert not any("k_grad_finish_group" in r[6] for r in reds[1]) and len(reds[1]) > len(reds[0]), (reds[0], reds[1])
    assert set(res[0]) == set(res[1]) and any(k.startswith("embeddings.") for k in res[0])
    for k in res[0]:
        assert same(res[0][k], res[1][k]), k
