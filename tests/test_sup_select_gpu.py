"""mmg_sup_draw_select (ops.sup_draw_select): the supervision subset and the two pair lists in two launches, against the
path it replaces -- ops.sup_mask_draw followed by ops.pair_select(pi, deg, thr, sup, io_perm=perm) on the same seed.
Everything it writes is an integer or an exactly representable value, so every comparison is torch.equal: the mask, both
list lengths, both lists up to their lengths, the subset size and its reciprocal."""
import numpy as np
import pytest
import torch

import rng_ref as R

pytestmark = pytest.mark.gpu

CH = 2048                                        # positions per chunk (csrc/pairs.hip: SEL_CH)
N_PAT = 97
SEEDS = (0, 2 ** 63 + 0x1234567)
# threshold: every pair low / every pair high / mixed (degrees are 0 .. 39)
THRS = (1000, 0, 20)
FRACTIONS = (0.0, 0.2, 1.0)


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


def as_i64(v):
    v &= R.M64
    return v - 2 ** 64 if v >= 2 ** 63 else v


_INPUTS = {}


def inputs(n, dev):
    """Pairs sorted by patient, a degree table, a permutation and two id sets: built once per size, never written to."""
    if n not in _INPUTS:
        g = torch.Generator().manual_seed(1000 + n)
        pi = torch.randint(0, N_PAT, (n,), generator=g).sort().values.to(torch.int32)
        deg = torch.randint(0, 40, (N_PAT,), generator=g).to(torch.int32)
        perm = torch.randperm(n, generator=g)
        ids_small = torch.randperm(3 * n + 5, generator=g)[:n]                     # scattered, not the caller index
        ids_big = ids_small + (2 ** 32 - n)                                        # both sides of 2^32 ...
        ids_big[::3] += 2 ** 40                                                    # ... and far beyond it
        _INPUTS[n] = dict(pi=pi.to(dev), deg=deg.to(dev), perm=perm.to(dev),
                          ids={"none": None, "small": ids_small.to(dev), "big": ids_big.to(dev)})
    return _INPUTS[n]


def old_path(ops, x, thr, fraction, perm, ids, seed=0, seed_dev=None):
    n = x["pi"].numel()
    sup, count, inv_den = ops.sup_mask_draw(n, fraction, x["pi"].device, seed=seed, seed_dev=seed_dev, ids=ids)
    sel = ops.pair_select(x["pi"], x["deg"], thr, sup, io_perm=perm)
    return sup, sel, count, inv_den


def bits64(t):
    return t.view(torch.int64)


def assert_same(got, want, what):
    (gs, (gl, gh, gc), gn, gi), (ws, (wl, wh, wc), wn, wi) = got, want
    assert torch.equal(gc, wc), (what, gc.tolist(), wc.tolist())
    n_low, n_high = wc.tolist()
    assert torch.equal(gs.view(torch.int32), ws.view(torch.int32)), what
    assert torch.equal(gl[:n_low], wl[:n_low]), what
    assert torch.equal(gh[:n_high], wh[:n_high]), what
    assert torch.equal(bits64(gn), bits64(wn)) and torch.equal(bits64(gi), bits64(wi)), (what, float(gn), float(wn))
    return n_low, n_high


def sweep(ops, dev, n, use_perm, max_groups=0):
    x = inputs(n, dev)
    perm = x["perm"] if use_perm else None
    seen = set()
    for which, ids in x["ids"].items():
        for fraction in FRACTIONS:
            for thr in THRS:
                seed = SEEDS[(len(seen) + n) % 2]
                got = ops.sup_draw_select(x["pi"], x["deg"], thr, fraction, seed=seed, ids=ids, io_perm=perm,
                                          max_groups=max_groups)
                want = old_path(ops, x, thr, fraction, perm, ids, seed=seed)
                n_low, n_high = assert_same(got, want, (n, use_perm, which, fraction, thr))
                seen.add((n_low > 0, n_high > 0))
                if fraction == 0.0:
                    assert n_low + n_high == 0
                if fraction == 1.0:
                    assert n_low + n_high == n and (thr != 1000 or n_high == 0) and (thr != 0 or n_low == 0)
    return seen


@pytest.mark.parametrize("use_perm", [False, True])
@pytest.mark.parametrize("n", [1, 7, 8, CH - 1, CH, CH + 1, 5 * CH + 3])
def test_equals_draw_then_select(ops, dev, n, use_perm):
    seen = sweep(ops, dev, n, use_perm)
    assert (False, False) in seen and (True, False) in seen and (False, True) in seen
    if n >= CH - 1:                              # (a handful of pairs may well all fall to one head)
        assert (True, True) in seen


@pytest.mark.parametrize("use_perm", [False, True])
def test_two_workgroups_walk_several_chunks_each(ops, dev, use_perm):
    """max_groups = 2 over 7 chunks: ranges of 4 and 3 chunks, the last chunk ragged -- a range's totals pass 2^11 (what
    one chunk holds) and the second workgroup's bases come from the first one's totals."""
    n = 6 * CH + 5
    seen = sweep(ops, dev, n, use_perm, max_groups=2)
    assert (True, True) in seen
    x = inputs(n, dev)
    for g in (1, 3, 7, 1024):                   # one range; a last range shorter than the rest; one chunk each; the cap
        got = ops.sup_draw_select(x["pi"], x["deg"], 20, 0.2, seed=5, io_perm=x["perm"] if use_perm else None, max_groups=g)
        want = old_path(ops, x, 20, 0.2, x["perm"] if use_perm else None, None, seed=5)
        assert_same(got, want, g)


def test_no_pairs(ops, dev):
    pi = torch.empty(0, dtype=torch.int32, device=dev)
    deg = torch.zeros(N_PAT, dtype=torch.int32, device=dev)
    count = torch.full((1,), 7.0, dtype=torch.float64, device=dev)
    inv_den = torch.full((1,), 7.0, dtype=torch.float64, device=dev)
    out = (torch.full((1,), -1, dtype=torch.int32, device=dev), torch.full((1,), -1, dtype=torch.int32, device=dev),
           torch.full((2,), 9, dtype=torch.int32, device=dev))
    sup, sel, c, d = ops.sup_draw_select(pi, deg, 20, 0.2, seed=3, out=out, count=count, inv_den=inv_den)
    assert sup.numel() == 0 and sel[2].tolist() == [0, 0] and float(c) == 0.0 and float(d) == 1.0
    assert sel[0].tolist() == [-1] and sel[1].tolist() == [-1]
    _, _, oc, od = old_path(ops, dict(pi=pi, deg=deg), 20, 0.2, None, None, seed=3)
    assert float(oc) == 0.0 and float(od) == 1.0


def test_mask_is_optional_and_outputs_are_written_in_place(ops, dev):
    x = inputs(CH + 1, dev)
    n = CH + 1
    want = old_path(ops, x, 20, 0.2, x["perm"], None, seed=11)
    sup = torch.full((n,), 5.0, device=dev)
    out = (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
           torch.empty(2, dtype=torch.int32, device=dev))
    count, inv_den = torch.empty(1, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float64, device=dev)
    got = ops.sup_draw_select(x["pi"], x["deg"], 20, 0.2, seed=11, io_perm=x["perm"], sup=sup, out=out, count=count,
                              inv_den=inv_den)
    assert got[0] is sup and got[1][0] is out[0] and got[1][2] is out[2] and got[2] is count and got[3] is inv_den
    assert_same(got, want, "in place")
    none = ops.sup_draw_select(x["pi"], x["deg"], 20, 0.2, seed=11, io_perm=x["perm"], want_sup=False)
    assert none[0] is None
    assert_same((want[0],) + tuple(none[1:]), want, "no mask")
    # a mask that does not start on a 16-byte boundary (a view one element into a buffer) takes the scalar stores
    buf = torch.full((n + 1,), 5.0, device=dev)
    got = ops.sup_draw_select(x["pi"], x["deg"], 20, 0.2, seed=11, io_perm=x["perm"], sup=buf[1:])
    assert_same(got, want, "unaligned mask")
    assert float(buf[0]) == 5.0


@pytest.mark.parametrize("which", ["none", "big"])
def test_against_the_host_restatement(ops, dev, which):
    """Independent of the old kernels: the draw from tests/rng_ref.py and a numpy stable partition."""
    n, thr, fraction, seed = 5 * CH + 3, 20, 0.2, 2 ** 63 + 5
    x = inputs(n, dev)
    ids = x["ids"][which]
    sup, (sel_low, sel_high, counts), count, inv_den = ops.sup_draw_select(x["pi"], x["deg"], thr, fraction, seed=seed,
                                                                           ids=ids, io_perm=x["perm"])
    keep_p = np.float32(1.0) - np.float32(fraction)
    perm = x["perm"].cpu().numpy()
    e = np.arange(n, dtype=np.uint64) if ids is None else ids.cpu().numpy().astype(np.uint64)
    kept = R.keep_at(seed, R.SITE_SUP, e, keep_p)                       # caller order
    assert np.array_equal(sup.cpu().numpy(), kept.astype(np.float32))
    kept_sorted = kept[perm]
    low = x["deg"].cpu().numpy()[x["pi"].cpu().numpy()] < thr
    pos = np.arange(n, dtype=np.int32)
    want_low, want_high = pos[kept_sorted & low], pos[kept_sorted & ~low]
    assert counts.tolist() == [want_low.size, want_high.size] and want_low.size and want_high.size
    assert np.array_equal(sel_low[:want_low.size].cpu().numpy(), want_low)
    assert np.array_equal(sel_high[:want_high.size].cpu().numpy(), want_high)
    assert float(count) == float(kept.sum()) and float(inv_den) == 1.0 / float(kept.sum())


def test_replays_of_a_captured_call_follow_the_device_seed(ops, dev):
    n, thr, fraction = 5 * CH + 3, 20, 0.2
    x = inputs(n, dev)
    seed_dev = torch.tensor([as_i64(SEEDS[1]), 77], dtype=torch.int64, device=dev)
    sup = torch.zeros(n, device=dev)
    out = (torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
           torch.zeros(2, dtype=torch.int32, device=dev))
    count, inv_den = torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)

    def call():
        return ops.sup_draw_select(x["pi"], x["deg"], thr, fraction, seed=123, seed_dev=seed_dev, io_perm=x["perm"],
                                   sup=sup, out=out, count=count, inv_den=inv_den)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                   # (sizes this stream's workspace outside the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            got = call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    lists = []
    for _ in range(3):
        ops.seed_advance(seed_dev)
        graph.replay()
        torch.cuda.synchronize()
        want = old_path(ops, x, thr, fraction, x["perm"], None, seed=123, seed_dev=seed_dev)
        n_low, n_high = assert_same(got, want, "replay")
        assert n_low and n_high
        lists.append((got[0].clone(), got[1][0][:n_low].clone(), got[1][1][:n_high].clone()))
    for a in range(3):
        for b in range(a + 1, 3):
            assert not torch.equal(lists[a][0], lists[b][0])
            assert lists[a][1].shape != lists[b][1].shape or not torch.equal(lists[a][1], lists[b][1])
            assert lists[a][2].shape != lists[b][2].shape or not torch.equal(lists[a][2], lists[b][2])


# ------------------------------------------------------------------------------------------ the training step
CFG = {"model": {"architecture": "RGCN", "hidden_dim": 128, "num_layers": 2, "dropout": 0.2, "use_batch_norm": True,
                 "activation": "relu"}}
LAB = ("patient", "has_lab", "lab")


def _three_steps(dev, setup, fused):
    import mmgnn.train as mt
    from mmgnn.model import build_model
    from mmgnn.optim import Adam
    mt.set_fused_select(fused)
    try:
        torch.manual_seed(42)
        model = build_model(CFG, (setup["g"].node_types, setup["g"].edge_types), None).to(dev)
        model._init_embeddings(setup["g"])
        opt = Adam([q for k, q in model.named_parameters() if not k.startswith("embeddings.")], lr=1e-2)
        step = mt.PiecewiseGraphedTrainStep(model, setup["plan"], setup["pi"], setup["li"], setup["y"], setup["wlab"], opt,
                                            None, None, mask_fraction=0.2)
        losses = [step.step().clone() for _ in range(3)]
        torch.cuda.synchronize()
        out = {f"param.{k}": p.detach().clone() for k, p in model.named_parameters()}
        out.update({f"loss{i}": v for i, v in enumerate(losses)})
        out.update(seed=model._seed_dev.clone(), sup=step.sup.clone(), counts=step._sel[2].clone(),
                   inv_den=step._sv.inv_den.clone(), pred=step.pred.clone())
        return out
    finally:
        mt.set_fused_select(True)


def test_three_training_steps_are_bitwise_the_same_with_and_without_the_switch(dev):
    """A PiecewiseGraphedTrainStep at the x1 eICU shape that draws 20 % of its pairs every step: three replays with the
    two-launch path and three with the five launches it replaces, from the same seeds -- every loss, every parameter, and
    what the last draw left (mask, list lengths, normaliser) and the predictions are the same bits."""
    import mmgnn  # noqa: F401
    import mmgnn.train as mt
    from mmgnn.data import build_plan
    from mmgnn.synth import make_graph
    assert mt.FUSED_SELECT is True
    g = make_graph(1, seed=0, device=dev)
    ei = g[LAB].edge_index
    E = ei.shape[1]
    tr = torch.randperm(E, generator=torch.Generator(device=dev).manual_seed(42), device=dev)[: int(0.7 * E)].sort().values
    setup = dict(g=g, plan=build_plan(g, dev, use_cache=False), pi=ei[0][tr].contiguous(), li=ei[1][tr].contiguous(),
                 y=g[LAB].edge_attr[tr].squeeze(-1).contiguous(), wlab=torch.ones(int(g["lab"].num_nodes), device=dev))
    a, b = _three_steps(dev, setup, True), _three_steps(dev, setup, False)
    assert set(a) == set(b)
    for k in a:
        x, y = a[k].contiguous(), b[k].contiguous()
        assert x.shape == y.shape and x.dtype == y.dtype, k
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        elif x.dtype == torch.float64:
            x, y = x.reshape(-1).view(torch.int64), y.reshape(-1).view(torch.int64)
        assert torch.equal(x, y), k
    assert float(a["loss0"]) != float(a["loss1"]) and int(a["counts"].sum()) > 0
    assert 0.15 < float(a["sup"].mean()) < 0.25
