"""mmg_step_advance (the step counter, the dropout seed and the BatchNorm counters of a captured step in ONE one-thread
launch) against the launches it replaces -- the bump behind mmg_adam_step_dev, mmg_seed_advance, mmg_counters_add -- and
mmg_adam_update_dev + mmg_step_advance against mmg_adam_step_dev.  Integer state is compared exactly, floats bitwise."""
import ctypes as C
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _counter_args(cs, incs):
    return (C.c_void_p * len(cs))(*[c.data_ptr() for c in cs]), (C.c_int64 * len(cs))(*incs)


@pytest.mark.parametrize("with_step, with_seed, with_counters", list(itertools.product([False, True], repeat=3)))
def test_step_advance_is_the_three_launches(dev, with_step, with_seed, with_counters):
    """Three consecutive calls, every part present or absent."""
    import mmgnn  # noqa: F401
    from mmgnn import ops
    incs = [1, 2, 0, 5, 1]

    def fresh():
        return (torch.full((), 7.0, device=dev), torch.tensor([123456789, -42], dtype=torch.int64, device=dev),
                [torch.tensor(10 * i, dtype=torch.int64, device=dev) for i in range(len(incs))])

    (s0, z0, c0), (s1, z1, c1) = fresh(), fresh()
    # a parameter bucket whose one tensor has no gradient: mmg_adam_step_dev leaves it alone and advances the counter
    p, m, v = (torch.ones(8, device=dev) for _ in range(3))
    hyper = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.0], device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    offs, none = (C.c_int32 * 2)(0, 8), (C.c_void_p * 1)(None)
    for _ in range(3):
        if with_step:
            ops._call("mmg_adam_step_dev", p, m, v, none, offs, 1, hyper, s0, ticket)
        if with_seed:
            ops._call("mmg_seed_advance", z0)
        if with_counters:
            ops._call("mmg_counters_add", *_counter_args(c0, incs), len(incs))
        ops._call("mmg_step_advance", s1 if with_step else None, z1 if with_seed else None,
                  *(_counter_args(c1, incs) if with_counters else (None, None)), len(incs) if with_counters else 0)
    torch.cuda.synchronize()
    assert torch.equal(_bits(s0), _bits(s1)) and float(s1) == (10.0 if with_step else 7.0)
    assert torch.equal(z0, z1) and (int(z1[1]) != -42) == with_seed
    assert [int(c) for c in c0] == [int(c) for c in c1] == [10 * i + (3 * k if with_counters else 0) for i, k in enumerate(incs)]
    assert bool((p == 1).all())


def test_step_advance_refusals(dev):
    import mmgnn  # noqa: F401
    from mmgnn import _lib
    lib = _lib.load()
    c = torch.zeros((), dtype=torch.int64, device=dev)
    ptrs, inc = _counter_args([c], [1])
    assert lib.mmg_step_advance(None, None, ptrs, inc, _lib.MMG_COUNTERS_MAX + 1, None) == _lib.MMG_E_ARG
    assert lib.mmg_step_advance(None, None, None, None, 1, None) == _lib.MMG_E_ARG
    assert lib.mmg_step_advance(None, None, (C.c_void_p * 1)(None), inc, 1, None) == _lib.MMG_E_ARG
    assert lib.mmg_step_advance(None, None, None, None, 0, None) == 0          # nothing to do: no launch
    assert lib.mmg_adam_update_dev(None, None, None, None, None, 1, None, None, None) == _lib.MMG_E_ARG
    torch.cuda.synchronize()
    assert int(c) == 0


def _adam_state(dev):
    gen = torch.Generator().manual_seed(5)
    sizes = [100, 250, 1, 449, 200]                         # 1,000 parameters over 5 tensors
    offs = [0]
    for n in sizes:
        offs.append(offs[-1] + n)
    p = torch.randn(1000, generator=gen).to(dev)
    grads = [[None if i == 2 else (torch.randn(n, generator=gen) * 10.0 ** (i - 2)).to(dev) for i, n in enumerate(sizes)]
             for _ in range(3)]                             # (tensor 2 has no gradient)
    return p, grads, (C.c_int32 * 6)(*offs)


def _gp(gs):
    return (C.c_void_p * len(gs))(*[g.data_ptr() if g is not None else None for g in gs])


def _reference(dev):
    from mmgnn import ops
    p, grads, offs = _adam_state(dev)
    m, v, step = torch.zeros(1000, device=dev), torch.zeros(1000, device=dev), torch.zeros((), device=dev)
    hyper = torch.tensor([1e-2, 0.9, 0.99, 1e-8, 1e-3], device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    for gs in grads:
        ops._call("mmg_adam_step_dev", p, m, v, _gp(gs), offs, 5, hyper, step, ticket)
    torch.cuda.synchronize()
    return p, m, v, step


def test_adam_without_the_bump_then_step_advance(dev):
    import mmgnn  # noqa: F401
    from mmgnn import ops
    ref = _reference(dev)
    p, grads, offs = _adam_state(dev)
    m, v, step = torch.zeros(1000, device=dev), torch.zeros(1000, device=dev), torch.zeros((), device=dev)
    hyper = torch.tensor([1e-2, 0.9, 0.99, 1e-8, 1e-3], device=dev)
    for gs in grads:
        ops._call("mmg_adam_update_dev", p, m, v, _gp(gs), offs, 5, hyper, step)
        ops._call("mmg_step_advance", step, None, None, None, 0)
    torch.cuda.synchronize()
    for a, b in zip(ref, (p, m, v, step)):
        assert torch.equal(_bits(a), _bits(b))
    assert float(step) == 3.0


def test_adam_without_the_bump_replayed_from_a_graph(dev):
    """The same three steps as three replays of one recorded step (the gradients are copied into static buffers)."""
    import mmgnn  # noqa: F401
    from mmgnn import ops
    ref = _reference(dev)
    p, grads, offs = _adam_state(dev)
    p0 = p.clone()
    m, v, step = torch.zeros(1000, device=dev), torch.zeros(1000, device=dev), torch.zeros((), device=dev)
    hyper = torch.tensor([1e-2, 0.9, 0.99, 1e-8, 1e-3], device=dev)
    static = [g.clone() if g is not None else None for g in grads[0]]
    gp = _gp(static)

    def body():
        ops._call("mmg_adam_update_dev", p, m, v, gp, offs, 5, hyper, step)
        ops._call("mmg_step_advance", step, None, None, None, 0)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()                                              # warm-up, undone below
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    torch.cuda.synchronize()
    p.copy_(p0); m.zero_(); v.zero_(); step.zero_()
    for gs in grads:
        for s, g in zip(static, gs):
            if s is not None:
                s.copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(ref, (p, m, v, step)):
        assert torch.equal(_bits(a), _bits(b))
