"""ops._call on the MI355X, through the calls the wrappers already make: one with the shared workspace (order_stats, with
b = None for a NULL pointer), one with its own workspace tensor (the deferred weight gradient) and one without a
workspace (row_degree).  Each succeeds, refuses a wrong dtype with a TypeError that names the header's parameter and
refuses a non-contiguous view with a ValueError; tensors on two devices are refused."""
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def test_shared_workspace_call():
    vals = [3.0, -1.0, 7.5, 0.0, 2.0, -4.0, 9.0, 1.0]
    a = torch.tensor(vals, device=DEV)
    out, nan_count = ops.order_stats(a, [0, 3, 7])                      # b = None: NULL
    assert out.tolist() == [sorted(vals)[r] for r in (0, 3, 7)] and nan_count.tolist() == [0]
    b = torch.tensor([1.0] * 8, device=DEV)
    out, _ = ops.order_stats(a, [0, 7], b)
    assert out.tolist() == [0.0, 8.0]                                   # |a - b|: exact in fp32 for these values
    with pytest.raises(TypeError, match=r"^a: expected torch\.float32, got torch\.float64"):
        ops.order_stats(a.double(), [0])
    with pytest.raises(TypeError, match=r"^nan_count: expected torch\.int64, got torch\.int32"):
        ops.order_stats(a, [0], nan_count=torch.empty(1, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match=r"^b: must be contiguous"):
        ops.order_stats(a, [0], torch.zeros(8, 2, device=DEV)[:, 0])


def test_own_workspace_tensor_call():
    M, N, K = 32, 64, 64
    g = torch.Generator().manual_seed(5)
    dy, x = torch.randn(M, N, generator=g).to(DEV), torch.randn(M, K, generator=g).to(DEV)
    want, want_b = ops.linear_wgrad(dy, x, with_bias=True)
    jobs = []
    got, got_b = ops.linear_wgrad(dy, x, with_bias=True, defer=jobs)
    assert len(jobs) == 1 and jobs[0][1].dtype == torch.uint8 and jobs[0][1].is_cuda     # the call's own slab buffer
    ops.wgrad_reduce_flush(jobs)
    assert jobs == [] and torch.equal(got, want) and torch.equal(got_b, want_b)
    for defer in (None, []):
        with pytest.raises(TypeError, match=r"^dY: expected torch\.float32, got torch\.float64"):
            ops.linear_wgrad(dy.double(), x, defer=defer)
        with pytest.raises(ValueError, match=r"^X: must be contiguous"):
            ops.linear_wgrad(dy, torch.zeros(M, 2 * K, device=DEV)[:, ::2], defer=defer)
        assert not defer


def test_call_without_a_workspace():
    rowptr = torch.tensor([0, 1, 3, 3, 6], dtype=torch.int32, device=DEV)
    deg, inv = ops.row_degree(rowptr)
    assert deg.tolist() == [1, 2, 0, 3] and deg.dtype == torch.int32
    torch.testing.assert_close(inv.cpu(), torch.tensor([1.0, 0.5, 1.0, 1.0 / 3.0]), rtol=2.0 ** -23, atol=0.0)
    with pytest.raises(TypeError, match=r"^rowptr: expected torch\.int32, got torch\.int64"):
        ops.row_degree(rowptr.long())
    with pytest.raises(ValueError, match=r"^rowptr: must be contiguous"):
        ops.row_degree(torch.zeros(5, 2, dtype=torch.int32, device=DEV)[:, 0])


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices")
def test_tensors_on_two_devices_are_refused():
    a = torch.zeros(8, device=DEV)
    with pytest.raises(ValueError, match=r"mmg_order_stats: out is on cuda:1, the tensors before it on cuda:0"):
        ops.order_stats(a, [0], out=torch.empty(1, device="cuda:1"))
    with pytest.raises(ValueError, match="order_stats: a and b must have the same length and device"):
        ops.order_stats(a, [0], torch.zeros(8, device="cuda:1"))       # the wrapper's own check comes first
