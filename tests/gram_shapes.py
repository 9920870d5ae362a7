"""What the GPU tests of the fp64 slab-Gram kernels (csrc/gram64.h: assoc, chain, pca) share: device copies, the padded
view whose padding is poison, bit views, and the row counts at which a slab plan takes another path."""
import numpy as np
import torch

DEV = torch.device("cuda:0")
F32 = np.float32
PAD = 5                                          # padding columns behind the L labs: ld_x = L + 5


def dv(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def padded(X):
    """The device copy of X as the [:, :L] view of a buffer whose padding columns hold NaN and 1e30: poison that must
    never be read."""
    n, L = X.shape
    buf = np.full((n, L + PAD), np.nan, F32)
    buf[:, L::2] = F32(1e30)
    buf[:, :L] = X
    view = dv(buf)[:, :L]
    assert view.stride(0) == L + PAD
    return view


def bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def row_counts(plan, chunk, L):
    """The n of one lab count, from the slab plan `plan(n, L) -> (rows per slab, slabs)`: one row; a chunk minus and plus
    a row; exactly one slab; a slab and a row; three slabs, the last ragged."""
    rows, slabs = plan(1, L)
    assert slabs == 1 and rows % chunk == 0
    ns = [1, chunk - 1, chunk + 1, rows, rows + 1, 2 * rows + 77]
    for n, want in zip(ns, (1, 1, 1, 1, 2, 3)):
        assert plan(n, L) == (rows, want), (n, L)
    return ns
