"""The two streaming matrix kernels at the x100 dense shape, for a kernel trace of their own."""
import os
import sys

import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import mmgnn  # noqa
from mmgnn import conformal_ops as co, ops
dev = torch.device("cuda:0")
P, L = 183400, 50
g = torch.Generator(dev).manual_seed(0)
m = torch.randn(P, L, device=dev, generator=g)
deg = torch.randint(0, 60, (P,), device=dev, generator=g, dtype=torch.int32)
q = torch.randn(2, L * 3, device=dev, generator=g).sort(0).values
table = torch.cat([q, torch.zeros(1, L * 3, device=dev)]).contiguous()
outs = tuple(torch.empty_like(m) for _ in range(3))
stats = torch.zeros(L, ops.LAB_STAT_FIELDS, dtype=torch.float64, device=dev)
stats[:, 1], stats[:, 2] = 1.5, 2.0
inv = torch.empty_like(m)
for _ in range(30):
    co.cf_apply_matrix(m, None, deg, [0.0, 6.0, 16.0, float("inf")], table, False, out=outs)
    ops.lab_inverse_matrix(m, stats, "zscore", out=inv)
torch.cuda.synchronize()
