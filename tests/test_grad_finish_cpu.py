"""Host side of ops.grad_finish (no GPU): how the deferred weight-gradient entries become jobs of mmg_grad_finish_group --
an accumulating entry on an earlier entry's gradient is a further slab series of that job, what cannot be one waits for
the next launch, entries without slabs are dropped -- and the library's refusals, which need no device."""
import ctypes as C

import torch

import mmgnn  # noqa: F401
from mmgnn import _lib, ops
from mmgnn._lib import SumJobT, WgradReduceT


def _entry(dW, acc, slab=0x1000, n4=8, n_split=2, view=None):
    e = (WgradReduceT(slab, n4, n_split, dW, None, n4, acc), None, torch.zeros(4 * n4), None)
    return e + (view,) if view is not None else e


def test_entries_become_series_and_launches(monkeypatch):
    calls = []

    class FakeLib:
        def mmg_grad_finish_group(self, series, n_series, sums, n_sums, stream):
            calls.append(([(series[i].dW, series[i].accumulate, series[i].slab, series[i].n_split) for i in range(n_series)],
                          [(sums[i].dst, sums[i].src[0], sums[i].n_src, sums[i].len, sums[i].cols, sums[i].ld_dst)
                           for i in range(n_sums)]))
            return 0

    monkeypatch.setattr(_lib, "load", lambda: FakeLib())
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_p", lambda t, *a, **k: None if t is None else t.data_ptr())
    wide = torch.zeros(2, 32)
    jobs = [_entry(100, 0, slab=0x10), _entry(200, 1, slab=0x20), _entry(100, 1, slab=0x30, n_split=5),
            _entry(300, 0, slab=None), _entry(100, 1, slab=0x40, n4=4),              # another size: not a series of job 100
            _entry(400, 0, slab=0x50, n4=4, view=wide[:, :8])]
    ops.grad_finish(jobs)
    assert jobs == []
    # the second entry of 100 follows the first as its further series; the view is a sum whose first source is the entry's dW
    assert calls == [([(100, 0, 0x10, 2), (100, 1, 0x30, 5), (200, 1, 0x20, 2), (400, 0, 0x50, 2)],
                      [(wide.data_ptr(), 400, 1, 16, 8, 32)]),
                     ([(100, 1, 0x40, 2)], [])]
    calls.clear()
    many = [_entry(100, 0)] + [_entry(100, 1, slab=0x100 + i) for i in range(5)]      # four series per job, then the next launch
    ops.grad_finish(many)
    assert [[e[1] for e in c[0]] for c in calls] == [[0, 1, 1, 1], [1, 1]]
    calls.clear()
    ops.grad_finish([_entry(1000 + i, 0) for i in range(30)])                         # the library splits a long list itself
    assert [len(c[0]) for c in calls] == [30]
    calls.clear()
    ops.wgrad_reduce_flush([_entry(400, 0, slab=0x50, n4=4, view=wide[:, 8:16])])     # a view: the old flush hands over
    assert calls == [([(400, 0, 0x50, 2)], [(wide.data_ptr() + 32, 400, 1, 16, 8, 32)])]


def test_refusals_need_no_device():
    lib = _lib.load()
    A, B, Cc, S = 0x100000, 0x200000, 0x300000, 0x400000

    def ser(dW, acc=0, n4=64, slab=S):
        return WgradReduceT(slab, n4, 2, dW, None, n4, acc)

    def summ(dst, srcs, n, cols=0, ld=0):
        sp, l = (C.c_void_p * 4)(*(list(srcs) + [None] * (4 - len(srcs)))), (C.c_int * 4)(*([cols] * 4))
        return SumJobT(dst, sp, len(srcs), n, cols, ld, l)

    def run(series, sums):
        rc = lib.mmg_grad_finish_group((WgradReduceT * max(len(series), 1))(*series), len(series),
                                       (SumJobT * max(len(sums), 1))(*sums), len(sums), None)
        return rc, lib.mmg_last_error()

    E = _lib.MMG_E_ARG
    rc, msg = run([ser(A)], [summ(B, [Cc, A], 256)])
    assert rc == E and b"reads the destination" in msg
    rc, msg = run([ser(A), ser(A + 512)], [])
    assert rc == E and b"overlapping" in msg
    rc, msg = run([ser(A), ser(A)], [])                                    # a second store to one gradient
    assert rc == E and b"cannot join" in msg
    # the halves of a [2, 256] matrix are disjoint, columns 96..223 against 0..127 are not
    rc, msg = run([ser(A)], [summ(B, [A], 256, 128, 256), summ(B + 4 * 96, [Cc], 256, 128, 256)])
    assert rc == E and b"overlapping" in msg
    rc, msg = run([ser(A)], [summ(B, [A], 256, 128, 256), summ(Cc, [A], 256)])   # A is left unwritten: nobody may read it
    assert rc == E and b"reads the destination" in msg
    assert run([ser(None)], [])[0] == E and run([], [summ(A, [None], 16)])[0] == E and run([ser(A, slab=None)], [])[0] == E
    assert run([ser(A + 4)], [])[0] == E                                   # with slabs: 16-byte addresses
    assert run([], [])[0] == E
