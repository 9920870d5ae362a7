"""mmg_grad_finish_group (one launch that finishes the gradients of a step) against the entry points it replaces, run one
after the other on the same slabs: mmg_wgrad_reduce_group launch(es) in today's order, then mmg_vec_sums.  Every comparison
is BITWISE (int32 views): the new kernel keeps the order of additions of every element.

Shapes sit at the loop boundaries of the slab sum: 16 slab groups, 8-deep load batches of 16 slabs (n_split 1, 15, 16, 17,
127, 128, 129, 250), 16 float4 per workgroup (n4 1, 15, 16, 17, 16 * 7 + 3, 2048 + 32)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

N_SPLITS = (1, 15, 16, 17, 127, 128, 129, 250)
N4S = (1, 15, 16, 17, 16 * 7 + 3, 2048 + 32)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    import mmgnn  # noqa: F401
    from mmgnn import _lib
    return _lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _slabs(gen, dev, n_split, n4, special=False):
    s = torch.randn(n_split, n4 * 4, generator=gen) * 10.0 ** torch.randint(-3, 4, (n_split, 1), generator=gen).float()
    if special:                                       # one special value per element column: bit patterns are compared
        s[n_split // 2, 0] = float("nan")
        if n4 * 4 > 3:
            s[0, 1] = float("inf")
            s[n_split - 1, 2] = float("-inf")
            s[0, 2] = float("inf")                    # inf - inf somewhere down the sum (n_split 1: the last write stays)
            s[:, 3] = torch.tensor(1e-41)             # denormals only
    return s.to(dev)


def _reduce_job(lib, slab, dW, dbias, nk4, acc):
    n_split, n = slab.shape
    return lib.WgradReduceT(slab.data_ptr(), n // 4, n_split, dW.data_ptr(), dbias.data_ptr() if dbias is not None else None,
                            nk4, int(acc))


def _reduce(lib, jobs):
    for j0 in range(0, len(jobs), lib.MMG_WGRAD_REDUCE_MAX):
        part = jobs[j0:j0 + lib.MMG_WGRAD_REDUCE_MAX]
        arr = (lib.WgradReduceT * len(part))(*part)
        assert lib.load().mmg_wgrad_reduce_group(arr, len(part), _stream()) == 0, lib.load().mmg_last_error()


def _finish_job(lib, slabs=(), n4=0, nk4=None, dW=None, dbias=None, acc=0, srcs=(), cols=0, ld_dst=0, ld_src=()):
    """One destination, as the tests think of it: slab series, dense sources, a destination with cols / ld_dst."""
    n4 = slabs[0].shape[1] // 4 if slabs else n4
    return dict(slabs=list(slabs), n4=n4, nk4=n4 if nk4 is None else nk4, dW=dW, dbias=dbias, acc=int(acc), srcs=list(srcs),
                cols=cols, ld_dst=ld_dst, ld_src=list(ld_src))


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _finish(lib, jobs):
    """The jobs as the two lists of mmg_grad_finish_group: every slab series an mmg_wgrad_reduce_t on the job's dW; dense
    sources or a strided destination a sum whose first source is that dW (a stand-in address when the value lands in a
    view: that dW is never written); a job without slabs a plain sum."""
    series, sums, keep = [], [], []
    for j in jobs:
        key = j["dW"]
        if j["slabs"] and j["cols"]:
            key = torch.empty(4 * j["nk4"], device=j["slabs"][0].device)
            keep.append(key)
        for s, slab in enumerate(j["slabs"]):
            series.append(lib.WgradReduceT(_ptr(slab), j["n4"], slab.shape[0] if slab is not None else 1, _ptr(key),
                                           _ptr(j["dbias"]), j["nk4"], j["acc"] if s == 0 else 1))
        if j["slabs"] and not (j["srcs"] or j["cols"]):
            continue
        srcs = ([key] if j["slabs"] else []) + j["srcs"]
        lds = ([j["cols"]] if j["slabs"] else []) + (j["ld_src"] or [0] * len(j["srcs"]))
        sp, ld = (C.c_void_p * 4)(), (C.c_int * 4)()
        for q, t in enumerate(srcs):
            sp[q], ld[q] = _ptr(t), lds[q]
        sums.append(lib.SumJobT(_ptr(j["dW"]), sp, len(srcs), 4 * j["nk4"] if j["slabs"] else j["n4"], j["cols"], j["ld_dst"], ld))
    return lib.load().mmg_grad_finish_group((lib.WgradReduceT * max(len(series), 1))(*series), len(series),
                                            (lib.SumJobT * max(len(sums), 1))(*sums), len(sums), _stream())


def _vec_sums(lib, jobs):
    """jobs: (dst, [srcs], cols, ld_dst, [ld_src]) -- the existing launch."""
    arr = (lib.SumJobT * len(jobs))()
    for i, (dst, srcs, cols, ld_dst, ld_src) in enumerate(jobs):
        sp, ld = (C.c_void_p * 4)(), (C.c_int * 4)()
        for q, t in enumerate(srcs):
            sp[q], ld[q] = t.data_ptr(), ld_src[q] if ld_src else 0
        n = dst.numel()
        arr[i] = lib.SumJobT(dst.data_ptr(), sp, len(srcs), n, cols, ld_dst, ld)
    assert lib.load().mmg_vec_sums(arr, len(jobs), _stream()) == 0, lib.load().mmg_last_error()


def _nk4(n4):
    return {1: 1, 15: 12, 16: 16, 17: 16, 16 * 7 + 3: 112, 2048 + 32: 2048}[n4]


@pytest.mark.parametrize("n_split", N_SPLITS)
def test_slab_sums_at_every_loop_boundary(dev, lib, n_split):
    """Six jobs of very different n4 in one launch; bias tails (nk4 < n4), stores and accumulating stores alternate; the
    slabs hold a NaN, infinities and denormals."""
    gen = torch.Generator().manual_seed(100 + n_split)
    ref_jobs, new_jobs, pairs = [], [], []
    for i, n4 in enumerate(N4S):
        slab = _slabs(gen, dev, n_split, n4, special=True)
        nk4, acc = _nk4(n4), i % 2
        init_w = torch.randn(nk4 * 4, generator=gen).to(dev)
        init_b = torch.randn(max(n4 - nk4, 1) * 4, generator=gen).to(dev)
        outs = []
        for _ in range(2):
            w, b = init_w.clone(), init_b.clone()
            outs.append((w, b if nk4 < n4 else None, b))
        ref_jobs.append(_reduce_job(lib, slab, outs[0][0], outs[0][1], nk4, acc))
        new_jobs.append(_finish_job(lib, [slab], nk4=nk4, dW=outs[1][0], dbias=outs[1][1], acc=acc))
        pairs.append((outs, slab))
    _reduce(lib, ref_jobs)
    assert _finish(lib, new_jobs) == 0, lib.load().mmg_last_error()
    torch.cuda.synchronize()
    for (ref, new), _ in pairs:
        assert _same(ref[0], new[0]) and _same(ref[2], new[2])


@pytest.mark.parametrize("first_acc", [0, 1])
def test_two_series_on_one_destination_in_both_orders(dev, lib, first_acc):
    gen = torch.Generator().manual_seed(7)
    n4, nk4 = 2048 + 32, 2048
    A, B = _slabs(gen, dev, 129, n4), _slabs(gen, dev, 17, n4)
    init_w, init_b = torch.randn(nk4 * 4, generator=gen).to(dev), torch.randn(128, generator=gen).to(dev)
    res = []
    for order in ((A, B), (B, A)):
        w0, b0, w1, b1 = init_w.clone(), init_b.clone(), init_w.clone(), init_b.clone()
        _reduce(lib, [_reduce_job(lib, order[0], w0, b0, nk4, first_acc)])           # dW = t_A, then dW = dW + t_B
        _reduce(lib, [_reduce_job(lib, order[1], w0, b0, nk4, 1)])
        assert _finish(lib, [_finish_job(lib, list(order), nk4=nk4, dW=w1, dbias=b1, acc=first_acc)]) == 0
        torch.cuda.synchronize()
        assert _same(w0, w1) and _same(b0, b1)
        res.append(w1)
    if first_acc:                             # (old + t_A) + t_B against (old + t_B) + t_A: the test can tell the orders apart
        assert not _same(res[0], res[1])


@pytest.mark.parametrize("n_src", [0, 1, 2, 3])
def test_dense_sources_behind_a_slab_sum_with_unequal_row_strides(dev, lib, n_src):
    gen = torch.Generator().manual_seed(20 + n_src)
    rows, cols = 64, 128
    slab = _slabs(gen, dev, 33, rows * cols // 4 + 16)                  # + a bias tail of 64
    wide = [torch.randn(rows, ld, generator=gen).to(dev) for ld in (256, 384, 132)]
    srcs = [wide[0][:, 128:], wide[1][:, 4:132], wide[2][:, 4:]][:n_src]
    lds = [256, 384, 132][:n_src]
    tmp, b_ref, b_new = torch.empty(rows, cols, device=dev), torch.zeros(64, device=dev), torch.zeros(64, device=dev)
    out_ref, out_new = torch.full((rows, 260), 7.0, device=dev), torch.full((rows, 260), 7.0, device=dev)
    _reduce(lib, [_reduce_job(lib, slab, tmp, b_ref, rows * cols // 4, 0)])
    _vec_sums(lib, [(out_ref[:, 4:132], [tmp] + srcs, cols, 260, [cols] + lds)])
    assert _finish(lib, [_finish_job(lib, [slab], nk4=rows * cols // 4, dW=out_new[:, 4:132], dbias=b_new, srcs=srcs, cols=cols,
                                     ld_dst=260, ld_src=lds)]) == 0, lib.load().mmg_last_error()
    torch.cuda.synchronize()
    assert _same(out_ref, out_new) and _same(b_ref, b_new)
    assert bool((out_new[:, :4] == 7.0).all()) and bool((out_new[:, 132:] == 7.0).all())


@pytest.mark.parametrize("n_src", [1, 2, 3, 4])
def test_dense_jobs_are_vec_sums_jobs(dev, lib, n_src):
    """No slabs: any length, any alignment, flat and strided, several jobs of very different length in one launch."""
    gen = torch.Generator().manual_seed(40 + n_src)
    flat = [torch.randn(70001 + 1, generator=gen).to(dev)[1:] for _ in range(n_src)]         # (4 bytes off a 16-byte boundary)
    tiny = [torch.randn(1, generator=gen).to(dev) for _ in range(n_src)]
    wide = [torch.randn(37, ld, generator=gen).to(dev) for ld in (131, 130, 257, 133)][:n_src]
    mats = [w[:, 1:130] for w in wide]
    lds = [131, 130, 257, 133][:n_src]
    outs = []
    for _ in range(2):
        outs.append((torch.zeros(70001, device=dev), torch.zeros(1, device=dev), torch.full((37, 140), 3.0, device=dev)))
    r, n = outs
    _vec_sums(lib, [(r[0], flat, 0, 0, None), (r[1], tiny, 0, 0, None), (r[2][:, 5:134], mats, 129, 140, lds)])
    # (SumJobT.len of the strided job is the view's element count)
    assert _finish(lib, [_finish_job(lib, n4=70001, dW=n[0], srcs=flat), _finish_job(lib, n4=1, dW=n[1], srcs=tiny),
                         _finish_job(lib, n4=37 * 129, dW=n[2][:, 5:134], srcs=mats, cols=129, ld_dst=140, ld_src=lds)]) == 0
    torch.cuda.synchronize()
    for a, b in zip(r, n):
        assert _same(a, b)


def test_both_halves_of_a_wider_matrix_in_one_launch(dev, lib):
    """[64, 2 * 128]: the left half from slabs, the right half from a one-source job; a launch with the left job alone
    leaves the right half unwritten."""
    gen = torch.Generator().manual_seed(60)
    K, D = 64, 128
    slab = _slabs(gen, dev, 250, K * D // 4)
    right = torch.randn(K, D, generator=gen).to(dev)
    tmp, ref = torch.empty(K, D, device=dev), torch.full((K, 2 * D), -5.0, device=dev)
    _reduce(lib, [_reduce_job(lib, slab, tmp, None, K * D // 4, 0)])
    _vec_sums(lib, [(ref[:, :D], [tmp], D, 2 * D, [D]), (ref[:, D:], [right], D, 2 * D, [D])])
    alone, both = torch.full((K, 2 * D), -5.0, device=dev), torch.full((K, 2 * D), -5.0, device=dev)
    left_job = lambda t: _finish_job(lib, [slab], dW=t[:, :D], cols=D, ld_dst=2 * D)                  # noqa: E731
    assert _finish(lib, [left_job(alone)]) == 0, lib.load().mmg_last_error()
    assert _finish(lib, [left_job(both), _finish_job(lib, n4=K * D, dW=both[:, D:], srcs=[right], cols=D, ld_dst=2 * D,
                                                     ld_src=[D])]) == 0, lib.load().mmg_last_error()
    torch.cuda.synchronize()
    assert _same(ref, both) and _same(ref[:, :D], alone[:, :D])
    assert bool((alone[:, D:] == -5.0).all())


@pytest.mark.parametrize("n_jobs", [17, 24, 31])
def test_more_jobs_than_the_old_limit(dev, lib, n_jobs):
    """17 and 24: one launch (the old limit was 16 jobs); 31: beyond MMG_GRAD_FINISH_MAX, several launches."""
    assert lib.MMG_WGRAD_REDUCE_MAX == 16 and lib.MMG_GRAD_FINISH_MAX == 24 and lib.MMG_GRAD_FINISH_SERIES == 4
    gen = torch.Generator().manual_seed(80 + n_jobs)
    ref_jobs, new_jobs, outs = [], [], []
    for i in range(n_jobs):
        n4 = N4S[i % len(N4S)] + 16 * (i // len(N4S))
        slab = _slabs(gen, dev, N_SPLITS[i % len(N_SPLITS)], n4)
        a, b = torch.ones(n4 * 4, device=dev), torch.ones(n4 * 4, device=dev)
        ref_jobs.append(_reduce_job(lib, slab, a, None, n4, i % 3 == 0))
        new_jobs.append(_finish_job(lib, [slab], dW=b, acc=i % 3 == 0))
        outs.append((a, b, slab))
    _reduce(lib, ref_jobs)
    assert _finish(lib, new_jobs) == 0, lib.load().mmg_last_error()
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b, _ in outs)


def test_refusals(dev, lib):
    gen = torch.Generator().manual_seed(90)
    slab = _slabs(gen, dev, 4, 64)
    a, b, c = (torch.zeros(256, device=dev) for _ in range(3))
    E = lib.MMG_E_ARG
    err = lambda: lib.load().mmg_last_error()                                                          # noqa: E731
    ok = _finish_job(lib, [slab], dW=a)
    # (a sum whose FIRST source is a series' dW belongs to that job; as a further source it reads another job's destination)
    assert _finish(lib, [ok, _finish_job(lib, n4=256, dW=b, srcs=[c, a])]) == E and b"reads the destination" in err()
    assert _finish(lib, [_finish_job(lib, n4=256, dW=b, srcs=[c, a]), ok]) == E and b"reads the destination" in err()
    two = [_finish_job(lib, n4=256, dW=b, srcs=[a, c]), _finish_job(lib, n4=256, dW=c, srcs=[a])]      # two sums on one dW
    assert _finish(lib, [ok] + two) == E and b"reads the destination" in err()
    assert _finish(lib, [ok, _finish_job(lib, [slab], dW=a)]) == E and b"cannot join" in err()         # a second store to a
    assert _finish(lib, [ok, _finish_job(lib, n4=100, dW=a[100:], srcs=[c[:100]])]) == E and b"overlapping" in err()
    wide = torch.zeros(2, 256, device=dev)                 # column slices of one matrix that share columns 96..127
    assert _finish(lib, [_finish_job(lib, [slab], dW=wide[:, :128], cols=128, ld_dst=256),
                         _finish_job(lib, n4=256, dW=wide[:, 96:224], srcs=[c], cols=128, ld_dst=256, ld_src=[128])]) == E
    assert b"overlapping" in err()
    assert _finish(lib, [_finish_job(lib, [slab], dW=None)]) == E and b"null" in err()
    assert _finish(lib, [_finish_job(lib, n4=256, dW=b, srcs=[a, None])]) == E and b"null" in err()
    bad = _finish_job(lib, [slab], dW=a)
    bad["slabs"][0] = None
    assert _finish(lib, [bad]) == E
    assert _finish(lib, [ok, _finish_job(lib, [slab[:, :128].contiguous()], dW=a, acc=1)]) == E and b"cannot join" in err()
    five = _finish_job(lib, [slab] * 5, dW=a)                # more series on one dW than a job takes
    assert _finish(lib, [five]) == E and b"cannot join" in err()
    assert _finish(lib, [_finish_job(lib, [slab], dW=wide[:, :128], cols=128, ld_dst=256, acc=1)]) == E and b"accumulating" in err()
    assert _finish(lib, [_finish_job(lib, [slab], nk4=32, dW=a, dbias=None)]) == E         # a bias tail without dbias
    assert lib.load().mmg_grad_finish_group(None, 1, None, 0, _stream()) == E
    assert lib.load().mmg_grad_finish_group(None, 0, None, 0, _stream()) == E
    assert _finish(lib, [_finish_job(lib, [slab], dW=a, srcs=[b[1:], c])]) == E and b"multiples of four" in err()
    torch.cuda.synchronize()
    assert float(a.abs().max()) == 0.0 and float(b.abs().max()) == 0.0       # nothing was launched
