"""tests/dense_plan_ref.py against what the library answers on the host, and the properties its case tables promise --
no GPU needed.

The library exports two views of plan_wgrad: the workspace size (n_split slabs of N * K + N floats, + 256) and the direct /
split query.  The block -> (tile, row set) map is device code; its restatement is checked for what the kernels rely on: a
bijection of the grid whenever it is on, the identity otherwise.  The last tests assert, shape by shape, the property each
case of tests/test_dense_plan_gpu.py exists for, so an edit of the table or of the plan cannot quietly move a case."""
import random

import pytest

import dense_plan_ref as D


@pytest.fixture(scope="module")
def lib():
    import mmgnn  # noqa: F401
    from mmgnn import _lib
    return _lib.load()


def large_ms():
    rnd = random.Random(20261)
    ms = [rnd.randrange(1101, 2_000_000) for _ in range(300)]
    return ms + [1834, 9000, 183400, 1_834_000, 2 ** 31 + 5] + [32 * 256 * k + d for k in (1, 2, 7) for d in (-1, 0, 1)]


@pytest.mark.parametrize("N", D.SIZES)
def test_restated_weight_gradient_plan_equals_the_library(lib, N):
    for K in D.SIZES:
        for M in list(range(1, 1101)) + large_ms():
            p = D.plan_wgrad(M, N, K)
            assert lib.mmg_linear_wgrad_ws_bytes(M, N, K) == p.n_split * (N * K + N) * 4 + 256, (M, N, K, p)
            assert bool(lib.mmg_linear_wgrad_is_direct(M, N, K)) == (p.n_split == 1) == p.direct, (M, N, K, p)
            # what the kernels assume of a plan: every stage has an owner, no stage set is empty
            assert 1 <= p.n_split <= D.cdiv(M, D.WG_ROWS) and p.n_split * p.n_tiles <= max(256, p.n_tiles), (M, N, K, p)
            assert p.direct == (M <= D.DIRECT_MAX_M or M <= D.WG_ROWS)


def test_forward_support_query_equals_the_restatement(lib):
    for K in (32, 64, 128, 192, 256, 512):
        for N in (0, 32, 64, 192, 4032, 4096, 4160):
            for M in (0, 1, 512, 513, 100000):
                assert bool(lib.mmg_linear_fwd_supported(0, M, N, K)) == bool(D.fwd_supported(M, N, K)), (M, N, K)


@pytest.mark.parametrize("nx", list(range(1, 10)) + [32, 63])
def test_xcd_map_is_a_bijection_when_on_and_the_identity_when_off(nx):
    for ny in range(1, 73):
        cells = [(bx, by) for by in range(ny) for bx in range(nx)]
        img = [D.xcd_map(bx, by, nx, ny) for bx, by in cells]
        if ny % 8 == 0 and nx > 1:
            assert D.xcd_on(nx, ny)
            assert sorted(img) == sorted(cells), (nx, ny)
            # what the map is for: linear ids 8 apart (one XCD) are the tiles of one row set
            for bx, by in cells:
                L = bx + nx * by
                if (L >> 3) % nx:
                    Lp = L - 8
                    assert D.xcd_map(Lp % nx, Lp // nx, nx, ny)[1] == D.xcd_map(bx, by, nx, ny)[1]
        else:
            assert not D.xcd_on(nx, ny)
            assert img == cells, (nx, ny)
        if nx == 1 and ny % 8 == 0:
            assert img == cells
    if nx > 1:
        assert D.xcd_map(1, 0, nx, 8) != (1, 0)              # it does move workgroups


@pytest.mark.parametrize("shape", list(D.WGRAD_CASES), ids=lambda s: "x".join(map(str, s)))
def test_every_weight_gradient_case_sits_on_its_edge(shape):
    M, N, K = shape
    w, p = D.WGRAD_CASES[shape], D.plan_wgrad(*shape)
    assert (p.n_tiles, p.n_split, p.remap) == (w.n_tiles, w.n_split, w.remap), (p, w)
    assert p.direct == (w.n_split == 1) == (M <= 256)
    assert D.wgrad_stage_counts(M, N, K) == w.stages and D.last_stage_rows(M) == w.last_rows
    assert p.grid == (w.n_tiles, w.n_split, 1)
    # the stage sets partition the stages
    got = sorted(s for y in range(p.n_split) for s in D.wgrad_stages(M, p.n_split, y))
    assert got == list(range(D.cdiv(M, 32)))


def test_the_switch_points_of_the_weight_gradient():
    for N, K in ((128, 128), (256, 256), (64, 64), (320, 192)):
        assert D.plan_wgrad(256, N, K).direct and not D.plan_wgrad(257, N, K).direct
        assert D.plan_wgrad(257, N, K).n_split == 9 and D.wgrad_stages(257, 9, 8) == [8] and D.stage_rows(257, 8) == 1
    # the shapes the suite had before: none of them runs the remap ...
    for shape in ((50, 64, 128), (1834, 128, 128), (9000, 256, 256), (3, 128, 64), (264, 128, 128), (1834, 256, 256)):
        assert not D.plan_wgrad(*shape).remap, shape
    assert D.plan_wgrad(9000, 256, 256).n_split == 57 and D.plan_wgrad(1834, 256, 256).n_split == 58
    # ... which the 256-d model at the x100 scale does
    big = D.plan_wgrad(183400, 256, 256)
    assert (big.n_tiles, big.n_split, big.remap) == (4, 64, True)
    # tile shapes and instances
    assert D.wgrad_symbol(128, 128) == "k_linear_wgrad_ws" and D.wgrad_symbol(256, 256, True) == "k_linear_wgrad_x6<128, 128, 4, 2, true>"
    assert D.wgrad_symbol(320, 128) == "k_linear_wgrad_x6<64, 128, 2, 4, false>" and D.wgrad_block(320, 128) == 512
    assert D.wgrad_symbol(192, 64) == "k_linear_wgrad_x6<64, 64, 2, 2, false>" and D.wgrad_block(192, 64) == 256
    assert D.wgrad_symbol(256, 192) == "k_linear_wgrad_x6<128, 64, 4, 2, false>"
    assert [D.wgrad_tile_origin(192, 192, b) for b in (0, 1, 3, 8)] == [(0, 0), (0, 64), (64, 0), (128, 128)]
    assert D.wgrad_tile_origin(320, 128, 4) == (256, 0) and D.wgrad_tile_origin(256, 256, 1) == (0, 128)


@pytest.mark.parametrize("N,K,prop", D.FOUND)
def test_the_finder_returns_the_smallest_m(N, K, prop):
    M = D.smallest_m(N, K, prop)

    def has(m):
        p = D.plan_wgrad(m, N, K)
        if not p.remap:
            return False
        return max(D.wgrad_stage_counts(m, N, K)) >= 5 if prop == "remap_5_stages" else D.last_stage_rows(m) < 32

    assert M > 256 and has(M) and not any(has(m) for m in range(257, M))
    assert (M, N, K) in D.wgrad_shapes()
    with pytest.raises(ValueError):
        D.smallest_m(N, K, "no such property")


def test_the_direct_shapes_cover_every_tile_shape():
    shapes = D.wgrad_shapes()
    assert len(shapes) == len(set(shapes))
    for M in D.DIRECT_MS:
        assert {(D.plan_wgrad(M, N, K).TN, D.plan_wgrad(M, N, K).TK) for N, K in D.DIRECT_SIZES} == \
               {(128, 128), (64, 128), (128, 64), (64, 64)}
        for N, K in D.DIRECT_SIZES:
            assert (M, N, K) in shapes and D.plan_wgrad(M, N, K).direct and D.plan_wgrad(M, N, K).n_tiles == 1
    assert max(s[0] for s in shapes) == 20470          # the largest tensor of the GPU file: 20470 x 256


@pytest.mark.parametrize("K,N", D.FWD_SWITCH_KN)
def test_the_forward_switches_kernels_between_512_and_513(K, N):
    lo, hi = D.plan_fwd(512, N, K), D.plan_fwd(513, N, K)
    assert lo.family == "small" and lo.symbol == f"k_linear_small<{K}>" and lo.grid == (N // 32, 16, 1) and lo.block == 256
    assert hi.family == ("h3" if (K, N) == (256, 256) else "x6") and hi.gy == 17 and hi.grid == (1, 17, 1)
    assert D.fwd_tiles_per_row_set(513, 17) == {1} and 513 - 16 * 32 == 1            # the last tile holds one row
    assert hi.symbol.startswith("k_linear_fwd_") and not hi.remap


@pytest.mark.parametrize("shape", list(D.FWD_CASES), ids=lambda s: "x".join(map(str, s)))
def test_every_forward_case_sits_on_its_edge(shape):
    M, N, K = shape
    w, p = D.FWD_CASES[shape], D.plan_fwd(*shape)
    assert (p.family, p.n_slices, p.gy, p.remap) == (w.family, w.n_slices, w.gy, w.remap), (p, w)
    assert D.fwd_tiles_per_row_set(M, p.gy) == w.tiles
    assert p.n_slices >= 3 and p.n_slices * p.BN == N and p.grid == (w.n_slices, w.gy, 1)
    assert p.gy <= 768                                   # the rows of the statistics workspace (mmg_epi_ws_bytes)


def test_the_forward_instances():
    assert D.plan_fwd(520, 4096, 128).symbol == "k_linear_fwd_x6<128, 4, false, false, false, false>"
    assert D.plan_fwd(520, 4032, 64, pro=True, acc=True).symbol == "k_linear_fwd_x6<64, 2, true, true, false, false>"
    assert D.plan_fwd(520, 4096, 256, pro=True, p=0.2, stats=True).symbol == "k_linear_fwd_h3_k256<2, false, true, 8>"
    assert D.plan_fwd(1000, 320, 256).symbol == "k_linear_fwd_x6<256, 2, false, false, false, false>"
    assert D.plan_fwd(1000, 320, 256).block == 128 and D.plan_fwd(1000, 384, 128).block == 256
    assert max(N for _, N, _ in D.FWD_CASES) == 4096 and not D.fwd_supported(520, 4160, 128)
