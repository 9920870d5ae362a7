"""The host-side launch plan of the dense GEMMs (csrc/gemm.hip), restated in plain Python -- no torch, no library.

plan_wgrad, fwd_x6_rows, fwd_k256_rows, linear_fwd_launch and xcd_tile_map decide on the host which kernel instance runs,
with which grid, and which (tile, row set) a workgroup takes.  tests/test_dense_plan_cpu.py holds this restatement against
what the library exports without a GPU (workspace sizes, the direct / split query); tests/test_dense_plan_gpu.py takes its
shapes from the tables below and asserts from the probe of every launch that the symbol and the grid are the restated ones,
so a retuned plan fails the case that sat on the old edge instead of silently moving it off.
"""
from collections import namedtuple

WG_ROWS = 32          # rows of one weight-gradient stage (and of one forward tile)
RING = 4              # stages a weight-gradient workgroup keeps in flight in registers
SMALL_MAX_M = 512     # linear_fwd_launch: k_linear_small up to here, the split kernels from 513
DIRECT_MAX_M = 256    # plan_wgrad: one workgroup per output tile writes dW itself up to here
SIZES = (64, 128, 192, 256, 320)


def tf(b):
    return "true" if b else "false"


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------ xcd_tile_map
def xcd_on(nx, ny):
    return nx > 1 and ny % 8 == 0


def xcd_map(bx, by, nx, ny):
    """(blockIdx.x, blockIdx.y) of a grid (nx, ny) -> the (tile, row set) that workgroup works on."""
    if not xcd_on(nx, ny):
        return bx, by
    L = bx + nx * by
    j = L >> 3
    return j % nx, (j // nx) * 8 + (L & 7)


# ------------------------------------------------------------------------------------------ mmg_linear_wgrad
WgradPlan = namedtuple("WgradPlan", "M N K TN TK n_tiles n_split rows_per_split direct remap symbol grid block")


def wgrad_symbol(N, K, pro=False):
    TN, TK = (128 if N % 128 == 0 else 64), (128 if K % 128 == 0 else 64)
    if TN == 128 and TK == 128 and not pro:
        return "k_linear_wgrad_ws"
    wnn, wnk = {(128, 128): (4, 2), (128, 64): (4, 2), (64, 128): (2, 4), (64, 64): (2, 2)}[(TN, TK)]
    return f"k_linear_wgrad_x6<{TN}, {TK}, {wnn}, {wnk}, {tf(pro)}>"


def wgrad_block(N, K, pro=False):
    return 256 if (N % 128 and K % 128) else 512


def plan_wgrad(M, N, K, pro=False):
    TN, TK = (128 if N % 128 == 0 else 64), (128 if K % 128 == 0 else 64)
    n_tiles = (N // TN) * (K // TK)
    max_split = max(cdiv(M, WG_ROWS), 1)
    want = max(256 // n_tiles, 1)
    n_split = min(want, max_split)
    if M <= DIRECT_MAX_M:
        n_split = 1
    rps = max(cdiv(cdiv(M, n_split), WG_ROWS) * WG_ROWS, WG_ROWS)
    n_split = max(cdiv(M, rps), 1)
    return WgradPlan(M, N, K, TN, TK, n_tiles, n_split, rps, n_split == 1, xcd_on(n_tiles, n_split),
                     wgrad_symbol(N, K, pro), (n_tiles, n_split, 1), wgrad_block(N, K, pro))


def wgrad_ws_bytes(M, N, K):
    return plan_wgrad(M, N, K).n_split * (N * K + N) * 4 + 256


def wgrad_stages(M, n_split, y):
    """The 32-row stages of stage set y: dealt round-robin, y, y + n_split, ..."""
    return list(range(y, cdiv(M, WG_ROWS), n_split))


def stage_rows(M, stage):
    return min(WG_ROWS, M - stage * WG_ROWS)


def wgrad_stage_counts(M, N, K):
    """The set of stage counts over the workgroups of the launch."""
    p = plan_wgrad(M, N, K)
    return {len(wgrad_stages(M, p.n_split, y)) for y in range(p.n_split)}


def last_stage_rows(M):
    return stage_rows(M, cdiv(M, WG_ROWS) - 1)


def wgrad_tile_origin(N, K, bx):
    """(tn0, tk0) of output tile bx (after the remap)."""
    p = plan_wgrad(WG_ROWS, N, K)
    tiles_k = K // p.TK
    return (bx // tiles_k) * p.TN, (bx % tiles_k) * p.TK


def smallest_m(N, K, prop, m_max=1 << 16):
    """The smallest M whose weight-gradient launch has the property:
    "remap_5_stages"  the XCD remap is on and some workgroup walks >= 5 stages (past one turn of the 4-stage ring);
    "remap_ragged"    the XCD remap is on and the last stage holds fewer than 32 rows."""
    if prop not in ("remap_5_stages", "remap_ragged"):
        raise ValueError(prop)
    for M in range(DIRECT_MAX_M + 1, m_max):
        if not plan_wgrad(M, N, K).remap:
            continue
        if prop == "remap_5_stages" and max(wgrad_stage_counts(M, N, K)) > RING:
            return M
        if prop == "remap_ragged" and M % WG_ROWS:
            return M
    raise ValueError(f"no M below {m_max} with {prop} at N = {N}, K = {K}")


# ------------------------------------------------------------------------------------------ mmg_linear_fwd
FwdPlan = namedtuple("FwdPlan", "M N K family BN n_slices gy remap symbol grid block")


def fwd_symbol(K, N, pro=False, acc=False, l2=False, nbn=False, stats=False, p=0.0):
    """The instance of the split kernels (M > 512) as the probe names it."""
    if K == 256 and N % 256 == 0:
        return f"k_linear_fwd_h3_k256<{2 if pro and p > 0 else int(pro)}, {tf(acc)}, {tf(stats)}, 8>"
    wn = 4 if N % 128 == 0 else 2
    return f"k_linear_fwd_x6<{K}, {wn}, {tf(pro)}, {tf(acc)}, {tf(l2)}, {tf(nbn)}>"


def fwd_supported(M, N, K):
    return M >= 0 and K in (64, 128, 256) and N > 0 and N % 64 == 0 and N <= 4096


def fwd_k256_rows(M, N):
    return min(max(256 // (N // 256), 1), cdiv(M, 32))


def fwd_x6_rows(M, N, BN, K=128):
    gy = ((768 if BN == 64 else 512) if K <= 128 else 256) // (N // BN)
    return min(max(gy, 1), cdiv(M, 32))


def plan_fwd(M, N, K, **inst):
    """inst: the keywords of fwd_symbol (pro, acc, l2, stats, p).  The affine part of a prologue does not pick the x6
    instance; for the h3 kernel pro with p > 0 means BatchNorm fold AND dropout (instance 2)."""
    assert fwd_supported(M, N, K)
    if M <= SMALL_MAX_M:
        nx, ny = N // 32, cdiv(M, 32)
        return FwdPlan(M, N, K, "small", 32, nx, ny, False, f"k_linear_small<{K}>", (nx, ny, 1), 256)
    if K == 256 and N % 256 == 0:
        nx, gy = N // 256, fwd_k256_rows(M, N)
        # (this kernel reads blockIdx itself: no remap)
        return FwdPlan(M, N, K, "h3", 256, nx, gy, False, fwd_symbol(K, N, **inst), (nx, gy, 1), 512)
    BN = 128 if N % 128 == 0 else 64
    nx, gy = N // BN, fwd_x6_rows(M, N, BN, K)
    return FwdPlan(M, N, K, "x6", BN, nx, gy, xcd_on(nx, gy), fwd_symbol(K, N, **inst), (nx, gy, 1), 2 * BN)


def fwd_tiles_per_row_set(M, gy):
    """The set of tile counts over the row sets of a forward launch."""
    t = cdiv(M, 32)
    return {len(range(y, t, gy)) for y in range(gy)}


# ------------------------------------------------------------------------------------------ the cases of the GPU file
# (M, N, K) -> what the case exists for; tests/test_dense_plan_cpu.py asserts every entry against the plan above
WgradWant = namedtuple("WgradWant", "n_tiles n_split remap stages last_rows why")
WGRAD_CASES = {
    (256, 128, 128): WgradWant(1, 1, False, {8}, 32, "the last direct M, one tile"),
    (257, 128, 128): WgradWant(1, 9, False, {1}, 1, "the first split M: the last workgroup has one row"),
    (256, 256, 256): WgradWant(4, 1, False, {8}, 32, "the last direct M, four tiles"),
    (257, 256, 256): WgradWant(4, 9, False, {1}, 1, "the first split M, four tiles"),
    (200, 256, 256): WgradWant(4, 1, False, {7}, 8, "direct write with several tiles"),
    (500, 256, 256): WgradWant(4, 16, True, {1}, 20, "remap on at the smallest size"),
    (500, 256, 128): WgradWant(2, 16, True, {1}, 20, "remap, two tiles"),
    (500, 192, 64): WgradWant(3, 16, True, {1}, 20, "remap, odd tile count, 64 x 64 tiles along n"),
    (500, 64, 192): WgradWant(3, 16, True, {1}, 20, "remap, odd tile count, 64 x 64 tiles along k"),
    (500, 320, 128): WgradWant(5, 16, True, {1}, 20, "remap, five 64 x 128 tiles"),
    (1000, 192, 192): WgradWant(9, 16, True, {2}, 8, "3 x 3 tile grid under the remap"),
    (4090, 256, 256): WgradWant(4, 64, True, {2}, 26, "remap with a ragged tail"),
    (4090, 192, 128): WgradWant(3, 64, True, {2}, 26, "remap with a ragged tail, 64 x 128 tiles"),
    (10230, 256, 256): WgradWant(4, 64, True, {5}, 22, "remap past one turn of the 4-stage ring"),
    (20470, 256, 128): WgradWant(2, 128, True, {5}, 22, "remap past one turn of the ring, 128 stage sets"),
    (10230, 256, 128): WgradWant(2, 107, False, {2, 3}, 22, "the same tiles with the remap off"),
}
# the direct path (M <= 256) at every tile shape: the kernels' direct_accumulate == 2 against an independent reference
DIRECT_SIZES = ((128, 128), (64, 128), (128, 64), (64, 64))
DIRECT_MS = (200, 256)
# the finder's shapes: (N, K, property)
FOUND = ((256, 256, "remap_5_stages"), (192, 128, "remap_5_stages"), (256, 256, "remap_ragged"), (64, 192, "remap_ragged"))


def wgrad_shapes():
    """Every weight-gradient shape of the GPU file, in a fixed order, without repeats."""
    out = list(WGRAD_CASES)
    out += [(M, N, K) for M in DIRECT_MS for N, K in DIRECT_SIZES]
    out += [(smallest_m(N, K, prop), N, K) for N, K, prop in FOUND]
    return list(dict.fromkeys(out))


FwdWant = namedtuple("FwdWant", "family n_slices gy remap tiles why")
FWD_SWITCH_KN = ((64, 64), (128, 128), (128, 64), (256, 64), (256, 256))          # (K, N) at M = 512 | 513
FWD_CASES = {                                                                     # (M, N, K)
    (1000, 192, 64): FwdWant("x6", 3, 32, True, {1}, "three 64-column slices under the remap"),
    (1000, 192, 128): FwdWant("x6", 3, 32, True, {1}, "three 64-column slices, K = 128"),
    (1000, 384, 128): FwdWant("x6", 3, 32, True, {1}, "three 128-column slices"),
    (1000, 320, 256): FwdWant("x6", 5, 32, True, {1}, "five 64-column slices of the K = 256 six-term kernel"),
    (1000, 1024, 256): FwdWant("h3", 4, 32, False, {1}, "four 256-column slices of the f16 kernel (it does not remap)"),
    (9000, 192, 128): FwdWant("x6", 3, 256, True, {1, 2}, "remap with two tiles on some row sets"),
    (520, 4096, 128): FwdWant("x6", 32, 16, True, {1, 2}, "the widest N: 32 slices"),
    (520, 4096, 256): FwdWant("h3", 16, 16, False, {1, 2}, "the widest N of the f16 kernel: 16 slices"),
    (520, 4032, 64): FwdWant("x6", 63, 12, False, {1, 2}, "63 slices, remap off"),
}
