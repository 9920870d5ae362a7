"""The slab plans behind csrc/gram64.h as the libraries answer them on the host -- no GPU needed.  Every literal was
recorded from the build of the commit BEFORE the three kernels moved onto the shared header (assoc.hip, chain.hip and
pca.hip each restated the plan then), so a change of gram64_plan, of a user's constants or of a workspace layout cannot
pass quietly.  n: one row, around the 256-row minimum slab, the first n with a second slab (257; 65 for the Gram of
pca.hip, whose minimum is 64 rows; at D = 4 its workspace first grows at 129), the x100 patient count and the largest n
taken, 2^31 - 2; n = 2^31 - 1 is refused."""
import ctypes as C

import pytest

BIG = 2 ** 31 - 1          # refused: n < 2^31 - 1

# (rows per slab, slabs) by n, the same for every L up to 64 and, from 183,400 rows on, per number of block pairs
SMALL = {1: (256, 1), 255: (256, 1), 256: (256, 1), 257: (256, 2)}
LARGE = {183400: {1: (384, 478), 3: (1088, 169), 6: (2176, 85), 36: (13120, 14)},
         BIG - 1: {1: (4194304, 512), 3: (12632288, 170), 6: (25264544, 85), 36: (153391712, 14)}}
PAIRS = {1: 1, 64: 1, 65: 3, 128: 3, 130: 6, 512: 36}

# moments workspace bytes by (n, L)
ASSOC_WS = {(1, 1): 512, (1, 64): 131328, (1, 65): 135680, (1, 128): 524544, (1, 130): 541184, (1, 512): 8388864,
            (257, 1): 512, (257, 64): 262400, (257, 65): 270848, (257, 128): 1048832, (257, 130): 1081856,
            (257, 512): 16777472,
            (183400, 1): 15616, (183400, 64): 62652672, (183400, 65): 22849280, (183400, 128): 88604928,
            (183400, 130): 45968384, (183400, 512): 117440768,
            (BIG - 1, 1): 16640, (BIG - 1, 64): 67109120, (BIG - 1, 65): 22984448, (BIG - 1, 128): 89129216,
            (BIG - 1, 130): 45968384, (BIG - 1, 512): 117440768}
CHAIN_WS = {(1, 1): 1024, (1, 64): 33792, (1, 65): 35328, (1, 128): 132608,
            (257, 1): 1024, (257, 64): 67072, (257, 65): 69632, (257, 128): 264704,
            (183400, 1): 11776, (183400, 64): 15911936, (183400, 65): 5802240, (183400, 128): 22326016,
            (BIG - 1, 1): 12544, (BIG - 1, 64): 17043712, (BIG - 1, 65): 5836544, (BIG - 1, 128): 22458112}
# mmg_centered_gram_ws_bytes by (n, D): the mean slabs and the Gram slabs
PCA_WS = {(2, 4): 768, (2, 64): 33536, (2, 68): 38144, (2, 256): 526592,
          (65, 4): 768, (65, 64): 66304, (65, 68): 75008, (65, 256): 1050880,
          (129, 4): 1024,
          (255, 4): 1024, (255, 64): 131840, (255, 68): 148992, (255, 256): 2099456,
          (256, 4): 1024, (256, 64): 131840, (256, 68): 148992, (256, 256): 2099456,
          (257, 4): 1280, (257, 64): 165120, (257, 68): 186624, (257, 256): 2625792,
          (183400, 4): 108544, (183400, 64): 23756544, (183400, 68): 9526272, (183400, 256): 40892672,
          (BIG - 1, 4): 114944, (BIG - 1, 64): 25428224, (BIG - 1, 68): 9748736, (BIG - 1, 256): 40894720}


def plan_of(lib, symbol, n, L):
    rows, slabs = C.c_int64(-7), C.c_int(-7)
    return getattr(lib, symbol)(n, L, C.byref(rows), C.byref(slabs)), rows.value, slabs.value


def check_satellite(mod, stem, ws_table, labs, first_refused_L):
    import mmgnn  # noqa: F401
    from mmgnn import _lib
    lib = mod.load()
    plan, ws = f"mmg_{stem}_plan", getattr(lib, f"mmg_{stem}_moments_ws_bytes")
    for L in labs:
        for n, want in SMALL.items():
            assert plan_of(lib, plan, n, L) == (0,) + want, (n, L)
            assert getattr(mod, f"{stem}_plan")(n, L) == want                       # the Python caller of the same symbol
            assert ws(n, L) == ws_table[(1 if n < 257 else 257, L)], (n, L)         # one slab's workspace up to 256 rows
        for n, by_pairs in LARGE.items():
            assert plan_of(lib, plan, n, L) == (0,) + by_pairs[PAIRS[L]], (n, L)
            assert ws(n, L) == ws_table[(n, L)], (n, L)
        assert plan_of(lib, plan, BIG, L) == (_lib.MMG_E_ARG, -7, -7) and ws(BIG, L) == 0
    for n, L in ((100, first_refused_L), (0, 8), (100, 0)):
        assert plan_of(lib, plan, n, L) == (_lib.MMG_E_ARG, -7, -7) and ws(n, L) == 0, (n, L)
    with pytest.raises(_lib.MmgError, match="labs"):
        getattr(mod, f"{stem}_plan")(100, first_refused_L)


def test_assoc_plan_and_workspace_are_the_recorded_ones():
    from mmgnn import assoc_ops
    check_satellite(assoc_ops, "assoc", ASSOC_WS, (1, 64, 65, 128, 130, 512), 513)


def test_chain_plan_and_workspace_are_the_recorded_ones():
    from mmgnn import chain_ops
    check_satellite(chain_ops, "chain", CHAIN_WS, (1, 64, 65, 128), 129)


def test_centered_gram_workspace_is_the_recorded_one():
    import mmgnn  # noqa: F401
    from mmgnn import _lib
    ws = _lib.load().mmg_centered_gram_ws_bytes
    for (n, D), want in PCA_WS.items():
        assert ws(n, D) == want, (n, D)
    for n, D in ((BIG, 4), (BIG, 64), (BIG, 68), (BIG, 256), (1, 64), (100, 66), (100, 260), (100, 0)):
        assert ws(n, D) == 0, (n, D)
