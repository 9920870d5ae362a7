"""tests/agg_plan_ref.py against what the library answers on the host, and the properties its case tables promise -- no GPU
needed.

The library exports one view of the scatter plan: mmg_scatter_rows_ws_bytes (n_ranges or n_split slabs of total_pad * D
floats, + 256).  It is called with fake non-null pointers (never touched).  The other tests assert, row by row, the property
each case of tests/test_agg_plan_gpu.py exists for, and that the tables hold every value of every switch of the plan, so an
edit of a table or of the plan cannot quietly move a case off its edge."""
import ctypes
import random

import pytest

import agg_plan_ref as A
from agg_plan_ref import MULTI, NO_MASK_R, SIMPLE


@pytest.fixture(scope="module")
def binding():
    import mmgnn  # noqa: F401
    from mmgnn import _lib
    return _lib, _lib.load()


def ws_bytes(binding, sizes, flags, rs, D, n_rows):
    _lib, lib = binding
    p = ctypes.c_void_p(256)
    rels = (_lib.RelT * len(sizes))()
    for i, (nc, fl) in enumerate(zip(sizes, flags)):
        rels[i] = _lib.RelT(p, p, p if rs else None, None, None, p, nc, _lib.MMG_REL_SIMPLE if fl != MULTI else 0,
                            p if fl != MULTI else None, p if fl == SIMPLE else None)
    return lib.mmg_scatter_rows_ws_bytes(rels, len(sizes), n_rows, D)


sid = A.case_id


def test_restated_workspace_equals_the_library_for_every_scatter_case(binding):
    for sizes, flags, D, n, what in A.SCATTER_CASES:
        p = A.scatter_plan(sizes, flags, what.get("rs", False), D, n)
        assert ws_bytes(binding, sizes, flags, what.get("rs", False), D, n) == p.ws_bytes, (sizes, flags, D, n, p)


def test_restated_workspace_equals_the_library_on_random_layouts(binding):
    rnd = random.Random(20263)
    for _ in range(3000):
        n_rel = rnd.randrange(1, 5)
        sizes = tuple(rnd.choice((rnd.randrange(1, 40), rnd.randrange(1, 300), 32 * rnd.randrange(1, 9))) for _ in range(n_rel))
        flags = tuple(rnd.choice((SIMPLE, SIMPLE, SIMPLE, MULTI)) for _ in range(n_rel))
        D, rs = rnd.choice(A.DS), rnd.random() < 0.5
        n = rnd.choice((1, 31, 63, 64, 65, 100, 255, 256, 257, 1834, rnd.randrange(1, 70000), 183400))
        p = A.scatter_plan(sizes, flags, rs, D, n)
        assert ws_bytes(binding, sizes, flags, rs, D, n) == p.ws_bytes, (sizes, flags, rs, D, n, p)
        # what the kernels assume of a plan
        if p.path == "units":
            U, R, waves = p.inst
            assert waves == U * R <= A.SU_MAXW and sorted(p.wave_map) == [(u, q) for u in range(U) for q in range(R)]
            assert all(1 <= t[2] <= A.SU_NT for t in p.units) and p.total_pad <= 768
        if p.path == "mfma":
            assert p.n_slabs >= 1 and (p.n_slabs - 1) * A.mfma_rows_per_split(p, n) < n


def holds(plan, key, val, sizes, flags, D, n):
    if key in ("rs", "cycle", "steady"):                       # inputs of the case, not properties of the plan
        return True
    if key == "gy":
        return plan.grid[1] == val
    if key == "units":
        got = [(u[1], u[2]) for u in plan.units] if isinstance(plan, A.GatherPlan) else [u[2] for u in plan.units]
        return got == val
    if key in ("U", "R", "waves") and isinstance(plan, A.ScatterPlan):
        return plan.inst[("U", "R", "waves").index(key)] == val
    if key in ("NT", "KT"):
        return plan.path == "mfma" and plan.inst[("NT", "KT").index(key)] == val
    if key == "gather_units":                                   # the unit count that made plan_gather_units give up
        nk = [A.cdiv(A.pad32(s) // 16, A.GU_KU) for s in sizes]
        return sum(nk) == val and val > A.GU_MAXU
    if key == "scatter_units":
        return sum(A.cdiv(A.pad32(s) // 32, A.SU_NT) for s in sizes) == val and val > A.SU_MAXU
    if key == "tiles":
        return sum(A.pad32(s) // 32 for s in sizes) == val
    if key == "items":
        return sum(sizes) == val
    if key == "max_rows_per_wave":
        return max(A.lds_rows_per_wave(plan, n)) == val
    if key == "deep":                                           # every wave of a full block takes >= 4 rows; ragged blocks
        rows = A.lds_rows_per_wave(plan, n)
        return plan.rows_per_blk >= 64 and n % plan.rows_per_blk != 0 and max(rows) >= 5 and \
            min(len(range(w, plan.rows_per_blk, 16)) for w in range(16)) >= 4
    return getattr(plan, key) == val


@pytest.mark.parametrize("row", [r for r in A.GATHER_CASES if not r[4].get("steady")], ids=sid)
def test_every_gather_case_sits_on_its_edge(row):
    sizes, flags, D, n, what = row
    for acc in (False, True):
        p = A.gather_plan(sizes, flags, D, n, accumulate=acc)
        for k, v in what.items():
            assert holds(p, k, v, sizes, flags, D, n), (k, v, p)
        assert p.probed == (p.path not in ("plain",))
        if p.path == "units":
            assert p.block == 64 * p.U * p.FT <= 512 and p.grid[0] * p.grid[1] <= 256 and p.lds <= 4096 + 1024 + 2 * 6 * 4096
            for r in range(len(sizes)):                          # the units of a relation tile its k-steps, starts even
                ks = [(u[1], u[2]) for u in p.units if u[0] == r]
                assert ks[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(ks, ks[1:]))
                assert sum(k[1] for k in ks) == A.pad32(sizes[r]) // 16 and all(k[0] % 2 == 0 and 0 < k[1] <= 8 for k in ks)
        if p.path == "lds":
            assert p.lds <= A.GL_LDS_BUDGET and (p.grid[0] - 1) * p.rows_per_blk < n <= p.grid[0] * p.rows_per_blk


@pytest.mark.parametrize("row", [r for r in A.GATHER_CASES if r[4].get("steady")], ids=sid)
def test_the_steady_gather_cases_walk_past_the_look_ahead(row):
    """n_rows comes from the probe on the GPU; here: at the n the rule gives for the restated grid, workgroups walk 3 and 4
    tiles -- more than the GU_DEPTH = 3 register sets of look-ahead."""
    sizes, flags, D, _, what = row
    g = A.gather_plan(sizes, flags, D, 40_000).grid[0]
    n = 32 * (3 * g + g // 2) + 5
    p = A.gather_plan(sizes, flags, D, n)
    assert (p.path, p.U, p.FT) == (what["path"], what["U"], what["FT"]) and p.grid[0] == g
    assert A.gather_tiles_per_workgroup(p, n) == {3, 4} and max(A.gather_tiles_per_workgroup(p, n)) > A.GU_DEPTH


@pytest.mark.parametrize("row", A.SCATTER_CASES, ids=sid)
def test_every_scatter_case_sits_on_its_edge(row):
    sizes, flags, D, n, what = row
    p = A.scatter_plan(sizes, flags, what.get("rs", False), D, n)
    for k, v in what.items():
        assert holds(p, k, v, sizes, flags, D, n), (k, v, p)
    assert p.probed == (p.path != "atomic")
    if p.path == "mfma":
        assert p.inst[2] == what.get("rs", False) and p.grid == (p.n_slabs, 1 if D < 256 else 2, 1)


def gplans(pred=lambda r: True):
    return [(r, A.gather_plan(*r[:4])) for r in A.GATHER_CASES if not r[4].get("steady") and pred(r)]


def splans():
    return [(r, A.scatter_plan(r[0], r[1], r[4].get("rs", False), r[2], r[3])) for r in A.SCATTER_CASES]


def test_the_gather_table_holds_every_switch_value():
    gp = gplans()
    assert {p.path for _, p in gp} == {"bits3", "bits1", "units", "lds", "plain"}
    un = [(r, p) for r, p in gp if p.path == "units"]
    # every unit count, every FT, the pairs the suite never ran before: U = 1, U = 2 with FT = 4, U = 5 and 6 with FT = 1
    assert {p.U for _, p in un} == {1, 2, 3, 4, 5, 6} and {p.FT for _, p in un} == {1, 2, 4}
    assert {(1, 2), (1, 4), (2, 2), (2, 4), (3, 2), (4, 2), (5, 1), (6, 1)} == {(p.U, p.FT) for _, p in un}
    assert {p.grid[1] for _, p in un} == {1, 2, 4, 8}                                   # gy > 1 occurs
    chunkings = {tuple(u[2] for u in p.units if u[0] == r) for _, p in un for r in range(4)}
    assert {(6, 4), (8, 6, 6), (8, 6), (8, 8), (2,), (4,), (8,)} <= chunkings
    assert any(len(r[0]) == 4 for r, _ in un) and any(sum(A.pad32(s) for s in r[0]) == 768 for r, _ in un)
    for sizes in {r[0] for r, _ in un if r[3] == 1834}:
        assert {r[3] for r, _ in un if r[0] == sizes} >= {32, 63, 65, 1834}
        assert {r[2] for r, _ in un if r[0] == sizes} == set(A.DS)
    # one tile; one workgroup with two tiles and a ragged one; many tiles per launch
    assert {A.cdiv(r[3], 32) for r, _ in un} >= {1, 2, 3, 58}
    # the bits instances on both sides of their vocabulary edges and of D = 64 | 128
    for sizes in ((33, 97, 97), (64, 128, 128), (33,), (64,)):
        for n in (32, 33, 1000):
            paths = [A.gather_plan(sizes, (SIMPLE,) * len(sizes), D, n).path for D in A.DS]
            assert paths == ["units"] + ["bits3" if len(sizes) == 3 else "bits1"] * 2
            assert (sizes, (SIMPLE,) * len(sizes), 128, n) in {r[:4] for r, _ in gp}
    assert A.gather_plan((32, 97, 97), A.S3, 128, 1000).path == "units" and A.gather_plan((65,), A.S1, 128, 1000).path == "units"
    # fall-throughs
    assert A.gather_plan(A.EICU, A.S3, 128, 31).path == "plain" and A.gather_plan(A.EICU, A.S3, 128, 32).path == "bits3"
    assert any(p.path == "lds" and NO_MASK_R in r[1] for r, p in gp)
    assert any(p.path == "lds" and set(r[1]) == {SIMPLE, MULTI} for r, p in gp)
    # k_gather_lds: both instances under every D, the 63 | 64 switch, the 300 | 301 and 600 | 601 column switches
    ld = [(r, p) for r, p in gp if p.path == "lds"]
    assert {(r[2], p.dc) for r, p in ld} == {(64, 64), (128, 128), (256, 128), (128, 64), (256, 64)}
    for sizes, fl in ((A.EICU, A.M3), ((20,), A.M1)):
        for D in A.DS:
            assert [A.gather_plan(sizes, fl, D, n).path for n in (63, 64, 65)] == ["plain", "lds", "lds"]
    for D in (128, 256):
        got = [(A.gather_plan(s, A.M2, D, 200).path, A.gather_plan(s, A.M2, D, 200).dc)
               for s in ((150, 150), (151, 150), (300, 300), (301, 300))]
        assert got == [("lds", 128), ("lds", 64), ("lds", 64), ("plain", None)]
    deep = [(r, p) for r, p in ld if r[4].get("deep")]
    assert {(r[2], p.dc, p.grid[1]) for r, p in deep} == {(64, 64, 1), (128, 128, 1), (256, 128, 2)}
    assert all(max(c for c in r[4]["cycle"]) >= 65 for r, _ in deep)
    # k_gather: one workgroup, two, a ragged last one; wide vocabularies; every D
    pl = [(r, p) for r, p in gp if p.path == "plain" and MULTI in r[1]]
    assert {r[3] for r, _ in pl} >= {1, 5, 63, 300} and {r[2] for r, _ in pl} == set(A.DS)
    assert any(sum(r[0]) > 600 for r, _ in pl)
    assert max(A.DEGREE_CYCLE) > 128 and {63, 64, 65} <= set(A.DEGREE_CYCLE) and 0 in A.DEGREE_CYCLE


def test_the_scatter_table_holds_every_switch_value():
    sp = splans()
    assert {p.path for _, p in sp} == {"strip", "units", "mfma", "atomic"}
    mf = [(r, p) for r, p in sp if p.path == "mfma"]
    assert {p.inst for _, p in mf} == {(nt, kt, rs) for nt in A.MFMA_NT for kt in (2, 4) for rs in (False, True)}
    assert {(r[2], p.inst[1]) for r, p in mf} == {(64, 2), (128, 4), (256, 4)}
    assert {r[3] for r, p in mf if set(r[1]) == {MULTI}} == {1, 33, 100, 1834}
    assert any(r[3] % A.mfma_rows_per_split(p, r[3]) not in (0,) and p.n_slabs > 1 for r, p in mf)       # ragged last split
    for D in A.DS:
        for rs in (False, True):
            assert A.scatter_plan((512,), A.M1, rs, D, 100).inst == (16, 2 if D == 64 else 4, rs)
            assert A.scatter_plan((513,), A.M1, rs, D, 100).path == "atomic"
        assert [A.scatter_plan(A.EICU, A.S3, False, D, n).path for n in (63, 64)] == ["mfma", "strip"]
        assert [A.scatter_plan(s, A.S3, False, D, 1834).path for s in ((152, 100, 100), (153, 100, 100))] == ["strip", "units"]
    assert any(set(r[1]) == {SIMPLE, MULTI} and p.inst[0] == 10 for r, p in mf)
    un = [(r, p) for r, p in sp if p.path == "units"]
    assert {p.inst for _, p in un} == {(1, 4, 4), (2, 4, 8), (4, 3, 12), (5, 2, 10), (6, 2, 12)}
    assert {r[3] for r, _ in un} == {64, 65, 1834} and {r[2] for r, _ in un} == set(A.DS)
    assert {bool(r[4].get("rs")) for r, _ in un} == {False, True}
    # the greedy placement spreads the tiles of every SIMD evenly where they divide: 6 units of 4 tiles on 12 waves
    p6 = A.scatter_plan((256, 256, 256), A.S3, True, 128, 1834)
    assert [sum(p6.units[p6.wave_map[w][0]][2] for w in range(s, 12, 4)) for s in range(4)] == [12] * 4
    at = [(r, p) for r, p in sp if p.path == "atomic"]
    assert any(r[0] == (270, 270, 40) and r[4].get("rs") for r, _ in at) and any(r[0] == (513,) for r, _ in at)
