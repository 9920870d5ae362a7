"""The host-side launch plan of the sparse aggregates (csrc/aggregate.hip), restated in plain Python -- no torch, no library.

gather_launch / plan_gather_units choose between five gather kernels, plan_strip / plan_units / plan_scatter between five
scatter kernels, from the vocabulary layout (relation count, order, padded sizes), MMG_REL_SIMPLE and the bit planes,
rowscale, D and n_rows.  tests/test_agg_plan_cpu.py holds this restatement against the library's workspace query and
asserts what every row of the tables below is for; tests/test_agg_plan_gpu.py takes its shapes ONLY from these tables and
asserts from the probe of every launch that the restated symbol, grid and block ran -- a retuned plan fails the case that
sat on the old edge instead of silently moving it off.

A relation's flag: MULTI (a multigraph: no MMG_REL_SIMPLE, no bit planes), SIMPLE (the flag and both bit planes), NO_MASK_R
(simple, but the row-major planes of the gather side withheld: the gather then may not take a bit-plane kernel).
"""
from collections import namedtuple

MULTI, SIMPLE, NO_MASK_R = 0, 1, 2

GU_KU, GU_MAXU, GU_DEPTH = 8, 6, 3            # gather units: k-steps (16 items) per unit, units per launch, look-ahead
GL_THREADS, GL_LDS_BUDGET = 1024, 150 * 1024   # k_gather_lds
SC_ROWS, SB_SR = 32, 64                        # rows per stage: k_scatter_mfma, the bit-plane scatters
SU_NT, SU_MAXU, SU_MAXW = 4, 6, 12             # scatter units: tiles per unit, units per launch, waves per workgroup
MFMA_NT = (2, 4, 6, 8, 10, 12, 16)
STRIP_INST = {8: (4, 4), 9: (5, 4), 10: (5, 5), 11: (6, 5)}
DEGREE_CYCLE = (0, 1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 72, 129, 200)     # multigraph rows, in turn
LIGHT_CYCLE = (0, 1, 3, 5, 8, 9, 65, 72)                              # ... of the many-row cases


def tf(b):
    return "true" if b else "false"


def cdiv(a, b):
    return (a + b - 1) // b


def pad32(n):
    return (n + 31) & ~31


def _flags(sizes, simple):
    simple = tuple(simple)
    assert len(simple) == len(sizes) and 1 <= len(sizes) <= 4 and all(s > 0 for s in sizes)
    return simple


# ------------------------------------------------------------------------------------------ mmg_gather_rows
GatherPlan = namedtuple("GatherPlan", "path symbol grid block probed units U FT waves dc rows_per_blk lds")


def gather_units(sizes, simple, D, n_rows):
    """plan_gather_units -> ([(rel, ks0, nks)], FT) or None."""
    if D % 32 or n_rows < 32 or n_rows * D * 4 >= 1 << 31:
        return None
    units = []
    for r, (nc, fl) in enumerate(zip(sizes, simple)):
        if fl != SIMPLE:
            return None
        nk = pad32(nc) // 16
        chunks = cdiv(nk, GU_KU)
        k0 = 0
        for c in range(chunks):
            n = cdiv(nk - k0, chunks - c)
            n = (n + 1) & ~1                           # even: the fields are read as dwords
            n = min(n, nk - k0)
            if len(units) >= GU_MAXU:
                return None
            units.append((r, k0, n))
            k0 += n
    U, tiles_d, FT = len(units), D // 32, 4
    while FT > 1 and (FT * U > 8 or tiles_d % FT):
        FT >>= 1
    return (units, FT) if FT * U <= 8 else None


def gather_plan(sizes, simple, D, n_rows, accumulate=False, nbn=False):
    """-> GatherPlan.  path: bits3 | bits1 | units | lds | plain.  accumulate / nbn only pick the template instance."""
    simple = _flags(sizes, simple)
    assert D in (64, 128, 256) and n_rows >= 1
    n_rel, total = len(sizes), sum(sizes)
    n_tiles = cdiv(n_rows, 32)
    okb = n_rel in (1, 3) and D >= 128 and n_rows >= 32 and n_rows * D * 4 < 1 << 32
    okb = okb and all(f == SIMPLE for f in simple) and pad32(sizes[0]) == 64
    if n_rel == 3:
        okb = okb and pad32(sizes[1]) == 128 and pad32(sizes[2]) == 128
    if okb:
        ndc = D // 128
        g = min(256 // ndc, n_tiles)
        nk = "20, 4, 12" if n_rel == 3 else "4, 4, 4"
        return GatherPlan("bits3" if n_rel == 3 else "bits1", f"k_gather_bits<{nk}, {tf(accumulate)}, {tf(nbn)}>",
                          (g, ndc, 1), 512, True, None, None, None, 8, None, None, 0)
    gu = gather_units(sizes, simple, D, n_rows)
    if gu is not None:
        units, FT = gu
        U = len(units)
        gy = (D // 32) // FT
        g = min(max(256 // gy, 1), n_tiles, 256)
        lds = 4096 + 8 * 32 * 4 + 2 * FT * max(U - 1, 1) * 16 * 64 * 4
        return GatherPlan("units", f"k_gather_units<{tf(accumulate)}>", (g, gy, 1), 64 * FT * U, True, units, U, FT, FT * U,
                          None, None, lds)
    dc = 128 if D >= 128 else 64
    while dc > 64 and total * dc * 4 > GL_LDS_BUDGET:
        dc >>= 1
    if total * dc * 4 <= GL_LDS_BUDGET and n_rows >= 64:
        ndc = D // dc
        nblk = min(max(256 // ndc, 1), cdiv(n_rows, 16))
        rpb = cdiv(n_rows, nblk)
        nblk = cdiv(n_rows, rpb)
        return GatherPlan("lds", f"k_gather_lds<{dc // 64}>", (nblk, ndc, 1), GL_THREADS, True, None, None, None, 16, dc, rpb,
                          total * dc * 4)
    # (launched without the probe hook)
    return GatherPlan("plain", f"k_gather<{D // 64}>", (cdiv(n_rows, 4), 1, 1), 256, False, None, None, None, 4, None, None, 0)


def gather_tiles_per_workgroup(plan, n_rows):
    """The set of 32-row tile counts over the workgroups of a bits / units launch (tiles are dealt round-robin)."""
    t = cdiv(n_rows, 32)
    return {len(range(b, t, plan.grid[0])) for b in range(plan.grid[0])}


def lds_rows_per_wave(plan, n_rows):
    """The set of row counts over the waves of a k_gather_lds launch (wave w of a block takes rows w, w + 16, ...)."""
    out = set()
    for b in range(plan.grid[0]):
        rows = min(n_rows, (b + 1) * plan.rows_per_blk) - b * plan.rows_per_blk
        out |= {len(range(w, rows, 16)) for w in range(16)}
    return out


# ------------------------------------------------------------------------------------------ mmg_scatter_rows
ScatterPlan = namedtuple("ScatterPlan", "path symbol grid block probed inst n_slabs total_pad ws_bytes units wave_map")


def scatter_units(sizes, simple, n_rows):
    """plan_units -> ([(rel, tile0, ntiles, out_tile)], R, [(unit, row sub-range) of wave w]) or None."""
    units, tile_off = [], 0
    for r, (nc, fl) in enumerate(zip(sizes, simple)):
        if fl == MULTI:
            return None
        tiles = pad32(nc) // 32
        chunks = cdiv(tiles, SU_NT)
        t0 = 0
        for c in range(chunks):
            nt = cdiv(tiles - t0, chunks - c)               # balanced: 7 -> 4 + 3
            if len(units) >= SU_MAXU:
                return None
            units.append((r, t0, nt, tile_off + t0))
            t0 += nt
        tile_off += tiles
    if n_rows < SB_SR:
        return None
    U = len(units)
    R = 4 if U <= 3 else (3 if U == 4 else 2)
    n_waves = U * R
    # greedy: heaviest unit first onto the SIMD (wave id % 4) with the least tiles that still has a free slot
    load, used, slots = [0] * 4, [0] * 4, cdiv(n_waves, 4)
    order = list(range(U))
    for i in range(U):
        for j in range(i + 1, U):
            if units[order[j]][2] > units[order[i]][2]:
                order[i], order[j] = order[j], order[i]
    wave_map = [None] * n_waves
    for u in order:
        for rq in range(R):
            best = -1
            for sd in range(4):
                if used[sd] >= slots or sd + 4 * used[sd] >= n_waves:
                    continue
                if best < 0 or load[sd] < load[best]:
                    best = sd
            assert best >= 0
            wave_map[best + 4 * used[best]] = (u, rq)
            load[best] += units[u][2]
            used[best] += 1
    return units, R, wave_map


def scatter_plan(sizes, simple, has_rowscale, D, n_rows):
    """-> ScatterPlan.  path: strip | units | mfma | atomic; inst: (NA, NB) | (U, R, waves) | (NT, KT, HAS_RS) | None;
    n_slabs: n_ranges (strip, units) or n_split (mfma); ws_bytes: what mmg_scatter_rows_ws_bytes returns."""
    simple = _flags(sizes, simple)
    assert D in (64, 128, 256) and n_rows >= 1
    strips, nst = D // 32, cdiv(n_rows, SB_SR)
    all_simple = all(f != MULTI for f in simple)
    items = sum(sizes)
    tiles = cdiv(items, 32)
    if all_simple and tiles <= 11 and n_rows >= SB_SR and not has_rowscale:
        nt = min(k for k in STRIP_INST if tiles <= k)
        nr = 256 // strips
        if nr * 4 > nst:
            nr = cdiv(nst, 4)
        nr = max(nr, 1)
        na, nb = STRIP_INST[nt]
        return ScatterPlan("strip", f"k_scatter_strip2<{na}, {nb}>", (nr, strips, 1), 512, True, (na, nb), nr, nt * 32,
                           nr * nt * 32 * D * 4 + 256, None, None)
    su = scatter_units(sizes, simple, n_rows)
    if su is not None:
        units, R, wave_map = su
        total_pad = sum(pad32(s) for s in sizes)
        nr = max(min(256 // strips, nst), 1)
        return ScatterPlan("units", f"k_scatter_units<{tf(has_rowscale)}>", (nr, strips, 1), 64 * len(units) * R, True,
                           (len(units), R, len(units) * R), nr, total_pad, nr * total_pad * D * 4 + 256, units, wave_map)
    ptiles = sum(pad32(s) // 32 for s in sizes)
    if ptiles <= MFMA_NT[-1]:
        NT = min(k for k in MFMA_NT if ptiles <= k)
        dc = 128 if D >= 128 else 64
        ndc = D // dc
        n_split = min(max(512 // ndc, 1), max(cdiv(n_rows, SC_ROWS), 1))
        rps = cdiv(cdiv(n_rows, n_split), SC_ROWS) * SC_ROWS
        n_split = max(cdiv(n_rows, rps), 1)
        return ScatterPlan("mfma", f"k_scatter_mfma<{NT}, {dc // 32}, {tf(has_rowscale)}>", (n_split, ndc, 1), 256, True,
                           (NT, dc // 32, bool(has_rowscale)), n_split, NT * 32, n_split * NT * 32 * D * 4 + 256, None, None)
    # zero + global float atomics (launched without the probe hook)
    return ScatterPlan("atomic", f"k_scatter_atomic<{D // 64}>", (cdiv(n_rows, 4), 1, 1), 256, False, None, 0, 0, 256, None, None)


def mfma_rows_per_split(plan, n_rows):
    return cdiv(cdiv(n_rows, plan.n_slabs), SC_ROWS) * SC_ROWS


# ------------------------------------------------------------------------------------------ the cases of the GPU file
# Each row: (sizes, flags, D, n_rows, what it is for).  `what` maps a field of the restated plan -- path, U, FT, gy, dc, NT,
# KT, R, waves, inst, units (the gather's (ks0, nks) list or the scatter's tile counts) -- or one of the derived keys
# below to the value the row promises; tests/test_agg_plan_cpu.py asserts every entry.  Keys that are INPUTS of the case:
#   rs     (scatter) every relation carries a rowscale -- the backward use; default False
#   cycle  (multigraph rows) the degree cycle of the graph; default DEGREE_CYCLE
#   steady (gather) n_rows is not in the table: the GPU test takes it from the probe (steady_n) -- the row carries 0
EICU = (50, 114, 100)
S1, S2, S3, S4 = (SIMPLE,), (SIMPLE,) * 2, (SIMPLE,) * 3, (SIMPLE,) * 4
M1, M2, M3 = (MULTI,), (MULTI,) * 2, (MULTI,) * 3
DS = (64, 128, 256)


# feature tiles per workgroup of k_gather_units, by unit count, at D = 64 / 128 / 256 (two waves per SIMD: FT * U <= 8)
FT_OF = {1: (2, 4, 4), 2: (2, 4, 4), 3: (2, 2, 2), 4: (2, 2, 2), 5: (1, 1, 1), 6: (1, 1, 1)}


def _gather_cases():
    rows = []
    # ---- simple relations: the unit-per-wave kernel, one layout per plan shape
    unit_layouts = [
        ((20,), [(0, 2)]), ((100,), [(0, 8)]),                              # U = 1: no LDS exchange
        ((130,), [(0, 6), (6, 4)]),                                        # nk = 10 -> 6 + 4
        ((114, 50, 100), [(0, 8), (0, 4), (0, 8)]),                        # eICU's sizes in another order
        ((64, 128), [(0, 4), (0, 8)]),                                     # exact fit
        ((20, 30, 40, 50), [(0, 2), (0, 2), (0, 4), (0, 4)]),              # four relations
        ((300, 90), [(0, 8), (8, 6), (14, 6), (0, 6)]),                    # nk = 20 -> 8 + 6 + 6
        ((50, 200, 200), [(0, 4), (0, 8), (8, 6), (0, 8), (8, 6)]),        # U = 5
        ((256, 256, 256), [(0, 8), (8, 8)] * 3),                           # U = 6, 768 padded items: the masks_fit limit
    ]
    for sizes, ks in unit_layouts:
        for D in DS:
            for n in (32, 63, 65, 1834):
                U = len(ks)
                FT = FT_OF[U][DS.index(D)]
                rows.append((sizes, (SIMPLE,) * len(sizes), D, n,
                             dict(path="units", U=U, FT=FT, gy=(D // 32) // FT, waves=U * FT, units=ks)))
    # ---- the bit-plane instances at their vocabulary edges; at D = 64 the same layouts are unit layouts
    for sizes in ((33, 97, 97), (64, 128, 128), (33,), (64,)):
        for D in DS:
            for n in (32, 33, 1000):
                path = "units" if D == 64 else ("bits3" if len(sizes) == 3 else "bits1")
                rows.append((sizes, (SIMPLE,) * len(sizes), D, n, dict(path=path)))
    # ---- fall-throughs of simple layouts
    for D in DS:
        rows.append((EICU, S3, D, 31, dict(path="plain")))                                  # under one tile
        rows.append(((270, 270, 40), S3, D, 300, dict(path="lds", dc=64, gather_units=7)))   # 7 units, 580 columns
        rows.append(((300, 300, 100), S3, D, 300, dict(path="plain", gather_units=7)))       # 7 units, 700 columns
        rows.append((EICU, (SIMPLE, NO_MASK_R, SIMPLE), D, 300, dict(path="lds")))           # no row-major planes
    # ---- past the look-ahead of k_gather_units: n_rows from the probe
    rows.append(((50, 200, 200), S3, 128, 0, dict(path="units", U=5, FT=1, steady=True)))
    rows.append(((130,), S1, 256, 0, dict(path="units", U=2, FT=4, steady=True)))
    # ---- multigraph relations: k_gather_lds at small n, on both sides of 63 | 64
    for sizes, fl in ((EICU, M3), ((20,), M1)):
        for D in DS:
            rows.append((sizes, fl, D, 63, dict(path="plain")))
            for n in (64, 65):
                rows.append((sizes, fl, D, n, dict(path="lds", dc=min(D, 128), max_rows_per_wave=1)))
    # ---- k_gather_lds, pipeline depth: every wave takes >= 4 rows, ragged blocks
    rows.append((EICU, M3, 128, 16400, dict(path="lds", dc=128, gy=1, deep=True, cycle=LIGHT_CYCLE)))
    rows.append((EICU, M3, 256, 8200, dict(path="lds", dc=128, gy=2, deep=True, cycle=LIGHT_CYCLE)))
    rows.append((EICU, M3, 64, 16400, dict(path="lds", dc=64, gy=1, deep=True, cycle=LIGHT_CYCLE)))
    # ---- k_gather_lds with dc = 64 under D >= 128 (300 < columns <= 600), and its two edges
    for D in (128, 256):
        rows.append(((200, 200, 100), M3, D, 200, dict(path="lds", dc=64, gy=D // 64)))
        rows.append(((150, 150), M2, D, 200, dict(path="lds", dc=128)))
        rows.append(((151, 150), M2, D, 200, dict(path="lds", dc=64)))
        rows.append(((300, 300), M2, D, 200, dict(path="lds", dc=64)))
        rows.append(((301, 300), M2, D, 200, dict(path="plain")))
    # ---- k_gather: fewer than 64 rows, more than 600 columns
    for D in DS:
        for n in (1, 5, 63):
            rows.append(((40, 30), M2, D, n, dict(path="plain")))
        rows.append(((700,), M1, D, 300, dict(path="plain")))
    # ---- mixed: one multigraph relation among simple ones
    for D in DS:
        rows.append((EICU, (SIMPLE, MULTI, SIMPLE), D, 300, dict(path="lds")))
    return rows


def _scatter_cases():
    rows = []
    # ---- multigraph relations: every NT instance, KT = 2 and 4, with and without rowscale, ragged last split
    for sizes, NT in (((20,), 2), ((40, 50), 4), ((100, 50), 6), ((100, 100), 8), ((128, 128, 128), 12),
                      ((150, 100, 100), 16), ((512,), 16)):
        for D in DS:
            for rs in (False, True):
                for n in (1, 33, 100, 1834):
                    rows.append((sizes, (MULTI,) * len(sizes), D, n,
                                 dict(path="mfma", NT=NT, KT=2 if D == 64 else 4, rs=rs)))
    for D in DS:
        for rs in (False, True):
            for n in (1, 33, 100, 1834):
                rows.append(((513,), M1, D, n, dict(path="atomic", rs=rs)))
    # ---- mixed and small
    for D in DS:
        for rs in (False, True):
            rows.append((EICU, (SIMPLE, MULTI, SIMPLE), D, 300, dict(path="mfma", NT=10, rs=rs)))
        rows.append((EICU, S3, D, 63, dict(path="mfma", NT=10)))
        rows.append((EICU, S3, D, 64, dict(path="strip", inst=(5, 4))))
    # ---- the unit-per-wave kernel
    for D in DS:
        for n in (64, 65, 1834):
            rows.append(((20,), S1, D, n, dict(path="units", U=1, R=4, waves=4, units=[1], rs=True)))
            rows.append(((200,), S1, D, n, dict(path="units", U=2, R=4, waves=8, units=[4, 3], rs=True)))
            rows.append(((50, 200, 200), S3, D, n, dict(path="units", U=5, R=2, waves=10, units=[2, 4, 3, 4, 3], rs=True)))
            rows.append(((256, 256, 256), S3, D, n, dict(path="units", U=6, R=2, waves=12, units=[4] * 6, rs=True)))
            rows.append(((152, 100, 100), S3, D, n, dict(path="strip", inst=(6, 5), items=352)))
            rows.append(((153, 100, 100), S3, D, n, dict(path="units", U=4, R=3, waves=12, units=[3, 2, 4, 4], items=353)))
            for rs in (False, True):
                rows.append(((270, 270, 40), S3, D, n, dict(path="atomic", scatter_units=7, tiles=20, rs=rs)))
    return rows


def case_id(row):
    sizes, flags, D, n, what = row
    return f"{'-'.join(map(str, sizes))}/{''.join('msn'[f] for f in flags)}/D{D}/n{n}" + ("/rs" if what.get("rs") else "")


GATHER_CASES = _gather_cases()
SCATTER_CASES = _scatter_cases()
