"""The sparse aggregates at the layouts and sizes where their launch plan switches.

mmg_gather_rows and mmg_scatter_rows (csrc/aggregate.hip) choose on the host between five gather and five scatter kernels.
The shapes here come ONLY from the tables of tests/agg_plan_ref.py, the plain-Python restatement of that plan
(tests/test_agg_plan_cpu.py holds it against the library and asserts what every row is for).  EVERY case asserts from the
probe of its own launch that the restated symbol, grid and block ran; k_gather and k_scatter_atomic are launched without
the probe hook, and for them the probe must have seen no gather / scatter kernel record.

Graphs: simple relations have no repeated (row, column) pair, ragged degrees and every seventh row empty; multigraph
relations have a prescribed degree per row (agg_plan_ref.DEGREE_CYCLE in turn, shifted per relation: empty rows, rows on
both sides of the 64-edge reload of the gathers, rows of 129 and 200 edges) and columns drawn with replacement.  Every
relation carries a random rowscale and colscale (the scatter: colscale always, rowscale where the row says so).

References are fp64 on the host, built from the edge list in row blocks.  Bars, as max|err| / max|ref| per output tensor,
are the ones the project already holds these kernels to: 1e-6 where every relation is simple, 1e-5 with a multigraph
relation and for the atomic fallback, 1e-6 for the epilogue statistics against fp64 sums of the device output.  Every
launch but the atomic scatter's runs twice and must give the same bits.

Measured worst error per kernel family (MI355X, these tables and seeds):
  gather  k_gather_bits<20, 4, 12> 2.1e-07 (statistics 9.4e-08)   k_gather_bits<4, 4, 4> 1.9e-07 (1.0e-07)
          k_gather_units 2.6e-07 (1.7e-07)   k_gather_lds simple 2.1e-07, multigraph 4.2e-07
          k_gather simple 2.1e-07, multigraph 6.6e-07
  scatter k_scatter_strip2 1.8e-07   k_scatter_units 2.4e-07 with and without rowscale
          k_scatter_mfma 2.3e-07 with and without rowscale   k_scatter_atomic 7.9e-07
"""
import functools

import pytest
import torch

import agg_plan_ref as A
from agg_plan_ref import MULTI, SIMPLE
from test_steady_state_gpu import _randn, launch_of, probed, regime, steady_n

pytestmark = pytest.mark.gpu

WORST = {}
ROW_BLOCK = 4096


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    import mmgnn  # noqa: F401
    from mmgnn import ops as o
    return o


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    assert bool(torch.isfinite(a).all())
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def note(family, err, bar):
    WORST[family] = max(WORST.get(family, 0.0), err)
    print(f"[agg] {family}: {err:.3e} (bar {bar:.0e})")


def bar_of(flags, path):
    return 1e-6 if MULTI not in flags and path != "atomic" else 1e-5


def ran_as_planned(recs, plan, n, prefix):
    """The one launch of the family in the probe records IS the restated plan's; the two kernels launched without the probe
    hook leave no record of the family."""
    seen = [r for r in recs if prefix in r[0]]
    if not plan.probed:
        assert not seen, f"plan: {plan.symbol} (no probe record); the probe saw {[r[0] for r in seen]}"
        return
    sym, m, grid, block = launch_of(recs, prefix)
    assert (sym, m, grid, block) == (plan.symbol, n, plan.grid, plan.block), \
        f"probe: {sym} M = {m} grid {grid} block {block}; plan: {plan.symbol} grid {plan.grid} block {plan.block}"
    print(f"[agg] {sym} grid {grid} block {block}")


# ------------------------------------------------------------------------------------------ graphs and references
SIMPLE_MAX_DEG = (50, 9, 25, 12)


class Graph:
    """One relation list on the host (CSR, fp64 scales) and on the device."""

    def __init__(self, ops, dev, n_rows, sizes, flags, cycle, cap):
        gen = torch.Generator().manual_seed(7 * n_rows + 13 * sum(sizes) + len(sizes) + sum(flags))
        self.n, self.sizes, self.flags, self.rels = n_rows, sizes, flags, []
        for r, (nc, fl) in enumerate(zip(sizes, flags)):
            if fl == MULTI:
                deg = torch.tensor([cycle[(i + 5 * r + 3) % len(cycle)] for i in range(n_rows)])
                if cap:
                    deg = deg.clamp(max=2 * nc)
                col = torch.randint(0, nc, (int(deg.sum()),), generator=gen)
            else:
                order = torch.rand(n_rows, nc, generator=gen).argsort(1)
                deg = torch.randint(0, min(SIMPLE_MAX_DEG[r], nc) + 1, (n_rows,), generator=gen)
                deg[::7] = 0
                if n_rows > 1:
                    deg[1] = nc if nc <= 64 else deg[1]            # (a full row of a small vocabulary)
                rr, kk = torch.nonzero(torch.arange(nc)[None, :] < deg[:, None], as_tuple=True)
                col = order[rr, kk]
            rowptr = torch.zeros(n_rows + 1, dtype=torch.long)
            rowptr[1:] = deg.cumsum(0)
            rs, cs = torch.rand(n_rows, generator=gen) + 0.25, torch.rand(nc, generator=gen) + 0.25
            d = dict(rowptr=rowptr, col=col, rs=rs, cs=cs, rp_d=rowptr.int().to(dev), col_d=col.int().to(dev),
                     rs_d=rs.to(dev), cs_d=cs.to(dev), mask_t=None, mask_r=None)
            if fl != MULTI:
                d["mask_t"], d["mask_r"] = ops.rel_mask_build(d["rp_d"], d["col_d"], nc)
            self.rels.append(d)

    def counts(self, r, b0, b1):
        """Rows [b0, b1) of relation r's edge-count matrix, fp64."""
        d, nc = self.rels[r], self.sizes[r]
        e0, e1 = int(d["rowptr"][b0]), int(d["rowptr"][b1])
        rows = torch.repeat_interleave(torch.arange(b1 - b0), d["rowptr"][b0 + 1:b1 + 1] - d["rowptr"][b0:b1])
        cnt = torch.zeros((b1 - b0) * nc, dtype=torch.float64)
        cnt.index_add_(0, rows * nc + d["col"][e0:e1], torch.ones(e1 - e0, dtype=torch.float64))
        return cnt.view(b1 - b0, nc)


@functools.lru_cache(maxsize=12)
def graph(ops, dev, n_rows, sizes, flags, cycle=A.DEGREE_CYCLE, cap=False):
    return Graph(ops, dev, n_rows, sizes, flags, cycle, cap)


def table(r, nc):
    return _randn(1000 + 10 * r + nc, nc, 256) * 2


@functools.lru_cache(maxsize=12)
def gather_ref(g):
    """[n_rows, 256] fp64: sum_r rowscale_r * (counts_r @ (colscale_r * table_r)); a case of width D takes columns [0, D)."""
    ref = torch.zeros(g.n, 256, dtype=torch.float64)
    for r, (d, nc) in enumerate(zip(g.rels, g.sizes)):
        src = table(r, nc).double() * d["cs"].double()[:, None]
        for b0 in range(0, g.n, ROW_BLOCK):
            b1 = min(g.n, b0 + ROW_BLOCK)
            ref[b0:b1] += (g.counts(r, b0, b1) @ src) * d["rs"][b0:b1].double()[:, None]
    return ref


@functools.lru_cache(maxsize=12)
def scatter_ref(g, with_rs):
    """Per relation [n_cols, 256] fp64: colscale_r * (counts_r^T @ (rowscale_r * x))."""
    x = _randn(77, g.n, 256).double() * 2 - 0.4
    out = []
    for r, (d, nc) in enumerate(zip(g.rels, g.sizes)):
        acc = torch.zeros(nc, 256, dtype=torch.float64)
        for b0 in range(0, g.n, ROW_BLOCK):
            b1 = min(g.n, b0 + ROW_BLOCK)
            xb = x[b0:b1] * d["rs"][b0:b1].double()[:, None] if with_rs else x[b0:b1]
            acc += g.counts(r, b0, b1).t() @ xb
        out.append(acc * d["cs"].double()[:, None])
    return out


def the_graph(ops, dev, row, n=None, cap=False):
    sizes, flags, _, n_rows, what = row
    return graph(ops, dev, n_rows if n is None else n, sizes, flags, what.get("cycle", A.DEGREE_CYCLE), cap)


# ------------------------------------------------------------------------------------------ mmg_gather_rows
def gather_rels(ops, dev, g, D):
    return [ops.Rel(d["rp_d"], d["col_d"], nc, rowscale=d["rs_d"], colscale=d["cs_d"],
                    table=table(r, nc)[:, :D].contiguous().to(dev), simple=fl != MULTI,
                    mask_r=d["mask_r"] if fl == SIMPLE else None)
            for r, (d, nc, fl) in enumerate(zip(g.rels, g.sizes, g.flags))]


def run_gather(ops, dev, row, variants, n=None, steady=False):
    sizes, flags, D, n_rows, what = row
    n = n_rows if n is None else n
    g = the_graph(ops, dev, row, n)
    rels = gather_rels(ops, dev, g, D)
    ref = gather_ref(g)[:, :D]
    base = _randn(D + 3, n, D)
    for variant in variants:
        acc, stats = variant == "acc", variant == "stats"
        plan = A.gather_plan(sizes, flags, D, n, accumulate=acc)
        assert plan.path == what["path"]

        def call():
            out = base.to(dev).clone() if acc else torch.full((n, D), 7.0, device=dev)
            return ops.gather_rows(rels, n, D, out, accumulate=acc, with_stats=stats)

        res, recs = probed(ops, call)
        ran_as_planned(recs, plan, n, "k_gather_")
        if steady:
            print("[agg] tiles per workgroup:", regime(recs, plan.symbol, n)[3])
        out, sums = (res[0], res[1]) if stats else (res, None)
        again = call()
        assert torch.equal(out, again[0] if stats else again), f"{plan.symbol}: the same call twice, other bits"
        bar = bar_of(flags, plan.path)
        e = rel(out, ref + base.double() if acc else ref)
        note(f"gather {plan.path}" + (" multigraph" if MULTI in flags else ""), e, bar)
        assert e <= bar, (plan, variant, e)
        if stats:
            od = out.double().cpu()
            e1, e2 = rel(sums[0], od.sum(0)), rel(sums[1], (od * od).sum(0))
            note(f"gather {plan.path} statistics", max(e1, e2), 1e-6)
            assert e1 <= 1e-6 and e2 <= 1e-6, (plan, e1, e2)
            assert torch.equal(sums, again[1]), f"{plan.symbol}: statistics of the same call twice, other bits"


def gather_rows_where(pred):
    return [r for r in A.GATHER_CASES if pred(r)]


@pytest.mark.parametrize("row", gather_rows_where(lambda r: MULTI not in r[1] and not r[4].get("steady")), ids=A.case_id)
def test_gather_of_simple_relations_at_the_plan_switches(ops, dev, row):
    """k_gather_units at one layout per plan shape (1 to 6 units, FT = 1, 2, 4, gy up to 8, chunkings 6 + 4 and 8 + 6 + 6,
    four relations, the 768-item limit), the bit-plane instances at their vocabulary edges, and the fall-throughs to
    k_gather_lds and k_gather: plain, accumulating into a random `out`, and with the epilogue statistics."""
    run_gather(ops, dev, row, ("plain", "acc", "stats"))


@pytest.mark.parametrize("row", gather_rows_where(lambda r: r[4].get("steady")), ids=A.case_id)
def test_gather_units_past_the_look_ahead(ops, dev, row):
    """FT = 1 with five units and FT = 4 with two: n from the probed grid, workgroups walk 3 and 4 tiles -- past the
    GU_DEPTH = 3 register sets of look-ahead."""
    sizes, flags, D, _, what = row

    def big():
        g = graph(ops, dev, 40_000, sizes, flags)
        return ops.gather_rows(gather_rels(ops, dev, g, D), 40_000, D, torch.empty(40_000, D, device=dev), accumulate=False)

    n = steady_n(ops, ("agg gather", sizes, D), "k_gather_units", big)
    p = A.gather_plan(sizes, flags, D, n)
    assert (p.U, p.FT) == (what["U"], what["FT"]) and A.gather_tiles_per_workgroup(p, n) == {3, 4}
    run_gather(ops, dev, row, ("plain", "acc", "stats"), n=n, steady=True)


@pytest.mark.parametrize("row", gather_rows_where(lambda r: MULTI in r[1]), ids=A.case_id)
def test_gather_of_multigraph_relations_at_the_plan_switches(ops, dev, row):
    """k_gather_lds on both sides of 63 | 64 rows, with every wave past its fourth row (the b0 / b1 / b2, c0 / c1 rotation)
    and ragged blocks, with dc = 64 under D >= 128 and at the 300 | 301 and 600 | 601 column edges; k_gather below 64 rows
    and above 600 columns; one multigraph relation among simple ones.  Rows of 65 .. 200 edges take the reload of the
    column ids inside a row.  Plain and accumulating."""
    run_gather(ops, dev, row, ("plain", "acc"))


# ------------------------------------------------------------------------------------------ mmg_scatter_rows
@pytest.mark.parametrize("row", A.SCATTER_CASES, ids=A.case_id)
def test_scatter_at_the_plan_switches(ops, dev, row):
    """k_scatter_mfma at every NT, KT = 2 and 4, with and without a per-relation rowscale (HAS_RS), one split, a ragged last
    split and 58 splits, on both sides of 512 | 513 padded items, mixed with simple relations and below 64 rows;
    k_scatter_units at 1, 2, 4, 5 and 6 units (R = 4, 3, 2; 12 waves); the strip kernel on its side of 352 | 353 items and of
    63 | 64 rows; the atomic fallback."""
    sizes, flags, D, n, what = row
    has_rs = what.get("rs", False)
    plan = A.scatter_plan(sizes, flags, has_rs, D, n)
    assert plan.path == what["path"]
    g = the_graph(ops, dev, row, cap=True)
    refs = scatter_ref(g, has_rs)
    xd = (_randn(77, n, 256) * 2 - 0.4)[:, :D].contiguous().to(dev)
    rels = [ops.Rel(d["rp_d"], d["col_d"], nc, rowscale=d["rs_d"] if has_rs else None, colscale=d["cs_d"],
                    out=torch.full((nc, D), 5.0, device=dev), simple=fl != MULTI, mask_t=d["mask_t"])
            for d, nc, fl in zip(g.rels, sizes, flags)]
    _, recs = probed(ops, lambda: ops.scatter_rows(rels, n, D, xd))
    ran_as_planned(recs, plan, n, "k_scatter_")
    # the slab sum follows every slab kernel and only them
    assert any("reduce_slabs" in r[0] for r in recs) == plan.probed, [r[0] for r in recs]
    first = [r.out.clone() for r in rels]
    bar = bar_of(flags, plan.path)
    for r, ref in zip(rels, refs):
        e = rel(r.out, ref[:, :D])
        note(f"scatter {plan.path}" + (" rowscale" if has_rs else ""), e, bar)
        assert e <= bar, (plan, e)
    if plan.path != "atomic":
        ops.scatter_rows(rels, n, D, xd)
        for r, f in zip(rels, first):
            assert torch.equal(r.out, f), f"{plan.symbol}: the same call twice, other bits"


def test_report():
    for k in sorted(WORST):
        print(f"[agg] worst {k}: {WORST[k]:.3e}")
