"""The f16 forward scatter (k_scatter_strip2 / strip_main_h) INSIDE one wave's row range, where its scale moves.

A wave of the strip kernel streams a range of 64-row stages of one 32-column strip and picks the power of two e of its two
f16 pieces x * 2^e from the 16-row blocks it has seen (H2Scale, csrc/mma.h; restated in tests/h2_ref.py).  The shapes of
tests/test_ops_gpu.py give a wave one stage.  Here every wave gets at least 6 stages = 24 blocks, and the data are shaped
PER BLOCK POSITION j of a wave -- the same profile in every wave:

  x[r, :] = randn * 2^p(j),  j = the block of row r inside its wave's range

and row r has an edge to "position item" j of every relation (plus one random edge to an item behind the position items),
so position item j sums the terms of block j of every wave and its own magnitude is that of position j alone.  Relations are
simple, with bit planes; the vocabularies reach the <6, 5> and the <4, 4> instance, with tiles that straddle two relations.

The launch is never assumed: n_q = 4 * gridDim.x comes from the probe (ops.probe_grids), the stage range of wave q is
[q * nst / n_q, (q + 1) * nst / n_q) as in strip_main_h, n_rows = 64 * 6 * n_q, and every case asserts from the probe of its
OWN launch that k_scatter_strip2 ran on that grid.  A case that lands in another kernel or gets fewer stages fails.

Bars, per output element, against an fp64 index_add_ of the same fp32 x (mag = the sum of |terms| of the same element):
  in-window profiles      |err| <= 6e-7 mag                 (the bar of test_scatter_f16_pieces_follow_the_data_range and its
                          derivation: 2^-22 = 2.4e-7 per term from the two f16 pieces, a few 6e-8 from fp32 accumulation);
                          finite; exactly 0 where mag == 0
  below-window profiles   |err| <= 6e-7 mag + sum over the element's terms of 2^-25 * 2^-e
                          (the absolute floor of a term split at exponent e; e per block and wave
                          strip from tests/h2_ref.py -- walk() fed the block maxima of x, floor_exponents(): the e a block is
                          split at, or that of a later re-anchor of the same wave if lower, see there.  Nothing is measured
                          for this bar.)
  the exact kernel        the same x with rowscale = 1 runs k_scatter_units<true> (three exact bf16 pieces): 6e-7 mag on
                          EVERY profile -- the loss below the window belongs to the shared scale, not to the reference
  paths                   h2_ref.walk() must report the path a profile is named for in every wave strip
  reproducibility         two launches agree bit for bit

Measured on an MI355X (worst |err| / mag: strip kernel | exact kernel; D = 256, <6, 5>, probed grid (32, 8) -> n_q = 128,
49,152 rows; paths over the 1,024 wave strips as first / lower / outlier / re-anchor):
  flat      6.3e-8 | 6.3e-8   1024/0/0/0          step95    7.5e-8 | 7.5e-8   1024/0/0/1024
  rise9     9.6e-8 | 9.1e-8   1024/3043/0/0       zero_head 7.5e-8 | 7.5e-8   1024/0/0/0
  fall14    1.2e-7 | 9.8e-8   1024/0/0/0          cols14    6.6e-8 | 6.3e-8   1024/0/0/0
  step12    6.2e-8 | 5.8e-8   1024/0/16384/0      fall23    7.1e-6 | 1.5e-7   1024/0/0/0
  step30    7.5e-8 | 7.5e-8   1024/0/16384/0      fall46    9.0e-2 | 1.8e-7   1024/0/0/0
  spike     1.5e-7 | 1.5e-7   1024/0/1024/0       cols20    3.0e-6 | 6.3e-8   1024/0/0/0
  step140   1.5e+3 | 7.5e-8   1024/0/0/1024   (the items before the step: a re-anchor multiplies the accumulators by
            2^max(d, -126), so a sum 2^140 below the new scale comes out 2^14 too large -- far inside the floor, and
            documented as unspecified in csrc/mma.h and include/mmgnn.h)
D = 128 runs <4, 4> on the probed grid (64, 4): 98,304 rows.  Every case takes well under a second.
"""
import re

import numpy as np
import pytest
import torch

import h2_ref as H

pytestmark = pytest.mark.gpu

STAGES = 6                      # stages of 64 rows per wave: 24 blocks
NPOS = 32                       # position items per relation (24 used; a ragged range has one stage more: 28)
BAR = 6e-7
VOCAB = {"<6, 5>": [50, 200, 100], "<4, 4>": [50, 114, 60]}      # 350 items = 11 tiles, 224 items = 7 tiles (-> 8)
REPORT = {}                     # (D, instance, profile) -> figures (printed by the last test of the module)


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


# ------------------------------------------------------------------------------------------ profiles: p(j), column factors
def _steps(lo, hi):
    return lambda j: torch.where(j < 8, float(lo), float(hi))


PROFILES = {       # name -> (exponent of the row multiplier at block position j | None: rows of zeros, column exponents, path)
    "flat": (lambda j: 0.0 * j, None, "first"),
    "rise9": (lambda j: 0.4 * j, None, "lower"),
    "fall14": (lambda j: -0.6 * j, None, "first"),
    "step12": (_steps(0, 12), None, "outlier"),
    "step30": (_steps(0, 30), None, "outlier"),
    "spike": (lambda j: torch.where(j == 8, 60.0, 0.0), None, "outlier"),
    "step95": (_steps(-40, 55), None, "reanchor"),
    "zero_head": (lambda j: torch.where(j < 8, float("-inf"), -40.0), None, "first"),
    "cols14": (lambda j: 0.0 * j, -14.0, "first"),
    "fall23": (lambda j: -1.0 * j, None, "first"),
    "fall46": (lambda j: -2.0 * j, None, "first"),
    "cols20": (lambda j: 0.0 * j, -20.0, "first"),
    "step140": (_steps(-80, 60), None, "reanchor"),
}
IN_WINDOW = ["flat", "rise9", "fall14", "step12", "step30", "spike", "step95", "zero_head", "cols14"]
BELOW_WINDOW = ["fall23", "fall46", "cols20", "step140"]
SHORT = ["rise9", "step30", "step95", "fall23"]


# ------------------------------------------------------------------------------------------ the launch, from the probe
def probed_scatter(ops, rels, n_rows, D, x):
    """scatter_rows under an armed probe -> (kernel symbol, grid xyz) of its scatter launch."""
    ops.probe_arm(8)
    ops.scatter_rows(rels, n_rows, D, x)
    torch.cuda.synchronize()
    rows, grids = ops.probe_read(), ops.probe_grids()
    ops.probe_arm(0)
    assert len(rows) == len(grids)
    hit = [(r[6], g) for r, (g, _) in zip(rows, grids) if r[1] == "scatter_rows"]
    assert len(hit) == 1, f"expected one scatter launch, the probe saw {[r[6] for r in rows]}"
    return hit[0]


def wave_ranges(n_rows, n_q):
    """-> (first stage of every wave quarter and the end: int64 [n_q + 1], stage count nst), as strip_main_h divides them."""
    nst = (n_rows + 63) // 64
    return (torch.arange(n_q + 1, dtype=torch.int64) * nst) // n_q, nst


class Problem:
    """Graph, CSR, bit planes and the block geometry of one (n_rows, n_q, vocabulary, D)."""

    def __init__(self, ops, dev, n_rows, n_q, sizes, D):
        self.n_rows, self.n_q, self.D, self.sizes = n_rows, n_q, D, sizes
        s_beg, nst = wave_ranges(n_rows, n_q)
        self.s_beg, self.nst = s_beg, nst
        r = torch.arange(n_rows, dtype=torch.int64)
        q = torch.searchsorted(s_beg, r // 64, right=True) - 1                  # the wave quarter that streams row r
        self.j = (r - 64 * s_beg[q]) // 16                                      # its block position inside that range
        assert int(self.j.max()) < NPOS
        gen = torch.Generator().manual_seed(n_rows + 7 * D + sum(sizes))
        self.rels, self.eis = [], []
        for nc in sizes:
            other = NPOS + torch.randint(0, nc - NPOS, (n_rows,), generator=gen)
            ei = torch.stack([torch.cat([r, r]), torch.cat([self.j, other])])
            ei = ei[:, torch.randperm(ei.shape[1], generator=gen)].contiguous()
            rp, col, _ = ops.csr_build(ei.to(dev), n_rows, 0)
            mask, _ = ops.rel_mask_build(rp, col, nc)
            self.rels.append(ops.Rel(rp, col, nc, out=torch.full((nc, D), 5.0, device=dev), simple=True, mask_t=mask))
            # edges in CSR order (what the kernel's sums are compared with), kept on the device for the fp64 reference
            self.eis.append((torch.repeat_interleave(torch.arange(n_rows, device=dev), (rp[1:] - rp[:-1]).long()), col.long()))
        self.ones = torch.ones(n_rows, device=dev)
        self.base = torch.randn(n_rows, D, generator=gen).to(dev)
        self.j_dev = self.j.to(dev)

    def x_of(self, name):
        p_of_j, col_exp, _ = PROFILES[name]
        mult = torch.exp2(p_of_j(self.j_dev.double())).float()                  # (2^-inf = 0: the all-zero blocks)
        x = self.base * mult[:, None]
        if col_exp is not None:                                                 # odd columns of every strip 2^col_exp below
            cm = torch.where(torch.arange(self.D, device=x.device) % 2 == 1, 2.0 ** col_exp, 1.0).float()
            x = x * cm[None, :]
        return x.contiguous()

    def trajectories(self, x):
        """-> per wave quarter q and strip: (e, path) per block from tests/h2_ref.py fed the block maxima of x, as arrays
        [n_blocks_total, strips] in global block order (a wave's blocks are consecutive 16-row blocks), plus the floor
        exponents."""
        strips, nblk = self.D // 32, self.nst * 4
        a = x.abs()
        fin = torch.where(torch.isfinite(a), a, torch.zeros_like(a))
        pad = nblk * 16 - self.n_rows
        if pad:
            fin = torch.cat([fin, fin.new_zeros(pad, self.D)])
            a = torch.cat([a, a.new_zeros(pad, self.D)])
        bm = fin.view(nblk, 16, strips, 32).amax((1, 3)).cpu().numpy()
        inf = torch.isinf(a).view(nblk, 16, strips, 32).any(3).any(1).cpu().numpy()
        es = np.zeros((nblk, strips), np.int64)
        paths, fl = np.zeros_like(es), np.zeros_like(es)
        for q in range(self.n_q):
            b0, b1 = 4 * int(self.s_beg[q]), 4 * int(self.s_beg[q + 1])
            for s in range(strips):
                e, p, _ = H.walk(bm[b0:b1, s], inf[b0:b1, s])
                es[b0:b1, s], paths[b0:b1, s], fl[b0:b1, s] = e, p, H.floor_exponents(e, p)
        return es, paths, fl

    def reference(self, x, fl=None):
        """-> per relation (ref, mag, floor) in fp64 on the device: index_add_ over the CSR-ordered edges of x, of |x|, and
        (fl given) of the per-term floor 2^-25 * 2^-e of the row's block and strip."""
        xd = x.double()
        out = []
        fl_rows = None
        if fl is not None:
            per_blk = torch.from_numpy(np.ldexp(1.0, -25 - fl)).to(x.device)                      # [n_blocks, strips]
            fl_rows = per_blk[torch.arange(self.n_rows, device=x.device) // 16].repeat_interleave(32, dim=1)
        for (row, col), rel in zip(self.eis, self.rels):
            z = torch.zeros(rel.n_cols, self.D, dtype=torch.float64, device=x.device)
            ref = z.clone().index_add_(0, col, xd[row])
            mag = z.clone().index_add_(0, col, xd[row].abs())
            floor = z.clone().index_add_(0, col, fl_rows[row]) if fl is not None else z
            out.append((ref, mag, floor))
        return out

    def launch(self, ops, x, exact=False):
        """-> (outputs, kernel symbol, grid).  exact: rowscale = 1 on every relation -> the three-piece kernel."""
        for r in self.rels:
            r.rowscale = self.ones if exact else None
            r.out.fill_(5.0)
        sym, grid = probed_scatter(ops, self.rels, self.n_rows, self.D, x)
        for r in self.rels:
            r.rowscale = None
        return [r.out.clone() for r in self.rels], sym, grid


_PROBLEMS = {}


def problem(ops, dev, inst, D, extra_rows=0):
    """The smallest n_rows that gives every wave STAGES stages: n_q from the probe of a launch at the size the rule gives for
    the n_q seen so far, until a launch at n_rows has that n_q."""
    key = (inst, D, extra_rows)
    if key not in _PROBLEMS:
        n_q, pb = 64, None
        for _ in range(6):
            n_rows = 64 * STAGES * n_q + extra_rows
            pb = Problem(ops, dev, n_rows, n_q, VOCAB[inst], D)
            sym, grid = probed_scatter(ops, pb.rels, n_rows, D, pb.base)
            assert sym.startswith("k_scatter_strip2<"), sym
            if 4 * grid[0] == n_q:
                break
            n_q = 4 * grid[0]
        else:
            raise AssertionError("the grid of k_scatter_strip2 did not settle")
        _PROBLEMS[key] = pb
    return _PROBLEMS[key]


def worst(got, ref, mag, floor=None):
    """-> (worst |err| / mag over mag > 0, number of elements over the bar)."""
    err = (got.double() - ref).abs()
    bound = BAR * mag + (floor if floor is not None else 0.0)
    pos = mag > 0
    w = float((err[pos] / mag[pos]).max()) if bool(pos.any()) else 0.0
    return w, int((~(err <= bound)).sum())


def run_case(ops, dev, inst, D, name, extra_rows=0):
    pb = problem(ops, dev, inst, D, extra_rows)
    x = pb.x_of(name)
    assert bool(torch.isfinite(x).all())
    below = name in BELOW_WINDOW
    # the launch of THIS case: the kernel, its grid, the stages every wave got
    outs, sym, grid = pb.launch(ops, x)
    m = re.match(r"k_scatter_strip2<(\d+), ?(\d+)>$", sym)
    assert m, sym
    assert f"<{m.group(1)}, {m.group(2)}>" == inst, (sym, inst)
    assert grid[1] == D // 32 and 4 * grid[0] == pb.n_q, (grid, pb.n_q)
    per_wave = (pb.s_beg[1:] - pb.s_beg[:-1])
    assert int(per_wave.min()) >= STAGES, per_wave.min()
    # paths, from the restated rule fed the block maxima of x
    es, paths, fl = pb.trajectories(x)
    want = getattr(H, PROFILES[name][2].upper())
    counts = np.zeros(5, np.int64)
    for q in range(pb.n_q):
        b0, b1 = 4 * int(pb.s_beg[q]), 4 * int(pb.s_beg[q + 1])
        for s in range(D // 32):
            took = paths[b0:b1, s]
            assert (took == H.FIRST).sum() == 1 and (took == want).any(), (name, q, s, took)
            if name == "zero_head":
                assert took[8] == H.FIRST, (q, s, took)
            counts += np.bincount(took, minlength=5)
    # the strip kernel against the fp64 sums
    refs = pb.reference(x, fl if below else None)
    w_strip, w_exact = 0.0, 0.0
    for k, (got, (ref, mag, floor)) in enumerate(zip(outs, refs)):
        assert bool(torch.isfinite(got).all()), (name, k)
        assert bool((got[mag == 0] == 0).all()), (name, k)
        w, bad = worst(got, ref, mag, floor if below else None)
        print(f"{name} D={D} {inst} relation {k}: strip kernel worst |err|/mag {w:.3e}, over the bar {bad}")
        w_strip = max(w_strip, w)
        if bad:
            err = (got.double() - ref).abs()
            over = err - (BAR * mag + (floor if below else 0.0))
            item, c = divmod(int(over.argmax()), D)
            raise AssertionError(f"{name}: relation {k} item {item} column {c} (strip {c // 32}; an item below {NPOS} collects "
                                 f"the block of that number of every wave): |err| {float(err[item, c]):.3e}, mag "
                                 f"{float(mag[item, c]):.3e}, worst |err|/mag {w:.3e}, {bad} elements over the bar")
    # bit-reproducible
    again, _, _ = pb.launch(ops, x)
    for a, b in zip(outs, again):
        assert torch.equal(a, b), name
    # the exact kernel on the same x: the plain bar on every profile
    outs_x, sym_x, _ = pb.launch(ops, x, exact=True)
    assert sym_x == "k_scatter_units<true>", sym_x
    for k, (got, (ref, mag, _)) in enumerate(zip(outs_x, refs)):
        assert bool(torch.isfinite(got).all()), (name, k)
        w, bad = worst(got, ref, mag)
        print(f"{name} D={D} {inst} relation {k}: exact kernel worst |err|/mag {w:.3e}, over the bar {bad}")
        w_exact = max(w_exact, w)
        assert bad == 0 and w <= BAR, (name, k, w, bad)
    REPORT[(D, inst, name, extra_rows)] = (w_strip, w_exact, counts.tolist(), grid, pb.n_rows)
    if not below:
        assert w_strip <= BAR, (name, w_strip)


@pytest.mark.parametrize("name", IN_WINDOW + BELOW_WINDOW)
def test_scale_profiles_d256_instance_6_5(ops, dev, name):
    run_case(ops, dev, "<6, 5>", 256, name)


@pytest.mark.parametrize("name", SHORT)
def test_scale_profiles_d256_instance_4_4(ops, dev, name):
    run_case(ops, dev, "<4, 4>", 256, name)


@pytest.mark.parametrize("name", SHORT)
def test_scale_profiles_d128_instance_4_4(ops, dev, name):
    run_case(ops, dev, "<4, 4>", 128, name)


@pytest.mark.parametrize("name", ["rise9", "fall23"])
def test_scale_profiles_ragged_ranges(ops, dev, name):
    """n_rows + 37: the last stage holds 37 rows and n_q does not divide the stage count -- one wave gets 7 stages."""
    pb = problem(ops, dev, "<6, 5>", 256, extra_rows=37)
    assert pb.nst % pb.n_q != 0 and pb.n_rows % 64 == 37
    per_wave = pb.s_beg[1:] - pb.s_beg[:-1]
    assert int(per_wave.min()) == STAGES and int(per_wave.max()) == STAGES + 1
    run_case(ops, dev, "<6, 5>", 256, name, extra_rows=37)


def test_nonfinite_values_stay_in_their_column_on_every_path(ops, dev):
    """An infinity, and separately a NaN, in column 17 of a row of a wave's FIRST block, of a block that LOWERS e and of an
    OUTLIER block: the sums of that row's items in column 17 are non-finite, every other column is bitwise what it is
    without it (a non-finite value takes part in no scale decision: tests/h2_ref.py gives the same trajectory with it)."""
    D, inst = 256, "<6, 5>"
    pb = problem(ops, dev, inst, D)
    # one profile with all three: rising 2^0.4 per block (lowers e), one block 2^40 above at position 16 (outlier)
    j = pb.j_dev.double()
    x = (pb.base * torch.exp2(0.4 * j + torch.where(j == 16, 40.0, 0.0)).float()[:, None]).contiguous()
    clean, sym, _ = pb.launch(ops, x)
    assert sym.startswith("k_scatter_strip2<"), sym
    es, paths, _ = pb.trajectories(x)
    q = pb.n_q // 2 + 1                                        # a wave in the middle; column 17 lies in strip 0
    b0, b1 = 4 * int(pb.s_beg[q]), 4 * int(pb.s_beg[q + 1])
    took = paths[b0:b1, 0]
    assert took[0] == H.FIRST and took[16] == H.OUTLIER and (took == H.LOWER).any(), took
    spots = {"first": b0, "lower": b0 + int(np.nonzero(took == H.LOWER)[0][0]), "outlier": b0 + 16}
    keep = torch.ones(D, dtype=torch.bool, device=dev)
    keep[17] = False
    for where, blk in spots.items():
        rows = torch.arange(16 * blk, 16 * blk + 16, device=dev)
        row = int(rows[x[rows, 17].abs().argmin()])            # (not the block's maximum: the finite maxima stay what they were)
        for bad in (float("inf"), float("nan")):
            xb = x.clone()
            xb[row, 17] = bad
            es_b, paths_b, _ = pb.trajectories(xb)
            assert np.array_equal(es_b, es) and np.array_equal(paths_b, paths), (where, bad)
            got, sym_b, _ = pb.launch(ops, xb)
            assert sym_b == sym
            for g, c, (erow, ecol) in zip(got, clean, pb.eis):
                hit = ecol[erow == row]
                assert hit.numel() == 2
                assert not bool(torch.isfinite(g[hit, 17]).any()), (where, bad)
                assert torch.equal(g[:, keep], c[:, keep]), (where, bad)


def test_report():
    """The figures of this run (pytest -rP shows them): per case the worst |err| / mag of the strip kernel and of the exact
    kernel, the path counts over all wave strips (nothing, first, lower, outlier, re-anchor) and the probed grid."""
    for (D, inst, name, extra), (ws, wx, counts, grid, n_rows) in sorted(REPORT.items()):
        print(f"D={D} {inst} n_rows={n_rows} grid={grid} {name:10s} strip {ws:.3e}  exact {wx:.3e}  paths {counts}")
