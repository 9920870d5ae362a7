"""The bootstrap kernels of libmmgnn_boot.so (csrc/boot.hip) against the loop reference of boot_ref.py and the host
restatement it pins (tests/test_bootstrap_cpu.py): the weights EQUAL, the counts EQUAL, every fp64 sum inside the bound
its exact terms give, the metrics EQUAL metrics_from_sums on the device's own sums, the percentiles EQUAL numpy's -- at
every shape where the kernels take another path -- and the whole is bitwise repeatable, eagerly and from a hipGraph."""
import math

import numpy as np
import pandas as pd
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import boot_ops as bo
from mmgnn import bootstrap as bt
from mmgnn import ops
from mmgnn._lib import MmgError
from mmgnn.evaluate import compute_regression_metrics, metrics_from_sums
from mmgnn.model import build_model
from mmgnn.synth import make_graph
from mmgnn.train import EdgeMasker
import boot_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = np.float32
C, RB = bo.BOOT_CHUNK, bo.BOOT_RB
U = 2.0 ** -53


@pytest.fixture(autouse=True)
def stop_at_a_device_fault():
    """A kernel fault surfaces at the next synchronisation: nothing more is started on the device after one."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device fault, stopping the session: {e}", returncode=3)


def same(got, want):
    got, want = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got), np.asarray(want)
    return got.shape == want.shape and bool(np.array_equal(got, want, equal_nan=got.dtype.kind == "f"))


def bits(t):
    return t.contiguous().view(torch.uint8)


def make_case(n, n_seg, n_units, seed=0, one_unit=False):
    """Random pairs whose segments are skewed (a few large ones that span chunks, many small ones, some empty)."""
    rng = np.random.default_rng(seed)
    t = rng.normal(1.0, 2.0, n).astype(F32)
    t[rng.random(n) < 0.05] = 0                                    # zero targets: outside the MAPE terms
    p = (t + rng.normal(0, 0.7, n)).astype(F32)
    pb = (t + rng.normal(0.2, 1.1, n)).astype(F32)
    seg = np.minimum((rng.random(n) ** 3 * n_seg).astype(np.int64), n_seg - 1)
    if n_seg >= 3:
        seg[seg == 1] = 0                                          # an empty segment between two filled ones
    unit = np.zeros(n, np.int64) if one_unit else rng.integers(0, n_units, n)
    return {"pred": p, "target": t, "pred_b": pb, "unit": unit, "seg": seg, "n_units": n_units, "n_seg": n_seg}


def dev_sums(c, R, seed, itype, with_b, out=None):
    d = lambda k, dt: torch.from_numpy(np.ascontiguousarray(c[k])).to(DEV, dt)      # noqa: E731
    if out is None:                        # NaN and -1 in every element: one the call does not write cannot pass
        out = (torch.full((R + 1, c["n_seg"], 10 if with_b else 7), float("nan"), dtype=torch.float64, device=DEV),
               torch.full((3,), -1, dtype=torch.int64, device=DEV))
    return bo.boot_sums(d("pred", torch.float32), d("target", torch.float32), d("unit", itype), d("seg", itype),
                        c["n_units"], c["n_seg"], R, seed, d("pred_b", torch.float32) if with_b else None, out=out)


def magnitudes(c, R, seed, with_b):
    """per (replicate, segment, field) the sum of w * |term|, and per segment the number of kept pairs"""
    X = np.abs(bt.host_terms(c["pred"], c["target"], c["pred_b"] if with_b else None))
    ok = ~np.isnan(X).any(1) & (c["seg"] >= 0) & (c["seg"] < c["n_seg"]) & (c["unit"] >= 0) & (c["unit"] < c["n_units"])
    units = np.unique(c["unit"][ok])
    W = np.zeros((R + 1, c["n_units"]))
    if units.size:
        W[:, units] = ref.weights_at(seed, units, R)
    mag = np.zeros((R + 1, c["n_seg"], X.shape[1]))
    count = np.bincount(c["seg"][ok], minlength=c["n_seg"])
    for s in np.unique(c["seg"][ok]):
        sel = ok & (c["seg"] == s)
        mag[:, s] = W[:, c["unit"][sel]] @ X[sel]
    return mag, count


def check_case(c, R, seed, itype, with_b, confidence=0.95, spread=True):
    sums, dropped = dev_sums(c, R, seed, itype, with_b)
    pb = c["pred_b"] if with_b else None
    if len(c["pred"]) <= 64 and R <= 8:
        want, wd = ref.sums(c["pred"], c["target"], c["unit"], c["seg"], c["n_units"], c["n_seg"], R, seed, pb)
    else:                                                          # the host path EQUALS the loop (test_bootstrap_cpu.py)
        want, wd = bt.host_sums(c["pred"], c["target"], c["unit"], c["seg"], c["n_units"], c["n_seg"], R, seed, pb)
    got = sums.cpu().numpy()
    assert same(dropped, wd)
    assert same(got[..., 0], want[..., 0]) and same(got[..., 6], want[..., 6]), "the counts are exact"
    mag, count = magnitudes(c, R, seed, with_b)
    bound = (count[None, :, None] + 8) * U * mag
    err = np.abs(got - want)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0.0))) if err.size else 0.0
    print(f"n {len(c['pred'])} R {R} n_seg {c['n_seg']} with_b {with_b}: largest |device - ref| / bound = {ratio:.3g}")
    assert (err <= bound).all()
    # replicate 0 is what the reducer it extends computes
    if len(c["pred"]):
        d = lambda k, dt: torch.from_numpy(np.ascontiguousarray(c[k])).to(DEV, dt)      # noqa: E731
        # the reducer knows no units and adds a NaN: a pair the bootstrap drops is outside its segments (-1)
        ok = ~np.isnan(bt.host_terms(c["pred"], c["target"], pb)).any(1) & (c["unit"] >= 0) & (c["unit"] < c["n_units"])
        seg8 = torch.from_numpy(np.where(ok, c["seg"], -1)).to(DEV, torch.int64)
        s8 = ops.seg_sums(d("pred", torch.float32), d("target", torch.float32), seg8, c["n_seg"])[0]
        s8 = s8.cpu().numpy()
        assert same(got[0, :, 0], s8[:, 0]) and same(got[0, :, 6], s8[:, 6])
        assert (np.abs(got[0, :, :7] - s8[:, :7]) <= bound[0, :, :7]).all()
    # metrics: the rules applied on the host to the device's own sums
    metrics = bo.boot_metrics(sums)
    gm = metrics.cpu().numpy()
    small = gm.shape[0] * gm.shape[1] <= 20000
    wm = ref.metrics(got) if small else bt.host_metrics(got)
    assert same(gm, wm), "metrics differ from metrics_from_sums on the device's sums"
    # summary
    gs = bo.boot_summary(metrics, confidence).cpu().numpy()
    rows = list(range(min(gm.shape[1], 24))) + [gm.shape[1] - 1]
    ws = ref.summary(gm[:, rows], confidence)
    gs = gs[rows]
    for f in (0, 3, 4, 5, 6):
        if not same(gs[..., f], ws[..., f]):
            for r, k in zip(*np.nonzero(~((gs[..., f] == ws[..., f]) | (np.isnan(gs[..., f]) & np.isnan(ws[..., f]))))):
                print(bt.SUMMARY_FIELDS[f], "row", rows[r], "metric", k, "device", repr(gs[r, k, f]), "numpy",
                      repr(ws[r, k, f]), "n_finite", gs[r, k, 5], ws[r, k, 5], "values", gm[1:, rows[r], k].tolist())
        assert same(gs[..., f], ws[..., f]), bt.SUMMARY_FIELDS[f]
    x = np.where(np.isfinite(gm[1:, rows]), gm[1:, rows], 0.0)
    nf = np.maximum(ws[..., 5], 1)
    ok = ws[..., 5] > 0
    assert (np.abs(gs[..., 1] - ws[..., 1])[ok] <= ((R + 8) * U * np.abs(x).sum(0) / nf)[ok]).all()
    ok = ws[..., 5] > 1
    if spread:
        assert (np.abs(gs[..., 2] - ws[..., 2])[ok] <= ((R + 8) * 2 * U * ws[..., 2])[ok]).all()
    else:       # replicates equal up to rounding: the deviations are cancellation noise, a relative bound says nothing
        assert (gs[..., 2][ok] <= 1e-12 * np.abs(ws[..., 1][ok])).all()
    assert np.isnan(gs[..., 1][ws[..., 5] == 0]).all() and np.isnan(gs[..., 2][ws[..., 5] <= 1]).all()
    return got, gm, gs


# ---------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("n", [0, 1, 2, C - 1, C, C + 1, 3 * C + 1])
def test_sums_metrics_summary_at_every_chunk_count(n):
    i = [0, 1, 2, C - 1, C, C + 1, 3 * C + 1].index(n)
    c = make_case(n, 3, 97, seed=n)
    check_case(c, 5, 11 + i, torch.int64 if i % 2 else torch.int32, with_b=bool(i % 2 == 0))


@pytest.mark.parametrize("R", [1, 2, RB - 1, RB, RB + 1, 4096])
def test_sums_metrics_summary_at_every_replicate_block_count(R):
    n = C + 1 if R == 4096 else 700
    c = make_case(n, 3, 211, seed=R)
    check_case(c, R, 2 ** 63 - 1 if R == RB else R, torch.int64, with_b=R in (2, RB + 1))


@pytest.mark.parametrize("n_seg", [1, 3, 65, 2048])
def test_sums_metrics_summary_at_every_segment_count(n_seg):
    """3 C + 1 pairs: with 1 and 3 segments a segment spans chunk boundaries, with 65 and 2048 a chunk holds many segments
    (written straight to the result), and some segments are empty."""
    c = make_case(3 * C + 1, n_seg, 1500, seed=n_seg)
    got, _, _ = check_case(c, 9, 5, torch.int32 if n_seg == 65 else torch.int64, with_b=n_seg == 65)
    if n_seg >= 65:
        assert (got[0, :, 0] == 0).any(), "an empty segment"
    if n_seg == 1:
        assert got[0, 0, 0] == 3 * C + 1


def test_all_pairs_in_one_unit():
    c = make_case(C + 7, 3, 5, seed=4, one_unit=True)
    got, gm, _ = check_case(c, 40, 8, torch.int64, with_b=False, spread=False)
    w = ref.weights_at(8, [0], 40)[:, 0]
    assert same(got[:, :, 0], w[:, None] * got[0:1, :, 0])
    assert np.isnan(gm[1:][w[1:] == 0]).all() and (w[1:] == 0).any()


# ---------------------------------------------------------------------------------- the chunk protocol
# kept (segment, pairs) runs in sorted order and the dropped pairs behind them; 6 segments, segment 1 always empty
CHUNK_LAYOUTS = {
    "ends_on_chunk_end_then_only_dropped": ([(0, 37), (2, C - 37)], 5),
    "ends_on_chunk_end_then_a_kept_pair": ([(0, 60), (2, C - 60), (4, 1)], 0),
    "direct_then_last_kept_mid_chunk": ([(0, 100), (2, 300), (3, 50)], 40),        # 3: not first, only dropped follow: TAIL
    "one_segment_over_three_chunks": ([(0, 100), (2, 2 * C - 98), (3, 1)], 0),
    "a_whole_chunk_of_dropped": ([(5, 10)], C),
    "all_dropped": ([], 7),
}


def layout_case(kept, n_dropped, seed):
    """The pairs of a layout, shuffled.  A dropped pair is, in turn, of segment -1, of segment n_seg, of a unit out of
    range (below, above), of a NaN target."""
    n_seg, n_units = 6, 97
    rng = np.random.default_rng(seed)
    seg = np.concatenate([np.full(m, s, np.int64) for s, m in kept] + [np.full(n_dropped, 4, np.int64)])
    n = len(seg)
    t = rng.normal(1.0, 2.0, n).astype(F32)
    t[rng.random(n) < 0.05] = 0
    unit = rng.integers(0, n_units, n)
    j = np.arange(n - n_dropped, n)
    seg[j[0::4]] = -1
    seg[j[1::4]] = n_seg
    unit[j[2::8]] = -2
    unit[j[6::8]] = n_units
    t[j[3::4]] = np.nan
    p = (t + rng.normal(0, 0.7, n)).astype(F32)
    pb = (t + rng.normal(0.2, 1.1, n)).astype(F32)
    o = rng.permutation(n)
    dropped = [len(j[0::4]) + len(j[1::4]), len(j[2::4]), len(j[3::4])]
    return {"pred": p[o], "target": t[o], "pred_b": pb[o], "unit": unit[o], "seg": seg[o], "n_units": n_units,
            "n_seg": n_seg}, dropped


@pytest.mark.parametrize("name,R", [(k, 5) for k in CHUNK_LAYOUTS] + [("direct_then_last_kept_mid_chunk", RB + 1)])
def test_head_tail_and_direct_segments_where_walk_and_combine_must_agree(name, R):
    """k_boot_sums closes a segment into its chunk's HEAD slot, its TAIL slot or straight into `sums`, and k_boot_combine
    must skip exactly the last kind (SegChunks, csrc/segsort.h).  The layouts sit where the two could disagree: the last
    kept segment followed only by dropped pairs, a segment that ends on a chunk's end, one over three chunks, a chunk
    without a kept pair, no kept pair at all.  `sums` is prefilled with NaN: an element nobody writes cannot pass, one
    written twice holds the combine's value and fails the bound or the counts."""
    kept, n_dropped = CHUNK_LAYOUTS[name]
    i = list(CHUNK_LAYOUTS).index(name)
    c, dropped = layout_case(kept, n_dropped, seed=100 + i)
    got, _, _ = check_case(c, R, 23 + i, torch.int64 if i % 2 else torch.int32, with_b=bool(i % 2))
    want_n = np.zeros(6)
    for s, m in kept:
        want_n[s] = m
    assert same(got[0, :, 0], want_n) and sum(dropped) == n_dropped
    assert dev_sums(c, 1, 0, torch.int64, False)[1].tolist() == dropped
    if not kept:
        assert not got.any(), "every element of sums is zero"


# ---------------------------------------------------------------------------------- weights
@pytest.mark.parametrize("seed", [0, 1, 2 ** 63 - 1])
@pytest.mark.parametrize("itype", [torch.int32, torch.int64])
def test_weights_recovered_exactly(seed, itype):
    """target = 0, pred = -1: every |e| is 1, so sum |e| is the sum of weights; one pair per segment: the weight itself."""
    n, R = 2048, RB + 3
    rng = np.random.default_rng(1)
    unit = rng.integers(0, 2 ** 31 - 1, n)
    unit[:6] = [0, 1, 2, 3, 2 ** 31 - 3, 2 ** 31 - 2]              # units 0 and 1 share a hash, the largest units
    c = {"pred": np.full(n, -1, F32), "target": np.zeros(n, F32), "unit": unit, "seg": rng.permutation(n),
         "n_units": 2 ** 31 - 1, "n_seg": n}
    sums, dropped = dev_sums(c, R, seed, itype, False)
    got = sums.cpu().numpy()
    want = ref.weights_at(seed, unit, R)                           # [R + 1, n] by pair
    assert not dropped.any().item()
    assert same(got[:, c["seg"], 1], want.astype(np.float64)) and same(got[..., 0], got[..., 1])
    assert same(got[..., 2], got[..., 1]) and not got[..., 3:].any()
    small = ref.weights(seed, 4, 3)                                # the scalar loop on the first units
    assert same(want[:4, :4], small)
    assert same(bt.poisson_weights(seed, 4, R).astype(np.int64), want[:, :4])


# ---------------------------------------------------------------------------------- metric branches
def test_every_metric_branch_and_a_segment_empty_in_some_replicates():
    t = np.array([1.5,                       # 0: one pair: r2 NaN; weight 0 in some replicates: all NaN there
                  2.0, -1.0, 0.5,            # 1: exact predictions: s_sq == 0, r2 1
                  3.0, 3.0, 3.0, 3.0,        # 2: constant target, non-zero residual: ss_tot == 0 exactly, r2 0
                  0.0, 0.0, 0.0,             # 3: no non-zero target: mape NaN
                  1.0, 2.0, 4.0, -3.0, 0.25], F32)            # 4: generic;   5: empty
    p = t.copy()
    p[0] += 0.5
    p[4:8] += np.array([0.5, -0.25, 1.0, 2.0], F32)
    p[8:11] += 1.0
    p[11:] += np.array([0.5, -1.0, 0.25, 0.75, 0.125], F32)
    seg = np.array([0] + [1] * 3 + [2] * 4 + [3] * 3 + [4] * 5)
    c = {"pred": p, "target": t, "pred_b": (t + 1).astype(F32), "unit": np.arange(16), "seg": seg, "n_units": 16, "n_seg": 6}
    R = 64
    for with_b in (False, True):
        sums, _ = dev_sums(c, R, 3, torch.int64, with_b)
        got = sums.cpu().numpy()
        gm = bo.boot_metrics(sums).cpu().numpy()
        assert same(gm, ref.metrics(got))
        for b in range(R + 1):
            for row in range(6):
                m = metrics_from_sums(got[b, row])
                assert same(gm[b, row, :4], [m["mae"], m["rmse"], m["r2"], m["mape"]])
        assert np.isnan(gm[0, 0, 2]) and gm[0, 0, 0] == 0.5 and gm[0, 1, 2] == 1 and gm[0, 2, 2] == 0
        assert np.isnan(gm[0, 3, 3]) and np.isnan(gm[:, 5]).all() and 0 < gm[0, 4, 2] < 1
        w0 = ref.weights_at(3, [0], R)[1:, 0]
        assert (w0 == 0).any() and same(np.isnan(gm[1:, 0, 0]), w0 == 0)
        gs = bo.boot_summary(bo.boot_metrics(sums), 0.9).cpu().numpy()
        assert gs[0, 0, 5] == (w0 > 0).sum() < R and gs[5, 0, 5] == 0 and np.isnan(gs[5, 0, 1:5]).all()
        ws = ref.summary(gm, 0.9)
        for f in (0, 3, 4, 5, 6):
            assert same(gs[..., f], ws[..., f])
        if with_b:
            with np.errstate(invalid="ignore"):
                assert same(gm[..., 8:], gm[..., :4] - gm[..., 4:8])


# ---------------------------------------------------------------------------------- dropped pairs
@pytest.mark.parametrize("itype", [torch.int32, torch.int64])
def test_dropped_pairs_are_counted_per_kind_and_absent_from_every_replicate(itype):
    c = make_case(C + 300, 5, 50, seed=9)
    n = C + 300
    rng = np.random.default_rng(2)
    idx = rng.permutation(n)[:70]
    c["seg"][idx[:10]], c["seg"][idx[10:20]] = -1, 5
    c["unit"][idx[20:30]], c["unit"][idx[30:40]] = -2, 50
    c["unit"][idx[5]] = 50                                         # both: counted under the segment
    c["pred"][idx[40:50]] = np.nan
    c["target"][idx[50:60]] = np.nan
    c["pred_b"][idx[60:70]] = np.nan
    c["pred"][idx[25]] = np.nan                                    # unit and NaN: counted under the unit
    for with_b in (False, True):
        sums, dropped = dev_sums(c, 12, 6, itype, with_b)
        assert dropped.tolist() == [20, 20, 30 if with_b else 20]
        keep = np.ones(n, bool)
        keep[idx[:70 if with_b else 60]] = False
        k = {key: (v[keep] if isinstance(v, np.ndarray) else v) for key, v in c.items()}
        clean, d2 = dev_sums(k, 12, 6, itype, with_b)
        assert not d2.any().item() and torch.equal(bits(sums), bits(clean))
        assert sums[0, :, 0].sum().item() == keep.sum()


# ---------------------------------------------------------------------------------- determinism and capture
def test_two_eager_runs_and_three_replays_of_a_captured_graph_are_bitwise_equal():
    c = make_case(3 * C + 1, 65, 900, seed=21)
    R = RB + 1
    d = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(DEV) for k in ("pred", "target", "pred_b", "unit", "seg")}

    def run():
        sums, dropped = bo.boot_sums(d["pred"], d["target"], d["unit"], d["seg"], 900, 65, R, 17, d["pred_b"])
        metrics = bo.boot_metrics(sums)
        return sums, dropped, metrics, bo.boot_summary(metrics, 0.95)

    first = [o.clone() for o in run()]
    for o, e in zip(run(), first):
        assert torch.equal(bits(o), bits(e)), "two eager runs differ"
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                                      # warm-up off the default stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for _ in range(3):
        for o in outs:
            o.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        for o, e in zip(outs, first):
            assert torch.equal(bits(o), bits(e)), "a replayed capture differs from the eager run"


# ---------------------------------------------------------------------------------- refusals
def test_every_refusal_raises_and_leaves_the_outputs_untouched():
    n = 100
    c = make_case(n, 3, 10)
    d = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(DEV) for k in ("pred", "target", "pred_b", "unit", "seg")}

    def filled(*shape, dtype=torch.float64):
        return torch.full(shape, -7, dtype=dtype, device=DEV)

    def untouched(*ts):
        torch.cuda.synchronize()
        return all(bool((t == -7).all()) for t in ts)

    for n_seg, R in ((3, 0), (3, bo.BOOT_MAX_REPLICATES + 1), (0, 4), (bo.BOOT_MAX_SEG + 1, 4)):
        assert bo.load().mmg_boot_sums_ws_bytes(n, n_seg, R, 0) == 0
        out = (filled(R + 1, n_seg, 7), filled(3, dtype=torch.int64))
        with pytest.raises(MmgError, match="replicates|segments"):
            bo.boot_sums(d["pred"], d["target"], d["unit"], d["seg"], 10, n_seg, R, 0, out=out)
        assert untouched(*out)
        m, s = filled(R + 1, n_seg + 1, 4), filled(n_seg + 1, 4, 7)
        with pytest.raises(MmgError, match="replicates|segments"):
            bo._call("mmg_boot_metrics", filled(R + 1, max(n_seg, 1), 7), n_seg, R, 0, m)
        with pytest.raises(MmgError, match="replicates|segments"):
            bo._call("mmg_boot_summary", m, n_seg, R, 0, 0.95, s)
        assert untouched(m, s)
    sums, dropped = filled(5, 3, 7), filled(3, dtype=torch.int64)
    ws = ops.workspace(bo.load().mmg_boot_sums_ws_bytes(n, 3, 4, 0), DEV)
    args = [d["pred"], d["target"], None, 0, ops._p(d["unit"], torch.int64), ops._p(d["seg"], torch.int64), 8, n, 10, 3, 4,
            0, sums, dropped]

    def with_(i, v):
        a = list(args)
        a[i] = v
        return a

    with pytest.raises(MmgError, match="index_bytes"):
        bo._call("mmg_boot_sums", *with_(6, 2), ws=ws)
    for i in (0, 1, 4, 5, 12, 13):                                 # null pred, target, unit, seg, sums, dropped
        with pytest.raises(MmgError, match="null"):
            bo._call("mmg_boot_sums", *with_(i, None), ws=ws)
    with pytest.raises(MmgError, match="null pred_b"):
        bo._call("mmg_boot_sums", *with_(3, 1), ws=ws)            # with_b without a second predictor
    with pytest.raises(MmgError, match="units"):
        bo._call("mmg_boot_sums", *with_(8, -1), ws=ws)
    with pytest.raises(MmgError, match="workspace"):
        bo._call("mmg_boot_sums", *args, ws=torch.empty(1024, dtype=torch.uint8, device=DEV))
    with pytest.raises(MmgError, match="workspace"):
        bo._call("mmg_boot_sums", *args)                           # no workspace at all
    assert untouched(sums, dropped)
    metrics, summary = filled(5, 4, 4), filled(4, 4, 7)
    for conf in (0.0, 1.0, -0.5, 1.5, float("nan")):
        with pytest.raises(MmgError, match="confidence"):
            bo.boot_summary(metrics, conf, out=summary)
    with pytest.raises(MmgError, match="null"):
        bo._call("mmg_boot_summary", None, 3, 4, 0, 0.95, summary)
    with pytest.raises(MmgError, match="null"):
        bo._call("mmg_boot_metrics", None, 3, 4, 0, metrics)
    assert untouched(metrics, summary)
    with pytest.raises(TypeError):
        bt.bootstrap_sums(d["pred"], d["target"], c["unit"], c["seg"], 10, 3, 4)      # device and host inputs mixed
    with pytest.raises(MmgError):
        bo.boot_metrics(torch.zeros(5, 3, 7, dtype=torch.float64))                    # a host tensor: no fallback


# ---------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def trained():
    g = make_graph(1, seed=0).to(DEV)
    cfg = {"model": {"architecture": "RGCN", "hidden_dim": 64, "num_layers": 2, "dropout": 0.0,
                     "use_batch_norm": True, "activation": "relu"},
           "evaluation": {"stratify_by": ["num_labs", "lab_frequency"]}}
    torch.manual_seed(0)
    model = build_model(cfg, (g.node_types, g.edge_types), None).to(DEV)
    model._init_embeddings(g)
    return g, cfg, model, EdgeMasker(g)


def test_bootstrap_metrics_end_to_end(trained):
    g, cfg, model, masker = trained
    ei, y, _, _ = masker.get_masked_data("test", want_mask=False)
    ei, y = ei.to(DEV), y.to(DEV).reshape(-1).float()
    model.eval()
    with torch.no_grad():
        pred = model.predict_lab_values(g, ei[0], ei[1]).reshape(-1)
    tr_v = masker.get_masked_data("train", want_mask=False)[1].to(DEV).float()
    base = tr_v.mean().expand(pred.numel()).contiguous()
    R = 200
    res = bt.bootstrap_metrics(pred, y, ei[0], ei[1], g, replicates=R, baseline=base, stratify=("num_labs", "lab_frequency"))
    assert list(res.overall.columns) == bt.COLUMNS and res.overall["metric"].tolist() == list(bt.METRICS)
    assert list(res.per_lab.columns) == ["lab_index", "lab_name", "num_samples"] + bt.COLUMNS
    assert list(res.comparison.columns) == ["scope", "lab_index"] + bt.COLUMNS + ["p_below_zero"]
    assert set(res.strata["stratification"]) == {"by_patient_degree", "by_lab_frequency"}
    mae = res.overall.set_index("metric").loc["mae"]
    assert mae["n_finite"] == R and math.isfinite(mae["estimate"]) and mae["lower"] <= mae["estimate"] <= mae["upper"]
    assert mae["std_error"] > 0
    # the estimate is what device_evaluate reports
    from mmgnn.evaluate import device_evaluate
    overall, num_capped, per_lab_df, _ = device_evaluate(pred, y, ei[0], ei[1], g, {}, stratify=())
    assert res.num_capped == num_capped and len(res.per_lab) == 4 * len(per_lab_df)
    for k in bt.METRICS:
        got = res.overall.set_index("metric").loc[k, "estimate"]
        assert abs(got - overall[k]) <= 1e-9 * max(1.0, abs(overall[k]))
    # the paired difference against the global mean is the difference of the two point estimates
    alone = bt.bootstrap_metrics(base, y, ei[0], ei[1], g, replicates=2, n_sigma=0.0)
    b_mae = alone.overall.set_index("metric").loc["mae", "estimate"]
    c = res.comparison[(res.comparison["scope"] == "overall") & (res.comparison["metric"] == "mae")].iloc[0]
    assert c["estimate"] == mae["estimate"] - b_mae
    want = compute_regression_metrics(base.cpu().numpy().astype(np.float64), y.cpu().numpy().astype(np.float64))["mae"]
    assert abs(b_mae - want) <= 1e-6 * want
    assert 0.0 <= c["p_below_zero"] <= 1.0 and c["lower"] <= c["upper"]
    # the patient bootstrap and the pair bootstrap share the estimate, not the interval
    pair = bt.bootstrap_metrics(pred, y, ei[0], ei[1], g, replicates=R, cluster="pair")
    assert pair.overall["estimate"].tolist() == res.overall["estimate"].tolist()
    assert pair.overall["lower"].tolist() != res.overall["lower"].tolist()


def test_evaluate_with_intervals_end_to_end(trained, tmp_path):
    g, cfg, model, masker = trained
    out = bt.evaluate_with_intervals(model, g, masker, cfg, tmp_path, replicates=100,
                                     baselines=("global_mean", "per_lab_mean", "nearest_neighbor"))
    for f in ("evaluation_intervals.json", "per_lab_metrics_ci.csv", "baseline_comparison.csv"):
        assert (tmp_path / f).exists(), f
    per_lab = pd.read_csv(tmp_path / "per_lab_metrics_ci.csv")
    assert list(per_lab.columns) == ["lab_index", "lab_name", "num_samples"] + bt.COLUMNS
    cmp_ = pd.read_csv(tmp_path / "baseline_comparison.csv")
    assert list(cmp_.columns) == ["baseline", "scope", "lab_index"] + bt.COLUMNS + ["p_below_zero"]
    assert set(cmp_["baseline"]) == {"global_mean", "per_lab_mean", "nearest_neighbor"}
    n_scopes = per_lab["lab_index"].nunique() + 1
    assert len(cmp_) == 3 * 4 * n_scopes                           # baseline x metric x scope
    assert out["replicates"] == 100 and [r["metric"] for r in out["overall"]] == list(bt.METRICS)
    mae = out["overall"][0]
    assert mae["n_finite"] == 100 and mae["lower"] <= mae["estimate"] <= mae["upper"]
    assert len(out["baseline_comparison"]) == 3 * 4 and len(out["strata"]) > 0
    import json
    assert json.load(open(tmp_path / "evaluation_intervals.json")) == out
    with pytest.raises(ValueError):
        bt.evaluate_with_intervals(model, g, masker, cfg, tmp_path, baselines=("median",))
