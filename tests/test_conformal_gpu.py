"""Split-conformal intervals on the MI355X (libmmgnn_conformal.so through mmgnn/conformal_ops.py): every device result
against the numpy path of mmgnn/conformal.py (which test_conformal_cpu.py holds equal to the loop reference) -- EQUAL
for the order statistics, tables, bounds and counts; the fp64 width sums within the reordering bound and bitwise equal
from run to run; captured and replayed; conformal_report end to end; every refusal before anything is enqueued."""
import math

import numpy as np
import pandas as pd
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import conformal as cf
from mmgnn import conformal_ops as co
from mmgnn import inference
from mmgnn._lib import MmgError
from mmgnn.model import build_model
from mmgnn.synth import make_graph
from mmgnn.train import EdgeMasker
import conformal_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = np.float32
EDGES3 = [0.0, 6.0, 16.0, float("inf")]
EDGES1 = [1.0, 6.0, 16.0, float("inf")]      # degree 0 lies in no bin
MODES = ["signed", "absolute"]


def dv(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def same(got, want):
    """device tensor against numpy: the same NaN positions, the same infinities, equal numbers"""
    got, want = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and bool(
        np.array_equal(got, want, equal_nan=want.dtype.kind == "f"))


# ---------------------------------------------------------------------------------- mmg_seg_order_stats
def seg_case(n, n_seg, sparse, seed):
    rng = np.random.default_rng(seed)
    keys = rng.standard_normal(n).astype(F32)
    keys[rng.random(n) < 0.2] = F32(0.5)                     # ties
    special = np.array([np.inf, -np.inf, 0.0, -0.0, np.nan, -1.5, 3e38, -3e38, 1e-45, -1e-45], F32)
    pos = rng.random(n) < 0.05
    keys[pos] = special[rng.integers(0, special.size, int(pos.sum()))]
    if sparse:
        used = rng.choice(n_seg, 9, replace=False)           # most segments empty
        seg = used[rng.integers(0, used.size, n)]
    else:
        seg = rng.integers(0, n_seg, n)
    seg = seg.astype(np.int32)
    seg[rng.random(n) < 0.1] = n_seg                         # ignored rows mixed in
    return keys, seg


@pytest.mark.parametrize("n_seg, sparse", [(1, False), (2, False), (65, False), (32768, False), (32768, True)])
@pytest.mark.parametrize("n", [0, 1, 2, 1023, 1024, 1025, 3 * 1024 + 1, 20000])
def test_segmented_order_statistics_equal_the_host(n, n_seg, sparse):
    """The sort's tile is 1,024 keys: with 1 or 2 segments and n past it a segment spans tile boundaries; with 32768
    segments nearly every segment holds one key or none."""
    keys, seg = seg_case(n, n_seg, sparse, n + n_seg)
    for mode in MODES:
        k = keys if mode == "signed" else np.abs(keys)
        for alpha, mc in ((0.1, 0), (0.5, 2), (0.05, 0)):
            got = co.seg_order_stats(dv(k), dv(seg), n_seg, alpha, mode, mc)
            want = cf.host_seg_order_stats(k, seg, n_seg, alpha, mode, mc)
            for g, w, name in zip(got, want, ("count", "q_lo", "q_hi", "shift", "usable")):
                assert same(g, w), (name, mode, alpha)
    if n >= 1023 and n_seg <= 2:
        assert want[0].max() > 400


def test_segments_of_equal_keys_and_of_one_key():
    n = 2500
    keys = np.full(n, -2.25, F32)
    seg = np.zeros(n, np.int32)
    seg[1200] = 1                                            # a segment of one key in the middle of another
    seg[2000:] = 3                                           # segment 2 stays empty
    for mode in MODES:
        k = keys if mode == "signed" else np.abs(keys)
        got = co.seg_order_stats(dv(k), dv(seg), 4, 0.1, mode, 0)
        want = cf.host_seg_order_stats(k, seg, 4, 0.1, mode, 0)
        for g, w in zip(got, want):
            assert same(g, w)
        assert got[0].tolist() == [1999, 1, 0, 500] and got[4].tolist() == [1, 0, 0, 1]
        assert float(got[2][0]) == float(k[0])


# ---------------------------------------------------------------------------------- mmg_cf_fit
def dev_case(c, itype):
    pi, li = c["patient"], c["lab"]
    if itype == torch.int32:
        pi = np.where(pi > 2 ** 31 - 1, 2 ** 31 - 1, pi)
    return dict(pred=dv(c["pred"]), target=dv(c["target"]), patient=dv(pi).to(itype), lab=dv(li).to(itype),
                deg=dv(c["deg"]))


def host_fit(c, edges, alpha, mode, mc=0):
    return cf.host_fit(c["pred"], c["target"], c["patient"], c["lab"], c["n_labs"], c["deg"], edges, alpha, mode, mc)


def dev_fit(d, n_labs, edges, alpha, mode, mc=0):
    return co.cf_fit(d["pred"], d["target"], d["patient"], d["lab"], n_labs, d["deg"], edges, alpha, mode, mc)


@pytest.mark.parametrize("itype", [torch.int64, torch.int32])
@pytest.mark.parametrize("mode", MODES)
def test_fit_tables_and_dropped_counts_equal_the_host(mode, itype):
    c = ref.make_case()
    d = dev_case(c, itype)
    for alpha in (0.05, 0.1, 0.2, 0.5):
        got, want = dev_fit(d, c["n_labs"], EDGES1, alpha, mode), host_fit(c, EDGES1, alpha, mode)
        for g, w, name in zip(got, want, ("table", "level", "n_used", "dropped")):
            assert same(g, w), (name, alpha)
        assert want[3].tolist()[:2] == [4, 3] and want[3][2] > 0 and want[3][3] >= 3
    c = ref.make_case(special=False, n=600)
    d = dev_case(c, itype)
    seen = set()
    for mc in (0, 30, 150, 450, 10 ** 6):                    # cell -> lab -> all -> none
        got, want = dev_fit(d, c["n_labs"], EDGES3, 0.1, mode, mc), host_fit(c, EDGES3, 0.1, mode, mc)
        for g, w in zip(got, want):
            assert same(g, w), mc
        seen |= set(want[1].tolist())
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("mode", MODES)
def test_fit_without_pairs_and_through_the_public_object(mode):
    z = torch.zeros(0, device=DEV)
    deg = dv(np.array([1, 7], np.int32))
    got = co.cf_fit(z, z, z.long(), z.long(), 3, deg, EDGES3, 0.1, mode, 0)
    assert set(got[1].tolist()) == {3} and got[3].tolist() == [0, 0, 0, 0] and not got[2].any()
    assert torch.isneginf(got[0][0]).all() and torch.isposinf(got[0][1]).all() and not got[0][2].any()
    c = ref.make_case()
    d = dev_case(c, torch.int64)
    a = cf.LabConformal(alpha=0.2, score=mode).fit(d["pred"], d["target"], d["lab"], d["patient"], d["deg"], n_labs=5)
    b = cf.LabConformal(alpha=0.2, score=mode).fit(c["pred"], c["target"], c["lab"], c["patient"], c["deg"], n_labs=5)
    for x, y in zip(a._host, b._host):
        assert same(x, y)
    for x, y in zip(a.predict(d["pred"], d["lab"], d["patient"]), b.predict(c["pred"], c["lab"], c["patient"])):
        assert same(x, y)
    # a table fitted on the host serves device predictions, and the other way round
    for x, y in zip(b.predict(d["pred"], d["lab"], d["patient"]), a.predict(c["pred"], c["lab"], c["patient"])):
        assert same(x, y)


# ---------------------------------------------------------------------------------- apply
def random_table(n_cells, rng):
    q = np.sort(rng.standard_normal((2, n_cells)).astype(F32), axis=0)
    t = np.stack([q[0], q[1], (rng.standard_normal(n_cells) * 0.1).astype(F32)])
    t[0, ::7], t[1, ::7], t[2, ::7] = -np.inf, np.inf, 0.0   # rows of no usable level
    return np.ascontiguousarray(t, F32)


N_PAT = 700
DEG = np.random.default_rng(1).integers(0, 40, N_PAT).astype(np.int32)


@pytest.mark.parametrize("itype", [torch.int64, torch.int32])
@pytest.mark.parametrize("n_labs", [3, 50, 2048])
def test_apply_pairs_is_bit_equal_to_the_host(n_labs, itype):
    """3 and 50 labs: the table in LDS; 2048 x 3 cells: read from memory."""
    rng = np.random.default_rng(n_labs)
    n = 5000
    table = random_table(n_labs * 3, rng)
    pred = rng.standard_normal(n).astype(F32)
    pred[:4] = [np.nan, np.inf, -np.inf, -0.0]
    patient, lab = rng.integers(-2, N_PAT + 2, n), rng.integers(-1, n_labs + 1, n)
    for shift in (False, True):
        got = co.cf_apply_pairs(dv(pred), dv(patient).to(itype), dv(lab).to(itype), n_labs, dv(DEG), EDGES1, dv(table), shift)
        want = cf.host_apply_pairs(pred, patient, lab, n_labs, DEG, EDGES1, table, shift)
        for g, w in zip(got, want):
            assert same(g, w)
    assert np.isneginf(want[1]).sum() > n // 10


@pytest.mark.parametrize("pad", ["none", "pad4", "odd"])
@pytest.mark.parametrize("n_rows", [1, 2, 1000])
@pytest.mark.parametrize("n_labs", [1, 3, 50, 63, 64, 65, 512, 2048])
def test_apply_matrix_is_bit_equal_to_the_host(n_labs, n_rows, pad):
    """Contiguous, padded to a multiple of 4 floats (16-byte lanes with a tail) and padded to an odd stride (one float
    per lane), on the input and on the outputs; the padding columns keep their sentinel.  rows None (row i is patient i;
    rows past the 700 patients have no cell), given, repeated and out of range."""
    rng = np.random.default_rng(n_labs * 7 + n_rows)
    table = random_table(n_labs * 3, rng)
    ld = {"none": n_labs, "pad4": (n_labs + 3) // 4 * 4 + 4, "odd": n_labs + 1 + (n_labs % 2)}[pad]
    buf = rng.standard_normal((n_rows, ld)).astype(F32)
    buf[0, 0] = np.nan
    pred_h = buf[:, :n_labs]
    pred_d = dv(buf)[:, :n_labs]
    rows_h = rng.integers(0, N_PAT, n_rows)
    if n_rows > 2:
        rows_h[1] = rows_h[0]                                # a repeated patient
        rows_h[2], rows_h[3] = -1, N_PAT                     # out of range
    for rows, itype in ((None, None), (rows_h, torch.int64), (rows_h, torch.int32)):
        for shift in (False, True):
            outs = [torch.full((n_rows, ld), -7.0, device=DEV) for _ in range(3)]
            got = co.cf_apply_matrix(pred_d, None if rows is None else dv(rows).to(itype), dv(DEG), EDGES1, dv(table), shift,
                                     out=tuple(o[:, :n_labs] for o in outs))
            want = cf.host_apply_matrix(pred_h, rows, DEG, EDGES1, table, shift)
            for g, w, o in zip(got, want, outs):
                assert same(g, w)
                assert bool((o[:, n_labs:] == -7.0).all())
    got = co.cf_apply_matrix(pred_d, None, dv(DEG), EDGES1, dv(table))            # outputs of its own
    for g, w in zip(got, cf.host_apply_matrix(pred_h, None, DEG, EDGES1, table)):
        assert same(g, w)


# ---------------------------------------------------------------------------------- coverage
def check_coverage(c, d, table, edges):
    counts, width = co.cf_coverage(d["pred"], d["target"], d["patient"], d["lab"], c["n_labs"], d["deg"], edges, dv(table))
    again = co.cf_coverage(d["pred"], d["target"], d["patient"], d["lab"], c["n_labs"], d["deg"], edges, dv(table))
    hc, _ = cf.host_coverage(c["pred"], c["target"], c["patient"], c["lab"], c["n_labs"], c["deg"], edges, table)
    assert same(counts, hc) and torch.equal(counts, again[0])
    assert np.array_equal(width.cpu().numpy().view(np.int64), again[1].cpu().numpy().view(np.int64)), "two runs differ"
    _, widths = ref.coverage(c["pred"], c["target"], c["patient"], c["lab"], c["n_labs"], c["deg"], edges, table)
    for cell, ws in enumerate(widths):
        tot, mag = math.fsum(float(w) for w in ws), math.fsum(abs(float(w)) for w in ws)
        assert abs(float(width[cell]) - tot) <= (len(ws) + 8) * 2.0 ** -53 * mag, cell
    return hc


@pytest.mark.parametrize("itype", [torch.int64, torch.int32])
@pytest.mark.parametrize("mode", MODES)
def test_coverage_counts_equal_the_host_and_width_sums_are_reproducible(mode, itype):
    c = ref.make_case(n=3000)
    table = host_fit(c, EDGES1, 0.1, mode)[0]
    ev = ref.make_case(seed=1, n=3000)
    hc = check_coverage(ev, dev_case(ev, itype), table, EDGES1)
    assert hc[-1, 5] > 7 and hc[:-1, 5].sum() == 2 and hc[:, 4].sum() > 0 and hc[:, 1].sum() > 1500


def test_coverage_of_many_cells_and_of_no_pairs():
    rng = np.random.default_rng(8)
    n, n_labs = 4000, 2048
    table = random_table(n_labs * 3, rng)
    c = dict(pred=rng.standard_normal(n).astype(F32), target=rng.standard_normal(n).astype(F32),
             patient=rng.integers(0, N_PAT, n), lab=rng.integers(0, n_labs, n), n_labs=n_labs, deg=DEG)
    check_coverage(c, dev_case(c, torch.int64), table, EDGES3)
    e = {k: (v[:0] if isinstance(v, np.ndarray) and k != "deg" else v) for k, v in c.items()}
    hc = check_coverage(e, dev_case(e, torch.int64), table, EDGES3)
    assert not hc.any()


# ---------------------------------------------------------------------------------- capture
def test_fit_apply_and_coverage_replay_from_one_captured_graph():
    """No allocation by the library, no memset node and no host synchronisation inside: the three calls are captured
    into ONE hipGraph, and every replay on changed input contents equals the eager result on those contents."""
    cases = [ref.make_case(seed=s, n=2500) for s in (0, 1, 2)]
    d = dev_case(cases[0], torch.int64)

    def run():
        table, level, n_used, dropped = dev_fit(d, 5, EDGES1, 0.1, "signed", 10)
        point, lower, upper = co.cf_apply_pairs(d["pred"], d["patient"], d["lab"], 5, d["deg"], EDGES1, table, True)
        m = co.cf_apply_matrix(d["pred"][:2000].view(400, 5), d["patient"][:400], d["deg"], EDGES1, table, True)
        counts, width = co.cf_coverage(d["pred"], d["target"], d["patient"], d["lab"], 5, d["deg"], EDGES1, table)
        return (table, level, n_used, dropped, point, lower, upper) + m + (counts, width)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                                # warm-up off the default stream, as torch.cuda.graph asks
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for c in cases[1:]:
        for k, v in dev_case(c, torch.int64).items():
            d[k].copy_(v)
        for o in outs:
            o.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [o.clone() for o in outs]
        eager = run()
        for r, e in zip(replayed, eager):
            assert torch.equal(r.view(torch.uint8), e.view(torch.uint8)), "a replayed capture differs from the eager run"
        want = host_fit(c, EDGES1, 0.1, "signed", 10)
        for g, w in zip(replayed[:4], want):
            assert same(g, w)


# ---------------------------------------------------------------------------------- end to end
def test_conformal_report_end_to_end(tmp_path):
    g = make_graph(1, seed=0).to(DEV)
    cfg = {"model": {"architecture": "RGCN", "hidden_dim": 64, "num_layers": 2, "dropout": 0.0,
                     "use_batch_norm": True, "activation": "relu"}}
    torch.manual_seed(0)
    model = build_model(cfg, (g.node_types, g.edge_types), None).to(DEV)
    model._init_embeddings(g)
    masker = EdgeMasker(g)
    pi, li, y = cf._split_pairs(g, masker, "train")
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    model.train()
    for _ in range(5):                                       # briefly trained
        opt.zero_grad()
        (model.predict_lab_values(g, pi, li).reshape(-1) - y).abs().mean().backward()
        opt.step()
    obj, table, cov = cf.conformal_report(model, g, masker, output_dir=tmp_path)
    # the host path on the same predictions copied to numpy
    _, pv, yv, piv, liv = cf._predict_split(model, g, masker, "val")
    _, pt, yt, pit, lit = cf._predict_split(model, g, masker, "test")
    deg = cf.patient_degrees(g, None)
    host = cf.LabConformal().fit(pv.cpu().numpy(), yv.cpu().numpy(), liv.cpu().numpy(), piv.cpu().numpy(), deg, n_labs=50)
    (tmp_path / "host").mkdir()
    cf.write_report(host.table_frame(), host.coverage(pt.cpu().numpy(), yt.cpu().numpy(), lit.cpu().numpy(),
                                                      pit.cpu().numpy()), tmp_path / "host")
    for f in ("conformal_table.csv", "conformal_coverage.csv"):
        a, b = pd.read_csv(tmp_path / f), pd.read_csv(tmp_path / "host" / f)
        if f == "conformal_coverage.csv":                    # the width sums are reordered fp64 sums of the same terms
            assert np.allclose(a.pop("mean_width"), b.pop("mean_width"), rtol=1e-12, atol=0, equal_nan=True)
        pd.testing.assert_frame_equal(a, b, check_exact=True)
    assert list(table.columns) == cf.TABLE_COLUMNS and len(table) == 150 and list(cov.columns) == cf.COVERAGE_COLUMNS
    m, n_eval = int(masker.val_mask.sum()), int(masker.test_mask.sum())
    overall = cov.iloc[0]
    bound = ref.coverage_bound(0.1, m, n_eval)
    print(f"overall test coverage {overall['coverage']:.4f} on {overall['n']} pairs (m {m}), allowed 0.9 +- {bound:.4f}; "
          f"levels {table.level.value_counts().to_dict()}")
    assert overall["n"] == n_eval and abs(overall["coverage"] - 0.9) <= bound
    # the dense form: one forward, every cell with its interval
    rows = torch.tensor([0, 5, 5, 1833], device=DEV)
    point, lower, upper, observed = cf.impute_intervals(model, g, obj, rows)
    assert point.shape == lower.shape == upper.shape == observed.shape == (4, 50)
    pp = obj.predict(point.reshape(-1), torch.arange(50, device=DEV).repeat(4), rows.repeat_interleave(50))
    assert torch.equal(lower.reshape(-1), pp[1]) and torch.equal(upper.reshape(-1), pp[2])
    assert bool((lower <= upper).all()) and torch.equal(lower[1], lower[2]) and torch.equal(upper[1], upper[2])
    # the patient reports: unchanged without intervals=, exactly four more keys per predicted entry with it
    lab_indexer = {f"L{i}": i for i in range(50)}
    lab_stats = pd.DataFrame({"ITEMID": list(lab_indexer), "mean": np.linspace(1.0, 2.0, 50), "std": np.linspace(0.5, 1.5, 50)})
    pidx = {str(i): i for i in range(1834)}
    model.eval()
    args = ([5, 1833], g, model, DEV, None, lab_stats, masker, pidx, lab_indexer)
    plain, with_iv = inference.predict_for_patients(*args), inference.predict_for_patients(*args, intervals=obj)
    extra = {"lower", "upper", "normalized_lower", "normalized_upper"}
    lo_h, hi_h = lower.cpu().numpy(), upper.cpu().numpy()
    seen = 0
    for row, a_, b_ in zip((1, 3), plain, with_iv):
        assert a_["measured_labs"] == b_["measured_labs"]
        for group in ("masked_labs", "truly_missing_labs"):
            assert list(a_[group]) == list(b_[group])
            for name, entry in b_[group].items():
                assert set(entry) == set(a_[group][name]) | extra
                assert {k: entry[k] for k in a_[group][name]} == a_[group][name]
                li_ = lab_indexer[name]
                assert entry["normalized_lower"] == float(lo_h[row, li_]) and entry["normalized_upper"] == float(hi_h[row, li_])
                seen += 1
    assert seen > 0                                          # (patients with many labs have few entries to predict)


# ---------------------------------------------------------------------------------- refusals
def test_every_limit_is_refused_before_anything_is_enqueued():
    c = ref.make_case(n=100)
    d = dev_case(c, torch.int64)
    table = dv(random_table(15, np.random.default_rng(0)))
    lib = co.load()
    k, s = d["pred"], d["lab"].to(torch.int32)
    with pytest.raises(MmgError, match="segments"):
        co.seg_order_stats(k, s, 0, 0.1)
    with pytest.raises(MmgError, match="segments"):
        co.seg_order_stats(k, s, co.CF_MAX_CELLS + 1, 0.1)
    for alpha in (0.0, 1.0, float("nan"), -0.1):
        with pytest.raises(MmgError, match="alpha"):
            co.seg_order_stats(k, s, 4, alpha)
        with pytest.raises(MmgError, match="alpha"):
            dev_fit(d, 5, EDGES3, alpha, "signed")
    with pytest.raises(MmgError, match="min_count"):
        co.seg_order_stats(k, s, 4, 0.1, "signed", -1)
    with pytest.raises(MmgError, match="labs"):
        dev_fit(d, co.CF_MAX_LABS + 1, [0.0, 1.0], 0.1, "signed")
    with pytest.raises(MmgError, match="cells"):
        dev_fit(d, 2048, [float(j) for j in range(18)], 0.1, "signed")          # 2048 x 17
    with pytest.raises(MmgError, match="bins"):
        dev_fit(d, 5, [float(j) for j in range(co.CF_MAX_BINS + 2)], 0.1, "signed")
    with pytest.raises(MmgError, match="bins"):
        dev_fit(d, 5, [0.0], 0.1, "signed")
    with pytest.raises(MmgError, match="ascending"):
        dev_fit(d, 5, [0.0, 6.0, 6.0], 0.1, "signed")
    with pytest.raises(MmgError, match="ascending"):
        co.cf_apply_pairs(d["pred"], d["patient"], d["lab"], 5, d["deg"], [0.0, float("nan"), 7.0, 9.0], table)
    with pytest.raises(MmgError, match="ascending"):
        co.cf_coverage(d["pred"], d["target"], d["patient"], d["lab"], 5, d["deg"], [3.0, 2.0, 1.0, 0.0], table)
    # a short and a missing workspace, straight through the C ABI
    n = 100
    z = torch.zeros(64, dtype=torch.int32, device=DEV)
    zf = torch.zeros(64, device=DEV)
    ws = torch.empty(64, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.mmg_seg_order_stats_ws_bytes(n, 4) > 64 and lib.mmg_cf_fit_ws_bytes(n, 5, 3) > 64
    assert lib.mmg_seg_order_stats_ws_bytes(-1, 4) == 0 and lib.mmg_cf_fit_ws_bytes(n, 2048, 17) == 0
    assert lib.mmg_cf_coverage_ws_bytes(n, 0, 3) == 0 and lib.mmg_seg_order_stats_ws_bytes(2 ** 31, 4) == 0
    before = zf.clone()
    for w, nbytes in ((ws.data_ptr(), 64), (None, 0)):
        rc = lib.mmg_seg_order_stats(k.data_ptr(), s.data_ptr(), n, 4, 0.1, 0, 0, z.data_ptr(), zf.data_ptr(), zf.data_ptr(),
                                     zf.data_ptr(), z.data_ptr(), w, nbytes, stream)
        assert rc == mmgnn._lib.MMG_E_WS
    rc = lib.mmg_seg_order_stats(k.data_ptr(), s.data_ptr(), 2 ** 31, 4, 0.1, 0, 0, z.data_ptr(), zf.data_ptr(), zf.data_ptr(),
                                 zf.data_ptr(), z.data_ptr(), ws.data_ptr(), 64, stream)
    assert rc == mmgnn._lib.MMG_E_ARG
    torch.cuda.synchronize()
    assert torch.equal(zf, before) and not z.any()
