"""Stacked recalibration on the MI355X (libmmgnn_stack.so through mmgnn/stack_ops.py): every device result EQUALS the
numpy path of mmgnn/stacking.py (which test_stacking_cpu.py holds to the loop reference) -- sums, coefficients, levels,
counts, dropped, applied values and scores; captured and replayed; stacking_report and impute_stacked end to end; every
refusal before anything is enqueued."""
import numpy as np
import pandas as pd
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import conformal as cf
from mmgnn import stack_ops as so
from mmgnn import stacking as st
from mmgnn._lib import MmgError
from mmgnn.model import build_model
from mmgnn.synth import make_graph
from mmgnn.train import EdgeMasker
import stack_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = np.float32
INF = float("inf")
EDGES3 = [0.0, 6.0, 16.0, INF]
EDGES1 = [1.0, 6.0, 16.0, INF]               # degree 0 lies in no bin; degrees 6 and 16 sit on the inner edges
ONE_BIN = [1.0, INF]
C = so.ST_CHUNK


def dv(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def same(got, want):
    """device tensor against numpy: the same dtype, NaN positions and infinities, equal numbers"""
    got, want = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and bool(
        np.array_equal(got, want, equal_nan=want.dtype.kind == "f"))


def dev_case(c, itype=torch.int64):
    return dict(feats=[dv(f) for f in c["feats"]], target=dv(c["target"]), patient=dv(c["patient"]).to(itype),
                lab=dv(c["lab"]).to(itype), deg=dv(c["deg"]))


def check_everything(c, edges, folds=1, seed=0, itype=torch.int64, ridge=1e-3, min_count=30):
    """sums, solve, both applies and the scores of one case on the device against the host -> the host's (sums, level)"""
    d, K, L, nb = dev_case(c, itype), len(c["feats"]), c["n_labs"], len(edges) - 1
    sums, dropped = so.stack_sums(d["feats"], d["target"], d["patient"], d["lab"], L, d["deg"], edges, folds, seed)
    hs, hd = st.host_sums(c["feats"], c["target"], c["patient"], c["lab"], L, c["deg"], edges, folds, seed)
    assert same(sums, hs), "sums"
    assert same(dropped, hd), "dropped"
    coef, level, n_used = so.stack_solve(sums, L, nb, K, ridge, min_count)
    hc, hl, hu = st.host_solve(hs, L, nb, K, ridge, min_count)
    assert same(level, hl), "level"
    assert same(n_used, hu), "n_used"
    assert same(coef, hc), "coef"
    y = None
    for cross in ((False, True) if folds > 1 else (False,)):
        y = so.stack_apply_pairs(d["feats"], d["patient"], d["lab"], L, d["deg"], edges, coef, seed, cross)
        hy = st.host_apply_pairs(c["feats"], c["patient"], c["lab"], L, c["deg"], edges, hc, seed, cross)
        assert same(y, hy), f"apply (cross {cross})"
    sc, sd = so.stack_scores(d["feats"][0], y, d["target"], d["patient"], d["lab"], L, d["deg"], edges)
    hsc, hsd = st.host_scores(c["feats"][0], hy, c["target"], c["patient"], c["lab"], L, c["deg"], edges)
    assert same(sc, hsc), "scores"
    assert same(sd, hsd), "scores: dropped"
    return hs, hl, hd


# ---------------------------------------------------------------------------------- fit, apply, scores
@pytest.mark.parametrize("itype", [torch.int64, torch.int32])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_every_result_equals_the_host(K, itype):
    """Every drop kind in its order of precedence (a bad lab with a NaN is a bad lab), +-inf values kept, three bins
    with a degree on each edge, three folds."""
    c = ref.make_case(seed=K, n=6000, K=K)
    hs, hl, hd = check_everything(c, EDGES1, 3, 7, itype)
    assert hd.tolist()[:2] == [5, 2] and hd[2] > 0 and hd[3] == 3
    assert {0, 6, 16} <= set(c["deg"][np.unique(c["patient"][(c["patient"] >= 0) & (c["patient"] < 40)])].tolist())
    c = ref.make_case(seed=K, n=6000, K=K, special=False)
    check_everything(c, EDGES3, 1, 0, itype, ridge=0.0, min_count=0)


@pytest.mark.parametrize("folds", [1, 2, 5])
@pytest.mark.parametrize("edges", [ONE_BIN, EDGES1])
def test_folds_and_bins(folds, edges):
    c = ref.make_case(seed=folds, n=5000, K=2, special=False)     # (an infinite value would spoil the all-pairs level)
    seen = set()
    for mc in (0, 30, 450, 2000, 10 ** 6):                  # cell -> lab -> all -> none
        _, hl, _ = check_everything(c, edges, folds, 3, min_count=mc)
        seen |= set(hl.reshape(-1).tolist())
    assert seen >= ({0, 2, 3} if len(edges) == 2 else {0, 1, 2, 3})


def test_no_pairs_and_one_pair():
    c = ref.make_case(seed=0, n=1500, K=2)
    empty = dict(c, feats=[f[:0] for f in c["feats"]], target=c["target"][:0], patient=c["patient"][:0], lab=c["lab"][:0])
    for folds in (1, 4):
        hs, hl, hd = check_everything(empty, EDGES3, folds, 1)
        assert not hs.any() and set(hl.reshape(-1).tolist()) == {3} and not hd.any()
    one = dict(c, feats=[f[20:21] for f in c["feats"]], target=c["target"][20:21], patient=c["patient"][20:21],
               lab=c["lab"][20:21])
    for folds in (1, 4):
        hs, hl, _ = check_everything(one, EDGES3, folds, 1, min_count=0)
        assert hs[:, :, 0].sum() == 1 and set(hl.reshape(-1).tolist()) == {3}       # one pair: below K + 2


def chunk_case(K=2, seed=0):
    """One bin.  Lab 0: exactly C pairs; lab 1: none, between full ones; lab 2: C + 1; lab 3: 1000, so that lab 4 begins
    in the middle of the sorted pairs' third 4096 and, with 9000 pairs, takes three chunks of its own; labs 5 .. 1004: one
    pair each.  19,193 pairs, shuffled."""
    rng = np.random.default_rng(seed)
    lab = np.concatenate([np.full(C, 0), np.full(C + 1, 2), np.full(1000, 3), np.full(9000, 4), np.arange(5, 1005)])
    rng.shuffle(lab)
    n = lab.size
    assert n < 20000
    t = rng.standard_normal(n).astype(F32)
    feats = [(0.4 * t + 0.5 * rng.standard_normal(n)).astype(F32) for _ in range(K)]
    return dict(feats=feats, target=t, patient=rng.integers(0, 300, n).astype(np.int64), lab=lab.astype(np.int64),
                n_labs=1005, deg=rng.integers(1, 30, 300).astype(np.int32))


@pytest.mark.parametrize("K, folds", [(1, 1), (4, 1), (2, 2)])
def test_cells_at_the_chunk_boundaries(K, folds):
    c = chunk_case(K)
    hs, hl, _ = check_everything(c, ONE_BIN, folds, 2)
    counts = hs[:, :, 0].sum(0)
    assert counts[:5].tolist() == [C, 0, C + 1, 1000, 9000] and set(counts[5:].tolist()) == {1}
    if folds == 1:
        assert hl[0, :5].tolist() == [0, 2, 0, 0, 0] and set(hl[0, 5:].tolist()) == {2}     # no lab level below one bin's


def test_two_runs_are_bitwise_equal():
    c = chunk_case(3, seed=1)
    d = dev_case(c)
    runs = [so.stack_sums(d["feats"], d["target"], d["patient"], d["lab"], 1005, d["deg"], ONE_BIN, 2, 0)[0] for _ in range(2)]
    assert torch.equal(runs[0].view(torch.int64), runs[1].view(torch.int64))


# ---------------------------------------------------------------------------------- the matrix epilogue
N_PAT = 300
DEG = np.random.default_rng(1).integers(0, 40, N_PAT).astype(np.int32)


@pytest.mark.parametrize("n_rows", [1, 65, 257])
@pytest.mark.parametrize("n_labs", [1, 50, 65])
def test_apply_matrix_equals_the_host_and_the_pair_path(n_labs, n_rows):
    """Inputs and output wider than n_labs (a canary border that must come back untouched), a broadcast per-lab feature,
    rows None (row i is patient i; rows past the 300 patients have no cell), given, repeated and out of range, the
    coefficients of all pairs."""
    rng = np.random.default_rng(n_labs * 7 + n_rows)
    coef = rng.standard_normal((4, n_labs * 3, 4))          # three folds and all pairs, K = 3
    coef[:, ::5] = [0.0, 1.0, 0.0, 0.0]
    ld, ld_out = n_labs + 3, n_labs + 5
    bufs = [rng.standard_normal((n_rows, ld)).astype(F32) for _ in range(2)]
    bufs[0][0, 0] = np.nan
    vec = rng.standard_normal(n_labs).astype(F32)
    host_feats = [bufs[0][:, :n_labs], vec, bufs[1][:, :n_labs]]
    dev_feats = [dv(bufs[0])[:, :n_labs], dv(vec), dv(bufs[1])[:, :n_labs]]
    rows_h = rng.integers(0, N_PAT, n_rows)
    if n_rows > 3:
        rows_h[1] = rows_h[0]                                # a repeated patient
        rows_h[2], rows_h[3] = -1, N_PAT                     # out of range
    for rows, itype in ((None, None), (rows_h, torch.int64), (rows_h, torch.int32)):
        out = torch.full((n_rows, ld_out), -7.0, device=DEV)
        got = so.stack_apply_matrix(dev_feats, None if rows is None else dv(rows).to(itype), dv(DEG), EDGES1, dv(coef),
                                    out=out[:, :n_labs])
        want = st.host_apply_matrix(host_feats, rows, DEG, EDGES1, coef)
        assert same(got, want)
        assert bool((out[:, n_labs:] == -7.0).all())
        r = np.arange(n_rows) if rows is None else rows
        pairs = so.stack_apply_pairs([dv(np.array(np.broadcast_to(f, (n_rows, n_labs))).reshape(-1))
                                      for f in host_feats], dv(np.repeat(r, n_labs)),
                                     dv(np.tile(np.arange(n_labs), n_rows)), n_labs, dv(DEG), EDGES1, dv(coef))
        assert torch.equal(got.reshape(-1).view(torch.int32), pairs.view(torch.int32))
    assert np.isnan(want[0, 0])
    got = so.stack_apply_matrix(dev_feats, dv(rows_h), dv(DEG), EDGES1, dv(coef), seed=5, cross=True)     # out of its own
    assert same(got, st.host_apply_matrix(host_feats, rows_h, DEG, EDGES1, coef, 5, True))


def test_the_public_object_on_the_device_equals_it_on_the_host():
    c = ref.make_case(seed=9, n=4000, K=2)
    d = dev_case(c)
    a = st.LabStacker(folds=3, seed=2).fit(d["feats"], d["target"], d["lab"], d["patient"], d["deg"], n_labs=5)
    b = st.LabStacker(folds=3, seed=2).fit(c["feats"], c["target"], c["lab"], c["patient"], c["deg"], n_labs=5)
    for x, y in zip(a._host, b._host):
        assert same(x, y)
    for fn in ("predict", "cross_fit_predict"):
        assert same(getattr(a, fn)(d["feats"], d["lab"], d["patient"]), getattr(b, fn)(c["feats"], c["lab"], c["patient"]))
    # a table fitted on the host serves device predictions, and the other way round
    assert same(b.predict(d["feats"], d["lab"], d["patient"]), a.predict(c["feats"], c["lab"], c["patient"]))
    sa, da = a.score_sums(d["feats"], d["target"], d["lab"], d["patient"])
    sb, db = b.score_sums(c["feats"], c["target"], c["lab"], c["patient"])
    assert same(sa, sb) and same(da, db)
    m = c["feats"][0][:200].reshape(40, 5).copy()
    vec = np.linspace(-1, 1, 5).astype(F32)
    assert same(a.predict_matrix([dv(m), dv(vec)]), b.predict_matrix([m, vec]))
    with pytest.raises(MmgError):                            # a device table never falls back to the host for host data
        so.stack_apply_pairs([torch.zeros(3)], torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64), 5,
                             d["deg"], EDGES3, dv(a.coef))


# ---------------------------------------------------------------------------------- capture
def test_fit_apply_and_scores_replay_from_one_captured_graph():
    """No allocation by the library, no memset node and no host synchronisation inside: the calls are captured into ONE
    hipGraph; two replays on changed input contents are bitwise the eager result on those contents, and equal the host."""
    cases = [ref.make_case(seed=s, n=6000, K=2) for s in (0, 1, 2)]
    d = dev_case(cases[0])

    def run():
        sums, dropped = so.stack_sums(d["feats"], d["target"], d["patient"], d["lab"], 5, d["deg"], EDGES1, 3, 4)
        coef, level, n_used = so.stack_solve(sums, 5, 3, 2, 1e-3, 30)
        y = so.stack_apply_pairs(d["feats"], d["patient"], d["lab"], 5, d["deg"], EDGES1, coef, 4, True)
        m = so.stack_apply_matrix([d["feats"][0][:2000].view(400, 5), d["feats"][1][:5]], d["patient"][:400], d["deg"], EDGES1,
                                  coef)
        sc, sd = so.stack_scores(d["feats"][0], y, d["target"], d["patient"], d["lab"], 5, d["deg"], EDGES1)
        return sums, dropped, coef, level, n_used, y, m, sc, sd

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                                # warm-up off the default stream, as torch.cuda.graph asks
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for c in cases[1:]:
        nd = dev_case(c)
        for k in ("target", "patient", "lab", "deg"):
            d[k].copy_(nd[k])
        for x, y in zip(d["feats"], nd["feats"]):
            x.copy_(y)
        for o in outs:
            o.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [o.clone() for o in outs]
        eager = run()
        for r, e in zip(replayed, eager):
            assert torch.equal(r.view(torch.uint8), e.view(torch.uint8)), "a replayed capture differs from the eager run"
        hs, hd = st.host_sums(c["feats"], c["target"], c["patient"], c["lab"], 5, c["deg"], EDGES1, 3, 4)
        hc, hl, hu = st.host_solve(hs, 5, 3, 2, 1e-3, 30)
        for g, w in zip(replayed[:5], (hs, hd, hc, hl, hu)):
            assert same(g, w)


# ---------------------------------------------------------------------------------- end to end
def test_stacking_report_and_impute_stacked_end_to_end(tmp_path):
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
    obj, table, scores, comparison = st.stacking_report(model, g, masker, output_dir=tmp_path, replicates=200)
    for f in ("stacking_table.csv", "stacking_scores.csv", "stacking_comparison.csv"):
        assert (tmp_path / f).exists() and len(pd.read_csv(tmp_path / f)) > 0
    assert len(table) == 150 and list(table.columns)[-3:] == ["intercept", "w_gnn", "w_per_lab_mean"]
    assert list(scores.columns) == st.SCORE_COLUMNS and scores.iloc[0]["n"] == int(masker.test_mask.sum())
    mae = comparison[(comparison.scope == "overall") & (comparison.metric == "mae")].iloc[0]
    top = scores.iloc[0]
    print(f"test MAE raw {top['mae_raw']:.4f} -> stacked {top['mae_stacked']:.4f}; stacked - raw {mae['estimate']:.4f} "
          f"[{mae['lower']:.4f}, {mae['upper']:.4f}]; levels {table.level.value_counts().to_dict()}")
    assert np.isclose(mae["estimate"], top["mae_stacked"] - top["mae_raw"], rtol=1e-9, atol=1e-12)
    # the host path on the same features copied to numpy gives the same table
    fitted = st._fit_named_baselines(model, g, masker, ("per_lab_mean",))
    _, feats, yv, piv, liv = st._split_features(model, g, masker, "val", fitted)
    host = st.LabStacker().fit({k: v.cpu().numpy() for k, v in feats.items()}, yv.cpu().numpy(), liv.cpu().numpy(),
                               piv.cpu().numpy(), cf.patient_degrees(g, None), n_labs=50)
    for x, y_ in zip(obj._host, host._host):
        assert same(x, y_)
    # both tables from the validation split, then the dense form: one forward, every cell stacked and with its interval
    stk, conf, fitted = st.fit_stacker_and_conformal(model, g, masker, folds=5)
    assert stk.coef.shape == (6, 150, 3) and conf.fitted
    rows = torch.tensor([0, 5, 5, 1833], device=DEV)
    point, lower, upper, raw, observed = st.impute_stacked(model, g, stk, fitted, conf, rows)
    assert point.shape == lower.shape == upper.shape == raw.shape == observed.shape == (4, 50)
    fin = torch.isfinite(lower) & torch.isfinite(upper)
    assert bool(fin.any()) and bool((lower[fin] <= point[fin]).all()) and bool((point[fin] <= upper[fin]).all())
    stacked, raw2, _ = st.impute_stacked(model, g, stk, fitted, None, rows)
    assert torch.equal(raw, raw2) and torch.equal(stacked[1], stacked[2])
    pp = stk.predict([raw.reshape(-1), fitted["per_lab_mean"][1].repeat(4)], torch.arange(50, device=DEV).repeat(4),
                     rows.repeat_interleave(50))
    assert torch.equal(stacked.reshape(-1), pp)


# ---------------------------------------------------------------------------------- refusals
def test_every_limit_is_refused_before_anything_is_enqueued():
    c = ref.make_case(n=100, K=2)
    d = dev_case(c)
    args = (d["target"], d["patient"], d["lab"], 5, d["deg"])
    with pytest.raises(ValueError, match="features"):
        so.stack_sums(d["feats"] * 3, *args, EDGES3)
    with pytest.raises(MmgError, match="folds"):
        so.stack_sums(d["feats"], *args, EDGES3, 9)
    with pytest.raises(MmgError, match="folds"):
        so.stack_sums(d["feats"], *args, EDGES3, 0)
    with pytest.raises(MmgError, match="labs"):
        so.stack_sums(d["feats"], d["target"], d["patient"], d["lab"], so.ST_MAX_LABS + 1, d["deg"], [0.0, 1.0])
    with pytest.raises(MmgError, match="cells"):
        so.stack_sums(d["feats"], d["target"], d["patient"], d["lab"], 2048, d["deg"], [float(j) for j in range(18)])
    with pytest.raises(MmgError, match="bins"):
        so.stack_sums(d["feats"], *args, [0.0])
    with pytest.raises(MmgError, match="ascending"):
        so.stack_sums(d["feats"], *args, [0.0, 6.0, 6.0])
    sums, _ = so.stack_sums(d["feats"], *args, EDGES3)
    for ridge in (-1.0, float("nan"), float("inf")):
        with pytest.raises(MmgError, match="ridge"):
            so.stack_solve(sums, 5, 3, 2, ridge, 0)
    with pytest.raises(MmgError, match="min_count"):
        so.stack_solve(sums, 5, 3, 2, 0.0, -1)
    coef, _, _ = so.stack_solve(sums, 5, 3, 2, 1e-3, 0)
    with pytest.raises(MmgError, match="folds >= 2"):
        so.stack_apply_pairs(d["feats"], d["patient"], d["lab"], 5, d["deg"], EDGES3, coef, 0, True)
    with pytest.raises(MmgError, match="ascending"):
        so.stack_scores(d["feats"][0], d["feats"][1], d["target"], d["patient"], d["lab"], 5, d["deg"], [3.0, 2.0])
    # a short and a missing workspace, straight through the C ABI
    lib = so.load()
    import ctypes as C_
    n = 100
    assert lib.mmg_stack_sums_ws_bytes(n, 5, 3, 2, 1) > 64 and lib.mmg_stack_solve_ws_bytes(5, 3, 2, 1) > 64
    assert lib.mmg_stack_scores_ws_bytes(n, 5, 3) > 64
    assert lib.mmg_stack_sums_ws_bytes(-1, 5, 3, 2, 1) == 0 and lib.mmg_stack_sums_ws_bytes(n, 5, 3, 5, 1) == 0
    assert lib.mmg_stack_sums_ws_bytes(2 ** 31, 5, 3, 2, 1) == 0 and lib.mmg_stack_solve_ws_bytes(2048, 17, 2, 1) == 0
    ws = torch.empty(64, dtype=torch.uint8, device=DEV)
    out = torch.zeros(15 * 10, dtype=torch.float64, device=DEV)
    dropped = torch.zeros(4, dtype=torch.int64, device=DEV)
    fp = (C_.c_void_p * 2)(d["feats"][0].data_ptr(), d["feats"][1].data_ptr())
    ed = (C_.c_double * 4)(*EDGES3)
    stream = torch.cuda.current_stream().cuda_stream
    for w, nbytes in ((ws.data_ptr(), 64), (None, 0)):
        rc = lib.mmg_stack_sums(fp, 2, d["target"].data_ptr(), d["patient"].data_ptr(), d["lab"].data_ptr(), 8, n, 5,
                                d["deg"].data_ptr(), 40, ed, 3, 1, 0, out.data_ptr(), dropped.data_ptr(), w, nbytes, stream)
        assert rc == mmgnn._lib.MMG_E_WS
    rc = lib.mmg_stack_sums(fp, 2, d["target"].data_ptr(), d["patient"].data_ptr(), d["lab"].data_ptr(), 8, 2 ** 31, 5,
                            d["deg"].data_ptr(), 40, ed, 3, 1, 0, out.data_ptr(), dropped.data_ptr(), ws.data_ptr(), 64, stream)
    assert rc == mmgnn._lib.MMG_E_ARG
    torch.cuda.synchronize()
    assert not out.any() and not dropped.any()
