"""CPU-side checks (no GPU): the C-ABI library loads and exports every symbol include/mmgnn.h
declares; the host mirror refuses to run without the HIP path; container + state_dict plumbing."""
import ctypes
import os
import re

import pytest
import torch

from oracle import fixtures as fx

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = {"model": {"architecture": "RGCN", "hidden_dim": 64, "num_layers": 2, "dropout": 0.0,
                 "use_batch_norm": True, "activation": "relu"}}


def header_symbols():
    txt = open(os.path.join(REPO, "include", "mmgnn.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mmg_[a-z0-9_]+)\s*\(", txt)))


def test_library_loads_and_exports_every_declared_symbol():
    import mmgnn  # noqa: F401
    from mmgnn import _lib
    lib = _lib.load()
    syms = header_symbols()
    assert len(syms) >= 20
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(raw, s), f"{s} declared in include/mmgnn.h but not exported"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes prototype in _lib.SIGNATURES"
    assert sorted(_lib.SIGNATURES) == syms
    assert lib.mmg_version() >= 100


def test_argument_errors_are_reported_without_a_gpu():
    import mmgnn  # noqa: F401
    from mmgnn import _lib
    lib = _lib.load()
    # bad D is rejected on the host side before any launch
    rc = lib.mmg_l2norm_fwd(None, None, None, 4, 100, 1e-12, None)
    assert rc == -1 and b"unsupported" in lib.mmg_last_error()
    rc = lib.mmg_csr_build(None, 10, 4, 2, None, None, None, None, 0, None)
    assert rc == -1
    assert lib.mmg_csr_build_ws_bytes(1000, 100) > 3 * 4000
    # the BatchNorm / L2-norm backward GEMM: the shape rules of every mode live in one query ...
    BN, L2, BN2, ROWS = 0, 1, 2, 3
    sup = lib.mmg_linear_bnbwd_supported
    assert sup(BN, 600, 64, 64, 0) and sup(L2, 600, 128, 64, 0) and sup(BN2, 600, 128, 128, 0) and sup(ROWS, 513, 128, 128, 1)
    assert not sup(BN, 512, 128, 128, 0) and not sup(BN2, 600, 64, 128, 0) and not sup(ROWS, 600, 128, 64, 0)
    assert not sup(BN, 600, 64, 128, 1) and not sup(L2, 600, 128, 256, 0) and not sup(4, 600, 128, 128, 0)
    # ... and the entry point refuses a bad descriptor on the host side (the buffers are never touched)
    fake = ctypes.c_void_p(256)
    pro = _lib.PrologueT()

    def bnbwd(mode, M=1000, N=128, K=128, nxt=None, **fields):
        d = _lib.BnBwdT(mode, fake, fake, fake, 0, fake, ctypes.pointer(pro), ctypes.pointer(pro), fake, fake, None, 1.0,
                        None, None, fake, 1e-12)
        for k, v in fields.items():
            setattr(d, k, v)
        rc = lib.mmg_linear_bnbwd(ctypes.byref(d), fake, fake, fake, M, N, K, nxt, None, None)
        return rc, lib.mmg_last_error()

    assert lib.mmg_linear_bnbwd(None, fake, fake, fake, 1000, 128, 128, None, None, None) == -1
    assert b"null descriptor" in lib.mmg_last_error()
    for mode in (-1, 4):
        rc, msg = bnbwd(mode)
        assert rc == -1 and b"unknown mode" in msg
    rc, msg = bnbwd(BN2, nxt=ctypes.byref(_lib.NextBnT()))
    assert rc == -1 and b"next-BatchNorm" in msg
    for mode, M, N, K in ((BN, 512, 128, 128), (L2, 1000, 256, 128), (BN2, 1000, 64, 128), (ROWS, 1000, 128, 64)):
        rc, msg = bnbwd(mode, M, N, K)
        assert rc == -1 and b"unsupported" in msg
    for mode, field in ((BN, "G"), (BN, "y"), (L2, "rnorm"), (BN2, "G2"), (BN2, "pro2"), (ROWS, "row_pos"), (ROWS, "pro")):
        rc, msg = bnbwd(mode, **{field: None})
        assert rc == -1 and b"null buffer" in msg, (mode, field)
    rc, msg = bnbwd(ROWS, G=None, n_sel=5)
    assert rc == -1 and b"bad row list" in msg


def test_forward_epilogue_rejections_without_a_gpu():
    """mmg_linear_fwd / mmg_gather_rows refuse a bad mmg_fwd_epi_t on the host side (the fake buffers are never touched)."""
    import mmgnn  # noqa: F401
    from mmgnn import _lib
    lib = _lib.load()
    NONE, STATS, NEXT_BN, L2 = 0, 1, 2, 3
    sup = lib.mmg_linear_fwd_supported
    for mode in (NONE, STATS, NEXT_BN):
        assert sup(mode, 0, 64, 64) and sup(mode, 8, 4096, 256) and sup(mode, 600, 192, 128)
        assert not sup(mode, -1, 64, 64) and not sup(mode, 8, 48, 64) and not sup(mode, 8, 4160, 64) and not sup(mode, 8, 64, 96)
    assert sup(L2, 513, 64, 64) and sup(L2, 600, 128, 128) and sup(L2, 600, 64, 128)
    assert not sup(L2, 512, 128, 128) and not sup(L2, 600, 256, 128) and not sup(L2, 600, 128, 256)
    assert not sup(-1, 600, 128, 128) and not sup(4, 600, 128, 128)
    fake = ctypes.c_void_p(256)
    M, N = 1000, 128
    need = lib.mmg_epi_ws_bytes(M, N)
    assert need >= lib.mmg_col_reduce2_ws_bytes(M, N) and need >= 768 * 2 * N * 8
    pro = _lib.PrologueT()
    nxt = _lib.NextBnT(fake, ctypes.pointer(pro), fake, fake, fake, 0, fake, need)
    rels = (_lib.RelT * 1)(_lib.RelT(fake, fake, None, None, fake, None, 50, 1, None, fake))

    def epi(mode, **fields):
        e = _lib.FwdEpiT(mode, fake, None, fake, need, None, fake, 1e-12)
        if mode == NEXT_BN:
            e.col_sums, e.next = None, ctypes.pointer(nxt)
        for k, v in fields.items():
            setattr(e, k, v)
        return e

    def linear(e, M=M, N=N, K=128, flags=0, X=fake):
        rc = lib.mmg_linear_fwd(X, None, fake, None, fake, M, N, K, flags, ctypes.byref(e) if e is not None else None, None)
        return rc, lib.mmg_last_error()

    def gather(e, n_rows=M, D=N):
        rc = lib.mmg_gather_rows(rels, 1, n_rows, D, fake, 0, ctypes.byref(e), None)
        return rc, lib.mmg_last_error()

    # NULL is the producer alone: the call gets as far as its own buffers
    rc, msg = linear(None, X=None)
    assert rc == -1 and b"null buffer" in msg
    for call in (linear, gather):
        for mode in (-1, 4):
            rc, msg = call(epi(mode))
            assert rc == -1 and b"unknown epilogue mode" in msg, call
        for mode, field in ((STATS, "col_sums"), (NEXT_BN, "next"), (L2, "rnorm")):
            if call is gather and mode == L2:
                continue
            rc, msg = call(epi(mode, **{field: None}))
            assert rc == -1 and b"null field" in msg, (call, mode)
        rc, msg = call(epi(STATS, ws_bytes=need - 1))
        assert rc == -1 and b"workspace" in msg
        rc, msg = call(epi(STATS, ws=None))
        assert rc == -1 and b"workspace" in msg
        short = _lib.NextBnT(fake, ctypes.pointer(pro), fake, fake, fake, 0, fake, need - 1)
        rc, msg = call(epi(NEXT_BN, next=ctypes.pointer(short)))
        assert rc == -1 and b"workspace" in msg
        rc, msg = call(epi(STATS, next=ctypes.pointer(nxt)))
        assert rc == -1 and b"exclusive" in msg
        for bad in (dict(count=0), dict(scale=None), dict(shift=None)):
            f = _lib.BnFinT(M, None, None, None, None, 1, 0.1, 1e-5, fake, fake, None, None)
            for k, v in bad.items():
                setattr(f, k, v)
            rc, msg = call(epi(STATS, fin=ctypes.pointer(f)))
            assert rc == -1 and b"BatchNorm fold" in msg, bad
    rc, msg = linear(epi(STATS), M=0)
    assert rc == -1 and b"empty" in msg
    rc, msg = gather(epi(STATS), n_rows=0)
    assert rc == -1 and b"empty" in msg
    # L2: the linear's only, at its shapes, without flags
    for M_, N_, K_ in ((512, 128, 128), (1000, 256, 128), (1000, 128, 256)):
        rc, msg = linear(epi(L2), M=M_, N=N_, K=K_)
        assert rc == -1 and b"unsupported" in msg
    rc, msg = linear(epi(L2), flags=1)
    assert rc == -1 and b"no flags" in msg
    rc, msg = gather(epi(L2))
    assert rc == -1 and b"L2" in msg
    # the plain shape rules keep their wording
    rc, msg = linear(epi(STATS), K=96)
    assert rc == -1 and b"K=96 unsupported" in msg
    rc, msg = linear(None, N=48)
    assert rc == -1 and b"multiple of 64" in msg


def test_short_workspace_is_refused_the_same_way_everywhere():
    """Every entry point that answers MMG_E_WS, with otherwise valid arguments: one byte short of its *_ws_bytes is -3, and
    the message names the entry point and the workspace.  The ones whose workspace check also covers a null `ws` refuse
    that the same way.  The fake buffers are never touched: the refusal comes before any HIP call."""
    import mmgnn  # noqa: F401
    from mmgnn import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    pro = _lib.PrologueT()
    pct = _lib.PercentileT(0, 1, 0.5)
    ranks = (ctypes.c_int64 * 1)(3)
    edges = (ctypes.c_double * 3)(0.0, 1.0, 2.0)
    cnt = ctypes.c_int64(0)
    rels = (_lib.RelT * 1)(_lib.RelT(p, p, None, None, p, p, 50, 1, None, p))
    bn = _lib.BnBwdT(0, p, None, None, 0, p, ctypes.pointer(pro), None, p, p, None, 1.0, None, None, None, 1e-12)
    assert lib.mmg_linear_bnbwd_supported(0, 1000, 128, 128, 1)

    def bnbwd(ws, nb):
        wg = _lib.BnBwdWgradT(p, None, p, None, 0, ws, nb, None)
        return lib.mmg_linear_bnbwd(ctypes.byref(bn), p, None, p, 1000, 128, 128, None, ctypes.byref(wg), None)

    # (name in the message, bytes needed, call(ws, ws_bytes), null ws is a workspace refusal too)
    table = [
        ("csr_build", lib.mmg_csr_build_ws_bytes(5000, 100),
         lambda ws, nb: lib.mmg_csr_build(p, 5000, 100, 0, p, p, p, ws, nb, None), False),
        ("scatter_rows", lib.mmg_scatter_rows_ws_bytes(rels, 1, 1000, 128),
         lambda ws, nb: lib.mmg_scatter_rows(rels, 1, 1000, 128, p, ws, nb, None), False),
        ("linear_wgrad", lib.mmg_linear_wgrad_ws_bytes(1000, 128, 128),
         lambda ws, nb: lib.mmg_linear_wgrad(p, p, None, p, None, 1000, 128, 128, 0, ws, nb, None), False),
        ("linear_wgrad", lib.mmg_linear_wgrad_ws_bytes(1000, 128, 128),
         lambda ws, nb: lib.mmg_linear_wgrad_deferred(p, p, None, p, None, 1000, 128, 128, 0, ws, nb, None,
                                                      ctypes.byref(_lib.WgradReduceT())), False),
        ("linear_bnbwd", lib.mmg_linear_bnbwd_wgrad_ws_bytes(1000, 128, 128), bnbwd, False),
        ("col_reduce2", lib.mmg_col_reduce2_ws_bytes(1000, 128),
         lambda ws, nb: lib.mmg_col_reduce2(p, p, p, 1000, 128, ws, nb, None), False),
        ("bn_bwd_stats", lib.mmg_col_reduce2_ws_bytes(1000, 128),
         lambda ws, nb: lib.mmg_bn_bwd_stats(p, p, ctypes.byref(pro), p, p, p, 1000, 128, ws, nb, None), False),
        ("bn_bwd_stats2", lib.mmg_col_reduce2_ws_bytes(1000, 128),
         lambda ws, nb: lib.mmg_bn_bwd_stats2(p, p, p, ctypes.byref(pro), ctypes.byref(pro), p, p, p, 1000, 128, ws, nb,
                                              None), False),
        ("sup_mask_draw", lib.mmg_sup_mask_ws_bytes(1000),
         lambda ws, nb: lib.mmg_sup_mask_draw(None, 1, p, 1000, 0.2, p, p, p, ws, nb, None), False),
        ("pair_loss", lib.mmg_pair_loss_ws_bytes(1000),
         lambda ws, nb: lib.mmg_pair_loss(p, p, None, None, 1000, 1.0, None, 0, p, p, ws, nb, None), False),
        ("knn_impute", lib.mmg_knn_impute_ws_bytes(100, 50, 10, 5),
         lambda ws, nb: lib.mmg_knn_impute(p, 100, 50, 50, p, 10, 5, 0, p, 50, ws, nb, None), True),
        ("order_stats", lib.mmg_order_stats_ws_bytes(10),
         lambda ws, nb: lib.mmg_order_stats(p, None, 10, ranks, 1, p, p, ws, nb, None), True),
        ("robust_sums", lib.mmg_robust_sums_ws_bytes(10),
         lambda ws, nb: lib.mmg_robust_sums(p, p, 10, p, 2, p, pct, pct, pct, p, ws, nb, None), True),
        ("split_membership", lib.mmg_split_membership_ws_bytes(100),
         lambda ws, nb: lib.mmg_split_membership(p, p, p, p, 10, 100, p, ws, nb, None), True),
        ("prep_sort", lib.mmg_prep_sort_ws_bytes(10),
         lambda ws, nb: lib.mmg_prep_sort(p, p, p, 0, 10, 4, 2, None, p, p, None, ws, nb, None), True),
        ("lab_stats", lib.mmg_lab_stats_ws_bytes(2),
         lambda ws, nb: lib.mmg_lab_stats(p, p, 10, 4, 2, p, ws, nb, None), True),
        ("lab_quantiles", lib.mmg_lab_quantiles_ws_bytes(2),
         lambda ws, nb: lib.mmg_lab_quantiles(p, p, 10, 4, 2, p, ws, nb, None), True),
        ("lab_aggregate", lib.mmg_lab_aggregate_ws_bytes(10),
         lambda ws, nb: lib.mmg_lab_aggregate(p, p, 10, 4, 2, 0, 0, 5.0, None, p, p, p, ctypes.byref(cnt), ws, nb, None),
         True),
        ("pair_analysis", lib.mmg_pair_analysis_ws_bytes(8, 10, 2),
         lambda ws, nb: lib.mmg_pair_analysis(p, p, p, p, 4, 8, 10, p, 4, edges, 2, p, p, ws, nb, None), True),
        ("pair_calibrated_abs", lib.mmg_pair_calibrated_abs_ws_bytes(8, 10, 2),
         lambda ws, nb: lib.mmg_pair_calibrated_abs(p, p, p, p, 4, 8, 10, p, p, p, 4, edges, 2, p, p, p, ws, nb, None),
         True),
    ]
    for name, need, call, null_too in table:
        assert need > 0, name
        for ws, nb in [(p, need - 1)] + ([(None, need)] if null_too else []):
            rc = call(ws, nb)
            msg = lib.mmg_last_error()
            assert rc == -3 and name.encode() in msg and b"workspace" in msg, (name, ws, rc, msg)


def test_cpu_model_fails_loudly():
    import mmgnn  # noqa: F401
    from mmgnn.model import build_model
    g = fx.graph_from_frames(fx.det_frames(60, 9, 11, 8))
    model = build_model(CFG, (g.node_types, g.edge_types), None)
    model._init_embeddings(g)
    with pytest.raises(Exception, match="HIP device|no CPU fallback"):
        model(g)
    from mmgnn import ops
    with pytest.raises(Exception, match="HIP device"):
        ops.linear_fwd(torch.zeros(4, 64), torch.zeros(64, 64))


def test_param_count_and_state_dict_layout():
    import mmgnn  # noqa: F401
    from mmgnn.model import build_model
    cfg = {"model": dict(CFG["model"], hidden_dim=128)}
    m = build_model(cfg, (fx.NODE_TYPES, fx.EDGE_TYPES), None)
    assert sum(p.numel() for p in m.parameters()) == 483970          # README.md:197 of the reference
    assert len(m.embeddings) == 0                                    # lazy (model.py:86-89)
    g = fx.graph_from_frames(fx.det_frames(1834, 50, 114, 100))
    m._init_embeddings(g)
    assert sum(p.numel() for p in m.parameters()) == 752514
    sd = fx.det_state({t: g[t].num_nodes for t in g.node_types}, 128)
    assert sorted(m.state_dict().keys()) == sorted(sd.keys())
    m.load_state_dict(sd)
    # PyG 2.3 key mangling 'src__rel__dst' is accepted too
    old = {}
    for k, v in sd.items():
        mt = re.match(r"(convs\.\d+\.convs\.)<(.+)>(\..+)", k)
        old[(mt.group(1) + mt.group(2).replace("___", "__") + mt.group(3)) if mt else k] = v
    assert any("patient__has_lab__lab" in k for k in old)
    m.load_state_dict(old)


def test_unknown_config_values_raise_like_the_reference():
    import mmgnn  # noqa: F401
    from mmgnn.model import build_model, compute_regression_loss
    with pytest.raises(ValueError, match="Unknown activation"):
        build_model({"model": dict(CFG["model"], activation="gelu")}, (fx.NODE_TYPES, fx.EDGE_TYPES), None)
    with pytest.raises(ValueError, match="Unknown architecture"):
        build_model({"model": dict(CFG["model"], architecture="GAT")}, (fx.NODE_TYPES, fx.EDGE_TYPES), None)
    with pytest.raises(ValueError, match="Unknown loss type"):
        compute_regression_loss(torch.zeros(3), torch.zeros(3), "l3")
    a, b = torch.tensor([1.0, 2.0, 4.0]), torch.tensor([0.0, 2.0, 2.0])
    assert float(compute_regression_loss(a, b, "mae")) == pytest.approx(1.0)
    assert float(compute_regression_loss(a, b, "mse")) == pytest.approx(5.0 / 3)


def test_hetero_graph_container_protocol():
    import mmgnn  # noqa: F401
    from mmgnn.data import HeteroGraph
    g = HeteroGraph()
    g["patient"].num_nodes = 3
    g["lab"].num_nodes = 2
    ei = torch.tensor([[0, 1, 2], [1, 0, 1]])
    g["patient", "has_lab", "lab"].edge_index = ei
    g["patient", "has_lab", "lab"].edge_attr = torch.ones(3, 1)
    g["lab", "has_lab_rev", "patient"].edge_index = ei.flip(0)
    g.indexers = {"x": 1}
    assert g.node_types == ["patient", "lab"]
    assert g.edge_types == [("patient", "has_lab", "lab"), ("lab", "has_lab_rev", "patient")]
    assert g.metadata() == (g.node_types, g.edge_types)
    assert set(g.edge_index_dict) == set(g.edge_types)
    assert g[("patient", "has_lab", "lab")].edge_attr.shape == (3, 1) and g.indexers == {"x": 1}
    assert g.to("cpu") is g


@pytest.mark.parametrize("E", [10, 61484])
def test_edge_masker_splits_match_the_reference(E):
    """mmgnn.train.EdgeMasker (train.py:37-176) on a CPU graph: the 70/15/15 masks are the ones the REFERENCE's EdgeMasker
    produced for seed 42 (tests/golden/splits.npz), the supervision mask follows the injected generator, and the masker
    follows the graph when Trainer moves it (EdgeMasker.to)."""
    import mmgnn  # noqa: F401
    from mmgnn.data import HeteroGraph
    from mmgnn.train import EdgeMasker
    from golden_io import load, unpack_mask
    gold, _ = load("splits.npz")
    g = HeteroGraph()
    g["patient"].num_nodes = E
    g["lab"].num_nodes = 3
    ei = torch.stack([torch.arange(E), torch.arange(E) % 3])
    g["patient", "has_lab", "lab"].edge_index = ei
    g["patient", "has_lab", "lab"].edge_attr = torch.arange(E, dtype=torch.float32).unsqueeze(-1)
    m = EdgeMasker(g, 0.7, 0.15, 0.15, mask_fraction=0.2, seed=42, mask_generator=torch.Generator().manual_seed(9))
    for nm, mask in zip(("train", "val", "test"), (m.train_mask, m.val_mask, m.test_mask)):
        assert torch.equal(mask, unpack_mask(gold[f"E{E}/{nm}"], E))
    if E == 61484:
        assert [int(x.sum()) for x in (m.train_mask, m.val_mask, m.test_mask)] == [43038, 9222, 9224]
    idx, val, mask, sup = m.get_masked_data("train")
    n_tr = int(m.train_mask.sum())
    assert idx.shape == (2, n_tr) and val.shape == (n_tr,) and sup.shape == (n_tr,) and torch.equal(mask, m.train_mask)
    assert torch.equal(sup, torch.rand(n_tr, generator=torch.Generator().manual_seed(9)) < 0.2)
    assert m.get_masked_data("train")[0] is idx                       # one tensor object per split (pair-cache key)
    assert bool(m.get_masked_data("val")[3].all())
    with pytest.raises(ValueError, match="Unknown split"):
        m.get_masked_data("dev")
    with pytest.raises(AssertionError):
        EdgeMasker(g, 0.7, 0.2, 0.2)
    m.to(g, "cpu")
    assert m._cache == {} and m.edge_index is g["patient", "has_lab", "lab"].edge_index


def test_strided_job_views_of_vec_sums():
    """Host side of mmg_vec_sums' 2-D jobs: a contiguous tensor is a flat vector, a column slice of a wider matrix is
    (columns, row stride), anything else is refused (no silent copy)."""
    import mmgnn  # noqa: F401
    from mmgnn import ops
    w = torch.zeros(6, 10)
    assert ops._rows_view(w) == (0, 0) and ops._rows_view(w[2]) == (0, 0)
    assert ops._rows_view(w[:, :4]) == (4, 10) and ops._rows_view(w[:, 4:]) == (6, 10)
    with pytest.raises(ValueError):
        ops._rows_view(w.t())
    with pytest.raises(ValueError):
        ops._rows_view(w[:, ::2])


def test_deferred_weight_gradient_jobs_keep_their_order(monkeypatch):
    """wgrad_reduce_flush: jobs of different gradients share a launch; a second contribution to a gradient that an earlier
    job of the list writes waits for a later launch (and so does everything behind it for that gradient); jobs without
    slabs (small direct launches) are dropped; at most 16 jobs per launch."""
    import mmgnn  # noqa: F401
    from mmgnn import _lib, ops
    from mmgnn._lib import WgradReduceT
    calls = []

    class FakeLib:
        def mmg_wgrad_reduce_group(self, arr, n, stream):
            calls.append([(arr[i].dW, arr[i].accumulate) for i in range(n)])
            return 0

    monkeypatch.setattr(_lib, "load", lambda: FakeLib())
    monkeypatch.setattr(ops, "_stream", lambda: None)

    def job(dW, acc, slab=1):
        return (WgradReduceT(slab, 4, 2, dW, None, 4, acc), None, None, None)

    jobs = [job(100, 0), job(200, 0), job(100, 1), job(300, 0, slab=None), job(100, 1), job(400, 0)]
    ops.wgrad_reduce_flush(jobs)
    assert jobs == []
    assert calls == [[(100, 0), (200, 0), (400, 0)], [(100, 1)], [(100, 1)]]
    calls.clear()
    many = [job(1000 + i, 0) for i in range(20)]
    ops.wgrad_reduce_flush(many)
    assert [len(c) for c in calls] == [16, 4]


def test_vec_sums_refuses_two_jobs_with_one_destination():
    """The jobs of one mmg_vec_sums launch run concurrently: a shared destination would lose a contribution.  Checked on
    the host before any launch (as mmg_wgrad_reduce_group does for its gradients)."""
    import ctypes as C
    import mmgnn  # noqa: F401
    from mmgnn import _lib
    from mmgnn._lib import SumJobT
    lib = _lib.load()
    arr = (SumJobT * 2)()
    for j in range(2):
        src = (C.c_void_p * 4)(0x2000 + 0x100 * j, None, None, None)
        arr[j] = SumJobT(0x1000, src, 1, 8, 0, 0, (C.c_int * 4)(0, 0, 0, 0))
    assert lib.mmg_vec_sums(arr, 2, None) == -1 and b"share a destination" in lib.mmg_last_error()


def test_flush_grad_sums_chains_more_than_three_contributions(monkeypatch):
    """_Run.flush_grad_sums with 5 contributions to one parameter: sums go to NEW tensors (the first contribution may be
    shared by other names or belong to the caller), 3 further sources per job, and the second job -- which reads the
    first one's result -- is a later launch."""
    import mmgnn  # noqa: F401
    from mmgnn import model as mm, ops
    launches = []
    monkeypatch.setattr(ops, "wgrad_reduce_flush", lambda jobs: None)

    def fake_vec_sums(jobs):
        launches.append(len(jobs))
        for dst, srcs in jobs:
            acc = srcs[0].clone()
            for s_ in srcs[1:]:
                acc = acc + s_
            dst.copy_(acc)

    monkeypatch.setattr(ops, "vec_sums", fake_vec_sums)
    run = object.__new__(mm._Run)
    run.grads, run.pending, run.partial, run.wgrad_jobs = {}, {}, set(), []
    parts = [torch.full((4, 3), float(i + 1)) for i in range(5)]
    shared = torch.full((2,), 10.0)
    for p_ in parts:
        run.acc("w", p_)
    run.acc("a", shared); run.acc("b", shared); run.acc("b", torch.ones(2))
    run.flush_grad_sums()
    assert torch.equal(run.grads["w"], torch.full((4, 3), 15.0))
    assert torch.equal(parts[0], torch.full((4, 3), 1.0))                   # the first contribution is not overwritten
    assert torch.equal(run.grads["b"], torch.full((2,), 11.0)) and torch.equal(run.grads["a"], torch.full((2,), 10.0))
    assert run.grads["a"] is shared and launches == [2, 1] and run.pending == {}
