"""Embedding maps on the MI355X (csrc/pca.hip, mmgnn/embed.py): the centred Gram matrix and the means against an 80-bit
evaluation, pca against the float64 restatement under embed_ref's BOUNDS, the 2-D histogram against numpy.histogram2d,
bitwise reproducibility (eager and replayed hipGraph), the end-to-end maps and the C-level refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import embed, ops
from mmgnn.model import build_model
from mmgnn.synth import make_graph
import embed_ref as er

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev_rows(x):
    """A host view with a padded row stride keeps that stride on the device."""
    base = x.base if x.base is not None and x.base.ndim == 2 else x
    return torch.from_numpy(np.ascontiguousarray(base)).to(DEV)[:, :x.shape[1]]


@pytest.mark.parametrize("n, D, ld", list(er.GRAM_CASES))
def test_centered_gram_and_means_against_80_bit(n, D, ld):
    xd = _dev_rows(er.gram_case_x(n, D, ld))
    assert xd.stride(0) == ld
    mean, gram = ops.centered_gram(xd)
    assert torch.equal(gram, gram.T.contiguous()), "S is not bit-exactly symmetric"
    dm, dg = er.distances(mean.cpu().numpy(), gram.cpu().numpy(), n, D, ld)
    bm, bg = er.gram_bounds(n, D, ld)
    print(f"({n}, {D}, ld {ld}): means {dm:.3e} (bound {bm:.3e}), Gram {dg:.3e} (bound {bg:.3e})")
    assert dm <= bm
    assert dg <= bg


@pytest.mark.parametrize("whiten", [False, True])
@pytest.mark.parametrize("k, sv", [(2, (8, 4, 2, 1)), (8, er.SV8)])
@pytest.mark.parametrize("n", [5000, 50])
def test_pca_against_the_restatement(n, k, sv, whiten):
    """make_case(n, 128) with the default spectrum for k = 2 and with eight planted values (embed_ref.SV8) for k = 8:
    with the default four, components 5 .. 8 lie in the noise and the gap assertion the bounds rest on cannot hold."""
    x = er.make_case(n, 128, seed=1, sv=sv)
    ref = er.pca_ref(x, k, whiten)
    res = embed.pca(torch.from_numpy(x).to(DEV), k, whiten)
    assert res.projection.is_cuda and res.projection.dtype == torch.float32 and res.projection.shape == (n, k)
    er.check_pca(res, ref, k, projection=res.projection.cpu().numpy())


def _points(gx, gy, seed=0, n=20000):
    rng = np.random.default_rng(seed)
    ex = np.linspace(-2.0, 2.0, gx + 1).astype(np.float32).astype(np.float64)      # edges an fp32 point can sit on
    ey = np.linspace(-1.5, 2.5, gy + 1).astype(np.float32).astype(np.float64)
    y = rng.normal(0.0, 1.2, (n, 2)).astype(np.float32)
    for axis, e in ((0, ex), (1, ey)):
        rows = slice(100 * axis, 100 * axis + 60)
        y[rows, axis] = rng.choice(e, 60).astype(np.float32)                       # on interior, first and last edges
        y[200 + 10 * axis, axis] = e[0]
        y[201 + 10 * axis, axis] = e[-1]
        y[202 + 10 * axis, axis] = e[-1] + 1.0                                     # outside
        y[203 + 10 * axis, axis] = np.nextafter(np.float32(e[0]), np.float32(-10))  # just below the first edge
        y[204 + 10 * axis, axis] = np.nan
    y[230] = (ex[0], ey[-1])
    y[231] = (ex[-1], ey[-1])
    w = rng.integers(0, 200, n).astype(np.int32)
    return y, ex, ey, w


@pytest.mark.parametrize("gx, gy", [(1, 1), (7, 5), (256, 256)])
def test_grid2d_equals_numpy_histogram2d(gx, gy):
    y, ex, ey, w = _points(gx, gy)
    yd, exd, eyd = torch.from_numpy(y).to(DEV), torch.from_numpy(ex).to(DEV), torch.from_numpy(ey).to(DEV)
    count, wsum = ops.grid2d(yd, exd, eyd, torch.from_numpy(w).to(DEV))
    want = er.hist2d_ref(y, ex, ey)
    assert 0 < want.sum() < y.shape[0]
    assert np.array_equal(count.cpu().numpy(), want)
    assert np.array_equal(wsum.cpu().numpy(), er.hist2d_ref(y, ex, ey, w))
    count2, none = ops.grid2d(yd, exd, eyd)
    assert none is None and np.array_equal(count2.cpu().numpy(), want)


def test_bitwise_reproducible_eager_and_replayed():
    x = torch.from_numpy(er.make_case(3001, 128, seed=5)).to(DEV)
    comps = torch.from_numpy(np.linalg.qr(np.random.default_rng(1).standard_normal((128, 8)))[0].T.copy()).to(DEV)
    scale = torch.linspace(0.5, 2.0, 8, dtype=torch.float64, device=DEV)
    y, ex, ey, w = _points(7, 5)
    yd, exd, eyd, wd = (torch.from_numpy(a).to(DEV) for a in (y, ex, ey, w))

    def gram_and_rows():
        mean, gram = ops.centered_gram(x)
        return mean, gram, ops.project_rows(x, mean, comps, scale)

    def bits(ts):
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in ts]

    ref, again = bits(gram_and_rows()), bits(gram_and_rows())
    for r, a in zip(ref, again):
        assert np.array_equal(r.view(np.uint8), a.view(np.uint8)), "two runs differ"
    g1, g2 = bits(ops.grid2d(yd, exd, eyd, wd)), bits(ops.grid2d(yd, exd, eyd, wd))
    assert all(np.array_equal(a, b) for a, b in zip(g1, g2))
    # captured and replayed twice: no memset node, no allocation, no host synchronisation inside the two entry points
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gram_and_rows()                                  # warm-up off the default stream, as torch.cuda.graph asks
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = gram_and_rows()
    for _ in range(2):
        for o in outs:
            o.fill_(-1.0)
        graph.replay()
        for r, o in zip(ref, bits(outs)):
            assert np.array_equal(r.view(np.uint8), o.view(np.uint8)), "a replayed capture differs from the eager run"


def test_embedding_maps_end_to_end(tmp_path):
    g = make_graph(1, seed=0).to(DEV)
    cfg = {"model": {"architecture": "RGCN", "hidden_dim": 64, "num_layers": 2, "dropout": 0.0,
                     "use_batch_norm": True, "activation": "relu"}}
    torch.manual_seed(0)
    model = build_model(cfg, (g.node_types, g.edge_types), None).to(DEV)
    model._init_embeddings(g)
    model.train()
    names = {i: n for i, n in enumerate(["pH", "PTT", "sodium"])}
    out = embed.embedding_maps(model, g, n_components=2, grid=16, output_dir=tmp_path, lab_names=names)
    assert model.training
    for f in ("lab_embeddings_pca.csv", "diagnosis_embeddings_pca.csv", "medication_embeddings_pca.csv",
              "pca_explained_variance.csv", "patient_embeddings_pca.npy", "patient_embedding_density.csv"):
        assert os.path.getsize(tmp_path / f) > 0, f
    assert list(out["lab"].columns) == ["idx", "name", "panel", "pc1", "pc2"]
    assert list(out["diagnosis"].columns) == ["idx", "name", "pc1", "pc2"]
    assert list(out["medication"].columns) == ["idx", "name", "pc1", "pc2"]
    assert list(out["lab"]["idx"]) == list(range(int(g["lab"].num_nodes))) and len(out["lab"]) == 50
    assert list(out["lab"]["panel"][:4]) == ["ABG", "Coag", "CMP", "Other"] and out["lab"]["name"][3] == "lab_3"
    assert list(out["variance"].columns) == embed.VARIANCE_COLUMNS and len(out["variance"]) == 8
    dens = out["density"]
    assert list(dens.columns) == embed.DENSITY_COLUMNS and len(dens) == 256
    assert int(dens["count"].sum()) == 1834
    ex, ey = out["edges"]
    assert ex.dtype == np.float64 and ex.size == 17 and ey.size == 17
    # the patient projection against the restatement of encode_nodes' output
    model.eval()
    with torch.no_grad():
        xp = model.encode_nodes(g)["patient"].float().cpu().numpy()
    ref = er.pca_ref(xp, 2)
    print(f"eigenvalues of the patient embeddings (seed 0): {ref['eigenvalues'][:3]}")
    er.assert_gaps(ref["eigenvalues"], 2)                            # the seed is fixed: this case has the gaps
    p = out["patient"].cpu().numpy()
    assert out["patient"].is_cuda and p.shape == (1834, 2)
    d = float((np.abs(p - ref["projection"]) / np.abs(ref["projection"]).max(axis=0)).max())
    print(f"patient projection {d:.3e} (of {er.PROJ_REL:.3e}); eigenvalues {ref['eigenvalues'][:3]}")
    assert d <= er.PROJ_REL
    assert np.array_equal(np.load(tmp_path / "patient_embeddings_pca.npy"), p)
    # the grid is numpy.histogram2d of that projection over the returned edges, the degree its weight
    deg = np.bincount(g["patient", "has_lab", "lab"].edge_index[0].cpu().numpy(), minlength=1834)
    count = dens["count"].to_numpy().reshape(16, 16)
    assert np.array_equal(count, er.hist2d_ref(p, ex, ey))
    ws = er.hist2d_ref(p, ex, ey, deg).reshape(-1)
    c = dens["count"].to_numpy()
    assert np.allclose(dens["mean_degree"].to_numpy()[c > 0], ws[c > 0] / c[c > 0], rtol=1e-15, atol=0)
    assert np.all(np.isnan(dens["mean_degree"].to_numpy()[c == 0]))
    # the final space runs too
    fin = embed.embedding_maps(model, g, space="final", grid=8)
    assert fin["patient"].shape == (1834, 2) and int(fin["density"]["count"].sum()) == 1834


def test_argument_and_workspace_refusals():
    from mmgnn import _lib
    lib = _lib.load()
    x = torch.zeros(64, 264, device=DEV)
    o = torch.zeros(64, 16, device=DEV)
    d = torch.zeros(264 * 264, dtype=torch.float64, device=DEV)
    i64 = torch.zeros(258 * 258, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                      # noqa: E731
    ws = ops.workspace(lib.mmg_centered_gram_ws_bytes(64, 256), DEV)
    st = ops._stream()
    for D in (260, 6):
        assert lib.mmg_centered_gram(p(x), 64, D, 264, p(d), p(d), p(ws), ws.numel(), st) == -1
        assert f"D {D}".encode() in lib.mmg_last_error()
        assert lib.mmg_project_rows(p(x), 64, D, 264, p(d), p(d), None, 2, p(o), 16, None, 0, st) == -1
        assert f"D {D}".encode() in lib.mmg_last_error()
    assert lib.mmg_project_rows(p(x), 64, 256, 264, p(d), p(d), None, 9, p(o), 16, None, 0, st) == -1
    assert b"k 9" in lib.mmg_last_error()
    need = lib.mmg_centered_gram_ws_bytes(64, 256)
    assert lib.mmg_centered_gram(p(x), 64, 256, 264, p(d), p(d), p(ws), need - 1, st) == -3
    assert b"workspace" in lib.mmg_last_error() and b"centered_gram" in lib.mmg_last_error()
    assert lib.mmg_grid2d(p(o), 16, None, 64, p(d), p(d), 257, 4, p(i64), None, None, 0, st) == -1
    assert b"257" in lib.mmg_last_error()
    torch.cuda.synchronize()
    # and through the Python layer
    with pytest.raises(ValueError, match="multiple of 4"):
        embed.pca(x[:, :260], 2)
    with pytest.raises(ValueError, match="multiple of 4"):
        embed.pca(x[:, :6], 2)
    with pytest.raises(ValueError, match="device limit of 8"):
        embed.pca(x[:, :128], 9)
