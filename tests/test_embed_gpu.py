"""Embedding maps on the MI355X (csrc/pca.hip, mmgnn/embed.py): the centred Gram matrix and the means against an 80-bit
evaluation (slabs at and above their minimum length, ragged last 64-blocks, non-finite input), the row projection
through the C ABI against an 80-bit evaluation under a derived bound, pca against the float64 restatement under
embed_ref's BOUNDS, the 2-D histogram against numpy.histogram2d (two passes of the grid loop, signed and 64-bit weight
sums, row stride 8, non-uniform and repeated edges, +-inf and -0.0), bitwise reproducibility (eager and replayed
hipGraph), the end-to-end maps and the C-level refusals."""
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


def _second_slab_at(D):
    """The first n at which the Gram of D columns takes a second slab, read off the workspace size (the means' slabs are
    256 rows and longer)."""
    from mmgnn import _lib
    ws = _lib.load().mmg_centered_gram_ws_bytes
    n = 2
    while ws(n + 1, D) == ws(2, D):
        n += 1
    assert n % 32 == 0 and n < 256, "a slab is whole chunks, and shorter than the means' first slab"
    return n + 1


@pytest.mark.parametrize("D, n", [(68, 64), (68, 65), (132, None)])
def test_lattice_gram_equals_the_loop_reference(D, n):
    """Multiples of 1/8 (assoc_ref.make_matrix) whose column means are exact: one slab of 64 = 2^6 rows, whose means are
    multiples of 1/512, and -- 65 rows, a second slab of one row; 132 columns, three blocks with a ragged last one, a
    slab and a row -- a last row chosen so that every mean IS the lattice centre.  Every difference, product and sum is
    then exact in fp64 in any order, so the mean and S EQUAL the loop reference, S about the device's returned mean."""
    import math
    import assoc_ref
    n = n or _second_slab_at(D)
    x = assoc_ref.make_matrix(n, D, seed=D + n, density=1.0, lattice=True, special=False)
    assert np.all(np.isfinite(x))
    if n == 64:
        want_mean = x.astype(np.float64).sum(axis=0) / n
    else:
        assert n == _second_slab_at(D) == 65
        want_mean = assoc_ref.lattice_center(D, D + n)
        x[-1] = (n * want_mean - x[:-1].astype(np.float64).sum(axis=0)).astype(np.float32)
        assert np.array_equal(x.astype(np.float64).sum(axis=0), n * want_mean) and np.abs(x).max() < 256
    mean, gram = ops.centered_gram(torch.from_numpy(x).to(DEV))
    mean, gram = mean.cpu().numpy(), gram.cpu().numpy()
    assert np.array_equal(mean, want_mean)
    u = x.astype(np.float64) - mean[None, :]
    want = np.zeros((D, D))
    for a in range(D):
        for b in range(a, D):
            want[a, b] = want[b, a] = math.fsum((u[:, a] * u[:, b]).tolist())
    assert np.array_equal(gram, want), float(np.abs(gram - want).max())


def test_non_finite_input_stays_in_its_own_row_and_column():
    """A NaN in column 5 and an inf in column 66 of the (300, 68, 72) case (the second 64-block is 4 columns wide): the
    two columns' means, and rows and columns 5 and 66 of S, are non-finite; every other entry is what the case gives
    with the two columns removed, under the clean case's bounds.  A wrong C/D lane map spreads the NaN over other
    rows, so this catches one without any tolerance."""
    n, D, ld = 300, 68, 72
    x = er.gram_case_x(n, D, ld)
    x[17, 5] = np.nan
    x[40, 66] = np.inf
    mean, gram = ops.centered_gram(_dev_rows(x))
    assert np.array_equal(gram.cpu().numpy().view(np.int64), gram.T.contiguous().cpu().numpy().view(np.int64)), \
        "S is not bit-exactly symmetric"
    mean, gram = mean.cpu().numpy(), gram.cpu().numpy()
    assert np.isnan(mean[5]) and np.all(np.isnan(gram[5, :])) and np.all(np.isnan(gram[:, 5]))
    assert mean[66] == np.inf and not np.any(np.isfinite(gram[66, :])) and not np.any(np.isfinite(gram[:, 66]))
    keep = np.array([c for c in range(D) if c not in (5, 66)])
    assert np.all(np.isfinite(mean[keep])) and np.all(np.isfinite(gram[np.ix_(keep, keep)]))
    dm, dg = er.distances_from(mean[keep], gram[np.ix_(keep, keep)], er.gram80_of(x[:, keep]))
    bm, bg = er.gram_bounds(n, D, ld)
    print(f"({n}, {D}, ld {ld}) without columns 5 and 66: means {dm:.3e} (bound {bm:.3e}), Gram {dg:.3e} (bound {bg:.3e})")
    assert dm <= bm
    assert dg <= bg


@pytest.mark.parametrize("n, D, k", er.PROJECT_CASES)
def test_project_rows_against_80_bit(n, D, k):
    """mmg_project_rows through the C entry point: out is an [n, 16] buffer of a sentinel (ld_out = 16 > k), the rows
    dense and with a padded stride (the padding holds 1e6), with and without a scale, general components; the bound is
    embed_ref.project_ratio's."""
    from mmgnn import _lib
    lib = _lib.load()
    case = er.project_case(n, D, k)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                      # noqa: E731
    mean, comps, scale = (torch.from_numpy(case[a].copy()).to(DEV) for a in ("mean", "comps", "scale"))
    sentinel = -12345.0
    for ld in (D, D + 8):
        buf = np.full((n, ld), 1e6, np.float32)
        buf[:, :D] = case["x"]
        xd = torch.from_numpy(buf).to(DEV)
        for scaled in (False, True):
            out = torch.full((n, 16), sentinel, device=DEV)
            rc = lib.mmg_project_rows(p(xd), n, D, ld, p(mean), p(comps), p(scale) if scaled else None, k, p(out), 16,
                                      None, 0, ops._stream())
            assert rc == 0, lib.mmg_last_error()
            o = out.cpu().numpy()
            assert np.all(o[:, k:] == np.float32(sentinel)), "columns k .. 15 of out were written"
            ratio = er.project_ratio(o[:, :k], case, D, scaled)
            print(f"({n}, {D}, k {k}) ld_x {ld} scale {scaled}: {ratio:.3f} of the bound")
            assert ratio <= 1.0


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


def test_grid2d_second_grid_pass_signed_weights_and_row_stride_8():
    """524,288 + 257 points: the 2,048-workgroup cap makes the grid loop take a second, ragged pass.  The points are the
    first two of eight columns (ld_y = 8: the grid over the first two of eight components; the other six hold values
    that would land in other cells), the weights are signed."""
    n = 524288 + 257
    y, ex, ey, _ = _points(7, 5, seed=3, n=n)
    rng = np.random.default_rng(4)
    w = rng.integers(-1000, 1001, n).astype(np.int32)
    y8 = rng.normal(0.0, 1.2, (n, 8)).astype(np.float32)
    y8[:, :2] = y
    yd = torch.from_numpy(y8).to(DEV)[:, :2]
    assert yd.stride(0) == 8
    count, wsum = ops.grid2d(yd, torch.from_numpy(ex).to(DEV), torch.from_numpy(ey).to(DEV), torch.from_numpy(w).to(DEV))
    want, want_w = er.hist2d_ref(y, ex, ey), er.hist2d_ref(y, ex, ey, w)
    assert 0 < want.sum() < n and want_w.min() < 0 < want_w.max()
    assert np.array_equal(count.cpu().numpy(), want)
    assert np.array_equal(wsum.cpu().numpy(), want_w)


@pytest.mark.parametrize("weight", [2 ** 31 - 1, -2 ** 31])
def test_grid2d_weight_sums_past_32_bits(weight):
    y = torch.zeros(3000, 2, device=DEV)
    e = torch.tensor([-1.0, 1.0], dtype=torch.float64, device=DEV)
    w = torch.full((3000,), weight, dtype=torch.int32, device=DEV)
    count, wsum = ops.grid2d(y, e, e, w)
    assert abs(3000 * weight) > 2 ** 32
    assert count.shape == (1, 1) and int(count[0, 0]) == 3000
    assert int(wsum[0, 0]) == 3000 * weight


# non-uniform edges with a repeated one (an empty cell) and the edge 0.0; every value is an fp32 number
EDGES5 = np.array([-2.0, -1.5, -1.5, 0.0, 0.125, 3.0])


def _edges256(seed):
    e = np.sort(np.random.default_rng(seed).uniform(-2.0, 3.0, 257).astype(np.float32).astype(np.float64))
    e[100] = e[101]
    e[np.searchsorted(e, 0.0)] = 0.0
    assert np.all(np.diff(e) >= 0.0) and e[0] < 0.0 < e[-1]
    return e


def _edge_points(ex, ey):
    """-0.0, +0.0, +-inf, NaN, every edge (the repeated one and both ends included) and its two fp32 neighbours, in
    both coordinates -> (y fp32 [n, 2], signed int32 weights)."""
    rng = np.random.default_rng(7)
    special = np.array([-0.0, 0.0, np.inf, -np.inf, np.nan], np.float32)
    vals = []
    for e in (ex, ey):
        e32 = e.astype(np.float32)
        assert np.array_equal(e32.astype(np.float64), e)
        vals.append(np.concatenate([special, e32, np.nextafter(e32, np.float32(-10)), np.nextafter(e32, np.float32(10)),
                                    rng.uniform(e[0] - 0.5, e[-1] + 0.5, 64).astype(np.float32)]))
    m = max(v.size for v in vals)
    # every value of one axis against values inside the other axis' range, then the two lists against each other
    inside = [np.float32(0.5 * (e[0] + e[-1])) for e in (ex, ey)]
    y = np.concatenate([
        np.stack([vals[0], np.full(vals[0].size, inside[1], np.float32)], axis=1),
        np.stack([np.full(vals[1].size, inside[0], np.float32), vals[1]], axis=1),
        np.stack([np.resize(vals[0], m), np.resize(vals[1], m)[::-1]], axis=1)]).astype(np.float32)
    return y, rng.integers(-50, 50, y.shape[0]).astype(np.int32)


@pytest.mark.parametrize("ex, ey", [(EDGES5, EDGES5[::-1] * -1.0), (np.array([-2.0, 3.0]), _edges256(0)),
                                    (_edges256(1), np.array([-1.0, 0.0]))], ids=["5x5", "1x256", "256x1"])
def test_grid2d_edge_values_equal_numpy(ex, ey):
    """Whatever numpy.histogram2d does with _edge_points over non-uniform edges (a repeated edge is an empty cell) is
    the specification."""
    y, w = _edge_points(ex, ey)
    with np.errstate(invalid="ignore"):
        want, want_w = er.hist2d_ref(y, ex, ey), er.hist2d_ref(y, ex, ey, w)
    assert 0 < want.sum() < y.shape[0]
    count, wsum = ops.grid2d(torch.from_numpy(y).to(DEV), torch.from_numpy(ex.copy()).to(DEV),
                             torch.from_numpy(ey.copy()).to(DEV), torch.from_numpy(w).to(DEV))
    assert np.array_equal(count.cpu().numpy(), want)
    assert np.array_equal(wsum.cpu().numpy(), want_w)


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
    # eight components: the grid is over the first two columns of an [n, 8] projection (row stride 8)
    er.assert_gaps(ref["eigenvalues"], 8)                            # seed 0 has the gaps up to k = 8
    out8 = embed.embedding_maps(model, g, n_components=8, grid=8)
    p8 = out8["patient"].cpu().numpy()
    assert out8["patient"].is_cuda and p8.shape == (1834, 8) and out8["patient"].stride(0) == 8
    d8 = float((np.abs(p8[:, :2] - ref["projection"]) / np.abs(ref["projection"]).max(axis=0)).max())
    print(f"first two of eight components {d8:.3e} (of {er.PROJ_REL:.3e}); eigenvalues {ref['eigenvalues'][:9]}")
    assert d8 <= er.PROJ_REL                                         # they do not depend on k
    ex8, ey8 = out8["edges"]
    count8 = out8["density"]["count"].to_numpy().reshape(8, 8)
    assert count8.sum() == 1834 and np.array_equal(count8, er.hist2d_ref(p8[:, :2], ex8, ey8))
    assert len(out8["variance"]) == 32 and list(out8["lab"].columns)[-1] == "pc8"
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
