"""Embedding maps without a GPU (mmgnn/embed.py): the host path of pca against the float64 restatement, the restatement
against sklearn, the panel rule on the reference's lab names, the refusals and the C symbols."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import embed
import embed_ref as er

HERE = os.path.dirname(os.path.abspath(__file__))


def _lab_names():
    with open(os.path.join(HERE, "golden", "embed_lab_names.json")) as f:
        d = json.load(f)
    return dict(zip(d["lab_index"], d["lab_name"]))


@pytest.mark.parametrize("n", [5000, 50])
@pytest.mark.parametrize("k, sv", [(2, (8, 4, 2, 1)), (8, er.SV8)])
@pytest.mark.parametrize("whiten", [False, True])
def test_host_pca_against_the_restatement(n, k, sv, whiten):
    x = er.make_case(n, 128, seed=1, sv=sv)
    ref = er.pca_ref(x, k, whiten)
    er.check_pca(embed.pca(x, k, whiten), ref, k)
    res = embed.pca(torch.from_numpy(x), k, whiten)                  # a host tensor takes the same path
    assert isinstance(res.projection, np.ndarray) and res.projection.dtype == np.float64
    er.check_pca(res, ref, k)


def test_host_pca_accepts_any_width_and_clamps_round_off():
    x = er.make_case(40, 6, seed=3)[:, :5]                           # D = 5: no device limit on the host
    x = np.concatenate([x, x[:, :1]], axis=1)                        # a duplicated column: one eigenvalue is round-off
    res = embed.pca(x, 6)
    assert res.components.shape == (6, 6) and np.all(res.explained_variance >= 0.0)
    assert res.explained_variance[-1] <= 1e-12 * res.explained_variance[0]
    assert abs(res.explained_variance_ratio.sum() - 1.0) <= 1e-12
    lead = np.argmax(np.abs(res.components), axis=1)
    assert np.all(res.components[np.arange(6), lead] > 0)


@pytest.mark.parametrize("whiten", [False, True])
@pytest.mark.parametrize("n, k, sv", [(5000, 2, (8, 4, 2, 1)), (50, 8, er.SV8)])
def test_restatement_against_sklearn(n, k, sv, whiten):
    skd = pytest.importorskip("sklearn.decomposition")
    x64 = er.make_case(n, 128, seed=1, sv=sv).astype(np.float64)
    ref = er.pca_ref(x64, k, whiten)
    er.assert_gaps(ref["eigenvalues"], k)
    m = skd.PCA(n_components=k, whiten=whiten, svd_solver="full").fit(x64)
    assert np.abs(m.components_ - ref["components"]).max() <= er.COMP_ABS
    assert np.abs(m.mean_ - ref["mean"]).max() <= er.COMP_ABS
    for a, b in ((m.explained_variance_, "explained_variance"), (m.explained_variance_ratio_, "explained_variance_ratio"),
                 (m.singular_values_, "singular_values")):
        assert (np.abs(a - ref[b]) / ref[b]).max() <= er.VAR_REL, b
    p = m.transform(x64)
    assert (np.abs(p - ref["projection"]) / np.abs(ref["projection"]).max(axis=0)).max() <= 1e-12


def test_gram_bounds_hold_for_the_host_arithmetic():
    """The recorded bounds are 8 x numpy's own distance from the 80-bit sums: numpy's evaluation on this machine has to
    lie inside them, on every case the GPU tests use (the 80-bit sums of the two largest take a few seconds each, once:
    embed_ref.gram80 keeps them)."""
    assert len(er.GRAM_CASES) == 14
    for n, D, ld in er.GRAM_CASES:
        dm, dg = er.numpy_distances(n, D, ld)
        bm, bg = er.gram_bounds(n, D, ld)
        print((n, D, ld), dm, dg, bm, bg)
        assert dm <= bm and dg <= bg


@pytest.mark.parametrize("n, D, k", [c for c in er.PROJECT_CASES if c[0] <= 1000])
def test_projection_bound_holds_for_the_host_arithmetic(n, D, k):
    """A float64 numpy evaluation rounded once to fp32 lies inside the derived bound of the row projection (its sums run
    over D terms, the device's over D / 16 + 4): the bound asks nothing a correct evaluation cannot give."""
    case = er.project_case(n, D, k)
    xc = case["x"].astype(np.float64) - case["mean"]
    for scaled in (False, True):
        out = (xc @ case["comps"].T) * (case["scale"] if scaled else 1.0)
        ratio = er.project_ratio(out.astype(np.float32), case, D, scaled)
        print((n, D, k), scaled, ratio)
        assert ratio <= 1.0
    wrong = (xc @ case["comps"].T).astype(np.float32).astype(np.float64) * (1.0 + 2.0 ** -22)
    assert er.project_ratio(wrong, case, D, False) > 1.0           # and it notices two fp32 ulps


def test_lab_panels_on_the_reference_lab_names():
    names = _lab_names()
    for must in ("pH", "phosphate", "alkaline phos.", "PT", "PT - INR", "PTT", "platelets x 1000"):
        assert must in names.values()
    got = embed.lab_panels(names)
    assert got == er.panel_ref(names) and set(got) == set(names)
    by_name = {names[i]: p for i, p in got.items()}
    # later panels overwrite earlier ones, substrings match: the reference's behaviour, kept
    assert by_name["pH"] == "ABG" and by_name["phosphate"] == "ABG" and by_name["alkaline phos."] == "ABG"
    assert by_name["-lymphs"] == "ABG" and by_name["paCO2"] == "ABG"
    assert by_name["PT"] == by_name["PT - INR"] == by_name["PTT"] == "Coag"
    assert by_name["platelets x 1000"] == "CBC" and by_name["MCHC"] == "CBC"
    assert by_name["bedside glucose"] == "CMP" and by_name["total protein"] == "LFT"
    assert by_name["lactate"] == "Other" and by_name["troponin - I"] == "Other"
    assert embed.lab_panels(list(names.values())) == got              # a sequence is indexed by position
    assert embed.lab_panels({7: "PH (ARTERIAL)"}) == {7: "ABG"}      # case-insensitive


def test_python_refusals():
    x = er.make_case(10, 8)
    with pytest.raises(ValueError, match="at least 2"):
        embed.pca(x[:1], 1)
    with pytest.raises(ValueError, match=r"min\(n, D\) = 8"):
        embed.pca(x, 9)
    with pytest.raises(ValueError, match=r"min\(n, D\) = 3"):
        embed.pca(x[:3], 4)
    with pytest.raises(ValueError, match="n_components"):
        embed.pca(x, 0)
    with pytest.raises(ValueError, match="2 dimensions|dimensions"):
        embed.pca(x[0], 1)
    with pytest.raises(ValueError, match="256"):
        embed.density_grid(np.zeros((4, 2)), np.zeros(4), grid=257)


def test_c_symbols_and_argument_refusals():
    """The six symbols are in libmmgnn.so; every refusal comes before any HIP call (the fake pointers are never
    touched)."""
    from mmgnn import _lib
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    want = ["mmg_centered_gram", "mmg_centered_gram_ws_bytes", "mmg_project_rows", "mmg_project_rows_ws_bytes",
            "mmg_grid2d", "mmg_grid2d_ws_bytes"]
    for s in want:
        assert hasattr(raw, s), s
    assert set(want) <= set(_lib.SIGNATURES)
    p = ctypes.c_void_p(256)
    need = lib.mmg_centered_gram_ws_bytes(1000, 128)
    assert need > 0 and lib.mmg_centered_gram_ws_bytes(1000, 260) == 0 and lib.mmg_centered_gram_ws_bytes(1000, 6) == 0
    assert lib.mmg_centered_gram_ws_bytes(1, 128) == 0

    def gram(n=1000, D=128, ld=128, ws=p, nb=need):
        return lib.mmg_centered_gram(p, n, D, ld, p, p, ws, nb, None), lib.mmg_last_error()

    for kw, word in ((dict(D=260), b"D 260"), (dict(D=6), b"D 6"), (dict(D=0), b"D 0"), (dict(n=1), b"n 1"),
                     (dict(ld=127), b"ld_x 127")):
        rc, msg = gram(**kw)
        assert rc == -1 and b"centered_gram" in msg and word in msg, (kw, rc, msg)
    for ws, nb in ((p, need - 1), (None, need)):
        rc, msg = gram(ws=ws, nb=nb)
        assert rc == -3 and b"centered_gram" in msg and b"workspace" in msg

    def proj(n=10, D=128, ld=128, k=2, ldo=2):
        return lib.mmg_project_rows(p, n, D, ld, p, p, None, k, p, ldo, None, 0, None), lib.mmg_last_error()

    for kw, word in ((dict(k=9), b"k 9"), (dict(k=0), b"k 0"), (dict(D=260), b"D 260"), (dict(D=6), b"D 6"),
                     (dict(ldo=1), b"ld_out 1"), (dict(ld=64), b"ld_x 64"), (dict(n=0), b"n 0")):
        rc, msg = proj(**kw)
        assert rc == -1 and b"project_rows" in msg and word in msg, (kw, rc, msg)

    def grid(gx=4, gy=4, n=10, ld=2, w=None, wsum=p):
        return lib.mmg_grid2d(p, ld, w, n, p, p, gx, gy, p, wsum, None, 0, None), lib.mmg_last_error()

    for kw, word in ((dict(gx=257), b"257"), (dict(gy=0), b"4 x 0"), (dict(ld=1), b"ld_y 1"), (dict(n=-1), b"n -1"),
                     (dict(w=p, wsum=None), b"wsum")):
        rc, msg = grid(**kw)
        assert rc == -1 and b"grid2d" in msg and word in msg, (kw, rc, msg)


def test_sharded_model_is_refused():
    class Sharded:
        _comm = object()
    with pytest.raises(NotImplementedError, match="dist.shard_model"):
        embed.embedding_maps(Sharded(), None)


def test_package_exports():
    assert mmgnn.embed is embed
    assert mmgnn.embedding_maps is embed.embedding_maps and mmgnn.lab_panels is embed.lab_panels
