"""Exact t-SNE on the MI355X (csrc/tsne.hip, mmgnn/embed.py tsne): the layers of the check are the distances (1 fp32
ulp), the perplexity search (bit-equal to the host search on the device's own distances, under an asserted margin), the
joint probabilities, one gradient under a derived bound, the update (exactly), twenty iterations under a measured
bound, the finished map by its objective, reproducibility, and the end-to-end frames and refusals.

Shapes: T = ops.TSNE_TILE = 512 points of Y per LDS tile, W = ops.TSNE_SEARCH_WIDTH = 256 threads per searched row; n = 4,
63, 65, W + 1, T - 1, T + 1 and 2 T + 3, D = 4, 68 and 256, every buffer with a padded row stride (ld_x = D + 8, ld_a =
n + 8) whose padding holds a sentinel that must survive."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import embed, ops
from mmgnn.model import build_model
from mmgnn.synth import make_graph
import tsne_ref as tr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T, W = ops.TSNE_TILE, ops.TSNE_SEARCH_WIDTH
SENTINEL = -12345.0
# (n, D, variant): "dup" = rows 5, 6 and 7 are equal (zero distances off the diagonal), "full" = perplexity n - 1
CASES = [(4, 4, ""), (63, 68, ""), (65, 256, ""), (W + 1, 16, ""), (T - 1, 8, ""), (T + 1, 128, ""), (2 * T + 3, 4, ""),
         (200, 32, ""), (63, 8, "dup"), (65, 64, "full")]
IDS = [f"n{n}-D{D}{'-' + v if v else ''}" for n, D, v in CASES]
assert (T, W) == (512, 256), "the shapes above are chosen for these two switches"


def _case_x(n, D, variant):
    x = tr.make_case(n, D)
    if variant == "dup":
        x[6] = x[5]
        x[7] = x[5]
    return x


def _perplexity(n, variant):
    return float(n - 1) if variant == "full" else tr.default_perplexity(n)


def _padded(a, pad=8, fill=SENTINEL):
    """A host matrix -> a device buffer with `pad` more columns of a sentinel, and the view of the data in it."""
    buf = np.full((a.shape[0], a.shape[1] + pad), fill, a.dtype)
    buf[:, :a.shape[1]] = a
    t = torch.from_numpy(buf).to(DEV)
    return t, t[:, :a.shape[1]]


@functools.lru_cache(maxsize=None)
def _affinities(n, D, variant):
    """The device's distances and joint probabilities of a case, computed once and shared (read-only) by the tests."""
    x = _case_x(n, D, variant)
    xbuf, xd = _padded(x, fill=1e6)
    assert xd.stride(0) == D + 8
    abuf = torch.full((n, n + 8), SENTINEL, device=DEV)
    a = abuf[:, :n]
    ops.tsne_sqdist(xd, out=a)
    dist = a.cpu().numpy().copy()
    pad_after_dist = abuf[:, n:].cpu().numpy().copy()
    beta, steps = ops.tsne_joint_p(a, _perplexity(n, variant))
    return dict(x=x, dist=dist, pad_after_dist=pad_after_dist, a=a, abuf=abuf, p=a.cpu().numpy().copy(),
                beta=beta.cpu().numpy(), steps=steps.cpu().numpy())


@pytest.mark.parametrize("n, D, variant", CASES, ids=IDS)
def test_distances_within_one_ulp_symmetric_zero_diagonal(n, D, variant):
    c = _affinities(n, D, variant)
    want = embed.tsne_sqdist_host(c["x"])
    got = c["dist"]
    assert np.array_equal(got, got.T), "A is not exactly symmetric"
    assert np.all(np.diag(got) == 0.0)
    ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(want, np.float32(1e-30)))
    print(f"({n}, {D}) {variant}: {int((ulps > 0).sum())} of {n * n} distances differ, at most {ulps.max():.0f} ulp")
    assert ulps.max() <= 1.0
    if variant == "dup":
        assert got[5, 6] == 0.0 and got[6, 7] == 0.0
    assert np.all(c["pad_after_dist"] == np.float32(SENTINEL)), "the padding of A was written"


@pytest.mark.parametrize("n, D, variant", CASES, ids=IDS)
def test_search_is_bit_equal_to_the_host_search_on_the_same_distances(n, D, variant):
    c = _affinities(n, D, variant)
    margin, (_, beta, steps) = tr.search_margin(c["dist"], _perplexity(n, variant))
    print(f"({n}, {D}) {variant}: margin {margin:.3e}, steps {steps.min()} .. {steps.max()}")
    assert margin >= tr.MARGIN, "a decision of the reference sits within rounding of the tolerance: not a case to keep"
    assert np.array_equal(c["steps"], steps)
    assert np.array_equal(c["beta"].view(np.int64), beta.view(np.int64))


@pytest.mark.parametrize("n, D, variant", CASES, ids=IDS)
def test_joint_p_against_the_host_path(n, D, variant):
    c = _affinities(n, D, variant)
    cond, _, _ = embed.tsne_search_host(c["dist"], _perplexity(n, variant))
    want = embed.tsne_joint_host(cond).astype(np.float64)
    got = c["p"]
    assert np.array_equal(got, got.T), "P is not exactly symmetric"
    assert np.all(np.diag(got) == 0.0)
    off = ~np.eye(n, dtype=bool)
    assert got[off].min() >= np.float32(tr.EPS)
    rel = (np.abs(got.astype(np.float64) - want) / np.maximum(want, tr.EPS))[off].max()
    print(f"({n}, {D}) {variant}: P {rel:.3e} relative (bound {4 * tr.U24:.3e}), sum {got.sum(dtype=np.float64):.9f}")
    assert rel <= 4 * tr.U24
    assert torch.all(c["abuf"][:, n:] == SENTINEL), "the padding of A was written"


def _maps(n):
    rng = np.random.default_rng(n)
    far = rng.normal(0.0, 10.0, (n, 2))
    far[::7] += 1e9                                   # num / Z of a pair across the gap is below eps: Q sits on its clamp
    return {"init": rng.normal(0.0, 1e-4, (n, 2)), "map": rng.normal(0.0, 10.0, (n, 2)), "far": far}


@pytest.mark.parametrize("exaggeration", [1.0, 12.0])
@pytest.mark.parametrize("scale", ["init", "map", "far"])
@pytest.mark.parametrize("n, D, variant", CASES[:8], ids=IDS[:8])
def test_one_gradient_under_the_derived_bound(n, D, variant, scale, exaggeration):
    c = _affinities(n, D, variant)
    y = _maps(n)[scale]
    kl, grad, z, b_kl, b_grad, b_z = tr.objective_bounds(c["p"], y, exaggeration, n)
    if scale == "far":
        num = 1.0 / (1.0 + ((y[:, None, :] - y[None, :, :]) ** 2).sum(-1))
        assert (num / z < tr.EPS).any(), "no pair of this map sits on the clamp of Q"
    rng = np.random.default_rng(1)
    yd = torch.from_numpy(y).to(DEV)
    u0, g0 = rng.normal(0.0, 1.0, (n, 2)), rng.uniform(0.01, 2.0, (n, 2))
    ud, gd = torch.from_numpy(u0).to(DEV), torch.from_numpy(g0).to(DEV)
    stats = torch.full((3,), SENTINEL, dtype=torch.float64, device=DEV)
    go = torch.full((n, 2), SENTINEL, dtype=torch.float64, device=DEV)
    ops.tsne_step(c["a"], yd, ud, gd, stats, exaggeration, 0.5, 200.0, 0.01, True, False, go)
    s, gdev = stats.cpu().numpy(), go.cpu().numpy()
    worst = float((np.abs(gdev - grad) / b_grad).max())
    print(f"({n}, {D}) {scale} x{exaggeration:g}: gradient {worst:.3f} of its bound, KL {abs(s[0] - kl) / b_kl:.3f}, "
          f"Z {abs(s[2] - z) / b_z:.3f}")
    assert worst <= 1.0
    assert abs(s[0] - kl) <= b_kl
    assert abs(s[2] - z) <= b_z
    assert np.array_equal(yd.cpu().numpy(), y) and np.array_equal(ud.cpu().numpy(), u0) \
        and np.array_equal(gd.cpu().numpy(), g0), "update = 0 wrote Y, U or G"
    # without the error: NaN, and the same gradient bit for bit
    go2 = torch.empty_like(go)
    ops.tsne_step(c["a"], yd, ud, gd, stats, exaggeration, 0.5, 200.0, 0.01, False, False, go2)
    assert np.isnan(stats.cpu().numpy()[0]) and torch.equal(go, go2)


@pytest.mark.parametrize("n, D, variant", [CASES[2], CASES[5]], ids=[IDS[2], IDS[5]])
def test_the_update_equals_numpy(n, D, variant):
    """One step from given Y, U, G: updates with and against the gradient's sign, U = 0 (U grad == 0 counts as "not
    inc"), gains at and just above min_gain (0.8 G falls below it).  Elementwise fp64 without contraction: equality."""
    c = _affinities(n, D, variant)
    rng = np.random.default_rng(3)
    y = rng.normal(0.0, 3.0, (n, 2))
    yd = torch.from_numpy(y).to(DEV)
    stats = torch.empty(3, dtype=torch.float64, device=DEV)
    go = torch.empty(n, 2, dtype=torch.float64, device=DEV)
    zeros, ones = torch.zeros_like(yd), torch.ones_like(yd)
    ops.tsne_step(c["a"], yd, zeros, ones, stats, 12.0, 0.5, 200.0, 0.01, False, False, go)
    grad = go.cpu().numpy()
    u = rng.normal(0.0, 1e-3, (n, 2)) * np.where(rng.random((n, 2)) < 0.5, np.sign(grad), -np.sign(grad))
    u[rng.random((n, 2)) < 0.2] = 0.0
    g = rng.uniform(0.01, 3.0, (n, 2))
    g[rng.random((n, 2)) < 0.3] = 0.01
    g[0] = 0.0124
    assert (u * grad < 0).any() and (u * grad > 0).any() and (u == 0).any()
    ud, gd = torch.from_numpy(u).to(DEV), torch.from_numpy(g).to(DEV)
    for momentum, lr in ((0.5, 200.0), (0.8, 37.5)):
        yh, uh, gh = yd.cpu().numpy().copy(), ud.cpu().numpy().copy(), gd.cpu().numpy().copy()
        ops.tsne_step(c["a"], yd, ud, gd, stats, 12.0, momentum, lr, 0.01, False, True, go)
        g2 = embed.tsne_update_host(yh, uh, gh, go.cpu().numpy(), momentum, lr, 0.01)
        assert (gh == 0.01).any()
        assert np.array_equal(gd.cpu().numpy(), gh), "gains"
        assert np.array_equal(ud.cpu().numpy(), uh), "update"
        assert np.array_equal(yd.cpu().numpy(), yh), "map"
        assert abs(stats.cpu().numpy()[1] - g2) <= 2 * n * tr.U53 * g2


def _run_device(a, y0, iters, lr, exaggeration=12.0, momentum=0.5):
    y = torch.from_numpy(np.ascontiguousarray(y0)).to(DEV)
    u, g = torch.zeros_like(y), torch.ones_like(y)
    stats = torch.empty(3, dtype=torch.float64, device=DEV)
    for _ in range(iters):
        ops.tsne_step(a, y, u, g, stats, exaggeration, momentum, lr, 0.01, False, True)
    return y, u, g


@pytest.mark.parametrize("n, D, variant", [CASES[7], CASES[5]], ids=[IDS[7], IDS[5]])
def test_twenty_iterations_under_the_measured_bound(n, D, variant):
    """Both runs start from the host path's PCA init and descend over the device's own P (read back), so that what is
    compared is the iteration; the bound is 8 x the host path's distance between a run and the same run with the
    points in reversed order, measured here."""
    c = _affinities(n, D, variant)
    y0 = tr.golden_starts(c["x"])[0]
    lr = max(n / 12.0 / 4.0, 50.0)
    host = tr.run_host(c["p"], y0, 20, lr)
    spread = float(np.abs(host - tr.run_host_reversed(c["p"], y0, 20, lr)).max())
    dev = _run_device(c["a"], y0, 20, lr)[0].cpu().numpy()
    d = float(np.abs(dev - host).max())
    ext = tr.extent(host)
    print(f"({n}, {D}): device against host {d:.3e} ({d / ext:.3e} of the extent {ext:.3e}); the host against its "
          f"reversed-order run {spread:.3e} ({spread / ext:.3e} of the extent); bound {8 * spread:.3e}")
    assert spread > 0.0
    assert d <= 8 * spread


@pytest.mark.parametrize("n, D", tr.GOLDEN_CASES)
def test_the_finished_map_by_its_objective(n, D, repo_root):
    with open(os.path.join(repo_root, "tests", "golden", "tsne_kl.json")) as f:
        kls = json.load(f)[f"{n}x{D}"]["kl"]
    assert len(kls) == 5
    x = tr.make_case(n, D)
    res = embed.tsne(torch.from_numpy(x).to(DEV), perplexity=tr.default_perplexity(n), max_iter=1000)
    assert res.embedding.is_cuda and res.embedding.dtype == torch.float64 and tuple(res.embedding.shape) == (n, 2)
    assert res.beta.is_cuda and res.beta.dtype == torch.float64 and res.n_iter <= 999
    p, _, _ = embed.tsne_affinities_host(x, tr.default_perplexity(n))
    kl = embed.tsne_objective_host(p, res.embedding.cpu().numpy())[0]
    bound = max(kls) + (max(kls) - min(kls))
    print(f"({n}, {D}): the device's map has KL {kl:.6f} (returned {res.kl_divergence:.6f}, n_iter {res.n_iter}); the "
          f"host path's five starts {min(kls):.6f} .. {max(kls):.6f}, bound {bound:.6f}")
    assert kl <= bound
    # the returned error is the device's objective at the map it returned: the host objective over the device's own P
    a = ops.tsne_sqdist(torch.from_numpy(x).to(DEV))
    ops.tsne_joint_p(a, tr.default_perplexity(n))
    again = embed.tsne_objective_host(a.cpu().numpy(), res.embedding.cpu().numpy())[0]
    print(f"  re-evaluated over the device's P: {again!r}, returned {res.kl_divergence!r}")
    assert abs(res.kl_divergence - again) <= 1e-12 * again


def test_bitwise_reproducible_eager_and_replayed():
    n, D = 2 * T + 3, 4
    x = torch.from_numpy(tr.make_case(n, D)).to(DEV)
    y0 = torch.from_numpy(tr.golden_starts(tr.make_case(n, D))[0]).to(DEV)
    a = torch.empty(n, n, device=DEV)
    y, u, g = torch.empty_like(y0), torch.empty_like(y0), torch.empty_like(y0)
    stats = torch.empty(3, dtype=torch.float64, device=DEV)
    beta = [None]

    def affinities():
        ops.tsne_sqdist(x, out=a)
        beta[0] = ops.tsne_joint_p(a, 30.0)[0]

    def step():
        ops.tsne_step(a, y, u, g, stats, 12.0, 0.5, 200.0, 0.01, True, True)

    def reset():
        a.fill_(-1.0)
        y.copy_(y0)
        u.zero_()
        g.fill_(1.0)

    def bits():
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in (a, beta[0], y, u, g, stats)]

    reset()
    affinities()
    for _ in range(60):
        step()
    ref = bits()
    assert np.all(np.isfinite(ref[2])) and np.isfinite(ref[5]).all()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        affinities()                                     # warm-up off the default stream, as torch.cuda.graph asks
        step()
    torch.cuda.current_stream().wait_stream(s)
    ga, gs = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(ga):
        affinities()
    with torch.cuda.graph(gs):
        step()
    for _ in range(2):
        reset()
        ga.replay()
        for _ in range(60):
            gs.replay()
        for name, r, o in zip(("P", "beta", "Y", "U", "G", "stats"), ref, bits()):
            assert np.array_equal(r.view(np.uint8), o.view(np.uint8)), f"{name}: a replayed capture differs from the eager run"


def test_embedding_tsne_end_to_end(tmp_path):
    g = make_graph(1, seed=0).to(DEV)
    cfg = {"model": {"architecture": "RGCN", "hidden_dim": 64, "num_layers": 2, "dropout": 0.0,
                     "use_batch_norm": True, "activation": "relu"}}
    torch.manual_seed(0)
    model = build_model(cfg, (g.node_types, g.edge_types), None).to(DEV)
    model._init_embeddings(g)
    model.train()
    names = {i: n for i, n in enumerate(["pH", "PTT", "sodium"])}
    out = embed.embedding_tsne(model, g, perplexity=60.0, max_points=300, seed=7, output_dir=tmp_path, lab_names=names)
    assert model.training
    for f in ("lab_embeddings_tsne.csv", "diagnosis_embeddings_tsne.csv", "medication_embeddings_tsne.csv",
              "patient_embeddings_tsne.csv", "tsne_summary.csv"):
        assert os.path.getsize(tmp_path / f) > 0, f
    assert list(out["lab"].columns) == ["idx", "name", "panel", "tsne1", "tsne2"]
    assert list(out["diagnosis"].columns) == ["idx", "name", "tsne1", "tsne2"]
    assert list(out["medication"].columns) == ["idx", "name", "tsne1", "tsne2"]
    assert list(out["patient"].columns) == ["patient_idx", "tsne1", "tsne2", "lab_degree"]
    assert list(out["summary"].columns) == embed.TSNE_SUMMARY_COLUMNS
    n_of = {t: int(g[t].num_nodes) for t in ("lab", "diagnosis", "medication")}
    assert len(out["lab"]) == n_of["lab"] == 50 and list(out["lab"]["panel"][:3]) == ["ABG", "Coag", "CMP"]
    summ = out["summary"].set_index("node_type")
    for t, n in n_of.items():
        assert summ.loc[t, "n"] == n and summ.loc[t, "perplexity"] == min(60.0, n - 1.0)
        assert summ.loc[t, "learning_rate"] == max(n / 12.0 / 4.0, 50.0)
    assert summ.loc["lab", "perplexity"] == 49.0                     # 50 labs: the per-type rule binds
    assert summ.loc["patient", "n"] == 300 and summ.loc["patient", "perplexity"] == 60.0
    pick = np.random.RandomState(7).choice(1834, 300, replace=False)
    assert np.array_equal(out["patient"]["patient_idx"].to_numpy(), pick)
    deg = np.bincount(g["patient", "has_lab", "lab"].edge_index[0].cpu().numpy(), minlength=1834)
    assert np.array_equal(out["patient"]["lab_degree"].to_numpy(), deg[pick])
    for t in ("lab", "diagnosis", "medication", "patient"):
        assert np.all(np.isfinite(out[t][["tsne1", "tsne2"]].to_numpy()))
        assert np.isfinite(summ.loc[t, "kl_divergence"]) and 0 < summ.loc[t, "n_iter"] <= 999


def test_c_level_refusals_leave_the_outputs_unwritten():
    from mmgnn import _lib
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())                      # noqa: E731
    st = ops._stream()
    x = torch.zeros(64, 16, device=DEV)
    a = torch.full((64, 64), SENTINEL, device=DEV)
    d = torch.full((64 * 2,), SENTINEL, dtype=torch.float64, device=DEV)
    i32 = torch.full((64,), -7, dtype=torch.int32, device=DEV)
    stats = torch.full((3,), SENTINEL, dtype=torch.float64, device=DEV)
    ws = ops.workspace(max(lib.mmg_tsne_joint_p_ws_bytes(64), lib.mmg_tsne_step_ws_bytes(64)), DEV)
    assert lib.mmg_tsne_joint_p_ws_bytes(3) == 0 and lib.mmg_tsne_joint_p_ws_bytes(16385) == 0
    assert lib.mmg_tsne_step_ws_bytes(3) == 0 and lib.mmg_tsne_step_ws_bytes(16385) == 0
    assert lib.mmg_tsne_step_ws_bytes(16384) > 0 and lib.mmg_tsne_joint_p_ws_bytes(4) > 0

    def sqdist(n, D, ld_x, ld_a):
        return lib.mmg_tsne_sqdist(p(x), n, D, ld_x, p(a), ld_a, None, 0, st)

    def joint(n, ld_a, perp, nbytes):
        return lib.mmg_tsne_joint_p(p(a), n, ld_a, perp, p(d), p(i32), p(ws), nbytes, st)

    def step(n, ld_a, nbytes):
        return lib.mmg_tsne_step(p(a), n, ld_a, 1.0, p(d), p(d), p(d), 0.5, 200.0, 0.01, 1, p(stats), None, 1, p(ws), nbytes,
                                 st)

    for n in (3, 16385):
        assert sqdist(n, 16, 16, 16385) == -1 and f"n {n}".encode() in lib.mmg_last_error()
        assert joint(n, 16385, 2.0, ws.numel()) == -1 and f"n {n}".encode() in lib.mmg_last_error()
        assert step(n, 16385, ws.numel()) == -1 and f"n {n}".encode() in lib.mmg_last_error()
    assert sqdist(64, 6, 16, 64) == -1 and b"D 6" in lib.mmg_last_error()
    assert sqdist(64, 16, 12, 64) == -1 and b"ld_x" in lib.mmg_last_error()
    assert sqdist(64, 16, 16, 63) == -1 and b"ld_a" in lib.mmg_last_error()
    assert joint(64, 63, 30.0, ws.numel()) == -1 and b"ld_a" in lib.mmg_last_error()
    assert step(64, 63, ws.numel()) == -1 and b"ld_a" in lib.mmg_last_error()
    assert joint(64, 64, 64.0, ws.numel()) == -1 and b"perplexity" in lib.mmg_last_error()
    assert joint(64, 64, 30.0, lib.mmg_tsne_joint_p_ws_bytes(64) - 1) == -3 and b"workspace" in lib.mmg_last_error()
    assert step(64, 64, lib.mmg_tsne_step_ws_bytes(64) - 1) == -3 and b"workspace" in lib.mmg_last_error()
    torch.cuda.synchronize()
    assert torch.all(a == SENTINEL) and torch.all(d == SENTINEL) and torch.all(i32 == -7) and torch.all(stats == SENTINEL)
    # and through the Python layer
    with pytest.raises(ValueError, match="perplexity"):
        embed.tsne(x, perplexity=64.0)
    with pytest.raises(ValueError, match="multiple of 4"):
        embed.tsne(torch.zeros(64, 6, device=DEV))
    with pytest.raises(ValueError, match="2 components"):
        embed.tsne(x, n_components=3)
    bad = x.clone()
    bad[3, 3] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        embed.tsne(bad)
