"""Exact t-SNE without a GPU (mmgnn/embed.py tsne): the host path -- the checker of test_tsne_gpu.py -- against sklearn
1.7's own pieces (_joint_probabilities, _kl_divergence, TSNE(method="exact")), the schedule and both stopping rules on a
stubbed objective, the refusals, the C symbols, and embedding_tsne's frames and files on a host stub."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import embed
from mmgnn.synth import make_graph
import tsne_ref as tr

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("n, D", [(60, 16), (200, 32)])
def test_host_p_against_sklearn_joint_probabilities(n, D):
    sk = pytest.importorskip("sklearn.manifold._t_sne")
    from scipy.spatial.distance import squareform
    x = tr.make_case(n, D)
    dist = embed.tsne_sqdist_host(x)
    assert dist.dtype == np.float32 and np.array_equal(dist, dist.T) and np.all(np.diag(dist) == 0)
    cond, beta, steps = embed.tsne_search_host(dist, tr.default_perplexity(n))
    p = embed.tsne_joint_host(cond)
    assert p.dtype == np.float32 and np.array_equal(p, p.T) and np.all(np.diag(p) == 0)
    assert steps.min() >= 1 and steps.max() < 100 and np.all(beta > 0)
    want = squareform(sk._joint_probabilities(dist, tr.default_perplexity(n), 0))
    off = ~np.eye(n, dtype=bool)
    rel = (np.abs(p.astype(np.float64) - want) / np.maximum(want, tr.EPS))[off].max()
    print(f"({n}, {D}): P against sklearn {rel:.3e} relative (bound {4 * tr.U24:.3e})")
    assert rel <= 4 * tr.U24
    # the entropy of every conditional row is the perplexity's, to the search's tolerance
    c = cond.astype(np.float64)
    h = -(c[off].reshape(n, n - 1) * np.log(np.maximum(c[off].reshape(n, n - 1), 1e-300))).sum(axis=1)
    assert np.abs(h - np.log(tr.default_perplexity(n))).max() <= 1e-5 + 1e-6


@pytest.mark.parametrize("exaggeration", [1.0, 12.0])
@pytest.mark.parametrize("n, D", [(60, 16), (200, 32)])
def test_host_objective_against_sklearn_kl_divergence(n, D, exaggeration):
    sk = pytest.importorskip("sklearn.manifold._t_sne")
    from scipy.spatial.distance import squareform
    p, _, _ = embed.tsne_affinities_host(tr.make_case(n, D), tr.default_perplexity(n))
    y = np.random.default_rng(1).normal(0.0, 10.0, (n, 2))
    kl, grad, _ = embed.tsne_objective_host(p, y, exaggeration)
    pc = exaggeration * squareform(p.astype(np.float64), checks=False)
    kl_sk, grad_sk = sk._kl_divergence(y.ravel().copy(), pc, 1.0, n, 2)
    d_kl = abs(kl - kl_sk) / abs(kl_sk)
    d_grad = np.abs(grad.ravel() - grad_sk).max() / np.abs(grad_sk).max()
    print(f"({n}, {D}) x{exaggeration:g}: KL {d_kl:.3e}, gradient {d_grad:.3e} relative")
    assert d_kl <= 1e-6 and d_grad <= 1e-6
    assert np.isnan(embed.tsne_objective_host(p, y, exaggeration, want_kl=False)[0])


def _stub(errors):
    """step / read over a scripted objective: errors(i) -> (error, sum g^2) of iteration i; the calls are recorded."""
    calls = []

    def step(exaggeration, momentum, want_kl, update):
        calls.append((exaggeration, momentum, want_kl, update))

    def read():
        assert calls[-1][2], "read() after an iteration that did not compute the error"
        return errors(sum(1 for c in calls if c[3]) - 1)
    return calls, step, read


def test_schedule_and_stage_switch_on_a_stubbed_objective():
    calls, step, read = _stub(lambda i: (1000.0 - i, 1.0))                      # always improving
    error, it = embed.tsne_descent(step, read, 1000, 12.0, 300, 1e-7)
    assert it == 999 and len(calls) == 1001
    assert all(c[:2] == (12.0, 0.5) for c in calls[:250]) and all(c[:2] == (1.0, 0.8) for c in calls[250:1000])
    assert [i for i, c in enumerate(calls[:1000]) if c[2]] == list(range(49, 1000, 50))
    assert all(c[3] for c in calls[:1000])
    assert calls[1000] == (1.0, 0.8, True, False)                               # the error AT the returned map
    assert error == 1000.0 - 999
    # a max_iter off the 50-grid: the last iteration computes the error too
    calls, step, read = _stub(lambda i: (1000.0 - i, 1.0))
    error, it = embed.tsne_descent(step, read, 777, 12.0, 300, 1e-7)
    assert it == 776 and calls[776][2] and not calls[775][2]


def test_both_stopping_rules_on_a_stubbed_objective():
    # no progress: the first stage's patience of 250 never runs out inside its 250 iterations; the second stage's first
    # check (299) sets its own best error, and 649 is the first check more than 300 iterations past it
    calls, step, read = _stub(lambda i: (1.0, 1.0))
    error, it = embed.tsne_descent(step, read, 1000, 12.0, 300, 1e-7)
    assert it == 649 and sum(1 for c in calls if c[3]) == 650
    calls, step, read = _stub(lambda i: (1.0, 1.0))
    assert embed.tsne_descent(step, read, 1000, 12.0, 100, 1e-7)[1] == 449
    # the gradient norm: each stage breaks at its first check
    calls, step, read = _stub(lambda i: (1000.0 - i, 1e-16))
    error, it = embed.tsne_descent(step, read, 1000, 12.0, 300, 1e-7)
    assert it == 99 and [c[:2] for c in calls[:100]] == [(12.0, 0.5)] * 50 + [(1.0, 0.8)] * 50
    calls, step, read = _stub(lambda i: (1000.0 - i, 1.0000001e-14))            # sqrt just above 1e-7: no break
    assert embed.tsne_descent(step, read, 300, 12.0, 300, 1e-7)[1] == 299


def test_stopping_rules_agree_with_sklearn_gradient_descent():
    sk = pytest.importorskip("sklearn.manifold._t_sne")
    for patience, err in ((300, lambda i: 1.0), (100, lambda i: 1.0), (300, lambda i: 5.0 + np.cos(i / 40.0))):
        seen = []

        def objective(p, compute_error=True):
            seen.append(0)
            return (err(len(seen) - 1) if compute_error else np.nan), np.ones_like(p)
        args = dict(n_iter_check=50, learning_rate=1.0, min_grad_norm=1e-7, args=[], kwargs={})
        p, _, it = sk._gradient_descent(objective, np.zeros(8), it=0, max_iter=250, n_iter_without_progress=250,
                                        momentum=0.5, **args)
        p, _, it = sk._gradient_descent(objective, p, it=it + 1, max_iter=1000, n_iter_without_progress=patience,
                                        momentum=0.8, **args)
        calls, step, read = _stub(lambda i: (err(i), 8.0))
        assert embed.tsne_descent(step, read, 1000, 12.0, patience, 1e-7)[1] == it


def test_learning_rate_rule(monkeypatch):
    monkeypatch.setattr(embed, "tsne_affinities_host", lambda x, perplexity: (None, np.ones(x.shape[0]), None))
    monkeypatch.setattr(embed, "tsne_descent", lambda *a: (0.0, 0))
    rng = np.random.default_rng(0)
    assert embed.tsne(rng.normal(size=(60, 4))).learning_rate == 50.0
    assert embed.tsne(rng.normal(size=(4800, 4))).learning_rate == 100.0
    assert embed.tsne(rng.normal(size=(4800, 4)), early_exaggeration=4.0).learning_rate == 300.0
    assert embed.tsne(rng.normal(size=(60, 4)), learning_rate=7.5).learning_rate == 7.5
    res = embed.tsne(rng.normal(size=(60, 4)))
    assert abs(np.std(res.embedding[:, 0]) - 1e-4) <= 1e-17 and res.embedding.shape == (60, 2)   # the PCA init
    init = rng.normal(size=(60, 2))
    assert np.array_equal(embed.tsne(rng.normal(size=(60, 4)), init=init).embedding, init)


def test_final_kl_against_sklearn_exact():
    skm = pytest.importorskip("sklearn.manifold")
    n, D = 60, 16
    with open(os.path.join(HERE, "golden", "tsne_kl.json")) as f:
        kls = json.load(f)[f"{n}x{D}"]["kl"]
    bound = max(kls) + (max(kls) - min(kls))
    x = tr.make_case(n, D)
    y0 = tr.golden_starts(x)[0]
    res = embed.tsne(x, perplexity=tr.default_perplexity(n), init=y0)
    m = skm.TSNE(method="exact", init=y0.astype(np.float32), perplexity=tr.default_perplexity(n), max_iter=1000).fit(x)
    print(f"host path: KL {res.kl_divergence:.6f} after n_iter {res.n_iter}; sklearn: KL {m.kl_divergence_:.6f} after "
          f"{m.n_iter_}; the five recorded starts {min(kls):.6f} .. {max(kls):.6f}, bound {bound:.6f}")
    assert res.n_iter <= 999 and isinstance(res.embedding, np.ndarray) and res.embedding.shape == (n, 2)
    assert res.kl_divergence <= bound and m.kl_divergence_ <= bound
    p, _, _ = embed.tsne_affinities_host(x, tr.default_perplexity(n))
    assert res.kl_divergence == embed.tsne_objective_host(p, res.embedding)[0]
    assert res.learning_rate == m.learning_rate_ == 50.0


def test_refusals():
    x = tr.make_case(30, 8)
    with pytest.raises(ValueError, match="perplexity"):
        embed.tsne(x, perplexity=30.0)
    with pytest.raises(ValueError, match="perplexity"):
        embed.tsne(x, perplexity=0.0)
    bad = x.copy()
    bad[3, 2] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        embed.tsne(bad, perplexity=5.0)
    with pytest.raises(ValueError, match="2 components"):
        embed.tsne(x, n_components=3, perplexity=5.0)
    with pytest.raises(ValueError, match="init"):
        embed.tsne(x, perplexity=5.0, init="random")
    with pytest.raises(ValueError, match="init"):
        embed.tsne(x, perplexity=5.0, init=np.zeros((30, 3)))
    with pytest.raises(ValueError, match="at least 4"):
        embed.tsne(x[:3], perplexity=2.0)
    with pytest.raises(ValueError, match="max_iter"):
        embed.tsne(x, perplexity=5.0, max_iter=100)

    class Sharded:
        _comm = object()
    with pytest.raises(NotImplementedError, match="dist.shard_model"):
        embed.embedding_tsne(Sharded(), None)
    with pytest.raises(ValueError, match="max_points"):
        embed.embedding_tsne(object(), None, max_points=16385)


def test_c_symbols_workspace_sizes_and_argument_refusals():
    """The symbols are in libmmgnn.so; every refusal comes before any HIP call (the fake pointers are never touched)."""
    from mmgnn import _lib, ops
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    want = ["mmg_tsne_sqdist", "mmg_tsne_sqdist_ws_bytes", "mmg_tsne_joint_p", "mmg_tsne_joint_p_ws_bytes", "mmg_tsne_step",
            "mmg_tsne_step_ws_bytes"]
    for s in want:
        assert hasattr(raw, s), s
    assert set(want) <= set(_lib.SIGNATURES)
    assert (_lib.MMG_TSNE_MAX_N, ops.TSNE_TILE, ops.TSNE_SEARCH_WIDTH) == (16384, 512, 256) == (embed.TSNE_MAX_N, 512, 256)
    for fn in (lib.mmg_tsne_joint_p_ws_bytes, lib.mmg_tsne_step_ws_bytes):
        assert fn(3) == 0 and fn(16385) == 0 and fn(-1) == 0 and 0 < fn(4) <= fn(16384)
    assert lib.mmg_tsne_joint_p_ws_bytes(16384) >= 256 * 256 * 8 and lib.mmg_tsne_step_ws_bytes(16384) >= 2 * 16384 * 8
    p = ctypes.c_void_p(256)
    need_j, need_s = lib.mmg_tsne_joint_p_ws_bytes(100), lib.mmg_tsne_step_ws_bytes(100)

    def sqdist(n=100, D=16, ld_x=16, ld_a=100, x=p, a=p):
        return lib.mmg_tsne_sqdist(x, n, D, ld_x, a, ld_a, None, 0, None), lib.mmg_last_error()

    def joint(n=100, ld_a=100, perp=30.0, a=p, ws=p, nb=need_j):
        return lib.mmg_tsne_joint_p(a, n, ld_a, perp, p, p, ws, nb, None), lib.mmg_last_error()

    def step(n=100, ld_a=100, y=p, stats=p, ws=p, nb=need_s):
        return lib.mmg_tsne_step(p, n, ld_a, 1.0, y, p, p, 0.5, 200.0, 0.01, 1, stats, None, 1, ws, nb, None), \
            lib.mmg_last_error()

    for fn, name in ((sqdist, b"tsne_sqdist"), (joint, b"tsne_joint_p"), (step, b"tsne_step")):
        for kw, word in ((dict(n=3), b"n 3"), (dict(n=16385, ld_a=16385), b"n 16385"), (dict(ld_a=99), b"ld_a 99")):
            rc, msg = fn(**kw)
            assert rc == -1 and name in msg and word in msg, (name, kw, rc, msg)
    for kw, word in ((dict(D=6), b"D 6"), (dict(D=260, ld_x=260), b"D 260"), (dict(ld_x=12), b"ld_x 12"), (dict(x=None), b"null"),
                     (dict(a=None), b"null")):
        rc, msg = sqdist(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    for perp in (0.0, 100.0, float("nan"), float("inf")):
        rc, msg = joint(perp=perp)
        assert rc == -1 and b"perplexity" in msg, (perp, rc, msg)
    assert joint(a=None)[0] == -1 and step(y=None)[0] == -1 and step(stats=None)[0] == -1
    for fn, need in ((joint, need_j), (step, need_s)):
        for ws, nb in ((p, need - 1), (None, need)):
            rc, msg = fn(ws=ws, nb=nb)
            assert rc == -3 and b"workspace" in msg, (rc, msg)


class _HostModel:
    """encode_nodes of a model on the host: fixed embeddings per node type."""
    training = True
    _comm = None

    def __init__(self, n_patients):
        rng = np.random.default_rng(0)
        self.x = {t: torch.from_numpy(tr.make_case(n, 8, seed=s))
                  for s, (t, n) in enumerate((("patient", n_patients), ("lab", 50), ("diagnosis", 12), ("medication", 4)))}
        self.w = torch.nn.Parameter(torch.from_numpy(rng.normal(size=2)))

    def parameters(self):
        return iter([self.w])

    def eval(self):
        self.training = False

    def train(self, flag=True):
        self.training = flag

    def encode_nodes(self, graph):
        assert not self.training
        return dict(self.x)


def test_embedding_tsne_frames_and_files_on_a_host_stub(tmp_path):
    g = make_graph(1, seed=0)
    n_pat = int(g["patient"].num_nodes)
    model = _HostModel(n_pat)
    names = {i: n for i, n in enumerate(["pH", "PTT", "sodium"])}
    out = embed.embedding_tsne(model, g, perplexity=10.0, max_points=40, seed=3, output_dir=tmp_path, lab_names=names)
    assert model.training
    assert list(out["lab"].columns) == ["idx", "name", "panel", "tsne1", "tsne2"] and len(out["lab"]) == 50
    assert list(out["lab"]["panel"][:4]) == ["ABG", "Coag", "CMP", "Other"] and out["lab"]["name"][3] == "lab_3"
    assert list(out["diagnosis"].columns) == ["idx", "name", "tsne1", "tsne2"] and len(out["diagnosis"]) == 12
    assert list(out["medication"].columns) == ["idx", "name", "tsne1", "tsne2"] and len(out["medication"]) == 4
    assert list(out["patient"].columns) == ["patient_idx", "tsne1", "tsne2", "lab_degree"] and len(out["patient"]) == 40
    pick = np.random.RandomState(3).choice(n_pat, 40, replace=False)
    assert np.array_equal(out["patient"]["patient_idx"].to_numpy(), pick)
    deg = np.bincount(g["patient", "has_lab", "lab"].edge_index[0].numpy(), minlength=n_pat)
    assert np.array_equal(out["patient"]["lab_degree"].to_numpy(), deg[pick])
    summ = out["summary"]
    assert list(summ.columns) == embed.TSNE_SUMMARY_COLUMNS
    assert list(summ["node_type"]) == ["lab", "diagnosis", "medication", "patient"]
    assert list(summ["n"]) == [50, 12, 4, 40] and list(summ["perplexity"]) == [10.0, 10.0, 3.0, 10.0]
    assert list(summ["learning_rate"]) == [50.0] * 4 and np.all(np.isfinite(summ["kl_divergence"])) and summ["n_iter"].max() <= 999
    for t in ("lab", "diagnosis", "medication", "patient"):
        assert np.all(np.isfinite(out[t][["tsne1", "tsne2"]].to_numpy()))
        assert os.path.getsize(tmp_path / f"{t}_embeddings_tsne.csv") > 0
    assert os.path.getsize(tmp_path / "tsne_summary.csv") > 0


def test_package_exports():
    assert mmgnn.tsne is embed.tsne and mmgnn.embedding_tsne is embed.embedding_tsne and mmgnn.TSNEResult is embed.TSNEResult
