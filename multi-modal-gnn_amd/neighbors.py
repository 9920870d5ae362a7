"""Neighbours in the embedding space and the quality of a 2-D map of it: exact k-nearest-neighbour search
(``sklearn.neighbors.NearestNeighbors(algorithm="brute")`` semantics, Euclidean), neighbour ranks, and sklearn's
``manifold.trustworthiness`` with its mirror image, continuity, without an n x n matrix (``csrc/nn.hip``:
``mmg_nn_search``, ``mmg_nn_rank``).

The result is defined by a total order (``include/mmgnn_nn.h``): the squared distance ``s(q, j) = sum_d (q_d - x_jd)^2`` is
taken in the difference form in float64 from the fp32 inputs, columns ascending; candidates are ordered by the key
``(s, j)`` -- equal sums by the smaller index, a non-finite sum as +inf; a row never lists itself in self mode.
``rank(i, j)`` is j's 1-based position in row i's full order, and the trustworthiness penalty is
``sum max(0, rank(i, j) - k)`` over the k map-neighbours j of every i.

A HIP fp32 tensor runs the kernels and the results stay on the device.  A numpy array (or host tensor) runs the float64
restatement below: that path is the checker and the only one without a GPU.  Only the Euclidean metric is offered; on
unit-norm rows (the initial patient embeddings) the cosine order is the same.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Sequence

import numpy as np
import pandas as pd
import torch

from . import embed, nn_ops

MAX_K = nn_ops.NN_MAX_K      # read from include/mmgnn_nn.h by the binding (the library itself is not loaded for it)
MAX_D = nn_ops.NN_MAX_D
NEIGHBOR_COLUMNS = ["patient_id", "neighbor_id", "rank", "distance"]
LAB_NEIGHBOR_COLUMNS = ["lab_idx", "lab_name", "panel", "rank", "neighbor_idx", "neighbor_name", "neighbor_panel",
                        "distance"]
PURITY_COLUMNS = ["panel", "n_labs", "n_neighbors", "same_panel", "purity"]
MAP_QUALITY_COLUMNS = ["node_type", "method", "n", "n_neighbors", "trustworthiness", "continuity", "overlap"]


@dataclass
class NeighborResult:
    indices: object                          # int64 [nq, k]: device tensor, or numpy on the host path
    distances: object                        # fp32 [nq, k]: the float64 root rounded once


def _rows(x, name: str):
    """-> (a device fp32 tensor or a host fp32 numpy array [n, D], on the device?).  A float64 input (t-SNE's map) is
    rounded once to fp32."""
    if embed._is_dev(x):
        x = x.detach()
        if x.dtype == torch.float64:
            x = x.float()
        if x.dtype != torch.float32:
            raise TypeError(f"{name}: expected torch.float32 (or float64, rounded once) on the device, got {x.dtype}")
        dev = True
    else:
        x = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x)
        if x.dtype.kind != "f":
            raise TypeError(f"{name}: expected a floating-point array, got {x.dtype}")
        x = x.astype(np.float32)
        dev = False
    if x.ndim != 2:
        raise ValueError(f"{name}: expected [n, D] rows, got {x.ndim} dimensions")
    if not 1 <= int(x.shape[1]) <= MAX_D:
        raise ValueError(f"{name}: D = {int(x.shape[1])} outside [1, {MAX_D}]")
    if int(x.shape[0]) < 1:
        raise ValueError(f"{name}: no rows")
    return x, dev


def _check_k(k, n_candidates: int, what: str) -> int:
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"{what}: k = {k} outside [1, {MAX_K}]")
    if k > n_candidates:
        raise ValueError(f"{what}: k = {k} exceeds the {n_candidates} candidates of a query")
    return k


# ---------------------------------------------------------------------------- the float64 host restatement
def sqdist_host(q, x) -> np.ndarray:
    """s[a, j] = sum_d (q[a, d] - x[j, d])^2 in float64 from the widened inputs, columns in ascending order; a
    non-finite sum is +inf."""
    q64, x64 = np.asarray(q, np.float32).astype(np.float64), np.asarray(x, np.float32).astype(np.float64)
    s = np.zeros((q64.shape[0], x64.shape[0]), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(x64.shape[1]):
            df = q64[:, d:d + 1] - x64[None, :, d]
            s += df * df
    s[~np.isfinite(s)] = np.inf
    return s


def _host_blocks(n_rows: int, n_cols: int):
    step = max(1, (1 << 24) // max(n_cols, 1))
    return [(a, min(a + step, n_rows)) for a in range(0, n_rows, step)]


def _order_host(s, first_row: Optional[int]):
    """Every row's candidates in ascending key order (a stable sort of the sums: ties by the smaller index); with
    ``first_row`` (self mode) row a drops candidate first_row + a -> int64 [rows, n or n - 1]."""
    order = np.argsort(s, axis=1, kind="stable")
    if first_row is None:
        return order
    me = np.arange(first_row, first_row + s.shape[0])[:, None]
    return order[order != me].reshape(s.shape[0], s.shape[1] - 1)


def nearest_neighbors_host(x, k: int, queries=None) -> NeighborResult:
    x = np.asarray(x, np.float32)
    q = x if queries is None else np.asarray(queries, np.float32)
    idx = np.empty((q.shape[0], k), np.int64)
    dist = np.empty((q.shape[0], k), np.float32)
    for a, b in _host_blocks(q.shape[0], x.shape[0]):
        s = sqdist_host(q[a:b], x)
        o = _order_host(s, a if queries is None else None)[:, :k]
        idx[a:b] = o
        dist[a:b] = np.sqrt(np.take_along_axis(s, o, axis=1)).astype(np.float32)
    return NeighborResult(idx, dist)


def neighbor_ranks_host(x, neighbors) -> np.ndarray:
    x = np.asarray(x, np.float32)
    nbr = np.asarray(neighbors, np.int64)
    n = x.shape[0]
    out = np.zeros(nbr.shape, np.int32)
    for a, b in _host_blocks(n, n):
        order = _order_host(sqdist_host(x[a:b], x), a)
        pos = np.zeros((b - a, n), np.int32)                      # the row itself keeps 0
        np.put_along_axis(pos, order, np.arange(1, n, dtype=np.int32)[None, :], axis=1)
        j = nbr[a:b]
        ok = (j >= 0) & (j < n)
        out[a:b] = np.where(ok, np.take_along_axis(pos, np.where(ok, j, 0), axis=1), 0)
    return out


# ---------------------------------------------------------------------------- the public calls
def nearest_neighbors(x, k: int, queries=None) -> NeighborResult:
    """The ``k`` nearest rows of ``x`` [n, D] for every query row, in ascending key order (module docstring).
    ``queries=None`` is self mode, ``NearestNeighbors.kneighbors()`` without X: every row of ``x`` queries the others and
    never lists itself (``k <= n - 1``).  With ``queries`` [nq, D] nothing is skipped (``k <= n``): a query equal to a
    row finds it at distance 0.  -> ``NeighborResult(indices int64 [nq, k], distances fp32 [nq, k])``."""
    x, dev = _rows(x, "x")
    n = int(x.shape[0])
    if queries is not None:
        queries, qdev = _rows(queries, "queries")
        if qdev != dev:
            raise ValueError("nearest_neighbors: x and queries must both be on the device or both on the host")
        if int(queries.shape[1]) != int(x.shape[1]):
            raise ValueError(f"nearest_neighbors: queries have {int(queries.shape[1])} columns, x has {int(x.shape[1])}")
    k = _check_k(k, n - 1 if queries is None else n, "nearest_neighbors")
    if dev:
        from . import nn_ops as ops
        dist, idx = ops.nn_search(x, k, queries)
        return NeighborResult(idx, dist)
    return nearest_neighbors_host(x, k, queries)


def neighbor_ranks(x, neighbors):
    """``rank(i, j)`` for ``j = neighbors[i, c]`` (int64 [n, k]): j's 1-based position in row i's full neighbour order
    over ``x``; 0 for an entry that is negative, >= n or i itself -> int32 [n, k]."""
    x, dev = _rows(x, "x")
    n = int(x.shape[0])
    if neighbors.ndim != 2 or int(neighbors.shape[0]) != n:
        raise ValueError(f"neighbor_ranks: neighbors has {tuple(neighbors.shape)} entries for {n} rows of x")
    _check_k(int(neighbors.shape[1]), MAX_K, "neighbor_ranks")
    if dev:
        from . import nn_ops as ops
        if not embed._is_dev(neighbors):
            raise ValueError("neighbor_ranks: x is on the device, neighbors is not")
        return ops.nn_rank(x, neighbors.to(torch.int64), True, False)[0]
    return neighbor_ranks_host(x, neighbors.cpu().numpy() if torch.is_tensor(neighbors) else neighbors)


def _pair(x, y, n_neighbors, what):
    x, dev = _rows(x, "x")
    y, ydev = _rows(y, "y")
    if int(x.shape[0]) != int(y.shape[0]):
        raise ValueError(f"{what}: x has {int(x.shape[0])} rows, y has {int(y.shape[0])}")
    if dev != ydev:
        raise ValueError(f"{what}: x and y must both be on the device or both on the host")
    n, k = int(x.shape[0]), int(n_neighbors)
    if k < 1 or k >= n / 2:
        raise ValueError(f"{what}: n_neighbors ({k}) should be at least 1 and less than n_samples / 2 ({n / 2})")
    if k > MAX_K:
        raise ValueError(f"{what}: n_neighbors = {k} exceeds {MAX_K}")
    return x, y, n, k, dev


def _penalty(x, nbr, dev) -> int:
    if dev:
        from . import nn_ops as ops
        return int(ops.nn_rank(x, nbr, False, True)[1].item())
    k = nbr.shape[1]
    return int(np.maximum(neighbor_ranks_host(x, nbr).astype(np.int64) - k, 0).sum())


def _trust(x, y, n, k, dev) -> float:
    """sklearn's trustworthiness: the ranks in ``x`` of every row's k nearest rows in ``y``."""
    nbr = nearest_neighbors(y, k).indices
    return 1.0 - _penalty(x, nbr, dev) * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)))


def trustworthiness(x, y, n_neighbors: int = 5) -> float:
    """``sklearn.manifold.trustworthiness(x, y, n_neighbors=...)`` (Euclidean): ``1 - 2 / (n k (2n - 3k - 1)) *
    sum_i sum_{j in kNN_y(i)} max(0, rank_x(i, j) - k)`` -- how far the map ``y`` invents neighbours that ``x`` does not
    have.  ``y`` is fp32 [n, 2..] or t-SNE's float64 map, which is rounded once to fp32 first.  ``n_neighbors >= n / 2``
    raises ValueError, as sklearn does."""
    x, y, n, k, dev = _pair(x, y, n_neighbors, "trustworthiness")
    return _trust(x, y, n, k, dev)


def continuity(x, y, n_neighbors: int = 5) -> float:
    """Trustworthiness with ``x`` and ``y`` exchanged: how far the map tears apart neighbours that ``x`` has.  ``y`` as
    for ``trustworthiness`` (a float64 map is rounded once to fp32 first)."""
    x, y, n, k, dev = _pair(x, y, n_neighbors, "continuity")
    return _trust(y, x, n, k, dev)


def _overlap(x, y, n, k) -> float:
    a, b = nearest_neighbors(x, k).indices, nearest_neighbors(y, k).indices
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    b = b.cpu().numpy() if torch.is_tensor(b) else b
    shared = 0
    for lo, hi in _host_blocks(n, k * k):
        shared += int((a[lo:hi, :, None] == b[lo:hi, None, :]).sum())
    return shared / float(n * k)


def neighborhood_overlap(x, y, n_neighbors: int = 5) -> float:
    """The mean over the rows of ``|N_x(i) & N_y(i)| / k``, N the k nearest rows in either space.  ``y`` as for
    ``trustworthiness`` (a float64 map is rounded once to fp32 first)."""
    x, y, n, k, _ = _pair(x, y, n_neighbors, "neighborhood_overlap")
    return _overlap(x, y, n, k)


def map_quality(x, y, n_neighbors: int = 5) -> dict:
    """``{"trustworthiness", "continuity", "overlap"}`` of the map ``y`` of the rows ``x``.  ``y`` may be fp32 [n, 2..8]
    or t-SNE's float64 map; the float64 map is rounded once to fp32 first."""
    x, y, n, k, dev = _pair(x, y, n_neighbors, "map_quality")
    return {"trustworthiness": _trust(x, y, n, k, dev), "continuity": _trust(y, x, n, k, dev),
            "overlap": _overlap(x, y, n, k)}


# ---------------------------------------------------------------------------- over a model's embeddings
def _node_embeddings(model, graph, space: str, who: str):
    if getattr(model, "_comm", None) is not None:
        raise NotImplementedError(f"{who} on a patient-sharded model (dist.shard_model) is not supported: the "
                                  "forward's collectives need every rank; analyse with an unsharded model")
    if space not in ("initial", "final"):
        raise ValueError(f'{who}: space must be "initial" or "final", got {space!r}')
    device = next(model.parameters()).device
    graph_dev = graph.to(device)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            x_dict = model.encode_nodes(graph_dev) if space == "initial" else model(graph_dev)
    finally:
        model.train(was_training)
    return {t: x.detach().float().contiguous() for t, x in x_dict.items()}


def _indexer(graph, node_type):
    ix = getattr(graph, "indexers", None) if hasattr(graph, "indexers") else None
    return ix.get(node_type) if ix else None


def similar_patients(model, graph, patient_ids: Sequence, k: int = 10, space: str = "final") -> pd.DataFrame:
    """The ``k`` patients nearest to each of ``patient_ids`` in the model's embedding space, searched over ALL patients
    of the graph (the patient itself is left out).  Ids go through ``graph.indexers["patient"]`` with the
    ``str(patient_id)`` rule of ``mmgnn.inference``; a graph without indexers takes the ids as node indices.
    ``1 <= k <= MAX_K - 1`` (127): the asked patients are searched as a query set with k + 1 candidates, of which the
    patient itself is dropped, instead of searching every patient of the graph in self mode.
    -> frame (patient_id, neighbor_id, rank 1 .. k, distance), ``len(patient_ids) * k`` rows."""
    x = _node_embeddings(model, graph, space, "similar_patients")["patient"]
    n = int(x.shape[0])
    if not 1 <= int(k) <= MAX_K - 1:
        raise ValueError(f"similar_patients: k = {int(k)} outside [1, {MAX_K - 1}] (one of the {MAX_K} listed candidates "
                         "is the patient itself)")
    k = _check_k(k, n - 1, "similar_patients")
    ix = _indexer(graph, "patient")
    if ix is not None:
        missing = [pid for pid in patient_ids if str(pid) not in ix["id_to_index"]]
        if missing:
            raise KeyError(f"similar_patients: unknown patient ids {missing[:5]}")
        rows = np.array([ix["id_to_index"][str(pid)] for pid in patient_ids], np.int64)
    else:
        rows = np.array([int(pid) for pid in patient_ids], np.int64)
        if rows.size and (rows.min() < 0 or rows.max() >= n):
            raise KeyError(f"similar_patients: patient index outside [0, {n})")
    if rows.size == 0:
        return pd.DataFrame({c: [] for c in NEIGHBOR_COLUMNS}, columns=NEIGHBOR_COLUMNS)
    q = x[torch.from_numpy(rows).to(x.device)].contiguous() if torch.is_tensor(x) else x[rows]
    # k + 1 candidates with nothing skipped, then the patient itself is dropped: the self-mode result of these rows
    res = nearest_neighbors(x, min(k + 1, n), q)
    idx = res.indices.cpu().numpy() if torch.is_tensor(res.indices) else res.indices
    dist = res.distances.cpu().numpy() if torch.is_tensor(res.distances) else res.distances
    out_i, out_d = np.empty((rows.size, k), np.int64), np.empty((rows.size, k), np.float32)
    for a in range(rows.size):
        keep = np.flatnonzero(idx[a] != rows[a])[:k]
        out_i[a], out_d[a] = idx[a][keep], dist[a][keep]
    to_id = (lambda j: ix["index_to_id"][int(j)]) if ix is not None else int
    return pd.DataFrame({"patient_id": [pid for pid in patient_ids for _ in range(k)],
                         "neighbor_id": [to_id(j) for j in out_i.reshape(-1)],
                         "rank": np.tile(np.arange(1, k + 1, dtype=np.int64), rows.size),
                         "distance": out_d.reshape(-1)}, columns=NEIGHBOR_COLUMNS)


def panel_purity(neighbors: pd.DataFrame) -> pd.DataFrame:
    """Per panel and overall ("all"), the share of listed neighbours that lie in the lab's own panel."""
    same = (neighbors["panel"] == neighbors["neighbor_panel"]).to_numpy()
    rows = []
    for panel in sorted(set(neighbors["panel"])):
        m = (neighbors["panel"] == panel).to_numpy()
        rows.append({"panel": panel, "n_labs": int(neighbors.loc[m, "lab_idx"].nunique()), "n_neighbors": int(m.sum()),
                     "same_panel": int(same[m].sum()), "purity": float(same[m].mean())})
    rows.append({"panel": "all", "n_labs": int(neighbors["lab_idx"].nunique()), "n_neighbors": int(same.size),
                 "same_panel": int(same.sum()), "purity": float(same.mean()) if same.size else float("nan")})
    return pd.DataFrame(rows, columns=PURITY_COLUMNS)


def embedding_neighbors(model, graph, space: str = "initial", k: int = 5, output_dir=None, lab_names=None) -> dict:
    """Each lab's ``k`` nearest labs in the model's embedding space, with names and ``embed.lab_panels`` panels, and the
    share of those neighbours that lie in the lab's own panel -- the number behind "labs cluster by clinical function".
    -> {"neighbors": frame (lab_idx, lab_name, panel, rank, neighbor_idx, neighbor_name, neighbor_panel, distance),
    "purity": frame (panel, n_labs, n_neighbors, same_panel, purity), the last row "all"}.  With ``output_dir``:
    ``lab_neighbors.csv`` and ``lab_panel_purity.csv``."""
    x = _node_embeddings(model, graph, space, "embedding_neighbors")["lab"]
    n = int(x.shape[0])
    k = _check_k(k, n - 1, "embedding_neighbors")
    res = nearest_neighbors(x, k)
    idx = res.indices.cpu().numpy() if torch.is_tensor(res.indices) else res.indices
    dist = res.distances.cpu().numpy() if torch.is_tensor(res.distances) else res.distances
    given = embed._names_of(graph, "lab", lab_names)
    names = {i: given.get(i, f"lab_{i}") for i in range(n)}
    panels = embed.lab_panels(names)
    lab = np.repeat(np.arange(n, dtype=np.int64), k)
    nb = idx.reshape(-1)
    frame = pd.DataFrame({"lab_idx": lab, "lab_name": [names[int(i)] for i in lab], "panel": [panels[int(i)] for i in lab],
                          "rank": np.tile(np.arange(1, k + 1, dtype=np.int64), n), "neighbor_idx": nb,
                          "neighbor_name": [names[int(j)] for j in nb], "neighbor_panel": [panels[int(j)] for j in nb],
                          "distance": dist.reshape(-1)}, columns=LAB_NEIGHBOR_COLUMNS)
    out = {"neighbors": frame, "purity": panel_purity(frame)}
    if output_dir is not None:
        d = Path(output_dir)
        d.mkdir(parents=True, exist_ok=True)
        out["neighbors"].to_csv(d / "lab_neighbors.csv", index=False)
        out["purity"].to_csv(d / "lab_panel_purity.csv", index=False)
        logging.info(f"  Saved lab neighbours to {d}")
    return out


def embedding_map_quality(model, graph, space: str = "initial", methods: Sequence[str] = ("pca", "tsne"),
                          n_neighbors: int = 5, max_points: int = 1000, seed: int = 42, output_dir=None) -> pd.DataFrame:
    """Trustworthiness, continuity and neighbourhood overlap of each node type's PCA and t-SNE map against the
    embedding it was made from.  The maps come from ``embed.pca`` (2 components) and ``embed.tsne`` (perplexity
    ``min(30, n - 1)``) as ``embedding_maps`` / ``embedding_tsne`` call them; more than ``max_points`` patients are
    sampled by ``numpy.random.RandomState(seed)`` as ``embedding_tsne`` samples them.  Per type ``n_neighbors`` is cut to
    the largest value below n / 2; a type too small for one neighbour is left out.
    -> frame (node_type, method, n, n_neighbors, trustworthiness, continuity, overlap); with ``output_dir``:
    ``map_quality.csv``."""
    for m in methods:
        if m not in ("pca", "tsne"):
            raise ValueError(f'embedding_map_quality: method must be "pca" or "tsne", got {m!r}')
    if not 4 <= int(max_points) <= embed.TSNE_MAX_N:
        raise ValueError(f"embedding_map_quality: max_points = {max_points} outside [4, {embed.TSNE_MAX_N}]")
    x_dict = _node_embeddings(model, graph, space, "embedding_map_quality")
    rows = []
    for t in embed.VOCAB_TYPES + ("patient",):
        if t not in x_dict:
            continue
        x = x_dict[t]
        if t == "patient" and int(x.shape[0]) > max_points:
            pick = np.random.RandomState(seed).choice(int(x.shape[0]), int(max_points), replace=False)
            x = x[torch.from_numpy(pick).to(x.device)].contiguous()
        n = int(x.shape[0])
        k = min(int(n_neighbors), (n - 1) // 2, MAX_K)           # the largest k < n / 2
        if n < 4 or k < 1:
            continue
        for m in methods:
            y = embed.pca(x, 2).projection if m == "pca" else embed.tsne(x, perplexity=min(30.0, float(n - 1))).embedding
            rows.append({"node_type": t, "method": m, "n": n, "n_neighbors": k, **map_quality(x, y, k)})
    frame = pd.DataFrame(rows, columns=MAP_QUALITY_COLUMNS)
    if output_dir is not None:
        d = Path(output_dir)
        d.mkdir(parents=True, exist_ok=True)
        frame.to_csv(d / "map_quality.csv", index=False)
        logging.info(f"  Saved map quality to {d}")
    return frame
