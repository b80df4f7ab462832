"""The kNN initial graph of the reference's ``--init_graph knng`` configurations, built on the device.

``get_knn_graph`` (gnn/utils.py:355-369) is ``torch_geometric.nn.knn_graph(X, k, loop=False, cosine=False)``, symmetrised,
with self loops; gnn/marglik_training.py:407-408 hands it to the model.  Here ``lgnn_knn`` (csrc/knn.hip) finds the exact
neighbours without forming N x N distances, and thin tensor code turns them into what the models take:

    nbr, dist = lg.knn(X, k)                 # [N, k] int64 / fp32, ordered by (distance, index)
    ei = lg.knn_graph(X, k)                  # PyG's directed graph: row 0 the neighbour, row 1 the centre
    ei = lg.get_knn_graph(X, k)              # symmetrised, off-diagonal, row-major sorted: feed it to lg.GCN / lg.STEGCN
    cand = lg.knn_candidates(model, X, k)    # the kNN pairs the model's graph does not store: STEGCN(candidates=...)

There is no CPU path: a CPU tensor is refused like everywhere else in the package.  The helpers that only rearrange indices
(``edge_index_from_nbr``, ``symmetrize_edge_index``, ``pairs_not_stored``) are plain tensor code and run anywhere.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

# ---- index helpers (no library involved) ----------------------------------------------------------------------------------
def edge_index_from_nbr(nbr: torch.Tensor) -> torch.Tensor:
    """[N, k] neighbour table -> edge_index [2, N k] in PyG's ``knn_graph`` convention for ``flow="source_to_target"``:
    row 0 the neighbour (source), row 1 the centre (target), centres ascending, a centre's neighbours in table order."""
    N, k = nbr.shape
    centre = torch.arange(N, dtype=torch.int64, device=nbr.device).repeat_interleave(k)
    return torch.stack([nbr.reshape(-1).to(torch.int64), centre])


def symmetrize_edge_index(edge_index: torch.Tensor, num_nodes: int) -> torch.Tensor:
    """``adj_to_edge_index((adj + adj^T).bool())`` of gnn/utils.py:333-336, :361-367 on an edge list: both orientations of
    every pair, duplicates and the diagonal dropped, ``nonzero()`` (row-major) order."""
    N = int(num_nodes)
    a, b = edge_index[0].to(torch.int64), edge_index[1].to(torch.int64)
    keys = torch.cat([a * N + b, b * N + a])
    keys = torch.unique(keys[torch.cat([a != b, a != b])])  # sorted
    return torch.stack([keys // N, keys % N])


def pairs_not_stored(pairs: torch.Tensor, stored_rows: torch.Tensor, stored_cols: torch.Tensor, num_nodes: int,
                     symmetric: bool) -> torch.Tensor:
    """The off-diagonal ``pairs`` [2, n] that a row-major sorted stored pattern does not hold -- the ``searchsorted`` test
    of the adjacency gradient's candidate check.  Deduplicated and sorted; ``symmetric``: a pair counts as stored if either
    orientation is, and one orientation (i < j) per unordered pair is returned."""
    N = int(num_nodes)
    ci, cj = pairs[0].to(torch.int64), pairs[1].to(torch.int64)
    off = ci != cj
    ci, cj = ci[off], cj[off]
    if symmetric:
        ci, cj = torch.minimum(ci, cj), torch.maximum(ci, cj)
    ckey = torch.unique(ci * N + cj)
    skey = stored_rows.to(torch.int64) * N + stored_cols.to(torch.int64)

    def stored(key):
        if not skey.numel():
            return torch.zeros_like(key, dtype=torch.bool)
        pos = torch.searchsorted(skey, key).clamp(max=skey.numel() - 1)
        return skey[pos] == key

    hit = stored(ckey)
    if symmetric:
        hit |= stored((ckey % N) * N + ckey // N)
    ckey = ckey[~hit]
    return torch.stack([ckey // N, ckey % N])


# ---- the device call --------------------------------------------------------------------------------------------------------
def knn(X: torch.Tensor, k: int):
    """Exact k nearest neighbours of every row of ``X`` [N, F] (fp32, on the GPU) by squared Euclidean distance, self
    excluded: ``(nbr int64 [N, k], dist fp32 [N, k])``, per row ordered by (distance, index) with the fp32 difference form
    ``sum_f (x_f - y_f)^2`` as distance.  ``1 <= k <= 32``, ``k < N``.  Rows may be strided (a column slice of a wider
    tensor); anything else is copied.  The call synchronises the current stream once.

    ``knn.last_fallback_rows``: how many rows of the LAST call the Gram-form filter could not certify and the brute-force
    kernel recomputed (0 on ordinary data; the result is exact either way)."""
    if not isinstance(X, torch.Tensor) or X.dim() != 2:
        raise ValueError("X must be a tensor of shape [N, F]")
    if not X.is_cuda:
        raise _lib.HipLibraryError(f"X must live on the GPU (got {X.device}); there is no CPU path")
    if X.dtype != torch.float32:
        raise TypeError(f"X must be torch.float32, got {X.dtype}")
    lib = _lib.load()
    N, F = X.shape
    if F > 0 and not (X.stride(1) == 1 and X.stride(0) >= F):
        X = X.contiguous()
    ld = X.stride(0) if F > 0 and N > 1 else F
    kk = max(int(k), 0)
    nbr = torch.empty(N, kk, dtype=torch.int32, device=X.device)
    dist = torch.empty(N, kk, dtype=torch.float32, device=X.device)
    nfb = C.c_int64(0)
    with torch.cuda.device(X.device):
        stream = C.c_void_p(torch.cuda.current_stream(X.device).cuda_stream)
        rc = lib.lgnn_knn(C.c_void_p(X.data_ptr()), N, F, ld, int(k), C.c_void_p(nbr.data_ptr()),
                          C.c_void_p(dist.data_ptr()), C.byref(nfb), stream)
    _lib.check(rc, "lgnn_knn")
    knn.last_fallback_rows = int(nfb.value)
    return nbr.to(torch.int64), dist


knn.last_fallback_rows = 0


def knn_graph(X: torch.Tensor, k: int) -> torch.Tensor:
    """``torch_geometric.nn.knn_graph(X, k, loop=False, flow="source_to_target", cosine=False)``: edge_index [2, N k], row 0
    the neighbour, row 1 the centre."""
    return edge_index_from_nbr(knn(X, k)[0])


def get_knn_graph(X: torch.Tensor, k: int = 3) -> torch.Tensor:
    """The edge_index of the reference's ``get_knn_graph(X, k, return_edge_index=True)`` (gnn/utils.py:355-369): the kNN
    graph symmetrised, deduplicated, off-diagonal, row-major sorted.  The models add (GCN) or drop (GraphSAGE) the self
    loops themselves, so this is all ``lg.GCN(..., init_adj=...)`` / ``lg.STEGCN`` need."""
    return symmetrize_edge_index(knn_graph(X, k), X.shape[0])


def knn_candidates(model_or_engine, X: torch.Tensor, k: int, symmetric: bool | None = None) -> torch.Tensor:
    """Feature-space neighbours as edge proposals: the kNN pairs of ``X`` that the engine's CURRENT graph does not store,
    int64 [2, n], no diagonal, sorted; for a symmetric model one orientation (i < j) per unordered pair.  Accepted as is
    by ``STEGCN(candidates=...)`` and ``neg_marglik_adj_grad(candidates=...)``.  ``symmetric`` defaults to the model's own
    flag; a bare engine only knows whether its stored pattern equals its transpose, which is what is used then."""
    eng = getattr(model_or_engine, "engine", model_or_engine)
    if symmetric is None:
        symmetric = getattr(model_or_engine, "symmetric", None)
    if symmetric is None:
        symmetric = eng.is_symmetric
    if X.shape[0] != eng.num_nodes:
        raise ValueError(f"X has {X.shape[0]} rows, the graph {eng.num_nodes} nodes")
    pairs = knn_graph(X.to(eng.device), k)
    rows, cols = eng.export_adj()  # row-major sorted
    return pairs_not_stored(pairs, rows, cols, eng.num_nodes, bool(symmetric))
