"""Host side of ``neg_marglik_adj_grad``: candidate pairs, the prelude and scope checks, and the one driver behind the
Kronecker, diagonal and full posteriors' fronts (laplace/kron.py, diag.py, full.py) -- buffers, rank sharding, the all-reduce,
the finish and the candidates' tail.  The device side is csrc/adjgrad.hip and its per-family files."""
from __future__ import annotations

import torch

from . import laplace as _front  # its _dist_info / all_reduce_flat_ are read at call time: the package imports this module


def _adjacency_candidates(eng, candidates, sym: bool):
    """Candidate pairs (i, j) of ``neg_marglik_adj_grad`` -> (a, b, accumulator) in the propagation matrix's coordinates, or
    None.  The device kernels index rows with these pairs: validated before the cast to int32 (one host round trip; this is not
    the per-batch path).  Stored pairs are not candidates: their gradient comes back with the stored entries (a GCN stores its
    diagonal, gnn/models/models.py:23; GraphSAGE's diagonal entries are genuine non-edges of the reference's dense adj.grad,
    gnn/models/models.py:47)."""
    if candidates is None:
        return None
    ci, cj = candidates[0].to(eng.device).to(torch.int64), candidates[1].to(eng.device).to(torch.int64)
    Nn = eng.num_nodes
    if ci.numel():
        if bool(((ci < 0) | (ci >= Nn) | (cj < 0) | (cj >= Nn)).any()):
            raise ValueError(f"candidate pairs must index nodes in [0, {Nn})")
        sr, sc = eng.export_adj()  # row-major sorted
        skey, ckey = sr * Nn + sc, ci * Nn + cj
        pos = torch.searchsorted(skey, ckey).clamp(max=max(skey.numel() - 1, 0))
        if skey.numel() and bool((skey[pos] == ckey).any()):
            raise ValueError("candidate pairs must not be stored entries of the adjacency")
    if sym:  # (adj + adj^T) / 2 feeds the model: both orientations are needed
        ci, cj = torch.cat([ci, cj]), torch.cat([cj, ci])
    # entry (i, j) of the adjacency is entry (a = j, b = i) of the GCN propagation matrix D A^T D and entry
    # (a = i, b = j) of GraphSAGE's A / rowsum
    ca, cb = (cj, ci) if eng.kind == "gcn" else (ci, cj)
    return (ca.to(torch.int32).contiguous(), cb.to(torch.int32).contiguous(),
            torch.zeros(ci.shape[0], dtype=torch.float32, device=eng.device))


def _adjgrad_scope(eng, what: str, depth: bool = False):
    """1-layer models: GCN only (the reference's Banana configurations).  ``depth``: also refuse models deeper than two layers
    here (the Kronecker and diagonal fronts leave that to the device entry points)."""
    if len(eng.dims) == 2 and eng.kind != "gcn":
        raise NotImplementedError(f"{what}: 1-layer GraphSAGE is not covered (1-layer GCN, 2-layer GCN / GraphSAGE)")
    if depth and len(eng.dims) not in (2, 3):
        raise NotImplementedError(f"{what}: 1- and 2-layer GCN / 2-layer GraphSAGE on the HIP backend")


def _dense_scope(eng, what: str):
    """``dense=True`` of ``neg_marglik_adj_grad``: the all-pairs gradient (LoRASTEGCN) covers plain 2-layer GCN models on the
    HIP backend, and N x N floats must fit the workspace limit and int32 indexing."""
    if eng is None or getattr(eng, "kind", None) != "gcn" or eng.num_layers != 2 or eng.has_extras:
        raise NotImplementedError(f"{what}(dense=True): plain 2-layer GCN models (no res / norm) on the HIP backend")
    N = eng.num_nodes
    limit = getattr(eng, "workspace_limit", None)  # (a stand-in engine of the tests has no workspace)
    if N * N >= 2 ** 31 or (limit is not None and 4 * N * N > limit):
        raise NotImplementedError(f"{what}(dense=True): an N x N gradient of {N} nodes exceeds the workspace limit "
                                  f"({limit} bytes) or int32 indexing")


def _adjgrad_prelude(la, name: str, under: str, fitted: bool, prior_precision, candidates, dense: bool, *, batch: str,
                     dense_offered: bool = True, depth: bool = False):
    """What ``neg_marglik_adj_grad`` of posterior ``name`` checks before its own value and weighting: a fit, the prior
    overwrite, the likelihood, an engine with the ``batch`` entry, ``dense`` against ``candidates``, the family.  Returns eng."""
    what = f"adjacency gradient under {under}"
    if not fitted:
        raise AttributeError("Laplace not fitted. Run fit() first.")
    if prior_precision is not None:
        la.prior_precision = prior_precision
    if la.likelihood != "classification":
        raise NotImplementedError("adjacency gradient: classification likelihood")
    if dense and not dense_offered:
        raise NotImplementedError(f"{what}: stored entries and candidates only "
                                  "(dense=True is offered by KronLaplace and DiagLaplace)")
    eng = getattr(la.backend, "engine", None)
    if eng is None or not hasattr(eng, batch) or eng.kind not in ("gcn", "sage"):
        raise NotImplementedError(f"{what}: 2-layer GCN / GraphSAGE on the HIP backend")
    if dense:
        if candidates is not None:
            raise ValueError("dense=True covers every pair: no candidates")
        _dense_scope(eng, f"{name}.neg_marglik_adj_grad")
    _adjgrad_scope(eng, what, depth=depth)
    return eng


def _adjgrad_drive(eng, train_loader, process_group, candidates, sym: bool, dense: bool, *, batch: str, finish: str, weight,
                   per_sample: bool, finish_args=(), **batch_kwargs):
    """Everything of ``neg_marglik_adj_grad`` behind the posterior's own refusals, value and weighting: returns what follows
    the value in its result -- ``(edge_index, grad)``, with candidates also their gradient, or ``(grad [N, N],)`` if ``dense``.

    ``batch`` / ``finish`` name the engine's methods (``dense``: their ``_dense`` forms); ``weight`` is the batch method's
    third argument (the B-factor gradients, gamma or Gamma).  ``per_sample`` is False for the Kronecker posterior -- its B
    factors depend on the batch boundaries, so whole batches are dealt round-robin over the ranks and the finish takes
    ``finish_args`` -- and True for the diagonal and the full posterior, whose terms are sums over samples: every rank takes its
    slice of every batch (a Cora-shaped loader has ONE batch; a candidate pair sees a repeated node id through each slice's own
    multiplicity), and the adjoints ``h1_bar`` / ``e_bar`` travel from the batch calls to the finish."""
    dev, N = eng.device, eng.num_nodes
    out_bar = torch.zeros(N, eng.dims[-1], dtype=torch.float32, device=dev)
    adjoints = []
    if per_sample:  # (a 1-layer model has no hidden layer: the device calls take a null h1_bar)
        adjoints = [torch.zeros(N, eng.dims[1], dtype=torch.float32, device=dev) if len(eng.dims) != 2 else None,
                    torch.zeros(N, eng.dims[0] + 1, dtype=torch.float32, device=dev)]
    if dense:
        target = torch.zeros(N, N, dtype=torch.float32, device=dev)
        cand, batch, finish = None, batch + "_dense", finish + "_dense"
        args, kwargs = (weight, out_bar, *adjoints, target), batch_kwargs
    else:
        target = torch.zeros(eng.nnz, dtype=torch.float32, device=dev)  # d/dP on the stored entries
        cand = _adjacency_candidates(eng, candidates, sym)
        args, kwargs = (weight, target, out_bar, *adjoints), dict(batch_kwargs, cand=cand)
    rank, world = _front._dist_info(process_group)
    if per_sample:
        eng.set_likelihood("classification")
    run = getattr(eng, batch)
    for t, (X, y) in enumerate(train_loader):
        if per_sample:
            M = X.shape[0]
            lo, hi = M * rank // world, M * (rank + 1) // world
            if hi > lo:
                run(X[lo:hi].to(dev), y[lo:hi].to(dev), *args, **kwargs)
        elif t % world == rank:
            run(X.to(dev), y.to(dev), *args, **kwargs)
    if world > 1:
        _front.all_reduce_flat_([b for b in (target, out_bar, *adjoints) if b is not None]
                                + ([cand[2]] if cand is not None else []), process_group)
    done, fin = getattr(eng, finish), (out_bar, *(adjoints if per_sample else finish_args), target)
    if dense:
        return (done(*fin),)
    rows, cols = eng.export_adj()
    if cand is None:
        return torch.stack([rows, cols]), done(*fin)
    grad, gc = done(*fin, cand=cand)
    if sym:
        K = candidates.shape[1]
        gc = 0.5 * (gc[:K] + gc[K:])
    return torch.stack([rows, cols]), grad, gc
