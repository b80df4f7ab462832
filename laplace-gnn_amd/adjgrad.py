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


# ---- propose_edges: the k non-edges the gradient most wants to add, from row bands of the all-pairs gradient -----------------
BAND_TILE = 64  # rows of the tile GEMMs behind a band (csrc/lora.hip: dense_nt_kernel)


def _propose_scope(la, eng, process_group=None):
    """``DiagLaplace.propose_edges`` covers plain directed 2-layer GCN models, ReLU, classification, one process: everything
    else is refused by name.  (A symmetric model's pair (i, j) needs row j and row i of d/dP at once -- a row band and a column
    band; the Kronecker posterior's B factors and GraphSAGE's local chain have no per-row split of the samples.)"""
    what = "propose_edges"
    if la.likelihood != "classification":
        raise NotImplementedError(f"{what}: the regression likelihood is not covered (classification only)")
    kind = getattr(eng, "kind", None)
    if eng is None or not hasattr(eng, "diag_adjgrad_band_sparse") or kind not in ("gcn", "sage"):
        raise NotImplementedError(f"{what}: plain 2-layer GCN models on the HIP backend")
    if kind != "gcn":
        raise NotImplementedError(f"{what}: GraphSAGE models are not covered (plain directed 2-layer GCN only)")
    if eng.num_layers != 2:
        raise NotImplementedError(f"{what}: {eng.num_layers}-layer models are not covered (2 layers only)")
    if eng.has_extras:
        raise NotImplementedError(f"{what}: models with res / norm are not covered (plain 2-layer GCN only)")
    if bool(getattr(la.model, "symmetric", False)) or bool(getattr(eng, "is_symmetric", False)):
        raise NotImplementedError(f"{what}: symmetric models are not covered (a pair needs a row band and a column band at "
                                  "once); symmetric=False only")
    if getattr(eng, "act", "relu") != "relu":
        raise NotImplementedError(f"{what}: the {eng.act} activation is not covered (ReLU only)")
    if _front._dist_info(process_group)[1] > 1:
        raise NotImplementedError(f"{what}: a torch.distributed world larger than 1 is not covered (single process)")


def _band_plan(N: int, band_bytes, workspace_limit):
    """``(height, [(a0, a1), ...])``: the row bands of an N-node graph under ``band_bytes`` (default: the smaller of the
    engine's workspace limit and 1 GiB).  The height is ``band_bytes / (4 N)`` rounded down to whole 64-row tiles -- at least one,
    otherwise ValueError --, the last band is ragged."""
    if band_bytes is None:
        band_bytes = min(int(workspace_limit), 1 << 30) if workspace_limit is not None else 1 << 30
    height = int(band_bytes) // (4 * N) // BAND_TILE * BAND_TILE
    if height < BAND_TILE:
        raise ValueError(f"band_bytes = {int(band_bytes)} holds fewer than one {BAND_TILE}-row tile of a {N}-node graph "
                         f"({4 * N * BAND_TILE} bytes)")
    return height, [(a0, min(a0 + height, N)) for a0 in range(0, N, height)]


def _deal_to_bands(idx: torch.Tensor, height: int, n_bands: int):
    """``(order, counts)``: ``idx[order]`` lists the samples band by band (the loader's order within a band), ``counts[b]`` of
    them in band b.  An id outside the graph goes to the nearest band, whose batch call flags it.  One host round trip."""
    band = torch.div(idx, height, rounding_mode="floor").clamp_(0, n_bands - 1)
    return torch.sort(band, stable=True).indices, torch.bincount(band, minlength=n_bands).tolist()


def _merge_smallest(best, vals, keys, k: int):
    """The k smallest of the running selection and a band's: a fixed order (the running ones first), so two runs agree bit
    for bit."""
    if best is not None:
        vals, keys = torch.cat([best[0], vals]), torch.cat([best[1], keys])
    if vals.numel() > k:
        vals, pick = torch.topk(vals, k, largest=False, sorted=True)
        keys = keys[pick]
    return vals, keys


def _propose_edges_drive(eng, train_loader, k: int, band_bytes, *, weight, loss_scale):
    """Everything of ``DiagLaplace.propose_edges`` behind its refusals and value: ``(pairs [2, k'], grad [k'])``.

    One sparse pass (``diag_adjgrad_band_sparse`` per batch: ``diag_adjgrad_batch`` with every sum in a fixed order, so that two
    calls return the same bits) leaves the adjoints ``out_bar`` / ``h1_bar`` / ``e_bar`` and the batches' part of d/dP on the stored
    entries; ``diag_adjgrad_band_prepare`` completes it and forms the whole-graph operands once.
    The samples are dealt to the bands once; per band the engine adds the per-sample term of its samples and the three bilinear
    terms, turns the band into d/d adj with the stored entries and the diagonal at +inf, and the band's k smallest join the
    running selection (``torch.topk`` on the band in place: no copy of it, index tensors of k entries).  Nothing waits for
    the device between bands; the buffer of one band is the only N-wide allocation."""
    dev, N = eng.device, eng.num_nodes
    height, bands = _band_plan(N, band_bytes, getattr(eng, "workspace_limit", None))
    target = torch.zeros(eng.nnz, dtype=torch.float32, device=dev)
    out_bar = torch.zeros(N, eng.dims[-1], dtype=torch.float32, device=dev)
    h1_bar = torch.zeros(N, eng.dims[1], dtype=torch.float32, device=dev)
    e_bar = torch.zeros(N, eng.dims[0] + 1, dtype=torch.float32, device=dev)
    eng.set_likelihood("classification")
    Xs, ys = [], []
    for X, y in train_loader:
        X, y = X.to(dev).to(torch.int64), y.to(dev)
        if not Xs:
            eng.forward(X[:1].clamp(0, N - 1))  # synchronises the parameter versions: the cached forward is current for the pass
        eng.diag_adjgrad_band_sparse(X, y, weight, target, out_bar, h1_bar, e_bar, loss_scale=loss_scale)
        Xs.append(X)
        ys.append(y)
    prepared = eng.diag_adjgrad_band_prepare(out_bar, h1_bar, e_bar, target)
    idx, y = torch.cat(Xs), torch.cat(ys)
    step = max(X.shape[0] for X in Xs)  # a band's samples go in pieces no larger than the loader's batches
    order, counts = _deal_to_bands(idx, height, len(bands))
    idx, y = idx[order], y[order]
    buf = torch.empty(min(height, N), N, dtype=torch.float32, device=dev)
    best, lo = None, 0
    for (a0, a1), count in zip(bands, counts):
        band = buf[:a1 - a0]
        band.zero_()
        for s in range(lo, lo + count, step):
            e = min(s + step, lo + count)
            eng.diag_adjgrad_band_batch(idx[s:e], y[s:e], weight, a0, a1, band)
        lo += count
        eng.diag_adjgrad_band_finish(out_bar, prepared, e_bar, a0, a1, band)
        flat = band.view(-1)
        vals, q = torch.topk(flat, min(k, flat.numel()), largest=False, sorted=True)
        # band[t, i] is the pair (i, j = a0 + t); key = i N + j
        best = _merge_smallest(best, vals, (q % N) * N + (a0 + torch.div(q, N, rounding_mode="floor")), k)
    vals, keys = best
    keep = torch.isfinite(vals)  # (k beyond the eligible pairs: the masked entries are +inf)
    vals, by_value = torch.sort(vals[keep], stable=True)
    keys = keys[keep][by_value]
    return torch.stack([torch.div(keys, N, rounding_mode="floor"), keys % N]), vals
