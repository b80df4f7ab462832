"""Drop-in model modules: ``GCN`` and ``GraphSAGE`` with the reference's constructor signature,
parameter names (``convs.{i}.lin.weight|bias``) and ``forward(x_indices) -> [M, C]`` contract
(gnn/models/base_gnn.py:11-161, gnn/models/models.py:14-62, gnn/models/layers.py:5-46), but a
sparse adjacency held by the HIP engine instead of a dense N x N ``nn.Parameter``.

Inference (eval mode) runs on the GPU through the C ABI, and so does training: in ``train()`` mode with grad enabled
``forward`` is a ``torch.autograd.Function`` over ``lgnn_train_forward`` / ``lgnn_train_backward`` (csrc/train.hip), so the
driver's weight update (gnn/marglik_training.py:165-186: ``f = model(idx); loss.backward(); optimizer.step()``) runs
unchanged with any ``torch.optim`` optimizer.  Dropout masks are drawn with torch on the model's device
(``torch.manual_seed`` governs them; the reference's random stream is not reproduced) or injected with
``set_dropout_masks``; ``norm="batch"`` in training mode is not supported.  ``res=True`` (``res.{i}`` Linears, base_gnn.py:97-113) and
``norm="layer"|"batch"`` (``norms.{i}``, base_gnn.py:86-95) are part of the HIP forward / backward (csrc/resnorm.hip).
Neighbour sampling (``num_sampled_nodes_per_hop``) needs an explicit ``sample_seed`` (the reference's sampler is unseeded).
"""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import nn

from .engine import GraphEngine


class _TrainForward(torch.autograd.Function):
    """``BaseGNN.forward`` in training mode: logits from ``lgnn_train_forward``, parameter gradients from
    ``lgnn_train_backward`` (one tape per engine; no double backward).  ``params`` are the model's bound parameters in
    ``named_parameters()`` order without the ``adj*`` ones -- the order ``GraphEngine.train_backward`` returns."""

    @staticmethod
    def forward(ctx, engine, idx, masks, p, *params):
        out = engine.train_forward(idx, masks, p)
        ctx.engine, ctx.token = engine, engine.train_token
        ctx.keep = (idx, masks)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        grads = ctx.engine.train_backward(grad_out, ctx.token)
        return (None, None, None, None, *grads)


class _Conv(nn.Module):
    """Holds the ``lin`` of GCNConv / GraphSAGEConv (layers.py:5-46) so parameter names match."""

    def __init__(self, in_channels: int, out_channels: int, mult: int):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin = nn.Linear(mult * in_channels, out_channels, bias=True)

    def reset_parameters(self):
        self.lin.reset_parameters()


def _to_edge_index(init_adj: torch.Tensor) -> torch.Tensor:
    """Dense 0/1 (or counted) adjacency -> COO.  Values > 1 are clamped like
    gnn/marglik_training.py:405 by the engine's deduplication."""
    if init_adj.dim() == 2 and init_adj.shape[0] == 2 and init_adj.dtype == torch.int64 and init_adj.shape[1] != 2:
        return init_adj
    if init_adj.dim() != 2 or init_adj.shape[0] != init_adj.shape[1]:
        raise ValueError("init_adj must be a dense [N, N] matrix or an int64 edge_index [2, E]")
    if not torch.all((init_adj == 0) | (init_adj == 1)):
        raise AssertionError("adjacency must be binary (gnn/models/base_gnn.py:73)")
    return init_adj.nonzero().t().contiguous()


class BaseGNN(nn.Module):
    kind = "gcn"
    _mult = 1

    def __init__(self, in_channels: int, hidden_channels: int, out_channels: int, num_layers: int,
                 X: torch.Tensor, init_adj: torch.Tensor, dropout_p: float = 0.5, act: Optional[str] = "relu",
                 act_kwargs=None, update_adj: bool = False, norm: Optional[str] = None, res: bool = False,
                 symmetric: bool = False, **kwargs):
        super().__init__()
        if norm not in (None, "none", "layer", "batch"):
            raise ValueError(f"Unknown normalization type: {norm}")  # base_gnn.py:94-95
        if update_adj:
            raise NotImplementedError("adjacency learning (STE variants) is out of scope")
        if act not in ("relu", "tanh"):
            raise NotImplementedError(f"activation {act!r} is not supported (relu, tanh)")
        if act_kwargs:
            raise NotImplementedError("act_kwargs are not supported")
        if num_layers < 1:
            raise ValueError("num_layers must be >= 1")
        self.X = X
        self.symmetric = symmetric
        self.in_channels, self.hidden_channels = in_channels, hidden_channels
        self.out_channels, self.num_layers = out_channels, num_layers
        self.act_name = act
        self.dropout = nn.Dropout(p=dropout_p)  # identity in eval mode, kept for interface parity
        self.register_buffer("edge_index", _to_edge_index(init_adj).to(torch.int64), persistent=False)
        self.num_nodes = X.shape[0]
        dims = [in_channels] + [hidden_channels] * (num_layers - 1) + [out_channels]
        # registration order as in the reference (base_gnn.py:94-98: norms, convs, res) -- it is the order of
        # named_parameters(), hence of the Laplace parameter vector: convs.* first, then res.* (norms.* are filtered out)
        self.norm_kind = None if norm in (None, "none") else norm
        if self.norm_kind == "layer":
            make_norm = lambda: nn.LayerNorm(hidden_channels)  # noqa: E731
        elif self.norm_kind == "batch":
            make_norm = lambda: nn.BatchNorm1d(hidden_channels)  # noqa: E731
        else:
            make_norm = nn.Identity
        self.norms = nn.ModuleList(make_norm() for _ in range(num_layers - 1))
        self.convs = nn.ModuleList(_Conv(dims[i], dims[i + 1], self._mult) for i in range(num_layers))
        # x = res[i](x) + convs[i](adj, x) for every hidden layer (base_gnn.py:100-113, 141-144)
        self.res = nn.ModuleList(nn.Linear(dims[i], hidden_channels) for i in range(num_layers - 1)) if res else nn.ModuleList()
        self._engine: GraphEngine | None = None

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """Checkpoints of the reference carry the graph as the dense ``adj`` parameter (gnn/models/base_gnn.py:75-76; the driver
        insists on the key, gnn/marglik_training.py:78-79; a GCN's holds its self loops, gnn/models/models.py:23).  Here the
        graph is the ``edge_index`` buffer of the HIP engine: an ``adj`` entry -- dense [N, N] or a sparse COO / CSR tensor,
        0/1 or the continuous values of an STE model, which propagate with ``adj > threshold`` (models.py:99-101) -- is turned
        into it (and dropped from the dict so that ``strict`` loading does not trip over it); the engine is rebuilt lazily."""
        key = prefix + "adj"
        if key in state_dict and not isinstance(getattr(self, "adj", None), nn.Parameter):
            adj = state_dict.pop(key)
            thr = float(getattr(self, "threshold", 0.0))
            if adj.layout != torch.strided:
                adj = adj.to_sparse_coo().coalesce()
                ei = adj.indices()[:, adj.values() > thr]
            else:
                if adj.dim() != 2 or adj.shape[0] != adj.shape[1] or adj.shape[0] != self.num_nodes:
                    error_msgs.append(f"adj has shape {tuple(adj.shape)}, expected ({self.num_nodes}, {self.num_nodes})")
                    ei = None
                else:
                    ei = (adj > thr).nonzero().t()
            if ei is not None:
                self.edge_index = ei.to(torch.int64).contiguous().to(self.edge_index.device)
                self._engine = None
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        self.X = fn(self.X)
        self._engine = None  # device may have changed; rebuilt lazily
        return self

    @property
    def engine(self) -> GraphEngine:
        """The HIP context for this model (graph ingested once, parameters bound by pointer)."""
        dev = self.convs[0].lin.weight.device
        if self._engine is None:
            if dev.type != "cuda":
                raise RuntimeError("the HIP engine needs the model on a GPU: call model.to('cuda') first "
                                   "(there is no CPU fallback)")
            eng = GraphEngine(self.edge_index.to(dev), self.num_nodes, kind=self.kind, symmetric=self.symmetric)
            eng.bind(self.X.to(dev).contiguous(), [c.lin.weight for c in self.convs],
                     [c.lin.bias for c in self.convs], act=self.act_name, **self._extras())
            self._engine = eng
        return self._engine

    def _extras(self) -> dict:
        """``res`` / ``norm`` state for ``GraphEngine.bind`` (borrowed tensors; BatchNorm runs on its running statistics:
        Laplace.fit calls model.eval(), laplace/baselaplace.py:805)."""
        kw = {}
        if len(self.res):
            kw["res_weights"], kw["res_biases"] = [m.weight for m in self.res], [m.bias for m in self.res]
        if self.norm_kind is not None and len(self.norms):
            kw.update(norm=self.norm_kind, norm_eps=float(self.norms[0].eps), norm_weight=[m.weight for m in self.norms],
                      norm_bias=[m.bias for m in self.norms])
            if self.norm_kind == "batch":
                kw.update(norm_mean=[m.running_mean for m in self.norms], norm_var=[m.running_var for m in self.norms])
        return kw

    def full_adj(self) -> torch.Tensor:
        """Dense 0/1 adjacency as the reference's ``model.adj`` holds it (small graphs only)."""
        rows, cols = self.engine.export_adj()
        adj = torch.zeros(self.num_nodes, self.num_nodes, device=rows.device)
        adj[rows, cols] = 1
        return adj

    @property
    def n_outputs(self) -> int:
        """Width of the logits: Laplace.fit reads it instead of running the one-sample forward pass the reference uses to
        find it (laplace/baselaplace.py:806-816)."""
        return self.out_channels

    def forward_adj(self) -> torch.Tensor:
        """Propagation matrix as a sparse COO tensor (normalize_adj / mean_agg result)."""
        r, c, v = self.engine.export_propagation()
        return torch.sparse_coo_tensor(torch.stack([r, c]), v, (self.num_nodes, self.num_nodes))

    def set_dropout_masks(self, masks):
        """Inject the dropout masks of the NEXT training-mode forward call instead of drawing them: one entry per hidden
        layer, ``[num_nodes, hidden]`` each, non-zero = kept (bool / uint8 / the 0-1 pattern of a float mask); kept
        activations are scaled by ``1 / (1 - dropout.p)`` as usual.  Used once, then drawing resumes; ``None`` cancels."""
        if masks is None:
            self._next_masks = None
            return
        masks = list(masks)
        if len(masks) != self.num_layers - 1:
            raise ValueError(f"need one dropout mask per hidden layer ({self.num_layers - 1}), got {len(masks)}")
        for l, m in enumerate(masks):
            if not isinstance(m, torch.Tensor) or tuple(m.shape) != (self.num_nodes, self.hidden_channels):
                raise ValueError(f"dropout mask {l} must be a tensor of shape {(self.num_nodes, self.hidden_channels)}")
        self._next_masks = [(m != 0).to(torch.uint8) for m in masks]

    def _train_params(self):
        """The engine's parameters in named_parameters() order (norms, convs, res); ``adj*`` belongs to the graph."""
        ps = []
        if self.norm_kind == "layer":
            for m in self.norms:
                ps += [m.weight, m.bias]
        for c in self.convs:
            ps += [c.lin.weight, c.lin.bias]
        for m in self.res:
            ps += [m.weight, m.bias]
        return ps

    def _dropout_masks(self, dev):
        """uint8 keep-masks of one training forward: the injected ones, or one draw per hidden layer with keep-probability
        ``1 - p`` from torch's generator of the model's device; ``None`` when nothing is dropped."""
        given = getattr(self, "_next_masks", None)
        self._next_masks = None
        if given is not None:
            return [m.to(dev).contiguous() for m in given]
        p = float(self.dropout.p)
        if p <= 0.0 or self.num_layers < 2:
            return None
        return [(torch.rand(self.num_nodes, self.hidden_channels, device=dev) >= p).to(torch.uint8)
                for _ in range(self.num_layers - 1)]

    def forward(self, x_indices: torch.Tensor) -> torch.Tensor:
        dev = self.convs[0].lin.weight.device
        if self.training and torch.is_grad_enabled():
            if self.norm_kind == "batch":
                raise NotImplementedError("norm='batch' in training mode (batch statistics, running-stat update) is not "
                                          "supported on the HIP path")
            p = float(self.dropout.p)
            if p >= 1.0:
                raise NotImplementedError("dropout_p must be below 1")
            eng = self.engine
            return _TrainForward.apply(eng, x_indices.to(dev), self._dropout_masks(dev), p, *self._train_params())
        if self.training and (self.dropout.p > 0 or self.norm_kind == "batch"):
            raise NotImplementedError("a training-mode forward under no_grad has no HIP path: call model.eval() "
                                      "(Laplace.fit does) or enable grad")
        return self.engine.forward(x_indices.to(dev))


class GCN(BaseGNN):
    """gnn/models/models.py:14-34 (self loops added, D^-1/2 A^T D^-1/2 propagation)."""
    kind = "gcn"
    _mult = 1


class GraphSAGE(BaseGNN):
    """gnn/models/models.py:37-62.  ``num_sampled_nodes_per_hop=k``: the reference multiplies the adjacency by a fresh random
    subgraph -- at most k of every row's neighbours, ``torch.randperm`` from the GLOBAL, unseeded generator -- on EVERY call of
    ``forward_adj`` (gnn/models/utils.py:115-131; its ``seed`` argument is commented out), so the three forward passes and the
    backward passes of one KFAC batch each see a different graph and no two runs agree: there is nothing to pin.  Here the draw
    is explicit: ``sample_seed`` (required with k) selects ONE subgraph -- every row keeps ``min(deg, k)`` of its neighbours,
    uniformly, from a generator seeded with it -- that all passes of a fit share; ``resample(seed)`` draws another.  The sampled
    graph is directed (a row's choice is its own), whatever ``symmetric`` says about the full one.  Parity unpinned by
    construction (tests hold the distributional properties and the equality with a model built on the sampled edge list)."""
    kind = "sage"
    _mult = 2

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, X, init_adj,
                 num_sampled_nodes_per_hop=None, sample_seed=None, **kwargs):
        if num_sampled_nodes_per_hop is not None:
            if sample_seed is None:
                raise NotImplementedError("neighbour sampling: the reference's sampler is unseeded (a new graph per forward "
                                          "call); pass sample_seed=<int> for one seeded draw per fit")
            if int(num_sampled_nodes_per_hop) < 1:
                raise ValueError("num_sampled_nodes_per_hop must be >= 1")
        super().__init__(in_channels, hidden_channels, out_channels, num_layers, X, init_adj, **kwargs)
        self.num_sampled_nodes_per_hop = None if num_sampled_nodes_per_hop is None else int(num_sampled_nodes_per_hop)
        self.sample_seed = sample_seed

    def resample(self, seed: int):
        """Draw another subgraph (the engine is rebuilt on next use; fitted posteriors belong to the previous graph)."""
        self.sample_seed = int(seed)
        self._engine = None

    def sampled_edge_index(self, device) -> torch.Tensor:
        """The seeded draw: [2, E'] int64, row-major sorted, at most k entries per row of the full 0/1 adjacency."""
        full = GraphEngine(self.edge_index.to(device), self.num_nodes, kind=self.kind, symmetric=self.symmetric)
        rows, cols = full.export_adj()
        full.close()
        gen = torch.Generator(device="cpu").manual_seed(int(self.sample_seed))
        key = torch.rand(rows.numel(), generator=gen).to(device)
        order = torch.argsort(key)                       # random order ...
        order = order[torch.argsort(rows[order], stable=True)]  # ... within every row
        r_sorted = rows[order]
        start = torch.searchsorted(r_sorted, r_sorted)  # first position of the entry's row
        keep = (torch.arange(rows.numel(), device=device) - start) < self.num_sampled_nodes_per_hop
        sel = torch.sort(order[keep]).values             # back to row-major order
        return torch.stack([rows[sel], cols[sel]]).contiguous()

    @property
    def engine(self) -> GraphEngine:
        if self.num_sampled_nodes_per_hop is None:
            return BaseGNN.engine.fget(self)
        dev = self.convs[0].lin.weight.device
        if self._engine is None:
            if dev.type != "cuda":
                raise RuntimeError("the HIP engine needs the model on a GPU: call model.to('cuda') first "
                                   "(there is no CPU fallback)")
            eng = GraphEngine(self.sampled_edge_index(dev), self.num_nodes, kind=self.kind, symmetric=False)
            eng.bind(self.X.to(dev).contiguous(), [c.lin.weight for c in self.convs],
                     [c.lin.bias for c in self.convs], act=self.act_name, **self._extras())
            self._engine = eng
        return self._engine


class _TrackedAdjacency:
    """What ``STEGCN`` and ``STEGraphSAGE`` share: a continuous ``adj`` parameter on the TRACKED pairs only -- the stored
    entries of the initial graph (1) and the caller's ``candidates`` (0), named by ``adj_index`` [2, n] (row-major sorted,
    both orientations for a symmetric model) -- with the binarised graph held by the HIP engine.  ``_track_diagonal`` says
    whether pairs ``(i, i)`` may be tracked (GraphSAGE: the diagonal is a learnable entry) or are dropped (GCN: the forward
    overwrites it)."""
    _track_diagonal = False
    _train_pair_grad = 0.1  # ``grad_adj_mask`` between two training nodes under ``train_masked_update`` (STEGCN's soft mask)
    _is_train = None  # bool [N] of ``train_nodes``, kept for ``add_candidates`` (set by ``_train_pair_mask``)

    def _track(self, candidates):
        """Registers ``adj_index`` and ``adj`` from the model's ``edge_index`` buffer and the candidate pairs."""
        N = self.num_nodes

        def pattern(pairs):
            k = pairs[0] * N + pairs[1]
            if self.symmetric:
                k = torch.cat([k, pairs[1] * N + pairs[0]])
            if not self._track_diagonal:
                k = k[(k // N) != (k % N)]
            return torch.unique(k)

        ei = self.edge_index.cpu()
        if self._track_diagonal:  # the initial graph itself has none (gnn/models/models.py:135)
            ei = ei[:, ei[0] != ei[1]]
        keys = pattern(ei)  # the stored pattern (duplicates clamp to one entry)
        vals = torch.ones(keys.numel())
        if candidates is not None and candidates.numel():
            ck = pattern(candidates.cpu().to(torch.int64))
            ck = ck[~torch.isin(ck, keys)]
            keys, order = torch.sort(torch.cat([keys, ck]))
            vals = torch.cat([vals, torch.zeros(ck.numel())])[order]
        self.register_buffer("adj_index", torch.stack([keys // N, keys % N]))
        self.adj = nn.Parameter(vals)  # (the Laplace parameter filter drops names containing 'adj', baselaplace.py:118-122)

    def _train_pair_mask(self, train_nodes) -> torch.Tensor:
        """bool [n]: the tracked pair joins two training nodes (gnn/models/utils.py:19-22)."""
        is_train = torch.zeros(self.num_nodes, dtype=torch.bool)
        is_train[torch.as_tensor(train_nodes).cpu().to(torch.int64)] = True
        self._is_train = is_train
        return is_train[self.adj_index[0]] & is_train[self.adj_index[1]]

    @torch.no_grad()
    def add_candidates(self, pairs) -> int:
        """Track the listed pairs ``[2, K]`` that are not tracked yet, with value 0 (implicit non-edges become explicit ones):
        ``adj_index`` / ``adj`` grow, existing values and the row-major order are kept, pairs ``(i, i)`` are dropped where the
        diagonal is not tracked (GCN), a symmetric model tracks both orientations, and ``grad_adj_mask`` is rebuilt under
        ``train_masked_update``.  Returns the number of entries added.  ``adj`` becomes a NEW ``nn.Parameter`` (without a
        ``.grad``): the caller rebuilds ``adj_optimizer`` over it.  With ``DiagLaplace.propose_edges`` the loop at scale reads

            la.fit(loader); _, pairs, grad = la.propose_edges(loader, k)
            model.add_candidates(pairs[:, grad < -threshold / lr_adj]); adj_optimizer = SGD([model.adj], lr_adj)
            model.adj_backward(la, loader); adj_optimizer.step(); model.apply_adj()"""
        N, dev = self.num_nodes, self.adj.device
        pairs = torch.as_tensor(pairs).to(dev, torch.int64).reshape(2, -1)
        if pairs.numel() and bool(((pairs < 0) | (pairs >= N)).any()):
            raise ValueError(f"candidate pairs must index nodes in [0, {N})")
        k = pairs[0] * N + pairs[1]
        if self.symmetric:
            k = torch.cat([k, pairs[1] * N + pairs[0]])
        if not self._track_diagonal:
            k = k[(k // N) != (k % N)]
        keys = self._keys().to(dev)
        k = torch.unique(k)
        k = k[~torch.isin(k, keys)]
        if not k.numel():
            return 0
        keys, order = torch.sort(torch.cat([keys, k]))
        vals = torch.cat([self.adj.detach(), torch.zeros(k.numel(), dtype=self.adj.dtype, device=dev)])[order]
        self.adj_index = torch.stack([keys // N, keys % N])
        self.adj = nn.Parameter(vals)
        if self.train_masked_update:
            is_train = self._is_train.to(dev)
            both = is_train[self.adj_index[0]] & is_train[self.adj_index[1]]
            self.grad_adj_mask = torch.where(both, self._train_pair_grad, 1.0).to(vals.dtype)
        return int(k.numel())

    def _keys(self) -> torch.Tensor:
        return self.adj_index[0] * self.num_nodes + self.adj_index[1]

    def _effective(self) -> torch.Tensor:
        """What is thresholded: the values, or (adj + adj^T) / 2 of a symmetric model (models.py:105-106, 162-163)."""
        v = self.adj.detach()
        if not self.symmetric:
            return v
        keys = self._keys()
        tpos = torch.searchsorted(keys, self.adj_index[1] * self.num_nodes + self.adj_index[0])
        return 0.5 * (v + v[tpos])  # (the tracked pattern of a symmetric model contains both orientations)

    def _tracked_dense(self) -> torch.Tensor:
        out = torch.zeros(self.num_nodes, self.num_nodes, device=self.adj.device)
        out[self.adj_index[0], self.adj_index[1]] = self.adj.detach()
        return out

    # -- the structure-learning step -----------------------------------------------------------------------------------
    @torch.no_grad()
    def adj_backward(self, la, train_loader, process_group=None):
        """``neg_marglik.backward()`` of the loop (gnn/marglik_training.py:212-216): ``adj.grad`` <- the gradient of the fitted
        posterior's negative log marginal likelihood w.r.t. the tracked entries, through the normalisation of the propagation
        matrix (a GCN's overwritten diagonal included), the STE (identity times ``grad_adj_mask``, gnn/models/utils.py:67-71)
        and the symmetric parameterisation.  Accumulates into an existing ``.grad`` like autograd does.  Returns the negative
        log marginal likelihood."""
        eng = self.engine
        keys = self._keys()
        sr, sc = eng.export_adj()
        skeys = sr * self.num_nodes + sc
        stored = torch.isin(keys, skeys)  # tracked pairs the engine currently stores
        ci, cj = self.adj_index[0][~stored], self.adj_index[1][~stored]
        if self.symmetric:  # one orientation per unordered pair: the call returns the symmetrised value for both
            half = ci <= cj
            ci, cj = ci[half], cj[half]
        cand = torch.stack([ci, cj]) if ci.numel() else None
        res = la.neg_marglik_adj_grad(train_loader, process_group=process_group, candidates=cand)
        value, _, gs = res[0], res[1], res[2]
        g = torch.zeros_like(self.adj)
        pos = torch.searchsorted(keys, skeys).clamp(max=max(keys.numel() - 1, 0))
        hit = keys[pos] == skeys  # (a GCN's diagonal and untracked stored pairs -- none by construction -- are skipped)
        g[pos[hit]] = gs[hit]
        if cand is not None:
            gc = res[3]
            ckeys = ci * self.num_nodes + cj
            g[torch.searchsorted(keys, ckeys)] = gc
            if self.symmetric:
                g[torch.searchsorted(keys, cj * self.num_nodes + ci)] = gc
        if self.train_masked_update:
            g = g * self.grad_adj_mask
        self.adj.grad = g if self.adj.grad is None else self.adj.grad + g
        return value

    @torch.no_grad()
    def apply_adj(self) -> int:
        """After ``adj_optimizer.step()``: re-binarise the tracked values (``> threshold``, models.py:103-116, 160-180) and flip
        the entries of the engine's graph whose side changed.  Returns the number of directed entries flipped."""
        eng = self.engine
        want = self._effective() > self.threshold
        sr, sc = eng.export_adj()
        have = torch.isin(self._keys(), sr * self.num_nodes + sc)
        flip = want != have
        n = int(flip.sum())
        if n:
            eng.update_adjacency(self.adj_index[0][flip], self.adj_index[1][flip], want[flip])
            self._graph_edited(eng)
        return n

    def _graph_edited(self, eng):
        """The buffer the engine is rebuilt from (``.to()`` / ``_apply``) follows the engine's graph."""
        self.edge_index = eng.adj_to_edge_index()


class STEGCN(_TrackedAdjacency, GCN):
    """The reference's structure-learning model (gnn/models/models.py:65-118) on a sparse pattern.

    The reference keeps a dense continuous ``adj`` parameter [N, N] (initialised with the 0/1 adjacency and the GCN's self
    loops), propagates with ``normalize_adj(fill_diagonal_(BinarizeSTE(adj) , 1))`` -- symmetric models binarise
    ``(adj + adj^T) / 2`` -- and lets ``neg_marglik.backward()`` / ``adj_optimizer.step()`` move every entry
    (gnn/marglik_training.py:197-224).  Here ``adj`` holds the continuous values of the TRACKED pairs only: the stored
    off-diagonal entries (1) and the caller's ``candidates`` (0), ``adj_index`` [2, n] names them (row-major sorted); every
    other pair stays an implicit non-edge with value 0.  The diagonal is not tracked: the forward overwrites it and its
    gradient is zero (models.py:114).  The binarised graph lives in the HIP engine; after an optimizer step ``apply_adj()``
    re-thresholds the values and hands the entries that changed side to ``lgnn_update_adjacency`` (no re-ingest).

        la.fit(loader)
        model.adj_backward(la, loader)        # adj.grad <- d(-marglik)/d adj   (neg_marglik.backward())
        adj_optimizer.step(); model.apply_adj()
        la.fit(loader)                        # the loop of gnn/marglik_training.py:211-224

    With every non-edge listed as a candidate this reproduces the reference's loop (tests/golden/steloop_*.npz); with a
    subset, ``clip_grad_norm_`` and the optimizer only see the tracked entries.  ``sign_grad=True`` is refused: the
    reference takes the sign of the gradient of every forward CALL (the curvature graph and the loss forward of each batch)
    and autograd sums the signs, which no accumulated gradient reproduces."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, X, init_adj, dropout_p: float = 0.5,
                 act="relu", act_kwargs=None, threshold: float = 0.5, train_masked_update: bool = False, train_nodes=None,
                 symmetric: bool = False, sign_grad: bool = False, candidates: Optional[torch.Tensor] = None, **kwargs):
        if sign_grad:
            raise NotImplementedError("sign_grad=True: the reference sums the signs of per-forward-call gradients "
                                      "(gnn/models/utils.py:75-76); not reproducible from one accumulated gradient")
        if train_masked_update and train_nodes is None:
            raise ValueError("'train_nodes' must be provided, to use train_masked_update.")  # models.py:91-93
        kwargs.pop("update_adj", None)
        super().__init__(in_channels, hidden_channels, out_channels, num_layers, X, init_adj, dropout_p=dropout_p, act=act,
                         act_kwargs=act_kwargs, symmetric=symmetric, **kwargs)
        self.threshold = float(threshold)
        self.sign_grad = False
        self.train_masked_update = bool(train_masked_update)
        self._track(candidates)
        if self.train_masked_update:
            # soft mask of BinarizeSTE (models.py:94-98): 0.1 between two training nodes, 1 elsewhere
            both = self._train_pair_mask(train_nodes)
            self.register_buffer("grad_adj_mask", torch.where(both, torch.tensor(0.1), torch.tensor(1.0)))

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """A reference checkpoint's dense ``adj`` [N, N] (continuous values) is reduced to the tracked pairs, and the engine's
        graph to its binarisation; this module's own checkpoints hold the tracked values as they are."""
        key = prefix + "adj"
        adj = state_dict.get(key)
        if adj is not None and adj.dim() == 2:
            if tuple(adj.shape) != (self.num_nodes, self.num_nodes):
                error_msgs.append(f"adj has shape {tuple(adj.shape)}, expected ({self.num_nodes}, {self.num_nodes})")
            else:
                dense = adj.to(torch.float32)
                ai = self.adj_index.to(dense.device)
                state_dict[key] = dense[ai[0], ai[1]]
                eff = 0.5 * (dense + dense.T) if self.symmetric else dense
                on = eff > self.threshold
                on.fill_diagonal_(False)
                self.edge_index = on.nonzero().t().to(torch.int64).contiguous().to(self.edge_index.device)
                self._engine = None
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def full_adj(self) -> torch.Tensor:
        """Dense binarised adjacency (models.py:99-101, with the propagated self loops), small graphs only."""
        return super().full_adj()

    def dense_adj(self) -> torch.Tensor:
        """The continuous parameter as the reference stores it (dense [N, N], untracked pairs 0, diagonal 1): small graphs."""
        out = self._tracked_dense()
        out.fill_diagonal_(1.0)
        return out


class STEGraphSAGE(_TrackedAdjacency, GraphSAGE):
    """The reference's GraphSAGE structure-learning model (gnn/models/models.py:121-183) on a sparse pattern: ``STEGCN``'s loop
    with mean aggregation ``P = A / max(rowsum, 1)`` (gnn/models/layers.py:18-24) and a LEARNABLE diagonal.

    The reference zeroes the diagonal of its dense ``adj`` once, in the constructor (models.py:135); its ``forward_adj``
    binarises ``adj`` -- ``(adj + adj^T) / 2`` of a symmetric model -- and never overwrites the diagonal again (models.py:160-180,
    against :114 of STEGCN).  So ``adj[i, i]`` is an ordinary entry: once it crosses the threshold node ``i`` averages over
    itself as well.  Here the engine is built with ``self_loops=True`` and ``candidates`` may list pairs ``(i, i)``, tracked like
    any other; entry ``(i, j)`` of ``adj`` is entry ``(a = i, b = j)`` of the propagation matrix.  With every pair listed --
    the stored entries, every non-edge and the diagonal, ``adj.numel() == N * N`` -- this reproduces the reference's loop
    (tests/golden/sageloop/steloop_sage_*.npz).

    ``train_masked_update``: the gradient mask is the hard one of ``train_adj_mask`` (models.py:152-154) -- 0 between two
    training nodes, ``(t, t)`` included, 1 elsewhere -- not STEGCN's 0.1.  ``num_sampled_nodes_per_hop`` is accepted and unused,
    as in the reference (its sampling line is commented out, models.py:174-177).  Plain 2-layer models only: ``sign_grad=True``,
    ``res=True``, a ``norm`` and other depths are refused here, as the adjacency gradient refuses them."""
    _track_diagonal = True
    _train_pair_grad = 0.0  # the hard mask of ``train_adj_mask``

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, X, init_adj, num_sampled_nodes_per_hop=None,
                 dropout_p: float = 0.5, act="relu", act_kwargs=None, threshold: float = 0.5, train_masked_update: bool = False,
                 train_nodes=None, symmetric: bool = False, sign_grad: bool = False, candidates: Optional[torch.Tensor] = None,
                 **kwargs):
        if sign_grad:
            raise NotImplementedError("sign_grad=True: the reference sums the signs of per-forward-call gradients "
                                      "(gnn/models/utils.py:75-76); not reproducible from one accumulated gradient")
        if kwargs.get("res"):
            raise NotImplementedError("STEGraphSAGE: res=True is not covered (the GraphSAGE adjacency gradient takes plain "
                                      "2-layer models)")
        if kwargs.get("norm") not in (None, "none"):
            raise NotImplementedError(f"STEGraphSAGE: norm={kwargs.get('norm')!r} is not covered (the GraphSAGE adjacency "
                                      "gradient takes plain 2-layer models)")
        if num_layers != 2:
            raise NotImplementedError(f"STEGraphSAGE: num_layers={num_layers} is not covered (the GraphSAGE adjacency "
                                      "gradient takes plain 2-layer models)")
        if train_masked_update and train_nodes is None:
            raise ValueError("'train_nodes' must be provided, to use train_masked_update.")  # models.py:149-151
        kwargs.pop("update_adj", None)
        kwargs.pop("sample_seed", None)
        # (num_sampled_nodes_per_hop does not reach GraphSAGE's sampler: the reference's sampling line is commented out)
        super().__init__(in_channels, hidden_channels, out_channels, num_layers, X, init_adj, dropout_p=dropout_p, act=act,
                         act_kwargs=act_kwargs, symmetric=symmetric, **kwargs)
        self.ste_num_sampled_nodes_per_hop = num_sampled_nodes_per_hop
        self.threshold = float(threshold)
        self.sign_grad = False
        self.train_masked_update = bool(train_masked_update)
        ei = self.edge_index
        self.edge_index = ei[:, ei[0] != ei[1]].contiguous()  # init_adj.fill_diagonal_(0), models.py:135
        self._track(candidates)
        if self.train_masked_update:
            both = self._train_pair_mask(train_nodes)  # train_adj_mask: hard 0 / 1 (gnn/models/utils.py:19-22)
            self.register_buffer("grad_adj_mask", torch.where(both, torch.tensor(0.0), torch.tensor(1.0)))

    @property
    def engine(self) -> GraphEngine:
        """The HIP context: a GraphSAGE graph that keeps and edits its diagonal (``self_loops=True``)."""
        dev = self.convs[0].lin.weight.device
        if self._engine is None:
            if dev.type != "cuda":
                raise RuntimeError("the HIP engine needs the model on a GPU: call model.to('cuda') first "
                                   "(there is no CPU fallback)")
            eng = GraphEngine(self.edge_index.to(dev), self.num_nodes, kind=self.kind, symmetric=self.symmetric,
                              self_loops=True)
            eng.bind(self.X.to(dev).contiguous(), [c.lin.weight for c in self.convs],
                     [c.lin.bias for c in self.convs], act=self.act_name)
            self._engine = eng
        return self._engine

    def _graph_edited(self, eng):
        # (adj_to_edge_index drops the diagonal, gnn/utils.py:333-336: the rebuild needs the learned self loops)
        self.edge_index = torch.stack(eng.export_adj()).contiguous()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """A reference checkpoint's dense ``adj`` [N, N] (continuous values) is reduced to the tracked pairs, and the engine's
        graph becomes its binarisation, diagonal included; this module's own checkpoints hold the tracked values as they are."""
        key = prefix + "adj"
        adj = state_dict.get(key)
        if adj is not None and adj.dim() == 2:
            if tuple(adj.shape) != (self.num_nodes, self.num_nodes):
                error_msgs.append(f"adj has shape {tuple(adj.shape)}, expected ({self.num_nodes}, {self.num_nodes})")
            else:
                dense = adj.to(torch.float32)
                ai = self.adj_index.to(dense.device)
                state_dict[key] = dense[ai[0], ai[1]]
                eff = 0.5 * (dense + dense.T) if self.symmetric else dense
                on = eff > self.threshold
                self.edge_index = on.nonzero().t().to(torch.int64).contiguous().to(self.edge_index.device)
                self._engine = None
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def full_adj(self) -> torch.Tensor:
        """Dense binarised adjacency (models.py:156-158) including the learned self loops, small graphs only."""
        return super().full_adj()

    def dense_adj(self) -> torch.Tensor:
        """The continuous parameter as the reference stores it (dense [N, N]): untracked pairs 0, the diagonal as tracked."""
        return self._tracked_dense()


class LoRASTEGCN(GCN):
    """The reference's low-rank structure-learning GCN (gnn/models/models.py:186-235) with the graph held by the HIP engine.

    The reference propagates with ``normalize_adj(fill_diagonal_(BinarizeSTE(M, threshold), 1))``,
    ``M = adj + (adj_lora_B @ adj_lora_A) * scaling`` (symmetric models: ``(M + M^T) / 2``), ``scaling = lora_alpha / r``.
    Here ``adj`` is the base pattern (``adj_index`` [2, n] names its entries, values 1; ``requires_grad=False``, never
    stepped -- the driver only insists that it exists, gnn/marglik_training.py:78) and lives on the device as a CSR pattern;
    the engine's graph is always the binarisation of the current A, B (set when the engine is built, kept by ``apply_adj``).
    Both LoRA names contain ``adj``: the Laplace parameter filter and the driver's weight optimizer drop them.

        la.fit(loader)
        model.adj_backward(la, loader)        # adj_lora_A.grad / adj_lora_B.grad <- neg_marglik.backward()
        adj_opt.step(); model.apply_adj()     # adj_opt = SGD([adj_lora_A, adj_lora_B], lr=lr_adj, weight_decay=weight_decay_adj)
        la.fit(loader)                        # the loop of gnn/marglik_training.py:97-100, 197-224

    The driver's optimizer has no momentum (marglik_training.py:97-100) and its ``clip_grad_norm_(model.adj)`` does not touch A
    and B.  The base ``adj`` is the given pattern as it is (the reference's ``reset_parameters`` copies the unsymmetrised
    ``init_adj`` back, base_gnn.py:120-122); a symmetric model averages ``M`` and ``M^T`` before the threshold, so a one-sided
    base edge enters at 0.5 + the averaged LoRA term.  Random draws: the convs are drawn at construction and A, B after them,
    once; the reference re-draws the convs in its ``reset_parameters`` before A and B, so one seed gives different values
    (goldens store the initial weights, A and B).  The gradient needs d(-marglik)/d adj on all N^2 pairs (``neg_marglik_adj_grad(..., dense=True)``), so graphs are
    limited to a few tens of thousands of nodes -- the reference holds several dense N x N tensors itself."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, X, edge_index, r, lora_alpha,
                 dropout_p: float = 0.5, act="relu", threshold: float = 0.5, symmetric: bool = False, **kwargs):
        if kwargs.get("res") or kwargs.get("norm") not in (None, "none"):
            raise NotImplementedError("LoRASTEGCN: res / norm are not supported (plain 2-layer GCN)")
        if num_layers != 2:
            raise NotImplementedError("LoRASTEGCN: num_layers must be 2 (the all-pairs adjacency gradient is 2-layer)")
        if int(r) < 1:
            raise ValueError("LoRASTEGCN: the rank r must be >= 1")
        if int(r) > 64:
            raise NotImplementedError("LoRASTEGCN: ranks above 64 are not supported (lgnn_lora_grad)")
        kwargs.pop("update_adj", None)
        super().__init__(in_channels, hidden_channels, out_channels, num_layers, X, edge_index, dropout_p=dropout_p, act=act,
                         symmetric=symmetric, **kwargs)
        self.threshold = float(threshold)
        self.r = int(r)
        self.lora_alpha = lora_alpha
        self.scaling = self.lora_alpha / self.r
        N = self.num_nodes
        self._set_base(self.edge_index.cpu())
        self.adj_lora_A = nn.Parameter(torch.zeros(self.r, N))
        self.adj_lora_B = nn.Parameter(torch.zeros(N, self.r))
        self.reset_lora_parameters()

    def reset_lora_parameters(self):
        nn.init.kaiming_uniform_(self.adj_lora_A, a=math.sqrt(5))  # models.py:211-225
        nn.init.normal_(self.adj_lora_B)
        self._engine = None

    def _set_base(self, ei: torch.Tensor):
        """The base pattern adj0 (``init_adj`` as given, models.py:205-209 + base_gnn.py:120-122): ``adj_index``, ``adj`` and
        the int32 CSR the threshold kernel reads."""
        N = self.num_nodes
        keys = torch.unique(ei[0] * N + ei[1])
        rows, cols = keys // N, keys % N
        dev = getattr(self, "adj", None).device if isinstance(getattr(self, "adj", None), torch.Tensor) else torch.device("cpu")
        self.register_buffer("adj_index", torch.stack([rows, cols]).to(dev))
        self.adj = nn.Parameter(torch.ones(keys.numel(), device=dev), requires_grad=False)
        rowptr = torch.zeros(N + 1, dtype=torch.int64)
        rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=N), 0)
        self.register_buffer("base_rowptr", rowptr.to(torch.int32).to(dev), persistent=False)
        self.register_buffer("base_col", cols.to(torch.int32).contiguous().to(dev), persistent=False)
        self.edge_index = torch.stack([rows, cols]).to(self.edge_index.device)
        self._engine = None

    @property
    def engine(self) -> GraphEngine:
        """The HIP context; a new one starts from the base graph and is re-thresholded at once (the initial A, B already push
        pairs over the threshold: 17 % of the non-edges at N = 64, r = 4, lora_alpha = 16)."""
        fresh = self._engine is None
        eng = BaseGNN.engine.fget(self)
        if fresh:
            self._fresh_flips = self._threshold(eng)  # (against the base graph the engine was built from)
        return eng

    def _threshold(self, eng) -> int:
        return eng.lora_threshold(self.base_rowptr, self.base_col, self.adj_lora_A, self.adj_lora_B, self.scaling,
                                  self.threshold, self.symmetric)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """A reference checkpoint's dense 0/1 ``adj`` [N, N] becomes the base pattern; A and B load as they are.  The engine is
        rebuilt (and re-thresholded) on next use.  This module's own checkpoints (1-D ``adj`` + ``adj_index``) rebuild the base
        pattern from ``adj_index``."""
        key = prefix + "adj"
        adj = state_dict.get(key)
        own_index = state_dict.get(prefix + "adj_index")
        if adj is not None and adj.dim() == 1 and own_index is not None:
            self._set_base(own_index.detach().cpu().to(torch.int64))
        elif adj is not None and adj.dim() == 2:
            if tuple(adj.shape) != (self.num_nodes, self.num_nodes):
                error_msgs.append(f"adj has shape {tuple(adj.shape)}, expected ({self.num_nodes}, {self.num_nodes})")
            elif not bool(((adj == 0) | (adj == 1)).all()):
                error_msgs.append("LoRASTEGCN: the base adj must be binary (gnn/models/base_gnn.py:73)")
            else:
                self._set_base(adj.detach().cpu().nonzero().t().to(torch.int64))
                state_dict[key] = self.adj.detach().clone()
            if prefix + "adj_index" not in state_dict:
                state_dict[prefix + "adj_index"] = self.adj_index
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        self._engine = None

    def full_adj(self) -> torch.Tensor:
        """What the reference returns: the base adjacency (gnn/models/base_gnn.py:133-134), dense, small graphs only."""
        out = torch.zeros(self.num_nodes, self.num_nodes, device=self.adj.device)
        out[self.adj_index[0], self.adj_index[1]] = self.adj.detach()
        return out

    def binarized_adj(self) -> torch.Tensor:
        """The graph the model currently propagates with (dense 0/1 with the self loops), small graphs only."""
        return BaseGNN.full_adj(self)

    @torch.no_grad()
    def adj_backward(self, la, train_loader, process_group=None):
        """``neg_marglik.backward()`` of the loop: ``adj_lora_A.grad += scaling B^T G``, ``adj_lora_B.grad += scaling G A^T`` with
        G = d(-marglik)/d adj on all pairs (``neg_marglik_adj_grad(..., dense=True)``; lgnn_lora_grad).  Returns the negative
        log marginal likelihood."""
        eng = self.engine
        N = self.num_nodes
        part = 4 * self.r * N * ((N + 63) // 64)  # lgnn_lora_grad's partials of grad_A
        limit = eng.workspace_limit
        if part > limit:
            raise NotImplementedError(f"LoRASTEGCN.adj_backward: {part} bytes of grad_A partials exceed the workspace limit "
                                      f"({limit} bytes)")
        value, G = la.neg_marglik_adj_grad(train_loader, process_group=process_group, dense=True)
        gA, gB = eng.lora_grad(G, self.adj_lora_A, self.adj_lora_B, self.scaling)
        for p, g in ((self.adj_lora_A, gA), (self.adj_lora_B, gB)):
            p.grad = g if p.grad is None else p.grad + g
        return value

    @torch.no_grad()
    def apply_adj(self) -> int:
        """After the optimizer step (or any change of A / B): re-binarise and flip the engine's entries that changed side
        (lgnn_lora_threshold).  Returns the number of directed entries flipped; a second call returns 0.  Without an engine (a
        new model, after ``load_state_dict`` or ``.to()``) one is built from the base graph and thresholded: the flips are
        counted against the base graph."""
        if self._engine is None:
            _ = self.engine
            return int(self.__dict__.pop("_fresh_flips", 0))
        return self._threshold(self._engine)
