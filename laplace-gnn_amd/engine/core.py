"""The core of ``GraphEngine``: lifetime, the call helper, graph queries and edits, bind / versions / tokens, the eval-mode
forward, async errors and the timing hook.  Behind it: csrc/context.hip (handle, bind, versions, workspace, timing),
graph.hip (ingest, edits, exports), gcn2_forward.hip / kernels.hip / resnorm.hip (forward), batchcache.hip."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import torch

from .. import _lib
from ._marshal import ACTS, DEFAULT_WORKSPACE_LIMIT, KINDS, LIKS, NORMS, BatchTagMap, _dev_ptr, _IdentityKey, _ptrs, _stream


class EngineCore:
    """Graph ingest + model binding + the one path into the library; the entry families are mixed in beside it."""

    def __init__(self, edge_index: torch.Tensor, num_nodes: int, kind: str = "gcn", symmetric: bool = False,
                 self_loops: bool = False):
        """``self_loops=True`` (GraphSAGE only): the pairs ``(i, i)`` of the edge list are kept and ``update_adjacency`` edits
        them -- the graph of ``STEGraphSAGE``, whose diagonal is a learnable entry (gnn/models/models.py:135, 160-180).
        ``export_adj``, ``nnz`` and ``export_propagation`` then include them; ``adj_to_edge_index`` drops the diagonal as ever."""
        self.lib = _lib.load()
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {list(KINDS)}")
        if self_loops and kind != "sage":
            raise ValueError("self_loops=True: GraphSAGE engines only (a GCN's diagonal is overwritten with ones)")
        self.self_loops = bool(self_loops)
        if edge_index.dim() != 2 or edge_index.shape[0] != 2:
            raise ValueError("edge_index must have shape [2, E]")
        ei = edge_index.contiguous()
        _dev_ptr(ei, torch.int64, "edge_index")  # raises for CPU tensors: there is no CPU path
        self.device, self.kind, self.num_nodes = ei.device, kind, int(num_nodes)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = self.lib.lgnn_create(  # (takes the handle by reference: not a ``_call``)
                C.byref(self._h), self.num_nodes, _dev_ptr(ei, torch.int64, "edge_index"), ei.shape[1],
                KINDS[kind] | (_lib.KIND_SELF_LOOPS if self_loops else 0), int(bool(symmetric)), _stream(self.device))
        _lib.check(rc, "lgnn_create")
        # every attribute an engine ever has.  The two borrows held across calls (see ``_call``):
        self._bound = None  # (X, weights, biases) of ``bind``; ``_extras`` holds its res / norm tensors
        self._train_keep = None  # (idx, masks) of ``train_forward`` until ``train_backward`` has run
        self._extras, self._bind_opts, self._versions = {}, None, None
        self.dims = self.in_dims = self.block_dims = None
        self.has_res, self.norm = False, None
        self._batch_tags = BatchTagMap(on_drop=self._drop_batch_tag)
        self._graph_edits = self._rebinds = 0  # (an edit may move the CSR buffers: graphs captured before it are stale)
        self._train_token = 0  # counts training forwards: one tape per engine
        self._ws_limit = DEFAULT_WORKSPACE_LIMIT
        self._timing_on = False

    # -- lifetime -----------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:  # (getattr: __del__ also runs when __init__ raised early)
            self.lib.lgnn_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- the one path into the library ------------------------------------------------------------------
    def _call(self, name: str, *args):
        """``name(handle, *args, current stream of self.device)``; a non-zero return raises ``HipLibraryError`` under that name.

        The borrow rule.  A tensor that is handed to an enqueue-only call, and that the engine itself created for that call (a
        dtype, device or contiguity copy), need not outlive the call: it was allocated on the current stream, the work is
        enqueued on that stream, and the allocator reuses freed blocks in stream order.  A local variable that lives until
        ``_call`` returns is all such a copy needs.  The engine holds exactly two borrows across calls: what ``bind`` bound
        (``_bound``, ``_extras``), and the training tape's ``idx`` and masks until the backward has run (``_train_keep``)."""
        _lib.check(getattr(self.lib, name)(self._h, *args, _stream(self.device)), name)

    def _call_host(self, name: str, *args):
        """``_call`` for the entries that take no stream (host-side state, cache bookkeeping, timing reads)."""
        _lib.check(getattr(self.lib, name)(self._h, *args), name)

    def _batch(self, idx: torch.Tensor):
        """The opening of a batch call: versions synchronised, then (contiguous idx, its device pointer, its length)."""
        self._sync_versions()
        idx = idx.contiguous()
        return idx, _dev_ptr(idx, torch.int64, "idx"), idx.shape[0]

    def _batch_y(self, idx: torch.Tensor, y: torch.Tensor):
        """``_batch`` of the entries that take int64 class ids whatever the likelihood bound: (idx, y, (idx pointer, y pointer,
        length)); the tensors stay in the caller's locals until its ``_call`` has returned."""
        idx, ip, M = self._batch(idx)
        y = y.contiguous()
        return idx, y, (ip, _dev_ptr(y, torch.int64, "y"), M)

    def _new(self, *shape):
        return torch.empty(*shape, dtype=torch.float32, device=self.device)

    # -- batch-structure cache ------------------------------------------------------------------------
    def _drop_batch_tag(self, tag: int):
        if self._h:
            self._call_host("lgnn_batch_cache_drop", int(tag))

    def batch_cache_stats(self) -> dict:
        """Host-only: the library's batch-structure cache (``LGNN_BATCH_CACHE_MB``, 0 = off): entries held, their device
        bytes, and the tagged KFAC accumulates so far by outcome -- hits (no list-building kernel launched), misses (first
        sight of a batch, or not cacheable), builds (an entry was filled)."""
        out = (C.c_int64 * 5)()
        self._call_host("lgnn_batch_cache_stats", out)
        return dict(zip(("entries", "bytes", "hits", "misses", "builds"), map(int, out)))

    def batch_cache_clear(self):
        """Forget every cached batch structure (the library's entries and the tags handed out so far)."""
        self._batch_tags.clear()
        self._call_host("lgnn_batch_cache_drop", 0)

    # -- graph (the value-returning queries return no error code: not a ``_call``) ---------------------
    @property
    def nnz(self) -> int:
        return int(self.lib.lgnn_nnz(self._h))

    @property
    def is_symmetric(self) -> bool:
        return bool(self.lib.lgnn_is_symmetric(self._h))

    @property
    def num_long_rows(self) -> int:
        """Rows with more than 64 stored entries that the 256-wide fused kernel takes from the side kernel (-1: not built)."""
        return int(self.lib.lgnn_num_long_rows(self._h))

    def device_bytes(self) -> int:
        return int(self.lib.lgnn_device_bytes(self._h))

    def export_adj(self):
        rows, cols = (torch.empty(self.nnz, dtype=torch.int64, device=self.device) for _ in range(2))
        self._call("lgnn_export_adj", rows.data_ptr(), cols.data_ptr())
        return rows, cols

    def adj_to_edge_index(self) -> torch.Tensor:
        n = C.c_int64(0)
        self._call("lgnn_adj_to_edge_index", None, C.byref(n))
        out = torch.empty(2, n.value, dtype=torch.int64, device=self.device)
        if n.value:
            self._call("lgnn_adj_to_edge_index", out.data_ptr(), C.byref(n))
        return out

    def update_adjacency(self, rows: torch.Tensor, cols: torch.Tensor, state: torch.Tensor):
        """Edit the stored 0/1 adjacency in place (``lgnn_update_adjacency``): pairs ``(rows[k], cols[k])`` and the state each
        shall have afterwards (True / 1 = stored).  A structure-learning step (gnn/marglik_training.py:211-221) without a
        re-ingest; the cached forward pass and everything else derived from the graph is dropped by the library."""
        rows, cols = rows.to(self.device, torch.int64).contiguous(), cols.to(self.device, torch.int64).contiguous()
        state = state.to(self.device, torch.uint8).contiguous()
        if not (rows.shape == cols.shape == state.shape) or rows.dim() != 1:
            raise ValueError("rows, cols, state must be 1-D and of one length")
        if rows.numel() == 0:
            return
        with torch.cuda.device(self.device):
            self._call("lgnn_update_adjacency", _dev_ptr(rows, torch.int64, "rows"), _dev_ptr(cols, torch.int64, "cols"),
                       _dev_ptr(state, torch.uint8, "state"), rows.numel())
        self._graph_edits += 1

    def export_propagation(self):
        rows, cols = (torch.empty(self.nnz, dtype=torch.int64, device=self.device) for _ in range(2))
        vals = self._new(rows.shape[0])
        self._call("lgnn_export_propagation", rows.data_ptr(), cols.data_ptr(), vals.data_ptr())
        return rows, cols, vals

    # -- model ----------------------------------------------------------------------------------
    def bind(self, X: torch.Tensor, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor],
             act: str = "relu", likelihood: str = "classification", res_weights=None, res_biases=None, norm=None,
             norm_weight=None, norm_bias=None, norm_mean=None, norm_var=None, norm_eps: float = 1e-5):
        """``res_*`` / ``norm*``: the optional pieces of ``BaseGNN.forward`` (gnn/models/base_gnn.py:86-113, 141-149), one
        entry per hidden layer: ``res.{l}`` Linear [dims[l+1], dims[l]] and ``norms.{l}`` ("layer": LayerNorm weight / bias,
        "batch": eval-mode BatchNorm1d weight / bias + running mean / variance).  The ``res.{l}`` parameters follow all
        ``convs.*`` in every per-parameter result."""
        L = len(weights)
        if L != len(biases) or L == 0:
            raise ValueError("need one bias per weight")
        if act not in ACTS:
            raise NotImplementedError(f"activation {act!r} is not supported (relu, tanh)")
        mult = 2 if self.kind == "sage" else 1
        dims = [X.shape[1]]
        for w, b in zip(weights, biases):
            if w.shape[1] != mult * dims[-1] or b.shape[0] != w.shape[0]:
                raise ValueError(f"weight shape {tuple(w.shape)} does not chain from width {dims[-1]}")
            dims.append(w.shape[0])
        if X.shape[0] != self.num_nodes:
            raise ValueError("X must have one row per node")
        Xp = _dev_ptr(X, torch.float32, "X")
        self._call_host("lgnn_bind_model", L, (C.c_int64 * (L + 1))(*dims), _ptrs(weights, torch.float32, "weight"),
                        _ptrs(biases, torch.float32, "bias"), Xp, ACTS[act], LIKS[likelihood])
        self._bound = (X, list(weights), list(biases))
        self._bind_opts = (act, likelihood)
        self.dims = dims
        self.in_dims = [mult * d for d in dims[:-1]]
        if norm in ("none", ""):
            norm = None
        if norm not in NORMS:
            raise ValueError(f"Unknown normalization type: {norm}")
        self._extras = dict(res_weights=res_weights, res_biases=res_biases, norm=norm, norm_weight=norm_weight,
                            norm_bias=norm_bias, norm_mean=norm_mean, norm_var=norm_var, norm_eps=norm_eps)
        self.has_res = bool(res_weights) and L > 1
        self.norm = norm if L > 1 else None
        if self.has_res or self.norm is not None:
            def ptrs(ts, what, shape_of):
                if ts is None:
                    return None
                if len(ts) != L - 1:
                    raise ValueError(f"need one {what} per hidden layer")
                for l, t in enumerate(ts):
                    if tuple(t.shape) != shape_of(l):
                        raise ValueError(f"{what}[{l}] has shape {tuple(t.shape)}, expected {shape_of(l)}")
                return _ptrs(ts, torch.float32, what)
            hid = lambda l: (dims[l + 1],)  # noqa: E731
            if self.has_res and (res_biases is None or len(res_biases) != L - 1):
                raise ValueError("need one res bias per res weight")
            if self.norm is not None and (norm_weight is None or norm_bias is None):
                raise ValueError("norm weight / bias missing")
            if self.norm == "batch" and (norm_mean is None or norm_var is None):
                raise ValueError("BatchNorm needs its running statistics")
            self._call_host(
                "lgnn_bind_extras", ptrs(res_weights if self.has_res else None, "res weight", lambda l: (dims[l + 1], dims[l])),
                ptrs(res_biases if self.has_res else None, "res bias", hid), NORMS[self.norm],
                ptrs(norm_weight if self.norm else None, "norm weight", hid), ptrs(norm_bias if self.norm else None, "norm bias", hid),
                ptrs(norm_mean if self.norm == "batch" else None, "norm running mean", hid),
                ptrs(norm_var if self.norm == "batch" else None, "norm running var", hid), float(norm_eps))
        # KFAC blocks in parameter order: (in, out) of convs.{0..L-1}.lin, then of res.{0..L-2}
        self.block_dims = list(zip(self.in_dims, dims[1:])) + ([(dims[l], dims[l + 1]) for l in range(L - 1)] if self.has_res else [])
        self._versions = self._param_versions()

    @property
    def has_extras(self) -> bool:
        return self.has_res or self.norm is not None

    def set_likelihood(self, likelihood: str):
        """Switch the bound model between the classification and the regression likelihood (re-binds the same tensors)."""
        if self._bound is None:
            raise _lib.HipLibraryError("no model bound")
        if self._bind_opts[1] != likelihood:
            self._bind_again(likelihood)

    def _bind_again(self, likelihood: str | None = None):
        X, ws, bs = self._bound
        self.bind(X, ws, bs, self._bind_opts[0], likelihood or self._bind_opts[1], **self._extras)

    @property
    def likelihood(self) -> str:
        return self._bind_opts[1]

    @property
    def act(self) -> str:
        """The bound model's activation ("relu" / "tanh")."""
        return self._bind_opts[0]

    def _labels(self, y: torch.Tensor, M: int):
        """(tensor, device pointer) of a batch's labels: int64 class ids [M] (classification) or fp32 targets [M, C]
        (regression).  The caller holds the tensor until its ``_call`` has returned (the borrow rule)."""
        if self.likelihood == "regression":
            if y.numel() != M * self.dims[-1]:
                raise ValueError(f"regression targets must have shape [{M}, {self.dims[-1]}]")
            y = y.to(torch.float32).contiguous()
            return y, _dev_ptr(y, torch.float32, "y")
        y = y.contiguous()
        return y, _dev_ptr(y, torch.int64, "y")

    def feature_token(self):
        """Exact identity of the bound feature tensor for callers that cache what depends on X only: the tensor object itself
        (holding it keeps its storage from being recycled under the token), its version counter and the engine's own
        ``rebind`` count.  Writes through ``X.data`` (``X.data.mul_()``, ``X.data.copy_()``) bump no version counter: after
        them call ``rebind()`` -- the same contract as for parameters written through ``p.data`` (``invalidate()``)."""
        X = self._bound[0]
        return (_IdentityKey(X), X._version, tuple(X.shape), self._rebinds)

    def capture_token(self):
        """What a hipGraph captured over this engine depends on besides the caller's own tensors: the feature token, the
        graph-edit count, the workspace limit and the bound tensors' data pointers.  A different token: capture again."""
        return (self.feature_token(), self._graph_edits, self._ws_limit, tuple(p for p, _ in self._param_versions()))

    def _param_versions(self):
        X, ws, bs = self._bound
        extra = [t for k in ("res_weights", "res_biases", "norm_weight", "norm_bias", "norm_mean", "norm_var")
                 for t in (self._extras.get(k) or [])]
        return [(t.data_ptr(), t._version) for t in (X, *ws, *bs, *extra)]

    def invalidate(self):
        """Drop the cached forward / input Grams.  Needed by hand only after writes the version counters cannot see
        (``p.data.add_()`` and friends); optimizer steps, ``p.add_()`` under ``no_grad`` and storage swaps are detected."""
        self._call_host("lgnn_invalidate")

    def rebind(self):
        """Bind the same tensors again: drops everything derived from X too (padded copy, P X, X^T X and the callers'
        caches keyed by ``feature_token``).  For feature writes through ``X.data``, which no version counter records."""
        if self._bound is None:
            raise _lib.HipLibraryError("no model bound")
        self._rebinds += 1
        self._bind_again()
        self.invalidate()

    def _sync_versions(self):
        """In-place updates of the bound parameters (optimizer steps) invalidate the cached forward."""
        if self._bound is None:
            raise _lib.HipLibraryError("no model bound")
        v = self._param_versions()
        if v != self._versions:
            if [p for p, _ in v] != [p for p, _ in self._versions] or v[0] != self._versions[0]:
                # storage replaced (``param.data = ...``, e.g. torch.nn.utils.vector_to_parameters): bind the new pointers.
                # The feature tensor changed in place: lgnn_invalidate keeps what depends on X only (padded copy, P X,
                # X^T X), a re-bind drops it
                self._bind_again()
            self.invalidate()
            self._versions = v

    @property
    def num_layers(self):
        return len(self.dims) - 1

    @property
    def n_params(self):
        return sum(i * o + o for i, o in self.block_dims)

    def set_workspace_limit(self, nbytes: int):
        self._call_host("lgnn_set_workspace_limit", int(nbytes))
        self._ws_limit = int(nbytes)

    @property
    def workspace_limit(self) -> int:
        """Bytes the library's chunked workspaces may take (``set_workspace_limit``; 32 GiB unless set)."""
        return self._ws_limit

    # -- forward --------------------------------------------------------------------------------
    def forward(self, idx: torch.Tensor) -> torch.Tensor:
        idx, ip, M = self._batch(idx)
        out = self._new(M, self.dims[-1])
        self._call("lgnn_forward", ip, M, out.data_ptr())
        return out

    def forward_all(self) -> torch.Tensor:
        self._sync_versions()
        out = self._new(self.num_nodes, self.dims[-1])
        self._call("lgnn_forward_all", out.data_ptr())
        return out

    def check_async_errors(self):
        """Synchronise and raise if any batch since the last check contained an invalid node id or label."""
        self._call("lgnn_check_async_errors")

    def peek_async_errors(self):
        """The same report without synchronising: errors of the kernels that have finished (lgnn_peek_async_errors)."""
        self._call_host("lgnn_peek_async_errors")

    # -- timing hook ----------------------------------------------------------------------------
    def enable_kernel_timing(self, on: bool = True):
        self._call_host("lgnn_enable_kernel_timing", int(on))
        self._timing_on = bool(on)

    @property
    def timing_enabled(self) -> bool:
        """Event records surround the dominant kernel: such a fit is not captured into a graph."""
        return self._timing_on

    def kernel_timing_launches(self):
        """Durations [ms] of the dominant kernel's launches since timing was enabled, in launch order."""
        n = C.c_int64(0)
        self._call_host("lgnn_kernel_timing_launches", None, 0, C.byref(n))
        buf = (C.c_double * max(n.value, 1))()
        self._call_host("lgnn_kernel_timing_launches", buf, n.value, C.byref(n))
        return [buf[i] for i in range(n.value)]

    def kernel_timing(self):
        n, ms, planes = C.c_int64(0), C.c_double(0.0), C.c_int64(0)
        self._call_host("lgnn_kernel_timing_read", C.byref(n), C.byref(ms), C.byref(planes))
        return n.value, ms.value, planes.value
