"""The curvature entries of ``GraphEngine``: per-batch accumulation into caller-owned buffers.  Behind them: csrc/kfac.hip,
kfac_seed.hip, kfac_top.hip, the path route (paths*.hip, toptiles.hip, toppairs.hip, fused256.hip, gram_stream.hip,
longrows.hip, backgemm.hip), fisher.hip (``kfac_accumulate_fisher``, ``ef_accumulate``), diag.hip, jacobian.hip
(``full_accumulate``, ``jacobians``), lastlayer_full.hip, lastlayer_kron.hip and subnet.hip."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import torch

from .. import _lib
from ._marshal import ACTS, DEFAULT_WORKSPACE_LIMIT, KINDS, _dev_ptr, _no_paths_default, _opt_ptr, _raw_ptrs

_f32 = torch.float32


def kfac_plan(kind: str, dims: Sequence[int], num_nodes: int, nnz: int, act: str = "relu", fuse: bool = True,
              workspace_limit: int = DEFAULT_WORKSPACE_LIMIT, paths: bool | None = None) -> dict:
    """Which kernels ``lgnn_kfac_accumulate`` would run for a model of this shape (host-only query, no GPU work):
    per backward step l = L-1 .. 1 whether the fused SpMM^T -> Gram kernel and the compacted backward GEMM are used,
    whether the second plane buffer is needed and how many class planes fit one chunk of the workspace.

    ``paths`` (and with it ``fused`` / ``backgemm`` / ``need_pong`` of the first level) says what the SHAPE allows: whether a call
    really takes the path route also depends on the graph and the call -- the expected number of 2-hop paths per node of the batch
    (hub-heavy graphs keep the class planes), a Fisher-type seed, ``res`` / ``norm``.  ``GraphEngine.last_kfac_used_paths`` /
    ``lgnn_kfac_last_route`` report what the last call did."""
    lib = _lib.load()
    L = len(dims) - 1
    out = (C.c_int64 * (4 + L))()
    no_paths = _no_paths_default() if paths is None else not paths
    rc = lib.lgnn_kfac_plan(KINDS[kind], L, (C.c_int64 * (L + 1))(*dims), int(num_nodes), int(nnz), ACTS[act],
                            (0 if fuse else _lib.FLAG_NO_FUSE) | (_lib.FLAG_NO_PATHS if no_paths else 0),
                            int(workspace_limit), out)  # (no context: not a ``_call``)
    _lib.check(rc, "lgnn_kfac_plan")
    return {"seeds_on_the_fly": bool(out[0]), "sage_compact": bool(out[1]), "need_pong": bool(out[2]),
            "classes_per_chunk": int(out[3]), "fused": [bool(out[4 + l] & 1) for l in range(L)],
            "backgemm": [bool(out[4 + l] & 2) for l in range(L)], "paths": bool(out[4 + L - 1] & 4)}


class CurvatureEntries:
    supports_shares = True  # kfac_accumulate(share=...): lgnn_kfac_accumulate_share

    @property
    def last_kfac_used_paths(self) -> bool:
        """Whether the last KFAC accumulate took the two-hop path route (csrc/paths.hip, paths_fused.hip) rather than class planes."""
        return bool(self.lib.lgnn_kfac_last_route(self._h))

    @property
    def last_kfac_top_on_tiles(self) -> bool:
        """Whether the last KFAC accumulate's top layer ran on one of the path route's matrix-pipe kernels (csrc/toptiles.hip
        or csrc/toppairs.hip; ``last_kfac_top_kernel`` says which) rather than on ``seed_spmm_gram_kernel``."""
        return bool(self.lib.lgnn_kfac_last_top(self._h))

    @property
    def last_kfac_top_kernel(self) -> int:
        """Which kernel ran the last KFAC accumulate's top layer: 0 ``seed_spmm_gram_kernel``, 1 ``top_tiles_kernel``
        (csrc/toptiles.hip), 2 ``top_pairs_kernel`` (csrc/toppairs.hip)."""
        return int(self.lib.lgnn_kfac_last_top_kernel(self._h))

    def kfac_plan(self, fuse: bool = True, paths: bool | None = None) -> dict:
        """The kernel choices a KFAC accumulate on the bound model makes (see ``kfac_plan``)."""
        if self.has_extras:
            fuse = False  # res / norm models take the unfused route (csrc/resnorm.hip)
        return kfac_plan(self.kind, self.dims, self.num_nodes, self.nnz, self.act, fuse, self._ws_limit, paths)

    def new_kfac_buffers(self):
        """Zeroed caller-owned accumulators, as ONE flat fp32 buffer [A_0|B_0|...|A_{L-1}|B_{L-1}|loss]
        (one all-reduce suffices) plus per-factor views."""
        flat = torch.zeros(sum(i * i + o * o for i, o in self.block_dims) + 1, dtype=_f32, device=self.device)
        views, off = [], 0
        for l, (i, o) in enumerate(self.block_dims):
            A = flat[off:off + i * i].view(i, i); off += i * i
            B = flat[off:off + o * o].view(o, o); off += o * o
            views.append((A, B))
        return flat, views, flat[off:off + 1]

    def kfac_accumulate(self, idx, y, n_train: int, views, loss, fork_exact: bool = True, fuse: bool = True,
                        classes: tuple[int, int] | None = None, paths: bool | None = None,
                        share: tuple[int, int, int] | None = None):
        """Add one batch's factors into the caller-owned buffers.  ``classes=(begin, end)`` restricts the call to
        that range of class columns (an exact additive share of the batch; the share with class 0 also adds
        the loss and the A increment).  ``share=(begin, end, count)``: parts ``[begin, end)`` of ``count`` equal parts of
        the batch's work, cut the way the route in use splits best (``lgnn_kfac_accumulate_share``: destination-node ranges
        on the path routes, class ranges otherwise) -- what a data-parallel caller deals to its ranks."""
        given = idx
        idx, ip, M = self._batch(idx)
        # what the library may keep for this batch across fits (lgnn_kfac_batch_tag; consumed by the accumulate call below)
        tag = self._batch_tags.tag(idx, copied=idx is not given)
        y, yp = self._labels(y, M)
        # 2-layer GCN: two-hop path route (csrc/paths.hip, paths_fused.hip).  paths=None: the library decides (shape and the batch's expected
        # paths per node; LGNN_NO_PATHS=1 keeps the planes); True / False force one route where the shape allows
        no_paths = _no_paths_default() if paths is None else not paths
        flags = (_lib.FLAG_FORK_EXACT_SEED if fork_exact else 0) | (0 if fuse else _lib.FLAG_NO_FUSE) | \
            (_lib.FLAG_NO_PATHS if no_paths else 0) | (_lib.FLAG_FORCE_PATHS if paths else 0)
        A, B = _raw_ptrs([a for a, _ in views]), _raw_ptrs([b for _, b in views])
        if share is not None and classes is not None:
            raise ValueError("pass either classes or share")
        self._call_host("lgnn_kfac_batch_tag", tag)  # (nothing below raises before the call)
        if share is not None:
            self._call("lgnn_kfac_accumulate_share", ip, yp, M, int(n_train), flags, int(share[0]), int(share[1]),
                       int(share[2]), A, B, loss.data_ptr())
            return
        cb, ce = (0, self.dims[-1]) if classes is None else (int(classes[0]), int(classes[1]))
        self._call("lgnn_kfac_accumulate_classes", ip, yp, M, int(n_train), flags, cb, ce, A, B, loss.data_ptr())

    def kfac_accumulate_fisher(self, idx, y_seed, y_loss, n_train: int, views, loss, resid_scale: float = 1.0,
                               b_scale: float = 1.0, fuse: bool = True):
        """Empirical / Monte-Carlo Fisher KFAC of one batch: ONE backward pass seeded with
        ``resid_scale * d loss(f, y_seed) / d f``; ``B += b_scale * g^T g``.  ``y_loss`` (the true labels) makes this
        call also add the loss and the A increment -- pass it with the first draw of a batch, ``None`` afterwards."""
        idx, ip, M = self._batch(idx)
        y_seed, ys = self._labels(y_seed, M)
        y_loss, yl = self._labels(y_loss, M) if y_loss is not None else (None, None)
        self._call("lgnn_kfac_accumulate_fisher", ip, ys, yl, M, int(n_train), 0 if fuse else _lib.FLAG_NO_FUSE,
                   float(resid_scale), float(b_scale), _raw_ptrs([a for a, _ in views]), _raw_ptrs([b for _, b in views]),
                   loss.data_ptr())

    # -- empirical Fisher, diagonal and full GGN over all weights -----------------------------------------
    def ef_accumulate(self, idx, y_seed, y_loss=None, resid_scale: float = 1.0, scale: float = 1.0,
                      diag: torch.Tensor | None = None, full: torch.Tensor | None = None, grads: bool = False,
                      loss: torch.Tensor | None = None):
        """Per-sample loss gradients ``G = J^T r`` of a batch (returned as [M, P] when ``grads``), ``diag += scale *
        sum G^2``, ``full += scale * G^T G``; ``loss += loss(model(idx), y_loss)`` when ``y_loss`` is given."""
        idx, ip, M = self._batch(idx)
        y_seed, ys = self._labels(y_seed, M)
        y_loss, yl = self._labels(y_loss, M) if y_loss is not None else (None, None)
        G = self._new(M, self.n_params) if grads else None
        self._call("lgnn_ef_accumulate", ip, ys, yl, M, float(resid_scale), float(scale), _opt_ptr(diag, _f32, "diag"),
                   _opt_ptr(full, _f32, "full"), None if G is None else G.data_ptr(),
                   None if loss is None else loss.data_ptr())
        return G

    def diag_accumulate(self, idx, y, diag: torch.Tensor, loss: torch.Tensor):
        """diag += diagonal GGN of the batch, loss += raw loss sum (CE, or the MSE sum for a regression binding)."""
        idx, ip, M = self._batch(idx)
        y, yp = self._labels(y, M)
        self._call("lgnn_diag_accumulate", ip, yp, M, 0, _dev_ptr(diag, _f32, "diag"), loss.data_ptr())

    def full_accumulate(self, idx, y, H: torch.Tensor, loss: torch.Tensor):
        """H [P, P] += full GGN of the batch over all weights (regression binding: sum J^T J), loss += raw loss sum."""
        idx, ip, M = self._batch(idx)
        y, yp = self._labels(y, M)
        self._call("lgnn_full_accumulate", ip, yp, M, _dev_ptr(H, _f32, "H"), loss.data_ptr())

    def jacobians(self, idx: torch.Tensor):
        """(J [M, C, P], f [M, C]): per-sample Jacobians of the logits w.r.t. all parameters, parameters in
        module order (weight row major, bias) -- laplace/curvature/curvature.py:89-130."""
        idx, ip, M = self._batch(idx)
        J, f = self._new(M, self.dims[-1], self.n_params), self._new(M, self.dims[-1])
        self._call("lgnn_jacobians", ip, M, J.data_ptr(), f.data_ptr())
        return J, f

    # -- last layer (classification bindings: int64 labels) --------------------------------------------------
    def lastlayer_full_accumulate(self, idx, y, H: torch.Tensor, loss: torch.Tensor):
        idx, y, batch = self._batch_y(idx, y)
        self._call("lgnn_lastlayer_full_accumulate", *batch, _dev_ptr(H, _f32, "H"), loss.data_ptr())

    def lastlayer_features(self, idx: torch.Tensor):
        """(phi [M, D], s [M], f [M, C]): the last Linear's input row seen from the batch node, the bias scale, the logits."""
        idx, ip, M = self._batch(idx)
        D = self.in_dims[-1]
        out, f = self._new(M, D + 1), self._new(M, self.dims[-1])
        self._call("lgnn_lastlayer_features", ip, M, out.data_ptr(), f.data_ptr())
        return out[:, :D], out[:, D], f

    def new_lastlayer_pair_buffers(self):
        """Zeroed pair-major accumulators of the last-layer full GGN as ONE flat buffer [S | Sb | loss] (one all-reduce)
        plus views: S [Q, D, D], Sb [Q, D + 1], loss [1], Q = C (C + 1) / 2."""
        C, D = self.dims[-1], self.in_dims[-1]
        Q = C * (C + 1) // 2
        flat = torch.zeros(Q * (D * D + D + 1) + 1, dtype=_f32, device=self.device)
        S = flat[:Q * D * D].view(Q, D, D)
        Sb = flat[Q * D * D:Q * (D * D + D + 1)].view(Q, D + 1)
        return flat, S, Sb, flat[-1:]

    def lastlayer_pairs_accumulate(self, idx, y, S: torch.Tensor, Sb: torch.Tensor, loss: torch.Tensor):
        idx, y, batch = self._batch_y(idx, y)
        self._call("lgnn_lastlayer_pairs_accumulate", *batch, _dev_ptr(S, _f32, "S"), _dev_ptr(Sb, _f32, "Sb"),
                   loss.data_ptr())

    def lastlayer_pairs_place(self, S: torch.Tensor, Sb: torch.Tensor, H: torch.Tensor):
        """H [P_ll, P_ll] += the accumulated blocks (upper triangle), then the mirror pass."""
        self._call("lgnn_lastlayer_pairs_place", _dev_ptr(S, _f32, "S"), _dev_ptr(Sb, _f32, "Sb"), _dev_ptr(H, _f32, "H"))

    def new_lastlayer_kron_buffers(self):
        """Zeroed accumulators of the last-layer Kronecker GGN as ONE flat buffer [A | B | B_b | loss] (one all-reduce) plus
        views: A [D, D], B [C, C], B_b [C, C] (the bias block's factor), loss [1]."""
        C, D = self.dims[-1], self.in_dims[-1]
        flat = torch.zeros(D * D + 2 * C * C + 1, dtype=_f32, device=self.device)
        A = flat[:D * D].view(D, D)
        B = flat[D * D:D * D + C * C].view(C, C)
        Bb = flat[D * D + C * C:D * D + 2 * C * C].view(C, C)
        return flat, A, B, Bb, flat[-1:]

    def lastlayer_kron_accumulate(self, idx, y, n_train: int, A: torch.Tensor, B: torch.Tensor, Bb: torch.Tensor,
                                  loss: torch.Tensor, fork_exact: bool = True):
        """A += Phi^T Phi / n_train, B += sum_n V_n V_n^T, B_b += sum_n s_n^2 V_n V_n^T, loss += CE sum of the batch over the
        final Linear alone (``lgnn_lastlayer_kron_accumulate``); classification bindings only."""
        idx, y, batch = self._batch_y(idx, y)
        self._call("lgnn_lastlayer_kron_accumulate", *batch, int(n_train), _lib.FLAG_FORK_EXACT_SEED if fork_exact else 0,
                   _dev_ptr(A, _f32, "A"), _dev_ptr(B, _f32, "B"), _dev_ptr(Bb, _f32, "Bb"), loss.data_ptr())

    def lastlayer_diag_accumulate(self, idx, y, diag: torch.Tensor, loss: torch.Tensor):
        """diag [C D + C] += diagonal of the last-layer GGN of the batch (weight row major, then bias), loss += CE sum."""
        idx, y, batch = self._batch_y(idx, y)
        self._call("lgnn_lastlayer_diag_accumulate", *batch, _dev_ptr(diag, _f32, "diag"), loss.data_ptr())

    # -- subnetwork Laplace (csrc/subnet.hip) ---------------------------------------------------------------------
    def _subnet(self, subnet: torch.Tensor) -> torch.Tensor:
        """int64 [S] on the device.  The indices address the Laplace parameter vector (the columns of ``jacobians``); the
        front validates them once on the host (``SubnetLaplace._check_subnetwork_indices``), the device only flags."""
        if subnet.dim() != 1 or subnet.numel() == 0:
            raise ValueError("subnetwork indices must be a non-empty 1-dimensional tensor")
        if subnet.dtype != torch.int64:
            raise TypeError(f"subnetwork indices must be torch.int64, got {subnet.dtype}")
        return subnet.to(self.device).contiguous()

    def jacobians_subset(self, idx: torch.Tensor, subnet: torch.Tensor):
        """(J [M, C, S], f [M, C]): the columns ``subnet`` (distinct indices into the Laplace parameter vector, any order)
        of ``jacobians(idx)`` in the caller's order -- laplace/curvature/curvature.py:127-128 without the M C P slab."""
        idx, ip, M = self._batch(idx)
        subnet = self._subnet(subnet)
        S = subnet.shape[0]
        J, f = self._new(M, self.dims[-1], S), self._new(M, self.dims[-1])
        self._call("lgnn_jacobians_subset", ip, M, subnet.data_ptr(), S, J.data_ptr(), f.data_ptr())
        return J, f

    def subnet_full_accumulate(self, idx, y, subnet: torch.Tensor, H: torch.Tensor, loss: torch.Tensor):
        """H [S, S] += the sub-block ``[subnet][:, subnet]`` of the batch's full GGN (regression binding: sum J_S^T J_S),
        loss += raw loss sum."""
        idx, ip, M = self._batch(idx)
        subnet = self._subnet(subnet)
        S = subnet.shape[0]
        if tuple(H.shape) != (S, S):
            raise ValueError(f"H must be [{S}, {S}], got {tuple(H.shape)}")
        y, yp = self._labels(y, M)
        self._call("lgnn_subnet_full_accumulate", ip, yp, M, subnet.data_ptr(), S, _dev_ptr(H, _f32, "H"), loss.data_ptr())
