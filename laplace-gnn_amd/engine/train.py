"""The training entries of ``GraphEngine``: a differentiable training-mode forward with dropout and the weight gradients of
its tape.  Behind them: csrc/train.hip."""
from __future__ import annotations

import torch

from .. import _lib
from ._marshal import _dev_ptr, _ptrs, _raw_ptrs


class TrainingEntries:
    @property
    def train_token(self) -> int:
        """Counts the training forwards of this engine; right after a ``train_forward`` it names that forward's tape."""
        return self._train_token

    def train_forward(self, idx: torch.Tensor, masks=None, p: float = 0.0) -> torch.Tensor:
        """Logits [M, C] of the training-mode forward (gnn/models/base_gnn.py:136-161 with dropout): ``masks`` is one uint8
        keep-mask [N, dims[l+1]] per hidden layer (1 = kept; ``None`` = no dropout), kept activations are scaled by
        ``1 / (1 - p)``.  Writes the tape ``train_backward`` consumes; the cached eval-mode forward is left alone."""
        idx, ip, M = self._batch(idx)
        L, N = self.num_layers, self.num_nodes
        if not 0.0 <= float(p) < 1.0:
            raise ValueError(f"dropout probability must be in [0, 1), got {p}")
        arr = None
        if masks is not None:
            masks = list(masks)
            if len(masks) != L - 1:
                raise ValueError(f"need one dropout mask per hidden layer ({L - 1}), got {len(masks)}")
            for l, m in enumerate(masks):
                if m is not None and tuple(m.shape) != (N, self.dims[l + 1]):
                    raise ValueError(f"dropout mask {l} has shape {tuple(m.shape)}, expected {(N, self.dims[l + 1])}")
            arr = _ptrs(masks, torch.uint8, "dropout mask")
        out = self._new(M, self.dims[-1])
        self._train_keep = (idx, masks)  # borrowed by the library until the backward has run
        self._train_token += 1
        self._call("lgnn_train_forward", ip, M, arr, 1.0 / (1.0 - float(p)), out.data_ptr())
        return out

    def train_backward(self, grad_out: torch.Tensor, token: int | None = None):
        """Gradients of ``sum(grad_out * logits)`` of the last ``train_forward`` w.r.t. every bound parameter, as new tensors
        in ``named_parameters()`` order: ``norms.{l}.weight|bias`` (LayerNorm), ``convs.{l}.lin.weight|bias``,
        ``res.{l}.weight|bias``.  Consumes the tape: a second call, or a call after the parameters or the graph changed,
        raises.  ``token``: the value of ``train_token`` right after the forward this backward belongs to."""
        self._sync_versions()  # (a parameter written since the forward invalidates the tape in the library)
        if token is not None and token != self._train_token:
            raise _lib.HipLibraryError("train_backward: another training forward ran on this engine since the forward this "
                                       "backward belongs to (one tape per engine)")
        _, ws, bs = self._bound
        grad_out = grad_out.to(torch.float32).contiguous()
        keep = self._train_keep
        if keep is not None and tuple(grad_out.shape) != (keep[0].shape[0], self.dims[-1]):
            raise ValueError(f"grad_out has shape {tuple(grad_out.shape)}, expected {(keep[0].shape[0], self.dims[-1])}")
        new = lambda ts: [torch.empty_like(t) for t in ts]  # noqa: E731
        gW, gb = new(ws), new(bs)
        ex = self._extras
        gWr, gbr = (new(ex["res_weights"]), new(ex["res_biases"])) if self.has_res else ([], [])
        gnw, gnb = (new(ex["norm_weight"]), new(ex["norm_bias"])) if self.norm == "layer" else ([], [])
        self._call("lgnn_train_backward", _dev_ptr(grad_out, torch.float32, "grad_out"),
                   *(_raw_ptrs(ts) if ts else None for ts in (gW, gb, gWr, gbr, gnw, gnb)))
        self._train_keep = None
        out = [t for pair in zip(gnw, gnb) for t in pair]
        out += [t for pair in zip(gW, gb) for t in pair]
        out += [t for pair in zip(gWr, gbr) for t in pair]
        return out
