"""What crosses the C ABI (include/laplace_gnn_hip.h) and how: the enum tables, tensors as checked raw device pointers, the
current torch stream as a ``hipStream_t``, and ``BatchTagMap``, which names a batch for csrc/batchcache.hip."""
from __future__ import annotations

import ctypes as C
import os
from collections import OrderedDict

import torch

from .. import _lib

KINDS = {"gcn": _lib.KIND_GCN, "sage": _lib.KIND_SAGE}
ACTS = {"relu": _lib.ACT_RELU, "tanh": _lib.ACT_TANH}
LIKS = {"classification": _lib.LIK_CLASSIFICATION, "regression": _lib.LIK_REGRESSION}
NORMS = {None: _lib.NORM_NONE, "layer": _lib.NORM_LAYER, "batch": _lib.NORM_BATCH}
DEFAULT_WORKSPACE_LIMIT = 32 << 30  # the library's own default (lgnn_set_workspace_limit)


def _stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _dev_ptr(t: torch.Tensor, dtype, what: str) -> C.c_void_p:
    if not t.is_cuda:
        raise _lib.HipLibraryError(f"{what} must live on the GPU (got {t.device}); there is no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{what} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    return C.c_void_p(t.data_ptr())


def _opt_ptr(t, dtype, what: str):
    """A buffer the call may go without (``h1_bar`` of a 1-layer model, ``diag`` / ``full`` of ``ef_accumulate``): None -> NULL."""
    return None if t is None else _dev_ptr(t, dtype, what)


def _ptrs(ts, dtype, what: str):
    """``void *[]`` of checked device pointers, one per tensor; a None entry -> NULL."""
    return _lib.ptr_array([None if t is None else _dev_ptr(t, dtype, what).value for t in ts])


def _raw_ptrs(ts):
    """``void *[]`` of tensors the engine laid out itself (accumulator views, fresh outputs): nothing to check."""
    return _lib.ptr_array([t.data_ptr() for t in ts])


def _no_paths_default() -> bool:
    """LGNN_NO_PATHS=1 (read per call): keep the class-plane route of the 2-layer GCN KFAC for A/B timing."""
    return os.environ.get("LGNN_NO_PATHS", "") not in ("", "0")


class _IdentityKey:
    """Hashable wrapper comparing by object identity (tensors define elementwise ``==``)."""
    __slots__ = ("obj",)

    def __init__(self, obj):
        self.obj = obj

    def __hash__(self):
        return id(self.obj)

    def __eq__(self, other):
        return isinstance(other, _IdentityKey) and other.obj is self.obj


class BatchTagMap:
    """Names a batch for the library's batch-structure cache (``lgnn_kfac_batch_tag``): index tensor -> non-zero 64-bit tag.

    Two calls get the same tag exactly when they hand over the same elements of the same tensor, unchanged as far as torch
    can tell: the key is the identity of the tensor's base (held by reference, so its address cannot be recycled while the key
    lives), the data pointer, storage offset, length and the version counter (shared by a base and its views; every in-place
    write through torch bumps it).  ``TensorBatchLoader`` yields slices of one index tensor, so its batches repeat their keys
    fit after fit; a loader that collates fresh tensors never does and only ever runs the uncached code.  Writes through
    ``.data`` bump no counter -- the library compares the ids on the device and reports such a batch as an error.

    The map is bounded: the least recently used key goes first, and ``on_drop(tag)`` tells the library."""

    def __init__(self, capacity: int = 64, on_drop=None):
        self._map = OrderedDict()
        self._next = 1
        self.capacity = int(capacity)
        self.on_drop = on_drop

    @staticmethod
    def key(idx: torch.Tensor):
        base = idx._base if idx._base is not None else idx
        return (_IdentityKey(base), idx.data_ptr(), idx.storage_offset(), tuple(idx.shape), idx._version)

    def tag(self, idx: torch.Tensor, copied: bool = False) -> int:
        """The batch's tag; 0 (never cached) for a tensor that had to be copied to be handed over."""
        if copied or idx.dim() != 1 or not idx.is_contiguous():
            return 0
        k = self.key(idx)
        t = self._map.get(k)
        if t is not None:
            self._map.move_to_end(k)
            return t
        t = self._next
        self._next += 1
        self._map[k] = t
        while len(self._map) > self.capacity:
            _, old = self._map.popitem(last=False)
            if self.on_drop is not None:
                self.on_drop(old)
        return t

    def clear(self):
        self._map.clear()

    def __len__(self):
        return len(self._map)
