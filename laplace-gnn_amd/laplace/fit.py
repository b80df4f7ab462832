"""``ParametricLaplace.fit`` (laplace/baselaplace.py:778-854): the batch loop, how its work is dealt to the ranks of a process
group, and the one protocol for backends that accumulate in place."""
import torch

from .base import BaseLaplace, _is_zero_number
from .dist import _dist_info, all_reduce_flat_
from .marglik import _MarglikMixin
from .predictive import _PredictiveMixin


class Accumulator:
    """"This fit accumulates in place": the HIP backend adds every batch's curvature and raw loss into caller-owned buffers.
    ``flat`` is the single tensor that is all-reduced, ``loss`` the one-element raw-loss slot inside it, ``bufs`` what the
    posterior's ``_curv_closure`` hands to its backend call, and ``fold(la)`` runs once per fit, after the reduce: it places or
    packs the result into ``la.H``.  A posterior offers one through ``_new_accumulator(override)``."""

    def __init__(self, flat, loss, bufs, fold=None, parts=None):
        self.flat, self.loss, self.bufs = flat, loss, bufs
        self.fold = fold if fold is not None else lambda la: None
        # (``parts``: a stand-in backend whose buffers are separate tensors, tests/oracle_backend.py)
        self.reduce_tensors = [flat] if flat is not None else parts

    def scaled_loss(self, factor: float):  # a tensor of its own: the buffers go away with the fit
        return factor * self.loss[0].clone()


class ParametricLaplace(_PredictiveMixin, _MarglikMixin, BaseLaplace):
    H = None
    _acc, _override = None, True  # this fit's accumulator (allocated on first use) and its ``override``
    _capturing = False  # True while DiagLaplace captures a fit into a hipGraph
    _on_accumulated = _on_phase = None  # measurement hooks (bench.py)

    def _init_H(self):
        raise NotImplementedError

    def _curv_closure(self, X, y, N):
        raise NotImplementedError

    def _reduce_tensors(self) -> list[torch.Tensor]:
        """What the generic route (``backend.kron`` / ``diag`` / ``full`` returning ``(loss, H)``) all-reduces."""
        return [self.H]

    def _new_accumulator(self, override: bool) -> Accumulator | None:
        """The in-place route of this posterior's backend, or None: the generic route."""
        return None

    def _accumulator(self) -> Accumulator | None:
        if self._acc is None:
            self._acc = self._new_accumulator(self._override)
        return self._acc

    def fit(self, train_loader, override: bool = True, progress_bar: bool = False, process_group=None) -> None:
        """laplace/baselaplace.py:778-854, plus the sharding described in the package's docstring."""
        if override:
            self._init_H()
            self.loss = 0
            self.n_data = 0
        self._acc, self._override = None, override
        dev = self._begin_fit(train_loader)
        N = len(train_loader.dataset)
        rank, world = _dist_info(process_group)
        # override=False inside a distributed job: self.H already holds the previous fits' ALL-REDUCED curvature; it must
        # not take part in this fit's all-reduce (it would be counted once per rank): accumulate into a fresh buffer
        H_prev = None
        if not override and world > 1 and torch.is_tensor(self.H):
            H_prev, self.H = self.H, torch.zeros_like(self.H)
        loss = None  # stays None on the in-place route (the raw loss is in the accumulator)
        plan = self._shard_plan(train_loader, rank, world)
        for t, (X, y) in enumerate(train_loader):
            todo = plan(t, X.shape[0])
            if todo is None:
                continue
            X, y = X.to(dev), y.to(dev)
            if isinstance(todo, slice):  # sample-additive structures: this rank's slice of the batch
                X, y = X[todo], y[todo]
            # (class_begin, class_end): an exact additive share of the batch's KFAC factors; True: the whole batch
            kw = {} if todo is True or isinstance(todo, slice) else {"classes": todo}
            loss_batch, H_batch = self._curv_closure(X, y, N=N, **kw)
            if H_batch is not None or torch.is_tensor(loss_batch):  # (the in-place route returns (0.0, None): nothing to add)
                loss = loss_batch if loss is None else loss + loss_batch
            if H_batch is not None:
                self.H += H_batch
        self._finish_accumulate()
        if self._on_accumulated is not None:
            self._on_accumulated()  # end of the accumulate loop, before reduce / decompose
        # invalid node ids / labels are flagged on the device; one sync per fit.  (Deferring this check until the
        # decomposition is queued was measured: 94.9 -> 95.9 ms per arxiv-shaped fit, the host running ahead costs more
        # than the ~1 ms of launches it hides.)
        if hasattr(self.backend, "check_async_errors") and not self._capturing:
            self.backend.check_async_errors()  # (a graph capture cannot hold the synchronisation: _fit_graph_try checks after the replay)
        # a rank without local batches still takes part in the all-reduce: its accumulator is allocated now
        acc = self._accumulator() if world > 1 else self._acc
        if world > 1:
            if self._on_phase is not None:
                self._on_phase("reduce_begin")  # brackets the factor all-reduce
            if acc is not None:
                all_reduce_flat_(acc.reduce_tensors, process_group)
            else:
                loss = torch.as_tensor(0.0 if loss is None else loss, dtype=torch.float32, device=dev)
                all_reduce_flat_(self._reduce_tensors() + [loss], process_group)
            if self._on_phase is not None:
                self._on_phase("reduce_end")
        if acc is not None:
            acc.fold(self)
            loss, self._acc = acc.scaled_loss(self.backend.factor), None
        if H_prev is not None:
            H_prev += self.H
            self.H = H_prev
        if loss is not None:
            self.loss = loss if _is_zero_number(self.loss) else self.loss + loss
        self.n_data += N

    # how the work of one fit is dealt to the ranks of the process group
    _sample_additive = False  # True: H is a plain sum over samples (diag, last-layer full) -> slice batches

    def _shard_plan(self, train_loader, rank: int, world: int):
        """Returns plan(t, M) -> None (skip) | True (whole batch) | slice (samples) | (c0, c1) (class range)."""
        if world == 1:
            return lambda t, M: True
        if self._sample_additive:
            def plan(t, M):
                lo, hi = M * rank // world, M * (rank + 1) // world
                return slice(lo, hi) if hi > lo else None
            return plan
        return lambda t, M: True if t % world == rank else None  # whole batches round-robin

    def _finish_accumulate(self):
        """After the last batch is queued, before the reduce (KronLaplace starts its side-stream decomposition here)."""
