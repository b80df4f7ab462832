"""``DiagLaplace``: the diagonal GGN over all weights, accumulated in one buffer ``[H | loss]``, and the capture of a repeated
fit into a hipGraph."""
import os
import warnings

import torch

from ..adjgrad import _adjgrad_drive, _adjgrad_prelude, _propose_edges_drive, _propose_scope
from ..curvature import HipGGN
from ..data import TensorBatchLoader
from .dist import _dist_info
from .fit import Accumulator, ParametricLaplace


class _SlotAccumulator(Accumulator):
    """``[H | loss]``: ``H`` is a view of the buffer, so nothing is folded, and the buffer outlives the fit.  A Cora-shaped fit
    is launch bound, hence no kernel for the loss where none is needed: ``override=True`` allocated the buffer for this fit and
    hands its loss slot out as it is; ``override=False`` restarts the slot and hands out a copy, because the next such fit
    zeroes it again.  No multiplication by a ``factor`` of 1."""

    def __init__(self, la, override: bool):
        hl, n = la._hl, la.H.numel()
        super().__init__(hl, hl[n:], la.H)
        self.override = override
        if not override:
            if torch.is_tensor(la.loss) and la.loss.data_ptr() == self.loss.data_ptr():
                la.loss = la.loss.clone()  # the earlier fit handed the slot itself out
            self.loss.zero_()  # the loss slot restarts; H keeps the earlier fits

    def scaled_loss(self, factor: float):
        raw = self.loss[0] if self.override else self.loss[0].clone()
        return raw if factor == 1.0 else factor * raw


class DiagLaplace(ParametricLaplace):
    _key = ("all", "diag")
    _sample_additive = True  # einsum('bcp,bck,bkp->p') is a sum over b: batches may be sliced by samples
    _hl = None  # [H | loss] of the current fits (None: H is a plain tensor)

    def _init_H(self):
        # H and the raw loss share one flat buffer [H | loss]: one fill per fit, one all-reduce message
        self._hl = torch.zeros(self.n_params + 1, device=self._device)
        self.H = self._hl[:self.n_params]

    def _inplace_backend(self) -> bool:
        """The HIP backend adds a batch's diagonal GGN and raw loss straight into caller-owned buffers (no per-batch
        temporaries, no per-batch torch kernels: a Cora-shaped fit is launch bound); other backends return (loss, H)."""
        be = self.backend
        return (hasattr(be, "diag_accumulate_") and not getattr(be, "stochastic", False) and not self._asdl_fisher_kwargs
                and type(be).diag is getattr(HipGGN, "diag", None) and self._owns_H())

    def _owns_H(self) -> bool:
        """``H`` is the view of ``[H | loss]``, not a plain tensor (a subnetwork's, a loaded one, a distributed refit's)."""
        return self._hl is not None and self.H.data_ptr() == self._hl.data_ptr()

    _accumulate_entry = "diag_accumulate_"  # the backend's in-place entry (DiagLLLaplace: the head's)

    def _new_accumulator(self, override):
        return _SlotAccumulator(self, override) if self._inplace_backend() else None

    def _curv_closure(self, X, y, N):
        acc = self._accumulator()
        if acc is None:
            return self.backend.diag(X, y, N=N, **self._asdl_fisher_kwargs)
        getattr(self.backend, self._accumulate_entry)(acc.bufs, acc.loss, X, y)
        return 0.0, None

    # ---- a whole fit as ONE graph launch ---------------------------------------------------------------------------------
    # A Cora-shaped diagonal fit is ~12 kernels of 3-40 us each: the gaps between their launches (host work of this front,
    # dispatch latency) are a quarter of its wall time.  ``fit_graph = True`` (or LGNN_FIT_GRAPH=1) lets a fit that is repeated
    # unchanged -- the reference's structure-learning and hyper-parameter loops refit after every step
    # (gnn/marglik_training.py:197-224) -- be captured into a hipGraph (torch.cuda.CUDAGraph) on its second identical call and
    # replayed afterwards: the same kernels on the same buffers, forward pass included (it is recomputed on every replay, as the
    # reference recomputes it per batch), one launch.  "Identical" is an exact key: the loader object and its tensors, every
    # parameter's storage, the feature tensor's binding -- values may change (they are read by the kernels), pointers and shapes
    # may not; anything else falls back to the ordinary path.  After a replay ``H`` / ``loss`` / ``mean`` are the tensors of the
    # captured fit (overwritten by the next replay).  Single process, override=True, in-place HIP backend, classification.
    fit_graph = os.environ.get("LGNN_FIT_GRAPH", "") not in ("", "0")
    _FIT_GRAPH_WARM = 1  # ordinary fits with the same key before the capture (the workspaces reach their final size in one)

    def _fit_graph_key(self, train_loader, override, process_group):
        eng = getattr(self.backend, "engine", None)
        # (an engine without ``capture_token`` -- the CPU stand-in of the tests -- captures nothing)
        if (not self.fit_graph or not override or not hasattr(eng, "capture_token") or _dist_info(process_group)[1] != 1
                or self.likelihood != "classification" or not isinstance(train_loader, TensorBatchLoader)
                or eng.timing_enabled or self._on_phase is not None):
            return None
        ts = (train_loader.indices, train_loader.labels)
        if any((not t.is_cuda) for t in ts):
            return None
        return (id(train_loader), tuple((t.data_ptr(), tuple(t.shape)) for t in ts), getattr(train_loader, "batch_size", None),
                tuple((p.data_ptr(), tuple(p.shape)) for p in self.params), float(self.backend.factor), eng.capture_token())

    def _fit_graph_try(self, train_loader, key) -> bool:
        st = self.__dict__.setdefault("_fit_graph_state", {"key": None, "seen": 0, "graph": None, "off": False})
        if st["off"]:
            return False
        if st["key"] != key:
            st.update(key=key, seen=0, graph=None, out=None)
        if st["graph"] is None:
            st["seen"] += 1
            if st["seen"] <= self._FIT_GRAPH_WARM or not self._inplace_backend():
                return False
            eng = self.backend.engine
            try:
                torch.cuda.synchronize()
                eng.invalidate()  # the captured fit always contains its forward pass
                g = torch.cuda.CUDAGraph()
                self._capturing = True
                with torch.cuda.graph(g):
                    ParametricLaplace.fit(self, train_loader)
                st["graph"] = g
                st["out"] = {k: getattr(self, k) for k in ("H", "_hl", "loss", "mean", "n_data", "n_outputs")}
            except Exception as exc:  # capture not possible here (e.g. a workspace still had to grow): ordinary path from now on
                st["off"] = True
                torch.cuda.synchronize()
                warnings.warn(f"fit_graph: capture failed, falling back to the ordinary path ({exc})")
                return False
            finally:
                self._capturing = False
        st["graph"].replay()
        for k, v in st["out"].items():
            setattr(self, k, v)
        if self._on_accumulated is not None:
            self._on_accumulated()
        # invalid ids / labels: the replay is not waited for (that round trip per fit is what the graph is there to save) -- the
        # sticky flags of everything that has finished are read; what this replay raises is reported by the next fit at the
        # latest, or by backend.check_async_errors()
        if hasattr(self.backend, "peek_async_errors"):
            self.backend.peek_async_errors()
        elif hasattr(self.backend, "check_async_errors"):
            self.backend.check_async_errors()
        return True

    def fit(self, train_loader, override: bool = True, progress_bar: bool = False, process_group=None) -> None:
        key = self._fit_graph_key(train_loader, override, process_group)
        if key is not None and self._fit_graph_try(train_loader, key):
            return
        ParametricLaplace.fit(self, train_loader, override=override, progress_bar=progress_bar, process_group=process_group)

    @property
    def posterior_precision(self) -> torch.Tensor:
        return self.H * self._H_factor + self.prior_precision_diag

    @property
    def log_det_posterior_precision(self) -> torch.Tensor:
        return self.posterior_precision.log().sum()

    def _matrix_free_operands(self, out_map=None):
        shapes = [tuple(p.shape) for p in self.params]
        if len(shapes) not in (2, 4, 6) or [len(sh) for sh in shapes] != [2, 1] * (len(shapes) // 2):
            return None
        if len(shapes) == 2:  # a 1-layer model: S1 [C, F'] and kappa [C] describe its only layer
            C, D = shapes[0]
            inv = 1.0 / self.posterior_precision
            w, b = inv[:C * D].view(C, D), inv[C * D:C * D + C]
            if out_map is not None:
                E2 = out_map.to(w).square()
                w, b = E2 @ w, E2 @ b
            return dict(S0=None, S1=w, kappa=b)
        (Hd, F), _, (C, D1), _ = shapes[:4]  # (GraphSAGE: F and D1 are the widths of the concatenations)
        inv = 1.0 / self.posterior_precision
        o = 0
        w0 = inv[o:o + Hd * F].view(Hd, F); o += Hd * F
        b0 = inv[o:o + Hd].view(Hd, 1); o += Hd
        w1 = inv[o:o + C * D1].view(C, D1); o += C * D1
        b1 = inv[o:o + C]; o += C
        Sr = None
        if len(shapes) == 6:  # res.0.{weight, bias} behind the convs (parameter order)
            Hr, Fr = shapes[4]
            Sr = torch.cat([inv[o:o + Hr * Fr].view(Hr, Fr), inv[o + Hr * Fr:o + Hr * Fr + Hr].view(Hr, 1)], dim=1)
        if out_map is not None:  # independent parameters: the variance of a combination weighs each class by E^2
            E2 = out_map.to(w1).square()
            w1, b1 = E2 @ w1, E2 @ b1
        ops = dict(S0=torch.cat([w0, b0], dim=1), S1=w1, kappa=b1)
        if Sr is not None:
            ops["Sr"] = Sr
        return ops

    def neg_marglik_adj_grad(self, train_loader, prior_precision=None, process_group=None, candidates=None, dense=False):
        """``-log_marginal_likelihood()`` of this fit and its gradient w.r.t. the adjacency -- what ``neg_marglik.backward()``
        leaves in ``model.adj.grad`` when the structure-learning loop runs with ``hessian_structure="diag"``, the shipped
        STE-GCN configuration (gnn/configs/original/stegcn_config.yaml:7; gnn/marglik_training.py:197-216; the fork's
        Jacobians keep the graph, laplace/curvature/curvature.py:89-130).  Same return values and candidate pairs as
        ``KronLaplace.neg_marglik_adj_grad``.  1-layer GCN, 2-layer GCN (STEGCN, also with res / norm) and plain 2-layer GraphSAGE (STEGraphSAGE),
        classification; the diagonal GGN is a sum over samples, so
        the loader's batch boundaries do not matter and the ranks of a job split every batch by samples.  ``dense=True``: as
        ``KronLaplace.neg_marglik_adj_grad`` (plain 2-layer GCN, ``(neg_marglik, grad [N, N])``)."""
        eng = _adjgrad_prelude(self, "DiagLaplace", "a diagonal posterior", self.H is not None and bool(self.n_data),
                               prior_precision, candidates, dense, batch="diag_adjgrad_batch")
        value = -self.log_marginal_likelihood()
        f = self._H_factor
        gamma = (0.5 * f / self.posterior_precision).to(torch.float32).contiguous()  # d(1/2 logdet P) / dH_p
        return (value, *_adjgrad_drive(eng, train_loader, process_group, candidates, bool(getattr(self.model, "symmetric", False)),
                                       dense, batch="diag_adjgrad_batch", finish="diag_adjgrad_finish", weight=gamma,
                                       per_sample=True, loss_scale=f))

    def propose_edges(self, train_loader, k: int, prior_precision=None, band_bytes=None):
        """The ``k`` non-edges whose entry of ``d(-marglik)/d adj`` is smallest: ``(neg_marglik, pairs [2, k'] int64, grad [k']
        fp32)``, ascending by ``grad`` (most negative first; ties in any order), ``k' = min(k, eligible pairs)``.  Eligible:
        ``i != j`` and ``(i, j)`` not stored in the engine's adjacency (``export_adj()``).  ``grad[t]`` is what
        ``neg_marglik_adj_grad(loader, candidates=pairs)[3]`` returns for the pair and what ``neg_marglik_adj_grad(loader,
        dense=True)[1][i, j]`` holds (normalize_adj backward included, the STE as identity) -- without the N x N floats: the
        all-pairs gradient is formed in row bands of at most ``band_bytes`` (default: the smaller of the engine's workspace
        limit and 1 GiB; it must hold one 64-row tile, else ValueError) and only each band's k smallest survive it.  No eligible
        pair outside the result has a gradient below the largest returned one, up to fp32 rounding of the values.  ``neg_marglik``
        and ``prior_precision`` as in ``neg_marglik_adj_grad``.

        The reference's dense ``adj`` moves every entry along ``adj.grad`` (gnn/marglik_training.py:197-224): its plain-SGD step
        flips exactly the non-edges with ``grad < -threshold / lr_adj``.  There is no threshold argument: filter ``grad`` by
        that bound, hand the surviving pairs to ``STEGCN.add_candidates`` and step them like any tracked entry.

        Plain directed 2-layer GCN (no res / norm, ``symmetric=False``), ReLU, classification, one process; everything else
        raises NotImplementedError."""
        if int(k) < 1:
            raise ValueError(f"propose_edges: k must be at least 1, got {k}")
        _propose_scope(self, getattr(self.backend, "engine", None))
        eng = _adjgrad_prelude(self, "DiagLaplace", "a diagonal posterior", self.H is not None and bool(self.n_data),
                               prior_precision, None, False, batch="diag_adjgrad_batch")
        value = -self.log_marginal_likelihood()
        f = self._H_factor
        gamma = (0.5 * f / self.posterior_precision).to(torch.float32).contiguous()
        return (value, *_propose_edges_drive(eng, train_loader, int(k), band_bytes, weight=gamma, loss_scale=f))

    def _scale_samples(self, eps):  # laplace/baselaplace.py:1912-1919: samples * posterior_scale
        return eps * (1.0 / self.posterior_precision.sqrt()).reshape(1, -1)

    def functional_variance(self, Js):  # laplace/baselaplace.py:1901-1903
        return torch.einsum("ncp,p,nkp->nck", Js, 1.0 / self.posterior_precision, Js)

    def _covariance_rows(self, J):  # laplace/baselaplace.py:1905-1910: einsum("np,p,mp->nm") one factor at a time
        return J / self.posterior_precision

    def _covariance_operands(self):
        """Per Linear block ``S = 1 / precision`` of ``(W | b)``, no eigenbases."""
        shapes = [tuple(p.shape) for p in self.params]
        if len(shapes) % 2 or [len(sh) for sh in shapes] != [2, 1] * (len(shapes) // 2):
            return None
        inv = 1.0 / self.posterior_precision
        o, S = 0, []
        for out, din in shapes[::2]:
            w = inv[o:o + out * din].view(out, din)
            o += out * din
            S.append(torch.cat([w, inv[o:o + out].view(out, 1)], dim=1))
            o += out
        return dict(QA=[None] * len(S), QB=[None] * len(S), S=S)
