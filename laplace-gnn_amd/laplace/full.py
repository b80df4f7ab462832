"""The dense posteriors: ``FullLaplace`` over all weights and ``FullLLLaplace`` over the final ``nn.Linear``."""
import torch
from torch import nn
from torch.distributions.multivariate_normal import _precision_to_scale_tril

from ..adjgrad import _adjgrad_drive, _adjgrad_prelude
from ..curvature import HipHessian
from .fit import Accumulator, ParametricLaplace


class FullLaplace(ParametricLaplace):
    """Full GGN over all weights (laplace/baselaplace.py:1380-1470): dense ``P x P`` precision, Cholesky-based scale,
    log determinant, functional variance and samples.  For the small models it fits (P^2 floats)."""
    _key = ("all", "full")
    _sample_additive = True

    def _init_H(self):
        self.H = torch.zeros(self.n_params, self.n_params, device=self._device)
        self._posterior_scale = None

    def _curv_closure(self, X, y, N):
        return self.backend.full(X, y, N=N)

    @property
    def posterior_precision(self) -> torch.Tensor:
        return self._H_factor * self.H + torch.diag(self.prior_precision_diag)

    @property
    def posterior_scale(self) -> torch.Tensor:
        """``P^-1/2`` as a lower-triangular factor (laplace/utils/utils.py:118-129).  Factorised in fp64 (P x P of a small
        model): the fp32 Cholesky of a GGN with near-zero directions lost three digits of the functional variance."""
        return _precision_to_scale_tril(self.posterior_precision.double()).float()

    @property
    def posterior_covariance(self) -> torch.Tensor:
        scale = self.posterior_scale
        return scale @ scale.T

    @property
    def log_det_posterior_precision(self) -> torch.Tensor:
        return self.posterior_precision.logdet()

    def functional_variance(self, Js):  # :1488-1489
        return torch.einsum("ncp,pq,nkq->nck", Js, self.posterior_covariance, Js)

    def _covariance_rows(self, J):  # :1491-1494: Js posterior_covariance Js^T, one factor at a time
        return J @ self.posterior_covariance

    def _scale_samples(self, eps):  # :1497-1508: samples @ posterior_scale
        return eps @ self.posterior_scale

    def _adj_gamma(self) -> torch.Tensor:
        """``Gamma = d(1/2 logdet(f H + Delta))/dH = (f / 2) (f H + Delta)^-1`` [P, P]: fp64 Cholesky and inverse, symmetrised,
        contiguous fp32.  The inverse is ``cholesky_inverse`` while the fp64 matrix stays below 2 GiB; above that the solver's
        one-call inverse fails on the device (seen at P = 23 063), so the identity is solved in column blocks of at most 1 GiB."""
        chol = torch.linalg.cholesky(self.posterior_precision.double())
        n = chol.shape[0]
        if n * n * 8 < 2 ** 31:
            Gamma = torch.cholesky_inverse(chol)
        else:
            Gamma = torch.empty_like(chol)
            step = max(1, 2 ** 30 // (8 * n))
            for c0 in range(0, n, step):
                c1 = min(n, c0 + step)
                E = torch.zeros(n, c1 - c0, dtype=chol.dtype, device=chol.device)
                E[c0:c1].fill_diagonal_(1.0)
                Gamma[:, c0:c1] = torch.cholesky_solve(E, chol)
        del chol
        Gamma.mul_(0.5 * float(self._H_factor))
        Gamma.add_(Gamma.T.clone()).mul_(0.5)
        return Gamma.to(torch.float32).contiguous()

    def neg_marglik_adj_grad(self, train_loader, prior_precision=None, process_group=None, candidates=None, dense=False):
        """``-log_marginal_likelihood()`` of this fit and its gradient w.r.t. the adjacency -- what ``neg_marglik.backward()``
        leaves in ``model.adj.grad`` when the structure-learning loop runs with ``hessian_structure="full"``
        (gnn/utils.py:57-59; gnn/marglik_training.py:197-216; laplace/baselaplace.py:1377-1505 over the fork's attached
        Jacobians, laplace/curvature/curvature.py:374-410, :89-130).  Same return values and candidate pairs as
        ``DiagLaplace.neg_marglik_adj_grad``.  1-layer GCN, 2-layer GCN (STEGCN, also with res / norm) and plain 2-layer GraphSAGE,
        classification.  ``d(1/2 logdet(f H + Delta))/dH = Gamma = (f / 2) (f H + Delta)^-1`` is held fixed; it is built once per
        call in fp64 (as ``posterior_scale``) and handed to the device in fp32.  The GGN is a sum over samples, so the ranks of a
        job split every batch by samples.  ``dense=True`` (LoRA) stays on the Kronecker and diagonal posteriors.  The gradient
        differentiates the GGN: a fit on the exact Hessian (``backend=HipHessian``) is refused."""
        if isinstance(self._backend_cls, type) and issubclass(self._backend_cls, HipHessian):
            raise NotImplementedError("neg_marglik_adj_grad differentiates the GGN; a posterior fitted with backend=HipHessian "
                                      "(the exact Hessian) has no adjacency gradient: fit with HipGGN")
        eng = _adjgrad_prelude(self, "FullLaplace", "the full posterior", self.H is not None and bool(self.n_data),
                               prior_precision, candidates, dense, batch="full_adjgrad_batch", dense_offered=False, depth=True)
        value = -self.log_marginal_likelihood()
        f = self._H_factor
        Gamma = self._adj_gamma()
        return (value, *_adjgrad_drive(eng, train_loader, process_group, candidates, bool(getattr(self.model, "symmetric", False)),
                                       False, batch="full_adjgrad_batch", finish="diag_adjgrad_finish", weight=Gamma,
                                       per_sample=True, loss_scale=f))


class FullLLLaplace(ParametricLaplace):
    """Last-layer full GGN (intent of laplace/lllaplace.py:369-378): parameters are the
    final ``nn.Linear``'s weight (row-major) then bias."""
    _key = ("last_layer", "full")
    _sample_additive = True

    def __init__(self, model, likelihood, *args, **kwargs):
        super().__init__(model, likelihood, *args, **kwargs)
        last = [m for m in model.modules() if isinstance(m, nn.Linear)][-1]
        self.params = [last.weight, last.bias]
        self.n_params = sum(p.numel() for p in self.params)
        self.n_layers = 2
        self._backend_kwargs = dict(self._backend_kwargs, last_layer=True)

    def _init_H(self):
        self.H = torch.zeros(self.n_params, self.n_params, device=self._device)

    def _inplace_backend(self) -> bool:
        """HIP backend: the batches of a fit accumulate in the pair-major layout of the weighted Grams and are placed into
        the P x P matrix once -- no placement / mirror pass per batch (2.3 GB each at the products shape), and the
        all-reduce of a data-parallel fit moves the pair buffers, half the bytes of H."""
        return hasattr(self.backend, "lastlayer_pairs_")

    def _new_accumulator(self, override):
        if not self._inplace_backend():
            return None
        eng = self.backend.engine
        flat, S, Sb, loss_buf = eng.new_lastlayer_pair_buffers()  # [S | Sb | loss]: one flat buffer, reduced in place
        return Accumulator(flat, loss_buf, (S, Sb), lambda la: eng.lastlayer_pairs_place(S, Sb, la.H))

    def _curv_closure(self, X, y, N):
        acc = self._accumulator()
        if acc is None:
            return self.backend.full(X, y, N=N)
        self.backend.lastlayer_pairs_(*acc.bufs, acc.loss, X, y)
        return 0.0, None

    posterior_precision, log_det_posterior_precision = FullLaplace.posterior_precision, FullLaplace.log_det_posterior_precision

    def functional_variance(self, Js):  # laplace/lllaplace.py via FullLaplace.functional_variance (baselaplace.py:1488-1489)
        cov = torch.linalg.inv(self.posterior_precision.double()).float()  # (fp64 inverse: see FullLaplace.posterior_scale)
        return torch.einsum("ncp,pq,nkq->nck", Js, cov, Js)

    def _covariance_rows(self, J):  # as FullLaplace (baselaplace.py:1491-1494) with the fp64 inverse above
        return J @ torch.linalg.inv(self.posterior_precision.double()).float()
