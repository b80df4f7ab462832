"""``LowRankLaplace``: the posterior class over the solver of ``laplace_gnn_amd.lowrank``."""
import torch

from .fit import ParametricLaplace


class LowRankLaplace(ParametricLaplace):
    """Low-rank GGN over all weights (laplace/baselaplace.py:1679-1835): ``P = U diag(l) U^T + P_0`` from the ``low_rank``
    leading eigenpairs of the GGN (``backend_kwargs={"low_rank": K}``, default 10), K P floats instead of P^2.  The reference's
    only backend for this class is power iteration on Hessian-vector products, which the fork's models cannot use; here the
    pairs come from block subspace iteration on the matrix-free GGN product (``HipGGN.eig_lowrank``, lowrank.py,
    csrc/ggnmat.hip).  ``n_sweeps`` / ``residuals`` / ``converged`` report the solver's last run.  Inversion, log determinant
    and samples cost a K x K matrix (fp64)."""
    _key = ("all", "lowrank")
    fit_graph = False  # an iterative fit with host-side stopping: a captured fit is refused by name

    def __init__(self, model, likelihood, *args, **kwargs):
        super().__init__(model, likelihood, *args, **kwargs)
        self._require_block_product()

    def _require_block_product(self):
        """The fit has one route, the GGN block product of the model's engine; an engine without it is refused where it is
        met (the reference refuses at construction too when its one backend is missing, laplace/baselaplace.py:1714-1718).  A
        model that is still on the CPU has no engine yet: ``fit`` asks again."""
        try:
            eng = getattr(self.model, "engine", None)
        except RuntimeError:  # BaseGNN.engine on a CPU model
            return
        if eng is not None and not hasattr(eng, "ggn_matmat_"):
            raise NotImplementedError(f"{self._key}: LowRankLaplace needs an engine with the GGN block product (ggn_matmat_); "
                                      f"{type(eng).__name__} has none")

    def _init_H(self):
        self.H = None
        self.n_sweeps, self.residuals, self.converged = 0, None, False

    def __setattr__(self, name, value):
        if name == "fit_graph" and value:
            raise NotImplementedError("LowRankLaplace: fit_graph (a captured fit) is not implemented")
        super().__setattr__(name, value)

    def fit(self, train_loader, override: bool = True, progress_bar: bool = False, process_group=None) -> None:
        """laplace/baselaplace.py:1747-1777: the eigenpairs are not additive over fits."""
        if not override:
            raise ValueError("LowRank LA does not support updating.")
        if process_group is not None:
            raise NotImplementedError("LowRankLaplace.fit: process_group (a multi-GPU reduction of the block) is not implemented")
        if not hasattr(self.backend, "eig_lowrank"):
            raise NotImplementedError(f"LowRankLaplace needs a backend with eig_lowrank (HipGGN), got {type(self.backend).__name__}")
        self._require_block_product()
        self._init_H()
        self._begin_fit(train_loader)
        eigenvectors, eigenvalues, loss = self.backend.eig_lowrank(train_loader)
        if hasattr(self.backend, "check_async_errors"):
            self.backend.check_async_errors()
        self.H = (eigenvectors, eigenvalues)
        self.loss = loss
        self.n_data = len(train_loader.dataset)
        info = getattr(self.backend, "lowrank_info", None)
        if info is not None:
            self.n_sweeps, self.residuals, self.converged = info.n_sweeps, info.residuals, info.converged

    def _check_H_init(self):
        if self.H is None:
            raise AttributeError("Laplace not fit. Run fit() first.")

    @property
    def posterior_precision(self):
        """``((U, H_factor * l), prior_precision_diag)``: the pieces of ``U diag(l) U^T + diag(p0)`` (:1779-1794)."""
        self._check_H_init()
        return (self.H[0], self._H_factor * self.H[1]), self.prior_precision_diag

    @property
    def V(self) -> torch.Tensor:  # :1737-1740
        (U, _), d = self.posterior_precision
        return U / d.reshape(-1, 1)

    def _K64(self) -> torch.Tensor:
        """``diag(1 / l) + U^T P_0^-1 U`` [K', K'] in fp64 (differentiable in the prior precision)."""
        (U, l), _ = self.posterior_precision
        return torch.diag(1 / l.double()) + (U.T @ self.V).double()

    @property
    def Kinv(self) -> torch.Tensor:  # :1742-1745, inverted in fp64 (1 / l spans twelve orders of magnitude)
        return torch.linalg.inv(self._K64()).to(self.H[0].dtype)

    def functional_variance(self, Js: torch.Tensor) -> torch.Tensor:  # :1796-1800
        prior_var = torch.einsum("ncp,nkp->nck", Js / self.prior_precision_diag, Js)
        Js_V = torch.einsum("ncp,pl->ncl", Js, self.V)
        return prior_var - torch.einsum("ncl,nkl->nck", Js_V @ self.Kinv, Js_V)

    def functional_covariance(self, Js: torch.Tensor) -> torch.Tensor:  # :1802-1810
        n_batch, n_outs, n_params = Js.shape
        Js = Js.reshape(n_batch * n_outs, n_params)
        prior_cov = torch.einsum("np,mp->nm", Js / self.prior_precision_diag, Js)
        Js_V = Js @ self.V
        return prior_cov - (Js_V @ self.Kinv) @ Js_V.T

    @property
    def log_det_posterior_precision(self) -> torch.Tensor:  # :1830-1835; -logdet(Kinv) = logdet(diag(1 / l) + U^T V) in fp64
        (_, l), d = self.posterior_precision
        return (l.double().log().sum() + d.double().log().sum() + torch.logdet(self._K64())).to(d.dtype)

    def _sample_transform(self, eps: torch.Tensor) -> torch.Tensor:
        """``T eps`` for ``eps`` [P, S] with ``T T^T = P^-1``.  With ``W = P_0^-1/2 U diag(l)^1/2`` and the eigenpairs
        ``W^T W = Q diag(s) Q^T`` (K' x K', fp64), ``T = P_0^-1/2 (I - W Q diag(1 / (sqrt(1 + s) (1 + sqrt(1 + s)))) Q^T W^T)`` is
        the symmetric ``(I + W W^T)^-1/2`` scaled by the prior.  The reference's lines (:1812-1828) multiply by ``sqrt(d)`` where
        ``1 / sqrt(d)`` is meant, leave the eigenvalues out of ``Vs`` and invert their ``C`` once too often: their draws do not
        have covariance ``P^-1`` (DESIGN 12.32 has the two-line counterexample); this map does."""
        (U, l), d = self.posterior_precision
        eps = eps.to(U.device, U.dtype)
        dis = d.rsqrt().reshape(-1, 1)
        W = U * l.clamp_min(0).sqrt().reshape(1, -1) * dis
        s, Q = torch.linalg.eigh((W.T @ W).double())
        root = (1 + s.clamp_min(0)).sqrt()
        Kern = ((Q / (root * (1 + root))) @ Q.T).to(U.dtype)
        return dis * (eps - W @ (Kern @ (W.T @ eps)))

    def _scale_samples(self, eps):
        return self._sample_transform(eps.T).T

    def _lowrank_matrix_free(self) -> bool:
        """A scalar prior precision on a plain 1- or 2-layer model: the predictive needs ``J V`` and the diagonal blocks of
        ``J J^T`` only, both of which the engine gives without handing Jacobians to the host side."""
        eng = getattr(self.backend, "engine", None)
        return (torch.as_tensor(self.prior_precision).numel() == 1 and eng is not None and hasattr(eng, "jvp_block")
                and len(eng.dims) in (2, 3) and not bool(getattr(eng, "has_extras", False)))

    def _covariance_rows(self, J):  # the P^-1 J^T of functional_covariance (:1802-1810), transposed
        return J / self.prior_precision_diag - ((J @ self.V) @ self.Kinv) @ self.V.T

    def _glm_predictive_distribution(self, x, diagonal_output: bool = False, joint: bool = False):
        if joint or not self._lowrank_matrix_free():
            return super()._glm_predictive_distribution(x, diagonal_output=diagonal_output, joint=joint)
        be = self.backend
        prior = torch.as_tensor(self.prior_precision, dtype=torch.float32, device=self._device).reshape(())
        f_mu = be.engine.forward(x)
        Js_V = be.jvp_block(x, self.V.T.contiguous())  # [M, C, K']
        if diagonal_output:
            prior_var = be.gp_kernel(x, x, independent=True, matched=True) / prior
            return f_mu, prior_var - ((Js_V @ self.Kinv) * Js_V).sum(-1)
        prior_var = be.gp_kernel(x, x, matched=True) / prior
        return f_mu, prior_var - torch.einsum("ncl,nkl->nck", Js_V @ self.Kinv, Js_V)

    def neg_marglik_adj_grad(self, *args, **kwargs):
        raise NotImplementedError("neg_marglik_adj_grad under the low-rank posterior is not implemented "
                                  "(KronLaplace, DiagLaplace and FullLaplace over all weights offer it)")
