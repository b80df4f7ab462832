"""``FunctionalLaplace``: the Laplace posterior in function space, a subset-of-data GP with the kernel
``k(x, x') = J(x) J(x')^T / delta`` (Khan et al. 2019, Immer et al. 2021).

The counterpart of the reference's class of the same name (laplace/baselaplace.py:1922-2960, factory key
``("all", "gp")``), restated for this project: the quantities and their layouts are the reference's, the kernel blocks come
from ``HipGGN.gp_kernel`` / ``gp_jvp`` (csrc/gpkernel.hip), which never form the Jacobians of the models they have a closed
form for.  A backend without ``gp_kernel`` (the CPU oracle backend of the host tests, the reference's own backends) gets the
same blocks by einsum from ``backend.jacobians``, so the class is a drop-in there too.

Two things follow the reference to the letter because its recorded results depend on them: the likelihood Hessian is cut to
its diagonal (``_build_L``), and ``_build_K_star_M`` flattens ``K_*M [b, m, c, e]`` (c: class of the test node, e: class of
the training node) as ``[b, (m, c), e]`` before the triangular solve.

Not implemented, refused by name: ``FunctionalLLLaplace``, ``enable_backprop=True``, ``process_group`` sharding,
``neg_marglik_adj_grad``, ``state_dict`` / ``load_state_dict``, ``method="gridsearch"``, a joint predictive with
``independent_outputs=True`` (the reference's own einsum for it does not run).
"""
from __future__ import annotations

import warnings
from math import pi

import numpy as np
import torch
import torch.distributed as dist
from torch.nn.utils import parameters_to_vector

from .data import TensorBatchLoader
from .laplace import BaseLaplace, _GLMLinkMixin


def sod_order(N: int, M: int, seed: int = 0) -> np.ndarray:
    """The subset-of-data order of the reference's ``SoDSampler`` (laplace/utils/utils.py:250-259)."""
    return np.random.default_rng(seed).choice(list(range(N)), M, replace=False)


class FunctionalLaplace(_GLMLinkMixin, BaseLaplace):
    _key = ("all", "gp")
    _K_STAR_BYTES_MAX = 1 << 30  # test nodes go in chunks whose K_*M [b, M, C, C] ([b, M, C]) stays under this and the workspace limit
    _JACOBIAN_BYTES_MAX = 1 << 62  # (the link code's switch to the parametric matrix-free covariance: never taken here)

    def __init__(self, model, likelihood, n_subset: int, sigma_noise=1.0, prior_precision=1.0, prior_mean=0.0,
                 temperature: float = 1.0, enable_backprop: bool = False, dict_key_x: str = "input_ids",
                 dict_key_y: str = "labels", backend=None, backend_kwargs=None, independent_outputs: bool = False,
                 seed: int = 0):
        if enable_backprop:
            raise NotImplementedError("FunctionalLaplace: enable_backprop=True is not implemented (the HIP kernel blocks "
                                      "carry no autograd graph)")
        self._check_prior_precision(prior_precision)
        self._recompute_Sigma = True
        super().__init__(model, likelihood, sigma_noise, prior_precision, prior_mean, temperature, enable_backprop,
                         dict_key_x, dict_key_y, backend, backend_kwargs)
        self.n_subset, self.independent_outputs, self.seed = int(n_subset), bool(independent_outputs), seed
        self.K_MM = None
        self.Sigma_inv = None  # Cholesky factor of  K_MM / delta' + Lambda^-1  (the reference's name)
        self.train_loader, self.batch_size, self._prior_factor_sod = None, None, None
        self.mu, self.L = None, None
        self.subset_order = None
        self.mean = parameters_to_vector(self.params).detach()
        self._fitted = False
        self._jac_cache = None

    # ---- prior: isotropic only; a change after fit asks for a new Cholesky factor ---------------------------------------
    @staticmethod
    def _check_prior_precision(prior_precision):
        if torch.is_tensor(prior_precision):
            if not (prior_precision.ndim == 0 or (prior_precision.ndim == 1 and len(prior_precision) == 1)):
                raise ValueError("Only isotropic priors supported in FunctionalLaplace")
        elif not (np.isscalar(prior_precision) and np.isreal(prior_precision)):
            raise ValueError("Only isotropic priors supported in FunctionalLaplace")

    @property
    def prior_precision(self):
        return self._prior_precision

    @prior_precision.setter
    def prior_precision(self, prior_precision):
        self._check_prior_precision(prior_precision)
        if torch.is_tensor(prior_precision):
            self._prior_precision = prior_precision.reshape(-1).to(self._device)
        else:
            self._prior_precision = torch.tensor([float(prior_precision)], device=self._device)
        self._recompute_Sigma = True

    @property
    def gp_kernel_prior_variance(self):
        return self._prior_factor_sod / self.prior_precision

    def _noise_var(self):
        return torch.as_tensor(self.sigma_noise, device=self._device).square()

    # ---- kernel blocks in the reference's layouts ----------------------------------------------------------------------
    @property
    def _on_device(self) -> bool:
        return hasattr(self.backend, "gp_kernel")

    def _jac(self, X):
        """Fallback backends: (Js, f) of a batch, kept for the duration of one fit / one predictive call."""
        key = tuple(X.reshape(-1).tolist())
        if self._jac_cache is None or key not in self._jac_cache:
            Js, f = self.backend.jacobians(X, enable_backprop=False)
            if self._jac_cache is None:
                return Js, f
            self._jac_cache[key] = (Js, f)
        return self._jac_cache[key]

    def _outputs(self, X):
        if self._on_device:
            with torch.no_grad():
                return self.model(X)
        return self._jac(X)[1]

    def _jvp(self, X, v):
        if self._on_device:
            return self.backend.gp_jvp(X, v)
        Js = self._jac(X)[0]
        return torch.einsum("bcp,p->bc", Js, v.to(Js.dtype))

    def _kernel_batch(self, Xa, Xb):
        """[a C, b C], or [a, b, C] with independent outputs (laplace/baselaplace.py:2684-2715)."""
        if self._on_device:
            K = self.backend.gp_kernel(Xa, Xb, independent=self.independent_outputs)
            return K.permute(1, 2, 0) if self.independent_outputs else K
        Ja, Jb = self._jac(Xa)[0], self._jac(Xb)[0]
        if self.independent_outputs:
            return torch.einsum("acp,bcp->abc", Ja, Jb)
        P = Ja.shape[-1]
        return torch.einsum("ap,bp->ab", Ja.reshape(-1, P), Jb.reshape(-1, P))

    def _kernel_batch_star(self, Xs, Xb):
        """[s, b, C, C] (class of the test node, then of the training node), or [s, b, C] (:2749-2776)."""
        if self._on_device:
            K = self.backend.gp_kernel(Xs, Xb, independent=self.independent_outputs)
            if self.independent_outputs:
                return K.permute(1, 2, 0)
            C = self.n_outputs
            return K.view(Xs.shape[0], C, Xb.shape[0], C).permute(0, 2, 1, 3)
        Js, Jb = self._jac(Xs)[0], self._jac(Xb)[0]
        if self.independent_outputs:
            return torch.einsum("bcp,ecp->bec", Js, Jb)
        return torch.einsum("bcp,dep->bdce", Js, Jb)

    def _kernel_star(self, Xs, joint: bool = False):
        """[s, C, C] or [s, C]; joint: [s, s, C, C] (:2717-2747)."""
        if joint:
            if self.independent_outputs:
                raise NotImplementedError("FunctionalLaplace: a joint predictive with independent_outputs=True is not "
                                          "implemented")
            C = self.n_outputs
            if self._on_device:
                return self.backend.gp_kernel(Xs, Xs).view(Xs.shape[0], C, Xs.shape[0], C).permute(0, 2, 1, 3)
            Js = self._jac(Xs)[0]
            return torch.einsum("acp,bep->abce", Js, Js)
        if self._on_device:
            return self.backend.gp_kernel(Xs, Xs, independent=self.independent_outputs, matched=True)
        Js = self._jac(Xs)[0]
        if self.independent_outputs:
            return torch.einsum("bcp,bcp->bc", Js, Js)
        return torch.einsum("bcp,bep->bce", Js, Js)

    # ---- fit -------------------------------------------------------------------------------------------------------------
    def _init_K_MM(self, like: torch.Tensor):
        M, C = self.n_subset, self.n_outputs
        if self.independent_outputs:
            self.K_MM = [torch.empty(M, M, device=like.device, dtype=like.dtype) for _ in range(C)]
        else:
            self.K_MM = torch.empty(M * C, M * C, device=like.device, dtype=like.dtype)

    def _store_K_batch(self, K_batch: torch.Tensor, i: int, j: int):
        """The block of subset batches (i, j) and, off the diagonal, its transpose at (j, i) (:2060-2088)."""
        b, M, C = self.batch_size, self.n_subset, self.n_outputs
        if self.independent_outputs:
            ri, rj = slice(i * b, min((i + 1) * b, M)), slice(j * b, min((j + 1) * b, M))
            for c in range(C):
                self.K_MM[c][ri, rj] = K_batch[:, :, c]
                if i != j:
                    self.K_MM[c][rj, ri] = K_batch[:, :, c].transpose(0, 1)
        else:
            ri, rj = slice(i * b * C, min((i + 1) * b * C, M * C)), slice(j * b * C, min((j + 1) * b * C, M * C))
            self.K_MM[ri, rj] = K_batch
            if i != j:
                self.K_MM[rj, ri] = K_batch.transpose(0, 1)

    def _build_L(self, lambdas):
        """The diagonal of the per-sample likelihood Hessians, [M C] in (n, c) order; one [M] slice per class with
        independent outputs (:2090-2114)."""
        L_diag = torch.diagonal(torch.cat(lambdas, dim=0), dim1=-2, dim2=-1).reshape(-1)
        if self.independent_outputs:
            return [L_diag[c::self.n_outputs] for c in range(self.n_outputs)]
        return L_diag

    def _build_Sigma_inv(self):
        """Cholesky factor of  K_MM / delta' + (H_factor Lambda)^-1  (:2116-2143); an infinite entry of the inverse reads 10."""
        var = self.gp_kernel_prior_variance.detach()
        if self.independent_outputs:
            self.Sigma_inv = [torch.linalg.cholesky(var.to(K.dtype) * K + torch.diag(
                torch.nan_to_num(1.0 / (self._H_factor * l), posinf=10.0).to(K.dtype))) for K, l in zip(self.K_MM, self.L)]
        else:
            K = self.K_MM
            self.Sigma_inv = torch.linalg.cholesky(var.to(K.dtype) * K + torch.diag(
                torch.nan_to_num(1.0 / (self._H_factor * self.L), posinf=10.0).to(K.dtype)))
        self._recompute_Sigma = False

    def _sod_loader(self, train_loader):
        if isinstance(train_loader, TensorBatchLoader):
            X, y = train_loader.indices, train_loader.labels
        else:
            parts = list(train_loader)
            X, y = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
        order = sod_order(len(train_loader.dataset), self.n_subset, self.seed)
        self.subset_order = order
        sel = torch.as_tensor(order, dtype=torch.int64, device=X.device)
        return TensorBatchLoader(X[sel], y[sel], batch_size=train_loader.batch_size)

    def fit(self, train_loader, progress_bar: bool = False, process_group=None) -> None:
        """Subset-of-data GP fit (:2156-2262): K_MM from the upper triangle of subset batch pairs, the diagonal Lambda, the
        scatter term's mean, the loss over the subset, the Cholesky factor.  ``n_data`` is the size of the whole training
        set."""
        if process_group is not None or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            raise NotImplementedError("FunctionalLaplace: process_group sharding is not implemented")
        dev = self._begin_fit(train_loader)
        self.batch_size = train_loader.batch_size
        if self.likelihood == "regression" and self.n_outputs > 1 and self.independent_outputs:
            warnings.warn("FunctionalLaplace with independent outputs is not recommended for multivariate regression: the "
                          "predictive variance will likely be overestimated.")
        N = len(train_loader.dataset)
        if self.n_subset > N:
            raise ValueError("`n_subset` must be less than or equal to the number of training points.")
        self.n_data = N
        self.train_loader = self._sod_loader(train_loader)
        self._prior_factor_sod = self.n_subset / self.n_data
        batches = [(X.to(dev), y.to(dev)) for X, y in self.train_loader]
        self._subset_batches = batches
        delta = self.mean - torch.as_tensor(self.prior_mean, device=dev, dtype=self.mean.dtype)  # -(prior_mean - mean)
        regression = self.likelihood == "regression"
        lambdas, mu = [], []
        self.loss, self.K_MM = 0.0, None
        self._jac_cache = None if self._on_device else {}
        try:
            for i, (X, y) in enumerate(batches):
                f = self._outputs(X)
                with torch.no_grad():
                    self.loss = self.loss + self.backend.factor * self.backend.lossfunc(f, y)
                if regression:
                    lambdas.append(torch.eye(f.shape[1], device=f.device, dtype=f.dtype).unsqueeze(0).repeat(f.shape[0], 1, 1))
                    mu.append(y - f + self._jvp(X, delta))
                else:  # second derivative of the log likelihood: diag(p) - p p^T
                    ps = torch.softmax(f, dim=-1)
                    lambdas.append(torch.diag_embed(ps) - torch.einsum("mk,mc->mck", ps, ps))
                    mu.append(self._jvp(X, delta))
                for j in range(i, len(batches)):
                    K_batch = self._kernel_batch(X, X if j == i else batches[j][0])
                    if self.K_MM is None:
                        self._init_K_MM(K_batch)
                    self._store_K_batch(K_batch, i, j)
        finally:
            self._jac_cache = None
        if hasattr(self.backend, "check_async_errors"):
            self.backend.check_async_errors()
        self.L = self._build_L(lambdas)
        self.mu = torch.cat(mu, dim=0)
        self._build_Sigma_inv()
        self._fitted = True

    # ---- predictive ------------------------------------------------------------------------------------------------------
    def _build_K_star_M(self, K_M_star, joint: bool = False):
        """``K_*M (K_MM / delta' + Lambda^-1)^-1 K_M*`` from the per-batch blocks (:2497-2545)."""
        K_M_star = torch.cat(K_M_star, dim=1)
        b = K_M_star.shape[0]
        # one triangular solve with all test nodes as right-hand sides (the reference's batched solve broadcasts the factor
        # over the test nodes; the numbers are the same)
        if self.independent_outputs:
            prods = []
            for c in range(self.n_outputs):
                v = torch.linalg.solve_triangular(self.Sigma_inv[c], K_M_star[:, :, c].transpose(0, 1), upper=False)  # [M, b]
                prods.append((v * v).sum(0).unsqueeze(1))
            return torch.cat(prods, dim=-1)
        C = K_M_star.shape[-1]
        K_M_star = K_M_star.reshape(b, -1, C)  # [b, (m, c), e]
        rhs = K_M_star.permute(1, 0, 2).reshape(K_M_star.shape[1], b * C)
        v = torch.linalg.solve_triangular(self.Sigma_inv, rhs, upper=False).view(-1, b, C)  # [(m, c), b, e]
        if joint:
            return torch.einsum("cam,cbn->abmn", v, v)
        return torch.einsum("cbm,cbn->bmn", v, v)

    def _K_M_star(self, Xs):
        var = self.gp_kernel_prior_variance.detach()
        return [var.to(K.dtype) * K for K in (self._kernel_batch_star(Xs, Xb) for Xb, _ in self._subset_batches)]

    def functional_variance(self, Xs) -> torch.Tensor:
        """``k_** - K_*M (...)^-1 K_M*`` per test node: [s, C, C] (:2420-2455)."""
        K_star = self._kernel_star(Xs)
        f_var = self.gp_kernel_prior_variance.detach().to(K_star.dtype) * K_star - self._build_K_star_M(self._K_M_star(Xs))
        return torch.diag_embed(f_var) if self.independent_outputs else f_var

    def functional_covariance(self, Xs) -> torch.Tensor:
        """The joint covariance of the test nodes: [s C, s C] (:2457-2495)."""
        K_star = self._kernel_star(Xs, joint=True)
        f_var = self.gp_kernel_prior_variance.detach().to(K_star.dtype) * K_star \
            - self._build_K_star_M(self._K_M_star(Xs), joint=True)
        return f_var.permute(0, 2, 1, 3).flatten(0, 1).flatten(1, 2)

    def _star_chunk(self) -> int:
        C = self.n_outputs
        budget = min(self._K_STAR_BYTES_MAX, int(getattr(getattr(self.backend, "engine", None), "workspace_limit", 1 << 62)))
        per_node = self.n_subset * C * (1 if self.independent_outputs else C) * 4  # K_*M of one test node
        return max(1, budget // max(1, per_node))

    @torch.no_grad()
    def _glm_predictive_distribution(self, x, diagonal_output: bool = False, joint: bool = False):
        """(f_mu [s, C], f_var [s, C, C]); ``diagonal_output``: f_var [s, C]; ``joint``: (f_mu [s C], f_var [s C, s C])."""
        self._jac_cache = None if self._on_device else {}
        try:
            if joint:
                return self._outputs(x).flatten(), self.functional_covariance(x)
            mus, fvars = [], []
            chunk = self._star_chunk()
            for s0 in range(0, max(int(x.shape[0]), 1), chunk):
                xs = x[s0:s0 + chunk]
                f_var = self.functional_variance(xs)
                mus.append(self._outputs(xs))
                fvars.append(torch.diagonal(f_var, dim1=-2, dim2=-1) if diagonal_output else f_var)
            return (mus[0], fvars[0]) if len(mus) == 1 else (torch.cat(mus), torch.cat(fvars))
        finally:
            self._jac_cache = None

    # (the matrix-free shortcuts of the parametric posteriors: none here, the link code takes f_var as computed above)
    def _bridge_moments_matrix_free(self, x):
        return None

    def _glm_covariance_matrix_free(self, x):
        return None

    _n_params_posterior = 0

    @torch.no_grad()
    def __call__(self, x, pred_type: str = "gp", joint: bool = False, link_approx: str = "probit", n_samples: int = 100,
                 diagonal_output: bool = False, generator: torch.Generator | None = None, eps: torch.Tensor | None = None,
                 **kwargs):
        """Posterior predictive (:2280-2372).  Classification: class probabilities through the link approximation;
        regression: (f_mu, f_var), with ``joint`` the joint mean and covariance of the nodes."""
        if not self._fitted:
            raise RuntimeError("Functional Laplace has not been fitted to any training dataset. Please call .fit method.")
        if self._recompute_Sigma:
            warnings.warn("The prior precision has been changed since fit. Re-computing its value...")
            self._build_Sigma_inv()
        if pred_type != "gp":
            raise ValueError("Only gp supported as prediction types.")
        if link_approx not in ("mc", "probit", "bridge", "bridge_norm"):
            raise ValueError(f"Unsupported link approximation {link_approx}.")
        x = x.to(self._device)
        if self.likelihood == "regression":
            f_mu, f_var = self._glm_predictive_distribution(x, joint=joint)
            if diagonal_output and not joint:
                f_var = torch.diagonal(f_var, dim1=-2, dim2=-1)
            return f_mu, f_var
        return self._glm_forward_call(x, link_approx, n_samples, diagonal_output, generator, eps)

    # ---- marginal likelihood -------------------------------------------------------------------------------------------
    @property
    def log_likelihood(self) -> torch.Tensor:
        factor = -self._H_factor
        if self.likelihood == "regression":
            sn = torch.as_tensor(self.sigma_noise, device=self._device)
            return factor * self.loss - self.n_data * self.n_outputs * torch.log(sn * (2 * pi) ** 0.5)
        return factor * self.loss

    def _scaled(self, K):
        return self.gp_kernel_prior_variance.to(K.dtype) * K

    @property
    def log_det_ratio(self) -> torch.Tensor:
        """classification: log |I + D^1/2 K D^1/2| with the diagonal D = H_factor Lambda; regression: log |K + sigma^2 I|
        (:2547-2592)."""
        Ks = self.K_MM if self.independent_outputs else [self.K_MM]
        Ls = self.L if self.independent_outputs else [self.L]
        total = 0.0
        for K, l in zip(Ks, Ls):
            eye = torch.eye(K.shape[0], device=K.device, dtype=K.dtype)
            if self.likelihood == "regression":
                total = total + torch.logdet(self._scaled(K) + eye * self._noise_var().to(K.dtype))
            else:
                W = torch.sqrt(self._H_factor * l).to(K.dtype)
                total = total + torch.logdet(W[:, None] * self._scaled(K) * W + eye)
        return total

    @property
    def scatter(self, eps: float = 0.00001) -> torch.Tensor:
        """``mu^T (K + noise I)^-1 mu`` with noise = sigma^2 (regression) or 1e-5 (classification) (:2594-2636)."""
        Ks = self.K_MM if self.independent_outputs else [self.K_MM]
        mus = [self.mu[:, c] for c in range(self.n_outputs)] if self.independent_outputs else [self.mu.reshape(-1)]
        total = 0.0
        for K, m in zip(Ks, mus):
            noise = self._noise_var().to(K.dtype) if self.likelihood == "regression" else eps
            chol = torch.linalg.cholesky(self._scaled(K) + torch.diag(torch.ones(K.shape[0], device=K.device, dtype=K.dtype) * noise))
            t = torch.linalg.solve_triangular(chol, m.to(K.dtype).unsqueeze(1), upper=False).squeeze(1)
            total = total + torch.dot(t, t)
        return total

    def log_marginal_likelihood(self, prior_precision=None, sigma_noise=None) -> torch.Tensor:
        """``log_lik - (log_det_ratio + scatter) / 2`` (:2814-2847), differentiable in ``prior_precision`` (and, for
        regression, ``sigma_noise``); passing either overwrites the current value."""
        if prior_precision is not None:
            self.prior_precision = prior_precision
        if sigma_noise is not None:
            if self.likelihood != "regression":
                raise ValueError("Can only change sigma_noise for regression.")
            self.sigma_noise = sigma_noise
            self._recompute_Sigma = True
        return self.log_likelihood - 0.5 * (self.log_det_ratio + self.scatter)

    def optimize_prior_precision(self, pred_type: str = "gp", method: str = "marglik", n_steps: int = 100, lr: float = 1e-1,
                                 init_prior_prec=1.0, prior_structure: str = "scalar", verbose: bool = False, **kwargs) -> None:
        """``method="marglik"``: Adam on the log of the scalar prior precision against ``-log_marginal_likelihood``
        (:2638-2682); the Cholesky factor is rebuilt for the value found."""
        if pred_type != "gp":
            raise ValueError("Only gp supported as prediction types.")
        if prior_structure != "scalar":
            raise ValueError("Only isotropic priors supported in FunctionalLaplace")
        if method == "gridsearch":
            raise NotImplementedError("FunctionalLaplace: method='gridsearch' is not implemented")
        if method != "marglik":
            raise ValueError("For now only marglik is implemented.")
        pp = init_prior_prec if torch.is_tensor(init_prior_prec) else torch.tensor(float(init_prior_prec))
        self._check_prior_precision(pp)
        log_pp = pp.detach().to(self._device, torch.float32).reshape(-1).log().clone().requires_grad_(True)
        opt = torch.optim.Adam([log_pp], lr=lr)
        with torch.enable_grad():
            for _ in range(n_steps):
                opt.zero_grad()
                neg = -self.log_marginal_likelihood(prior_precision=log_pp.exp())
                neg.backward()
                opt.step()
        self.prior_precision = log_pp.detach().exp()
        self._build_Sigma_inv()
        if verbose:
            print(f"Optimized prior precision is {self.prior_precision}.")

    # ---- out of scope ----------------------------------------------------------------------------------------------------
    def neg_marglik_adj_grad(self, *args, **kwargs):
        raise NotImplementedError("FunctionalLaplace: neg_marglik_adj_grad is not implemented under a GP posterior")

    def state_dict(self) -> dict:
        raise NotImplementedError("FunctionalLaplace: state_dict is not implemented")

    def load_state_dict(self, state_dict: dict) -> None:
        raise NotImplementedError("FunctionalLaplace: load_state_dict is not implemented")
