"""The posterior predictive of the parametric posteriors: the link code, posterior samples and the "nn" route, the
matrix-free variance / bridge / covariance routes (csrc/predictive.hip) and the chunked Jacobian route."""
from math import pi

import torch
from torch.nn.utils import vector_to_parameters


class _GLMLinkMixin:
    """The link code of the classification predictive, shared by the parametric posteriors and ``FunctionalLaplace``: both hand
    it ``_glm_predictive_distribution(x, diagonal_output)`` (and, where they have one, the matrix-free shortcuts
    ``_bridge_moments_matrix_free`` / ``_glm_covariance_matrix_free``; ``None`` from either means the Jacobian route)."""

    def _glm_forward_call(self, x, link_approx, n_samples, diagonal_output, generator, eps):
        """laplace/baselaplace.py:570-665 (classification branches)."""
        if link_approx == "probit":  # reads the diagonal of f_var only (laplace/baselaplace.py:610-616)
            f_mu, f_var_diag = self._glm_predictive_distribution(x, diagonal_output=True)
            kappa = 1 / torch.sqrt(1.0 + pi / 8 * f_var_diag)
            return torch.softmax(kappa * f_mu, dim=-1)
        if link_approx == "mc":
            if diagonal_output:  # samples of N(f_mu, diag f_var): the diagonal is all that is read (:667-709)
                f_mu, f_var_diag = self._glm_predictive_distribution(x, diagonal_output=True)
                return self._glm_predictive_samples(f_mu, f_var_diag, n_samples, False, generator, eps).mean(dim=0)
            big = x.shape[0] * self.n_outputs * self._n_params_posterior * 4 > self._JACOBIAN_BYTES_MAX
            full = self._glm_covariance_matrix_free(x) if big else None
            if full is not None:
                f_mu, f_var = full
                # polarised off-diagonals can leave a node's matrix indefinite in the last bits: those nodes (if any) take the
                # Jacobian route, 32 at a time
                info = torch.linalg.cholesky_ex(f_var).info
                bad = info.nonzero().squeeze(1)
                for b0 in range(0, bad.numel(), 32):
                    sel = bad[b0:b0 + 32]
                    f_var[sel] = self._glm_predictive_distribution(x[sel])[1]
            else:
                f_mu, f_var = self._glm_predictive_distribution(x)
            return self._glm_predictive_samples(f_mu, f_var, n_samples, diagonal_output, generator, eps).mean(dim=0)
        # Laplace bridge with zero-mean correction (:630-660): reads the diagonal, the row sums and the total of f_var only
        moments = self._bridge_moments_matrix_free(x)
        if moments is None:
            f_mu, f_var = self._glm_predictive_distribution(x)
            moments = (f_mu, torch.diagonal(f_var, dim1=1, dim2=2), f_var.sum(-1), f_var.sum(dim=(1, 2)))
        f_mu, f_var_diag, rows, total = moments  # (symmetric f_var: f_var.sum(-1) == f_var.sum(-2))
        f_mu = f_mu - rows * f_mu.sum(-1).reshape(-1, 1) / total.reshape(-1, 1)
        f_var_diag = f_var_diag - rows * rows / total.reshape(-1, 1)
        K = f_mu.size(-1)
        if link_approx == "bridge_norm":
            f_var_diag_mean = f_var_diag.mean(dim=1)
            f_var_diag_mean = f_var_diag_mean / torch.as_tensor([K / 2], device=self._device).sqrt()
            f_mu = f_mu / f_var_diag_mean.sqrt().unsqueeze(-1)
            f_var_diag = f_var_diag / f_var_diag_mean.unsqueeze(-1)
        sum_exp = torch.exp(-f_mu).sum(dim=1).unsqueeze(-1)
        alpha = (1 - 2 / K + f_mu.exp() / K ** 2 * sum_exp) / f_var_diag
        return torch.nan_to_num(alpha / alpha.sum(dim=1).unsqueeze(-1), nan=1.0)

    def _glm_predictive_samples(self, f_mu, f_var, n_samples, diagonal_output=False, generator=None, eps=None):
        """softmax of samples of N(f_mu, f_var): laplace/baselaplace.py:667-709 + utils.normal_samples (:329-369)."""
        if diagonal_output:
            f_var = torch.diagonal(f_var, dim1=1, dim2=2)
        C = f_mu.shape[1]
        if eps is None:
            eps = torch.randn((C, n_samples), device=f_mu.device, dtype=f_mu.dtype, generator=generator)
        eps = eps.to(f_mu.device)
        if f_var.ndim == 2:
            scaled = f_var.sqrt().unsqueeze(-1) * eps.unsqueeze(0)
        else:
            scaled = torch.matmul(torch.linalg.cholesky(f_var), eps.unsqueeze(0))
        f_samples = (f_mu.unsqueeze(-1) + scaled).permute((2, 0, 1))
        if self.likelihood == "regression":  # (reached through predictive_samples only: the samples themselves)
            return f_samples
        return torch.softmax(f_samples, dim=-1)


class _PredictiveMixin(_GLMLinkMixin):
    # ---- posterior samples and the sampling ("nn", link_approx="mc") predictive the GNN driver evaluates with
    # (gnn/marglik_training.py:338-352 -> laplace/baselaplace.py:1183-1199): theta ~ N(mean, P^-1), softmax, mean.  Plain
    # 1- / 2-layer models: all samples in one pass on the device, nothing written (csrc/sampled.hip); otherwise one
    # full-graph forward per sample (the in-place parameter writes invalidate the engine's cache).
    def sample(self, n_samples: int = 100, generator: torch.Generator | None = None, eps: torch.Tensor | None = None):
        """``eps`` (n_samples x n_params standard normal draws) may be passed instead of a generator so that
        results are reproducible across devices."""
        if eps is None:
            eps = torch.randn(n_samples, self.n_params, device=self._device, generator=generator)
        return self.mean.reshape(1, self.n_params) + self._scale_samples(eps.to(self._device))

    def _scale_samples(self, eps):
        raise NotImplementedError

    @torch.no_grad()
    def __call__(self, x, pred_type: str = "glm", link_approx: str = "probit", n_samples: int = 100,
                 diagonal_output: bool = False, generator: torch.Generator | None = None,
                 eps: torch.Tensor | None = None, joint: bool = False, **kwargs):
        """Posterior predictive (laplace/baselaplace.py:975-1072).

        ``pred_type="glm"`` (default, with ``link_approx`` in probit / mc / bridge / bridge_norm): linearised model,
        ``f ~ N(f_mu, J P^-1 J^T)`` from explicit Jacobians (:1123-1158, :570-665).  ``pred_type="nn"`` with
        ``link_approx="mc"``: parameter samples, one forward each (:1183-1199).  ``eps`` replaces the random draws
        (standard normal, [n_samples, n_params] for "nn", [n_outputs, n_samples] for "glm"/"mc").  ``joint=True`` (regression,
        "glm"): the joint predictive over the evaluation nodes, ``(f_mu [M C], f_cov [M C, M C])`` (:618-625, :1123-1158);
        classification does not read it (:618-620).  Other keyword arguments are accepted and ignored."""
        if pred_type not in ("glm", "nn"):
            raise ValueError("Only glm and nn supported as prediction types.")
        if link_approx not in ("mc", "probit", "bridge", "bridge_norm"):
            raise ValueError(f"Unsupported link approximation {link_approx}.")
        if pred_type == "nn" and link_approx != "mc":
            raise ValueError("Only mc link approximation is supported for nn prediction type.")
        x = x.to(self._device)
        regression = self.likelihood == "regression"
        if pred_type == "glm":
            if regression and joint:  # N([f(x_1) .. f(x_M)], Cov): diagonal_output is not read (:622-625)
                return self._glm_predictive_distribution(x, joint=True)
            if regression:  # (f_mu [M, C], f_var [M, C, C]) of the linearised model (:620-624)
                f_mu, f_var = self._glm_predictive_distribution(x)
                return f_mu, (torch.diagonal(f_var, dim1=-2, dim2=-1) if diagonal_output else f_var)
            return self._glm_forward_call(x, link_approx, n_samples, diagonal_output, generator, eps)
        # the reduction of _nn_predictive_samples over chunks of samples: [S, M, C] need not exist
        samples = self.sample(n_samples, generator=generator, eps=eps)
        S = samples.shape[0]
        chunk = max(1, min(S, self._NN_CHUNK_FLOATS // max(1, x.shape[0] * int(self.n_outputs or 1))))
        if chunk >= S:
            outs = self._nn_forward_samples(x, samples)
            if regression:  # mean and variance over the parameter samples (:1060-1066)
                return outs.mean(dim=0), outs.var(dim=0)
            return outs.mean(dim=0)
        # chunks meet as (count, mean, sum of squared deviations from the mean): the variance never subtracts two large sums
        n, mean, m2 = 0, None, None
        for s0 in range(0, S, chunk):
            outs = self._nn_forward_samples(x, samples[s0:s0 + chunk])
            nb, mean_b = outs.shape[0], outs.mean(dim=0)
            m2_b = ((outs - mean_b) ** 2).sum(dim=0) if regression else None
            if mean is None:
                n, mean, m2 = nb, mean_b, m2_b
                continue
            delta = mean_b - mean
            if regression:
                m2 = m2 + m2_b + delta * delta * (n * nb / (n + nb))
            mean = mean + delta * (nb / (n + nb))
            n += nb
        if regression:
            return mean, m2 / (n - 1)
        return mean

    _NN_CHUNK_FLOATS = 1 << 27  # floats of a chunk of sampled outputs [S_chunk, M, C] in ``__call__(pred_type="nn")``

    def _nn_device_route(self) -> bool:
        """Whether the backend evaluates parameter samples without writing them into the model (``sampled_forward``: plain
        1- or 2-layer GCN / GraphSAGE on the HIP engine, posterior over all of the model's parameters)."""
        be = self.backend
        scope = getattr(be, "sampled_forward_in_scope", None)
        return scope is not None and hasattr(be, "sampled_forward") and bool(scope(self.n_params))

    def _nn_forward_samples(self, x, samples):
        """[S, M, C]: the model's outputs at ``x`` under each row of ``samples`` [S, n_params]; classification: their softmax."""
        regression = self.likelihood == "regression"
        if self._nn_device_route():  # one pass on the device, the parameters are never written
            return self.backend.sampled_forward(x, samples, softmax=not regression)
        outs = []
        try:
            for theta in samples:
                vector_to_parameters(theta, self.params)
                f = self.model(x)
                outs.append(f if regression else torch.softmax(f, dim=-1))
        finally:
            vector_to_parameters(self.mean.clone(), self.params)  # the parameters must not alias self.mean afterwards
        return torch.stack(outs)

    @torch.no_grad()
    def _nn_predictive_samples(self, x, n_samples: int = 100, generator: torch.Generator | None = None,
                               eps: torch.Tensor | None = None):
        """laplace/baselaplace.py:1160-1181: [S, M, C] outputs of the model under S posterior samples (classification: their
        softmax).  ``eps``: [n_samples, n_params] standard normal draws instead of the generator."""
        return self._nn_forward_samples(x.to(self._device), self.sample(n_samples, generator=generator, eps=eps))

    @torch.no_grad()
    def predictive_samples(self, x, pred_type: str = "glm", n_samples: int = 100, diagonal_output: bool = False,
                           generator: torch.Generator | None = None, eps: torch.Tensor | None = None):
        """Samples of the posterior predictive [n_samples, M, C] (laplace/baselaplace.py:1074-1120).  ``"glm"``: samples of the
        linearised model's ``N(f_mu, f_var)`` through the link (``diagonal_output``: of its diagonal); ``"nn"``: the network
        under parameter samples.  ``eps`` replaces the random draws ([n_outputs, n_samples] for "glm", [n_samples, n_params]
        for "nn")."""
        if pred_type not in ("glm", "nn"):
            raise ValueError("Only glm and nn supported as prediction types.")
        if pred_type == "nn":
            return self._nn_predictive_samples(x, n_samples, generator=generator, eps=eps)
        x = x.to(self._device)
        f_mu, f_var = self._glm_predictive_distribution(x)
        return self._glm_predictive_samples(f_mu, f_var, n_samples, diagonal_output, generator, eps)

    # ---- GLM predictive ("next" row 8(f)-3) ---------------------------------------------------------------------
    def functional_variance(self, Js: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def _covariance_rows(self, J: torch.Tensor) -> torch.Tensor:
        """``J P^-1`` [R, P] for rows ``J`` [R, P] of Jacobians: what the cross-node covariance multiplies with the other
        side's rows."""
        raise NotImplementedError

    def functional_covariance(self, Js: torch.Tensor) -> torch.Tensor:
        """``[M C, M C]`` joint covariance ``J P^-1 J^T`` of Jacobians ``Js`` [M, C, P] (laplace/baselaplace.py:1491-1494,
        :1638-1644, :1905-1910), symmetrised (the two triangles differ in the last bit otherwise)."""
        if Js.ndim != 3 or Js.shape[1:] != (self.n_outputs, self._n_params_posterior):
            raise ValueError("Invalid Jacobians shape for Laplace posterior approx.")
        J = Js.reshape(Js.shape[0] * Js.shape[1], Js.shape[2])
        cov = self._covariance_rows(J) @ J.T
        return 0.5 * (cov + cov.T)

    def _covariance_operands(self):
        """``dict(QA, QB, S)`` of ``GraphEngine.glm_covariance`` -- one entry per Linear block of the model -- for this
        posterior, or None when the device route does not apply (the chunked Jacobian route in torch serves it then)."""
        return None

    def _glm_covariance_device(self, xa, xb):
        """``J(xa) P^-1 J(xb)^T`` from ``lgnn_glm_covariance`` (csrc/glmcov.hip), or None: Kronecker and diagonal posteriors
        over all weights, any model, either likelihood.  ``xb=None``: the same nodes on both sides."""
        be = self.backend
        eng = getattr(be, "engine", None)
        if eng is None or not hasattr(be, "glm_covariance") or not hasattr(eng, "glm_covariance"):
            return None
        if getattr(be, "last_layer", False) or getattr(be, "subnetwork_indices", None) is not None:
            return None
        ops = self._covariance_operands()
        if ops is None or len(ops["S"]) != len(eng.block_dims):
            return None
        return be.glm_covariance(xa, xb, **ops)

    def _glm_covariance_jacobians(self, xa, xb):
        """``(J(xa) P^-1 J(xb)^T, f(xa))`` from chunk pairs of the backend's Jacobians: three chunks of rows (one side, its
        product with P^-1, the other side) stay under ``_JACOBIAN_BYTES_MAX``, so no ``[M, C, P]`` above it exists."""
        C, P = self.n_outputs, self._n_params_posterior
        same = xb is None
        xb = xa if same else xb
        Ma, Mb = int(xa.shape[0]), int(xb.shape[0])
        chunk = max(1, self._JACOBIAN_BYTES_MAX // (3 * max(1, C * P * 4)))
        K = torch.empty(Ma * C, Mb * C, device=self._device)
        mus = []
        for a0 in range(0, Ma, chunk):
            Ja, f_mu = self.backend.jacobians(xa[a0:a0 + chunk], enable_backprop=False)
            if Ja.shape[1:] != (C, P):
                raise ValueError("Invalid Jacobians shape for Laplace posterior approx.")
            mus.append(f_mu)
            Ja = Ja.reshape(-1, P)
            SJa = self._covariance_rows(Ja)
            for b0 in range(a0 if same else 0, Mb, chunk):
                if same and b0 == a0:
                    blk = SJa @ Ja.T
                    blk = 0.5 * (blk + blk.T)
                else:
                    blk = SJa @ self.backend.jacobians(xb[b0:b0 + chunk], enable_backprop=False)[0].reshape(-1, P).T
                K[a0 * C:a0 * C + blk.shape[0], b0 * C:b0 * C + blk.shape[1]] = blk
                if same and b0 != a0:
                    K[b0 * C:b0 * C + blk.shape[1], a0 * C:a0 * C + blk.shape[0]] = blk.T
            del Ja, SJa
        return K, (mus[0] if len(mus) == 1 else torch.cat(mus))

    @torch.no_grad()
    def glm_covariance(self, x, x_other=None) -> torch.Tensor:
        """``Cov[f(x), f(x_other)]`` [M C, M' C] of the linearised model, ``J(x) P^-1 J(x_other)^T``: the cross block between
        two node lists (candidates against test nodes; the reference's ``functional_covariance`` only ever gives the square
        block).  ``x_other=None``: the square block of ``x``, exactly symmetric.  Either likelihood."""
        x = x.to(self._device)
        x_other = None if x_other is None else x_other.to(self._device)
        K = self._glm_covariance_device(x, x_other)
        return K if K is not None else self._glm_covariance_jacobians(x, x_other)[0]

    def _matrix_free_operands(self, out_map=None):
        """Operands of ``GraphEngine.glm_variance`` for this posterior (mapped by ``out_map`` = E [Cm, C] where they depend on
        the outputs), or None when the matrix-free route does not apply."""
        return None

    def _glm_variance_matrix_free(self, x, out_map=None):
        """(f_mu [M, C], diag f_var [M, C]) without Jacobians (csrc/predictive.hip), or None: 2-layer GCN / GraphSAGE models
        with a ReLU and hidden width <= 256, and 1-layer ones, classification, Kronecker or diagonal posterior over all weights.  ``out_map`` =
        E [Cm, C]: the variances of E f instead ([M, Cm]).  Models built with res / norm take the per-class table route
        (``GraphEngine.glm_variance_ext``), plain ones the entry they always had."""
        eng = getattr(self.backend, "engine", None)
        extras = bool(getattr(eng, "has_extras", False))
        if (eng is None or not hasattr(eng, "glm_variance") or getattr(eng, "kind", None) not in ("gcn", "sage")
                or len(eng.dims) not in (2, 3) or (extras and not hasattr(eng, "glm_variance_ext"))
                or self.likelihood != "classification"):
            return None
        # (a 1-layer model has no hidden layer: no width limit, any activation)
        if len(eng.dims) == 3 and (eng.dims[1] > 256 or eng.act != "relu"):
            return None
        ops = self._matrix_free_operands(out_map)
        if ops is None:
            return None
        if ("Sr" in ops) != bool(getattr(eng, "has_res", False)):  # the res.0 block comes with a res model, and only with one
            return None
        eng.set_likelihood("classification")
        if extras and len(eng.dims) == 3:
            return eng.glm_variance_ext(x, out_map=out_map, **ops)
        return eng.glm_variance(x, **ops) if out_map is None else eng.glm_variance(x, out_map=out_map, **ops)

    def _bridge_moments_matrix_free(self, x):
        """What the Laplace bridge reads of the C x C predictive covariance S (laplace/baselaplace.py:637-661) -- its diagonal,
        its row sums S 1 and its total 1^T S 1 -- without Jacobians, or None.  One matrix-free pass over the 2 C + 1 outputs
        E f, E = [I ; 1^T / C ; I + 1 1^T / C]: with m = mean(f), var(f_c + m) - var(f_c) - var(m) = 2 cov(f_c, m) = 2 (S 1)_c / C
        and 1^T S 1 = C^2 var(m) (polarisation against the MEAN keeps the three terms at the same magnitude)."""
        C = self.n_outputs
        eye = torch.eye(C, device=self._device)
        ones = torch.full((1, C), 1.0 / C, device=self._device)
        fast = self._glm_variance_matrix_free(x, out_map=torch.cat([eye, ones, eye + ones], dim=0))
        if fast is None:
            return None
        f_mu, v = fast
        diag, vm, vsum = v[:, :C], v[:, C:C + 1], v[:, C + 1:]
        return f_mu, diag, 0.5 * C * (vsum - diag - vm), (C * C) * vm.squeeze(1)

    _JACOBIAN_BYTES_MAX = 1 << 30  # above this size of Js [M, C, P] the full-covariance links go matrix free where they can

    def _glm_covariance_matrix_free(self, x, budget_floats: int = 1 << 30):
        """(f_mu [M, C], f_var [M, C, C]) without Jacobians, or None: the C (C + 1) / 2 variances var(f_c + f_c') of one
        matrix-free pass (lgnn_glm_variance_mapped) give every entry by polarisation, cov(f_c, f_c') = (var(f_c + f_c') -
        var(f_c) - var(f_c')) / 2.  Evaluation nodes go in chunks sized so that the rotated-row table of a chunk (needed nodes x
        pairs x hidden floats) stays near ``budget_floats``.  Off-diagonal entries carry the rounding of the three variances
        (absolute ~1e-6 of the diagonal): what ``link_approx="mc"`` needs of a model whose Jacobians do not fit."""
        C = self.n_outputs
        iu = torch.triu_indices(C, C, device=self._device)
        if iu.shape[1] > 4096:
            return None
        E = torch.zeros(iu.shape[1], C, device=self._device)
        ar = torch.arange(iu.shape[1], device=self._device)
        E[ar, iu[0]] += 1.0
        E[ar, iu[1]] += 1.0
        eng = getattr(self.backend, "engine", None)
        if eng is None:
            return None
        per_node = iu.shape[1] * eng.dims[1] * (eng.nnz / max(eng.num_nodes, 1) + 2.0)  # table floats per evaluation node
        chunk = max(1, int(budget_floats / per_node))
        dsel = (iu[0] == iu[1]).nonzero().squeeze(1)  # positions of the pairs (c, c): var(2 f_c) = 4 var(f_c)
        mus, covs = [], []
        for s0 in range(0, x.shape[0], chunk):
            fast = self._glm_variance_matrix_free(x[s0:s0 + chunk], out_map=E)
            if fast is None:
                return None
            f_mu, v = fast
            d = 0.25 * v[:, dsel]
            off = 0.5 * (v - d[:, iu[0]] - d[:, iu[1]])
            cov = torch.zeros(v.shape[0], C, C, device=v.device)
            cov[:, iu[0], iu[1]] = off
            cov[:, iu[1], iu[0]] = off
            cov[:, dsel.new_tensor(range(C)), dsel.new_tensor(range(C))] = d
            mus.append(f_mu)
            covs.append(cov)
        return torch.cat(mus), torch.cat(covs)

    def _glm_predictive_distribution(self, x, diagonal_output: bool = False, joint: bool = False):
        """(f_mu [M, C], f_var [M, C, C]) (laplace/baselaplace.py:1123-1158); ``diagonal_output``: f_var [M, C], matrix free
        where the model family allows it; ``joint``: (f_mu [M C], f_cov [M C, M C]) over all evaluation nodes (:1145-1147),
        on the device for Kronecker and diagonal posteriors over all weights."""
        if joint:
            f_cov = self._glm_covariance_device(x, None)
            if f_cov is not None:
                return self.backend.engine.forward(x).flatten(), f_cov
            f_cov, f_mu = self._glm_covariance_jacobians(x, None)
            return f_mu.flatten(), f_cov
        if diagonal_output:
            fast = self._glm_variance_matrix_free(x)
            if fast is not None:
                return fast
        # Jacobian route (models with res / norm, deeper models, full posteriors): the reference forms Js [M, C, P] for all
        # evaluation nodes at once (laplace/baselaplace.py:1123-1158), which cannot exist at scale; here the nodes go in chunks
        # whose Jacobians stay under _JACOBIAN_BYTES_MAX -- the same numbers, any M
        per_node = max(1, self.n_outputs * self._n_params_posterior * 4)
        chunk = max(1, min(int(x.shape[0]), self._JACOBIAN_BYTES_MAX // per_node))
        mus, fvars = [], []
        for s0 in range(0, max(int(x.shape[0]), 1), chunk):
            Js, f_mu = self.backend.jacobians(x[s0:s0 + chunk], enable_backprop=False)
            if Js.shape[1:] != (self.n_outputs, self._n_params_posterior):
                raise ValueError("Invalid Jacobians shape for Laplace posterior approx.")
            f_var = self.functional_variance(Js)
            if diagonal_output:
                f_var = torch.diagonal(f_var, dim1=-2, dim2=-1)
            mus.append(f_mu)
            fvars.append(f_var)
            del Js
        return (mus[0], fvars[0]) if len(mus) == 1 else (torch.cat(mus), torch.cat(fvars))
