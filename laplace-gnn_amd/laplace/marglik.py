"""What the parametric posteriors share around the marginal likelihood: scatter and log determinants, the post-hoc
prior-precision tuning, and serialisation."""
import warnings

import torch


class _MarglikMixin:
    @property
    def scatter(self) -> torch.Tensor:
        delta = self.mean - torch.as_tensor(self.prior_mean, device=self.mean.device, dtype=self.mean.dtype)
        return (delta * self.prior_precision_diag) @ delta

    @property
    def log_det_prior_precision(self) -> torch.Tensor:
        return self.prior_precision_diag.log().sum()

    @property
    def log_det_ratio(self) -> torch.Tensor:
        return self.log_det_posterior_precision - self.log_det_prior_precision

    def log_marginal_likelihood(self, prior_precision=None, sigma_noise=None) -> torch.Tensor:
        """laplace/baselaplace.py:938-973: ``log_lik - 0.5 (log det P - log det P_0 + scatter)``; passing
        ``prior_precision`` overwrites the current value (useful when iterating on the marginal likelihood)."""
        if prior_precision is not None:
            self.prior_precision = prior_precision
        if sigma_noise is not None:
            if self.likelihood != "regression":
                raise ValueError("Can only change sigma_noise for regression.")
            self.sigma_noise = sigma_noise
        return self.log_likelihood - 0.5 * (self.log_det_ratio + self.scatter)

    # ---- serialisation (laplace/baselaplace.py:1314-1368): plain dict of tensors and scalars, torch.save-able -----
    def state_dict(self) -> dict:
        if self.H is None:
            raise AttributeError("Laplace not fit. Run fit() first.")
        return {"mean": self.mean, "H": self.H, "loss": self.loss, "prior_mean": self.prior_mean,
                "prior_precision": self.prior_precision, "sigma_noise": self.sigma_noise, "n_data": self.n_data,
                "n_outputs": self.n_outputs, "likelihood": self.likelihood, "temperature": self.temperature,
                "enable_backprop": self.enable_backprop, "cls_name": self.__class__.__name__}

    def load_state_dict(self, state_dict: dict) -> None:
        if self.__class__.__name__ != state_dict["cls_name"]:
            raise ValueError("Loading a wrong Laplace type. Make sure `subset_of_weights` and `hessian_structure` "
                             "are correct!")
        if self.n_params is not None and len(state_dict["mean"]) != self.n_params:
            raise ValueError("Attempting to load Laplace with different number of parameters than the model.")
        if self.likelihood != state_dict["likelihood"]:
            raise ValueError("Different likelihoods detected!")
        if self.temperature != state_dict["temperature"]:
            warnings.warn("Different `temperature` parameters detected. Some calculation might be off!")
        for k in ("mean", "H", "loss", "prior_mean", "prior_precision", "sigma_noise", "n_data", "n_outputs",
                  "likelihood", "temperature", "enable_backprop"):
            setattr(self, k, state_dict[k])
        setattr(self.model, "output_size", self.n_outputs)

    # ---- post-hoc prior precision tuning (laplace/baselaplace.py:342-560) ------------------------------------------
    def optimize_prior_precision(self, pred_type: str = "glm", method: str = "marglik", n_steps: int = 100,
                                 lr: float = 1e-1, init_prior_prec=1.0, prior_structure: str = "scalar",
                                 val_loader=None, loss=None, log_prior_prec_min: float = -4,
                                 log_prior_prec_max: float = 4, grid_size: int = 100, link_approx: str = "probit",
                                 n_samples: int = 100, verbose: bool = False, progress_bar: bool = False) -> None:
        """``method="marglik"``: Adam on the log prior precision against ``-log_marginal_likelihood`` (the fitted
        factors and their decomposition are constants, only ``logdet(P)``, ``logdet(P_0)`` and the scatter term move:
        :444-463).  ``method="gridsearch"``: the value of a log-spaced grid with the lowest validation loss of the
        chosen predictive (:464-560; default loss = mean negative log likelihood of the predictive, the
        reference's RunningNLLMetric)."""
        if method == "marglik":
            pp = init_prior_prec if torch.is_tensor(init_prior_prec) else torch.tensor(float(init_prior_prec))
            pp = pp.detach().to(self._device, torch.float32).reshape(-1)
            if pp.numel() == 1 and prior_structure != "scalar":
                n = {"layerwise": self.n_layers, "diag": self._n_params_posterior}.get(prior_structure)
                if n is None:
                    raise ValueError(f"Invalid prior structure {prior_structure}.")
                pp = torch.full((n,), float(pp), device=self._device)
            log_pp = pp.log().clone().requires_grad_(True)
            opt = torch.optim.Adam([log_pp], lr=lr)
            with torch.enable_grad():
                for _ in range(n_steps):
                    opt.zero_grad()
                    neg = -self.log_marginal_likelihood(prior_precision=log_pp.exp())
                    neg.backward()
                    opt.step()
            self.prior_precision = log_pp.detach().exp()
        elif method == "gridsearch":
            if val_loader is None:
                raise ValueError("gridsearch requires a validation set DataLoader")
            if loss is None:
                def loss(probs, y):  # mean NLL of the predictive (laplace/utils/metrics.py RunningNLLMetric)
                    return float(torch.nn.functional.nll_loss(probs.clamp_min(1e-30).log(), y, reduction="mean"))
            best, best_pp = None, None
            for pp in torch.logspace(log_prior_prec_min, log_prior_prec_max, grid_size):
                self.prior_precision = pp
                try:
                    outs, ys = [], []
                    for X, y in val_loader:
                        outs.append(self(X.to(self._device), pred_type=pred_type, link_approx=link_approx,
                                         n_samples=n_samples))
                        ys.append(y.to(self._device))
                    val = loss(torch.cat(outs), torch.cat(ys))
                except RuntimeError:
                    val = float("inf")
                if best is None or val < best:
                    best, best_pp = val, pp
            self.prior_precision = best_pp
        else:
            raise ValueError("For now only marglik and gridsearch is implemented.")
        if verbose:
            print(f"Optimized prior precision is {self.prior_precision}.")
