"""``BaseLaplace``: parameter filter, lazy backend, prior precision, likelihood term."""
from math import log, pi
from typing import Any

import torch
from torch import nn
from torch.nn.utils import parameters_to_vector

from ..curvature import HipGGN


class BaseLaplace:
    def __init__(self, model: nn.Module, likelihood: str, sigma_noise: float = 1.0, prior_precision: float = 1.0,
                 prior_mean: float = 0.0, temperature: float = 1.0, enable_backprop: bool = False,
                 dict_key_x: str = "input_ids", dict_key_y: str = "labels", backend: type | None = None,
                 backend_kwargs: dict[str, Any] | None = None, asdl_fisher_kwargs: dict[str, Any] | None = None):
        if likelihood not in ("classification", "regression", "reward_modeling"):
            raise ValueError(f"Invalid likelihood type {likelihood}")
        self.model, self.likelihood = model, likelihood
        # only do Laplace on params that require grad; the fork also drops 'adj' / 'norms' (baselaplace.py:118-122)
        self.params, self.is_subset_params = [], False
        for k, p in model.named_parameters():
            if p.requires_grad and "adj" not in k and "norms" not in k:
                self.params.append(p)
            else:
                self.is_subset_params = True
        self.n_params = sum(p.numel() for p in self.params)
        self.n_layers = len(self.params)
        if sigma_noise != 1 and likelihood != "regression":
            raise ValueError("Sigma noise != 1 only available for regression.")
        self.sigma_noise, self.temperature = sigma_noise, temperature
        self.prior_precision, self.prior_mean = prior_precision, prior_mean
        self.enable_backprop = enable_backprop
        self.dict_key_x, self.dict_key_y = dict_key_x, dict_key_y
        self._backend = None
        self._backend_cls = HipGGN if backend is None else backend
        self._backend_kwargs = dict() if backend_kwargs is None else backend_kwargs
        self._asdl_fisher_kwargs = dict() if asdl_fisher_kwargs is None else asdl_fisher_kwargs
        self.loss, self.n_outputs, self.n_data = 0.0, 0, 0

    @property
    def _device(self):
        # (walking named_parameters() costs 7 us per call on the host: a Cora-shaped fit asks twice and takes 0.2 ms in all)
        p = self.params[0] if self.params else next(self.model.parameters())
        return p.device

    @property
    def backend(self):
        if self._backend is None:
            lik = "classification" if self.likelihood == "reward_modeling" else self.likelihood
            self._backend = self._backend_cls(self.model, lik, dict_key_x=self.dict_key_x,
                                              dict_key_y=self.dict_key_y, **self._backend_kwargs)
        return self._backend

    def _begin_fit(self, train_loader) -> torch.device:
        """What every fit starts with: eval mode, ``mean``, ``n_outputs``, the model's ``output_size``.  Returns the device."""
        if self.model.training:
            self.model.eval()
        # the flattened parameters, recomputed on every fit exactly as laplace/baselaplace.py:800 does (one concatenation
        # kernel).  Version counters cannot stand in for it: ``p.data.add_()`` / ``p.data.copy_()`` do not bump
        # ``p._version``, and ``load_state_dict`` / ``la.mean = ...`` replace the vector behind any key
        self.mean = parameters_to_vector(self.params).detach()
        dev = self._device
        # the reference finds the output width with a forward pass of one sample (laplace/baselaplace.py:806-816); a model
        # that states it (laplace_gnn_amd.models.BaseGNN.n_outputs) saves that pass' launches -- a Cora-shaped fit is
        # launch bound
        self.n_outputs = getattr(self.model, "n_outputs", None)
        if self.n_outputs is None:
            X0 = next(iter(train_loader))[0]
            with torch.no_grad():
                try:
                    out = self.model(X0[:1].to(dev))
                except (TypeError, AttributeError):
                    out = self.model(X0.to(dev))
            self.n_outputs = out.shape[-1]
        setattr(self.model, "output_size", self.n_outputs)
        return dev

    def _block_prior_precision(self, n: int, dtype=torch.float32) -> torch.Tensor:
        """The prior precision per block, [n]: a scalar is expanded, anything else comes back flattened (callers refuse)."""
        pp = torch.as_tensor(self.prior_precision, dtype=dtype, device=self._device).reshape(-1)
        return pp.expand(n) if pp.numel() == 1 else pp

    @property
    def _H_factor(self):
        return 1 / self.sigma_noise ** 2 / self.temperature

    @property
    def _n_params_posterior(self) -> int:
        """Width of the posterior: the columns of the Jacobians the predictive asks its backend for (SubnetLaplace: S)."""
        return self.n_params

    @property
    def prior_precision_diag(self) -> torch.Tensor:
        pp = torch.as_tensor(self.prior_precision, dtype=torch.float32, device=self._device).reshape(-1)
        if pp.numel() == 1:
            return pp.expand(self.n_params).clone()
        if pp.numel() == self.n_params:
            return pp
        if pp.numel() == self.n_layers:
            return torch.cat([d.expand(p.numel()) for d, p in zip(pp, self.params)])
        raise ValueError("Mismatch of prior and model. Diagonal, scalar, or per-layer prior.")

    @property
    def log_likelihood(self) -> torch.Tensor:
        """laplace/baselaplace.py:895-922: -H_factor * loss for classification."""
        factor = -self._H_factor
        if self.likelihood == "regression":
            c = self.n_data * self.n_outputs * log(self.sigma_noise * (2 * pi) ** 0.5)
            return factor * self.loss - c
        return factor * self.loss


def _is_zero_number(v) -> bool:
    return isinstance(v, (int, float)) and v == 0
