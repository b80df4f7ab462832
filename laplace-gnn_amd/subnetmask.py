"""Subnetwork masks for ``SubnetLaplace``: ways to choose ``subnetwork_indices``.

The counterpart of laplace/utils/subnetmask.py:28-420, with one deliberate difference: every mask here works on the LAPLACE
PARAMETER VECTOR -- the parameters in ``named_parameters()`` order without names containing ``adj`` or ``norms`` and without
frozen ones (the fork's filter, laplace/baselaplace.py:118-122), each flattened row major; the vector ``la.mean``,
``lgnn_jacobians`` and ``FullLaplace.H`` use.  The reference builds its masks from ``model.parameters()``; its GNNs register
the dense ``adj`` as a parameter, so e.g. the largest-magnitude mask of a 64-node model ranks 64^2 adjacency entries next to
131 weights and returns indices its own ``SubnetLaplace`` refuses.

Nothing here touches the HIP engine: the masks work on a model on any device (``LargestVarianceDiagLaplaceSubnetMask`` runs
whatever ``DiagLaplace`` it is given).  ``LargestVarianceSWAGSubnetMask`` is not offered: it needs an SGD training loop of its
own.

    mask = lg.LargestMagnitudeSubnetMask(model, n_params_subnet=2048)
    la = lg.Laplace(model, "classification", "subnetwork", "full", subnetwork_indices=mask.select())
"""
from __future__ import annotations

import torch
from torch import nn
from torch.nn.utils import parameters_to_vector

__all__ = ["SubnetMask", "ScoreBasedSubnetMask", "RandomSubnetMask", "LargestMagnitudeSubnetMask",
           "LargestVarianceDiagLaplaceSubnetMask", "ParamNameSubnetMask", "ModuleNameSubnetMask", "LastLayerSubnetMask",
           "laplace_named_parameters"]


def laplace_named_parameters(model: nn.Module) -> list[tuple[str, nn.Parameter]]:
    """(name, parameter) of the Laplace parameter vector, in its order."""
    return [(k, p) for k, p in model.named_parameters() if p.requires_grad and "adj" not in k and "norms" not in k]


class SubnetMask:
    """Base class: ``select(train_loader=None)`` computes the indices once, ``indices`` / ``n_params_subnet`` read them back.
    Indices are sorted increasingly, int64, on the model's device."""

    def __init__(self, model: nn.Module) -> None:
        self.model = model
        self._named = laplace_named_parameters(model)
        if not self._named:
            raise ValueError("The model has no Laplace parameters.")
        self.parameter_vector = parameters_to_vector([p for _, p in self._named]).detach()
        self._n_params = int(self.parameter_vector.numel())
        self._indices = None
        self._n_params_subnet = None

    @property
    def _device(self) -> torch.device:
        return self.parameter_vector.device

    def _check_select(self) -> None:
        if self._indices is None:
            raise AttributeError("Subnetwork mask not selected. Run select() first.")

    @property
    def indices(self) -> torch.Tensor:
        self._check_select()
        return self._indices

    @property
    def n_params_subnet(self) -> int:
        if self._n_params_subnet is None:
            self._check_select()
            self._n_params_subnet = int(self._indices.numel())
        return self._n_params_subnet

    def convert_subnet_mask_to_indices(self, subnet_mask: torch.Tensor) -> torch.Tensor:
        """A 0/1 (integral or boolean) vector over the Laplace parameter vector -> the positions of its ones."""
        if not torch.is_tensor(subnet_mask):
            raise ValueError("Subnetwork mask needs to be torch.Tensor!")
        if subnet_mask.dtype.is_floating_point or subnet_mask.dtype.is_complex or subnet_mask.dim() != 1:
            raise ValueError("Subnetwork mask needs to be 1-dimensional integral or boolean tensor!")
        if subnet_mask.numel() != self._n_params or bool(((subnet_mask != 0) & (subnet_mask != 1)).any()):
            raise ValueError(f"Subnetwork mask needs to be a binary vector of size n_params={self._n_params} over the Laplace "
                             "parameter vector.")
        return subnet_mask.nonzero(as_tuple=True)[0]

    def select(self, train_loader=None) -> torch.Tensor:
        if self._indices is not None:
            raise ValueError("Subnetwork mask already selected.")
        self._indices = self.convert_subnet_mask_to_indices(self.get_subnet_mask(train_loader))
        return self._indices

    def get_subnet_mask(self, train_loader) -> torch.Tensor:
        raise NotImplementedError


class ScoreBasedSubnetMask(SubnetMask):
    """The ``n_params_subnet`` parameters with the highest score (ties: the lower index first)."""

    def __init__(self, model: nn.Module, n_params_subnet: int) -> None:
        super().__init__(model)
        if n_params_subnet is None:
            raise ValueError("Need to pass number of subnetwork parameters when using subnetwork Laplace.")
        if n_params_subnet > self._n_params:
            raise ValueError(f"Subnetwork ({n_params_subnet}) cannot be larger than model ({self._n_params}).")
        if n_params_subnet < 1:
            raise ValueError("The subnetwork needs at least one parameter.")
        self._n_params_subnet = int(n_params_subnet)
        self._param_scores = None

    def compute_param_scores(self, train_loader) -> torch.Tensor:
        raise NotImplementedError

    def get_subnet_mask(self, train_loader) -> torch.Tensor:
        if self._param_scores is None:
            self._param_scores = self.compute_param_scores(train_loader)
        if self._param_scores.shape != self.parameter_vector.shape:
            raise ValueError("Parameter scores need to be of same shape as parameter vector.")
        top = torch.argsort(self._param_scores, descending=True, stable=True)[:self._n_params_subnet]
        mask = torch.zeros(self._n_params, dtype=torch.bool, device=self._param_scores.device)
        mask[top] = True
        return mask


class RandomSubnetMask(ScoreBasedSubnetMask):
    """Parameters drawn uniformly at random; ``generator`` makes the draw reproducible (it lives on the CPU: the same
    subnetwork on every device)."""

    def __init__(self, model: nn.Module, n_params_subnet: int, generator: torch.Generator | None = None) -> None:
        super().__init__(model, n_params_subnet)
        self.generator = generator

    def compute_param_scores(self, train_loader) -> torch.Tensor:
        return torch.rand(self._n_params, generator=self.generator).to(self._device)


class LargestMagnitudeSubnetMask(ScoreBasedSubnetMask):
    """The parameters of largest absolute value."""

    def compute_param_scores(self, train_loader) -> torch.Tensor:
        return self.parameter_vector.abs()


class LargestVarianceDiagLaplaceSubnetMask(ScoreBasedSubnetMask):
    """The parameters of largest marginal variance under a diagonal Laplace posterior over all weights: ``select`` fits
    ``diag_laplace_model`` (a ``laplace_gnn_amd.DiagLaplace`` of the same model) on the loader."""

    def __init__(self, model: nn.Module, n_params_subnet: int, diag_laplace_model) -> None:
        super().__init__(model, n_params_subnet)
        self.diag_laplace_model = diag_laplace_model

    def compute_param_scores(self, train_loader) -> torch.Tensor:
        if train_loader is None:
            raise ValueError("Need to pass train loader for subnet selection.")
        self.diag_laplace_model.fit(train_loader)
        return (1.0 / self.diag_laplace_model.posterior_precision).detach()


class ParamNameSubnetMask(SubnetMask):
    """All entries of the named parameters (names as in ``model.named_parameters()``; Laplace parameters only)."""

    def __init__(self, model: nn.Module, parameter_names: list[str]) -> None:
        super().__init__(model)
        self._parameter_names = list(parameter_names)

    def get_subnet_mask(self, train_loader) -> torch.Tensor:
        if not self._parameter_names:
            raise ValueError("Parameter name list cannot be empty.")
        missing = [k for k in self._parameter_names if k not in dict(self._named)]
        if missing:
            raise ValueError(f"Parameters {missing} are not Laplace parameters of the model.")
        return torch.cat([torch.full((p.numel(),), k in self._parameter_names, dtype=torch.bool, device=self._device)
                          for k, p in self._named])


class ModuleNameSubnetMask(SubnetMask):
    """All Laplace parameters of the named leaf modules (names as in ``model.named_modules()``)."""

    def __init__(self, model: nn.Module, module_names: list[str]) -> None:
        super().__init__(model)
        self._module_names = list(module_names)

    def get_subnet_mask(self, train_loader) -> torch.Tensor:
        if not self._module_names:
            raise ValueError("Module name list cannot be empty.")
        modules = dict(self.model.named_modules())
        owner = [k.rpartition(".")[0] for k, _ in self._named]  # the module a Laplace parameter belongs to
        for name in self._module_names:
            if name not in modules:
                raise ValueError(f"Modules ['{name}'] do not exist in model.")
            if len(list(modules[name].children())) > 0:
                raise ValueError(f'Module "{name}" has children, which is not supported.')
            if name not in owner:
                raise ValueError(f'Module "{name}" does not have any Laplace parameters.')
        return torch.cat([torch.full((p.numel(),), o in self._module_names, dtype=torch.bool, device=self._device)
                          for o, (_, p) in zip(owner, self._named)])


class LastLayerSubnetMask(ModuleNameSubnetMask):
    """The head's weight and bias.  ``last_layer_name`` None: ``model.convs[-1].lin`` of the GCN / GraphSAGE models (not the
    last ``nn.Linear`` in module order, which is a residual Linear for ``res=True``); otherwise the last leaf module that owns
    Laplace parameters."""

    def __init__(self, model: nn.Module, last_layer_name: str | None = None) -> None:
        super().__init__(model, [])
        if last_layer_name is None:
            convs = getattr(model, "convs", None)
            head = getattr(convs[-1], "lin", None) if convs is not None and len(convs) else None
            if head is not None:
                last_layer_name = next(k for k, m in model.named_modules() if m is head)
            else:
                last_layer_name = self._named[-1][0].rpartition(".")[0]
        self._module_names = [last_layer_name]
