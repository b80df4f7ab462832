"""Subnetwork Laplace: the posterior over a chosen subset of the weights, full or diagonal."""
import torch

from .diag import DiagLaplace
from .fit import ParametricLaplace
from .full import FullLaplace


class SubnetLaplace(ParametricLaplace):
    """Subnetwork Laplace (Daxberger et al. 2021; laplace/subnetlaplace.py:15-172): the posterior covers the ``S`` weights
    named by ``subnetwork_indices``, everything else stays at the MAP.  Full or diagonal Hessian structure only.

    ``subnetwork_indices`` index the LAPLACE PARAMETER VECTOR ``la.mean``: the parameters in ``named_parameters()`` order
    without names containing ``adj`` or ``norms`` (the fork's filter, laplace/baselaplace.py:118-122), each flattened row
    major -- the vector ``lgnn_jacobians`` and ``FullLaplace.H`` use.  (The reference documents
    ``parameters_to_vector(model.parameters())``; for its GNNs that vector contains the dense ``adj`` and is not the one its
    own ``SubnetLaplace`` checks the indices against.)  Non-empty 1-D int64, in ``[0, n_params)``, no duplicates, any device,
    any order: ``H``, ``prior_precision_diag``, ``mean_subnet`` and the Jacobians follow the order of the indices.
    ``laplace_gnn_amd.subnetmask`` builds such index sets.

    ``n_params`` stays the size of the whole vector (``mean``, ``sample()``), ``n_params_subnet = S`` is the size of ``H``.
    The prior is scalar or a length-``S`` diagonal.  Marginal likelihood, prior-precision tuning, the GLM predictive with
    every link, ``state_dict`` and the ``process_group`` reduction are the inherited code on the ``S``-sized objects;
    ``sample()`` returns full ``[n, P]`` vectors, so ``pred_type="nn"`` works unchanged."""

    def __init__(self, model, likelihood, subnetwork_indices, *args, asdl_fisher_kwargs=None, **kwargs):
        if asdl_fisher_kwargs is not None:
            raise ValueError("Subnetwork Laplace does not support asdl_fisher_kwargs.")
        super().__init__(model, likelihood, *args, **kwargs)
        self._check_subnetwork_indices(subnetwork_indices)
        self.subnetwork_indices = subnetwork_indices.detach().to(self._device).contiguous()
        # laplace/subnetlaplace.py:108-112: the backend learns the indices after its construction (a backend that cannot
        # serve a subnetwork -- HipEF, last_layer / stochastic flags -- refuses here, by name)
        self.backend.subnetwork_indices = self.subnetwork_indices
        self.n_params_subnet = int(subnetwork_indices.numel())
        self._init_H()

    def _check_subnetwork_indices(self, subnetwork_indices) -> None:
        """laplace/subnetlaplace.py:114-138, against the Laplace parameter vector; one host round trip per construction."""
        if subnetwork_indices is None:
            raise ValueError("Subnetwork indices cannot be None.")
        if not (torch.is_tensor(subnetwork_indices) and subnetwork_indices.dtype == torch.int64
                and subnetwork_indices.dim() == 1 and subnetwork_indices.numel() > 0):
            raise ValueError("Subnetwork indices must be non-empty 1-dimensional torch.LongTensor.")
        if bool(((subnetwork_indices < 0) | (subnetwork_indices >= self.n_params)).any()):
            raise ValueError(f"Subnetwork indices must lie between 0 and n_params={self.n_params}.")
        if subnetwork_indices.unique().numel() != subnetwork_indices.numel():
            raise ValueError("Subnetwork indices must not contain duplicate entries.")

    @property
    def _n_params_posterior(self) -> int:
        return self.n_params_subnet

    @property
    def prior_precision_diag(self) -> torch.Tensor:
        """Scalar or length-S diagonal prior (laplace/subnetlaplace.py:140-158)."""
        pp = torch.as_tensor(self.prior_precision, dtype=torch.float32, device=self._device).reshape(-1)
        if pp.numel() == 1:
            return pp.expand(self.n_params_subnet).clone()
        if pp.numel() == self.n_params_subnet:
            return pp
        raise ValueError("Mismatch of prior and model. Diagonal or scalar prior.")

    @property
    def mean_subnet(self) -> torch.Tensor:
        return self.mean[self.subnetwork_indices.to(self.mean.device)]

    @property
    def scatter(self) -> torch.Tensor:
        delta = self.mean_subnet - torch.as_tensor(self.prior_mean, device=self.mean.device, dtype=self.mean.dtype)
        return (delta * self.prior_precision_diag) @ delta

    def assemble_full_samples(self, subnet_samples: torch.Tensor) -> torch.Tensor:
        """[n, S] samples of the subnetwork -> [n, P] parameter vectors, the MAP everywhere else
        (laplace/subnetlaplace.py:169-172)."""
        full_samples = self.mean.repeat(subnet_samples.shape[0], 1)
        full_samples[:, self.subnetwork_indices.to(self.mean.device)] = subnet_samples.to(full_samples.dtype)
        return full_samples

    def sample(self, n_samples: int = 100, generator: torch.Generator | None = None, eps: torch.Tensor | None = None):
        """Full parameter vectors [n, P] (laplace/subnetlaplace.py:191-198, 224-233); ``eps``: [n, S] standard normal draws."""
        if eps is None:
            eps = torch.randn(n_samples, self.n_params_subnet, device=self._device, generator=generator)
        return self.assemble_full_samples(self.mean_subnet.reshape(1, -1) + self._scale_samples(eps.to(self._device)))

    def _matrix_free_operands(self, out_map=None):
        return None  # the matrix-free predictive covers posteriors over all weights; here: Jacobian columns [M, C, S]

    def _covariance_operands(self):
        return None  # (likewise the joint predictive: chunk pairs of the selected columns)

    def state_dict(self) -> dict:
        state = super().state_dict()
        state["subnetwork_indices"] = self.subnetwork_indices
        return state

    def load_state_dict(self, state_dict: dict) -> None:
        if tuple(state_dict["H"].shape) != tuple(self.H.shape):
            raise ValueError(f"Attempting to load a subnetwork Laplace with H of shape {tuple(state_dict['H'].shape)} into "
                             f"one with {tuple(self.H.shape)}.")
        saved = state_dict.get("subnetwork_indices")
        if saved is not None and not torch.equal(saved.to(self.subnetwork_indices.device), self.subnetwork_indices):
            raise ValueError("Attempting to load a subnetwork Laplace fitted on different subnetwork indices.")
        super().load_state_dict(state_dict)

    def neg_marglik_adj_grad(self, *args, **kwargs):
        raise NotImplementedError("adjacency gradient under a subnetwork posterior is not implemented "
                                  "(KronLaplace, DiagLaplace and FullLaplace over all weights offer it)")

    def propose_edges(self, *args, **kwargs):
        raise NotImplementedError("propose_edges under a subnetwork posterior is not implemented (DiagLaplace over all weights "
                                  "offers it)")


class FullSubnetLaplace(SubnetLaplace, FullLaplace):
    """Dense ``S x S`` posterior precision over the subnetwork (laplace/subnetlaplace.py:175-199).  With the HIP backend only
    the selected Jacobian columns are built (``lgnn_subnet_full_accumulate``): M C S floats and 2 M C S^2 flops per batch
    where ``FullLaplace`` needs M C P and 2 M C P^2."""
    _key = ("subnetwork", "full")

    def _init_H(self):
        self.H = torch.zeros(self.n_params_subnet, self.n_params_subnet, device=self._device)
        self._posterior_scale = None


class DiagSubnetLaplace(SubnetLaplace, DiagLaplace):
    """Diagonal posterior precision over the subnetwork (laplace/subnetlaplace.py:201-233): the existing closed-form diagonal
    indexed by the subnetwork.  Plain per-batch path (no in-place buffer, no captured-graph fit)."""
    _key = ("subnetwork", "diag")
    fit_graph = False

    fit = ParametricLaplace.fit  # (never captured)

    def _init_H(self):
        self._hl = None
        self.H = torch.zeros(self.n_params_subnet, device=self._device)
