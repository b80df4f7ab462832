"""Thin ``Laplace`` front for the curvature path: the caller of the backend.

Mirrors what the fit path of the reference does and nothing else:
``Laplace`` factory (laplace/laplace.py:13-47), ``BaseLaplace.__init__`` parameter filter and lazy
backend (laplace/baselaplace.py:94-190), ``ParametricLaplace.fit`` (:778-854), ``KronLaplace``
(:1556-1610 incl. the ``override=False`` discounting), ``DiagLaplace`` (:1848-1857), and the
last-layer ``FullLLLaplace`` / ``KronLLLaplace`` / ``DiagLLLaplace`` (laplace/lllaplace.py:369-378, 381-475, 477-... intent).  Attributes after ``fit``:
``H``, ``H_facs`` (kron), ``loss``, ``n_data``, ``n_outputs``, ``n_params``, ``mean``,
``model.output_size``.

Data parallelism (new; the reference is single process).  The accumulated factors + loss are summed
with ONE all-reduce of a flat fp32 buffer (RCCL over xGMI on GPUs, gloo in the CPU tests).  What is
dealt to the ranks of the ``torch.distributed`` group depends on the structure:
* kron: a batch's SAMPLES are never split -- the B factors have cross-sample terms inside a batch
  (SURVEY.md 0.5), so the reference loader's boundaries are part of the result -- but
  ``B = sum_batches sum_classes g_c^T g_c``, so the unit of work is (batch, class column) and the T*C
  units are dealt in balanced contiguous runs (``data.units_of_rank``); backends without class-range
  support get whole batches round-robin (batch t -> rank t mod world);
* diag / last layer (full, kron, diag): plain sums over samples -> every rank takes its slice of every batch.

One module per concern (``dist``, ``base``, ``fit``, ``predictive``, ``marglik``) and per posterior family; DESIGN.md 12.36.
"""
from torch import nn

from ..adjgrad import _adjacency_candidates, _adjgrad_drive, _adjgrad_scope, _dense_scope  # noqa: F401  (re-exported)
from ..curvature import HipGGN  # noqa: F401
from ..data import TensorBatchLoader  # noqa: F401
from ..matrix import Kron, KronDecomposed  # noqa: F401
from .base import BaseLaplace, _is_zero_number  # noqa: F401
from .diag import DiagLaplace  # noqa: F401
from .dist import _dist_info, all_reduce_flat_  # noqa: F401
from .fit import Accumulator, ParametricLaplace  # noqa: F401
from .full import FullLaplace, FullLLLaplace  # noqa: F401
from .kron import KronLaplace  # noqa: F401
from .lastlayer import DiagLLLaplace, KronLLLaplace, _LastLayerHead  # noqa: F401
from .lowrank_posterior import LowRankLaplace  # noqa: F401
from .predictive import _GLMLinkMixin  # noqa: F401
from .subnet import DiagSubnetLaplace, FullSubnetLaplace, SubnetLaplace  # noqa: F401


def _all_subclasses(cls) -> set:
    return set(cls.__subclasses__()).union([s for c in cls.__subclasses__() for s in _all_subclasses(c)])


def Laplace(model: nn.Module, likelihood: str, subset_of_weights: str = "last_layer",
            hessian_structure: str = "kron", *args, **kwargs) -> BaseLaplace:
    """String-keyed factory with the reference's call signature (laplace/laplace.py:13-47)."""
    if subset_of_weights == "subnetwork" and hessian_structure not in ["full", "diag"]:
        raise ValueError("Subnetwork Laplace requires a full or diagonal Hessian approximation!")
    if hessian_structure == "gp" and subset_of_weights != "all":
        raise NotImplementedError("FunctionalLLLaplace (a GP posterior over the last layer) is not implemented; "
                                  "use subset_of_weights='all'")
    laplace_map = {sub._key: sub for sub in _all_subclasses(BaseLaplace) if hasattr(sub, "_key")}
    key = (subset_of_weights, hessian_structure)
    if key not in laplace_map:
        raise NotImplementedError(f"{key} is outside the accelerated path; available: {sorted(laplace_map)}")
    return laplace_map[key](model, likelihood, *args, **kwargs)
