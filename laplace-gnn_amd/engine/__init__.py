"""Python handle on one ``lgnn_ctx`` (graph + bound model + caches) of the HIP library.

PyTorch-ROCm is used for device memory and streams only: every tensor is handed over as a raw device pointer, the current
torch stream as a ``hipStream_t``.  No CPU fallback exists.  One class, cut by family like the library under it: ``_marshal``
(what crosses the ABI), ``core`` (lifetime, ``_call`` and the borrow rule, graph, bind, forward) and the four mixins."""
from ._marshal import ACTS, KINDS, LIKS, NORMS, BatchTagMap, _IdentityKey  # noqa: F401
from .core import EngineCore
from .curvature import CurvatureEntries, kfac_plan  # noqa: F401
from .matfree import MatrixFreeEntries
from .structure import StructureEntries
from .train import TrainingEntries


class GraphEngine(EngineCore, CurvatureEntries, MatrixFreeEntries, StructureEntries, TrainingEntries):
    """Graph ingest + model binding + per-batch curvature accumulation on one GPU."""
