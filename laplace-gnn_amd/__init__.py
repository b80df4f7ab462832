"""MI355X-native curvature accumulation for ``Laplace(...).fit()`` on GCN / GraphSAGE models.

Only the hot path of anitasyang/Laplace-GNN is implemented: graph ingest,
the cached sparse forward, KFAC / diagonal / last-layer GGN accumulation as hand-written gfx950
kernels behind a C ABI (``include/laplace_gnn_hip.h``), a ``laplace.curvature``-compatible
backend class and the thin ``Laplace`` front that drives it.
"""
from . import _lib  # noqa: F401
from .curvature import HipCurvatureInterface, HipEF, HipGGN  # noqa: F401
from .data import TensorBatchLoader, batches_of_rank, units_of_rank  # noqa: F401
from .engine import GraphEngine  # noqa: F401
from .knn import get_knn_graph, knn, knn_candidates, knn_graph  # noqa: F401
from . import lowrank, subnetmask  # noqa: F401
from .laplace import (BaseLaplace, DiagLaplace, DiagLLLaplace, DiagSubnetLaplace, FullLaplace, FullLLLaplace,  # noqa: F401
                      FullSubnetLaplace, KronLaplace, KronLLLaplace, Laplace, LowRankLaplace, ParametricLaplace, SubnetLaplace,
                      all_reduce_flat_)
from .gp import FunctionalLaplace  # noqa: F401
from .matrix import Kron, KronDecomposed, symeig  # noqa: F401
from .subnetmask import (LargestMagnitudeSubnetMask, LargestVarianceDiagLaplaceSubnetMask,  # noqa: F401
                         LastLayerSubnetMask, ModuleNameSubnetMask, ParamNameSubnetMask, RandomSubnetMask, SubnetMask)
from .models import GCN, STEGCN, GraphSAGE, LoRASTEGCN  # noqa: F401

__all__ = ["GraphEngine", "HipGGN", "HipEF", "HipCurvatureInterface", "Laplace", "BaseLaplace", "ParametricLaplace",
           "KronLaplace", "DiagLaplace", "FullLaplace", "FullLLLaplace", "KronLLLaplace", "DiagLLLaplace", "Kron", "KronDecomposed", "symeig", "GCN", "STEGCN", "LoRASTEGCN", "GraphSAGE",
           "TensorBatchLoader", "batches_of_rank", "units_of_rank", "all_reduce_flat_", "knn", "knn_graph", "get_knn_graph",
           "knn_candidates", "SubnetLaplace", "FullSubnetLaplace", "DiagSubnetLaplace", "subnetmask", "SubnetMask",
           "RandomSubnetMask", "LargestMagnitudeSubnetMask", "LargestVarianceDiagLaplaceSubnetMask", "ParamNameSubnetMask",
           "ModuleNameSubnetMask", "LastLayerSubnetMask", "FunctionalLaplace", "LowRankLaplace"]
