"""MI355X-native curvature accumulation for ``Laplace(...).fit()`` on GCN / GraphSAGE models.

Only the hot path of anitasyang/Laplace-GNN is implemented: graph ingest,
the cached sparse forward, KFAC / diagonal / last-layer GGN accumulation as hand-written gfx950
kernels behind a C ABI (``include/laplace_gnn_hip.h``), a ``laplace.curvature``-compatible
backend class and the thin ``Laplace`` front that drives it.
"""
from . import _lib  # noqa: F401
from .curvature import HipCurvatureInterface, HipEF, HipGGN, HipHessian  # noqa: F401
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
from .models import GCN, STEGCN, GraphSAGE, LoRASTEGCN, STEGraphSAGE  # noqa: F401

__all__ = ["BaseLaplace", "DiagLLLaplace", "DiagLaplace", "DiagSubnetLaplace", "FullLLLaplace", "FullLaplace",
           "FullSubnetLaplace", "FunctionalLaplace", "GCN", "GraphEngine", "GraphSAGE", "HipCurvatureInterface", "HipEF",
           "HipGGN", "HipHessian", "Kron", "KronDecomposed", "KronLLLaplace", "KronLaplace", "Laplace", "LargestMagnitudeSubnetMask",
           "LargestVarianceDiagLaplaceSubnetMask", "LastLayerSubnetMask", "LoRASTEGCN", "LowRankLaplace",
           "ModuleNameSubnetMask", "ParamNameSubnetMask", "ParametricLaplace", "RandomSubnetMask", "STEGCN", "STEGraphSAGE",
           "SubnetLaplace", "SubnetMask", "TensorBatchLoader", "all_reduce_flat_", "batches_of_rank", "get_knn_graph", "knn", "knn_candidates",
           "knn_graph", "subnetmask", "symeig", "units_of_rank"]
