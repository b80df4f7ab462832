"""Helpers shared by the subnetwork-Laplace tests (CPU and GPU): models rebuilt from golden fixtures, the subnet goldens'
index sets, the offsets of named parameters inside the Laplace parameter vector."""
import os

import numpy as np
import torch

from conftest import GOLDEN
from golden_utils import constructor_extras

SUBNET_GOLDEN = os.path.join(GOLDEN, "subnet")
SUBNET_CASES = ("gcn_small_1batch_s0", "sage_small_1batch_s0", "gcn3_small_1batch_s0", "sage_resln_small_1batch_s0")
SETS = ("rand", "struct")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def model_from_golden(g, device=None):
    import laplace_gnn_amd as lg

    kind, L = str(g["kind"]), int(g["num_layers"])
    X, ei = torch.from_numpy(g["X"]), torch.from_numpy(g["edge_index"])
    cls = lg.GCN if kind == "gcn" else lg.GraphSAGE
    m = cls(X.shape[1], g["W0"].shape[0], g[f"W{L - 1}"].shape[0], L, X, ei, symmetric=bool(g["symmetric"]),
            **constructor_extras(g))
    with torch.no_grad():
        for l, conv in enumerate(m.convs):
            conv.lin.weight.copy_(torch.from_numpy(g[f"W{l}"]))
            conv.lin.bias.copy_(torch.from_numpy(g[f"b{l}"]))
        for l, lin in enumerate(m.res):
            lin.weight.copy_(torch.from_numpy(g[f"Wr{l}"]))
            lin.bias.copy_(torch.from_numpy(g[f"br{l}"]))
        if m.norm_kind is not None:
            for l, nm in enumerate(m.norms):
                nm.weight.copy_(torch.from_numpy(g[f"norm_w{l}"]))
                nm.bias.copy_(torch.from_numpy(g[f"norm_b{l}"]))
                if m.norm_kind == "batch":
                    nm.running_mean.copy_(torch.from_numpy(g[f"norm_rm{l}"]))
                    nm.running_var.copy_(torch.from_numpy(g[f"norm_rv{l}"]))
    m.eval()
    return m.to(device) if device else m


def param_ranges(model):
    """{name: (offset, numel)} of the Laplace parameter vector (named_parameters order without ``adj`` / ``norms``)."""
    out, off = {}, 0
    for k, p in model.named_parameters():
        if p.requires_grad and "adj" not in k and "norms" not in k:
            out[k] = (off, p.numel())
            off += p.numel()
    return out


def subnet_golden(case):
    return np.load(os.path.join(SUBNET_GOLDEN, case + ".npz"))
