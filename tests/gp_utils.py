"""Helpers shared by the functional-Laplace tests (CPU and GPU): the goldens of tools/make_gp_golden.py, models rebuilt from
them, and a test-only fp64 backend for the activation the CPU oracle does not cover."""
import os

import numpy as np
import torch
from torch.nn import CrossEntropyLoss, MSELoss

from conftest import GOLDEN
from golden_utils import constructor_extras

GP_GOLDEN = os.path.join(GOLDEN, "gp")
GP_CASES = ("gcn_small", "sage_small", "gcn_mid", "gcn_regression", "gcn_tanh", "gcn3_small", "sage_resln_small")
PREFIXES = ("full", "indep")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def gp_golden(case):
    return np.load(os.path.join(GP_GOLDEN, case + ".npz"))


def gp_model(g, device=None):
    import laplace_gnn_amd as lg

    kind, L = str(g["kind"]), int(g["num_layers"])
    X, ei = torch.from_numpy(g["X"]), torch.from_numpy(g["edge_index"])
    cls = lg.GCN if kind == "gcn" else lg.GraphSAGE
    m = cls(X.shape[1], g["W0"].shape[0], g[f"W{L - 1}"].shape[0], L, X, ei, symmetric=bool(g["symmetric"]), act=str(g["act"]),
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
    m.eval()
    return m.to(device) if device else m


def gp_loader(g, device="cpu"):
    import laplace_gnn_amd as lg

    return lg.TensorBatchLoader(torch.from_numpy(g["train_idx"]).to(device), torch.from_numpy(g["train_y"]).to(device),
                                batch_size=int(g["batch_size"]))


class ActBackend:
    """TEST ONLY: ``jacobians`` in fp64 by autograd (tests/act_reference.py), any activation; no ``gp_kernel``, so the front
    takes its einsum route."""

    def __init__(self, model, likelihood, dict_key_x="input_ids", dict_key_y="labels", **kwargs):
        import gnn_laplace_oracle as O
        from act_reference import ActReference

        self.model, self.likelihood = model, likelihood
        self.lossfunc, self.factor = (MSELoss(reduction="sum"), 0.5) if likelihood == "regression" else (
            CrossEntropyLoss(reduction="sum"), 1.0)
        rp, col = O.edge_index_to_adj_csr(model.edge_index.numpy(), model.num_nodes, model.kind, model.symmetric)
        kw = {}
        if len(getattr(model, "res", [])):
            kw.update(res_weights=[r.weight for r in model.res], res_biases=[r.bias for r in model.res])
        if getattr(model, "norm_kind", None) is not None:
            kw.update(norm=model.norm_kind, norm_eps=float(model.norms[0].eps), norm_weight=[n.weight for n in model.norms],
                      norm_bias=[n.bias for n in model.norms])
        self.ref = ActReference(model.kind, O.propagation_matrix(rp, col, model.kind), model.X,
                                [c.lin.weight for c in model.convs], [c.lin.bias for c in model.convs],
                                act=model.act_name,
                                likelihood=likelihood, **kw)

    def jacobians(self, x, enable_backprop=False):
        with torch.enable_grad():  # (the front's predictive runs under no_grad)
            return self.ref.jacobians(x)
