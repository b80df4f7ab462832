"""fp64 autograd restatement of the structure-learning loop's objective (gnn/marglik_training.py:197-216): the negative log
marginal likelihood of a Laplace posterior over a 2-layer STE-GCN / STE-GraphSAGE as a differentiable function of the dense
adjacency parameter, and its gradient.  The yardstick of the full posterior's adjacency gradient; with the diagonal log
determinant it reproduces the reference's own ``model.adj.grad`` goldens (tests/test_adjgrad_restatement.py), which pins it to
the reference.  Plain torch on the CPU: nothing from the oracle, nothing from the library.

    symmetric models          A <- (A + A^T) / 2
    straight-through          A <- A + ((A > 0.5) - A).detach()                       (identity in backward)
    GCN                       A <- A (1 - I) + I;  P = (A d)^T d, d = diag(rowsum^-1/2)
                              s = P (X W0^T + b0) [+ X Wr0^T + br0];  LayerNorm / eval-BatchNorm;  ReLU;  out = P (h W1^T + b1)
    GraphSAGE                 P = A / rowsum (zero row sums -> 1);  h = relu([X | P X] W0^T + b0);  out = [h | P h] W1^T + b1
    f = out[idx];  J = d f / d theta (graph kept);  H = sum_n J_n^T Lambda_n J_n
    neg = CE_sum + 1/2 (logdet - sum_p log delta_p) + 1/2 sum_p delta_p theta_p^2
    logdet = sum log(diag H + delta)  ("diag")   or   logdet(H + diag(delta))  ("full")

theta is ordered W0, b0, W1, b1[, Wr0, br0]; norm parameters are not part of it (laplace/curvature/curvature.py:74-79)."""
import numpy as np
import torch


def spec_from_golden(g):
    """The model of a golden fixture as the keyword arguments of ``neg_marglik_adj_grad``."""
    spec = dict(kind=str(g["kind"]), num_nodes=int(g["num_nodes"]), X=g["X"], symmetric=bool(g["symmetric"]),
                theta=[g["W0"], g["b0"], g["W1"], g["b1"]])
    if "norm" in g.files:
        if bool(g["res"]):
            spec["theta"] += [g["Wr0"], g["br0"]]
        norm = str(g["norm"])
        if norm in ("layer", "batch"):
            spec["norm"] = dict(kind=norm, eps=float(g["norm_eps"]), weight=g["norm_w0"], bias=g["norm_b0"])
            if norm == "batch":
                spec["norm"].update(mean=g["norm_rm0"], var=g["norm_rv0"])
    return spec


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def _forward(kind, A, X, theta, symmetric, norm):
    N = A.shape[0]
    eye = torch.eye(N, dtype=torch.float64)
    if symmetric:
        A = (A + A.T) / 2
    A = A + ((A > 0.5).to(A.dtype) - A).detach()
    W0, b0, W1, b1 = theta[:4]
    if kind == "gcn":
        A = A * (1 - eye) + eye
        d = A.sum(1).pow(-0.5)
        P = (A * d[None, :]).T * d[None, :]
        s = P @ (X @ W0.T + b0)
        if len(theta) == 6:
            s = s + X @ theta[4].T + theta[5]
        if norm is not None:
            if norm["kind"] == "layer":
                mu = s.mean(1, keepdim=True)
                var = ((s - mu) ** 2).mean(1, keepdim=True)
            else:
                mu, var = _t(norm["mean"]), _t(norm["var"])
            s = (s - mu) / torch.sqrt(var + norm["eps"]) * _t(norm["weight"]) + _t(norm["bias"])
        h = torch.relu(s)
        return P @ (h @ W1.T + b1)
    assert len(theta) == 4 and norm is None, "GraphSAGE: plain models"
    rs = A.sum(1)
    P = A / torch.where(rs == 0, torch.ones_like(rs), rs)[:, None]
    h = torch.relu(torch.cat([X, P @ X], 1) @ W0.T + b0)
    return torch.cat([h, P @ h], 1) @ W1.T + b1


def neg_marglik_adj_grad(adj_rows, adj_cols, idx, y, prior, logdet, *, kind, num_nodes, X, theta, symmetric=False, norm=None):
    """(neg marglik, d neg / d adjacency [N, N], H [P, P]); ``prior``: a scalar or one precision per parameter [P];
    ``logdet``: "diag" or "full"."""
    N = int(num_nodes)
    A = torch.zeros(N, N, dtype=torch.float64)
    A[torch.as_tensor(np.asarray(adj_rows)), torch.as_tensor(np.asarray(adj_cols))] = 1.0
    A.requires_grad_(True)
    theta = [_t(p).clone().requires_grad_(True) for p in theta]
    idx, y = torch.as_tensor(np.asarray(idx)), torch.as_tensor(np.asarray(y))
    f = _forward(kind, A, _t(X), theta, symmetric, norm)[idx]
    M, C = f.shape
    rows = []
    for m in range(M):
        for c in range(C):
            gs = torch.autograd.grad(f[m, c], theta, create_graph=True)
            rows.append(torch.cat([gq.reshape(-1) for gq in gs]))
    J = torch.stack(rows).reshape(M, C, -1)
    p = torch.softmax(f, 1)
    Lam = torch.diag_embed(p) - p[:, :, None] * p[:, None, :]
    H = torch.einsum("mcp,mck,mkq->pq", J, Lam, J)
    P = H.shape[0]
    delta = _t(prior) * torch.ones(P, dtype=torch.float64)
    flat = torch.cat([q.reshape(-1) for q in theta])
    ce = torch.nn.functional.cross_entropy(f, y, reduction="sum")
    ld = torch.log(torch.diagonal(H) + delta).sum() if logdet == "diag" else torch.logdet(H + torch.diag(delta))
    assert logdet in ("diag", "full")
    neg = ce + 0.5 * (ld - torch.log(delta).sum()) + 0.5 * (delta * flat ** 2).sum()
    (gA,) = torch.autograd.grad(neg, A)
    return float(neg.detach()), gA.numpy(), H.detach().numpy()
