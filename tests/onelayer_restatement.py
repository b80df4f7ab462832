"""fp64 autograd restatement of the structure-learning objective (gnn/marglik_training.py:197-216) of a ONE-layer STE-GCN
(the Banana block of gnn/configs/original/stegcn_config.yaml: ``num_layers: 1``): the negative log marginal likelihood of a
Laplace posterior as a differentiable function of the dense adjacency parameter, and its gradient.  Plain torch on the CPU:
nothing from the oracle, nothing from the library.  Pinned to the reference's own ``model.adj.grad`` by
tests/test_onelayer_restatement.py (tests/golden/onelayer/one1_*.npz).

    symmetric models          A <- (A + A^T) / 2
    straight-through          A <- A + ((A > 0.5) - A).detach()                       (identity in backward)
    GCN                       A <- A (1 - I) + I;  P = (A d)^T d, d = diag(rowsum^-1/2);  out = P (X W^T + 1 b^T)
    f = out[idx] = W phi + b rho,  psi = [phi | rho] = [P X | rowsum(P)][idx]
    J_n[c, (c', j)] = delta_cc' psi_n[j]     (the model is linear in theta = (W row major, b); checked against autograd
                                               in the test);   H = sum_n J_n^T Lambda_n J_n
    neg = CE_sum + 1/2 (logdet - sum_p log delta_p) + 1/2 sum_p delta_p theta_p^2
    logdet = sum log(diag H + delta)  ("diag")   or   logdet(H + diag(delta))  ("full")   or   the Kronecker posterior's
    sum_ij log(lB_i lA_j + delta) + sum_i log(lB_i + delta)  ("kron"): A = n_batches X^T X / n_train over ALL N rows,
    B = sum_batches sum_c g_c^T g_c, g_c = P^T scatter(V[:, :, c]), V[n, :, c] = d/df_n sum_k f_nk S_kc(f_n) with
    S_kc = sqrt(p_c) (delta_kc - p_k) NOT detached (the fork's seeds, curvlinops/kfac.py:637-661)."""
import numpy as np
import torch


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def propagation(A, symmetric):
    N = A.shape[0]
    eye = torch.eye(N, dtype=torch.float64)
    if symmetric:
        A = (A + A.T) / 2
    A = A + ((A > 0.5).to(A.dtype) - A).detach()
    A = A * (1 - eye) + eye
    d = A.sum(1).pow(-0.5)
    return (A * d[None, :]).T * d[None, :]


def forward(P, X, W, b):
    return P @ (X @ W.T + b)


def closed_form_jacobians(P, X, idx, C):
    """J [M, C, C (F + 1)]: weight entries (c, j) at c F + j, bias entries at C F + c."""
    F = X.shape[1]
    phi, rho = (P @ X)[idx], P.sum(1)[idx]
    M = phi.shape[0]
    J = torch.zeros(M, C, C * F + C, dtype=torch.float64)
    for c in range(C):
        J[:, c, c * F:(c + 1) * F] = phi
        J[:, c, C * F + c] = rho
    return J


def _kron_logdet(P, X, f_all, batches, n_train, delta):
    N, C = f_all.shape
    B = torch.zeros(C, C, dtype=torch.float64)
    for idx in batches:
        f = f_all[idx]
        p = torch.softmax(f, 1)
        S = p.sqrt()[:, None, :] * (torch.eye(C, dtype=torch.float64)[None] - p[:, :, None])  # [M, k, c]
        s = (f[:, :, None] * S).sum(1)  # [M, c]
        for c in range(C):
            (V,) = torch.autograd.grad(s[:, c].sum(), f, create_graph=True)  # [M, k]
            G = torch.zeros(N, C, dtype=torch.float64).index_add(0, idx, V)
            g = P.T @ G
            B = B + g.T @ g
    A = len(batches) * (X.T @ X) / n_train
    lB, lA = torch.linalg.eigvalsh(B), torch.linalg.eigvalsh(A)
    ld = torch.log(lB[:, None] * lA[None, :] + delta).sum() + torch.log(lB + delta).sum()
    return ld, B, A


def neg_marglik_adj_grad(adj_rows, adj_cols, idx, y, prior, logdet, *, num_nodes, X, W, b, symmetric=False, batch_size=None):
    """(neg marglik, d neg / d adjacency [N, N], H): ``H`` is the full GGN [P, P] ("diag" / "full") or the pair (B, A) of the
    Kronecker factors ("kron", which needs the loader's ``batch_size``); ``prior``: a scalar precision."""
    assert logdet in ("diag", "full", "kron")
    N = int(num_nodes)
    A = torch.zeros(N, N, dtype=torch.float64)
    A[torch.as_tensor(np.asarray(adj_rows)), torch.as_tensor(np.asarray(adj_cols))] = 1.0
    A.requires_grad_(True)
    X, W, b = _t(X), _t(W), _t(b)
    idx, y = torch.as_tensor(np.asarray(idx)), torch.as_tensor(np.asarray(y))
    C = W.shape[0]
    P = propagation(A, symmetric)
    f_all = forward(P, X, W, b)
    f = f_all[idx]
    n_par = W.numel() + b.numel()
    delta = float(prior)
    if logdet == "kron":
        M = idx.shape[0]
        bs = M if batch_size is None else int(batch_size)
        batches = [idx[s:s + bs] for s in range(0, M, bs)]
        ld, Bf, Af = _kron_logdet(P, X, f_all, batches, M, delta)
        H = (Bf.detach().numpy(), Af.detach().numpy())
    else:
        J = closed_form_jacobians(P, X, idx, C)
        p = torch.softmax(f, 1)
        Lam = torch.diag_embed(p) - p[:, :, None] * p[:, None, :]
        Hm = torch.einsum("mcp,mck,mkq->pq", J, Lam, J)
        ld = torch.log(torch.diagonal(Hm) + delta).sum() if logdet == "diag" else \
            torch.logdet(Hm + delta * torch.eye(n_par, dtype=torch.float64))
        H = Hm.detach().numpy()
    flat = torch.cat([W.reshape(-1), b.reshape(-1)])
    ce = torch.nn.functional.cross_entropy(f, y, reduction="sum")
    neg = ce + 0.5 * (ld - n_par * np.log(delta)) + 0.5 * delta * (flat ** 2).sum()
    (gA,) = torch.autograd.grad(neg, A)
    return float(neg.detach()), gA.numpy(), H


def full_from_blocks(P, X, idx, W, b, Gamma):
    """The issue's per-sample formulas with a dense Gamma [P, P] (blocks G_ck linking (W[c, :], b[c]) to (W[k, :], b[k])):
    ``K_n[c, k] = psi^T G_ck psi``, ``pbar_c = K_cc - 2 sum_k K_ck p_k``, ``ebar_n = 2 sum_ck Lambda_ck G_ck psi``.
    Returns (pbar [M, C], ebar [M, F + 1]) -- the unit check that the diagonal case is G_ck = delta_ck diag(Gamma_c)."""
    X, W, b, P, Gamma = _t(X), _t(W), _t(b), _t(P), _t(Gamma)
    idx = torch.as_tensor(np.asarray(idx))
    C, F = W.shape
    psi = torch.cat([(P @ X)[idx], P.sum(1)[idx][:, None]], 1)  # [M, F + 1]
    pos = torch.tensor([[c * F + j for j in range(F)] + [C * F + c] for c in range(C)])  # [C, F + 1]
    G = Gamma[pos[:, None, :, None], pos[None, :, None, :]]  # [C, C, F + 1, F + 1]
    p = torch.softmax(forward(P, X, W, b)[idx], 1)
    Lam = torch.diag_embed(p) - p[:, :, None] * p[:, None, :]
    K = torch.einsum("mi,ckij,mj->mck", psi, G, psi)
    pbar = torch.diagonal(K, dim1=1, dim2=2) - 2 * torch.einsum("mck,mk->mc", K, p)
    ebar = 2 * torch.einsum("mck,ckij,mj->mi", Lam, G, psi)
    return pbar.numpy(), ebar.numpy()


def diag_formulas(P, X, idx, W, b, gamma):
    """The diagonal posterior's per-sample formulas: ``kappa_c = sum_j Gamma_c[j] psi_j^2``, ``pbar_c = (1 - 2 p_c) kappa_c``,
    ``ebar = 2 psi * sum_c Lambda_cc Gamma_c``."""
    X, W, b, P, gamma = _t(X), _t(W), _t(b), _t(P), _t(gamma)
    idx = torch.as_tensor(np.asarray(idx))
    C, F = W.shape
    psi = torch.cat([(P @ X)[idx], P.sum(1)[idx][:, None]], 1)
    Gc = torch.cat([gamma[:C * F].reshape(C, F), gamma[C * F:].reshape(C, 1)], 1)  # [C, F + 1]
    p = torch.softmax(forward(P, X, W, b)[idx], 1)
    kappa = (psi ** 2) @ Gc.T
    pbar = (1 - 2 * p) * kappa
    ebar = 2 * psi * ((p * (1 - p)) @ Gc)
    return pbar.numpy(), ebar.numpy()
