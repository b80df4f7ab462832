"""Top-K eigenpairs of a symmetric positive semi-definite operator that is only available as a block product: block
subspace iteration with Rayleigh-Ritz (what ``HipGGN.eig_lowrank`` runs on ``lgnn_ggn_matmat``).

The reference's ``LowRankLaplace`` takes its pairs from power iteration with deflation, one Hessian-vector product at a time
(laplace/curvature/asdfghjkl.py:212-236, ``max_iters = 10 * low_rank``).  Here one sweep multiplies a whole block:

* block size ``b = K + max(8, K // 4)``, capped at P; the start block is Gaussian from a generator of its own (seed 0);
* a block is ``[b, P]``, one direction per contiguous row (the layout the device product takes);
* rows are orthonormalised by CholeskyQR2 on the block's Gram matrix (``gram``: the library's fixed-order NT GEMM on the
  device), the ``b x b`` factorisations in fp64.  A Gram matrix whose Cholesky factorisation fails (a block that lost rank)
  falls back to its eigen-decomposition and drops the directions below ``1e-12`` of the largest;
* Ritz step: ``T = Q (H Q)^T`` symmetrised, ``eigh`` in fp64, the block and its product rotated to the Ritz vectors;
* stop when the K leading pairs satisfy ``||H v_i - l_i v_i|| <= tol * l_1``, or after ``max_iters`` (default ``10 K``) sweeps;
* the next block is the rotated product with its rows normalised (after the rotation they are close to orthogonal with norms
  ``l_i``, so the Gram matrix CholeskyQR2 sees is well conditioned whatever the spectrum's range); a row whose norm is below
  ``1e-7 l_1`` -- a direction of the operator's numerical null space -- keeps its Ritz vector instead, so the block never
  loses rank when the operator's rank is below b;
* pairs with ``l > eps`` (the reference's EPS = 1e-6) are returned.

Everything of size ``[b, P]`` stays on the device of the start block; the ``b x b`` algebra is torch in fp64.  The result
is a pure function of (product, P, K, tol, max_iters, seed): no global random state is read or written."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable

import torch

EPS = 1e-6  # laplace/curvature/asdfghjkl.py:24
# Default stopping tolerance: 8 x the fp32 floor of the residual measured WITHOUT the solver (exact fp64 eigenvectors rounded to
# fp32, pushed through the fp32 Jacobians): 2.40e-7 at P = 195 and 7.98e-8 at P = 2 887 (tests/test_gpu_lowrank.py).
# The 8 is headroom for other shapes' reduction lengths.
DEFAULT_TOL = 8 * 2.40e-7


def block_size(K: int, P: int) -> int:
    """Directions per sweep: K plus ``max(8, K // 4)`` of oversampling, at most P."""
    if K < 1:
        raise ValueError(f"low_rank must be >= 1, got {K}")
    return int(min(P, K + max(8, K // 4)))


def default_max_iters(K: int) -> int:
    """The reference's iteration budget (``max_iters = low_rank * 10``), counted in block products."""
    return 10 * int(K)


def start_block(b: int, P: int, seed: int, device, dtype=torch.float32) -> torch.Tensor:
    """Seeded Gaussian block [b, P]; drawn on the host from a generator of its own (the same bits for every device)."""
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    return torch.randn(b, P, generator=g, dtype=dtype).to(device)


def _gram_torch(A: torch.Tensor, B: torch.Tensor | None = None) -> torch.Tensor:
    return A @ (A if B is None else B).T


def cholqr2(Q: torch.Tensor, gram: Callable = _gram_torch) -> torch.Tensor:
    """Rows of ``Q`` [b, P] orthonormalised: twice ``Q <- L^-1 Q`` with ``L L^T = Q Q^T`` (fp64 factor of the fp32 Gram).  A
    failed factorisation takes the Gram's eigenvectors instead and drops the directions below 1e-12 of the largest."""
    for _ in range(2):
        G = gram(Q).double()
        G = 0.5 * (G + G.T)
        L, info = torch.linalg.cholesky_ex(G)
        if int(info) == 0:
            Linv = torch.linalg.solve_triangular(L, torch.eye(L.shape[0], dtype=L.dtype, device=L.device), upper=False)
            Q = Linv.to(Q.dtype) @ Q
        else:
            s, S = torch.linalg.eigh(G)
            keep = s > 1e-12 * s.max().clamp_min(1e-300)
            Q = ((S[:, keep] / s[keep].sqrt()).T).to(Q.dtype) @ Q
    return Q


@dataclass
class LowRankResult:
    eigenvectors: torch.Tensor  # [P, K'] orthonormal columns
    eigenvalues: torch.Tensor   # [K'] descending, all > eps
    n_sweeps: int               # block products spent
    residuals: torch.Tensor     # [K'] ||H v_i - l_i v_i|| of the returned pairs, as the solver measured them
    converged: bool             # the stopping rule was met (False: max_iters sweeps were spent)
    lambda_max: float


def ritz(Q: torch.Tensor, Y: torch.Tensor, gram: Callable = _gram_torch):
    """Rayleigh-Ritz on the rows of Q with Y = H Q: (theta [b] descending, X = W^T Q, HX = W^T Y)."""
    T = gram(Q, Y).double()
    T = 0.5 * (T + T.T)
    theta, W = torch.linalg.eigh(T)
    theta, W = theta.flip(0), W.flip(1)
    Wt = W.T.to(Q.dtype).contiguous()
    return theta, Wt @ Q, Wt @ Y


def stop_rule(theta: torch.Tensor, res: torch.Tensor, K: int, tol: float) -> bool:
    """The K leading pairs' residuals against ``tol * l_1``."""
    lam1 = float(theta[0].clamp_min(0))
    return bool((res[:K] <= tol * lam1).all())


def mask_pairs(theta: torch.Tensor, K: int, eps: float = EPS) -> torch.Tensor:
    """Indices of the pairs that are returned: among the K leading ones, those with ``l > eps``."""
    return (theta[:K] > eps).nonzero().squeeze(1)


def subspace_eig(matmat: Callable[[torch.Tensor], torch.Tensor], P: int, K: int, device, tol: float | None = None,
                 max_iters: int | None = None, seed: int = 0, gram: Callable = _gram_torch, eps: float = EPS,
                 dtype=torch.float32) -> LowRankResult:
    """``matmat(Q [b, P]) -> H Q [b, P]`` (rows are directions).  See the module docstring."""
    tol = DEFAULT_TOL if tol is None else float(tol)
    max_iters = default_max_iters(K) if max_iters is None else int(max_iters)
    if max_iters < 1:
        raise ValueError("max_iters must be >= 1")
    b = block_size(K, P)
    K = min(K, b)
    Q = cholqr2(start_block(b, P, seed, device, dtype), gram)
    sweeps, converged = 0, False
    while True:
        Y = matmat(Q)
        sweeps += 1
        theta, X, HX = ritz(Q, Y, gram)
        th = theta.to(X.dtype).clamp_min(0).unsqueeze(1)
        res = torch.linalg.vector_norm(HX - th * X, dim=1)
        converged = stop_rule(theta, res.double(), K, tol)
        if converged or sweeps >= max_iters:
            break
        norms = torch.linalg.vector_norm(HX, dim=1, keepdim=True)
        live = norms > 1e-7 * float(theta[0].clamp_min(0))
        Q = cholqr2(torch.where(live, HX / norms.clamp_min(1e-30), X), gram)
    sel = mask_pairs(theta, K, eps)
    return LowRankResult(eigenvectors=X[sel].T.contiguous(), eigenvalues=theta[sel].to(X.dtype), n_sweeps=sweeps,
                         residuals=res[sel], converged=converged, lambda_max=float(theta[0]))
