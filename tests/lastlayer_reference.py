"""TEST-ONLY: the last-layer Kronecker and diagonal GGN restated in fp64 from ``O.lastlayer_features`` and the seed
definition of ``O.kfac_seeds``, and a CPU stand-in backend that serves them behind the ``CurvatureInterface`` signatures
(``last_layer=True``) so that ``KronLLLaplace`` / ``DiagLLLaplace`` run without a GPU.

Per batch sample n: ``f_n = W phi_n + s_n b``;  ``A += Phi^T Phi / N``, ``B += sum_n V_n V_n^T``, ``B_b += sum_n s_n^2 V_n V_n^T``,
``diag[c D + d] += sum_n Lambda_n[c, c] phi_n[d]^2``, ``diag[C D + c] += sum_n Lambda_n[c, c] s_n^2``, ``loss += CE_sum``."""
import numpy as np
import torch

import gnn_laplace_oracle as O
from laplace_gnn_amd.matrix import Kron
from oracle_backend import OracleBackend

F64 = np.float64


def softmax64(f):
    f = np.asarray(f, F64)
    e = np.exp(f - f.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def seeds64(f, fork_exact=True):
    """``V[n, k, c]`` of ``O.kfac_seeds`` in fp64 (oracle/gnn_laplace_oracle.py:424-448)."""
    f = np.asarray(f, F64)
    p = softmax64(f)
    sp = np.sqrt(p)
    eye = np.eye(f.shape[1])
    if not fork_exact:
        return sp[:, None, :] * (eye[None] - p[:, :, None])
    fm = f - (p * f).sum(axis=1, keepdims=True)
    return sp[:, None, :] * (eye[None] - (p * (1 + fm))[:, :, None] + 0.5 * (eye[None] - p[:, :, None]) * fm[:, None, :])


def ce_sum64(f, y):
    f = np.asarray(f, F64)
    mx = f.max(axis=1)
    return float((np.log(np.exp(f - mx[:, None]).sum(axis=1)) + mx - f[np.arange(len(y)), np.asarray(y)]).sum())


def kron_from_features(phi, s, f, y, n_train, fork_exact=True):
    """(loss, A [D, D], B [C, C], B_b [C, C]) of one batch, fp64."""
    phi, s = np.asarray(phi, F64), np.asarray(s, F64)
    V = seeds64(f, fork_exact)
    VVt = np.einsum("nkc,njc->nkj", V, V)
    return ce_sum64(f, y), phi.T @ phi / n_train, VVt.sum(axis=0), np.einsum("n,nkj->kj", s * s, VVt)


def diag_from_features(phi, s, f, y):
    """(loss, diag [C D + C]) of one batch, fp64: weight entries row major, then the bias entries."""
    phi, s = np.asarray(phi, F64), np.asarray(s, F64)
    p = softmax64(f)
    lam = p * (1 - p)
    return ce_sum64(f, y), np.concatenate([(lam.T @ (phi * phi)).reshape(-1), lam.T @ (s * s)])


def jacobians_from_features(phi, s, C):
    """``J_n = [I_C (x) phi_n^T | s_n I_C]`` [M, C, C D + C] (laplace/curvature/curvature.py:152-165)."""
    phi, s = np.asarray(phi, F64), np.asarray(s, F64)
    M, D = phi.shape
    eye = np.eye(C)
    return np.concatenate([np.einsum("kp,ij->kijp", phi, eye).reshape(M, C, C * D), s[:, None, None] * eye[None]], axis=2)


def batches(n, batch_size):
    return [slice(s0, min(n, s0 + batch_size)) for s0 in range(0, n, batch_size)]


def fit_from_model(om, idx, y, batch_size, fork_exact=True):
    """Sums over the loader's batches (N = len(idx)): dict(loss, A, B, Bb, diag), fp64."""
    idx, y = np.asarray(idx, np.int64), np.asarray(y, np.int64)
    out = None
    for b in batches(len(idx), batch_size):
        phi, s, f = O.lastlayer_features(om, idx[b])
        loss, A, B, Bb = kron_from_features(phi, s, f, y[b], len(idx), fork_exact)
        _, dg = diag_from_features(phi, s, f, y[b])
        cur = dict(loss=loss, A=A, B=B, Bb=Bb, diag=dg)
        out = cur if out is None else {k: out[k] + cur[k] for k in cur}
    return out


def rel(a, b):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


class LastLayerOracleBackend(OracleBackend):
    """``OracleBackend`` that also serves ``kron`` / ``diag`` / Jacobians / features of the head for ``last_layer=True``."""

    def __init__(self, model, likelihood, last_layer=False, fork_exact_seed=True, **kw):
        super().__init__(model, likelihood, last_layer=last_layer, **kw)
        self.fork_exact_seed = fork_exact_seed

    def _features(self, x):
        return O.lastlayer_features(self.model.oracle_model(), x.numpy())

    def lastlayer_features(self, x):
        phi, s, f = self._features(x)
        return (torch.from_numpy(np.ascontiguousarray(phi, np.float32)), torch.from_numpy(np.ascontiguousarray(s, np.float32)),
                torch.from_numpy(np.ascontiguousarray(f, np.float32)))

    def kron(self, x, y, N, **kw):
        if not self.last_layer:
            return super().kron(x, y, N, **kw)
        self.calls.append(("kron", tuple(x.tolist())))
        phi, s, f = self._features(x)
        loss, A, B, Bb = kron_from_features(phi, s, f, y.numpy(), N, self.fork_exact_seed)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))  # noqa: E731
        return torch.tensor(float(loss)), Kron([[t(B), t(A)], [t(Bb)]])

    def diag(self, x, y, **kw):
        if not self.last_layer:
            return super().diag(x, y, **kw)
        self.calls.append(("diag", tuple(x.tolist())))
        phi, s, f = self._features(x)
        loss, dg = diag_from_features(phi, s, f, y.numpy())
        return torch.tensor(float(loss)), torch.from_numpy(dg.astype(np.float32))

    def jacobians(self, x, enable_backprop=False):
        if not self.last_layer:
            return super().jacobians(x, enable_backprop)
        phi, s, f = self._features(x)
        return (torch.from_numpy(jacobians_from_features(phi, s, f.shape[1]).astype(np.float32)),
                torch.from_numpy(np.ascontiguousarray(f, np.float32)))

    last_layer_jacobians = jacobians
