"""The matrix-free entries of ``GraphEngine``: products with the Jacobian that never write it where the model has a closed
form.  Behind them: csrc/gpkernel.hip (``gp_kernel``, ``gp_jvp``), ggnmat.hip (``jvp_block``, ``block_gram``,
``ggn_matmat_``), hessmat.hip (``hessian_resid_matmat_``), predictive.hip (``glm_variance*``), glmcov.hip (``glm_covariance``)
and sampled.hip (``sampled_forward``)."""
from __future__ import annotations

import torch

from .. import _lib
from .._lib import HESSIAN_RESID_MATMAT
from ._marshal import _dev_ptr, _opt_ptr, _ptrs

_f32 = torch.float32


class MatrixFreeEntries:
    @property
    def sampled_forward_in_scope(self) -> bool:
        """Whether ``sampled_forward`` covers the bound model: plain GCN / GraphSAGE (no res / norm) with 1 or 2 layers."""
        return self._bound is not None and not self.has_extras and self.num_layers <= 2

    def sampled_forward(self, idx: torch.Tensor, theta: torch.Tensor, softmax: bool = False) -> torch.Tensor:
        """[S, M, C]: the logits (``softmax``: their softmax) the model would give at ``idx`` under each of the S parameter
        vectors ``theta`` [S, n_params] (Laplace parameter order), in one pass (``lgnn_sampled_forward``, csrc/sampled.hip).
        The bound parameters are not written and the cached forward stays valid.  Models with res / norm or more than two
        layers are refused by the library."""
        idx, ip, M = self._batch(idx)
        theta = theta.detach().to(self.device, _f32).contiguous()
        if theta.dim() != 2 or theta.shape[1] != self.n_params:
            raise ValueError(f"theta must be [S, {self.n_params}], got {tuple(theta.shape)}")
        S = theta.shape[0]
        out = self._new(S, M, self.dims[-1])
        self._call("lgnn_sampled_forward", ip, M, theta.data_ptr(), S, _lib.SAMPLED_SOFTMAX if softmax else 0, out.data_ptr())
        return out

    # -- functional Laplace (csrc/gpkernel.hip) --------------------------------------------------------------------
    def _batch_pair(self, idx_a, idx_b):
        """The opening of a call on two index lists; ``idx_b`` None or ``idx_a`` itself: the same tensor on both sides."""
        self._sync_versions()
        same = idx_b is None or idx_b is idx_a
        idx_a = idx_a.contiguous()
        idx_b = idx_a if same else idx_b.contiguous()
        return idx_a, idx_b, idx_a.shape[0], idx_b.shape[0]

    def gp_kernel(self, idx_a: torch.Tensor, idx_b: torch.Tensor, independent: bool = False, matched: bool = False,
                  from_jacobians: bool = False) -> torch.Tensor:
        """``J(idx_a) J(idx_b)^T`` without the Jacobians where the model has a closed form (``lgnn_gp_kernel``): [Ma C, Mb C];
        ``independent``: [C, Ma, Mb]; ``matched`` (Ma == Mb): [Ma, C, C], with ``independent`` [Ma, C].  Passing the same
        tensor twice gives an exactly symmetric result.  ``from_jacobians`` forces the route over ``lgnn_jacobians`` rows."""
        idx_a, idx_b, Ma, Mb = self._batch_pair(idx_a, idx_b)
        C = self.dims[-1]
        flags = ((_lib.GP_INDEPENDENT if independent else 0) | (_lib.GP_MATCHED if matched else 0)
                 | (_lib.GP_FROM_JACOBIANS if from_jacobians else 0))
        if matched:
            if Ma != Mb:
                raise ValueError(f"matched=True needs as many samples on both sides, got {Ma} and {Mb}")
            shape, ldk = ((Ma, C) if independent else (Ma, C, C)), C
        elif independent:
            shape, ldk = (C, Ma, Mb), Mb
        else:
            shape, ldk = (Ma * C, Mb * C), Mb * C
        K = self._new(shape)
        self._call("lgnn_gp_kernel", _dev_ptr(idx_a, torch.int64, "idx_a"), Ma, _dev_ptr(idx_b, torch.int64, "idx_b"), Mb,
                   flags, K.data_ptr(), ldk)
        return K

    def gp_jvp(self, idx: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
        """``out[m, c] = sum_p J[m, c, p] v[p]`` for ``v`` [n_params] (``lgnn_gp_jvp``); no Jacobian is written where the
        model has a closed form."""
        idx, ip, M = self._batch(idx)
        v = v.detach().to(self.device, _f32).contiguous()
        if v.dim() != 1 or v.shape[0] != self.n_params:
            raise ValueError(f"v must be [{self.n_params}], got {tuple(v.shape)}")
        out = self._new(M, self.dims[-1])
        self._call("lgnn_gp_jvp", ip, M, v.data_ptr(), out.data_ptr())
        return out

    # -- low-rank Laplace (csrc/ggnmat.hip) -----------------------------------------------------------------------
    def _directions(self, V: torch.Tensor) -> torch.Tensor:
        """A block of parameter directions: fp32 [k, n_params] on the device, one contiguous row per direction."""
        V = V.detach().to(self.device, _f32).contiguous()
        if V.dim() != 2 or V.shape[0] == 0 or V.shape[1] != self.n_params:
            raise ValueError(f"V must be [k, {self.n_params}] with k >= 1, got {tuple(V.shape)}")
        return V

    def jvp_block(self, idx: torch.Tensor, V: torch.Tensor) -> torch.Tensor:
        """``out[m, c, i] = <J[m, c, :], V[i, :]>`` for ``V`` [k, n_params] (``lgnn_jvp_block``): [M, C, k]."""
        idx, ip, M = self._batch(idx)
        V = self._directions(V)
        out = self._new(M, self.dims[-1], V.shape[0])
        self._call("lgnn_jvp_block", ip, M, V.data_ptr(), V.shape[0], out.data_ptr())
        return out

    def block_gram(self, A: torch.Tensor, B: torch.Tensor | None = None) -> torch.Tensor:
        """``A B^T`` [ka, kb] of two blocks of directions [k, P] on the library's NT GEMM (``lgnn_block_gram``): fixed summation
        order, exactly symmetric for ``B is None`` (= A)."""
        A = A.contiguous()
        B = A if B is None else B.contiguous()
        if A.dim() != 2 or B.dim() != 2 or A.shape[1] != B.shape[1]:
            raise ValueError(f"blocks must be [k, P] with the same P, got {tuple(A.shape)} and {tuple(B.shape)}")
        out = self._new(A.shape[0], B.shape[0])
        self._call("lgnn_block_gram", _dev_ptr(A, _f32, "A"), A.shape[0], _dev_ptr(B, _f32, "B"), B.shape[0], A.shape[1],
                   out.data_ptr())
        return out

    def ggn_matmat_(self, G: torch.Tensor, loss_buf: torch.Tensor, idx, y, V: torch.Tensor, from_jacobians: bool = False):
        """``G[i, :] += sum_n J_n^T Lambda_n J_n V[i, :]`` for ``V`` [k, n_params], ``loss_buf += `` raw loss sum
        (``lgnn_ggn_matmat``); the P x P matrix is never formed.  ``from_jacobians``: the library's flag of that name."""
        idx, ip, M = self._batch(idx)
        V = self._directions(V)
        if tuple(G.shape) != tuple(V.shape) or not G.is_contiguous():
            raise ValueError(f"G must be contiguous [{V.shape[0]}, {V.shape[1]}], got {tuple(G.shape)}")
        y, yp = self._labels(y, M)
        self._call("lgnn_ggn_matmat", ip, yp, M, V.data_ptr(), V.shape[0], _lib.GGN_FROM_JACOBIANS if from_jacobians else 0,
                   _dev_ptr(G, _f32, "G"), loss_buf.data_ptr())

    def hessian_resid_matmat_(self, G: torch.Tensor, idx, y, V: torch.Tensor):
        """``G[i, :] += R V[i, :]`` with ``R = sum_n sum_c r_nc grad^2 f_nc`` (r = softmax(f) - onehot(y); regression f - y): what
        the exact Hessian of the loss adds to the GGN (csrc/hessmat.hip).  Plain 1- and 2-layer models; the library refuses
        the others.  It opens no batch of its own: it runs right after ``ggn_matmat_`` on the same batch, which has
        synchronised the parameter versions, and marshals ``idx`` / ``y`` itself."""
        V = self._directions(V)
        if tuple(G.shape) != tuple(V.shape) or not G.is_contiguous():
            raise ValueError(f"G must be contiguous [{V.shape[0]}, {V.shape[1]}], got {tuple(G.shape)}")
        idx = idx.contiguous()
        y, yp = self._labels(y, idx.shape[0])
        self._call(HESSIAN_RESID_MATMAT, _dev_ptr(idx, torch.int64, "idx"), yp, idx.shape[0], V.data_ptr(), V.shape[0],
                   _dev_ptr(G, _f32, "G"))

    # -- matrix-free GLM predictive (csrc/predictive.hip) ------------------------------------------------------------
    def glm_variance(self, idx: torch.Tensor, S0, S1, kappa, QA0=None, QB0=None, QA1=None, QB1sq=None, out_map=None):
        """Matrix-free GLM predictive of a 2-layer GCN / GraphSAGE: (f_mu [M, C], diag(J P^-1 J^T) [M, C]) from the closed-form
        Jacobian (see include/laplace_gnn_hip.h lgnn_glm_variance for the operand conventions).  ``out_map`` = E [Cm, C]:
        the variances of the linear map E f instead, [M, Cm]; S1 / QB1sq / kappa are then the caller's mapped operands
        (lgnn_glm_variance_mapped)."""
        return self._glm_variance(idx, (QA0, QB0, S0, QA1, S1, QB1sq, kappa), out_map, ext=False)

    def glm_variance_ext(self, idx: torch.Tensor, S0, S1, kappa, QA0=None, QB0=None, QA1=None, QB1sq=None, Sr=None, QAr=None,
                         QBr=None, out_map=None):
        """``glm_variance`` for 2-layer models built with res / norm (and, through the same route, plain ones): one entry
        with or without ``out_map`` (lgnn_glm_variance_ext).  ``Sr`` [H, F + 1] (and ``QAr`` / ``QBr`` under a Kronecker
        posterior) are the operands of the res.0 block; None for a model without res."""
        return self._glm_variance(idx, (QA0, QB0, S0, QA1, S1, QB1sq, kappa, QAr, QBr, Sr), out_map, ext=True)

    def _glm_variance(self, idx, operands, out_map, ext):
        """The one call behind ``glm_variance`` (lgnn_glm_variance, with ``out_map`` lgnn_glm_variance_mapped) and
        ``glm_variance_ext`` (lgnn_glm_variance_ext, which takes a null head for the model's own classes)."""
        idx, ip, M = self._batch(idx)
        C = self.dims[-1]
        head = []
        if out_map is not None:
            if out_map.ndim != 2 or out_map.shape[1] != C:
                raise ValueError(f"out_map must be [rows, {C}]")
            W1m = (out_map.to(device=self.device, dtype=_f32) @ self._bound[1][-1].detach().to(_f32)).contiguous()
            head = [W1m.data_ptr(), int(out_map.shape[0])]
        elif ext:
            head = [None, 0]
        f_mu, f_var = self._new(M, C), self._new(M, C if out_map is None else out_map.shape[0])
        keep = [t.contiguous().to(_f32) if t is not None else None for t in operands]  # (locals: the borrow rule of ``_call``)
        ptr = [_opt_ptr(t, _f32, "posterior operand") for t in keep]
        self._call("lgnn_glm_variance_ext" if ext else ("lgnn_glm_variance" if out_map is None else "lgnn_glm_variance_mapped"),
                   ip, M, *head, *ptr, f_mu.data_ptr(), f_var.data_ptr())
        return f_mu, f_var

    # -- joint GLM predictive (csrc/glmcov.hip) --------------------------------------------------------------------
    def glm_covariance(self, idx_a: torch.Tensor, idx_b: torch.Tensor | None = None, *, QA, QB, S,
                       from_jacobians: bool = False) -> torch.Tensor:
        """``J(idx_a) P^-1 J(idx_b)^T`` [Ma C, Mb C] for a posterior that is block diagonal over the Linear layers
        (``lgnn_glm_covariance``; see include/laplace_gnn_hip.h for the operands).  ``QA`` / ``QB`` / ``S``: one entry per block
        in ``block_dims`` order -- ``S[l]`` [out_l, in_l + 1] inverse precisions (last column: the bias), ``QA[l]`` [in_l, in_l]
        and ``QB[l]`` [out_l, out_l] eigenvectors in columns, or None / None for a diagonal block.  ``idx_b=None``: the same
        tensor on both sides, and an exactly symmetric result.  No Jacobian is written where the model has a closed form;
        ``from_jacobians`` forces the route over ``lgnn_jacobians`` rows."""
        idx_a, idx_b, Ma, Mb = self._batch_pair(idx_a, idx_b)
        bd, nb = self.block_dims, len(self.block_dims)
        if not (len(QA) == len(QB) == len(S) == nb):
            raise ValueError(f"QA, QB and S must have one entry per Linear layer ({nb}), got {len(QA)}, {len(QB)}, {len(S)}")

        def operands(ts, what, shape_of):
            ts = [None if t is None else t.detach().to(self.device, _f32).contiguous() for t in ts]
            for l, t in enumerate(ts):
                if t is not None and tuple(t.shape) != shape_of(l):
                    raise ValueError(f"{what}[{l}] must be {shape_of(l)}, got {tuple(t.shape)}")
            return ts, _ptrs(ts, _f32, what)

        QA, qa = operands(QA, "QA", lambda l: (bd[l][0], bd[l][0]))  # (the copies stay in these locals: the borrow rule
        QB, qb = operands(QB, "QB", lambda l: (bd[l][1], bd[l][1]))  # of ``_call``)
        S, sv = operands(S, "S", lambda l: (bd[l][1], bd[l][0] + 1))
        C = self.dims[-1]
        K = self._new(Ma * C, Mb * C)
        self._call("lgnn_glm_covariance", _dev_ptr(idx_a, torch.int64, "idx_a"), Ma, _dev_ptr(idx_b, torch.int64, "idx_b"), Mb,
                   nb, qa, qb, sv, _lib.COV_FROM_JACOBIANS if from_jacobians else 0, K.data_ptr(), Mb * C)
        return K

    def glm_covariance_chunk_pairs(self) -> int:
        """How many chunk pairs of the two index lists the last ``glm_covariance`` computed (chunks follow the workspace limit)."""
        return int(self.lib.lgnn_glm_covariance_chunk_pairs(self._h))
