"""The structure-learning entries of ``GraphEngine``: the marginal likelihood's gradient w.r.t. the adjacency, on the stored
entries (plus candidate pairs) or on all N x N pairs, and the LoRA graph.  Behind them: csrc/adjgrad.hip (driver),
adjgrad_gcn.hip, adjgrad_sage.hip, adjgrad_onelayer.hip, adjgrad_ext.hip, adjgrad_diag.hip, fulladj.hip
(``full_adjgrad_batch``, ``full_directions``) and lora.hip (the ``*_dense`` entries, ``lora_*``)."""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib
from .._lib import BAND_BATCH, BAND_FINISH, BAND_PREPARE, BAND_SPARSE
from ._marshal import _dev_ptr, _opt_ptr, _ptrs

_f32 = torch.float32


def _cand_ptrs(cand):
    """cand = (a int32 [K], b int32 [K], accumulator fp32 [K]) in the propagation matrix's coordinates, or None."""
    if cand is None:
        return None, None, 0, None
    a, b, acc = cand
    return _dev_ptr(a, torch.int32, "cand_a"), _dev_ptr(b, torch.int32, "cand_b"), int(a.shape[0]), _dev_ptr(acc, _f32, "grad_cand")


class StructureEntries:
    def _finish(self, name, cand, *args):
        """The close of ``adjgrad_finish`` / ``diag_adjgrad_finish``: the gradient on the stored entries (``export_adj``
        order) and, with candidates, on every listed pair (second return value)."""
        out = torch.zeros(self.nnz, dtype=_f32, device=self.device)
        ca, cb, K, cacc = _cand_ptrs(cand)
        cout = torch.zeros(K, dtype=_f32, device=self.device) if K else None
        self._call(name, *args, out.data_ptr(), ca, cb, K, cacc, None if cout is None else cout.data_ptr())
        return out if cand is None else (out, cout)

    # -- on the stored entries and candidate pairs ("next" row 8(f)-4) -------------------------------------------------
    def adjgrad_batch(self, idx, y, gammas_B, grad_P: torch.Tensor, out_bar: torch.Tensor, fork_exact: bool = True,
                      loss_scale: float = 1.0, cand=None):
        """Add one batch's terms to ``grad_P`` [nnz] (stored entries of the propagation matrix), ``out_bar`` [N, C] and,
        for candidate pairs ``cand = (a, b, acc)``, to ``acc``."""
        idx, y, batch = self._batch_y(idx, y)
        gammas_B = [g.contiguous() for g in gammas_B]
        self._call("lgnn_kfac_adjgrad_batch", *batch, _lib.FLAG_FORK_EXACT_SEED if fork_exact else 0,
                   _ptrs(gammas_B, _f32, "gamma_B"), float(loss_scale), _dev_ptr(grad_P, _f32, "grad_P"),
                   _dev_ptr(out_bar, _f32, "out_bar"), *_cand_ptrs(cand))

    def adjgrad_finish(self, out_bar: torch.Tensor, gammas_A, a_scale: float, grad_P: torch.Tensor, cand=None):
        """Forward-pass terms + normalize_adj / STE backward: gradient w.r.t. the stored entries of the 0/1 adjacency
        (``export_adj`` order); with candidates also ``d / d adj[i, j]`` of every listed pair (second return value)."""
        self._sync_versions()
        gammas_A = [g.contiguous() for g in gammas_A]
        return self._finish("lgnn_adjgrad_finish", cand, _dev_ptr(out_bar, _f32, "out_bar"), _ptrs(gammas_A, _f32, "gamma_A"),
                            float(a_scale), _dev_ptr(grad_P, _f32, "grad_P"))

    def diag_adjgrad_batch(self, idx, y, gamma: torch.Tensor, grad_P: torch.Tensor, out_bar: torch.Tensor, h1_bar: torch.Tensor,
                           e_bar: torch.Tensor, loss_scale: float = 1.0, cand=None):
        """Diagonal posterior (1- and 2-layer GCN): add one batch's terms to ``grad_P`` [nnz], ``out_bar`` [N, C], ``h1_bar`` [N, H]
        (None for a 1-layer model), ``e_bar`` [N, F + 1] and the candidates' accumulator; ``gamma`` [n_params] = d(-marglik)/dH
        (lgnn_diag_adjgrad_batch)."""
        idx, y, batch = self._batch_y(idx, y)
        gamma = gamma.contiguous()
        self._call("lgnn_diag_adjgrad_batch", *batch, _dev_ptr(gamma, _f32, "gamma"), float(loss_scale),
                   _dev_ptr(grad_P, _f32, "grad_P"), _dev_ptr(out_bar, _f32, "out_bar"), _opt_ptr(h1_bar, _f32, "h1_bar"),
                   _dev_ptr(e_bar, _f32, "e_bar"), *_cand_ptrs(cand))

    def diag_adjgrad_finish(self, out_bar: torch.Tensor, h1_bar: torch.Tensor, e_bar: torch.Tensor, grad_P: torch.Tensor,
                            cand=None):
        """The forward-pass terms of ``out_bar`` / ``h1_bar`` / ``e_bar`` + normalize_adj / STE backward (as ``adjgrad_finish``)."""
        self._sync_versions()
        return self._finish("lgnn_diag_adjgrad_finish", cand, _dev_ptr(out_bar, _f32, "out_bar"),
                            _opt_ptr(h1_bar, _f32, "h1_bar"), _dev_ptr(e_bar, _f32, "e_bar"), _dev_ptr(grad_P, _f32, "grad_P"))

    def full_adjgrad_batch(self, idx, y, Gamma: torch.Tensor, grad_P: torch.Tensor, out_bar: torch.Tensor, h1_bar: torch.Tensor,
                           e_bar: torch.Tensor, loss_scale: float = 1.0, cand=None):
        """Full posterior (1-layer GCN; 2-layer GCN, also with res / norm; plain 2-layer GraphSAGE): as ``diag_adjgrad_batch`` with
        the dense symmetric ``Gamma`` [n_params, n_params] = d(-marglik)/dH as weighting (lgnn_full_adjgrad_batch); finished by
        ``diag_adjgrad_finish``."""
        idx, y, batch = self._batch_y(idx, y)
        self._check_gamma(Gamma)
        self._call("lgnn_full_adjgrad_batch", *batch, _dev_ptr(Gamma, _f32, "Gamma"), float(loss_scale),
                   _dev_ptr(grad_P, _f32, "grad_P"), _dev_ptr(out_bar, _f32, "out_bar"), _opt_ptr(h1_bar, _f32, "h1_bar"),
                   _dev_ptr(e_bar, _f32, "e_bar"), *_cand_ptrs(cand))

    def full_directions(self, idx: torch.Tensor, Gamma: torch.Tensor):
        """(K [M, C, C], R [M, C, P]): ``K_m = J_m Gamma J_m^T`` and ``R_m = 2 Lambda_m J_m Gamma`` of the samples ``idx`` for a
        symmetric ``Gamma`` [n_params, n_params], ``Lambda_m`` the softmax Hessian of the model's logits (lgnn_full_directions)."""
        idx, ip, M = self._batch(idx)
        self._check_gamma(Gamma)
        Kn, R = self._new(M, self.dims[-1], self.dims[-1]), self._new(M, self.dims[-1], self.n_params)
        self._call("lgnn_full_directions", ip, M, _dev_ptr(Gamma, _f32, "Gamma"), Kn.data_ptr(), R.data_ptr())
        return Kn, R

    def _check_gamma(self, Gamma: torch.Tensor):
        if tuple(Gamma.shape) != (self.n_params, self.n_params) or not Gamma.is_contiguous():
            raise ValueError(f"Gamma: a contiguous [{self.n_params}, {self.n_params}] matrix, got {tuple(Gamma.shape)}")

    # -- the same gradient on all N x N pairs (LoRASTEGCN: lgnn_*_dense, csrc/lora.hip) ---------------------------------
    def adjgrad_batch_dense(self, idx, y, gammas_B, out_bar: torch.Tensor, grad_dense: torch.Tensor, fork_exact: bool = True,
                            loss_scale: float = 1.0):
        """Add one batch's terms to ``out_bar`` [N, C] and to ``grad_dense`` [N, N] (d/dP on the full grid until the finish)."""
        idx, y, batch = self._batch_y(idx, y)
        gammas_B = [g.contiguous() for g in gammas_B]
        self._call("lgnn_kfac_adjgrad_batch_dense", *batch, _lib.FLAG_FORK_EXACT_SEED if fork_exact else 0,
                   _ptrs(gammas_B, _f32, "gamma_B"), float(loss_scale), _dev_ptr(out_bar, _f32, "out_bar"),
                   _dev_ptr(grad_dense, _f32, "grad_dense"))

    def adjgrad_finish_dense(self, out_bar: torch.Tensor, gammas_A, a_scale: float, grad_dense: torch.Tensor):
        """Forward-pass terms + normalize_adj / STE backward, in place: ``grad_dense[i, j] = d / d adj[i, j]``."""
        self._sync_versions()
        gammas_A = [g.contiguous() for g in gammas_A]
        self._call("lgnn_adjgrad_finish_dense", _dev_ptr(out_bar, _f32, "out_bar"), _ptrs(gammas_A, _f32, "gamma_A"),
                   float(a_scale), _dev_ptr(grad_dense, _f32, "grad_dense"))
        return grad_dense

    def diag_adjgrad_batch_dense(self, idx, y, gamma: torch.Tensor, out_bar: torch.Tensor, h1_bar: torch.Tensor,
                                 e_bar: torch.Tensor, grad_dense: torch.Tensor, loss_scale: float = 1.0):
        """Diagonal posterior: as ``diag_adjgrad_batch`` with the full grid ``grad_dense`` [N, N] in place of the stored entries."""
        idx, y, batch = self._batch_y(idx, y)
        gamma = gamma.contiguous()
        self._call("lgnn_diag_adjgrad_batch_dense", *batch, _dev_ptr(gamma, _f32, "gamma"), float(loss_scale),
                   _dev_ptr(out_bar, _f32, "out_bar"), _dev_ptr(h1_bar, _f32, "h1_bar"), _dev_ptr(e_bar, _f32, "e_bar"),
                   _dev_ptr(grad_dense, _f32, "grad_dense"))

    def diag_adjgrad_finish_dense(self, out_bar: torch.Tensor, h1_bar: torch.Tensor, e_bar: torch.Tensor,
                                  grad_dense: torch.Tensor):
        self._sync_versions()
        self._call("lgnn_diag_adjgrad_finish_dense", _dev_ptr(out_bar, _f32, "out_bar"), _dev_ptr(h1_bar, _f32, "h1_bar"),
                   _dev_ptr(e_bar, _f32, "e_bar"), _dev_ptr(grad_dense, _f32, "grad_dense"))
        return grad_dense

    # -- the same gradient in row bands (DiagLaplace.propose_edges: csrc/adjband.hip) ------------------------------------
    # The four calls run inside one ``propose_edges`` pass, whose driver has made the cached forward current (``forward``
    # synchronises the parameter versions): they open no batch of their own.
    def diag_adjgrad_band_sparse(self, idx, y, gamma: torch.Tensor, grad_P: torch.Tensor, out_bar: torch.Tensor,
                                 h1_bar: torch.Tensor, e_bar: torch.Tensor, loss_scale: float = 1.0):
        """``diag_adjgrad_batch`` without candidates and with every sum in a fixed order: the same bits on every run."""
        idx, y, gamma = idx.contiguous(), y.contiguous(), gamma.contiguous()
        self._call(BAND_SPARSE, _dev_ptr(idx, torch.int64, "idx"), _dev_ptr(y, torch.int64, "y"), idx.shape[0],
                   _dev_ptr(gamma, _f32, "gamma"), float(loss_scale), _dev_ptr(grad_P, _f32, "grad_P"),
                   _dev_ptr(out_bar, _f32, "out_bar"), _dev_ptr(h1_bar, _f32, "h1_bar"), _dev_ptr(e_bar, _f32, "e_bar"))

    def diag_adjgrad_band_prepare(self, out_bar: torch.Tensor, h1_bar: torch.Tensor, e_bar: torch.Tensor, grad_P: torch.Tensor):
        """Once per pass, after the last ``diag_adjgrad_band_sparse``: completes ``grad_P`` in place (the finish's bilinear terms
        on the stored entries) and returns ``(Hb [N, H], Z0 [N, H], Z1 [N, C], rs [N], cs [N])`` -- the whole-graph operands of
        every band's bilinear terms and the row / column sums behind normalize_adj backward."""
        N, (H, Cc) = self.num_nodes, self.dims[1:]
        Hb, Z0, Z1, rs, cs = self._new(N, H), self._new(N, H), self._new(N, Cc), self._new(N), self._new(N)
        self._call(BAND_PREPARE, _dev_ptr(out_bar, _f32, "out_bar"), _dev_ptr(h1_bar, _f32, "h1_bar"),
                   _dev_ptr(e_bar, _f32, "e_bar"), _dev_ptr(grad_P, _f32, "grad_P"), Hb.data_ptr(), Z0.data_ptr(), Z1.data_ptr(),
                   rs.data_ptr(), cs.data_ptr())
        return Hb, Z0, Z1, rs, cs

    def diag_adjgrad_band_batch(self, idx, y, gamma: torch.Tensor, a0: int, a1: int, band: torch.Tensor):
        """Add the per-sample all-pairs term of the samples ``idx`` (int64, nodes in ``[a0, a1)``) to ``band`` [a1 - a0, N]."""
        idx, y, gamma = idx.contiguous(), y.contiguous(), gamma.contiguous()
        self._band_check(a0, a1, band)
        self._call(BAND_BATCH, _dev_ptr(idx, torch.int64, "idx"), _dev_ptr(y, torch.int64, "y"), idx.shape[0],
                   _dev_ptr(gamma, _f32, "gamma"), int(a0), int(a1), _dev_ptr(band, _f32, "band"))

    def diag_adjgrad_band_finish(self, out_bar: torch.Tensor, prepared, e_bar: torch.Tensor, a0: int, a1: int,
                                 band: torch.Tensor):
        """Add the bilinear terms of the rows ``[a0, a1)`` and turn ``band`` in place into ``band[j - a0, i] = d / d adj[i, j]``;
        the diagonal and the stored entries leave as ``+inf``.  ``prepared``: what ``diag_adjgrad_band_prepare`` returned."""
        Hb, Z0, Z1, rs, cs = prepared
        self._band_check(a0, a1, band)
        self._call(BAND_FINISH, _dev_ptr(out_bar, _f32, "out_bar"), _dev_ptr(Hb, _f32, "Hb"), _dev_ptr(Z0, _f32, "Z0"),
                   _dev_ptr(Z1, _f32, "Z1"), _dev_ptr(e_bar, _f32, "e_bar"), _dev_ptr(rs, _f32, "rs"), _dev_ptr(cs, _f32, "cs"),
                   int(a0), int(a1), _dev_ptr(band, _f32, "band"))
        return band

    def _band_check(self, a0: int, a1: int, band: torch.Tensor):
        if not 0 <= a0 < a1 <= self.num_nodes or tuple(band.shape) != (a1 - a0, self.num_nodes):
            raise ValueError(f"band: rows [{a0}, {a1}) of {self.num_nodes} nodes need a [{a1 - a0}, {self.num_nodes}] buffer, "
                             f"got {tuple(band.shape)}")

    # -- LoRA (lgnn_lora_threshold / lgnn_lora_grad) ------------------------------------------------------------------
    def lora_threshold(self, base_rowptr: torch.Tensor, base_col: torch.Tensor, A: torch.Tensor, B: torch.Tensor,
                       scaling: float, threshold: float, symmetric: bool) -> int:
        """Re-binarise ``adj0 + scaling B A`` (symmetrised for symmetric models) into the stored graph; returns the flips."""
        A, B = A.detach().contiguous(), B.detach().contiguous()
        r = A.shape[0]
        if A.shape != (r, self.num_nodes) or B.shape != (self.num_nodes, r):
            raise ValueError("lora_A must be [r, N] and lora_B [N, r]")
        n = C.c_int64(0)
        with torch.cuda.device(self.device):
            self._call("lgnn_lora_threshold", _dev_ptr(base_rowptr, torch.int32, "base_rowptr"),
                       _dev_ptr(base_col, torch.int32, "base_col"), _dev_ptr(A, _f32, "lora_A"), _dev_ptr(B, _f32, "lora_B"), r,
                       float(scaling), float(threshold), int(bool(symmetric)), C.byref(n))
        if n.value:
            self._graph_edits += 1
        return int(n.value)

    def lora_grad(self, grad_dense: torch.Tensor, A: torch.Tensor, B: torch.Tensor, scaling: float):
        """``(scaling B^T G, scaling G A^T)`` from the dense adjacency gradient G [N, N]."""
        A, B = A.detach().contiguous(), B.detach().contiguous()
        gA, gB = torch.empty_like(A), torch.empty_like(B)
        self._call("lgnn_lora_grad", _dev_ptr(grad_dense, _f32, "grad_dense"), _dev_ptr(A, _f32, "lora_A"),
                   _dev_ptr(B, _f32, "lora_B"), A.shape[0], float(scaling), gA.data_ptr(), gB.data_ptr())
        return gA, gB
