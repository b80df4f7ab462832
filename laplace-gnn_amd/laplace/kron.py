"""``KronLaplace``: KFAC over all weights -- the (batch, class) shard plan, the early side-stream decomposition of large input
covariances, the decompose cache, fp64 eigenpairs of the fitted factors and what reads them (matrix-free operands, the
adjacency gradient's factor gradients)."""
import numpy as np
import torch

from ..adjgrad import _adjgrad_drive, _adjgrad_prelude
from ..data import units_of_rank
from ..matrix import _SMALL_EIG, Kron, KronDecomposed, symeig_batched_hip
from .dist import _dist_info
from .fit import Accumulator, ParametricLaplace


class KronLaplace(ParametricLaplace):
    _key = ("all", "kron")

    def __init__(self, model, likelihood, *args, damping: bool = False, cache_decompositions: bool = True, **kwargs):
        self.damping = damping
        self.H_facs = None
        # reuse the eigendecomposition of a GCN's first input covariance across fits of the same model (``_decompose_cache``)
        self.cache_decompositions = bool(cache_decompositions)
        super().__init__(model, likelihood, *args, **kwargs)
        # the early decomposition of large input covariances (_snapshot_large_input_factors): whether this fit takes it, the
        # snapshots waiting for the side stream, and the eigenpairs that came back
        self._early_ok, self._early_pending, self._early, self._side_stream = False, None, {}, None

    def _init_H(self):
        self.H = Kron.init_from_model(self.params, self._device)

    def state_dict(self) -> dict:  # laplace/baselaplace.py:1664-1677: the factors, not their decomposition
        sd = super().state_dict()
        sd["H"] = self.H_facs.kfacs
        return sd

    def load_state_dict(self, state_dict: dict) -> None:
        super().load_state_dict(state_dict)
        # a fresh container WITHOUT the tied-factor hint: the loaded bias blocks need not repeat their weight block's B
        # (regression: sqrt(.5) B vs .5 B), so decompose compares the tensors
        self.H_facs = Kron(state_dict["H"])
        self.H = self.H_facs.decompose(damping=self.damping)

    def _inplace_backend(self) -> bool:
        """The in-place (flat buffer, class-range capable) fast path exists for the GGN factors of the HIP backend; the
        empirical / MC Fisher variants go through ``backend.kron`` like any other backend."""
        be = self.backend
        return hasattr(be, "kron_accumulate_") and getattr(be, "_kron_fisher_type", "type2") == "type2"

    def _new_accumulator(self, override):
        be = self.backend
        if not self._inplace_backend():
            return None
        flat, views, loss_buf = be.new_kfac_buffers() if hasattr(be, "new_kfac_buffers") else be.engine.new_kfac_buffers()

        def fold(la):
            la.H = la.H + be.pack_kron(views)
        # [A_0|B_0|...|loss] is one buffer (a stand-in without one: every factor and the loss on their own)
        parts = None if flat is not None else [t for pair in views for t in pair] + [loss_buf]
        return Accumulator(flat, loss_buf, views, fold, parts)

    def _curv_closure(self, X, y, N, classes=None):
        first = self._acc is None
        acc = self._accumulator()
        if acc is None:
            return self.backend.kron(X, y, N=N, **self._asdl_fisher_kwargs)
        self.backend.kron_accumulate_(acc.bufs, acc.loss, X, y, N, classes=classes)
        if first and self._early_ok:
            self._snapshot_large_input_factors(acc.bufs)
        return 0.0, None

    def _snapshot_large_input_factors(self, views):
        """The input covariances do not depend on the batch: every batch adds the same ``in_l^T in_l / N_train`` (the forward
        pass is cached per weight version), so after the FIRST batch of an ``override=True`` fit a factor already has its
        final eigenvectors and its eigenvalues up to the scale ``T``.  Factors too large for the one-workgroup
        decomposition (more than 256 rows: a GraphSAGE's ``A_1`` is 2 H wide, 512 at the arxiv shape) cost a library
        ``syevd`` of ~12 ms -- a chain of a few thousand tiny launches that used to run after the batch loop.  They are
        copied here, behind the first batch; ``_finish_accumulate`` -- the host has queued every batch by then and the
        device is tens of milliseconds behind -- starts their decomposition on a side stream, where it overlaps the
        remaining batches; ``fit`` hands the result (eigenvalues rescaled by the ratio of the traces, a device scalar: no
        synchronisation) to ``decompose``."""
        big = [l for l, (A, _) in enumerate(views) if A.is_cuda and A.shape[0] > _SMALL_EIG]
        if not big:
            return
        snaps = [views[l][0].clone() for l in big]  # A_l after one batch (the buffers keep accumulating)
        ev = torch.cuda.Event()
        ev.record()
        self._early_pending = (big, snaps, [a.diagonal().sum() for a in snaps], ev)

    def _finish_accumulate(self):
        pending, self._early_pending = self._early_pending, None
        if pending is None:
            return
        big, snaps, traces, ev = pending
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream(device=snaps[0].device)
        self._side_stream.wait_event(ev)
        with torch.cuda.stream(self._side_stream):
            pairs = symeig_batched_hip(snaps)
        for a in snaps:
            a.record_stream(self._side_stream)
        self._early = {l: (lam, Q, tr) for l, (lam, Q), tr in zip(big, pairs, traces)}

    def _shard_plan(self, train_loader, rank: int, world: int):
        """Backends that can restrict a call to a range of class columns get the balanced (batch, class)
        decomposition of ``data.units_of_rank``; others fall back to whole batches round-robin."""
        be = self.backend
        if world == 1 or not (self._inplace_backend() and hasattr(be, "num_classes")):
            return super()._shard_plan(train_loader, rank, world)
        mine = {t: (c0, c1) for t, c0, c1 in units_of_rank(len(train_loader), be.num_classes, rank, world)}
        return lambda t, M: mine.get(t)

    def _reduce_tensors(self):
        # every block is reduced on its own: a ring sums the elements of a bias block's B and of its weight block's B in
        # different rank orders, so the two may differ in the last bit afterwards -- and a rank without local batches
        # would still carry the "tied" hint of its zero-initialised container.  All ranks compare instead.
        self.H._tied = frozenset()
        return [Hi for F in self.H.kfacs for Hi in F]

    @staticmethod
    def _rescale_factors(kron: Kron, factor: float) -> Kron:
        for F in kron.kfacs:
            if len(F) == 2:
                F[1] *= factor
        return kron

    def fit(self, train_loader, override: bool = True, progress_bar: bool = False, process_group=None) -> None:
        rank_world = _dist_info(process_group)
        self._early, self._early_pending = {}, None
        # (see _snapshot_large_input_factors; single process, fresh factors, and no exact-key cache for the same factor)
        self._early_ok = (override and rank_world[1] == 1 and self.cache_decompositions and self._inplace_backend()
                          and self._decompose_cache(train_loader, override)[0] is None)
        if override:
            self.H_facs = None
        if self.H_facs is not None:
            n_data_old, n_data_new = self.n_data, len(train_loader.dataset)
            self._init_H()
            self.H_facs = self._rescale_factors(self.H_facs, n_data_old / (n_data_old + n_data_new))
        super().fit(train_loader, override=override, progress_bar=progress_bar, process_group=process_group)
        if self.H_facs is None:
            self.H_facs = self.H
        else:
            self.H = self._rescale_factors(self.H, n_data_new / (n_data_new + n_data_old))
            self.H_facs += self.H
        cache, keys = self._decompose_cache(train_loader, override)
        if self._early and cache is None:
            torch.cuda.current_stream(self._side_stream.device).wait_stream(self._side_stream)
            cache, keys = {}, {}
            main = torch.cuda.current_stream(self._side_stream.device)
            for l, (lam, Q, tr) in self._early.items():  # block 2 l = layer l's weight block, factor 1 = its A
                lam.record_stream(main)  # (allocated on the side stream, read on this one from here on)
                Q.record_stream(main)
                final = self.H_facs.kfacs[2 * l][1]
                cache[("early", l)] = (lam * (final.diagonal().sum() / tr), Q)
                keys[(2 * l, 1)] = ("early", l)
        self._early = {}
        self.H = self.H_facs.decompose(damping=self.damping, process_group=process_group, cache=cache, cache_keys=keys)

    def _decompose_cache(self, train_loader, override: bool):
        """A GCN's first input covariance is ``factor^(1/2) (T / N_train) X^T X``: a function of the feature tensor, the batch
        count and N_train only -- not of the weights, not of the adjacency -- yet at the Cora shape (1 433 x 1 433) its
        decomposition is 30 ms of a 2 ms fit, and the fork's structure-learning loop refits after every adjacency step
        (gnn/marglik_training.py:197-216).  The eigenpairs are kept ON THE MODEL OBJECT under an exact key: the identity and
        version counter of the feature tensor (a strong reference is held, so the storage cannot be recycled under the key),
        T, N_train and the likelihood factor.  Nothing is compared numerically; ``cache_decompositions=False`` opts out."""
        be = self._backend
        eng = getattr(be, "engine", None) if be is not None else None
        if (not self.cache_decompositions or not override or eng is None or getattr(eng, "kind", None) != "gcn"
                or not hasattr(eng, "feature_token") or getattr(be, "_kron_fisher_type", "type2") != "type2"):
            return None, None
        store = self.model.__dict__.setdefault("_lgnn_eig_cache", {})
        key = ("gcn_A0", eng.feature_token(), len(train_loader), len(train_loader.dataset), float(be.factor))
        return store, {(0, 1): key}

    def _precision_of(self, H) -> KronDecomposed:
        pp = torch.as_tensor(self.prior_precision, dtype=torch.float32, device=self._device).reshape(-1)
        if pp.numel() not in (1, self.n_layers):
            raise ValueError("Prior precision for Kron either scalar or per-layer.")
        return H * self._H_factor + pp

    @property
    def posterior_precision(self) -> KronDecomposed:
        return self._precision_of(self.H)

    # ---- fp64 eigenpairs of the fitted factors: what divides by (eigenvalue products + prior precision) reads these -----
    _FP64_EIG_MAX = 512  # factors up to this size are re-decomposed in fp64 (larger ones keep the fit's own eigenpairs)

    def _eigh64(self, block: int, k: int):
        """(eigenvalues, eigenvectors) in fp64 of factor ``k`` of block ``block`` of the fitted (fp32) factors, cached per fit.
        The fit's own decomposition is fp32 (hand-written tridiagonalisation + divide and conquer): its eigenvalues carry an
        ABSOLUTE error of ~1e-6 of the factor's largest one, i.e. the small ones -- which dominate ``1 / (f lB_i lA_j + delta)``
        -- have no correct digit, and the float atomics of the accumulation make that error differ from run to run.  An fp64
        decomposition of the same fp32 factor has none of it: what remains is the factors' own last-bit noise (~1e-7).
        Factors of up to 128 rows on a host core (numpy: 0.1 ms; the device needs 2 ms of launches for a 64 x 64 matrix, and
        torch's CPU eigh spins up the whole intra-op pool), up to ``_FP64_EIG_MAX`` rows on the device, larger ones (Cora's
        1 433 x 1 433 X^T X: 40 ms in fp64) keep the fit's pairs."""
        store = self.__dict__.setdefault("_eig64", {})
        if store.get("for") is not self.H:  # a new fit / load_state_dict made a new decomposition object
            store.clear()
            store["for"] = self.H
        t = self.H_facs.kfacs[block][k]
        key = (t.data_ptr(), tuple(t.shape))
        if key not in store:
            n = t.shape[0]
            if n <= 128:
                lam, Q = np.linalg.eigh(t.double().cpu().numpy())
                pair = (torch.from_numpy(lam).to(t.device), torch.from_numpy(Q).to(t.device))
            elif n <= self._FP64_EIG_MAX:
                pair = torch.linalg.eigh(t.double())
            else:
                pair = (self.H.eigenvalues[block][k].double(), self.H.eigenvectors[block][k].double())
            store[key] = (pair[0].clamp(min=0.0), pair[1])  # (symeig's clamp, laplace/utils/utils.py:193-226)
        return store[key]

    def _refined_decomposition(self) -> KronDecomposed:
        """The fit's ``KronDecomposed`` with every factor's eigenpairs replaced by the fp64 ones (rounded to fp32: each
        eigenvalue then has a RELATIVE error of 6e-8).  What the predictive and the samples invert; the marginal likelihood
        -- the per-epoch quantity -- keeps the fit's own pairs (its logdet is insensitive: 3.7e-7 measured)."""
        H = self.H
        if not isinstance(H, KronDecomposed):
            return H
        store = self.__dict__.setdefault("_eig64", {})
        if store.get("for") is H and "refined" in store:
            return store["refined"]
        vals, vecs = [], []
        for i, ls in enumerate(H.eigenvalues):
            pairs = [self._eigh64(i, k) for k in range(len(ls))]
            vals.append([lam.float() for lam, _ in pairs])
            vecs.append([Q.float() for _, Q in pairs])
        store["refined"] = KronDecomposed(vecs, vals, H.deltas, H.damping)
        return store["refined"]

    @property
    def posterior_precision_refined(self) -> KronDecomposed:
        return self._precision_of(self._refined_decomposition())

    # ---- 8(f)-4: what the GNN driver differentiates (gnn/marglik_training.py:197-216) ------------------------------
    def _logdet_factor_gradients(self):
        """``d logdet(P) / d B_l`` and ``/ d A_l`` per layer (laplace/utils/matrix.py:371-394: ``sum log(f lB_i lA_j + delta)``
        per weight block, ``sum log(f lB_i + delta)`` per bias block, f = H_factor): ``Q diag(.) Q^T`` in the factor's own
        eigenbasis, formed in fp64 from the fp64 eigenpairs (``_eigh64``): with the fit's fp32 pairs these matrices are off
        by up to 3e-3, and that was the adjacency gradient's whole device error (3.3e-4 at a GraphSAGE with 256 hidden units,
        4.4e-6 with this; tools/adjgrad_attribution.py, profiles/r03_adjgrad_attribution.log)."""
        f = float(self._H_factor)
        deltas = self._block_prior_precision(self.n_layers, torch.float64)
        kf = self.H_facs.kfacs
        eigh64 = self._eigh64

        gB, gA = [], []
        for l in range(len(kf) // 2):
            (lB, QB), (lA, QA), (lBb, QBb) = eigh64(2 * l, 0), eigh64(2 * l, 1), eigh64(2 * l + 1, 0)
            den = f * torch.outer(lB, lA) + deltas[2 * l]
            cB = (f * lA.unsqueeze(0) / den).sum(dim=1)
            cA = (f * lB.unsqueeze(1) / den).sum(dim=0)
            cBb = f / (f * lBb + deltas[2 * l + 1])
            gB.append(((QB * cB) @ QB.T + (QBb * cBb) @ QBb.T).float())
            gA.append(((QA * cA) @ QA.T).float())
        return gB, gA

    def neg_marglik_adj_grad(self, train_loader, prior_precision=None, process_group=None, candidates=None, dense=False):
        """``-log_marginal_likelihood()`` of this fit and its gradient w.r.t. the adjacency the model propagates with --
        what ``neg_marglik.backward()`` leaves in ``model.adj.grad`` in the reference's structure-learning loop
        (gnn/marglik_training.py:197-216), here on the stored sparsity pattern: returns ``(neg_marglik, edge_index [2, nnz],
        grad [nnz])`` over the stored entries of the 0/1 adjacency (``model.engine.export_adj()`` order; a GCN's self loops
        carry gradient 0 like the reference's overwritten diagonal).  1- and 2-layer GCN (STEGCN) and 2-layer GraphSAGE (STEGraphSAGE).  ``train_loader`` must be the loader of the fit
        (same batch boundaries: the B factors depend on them).  Inside a ``torch.distributed`` job whole batches are
        dealt round-robin and the accumulators are all-reduced once.

        ``candidates`` (int64 [2, K], pairs (i, j) that are NOT stored): the reference's dense ``adj.grad`` also has an
        entry for every non-edge -- that is how its structure learning proposes new edges.  With candidates a fourth value
        is returned: ``d(-marglik) / d adj[i, j]`` for each listed pair.

        ``dense=True`` (plain 2-layer GCN; LoRASTEGCN, gnn/models/models.py:186-235): returns ``(neg_marglik, grad [N, N])``,
        ``d(-marglik) / d adj[i, j]`` for EVERY pair (symmetrised for symmetric models, diagonal 0) -- the dense ``adj.grad`` of
        the reference, from tile GEMMs on the full grid (csrc/lora.hip)."""
        eng = _adjgrad_prelude(self, "KronLaplace", "the Kronecker posterior", self.H_facs is not None, prior_precision,
                               candidates, dense, batch="adjgrad_batch")
        value = -self._log_marginal_likelihood64()
        gB, gA = self._logdet_factor_gradients()
        gB = [0.5 * g for g in gB]  # neg marglik = H_factor * loss + 1/2 (logdet P - logdet P_0 + scatter)
        gA = [0.5 * g for g in gA]
        a_scale = len(train_loader) / len(train_loader.dataset)
        return (value, *_adjgrad_drive(eng, train_loader, process_group, candidates, bool(getattr(self.model, "symmetric", False)),
                                       dense, batch="adjgrad_batch", finish="adjgrad_finish", weight=gB, per_sample=False,
                                       finish_args=(gA, a_scale), fork_exact=getattr(self.backend, "fork_exact_seed", True),
                                       loss_scale=self._H_factor))

    @property
    def log_det_posterior_precision(self) -> torch.Tensor:
        return self.posterior_precision.logdet()

    def _log_marginal_likelihood64(self) -> torch.Tensor:
        """``log_marginal_likelihood()`` with the log determinant summed in fp64 over the fp64 eigenvalues (the structure-
        learning step needs them for its gradient anyway): fp32 value within 1e-6 of the fp64 oracle where the fit's own
        pairs left 5.7e-5 on one configuration of 420 (seed 346 of tools/stress_adjgrad.py, H = 256: a near-singular B_0
        whose ~200 smallest eigenvalues each carried the fp32 decomposition's absolute error into log(f lB lA + delta))."""
        if self.damping:
            return self.log_marginal_likelihood()
        f = float(self._H_factor)
        deltas = self._block_prior_precision(self.n_layers, torch.float64)
        ld = torch.zeros((), dtype=torch.float64, device=self._device)
        for i, F in enumerate(self.H_facs.kfacs):
            l0 = self._eigh64(i, 0)[0]
            if len(F) == 1:
                ld = ld + torch.log(f * l0 + deltas[i]).sum()
            else:
                ld = ld + torch.log(f * torch.outer(l0, self._eigh64(i, 1)[0]) + deltas[i]).sum()
        ld_prior = self.prior_precision_diag.double().log().sum()
        mean = self.mean.double()
        delta = mean - torch.as_tensor(self.prior_mean, device=mean.device, dtype=mean.dtype)
        scatter = (delta * self.prior_precision_diag.double()) @ delta
        return (self.log_likelihood - 0.5 * (ld - ld_prior + scatter)).float()

    def _matrix_free_operands(self, out_map=None):
        H = self._refined_decomposition()
        nb = len(H.eigenvalues) if isinstance(H, KronDecomposed) else 0
        if nb not in (2, 4, 6) or H.damping:  # convs.0.{W,b}, convs.1.{W,b} and, models with res, res.0.{W,b}
            return None
        if nb == 2:  # a 1-layer model: its only layer's operands go where the last layer's go, the first layer's stay None
            (lB, lA), (QB, QA) = H.eigenvalues[0], H.eigenvectors[0]
            (lBb,), (QBb,) = H.eigenvalues[1], H.eigenvectors[1]
            d = self._block_prior_precision(nb)
            if d.numel() != nb:
                return None
            f = self._H_factor
            if out_map is not None:
                E = out_map.to(QB)
                QB, QBb = E @ QB, E @ QBb
            return dict(S0=None, S1=1.0 / (f * torch.outer(lB, lA) + d[0]), kappa=(QBb * QBb) @ (1.0 / (f * lBb + d[1])), QA1=QA,
                        QB1sq=QB * QB)
        (lB0, lA0), (QB0, QA0) = H.eigenvalues[0], H.eigenvectors[0]
        (lB0b,), (QB0b,) = H.eigenvalues[1], H.eigenvectors[1]
        (lB1, lA1), (QB1, QA1) = H.eigenvalues[2], H.eigenvectors[2]
        (lB1b,), (QB1b,) = H.eigenvalues[3], H.eigenvectors[3]
        if not (QB0b is QB0 or torch.equal(QB0b, QB0)):  # the bias block must share its weight block's eigenbasis of B_0
            return None
        d = self._block_prior_precision(nb)
        if d.numel() != nb:
            return None
        f = self._H_factor
        S0 = torch.cat([1.0 / (f * torch.outer(lB0, lA0) + d[0]), (1.0 / (f * lB0b + d[1])).unsqueeze(1)], dim=1)
        S1 = 1.0 / (f * torch.outer(lB1, lA1) + d[2])
        if out_map is not None:  # the rows of E f: E Q_B takes Q_B's place in the last-layer blocks
            E = out_map.to(QB1)
            QB1, QB1b = E @ QB1, E @ QB1b
        kappa = (QB1b * QB1b) @ (1.0 / (f * lB1b + d[3]))
        ops = dict(S0=S0, S1=S1, kappa=kappa, QA0=QA0, QB0=QB0, QA1=QA1, QB1sq=QB1 * QB1)
        if nb == 6:
            (lBr, lAr), (QBr, QAr) = H.eigenvalues[4], H.eigenvectors[4]
            (lBrb,), (QBrb,) = H.eigenvalues[5], H.eigenvectors[5]
            if not (QBrb is QBr or torch.equal(QBrb, QBr)):
                return None
            ops.update(Sr=torch.cat([1.0 / (f * torch.outer(lBr, lAr) + d[4]), (1.0 / (f * lBrb + d[5])).unsqueeze(1)], dim=1),
                       QAr=QAr, QBr=QBr)
        return ops

    def _scale_samples(self, eps):  # laplace/baselaplace.py:1646-1655
        return self.posterior_precision_refined.bmm(eps, exponent=-0.5).reshape(eps.shape[0], self.n_params)

    def functional_variance(self, Js):  # laplace/baselaplace.py:1635-1636 (fp64 eigenpairs: see _eigh64)
        return self.posterior_precision_refined.inv_square_form(Js)

    def _covariance_rows(self, J):  # the P^-1 W^T of inv_square_form (laplace/baselaplace.py:1638-1644, utils/matrix.py)
        return self.posterior_precision_refined.bmm(J, exponent=-1)

    def _covariance_operands(self):
        """Per Linear block: ``QA`` / ``QB`` the refined eigenvectors of its factors, ``S = [1 / (f lB (x) lA + delta_W) |
        1 / (f lB_b + delta_b)]``.  None under damping, and where a bias block's ``B`` factor is not a multiple of its weight
        block's (the device rotates both with one ``Q_B``)."""
        H = self._refined_decomposition()
        if not isinstance(H, KronDecomposed) or H.damping or len(H.eigenvalues) % 2:
            return None
        nb = len(H.eigenvalues)
        d = self._block_prior_precision(nb)
        if d.numel() != nb:
            return None
        f = self._H_factor
        QA, QB, S = [], [], []
        for l in range(0, nb, 2):
            if len(H.eigenvalues[l]) != 2 or len(H.eigenvalues[l + 1]) != 1:
                return None
            (lB, lA), (qB, qA) = H.eigenvalues[l], H.eigenvectors[l]
            (lBb,), (qBb,) = H.eigenvalues[l + 1], H.eigenvectors[l + 1]
            if not (qBb is qB or (qBb.shape == qB.shape and torch.equal(qBb, qB))):
                # a multiple of the weight block's B (regression: sqrt(factor) there, factor here) has its eigenvectors up to
                # the gauge: take Q_B if it diagonalises the bias block's factor to 1e-5 of its largest eigenvalue
                if qBb.shape != qB.shape:
                    return None
                Q64 = self._eigh64(l, 0)[1]
                D = Q64.T @ self.H_facs.kfacs[l + 1][0].double() @ Q64
                lam = torch.diagonal(D)
                if float((D - torch.diag(lam)).abs().max()) > 1e-5 * float(lam.abs().max()):
                    return None
                lBb = lam.clamp(min=0.0).float()
            S.append(torch.cat([1.0 / (f * torch.outer(lB, lA) + d[l]), (1.0 / (f * lBb + d[l + 1])).unsqueeze(1)], dim=1))
            QA.append(qA)
            QB.append(qB)
        return dict(QA=QA, QB=QB, S=S)
