"""The Kronecker and the diagonal posterior over the head ``model.convs[-1].lin`` alone."""
import torch

from .diag import DiagLaplace
from .fit import Accumulator, ParametricLaplace
from .kron import KronLaplace


class _LastLayerHead:
    """What the Kronecker and the diagonal last-layer posteriors share (laplace/lllaplace.py:381-475, 477-...): the parameters
    are the head's -- ``model.convs[-1].lin``, weight (row major) then bias; NOT the last ``nn.Linear`` in module order, which is
    a residual Linear for ``res=True`` -- and the predictive is evaluated from the head's feature rows (``f_n = W phi_n + s_n b``,
    ``lgnn_lastlayer_features``) in chunks: no ``[M, C, P_ll]`` Jacobians, no forward pass per parameter sample."""
    _sample_additive = True  # A = Phi^T Phi / N, B = sum_n V_n V_n^T, the diagonal: plain sums over the batch rows

    def _init_head(self, model, likelihood):
        if likelihood != "classification":
            raise NotImplementedError("last-layer Kronecker / diagonal Laplace: classification likelihood only")
        convs = getattr(model, "convs", None)
        if convs is None or not hasattr(convs[-1], "lin"):
            raise TypeError("last-layer Laplace needs a model whose head is model.convs[-1].lin (GCN / GraphSAGE)")
        self._head = convs[-1].lin
        self.params = [self._head.weight, self._head.bias]
        self.n_params = sum(p.numel() for p in self.params)
        self.n_layers = 2
        self._backend_kwargs = dict(self._backend_kwargs, last_layer=True)

    def _matrix_free_operands(self, out_map=None):
        return None  # (csrc/predictive.hip serves posteriors over all weights)

    def _covariance_operands(self):
        return None  # (csrc/glmcov.hip likewise: the joint predictive takes the head's explicit Jacobians)

    def neg_marglik_adj_grad(self, *args, **kwargs):
        raise NotImplementedError("adjacency gradient: posteriors over all weights (KronLaplace, DiagLaplace, FullLaplace)")

    def propose_edges(self, *args, **kwargs):
        raise NotImplementedError("propose_edges: the diagonal posterior over all weights (DiagLaplace)")

    def _ll_variance(self, phi, s, diagonal_output: bool):
        raise NotImplementedError

    _LL_CHUNK_FLOATS = 1 << 27  # floats of a chunk's largest temporary ([M, C, C] covariances, [S, M, C] sampled logits)

    def _glm_predictive_distribution(self, x, diagonal_output: bool = False, joint: bool = False):
        """(f_mu [M, C], f_var [M, C, C] or its diagonal [M, C]) in closed form from the feature rows; ``joint``: the
        cross-node covariance from the head's explicit Jacobians (``last_layer_jacobians``)."""
        if joint:
            return ParametricLaplace._glm_predictive_distribution(self, x, joint=True)
        C = self.n_outputs
        chunk = max(1, self._LL_CHUNK_FLOATS // max(C * C, self._head.weight.shape[1]))
        mus, fvars = [], []
        for s0 in range(0, max(int(x.shape[0]), 1), chunk):
            phi, s, f = self.backend.lastlayer_features(x[s0:s0 + chunk])
            mus.append(f)
            fvars.append(self._ll_variance(phi, s, diagonal_output))
        return (mus[0], fvars[0]) if len(mus) == 1 else (torch.cat(mus), torch.cat(fvars))

    @torch.no_grad()
    def __call__(self, x, pred_type: str = "glm", link_approx: str = "probit", n_samples: int = 100,
                 diagonal_output: bool = False, generator: torch.Generator | None = None,
                 eps: torch.Tensor | None = None, **kwargs):
        """As ``ParametricLaplace.__call__``; ``pred_type="nn"`` draws HEAD samples only (laplace/lllaplace.py:209-232) and
        evaluates ``f_s = Phi W_s^T + s (x) b_s`` as one batched product per chunk of nodes: the model's parameters are never
        written."""
        if pred_type != "nn":
            return super().__call__(x, pred_type=pred_type, link_approx=link_approx, n_samples=n_samples,
                                    diagonal_output=diagonal_output, generator=generator, eps=eps, **kwargs)
        if link_approx != "mc":
            raise ValueError("Only mc link approximation is supported for nn prediction type.")
        theta = self.sample(n_samples, generator=generator, eps=eps)  # [S, C D + C]
        outs = [p.mean(dim=0) for p in self._nn_sample_chunks(x.to(self._device), theta)]
        return outs[0] if len(outs) == 1 else torch.cat(outs)

    def _nn_sample_chunks(self, x, theta):
        """The per-sample softmax [S, m, C] of the head samples ``theta``, one chunk of evaluation nodes at a time."""
        S = theta.shape[0]
        C, D = self._head.weight.shape
        Ws, bs = theta[:, :C * D].reshape(S, C, D), theta[:, C * D:]
        chunk = max(1, self._LL_CHUNK_FLOATS // max(S * C, D))
        for s0 in range(0, max(int(x.shape[0]), 1), chunk):
            phi, s, _ = self.backend.lastlayer_features(x[s0:s0 + chunk])
            f = torch.einsum("nd,scd->snc", phi, Ws) + s.reshape(1, -1, 1) * bs.unsqueeze(1)
            yield torch.softmax(f, dim=-1)

    @torch.no_grad()
    def _nn_predictive_samples(self, x, n_samples: int = 100, generator: torch.Generator | None = None,
                               eps: torch.Tensor | None = None):
        """[S, M, C]: the softmax under each HEAD sample (what ``__call__(pred_type="nn")`` averages); nothing is written."""
        theta = self.sample(n_samples, generator=generator, eps=eps)
        outs = list(self._nn_sample_chunks(x.to(self._device), theta))
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)


class KronLLLaplace(_LastLayerHead, KronLaplace):
    """Kronecker-factored GGN of the head alone (laplace/lllaplace.py:381-475 with CurvlinopsInterface.kron on the final
    nn.Linear, laplace/curvature/curvlinops.py:77-108): ``H = Kron([[B, A], [B_b]])`` with ``A = Phi^T Phi / N`` [D, D],
    ``B = sum_n V_n V_n^T`` and the bias block ``B_b = sum_n s_n^2 V_n V_n^T`` [C, C].  Decomposition, the
    ``override=False`` discounting, marginal likelihood, prior-precision optimisation, ``state_dict`` and ``sample`` are
    ``KronLaplace``'s.  No decomposition cache keyed on the features and no early side-stream snapshot: the factors here are
    not ``X^T X``, they move with every weight update."""
    _key = ("last_layer", "kron")

    def __init__(self, model, likelihood, *args, **kwargs):
        super().__init__(model, likelihood, *args, **kwargs)
        self._init_head(model, likelihood)

    def _inplace_backend(self) -> bool:
        return hasattr(self.backend, "lastlayer_kron_accumulate_")

    def _shard_plan(self, train_loader, rank: int, world: int):
        return ParametricLaplace._shard_plan(self, train_loader, rank, world)  # sample slices, not (batch, class) units

    def _new_accumulator(self, override):
        be = self.backend
        if not self._inplace_backend():
            return None
        flat, A, B, Bb, loss_buf = be.engine.new_lastlayer_kron_buffers()  # [A | B | B_b | loss]: one flat buffer

        def fold(la):
            la.H = la.H + be.pack_lastlayer_kron(A, B, Bb)
        return Accumulator(flat, loss_buf, (A, B, Bb), fold)

    def _curv_closure(self, X, y, N):
        acc = self._accumulator()
        if acc is None:
            return self.backend.kron(X, y, N=N, **self._asdl_fisher_kwargs)
        self.backend.lastlayer_kron_accumulate_(*acc.bufs, acc.loss, X, y, N)
        return 0.0, None

    def _decompose_cache(self, train_loader, override: bool):
        return None, None

    def _ll_variance(self, phi, s, diagonal_output: bool):
        """``f_var[n] = Q_B diag_c(sum_d u_nd^2 / (f l_B,c l_A,d + delta_w)) Q_B^T + s_n^2 Q_b diag(1 / (f l_b + delta_b)) Q_b^T``
        with ``u_n = Q_A^T phi_n``: ``J_n P^-1 J_n^T`` of ``J_n = [I_C (x) phi_n^T | s_n I_C]`` under the decomposed posterior
        precision (``damping``: ``(sqrt(f) l_B + sqrt(delta)) (sqrt(f) l_A + sqrt(delta))`` as ``KronDecomposed``), from the fp64
        eigenpairs of the fitted factors (``_eigh64``)."""
        f = float(self._H_factor)
        pp = self._block_prior_precision(self.n_layers, torch.float64)
        if pp.numel() != self.n_layers:
            raise ValueError("Prior precision for Kron either scalar or per-layer.")
        dw, db = pp[0], pp[1]
        (lB, QB), (lA, QA), (lb, Qb) = self._eigh64(0, 0), self._eigh64(0, 1), self._eigh64(1, 0)
        if self.damping:
            den = torch.outer(f ** 0.5 * lB + dw.sqrt(), f ** 0.5 * lA + dw.sqrt())
        else:
            den = f * torch.outer(lB, lA) + dw
        kb = 1.0 / (f * lb + db)
        u = phi @ QA.to(phi.dtype)
        w = (u * u) @ (1.0 / den).to(phi.dtype).T  # [M, C]
        s2 = (s * s).to(phi.dtype)
        if diagonal_output:
            return w @ (QB * QB).to(phi.dtype).T + s2.unsqueeze(1) * ((Qb * Qb) @ kb).to(phi.dtype)
        QBf = QB.to(phi.dtype)
        return (QBf.unsqueeze(0) * w.unsqueeze(1)) @ QBf.T + s2.reshape(-1, 1, 1) * ((Qb * kb) @ Qb.T).to(phi.dtype)


class DiagLLLaplace(_LastLayerHead, DiagLaplace):
    """Diagonal GGN of the head alone (laplace/lllaplace.py:477-... with GGNInterface.diag on last_layer_jacobians,
    laplace/curvature/curvature.py:132-167, 412-432): ``H[c D + d] = sum_n Lambda_n[c, c] phi_n[d]^2``,
    ``H[C D + c] = sum_n Lambda_n[c, c] s_n^2``.  Stands to ``DiagLaplace`` as ``KronLLLaplace`` to ``KronLaplace``; its fits are
    not captured into a hipGraph."""
    _key = ("last_layer", "diag")

    def __init__(self, model, likelihood, *args, **kwargs):
        super().__init__(model, likelihood, *args, **kwargs)
        self._init_head(model, likelihood)

    fit = ParametricLaplace.fit  # (never captured)
    _accumulate_entry = "lastlayer_diag_accumulate_"

    def _inplace_backend(self) -> bool:
        return hasattr(self.backend, self._accumulate_entry) and not self._asdl_fisher_kwargs and self._owns_H()

    def _ll_variance(self, phi, s, diagonal_output: bool):
        """``f_var[n] = diag_c(sum_d phi_nd^2 / P_w[c, d] + s_n^2 / P_b[c])``: independent parameters, a diagonal covariance."""
        C, D = self._head.weight.shape
        inv = 1.0 / self.posterior_precision
        v = (phi * phi) @ inv[:C * D].view(C, D).T + (s * s).unsqueeze(1) * inv[C * D:].unsqueeze(0)
        return v if diagonal_output else torch.diag_embed(v)
