"""Activation-generic fp64 reference of the curvature quantities (test helper; nothing of the HIP path and none of the
oracle's accumulators is involved): ``BaseGNN.forward`` (gnn/models/base_gnn.py:136-161) restated in fp64 torch over a dense
propagation matrix, every derivative taken by ``torch.autograd`` -- so ``act`` may be any differentiable function, here
``relu`` and ``tanh``.  What the oracle hard-codes as ``pre > 0`` is whatever autograd makes of the activation.

Conventions (pinned against the oracle at ``act="relu"`` by tests/test_act_reference.py):
* KFAC factors as ``Kron.kfacs`` = [[B_0, A_0], [B_0], [B_1, A_1], [B_1], ...], blocks convs.{0..L-1}.lin then res.{0..L-2};
  ``A = in^T in / n_train`` over ALL rows the Linear sees (no bias column), ``B = sum_c g_c^T g_c`` with ``g_c`` the gradient
  at the Linear's OUTPUT (all N rows) of ``sum_m <V[m, :, c], out[idx[m]]>``; regression: seeds ``sqrt(2) I`` and the factor
  0.5 spread like ``Kron.__mul__`` (sqrt(0.5) per factor of a weight block, 0.5 on a bias block), loss ``0.5 * MSE_sum``.
* Jacobians [M, C, P], parameters in module order: convs.{l}.lin.weight (row major), .bias, l = 0..L-1, then res.{l}.
* GGN: ``sum_m J^T Lambda J`` with Lambda = diag(p) - p p^T (regression: ``J^T J``, no factor; loss 0.5 * MSE_sum).
* EF: ``factor * G^T G``, ``G_m = J_m^T r_m``, r = softmax - onehot (regression: 2 (f - y), factor 0.5); loss factor * loss_sum.

Sized for tests: P is held dense (N up to a few thousand) and the Jacobians cost one backward pass per (sample, class)."""
import numpy as np
import torch

import gnn_laplace_oracle as O

F64 = torch.float64


def dense_propagation(P, N, device="cpu"):
    """[N, N] fp64 from a scipy sparse matrix, a dense array / tensor, or the (rows, cols, vals) triple of
    ``GraphEngine.export_propagation`` (duplicates add up)."""
    if isinstance(P, (tuple, list)):
        r, c, v = (torch.as_tensor(t).detach().cpu() for t in P)
        D = torch.zeros(N, N, dtype=F64)
        D.index_put_((r.long(), c.long()), v.to(F64), accumulate=True)
        return D.to(device)
    if hasattr(P, "toarray"):
        P = P.toarray()
    return torch.as_tensor(np.asarray(P.detach().cpu()) if torch.is_tensor(P) else np.asarray(P)).to(F64).to(device)


def _t(a, device):
    if a is None:
        return None
    a = a.detach().cpu() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    return a.to(F64).to(device)


class ActReference:
    def __init__(self, kind, P, X, Ws, bs, act="relu", likelihood="classification", res_weights=None, res_biases=None,
                 norm=None, norm_weight=None, norm_bias=None, norm_mean=None, norm_var=None, norm_eps=1e-5, device="cpu"):
        assert kind in ("gcn", "sage") and act in ("relu", "tanh") and likelihood in ("classification", "regression")
        self.kind, self.act, self.likelihood, self.device = kind, act, likelihood, device
        self.X = _t(X, device)
        self.N = self.X.shape[0]
        self.P = dense_propagation(P, self.N, device)
        self.L = len(Ws)
        self.Ws = [_t(w, device).requires_grad_(True) for w in Ws]
        self.bs = [_t(b, device).requires_grad_(True) for b in bs]
        self.has_res = bool(res_weights) and self.L > 1
        self.Wr = [_t(w, device).requires_grad_(True) for w in res_weights] if self.has_res else []
        self.br = [_t(b, device).requires_grad_(True) for b in res_biases] if self.has_res else []
        self.norm = None if norm in (None, "none", "", "None") or self.L == 1 else norm
        lst = lambda ts: None if ts is None else [_t(t, device) for t in ts]  # noqa: E731
        self.nw, self.nb, self.nm, self.nv, self.eps = lst(norm_weight), lst(norm_bias), lst(norm_mean), lst(norm_var), norm_eps
        self.C = self.Ws[-1].shape[0]
        self._fw = None

    # -- parameters ------------------------------------------------------------------------------------------------
    @property
    def params(self):
        ps = [t for pair in zip(self.Ws, self.bs) for t in pair]
        return ps + [t for pair in zip(self.Wr, self.br) for t in pair]

    @property
    def n_params(self):
        return sum(p.numel() for p in self.params)

    # -- forward ---------------------------------------------------------------------------------------------------
    def _act(self, x):
        return torch.relu(x) if self.act == "relu" else torch.tanh(x)

    def forward(self):
        """out [N, C]; per conv the Linear's input ``a[l]`` and output ``z[l]``; per res Linear its output ``r[l]``; ``pre[l]`` what
        the activation sees and ``hid[l]`` what it returns.  All graph tensors (cached: the parameters never change)."""
        if self._fw is not None:
            return self._fw
        h = self.X
        a, z, r, pre, hid = [], [], [], [], []
        for l in range(self.L):
            if self.kind == "gcn":
                a.append(h)
                z.append(h @ self.Ws[l].T + self.bs[l])
                s = self.P @ z[-1]
            else:
                a.append(torch.cat([h, self.P @ h], dim=1))
                z.append(a[-1] @ self.Ws[l].T + self.bs[l])
                s = z[-1]
            if l == self.L - 1:
                out = s
                break
            if self.has_res:
                r.append(h @ self.Wr[l].T + self.br[l])
                s = r[-1] + s
            if self.norm == "layer":
                mu = s.mean(dim=1, keepdim=True)
                var = ((s - mu) ** 2).mean(dim=1, keepdim=True)
                s = (s - mu) / torch.sqrt(var + self.eps) * self.nw[l] + self.nb[l]
            elif self.norm == "batch":  # eval mode: the affine map of the running statistics
                s = (s - self.nm[l]) / torch.sqrt(self.nv[l] + self.eps) * self.nw[l] + self.nb[l]
            pre.append(s)
            h = self._act(s)
            hid.append(h)
        self._fw = dict(out=out, a=a, z=z, r=r, pre=pre, hid=hid)
        return self._fw

    def _idx(self, idx):
        return torch.as_tensor(np.asarray(idx.detach().cpu()) if torch.is_tensor(idx) else np.asarray(idx)).long().to(self.device)

    def _loss(self, f, y):
        """The interface's loss: CE sum, or 0.5 * MSE sum."""
        if self.likelihood == "regression":
            return 0.5 * float(((f - _t(y, self.device).reshape(f.shape)) ** 2).sum())
        return float(torch.nn.functional.cross_entropy(f, self._idx(y), reduction="sum"))

    # -- KFAC ------------------------------------------------------------------------------------------------------
    def _seeds(self, f, fork_exact):
        M, C = f.shape
        if self.likelihood == "regression":  # Hessian square root of MSELoss(sum): sqrt(2) I
            return (2.0 ** 0.5) * torch.eye(C, dtype=F64, device=self.device).expand(M, C, C)
        return torch.from_numpy(O.kfac_seeds(f.detach().cpu().numpy().astype(np.float32), fork_exact)).to(F64).to(self.device)

    def _raw_kfac(self, idx, n_train, V, first):
        """(A list, B list) of one batch for the seed columns V [M, C, S]; ``first``: this share carries the A increments."""
        fw = self.forward()
        sel = fw["out"][self._idx(idx)]
        outs = list(fw["z"]) + list(fw["r"])
        ins = list(fw["a"]) + ([fw["a"][l] if self.kind == "gcn" else fw["a"][l][:, :fw["a"][l].shape[1] // 2]
                                for l in range(self.L - 1)] if self.has_res else [])
        A = [(x.detach().T @ x.detach()) / n_train if first else torch.zeros(x.shape[1], x.shape[1], dtype=F64, device=self.device)
             for x in ins]
        B = [torch.zeros(t.shape[1], t.shape[1], dtype=F64, device=self.device) for t in outs]
        for s in range(V.shape[2]):
            gs = torch.autograd.grad((V[:, :, s] * sel).sum(), outs, retain_graph=True)
            for k, g in enumerate(gs):
                B[k] += g.T @ g
        return A, B

    def _pack(self, A, B):
        f = 0.5 if self.likelihood == "regression" else 1.0
        kf = []
        for Ak, Bk in zip(A, B):
            kf.append([f ** 0.5 * Bk, f ** 0.5 * Ak])
            kf.append([f * Bk])
        return kf

    def kfac_batch(self, idx, y, n_train, fork_exact=True, classes=None):
        """(loss, kfacs) of one batch; ``classes=(c0, c1)``: that share of the class columns (the one with class 0 carries
        the loss and A).  Repeated node ids accumulate through ``out[idx]``."""
        fw = self.forward()
        f = fw["out"][self._idx(idx)].detach()
        V = self._seeds(f, fork_exact)
        c0, c1 = (0, self.C) if classes is None else classes
        A, B = self._raw_kfac(idx, n_train, V[:, :, c0:c1], c0 == 0)
        return (self._loss(f, y) if c0 == 0 else 0.0), self._pack(A, B)

    def kfac_fit(self, idx, y, batch_size, fork_exact=True, shares=None):
        """The fit loop over contiguous batches; ``shares``: a list of class ranges each batch is accumulated as."""
        n = len(idx)
        loss, total = 0.0, None
        for s in range(0, n, batch_size):
            for cr in (shares or [None]):
                lb, kb = self.kfac_batch(idx[s:s + batch_size], y[s:s + batch_size], n, fork_exact, cr)
                loss += lb
                total = kb if total is None else [[a + b for a, b in zip(Fa, Fb)] for Fa, Fb in zip(total, kb)]
        return loss, total

    def kfac_fisher_batch(self, idx, y, n_train, mc_labels=None):
        """Empirical (``mc_labels=None``) / Monte-Carlo Fisher KFAC: the loss gradient itself is the seed, one backward pass
        per draw, each draw weighted 1 / S."""
        fw = self.forward()
        f = fw["out"][self._idx(idx)].detach()
        draws = [y] if mc_labels is None else list(mc_labels)
        V = torch.stack([self._residual(f, d) for d in draws], dim=2) / len(draws) ** 0.5
        A, B = self._raw_kfac(idx, n_train, V, True)
        return self._loss(f, y), self._pack(A, B)

    def _residual(self, f, y):
        """d loss_sum / d f per sample: softmax - onehot, or 2 (f - y)."""
        if self.likelihood == "regression":
            return 2.0 * (f - _t(y, self.device).reshape(f.shape))
        r = torch.softmax(f, dim=1)
        r[torch.arange(f.shape[0], device=self.device), self._idx(y)] -= 1.0
        return r

    # -- Jacobians and what follows from them --------------------------------------------------------------------
    def jacobians(self, idx):
        """(J [M, C, P], f [M, C]): one autograd backward pass per (sample, class)."""
        fw = self.forward()
        idx = self._idx(idx)
        f = fw["out"][idx]
        M, C = f.shape
        J = torch.zeros(M, C, self.n_params, dtype=F64, device=self.device)
        ps = self.params
        for m in range(M):
            for c in range(C):
                gs = torch.autograd.grad(fw["out"][idx[m], c], ps, retain_graph=True)
                J[m, c] = torch.cat([g.reshape(-1) for g in gs])
        return J, f.detach()

    def _lam(self, f):
        p = torch.softmax(f, dim=1)
        return torch.diag_embed(p) - p[:, :, None] * p[:, None, :]

    def ggn(self, idx, y, full=False, J=None):
        """(loss, H): the GGN over all weights, diagonal [P] or full [P, P]."""
        J, f = self.jacobians(idx) if J is None else J
        if self.likelihood == "regression":
            H = torch.einsum("mcp,mcq->pq", J, J) if full else (J * J).sum((0, 1))
        else:
            LJ = torch.einsum("mck,mkp->mcp", self._lam(f), J)
            H = torch.einsum("mcp,mcq->pq", J, LJ) if full else (J * LJ).sum((0, 1))
        return self._loss(f, y), H

    def lastlayer_slice(self):
        o = sum(w.numel() + b.numel() for w, b in zip(self.Ws[:-1], self.bs[:-1]))
        return slice(o, o + self.Ws[-1].numel() + self.bs[-1].numel())

    def lastlayer_full(self, idx, y, J=None):
        """(loss, H): the full GGN over convs.{L-1}.lin's weight and bias."""
        J, f = self.jacobians(idx) if J is None else J
        return self.ggn(idx, y, True, (J[:, :, self.lastlayer_slice()], f))

    def ef(self, idx, y, full=False, J=None, resid_scale=None, scale=None):
        """(loss, H, G): empirical Fisher from the per-sample gradients G [M, P]; the interface's factors unless
        ``resid_scale`` / ``scale`` are given."""
        J, f = self.jacobians(idx) if J is None else J
        reg = self.likelihood == "regression"
        r = self._residual(f, y)
        if resid_scale is not None:
            r = r * (resid_scale / (2.0 if reg else 1.0))
        G = torch.einsum("mc,mcp->mp", r, J)
        factor = (0.5 if reg else 1.0) if scale is None else scale
        H = G.T @ G if full else (G * G).sum(0)
        return self._loss(f, y), factor * H, G

    @staticmethod
    def functional_variance(J, Sigma):
        """J Sigma J^T [M, C, C] for a posterior covariance Sigma [P, P] (or its diagonal [P])."""
        Sigma = Sigma.to(J)
        if Sigma.dim() == 1:
            return torch.einsum("mcp,p,mkp->mck", J, Sigma, J)
        return torch.einsum("mcp,pq,mkq->mck", J, Sigma, J)
