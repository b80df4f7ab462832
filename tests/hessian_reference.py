"""fp64 reference of the exact loss Hessian of plain GCN / GraphSAGE models (test helper).  Plain torch on the CPU: a dense
forward as a function of the flat parameter vector, every derivative by ``torch.autograd``.  Nothing of the library and nothing
of the oracle is imported; tests/test_hessian_reference.py pins it to the reference's goldens.

Conventions: parameters in Laplace order, ``convs.{l}.lin.weight`` (row major) then ``.bias`` for l = 0 .. L-1.  The loss is the
interface's ``factor * lossfunc``: the summed cross entropy, or 0.5 times the summed squared error.  Then
``H = GGN + R`` with ``GGN = sum_n J_n^T Lambda_n J_n`` (regression: ``sum J^T J``) and ``R = sum_n sum_c r_nc grad^2 f_nc``,
``r = softmax(f) - onehot(y)`` (regression: ``f - y``)."""
import torch

F64 = torch.float64


def propagation(kind, edge_index, N):
    """Dense fp64 [N, N] of what the convs multiply with.  The edges are a set (duplicates count once) without self loops.
    GCN (gnn/models/utils.py:106-112): self loops added, ``D A^T D`` with ``D = rowsum(A)^-1/2``.  GraphSAGE
    (gnn/models/layers.py:18-24): ``A / rowsum(A)``, a zero row sum read as 1."""
    ei = torch.as_tensor(edge_index).long()
    A = torch.zeros(N, N, dtype=F64)
    A[ei[0], ei[1]] = 1.0
    A.fill_diagonal_(1.0 if kind == "gcn" else 0.0)
    deg = A.sum(1)
    if kind == "gcn":
        d = deg.pow(-0.5)
        return d[:, None] * A.T * d[None, :]
    return A / torch.where(deg == 0, torch.ones_like(deg), deg)[:, None]


class HessianReference:
    def __init__(self, kind, P, X, dims, act="relu", likelihood="classification"):
        """``dims`` = [F, (H,) C]: one or two layers; ``P`` dense [N, N]."""
        assert kind in ("gcn", "sage") and act in ("relu", "tanh") and likelihood in ("classification", "regression")
        assert len(dims) in (2, 3)
        self.kind, self.act, self.likelihood = kind, act, likelihood
        self.P, self.X = torch.as_tensor(P).detach().cpu().to(F64), torch.as_tensor(X).detach().cpu().to(F64)
        self.dims, self.L = [int(d) for d in dims], len(dims) - 1
        mult = 2 if kind == "sage" else 1
        self.shapes = [(self.dims[l + 1], mult * self.dims[l]) for l in range(self.L)]
        self.n_params = sum(o * i + o for o, i in self.shapes)

    @staticmethod
    def flatten(weights, biases):
        return torch.cat([t.detach().cpu().to(F64).reshape(-1) for pair in zip(weights, biases) for t in pair])

    def unflatten(self, theta):
        out, p = [], 0
        for o, i in self.shapes:
            out.append((theta[p:p + o * i].reshape(o, i), theta[p + o * i:p + o * i + o]))
            p += o * i + o
        return out

    def _layer(self, h, W, b):
        if self.kind == "gcn":
            return self.P @ (h @ W.T + b)
        return torch.cat([h, self.P @ h], dim=1) @ W.T + b

    def preactivation(self, theta):
        """s [N, H]: what the activation of a two-layer model sees."""
        assert self.L == 2
        W, b = self.unflatten(theta)[0]
        return self._layer(self.X, W, b)

    def min_abs_preactivation(self, theta):
        return float(self.preactivation(theta).abs().min())

    def logits(self, theta):
        """[N, C] at all nodes."""
        h = self.X
        for l, (W, b) in enumerate(self.unflatten(theta)):
            h = self._layer(h, W, b)
            if l < self.L - 1:
                h = torch.relu(h) if self.act == "relu" else torch.tanh(h)
        return h

    def _targets(self, y):
        y = torch.as_tensor(y).detach().cpu()
        return y.to(F64) if self.likelihood == "regression" else y.long()

    def loss(self, theta, idx, y):
        f = self.logits(theta)[torch.as_tensor(idx).cpu().long()]
        if self.likelihood == "regression":
            return 0.5 * ((f - self._targets(y).reshape(f.shape)) ** 2).sum()
        return torch.nn.functional.cross_entropy(f, self._targets(y), reduction="sum")

    def residual(self, theta, idx, y):
        """r [M, C], no graph."""
        f = self.logits(theta.detach())[torch.as_tensor(idx).cpu().long()]
        if self.likelihood == "regression":
            return f - self._targets(y).reshape(f.shape)
        return torch.softmax(f, dim=-1) - torch.nn.functional.one_hot(self._targets(y), f.shape[1]).to(F64)

    def _resid_scalar(self, theta, idx, y):
        """``sum_nc r_nc f_nc(theta)`` with r held fixed: its Hessian is R."""
        return (self.residual(theta, idx, y) * self.logits(theta)[torch.as_tensor(idx).cpu().long()]).sum()

    @staticmethod
    def _vhp(fn, theta, V):
        """``V @ (grad^2 fn)(theta)`` [k, P] by double backward, one pass per row of V."""
        theta = theta.detach().clone().requires_grad_(True)
        (g,) = torch.autograd.grad(fn(theta), theta, create_graph=True)
        rows = []
        for v in torch.as_tensor(V).detach().cpu().to(F64):
            if not g.requires_grad:  # a model that is linear in theta
                rows.append(torch.zeros_like(theta))
                continue
            (hv,) = torch.autograd.grad(g, theta, v, retain_graph=True, allow_unused=True)
            rows.append(torch.zeros_like(theta) if hv is None else hv)
        return torch.stack(rows).detach()

    def hvp(self, theta, idx, y, V):
        """``V @ H`` for the exact Hessian of the loss."""
        return self._vhp(lambda t: self.loss(t, idx, y), theta, V)

    def resid_vp(self, theta, idx, y, V):
        """``V @ R``."""
        return self._vhp(lambda t: self._resid_scalar(t, idx, y), theta, V)

    def dense(self, theta, idx, y):
        """H [P, P] (small P)."""
        return self.hvp(theta, idx, y, torch.eye(self.n_params, dtype=F64))

    def dense_resid(self, theta, idx, y):
        return self.resid_vp(theta, idx, y, torch.eye(self.n_params, dtype=F64))

    def jacobians(self, theta, idx):
        """[M, C, P] of the logits at ``idx``."""
        idx = torch.as_tensor(idx).cpu().long()
        J = torch.autograd.functional.jacobian(lambda t: self.logits(t)[idx], theta.detach(), vectorize=True)
        return J.detach()

    def dense_ggn(self, theta, idx, y=None):
        J = self.jacobians(theta, idx)
        if self.likelihood == "regression":
            return torch.einsum("ncp,ncq->pq", J, J)
        p = torch.softmax(self.logits(theta.detach())[torch.as_tensor(idx).cpu().long()], dim=-1)
        Lam = torch.diag_embed(p) - p.unsqueeze(2) * p.unsqueeze(1)
        return torch.einsum("ncp,nck,nkq->pq", J, Lam, J)

    def split(self, theta, idx, y):
        """(GGN, R), each [P, P] and each from its own definition; ``GGN + R`` is ``dense``."""
        return self.dense_ggn(theta, idx, y), self.dense_resid(theta, idx, y)
