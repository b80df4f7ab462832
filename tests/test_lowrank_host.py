"""Host-side checks of the low-rank Laplace: the factory, the C ABI of the two block products and the eigensolver's block-size,
stopping and masking logic on dense fp64 matrices through a stub product (no GPU)."""
import os
import re

import pytest
import torch

import laplace_gnn_amd as lg
from laplace_gnn_amd import lowrank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_factory_resolves_the_lowrank_key():
    X = torch.randn(12, 4, generator=torch.Generator().manual_seed(0))
    ei = torch.randint(0, 12, (2, 30), generator=torch.Generator().manual_seed(1))
    m = lg.GCN(4, 3, 2, 2, X, ei)
    la = lg.Laplace(m, "classification", subset_of_weights="all", hessian_structure="lowrank",
                    backend_kwargs={"low_rank": 4})
    assert type(la) is lg.LowRankLaplace and la._key == ("all", "lowrank")
    assert la._backend_cls is lg.HipGGN and la._backend_kwargs == {"low_rank": 4}
    with pytest.raises(AttributeError, match="not fit"):
        la.posterior_precision
    with pytest.raises(ValueError, match="LowRank LA does not support updating."):
        la.fit([], override=False)


def test_an_engine_without_the_block_product_is_refused_at_construction():
    class Engine:  # a stand-in engine that offers no ggn_matmat_
        pass

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(3, 2)
            self.engine = Engine()

    with pytest.raises(NotImplementedError, match="ggn_matmat_"):
        lg.Laplace(Model(), "classification", "all", "lowrank")
    with pytest.raises(NotImplementedError, match="outside the accelerated path"):
        lg.Laplace(Model(), "classification", "last_layer", "lowrank")


def _c_args(decl):
    inner = decl[decl.index("(") + 1:decl.rindex(")")]
    return [a for a in re.sub(r"/\*.*?\*/", "", inner, flags=re.S).split(",") if a.strip()]


@pytest.mark.parametrize("name", ["lgnn_jvp_block", "lgnn_ggn_matmat", "lgnn_block_gram"])
def test_header_declares_the_entry_points_and_the_binding_matches(name):
    text = open(os.path.join(ROOT, "include", "laplace_gnn_hip.h")).read()
    m = re.search(r"LGNN_API int " + name + r"\s*\([^;]*\);", text)
    assert m, f"{name} is not declared in the header"
    res, args = lg._lib.SIGNATURES[name]
    assert len(args) == len(_c_args(m.group(0))), (name, m.group(0))
    src = open(os.path.join(ROOT, "laplace-gnn_amd", "csrc", "ggnmat.hip")).read()
    d = re.search(r'extern "C" int ' + name + r"\s*\([^{]*\)\s*\{", src)
    assert d and len(_c_args(d.group(0))) == len(args)
    assert "LGNN_GGN_FROM_JACOBIANS" in text and lg._lib.GGN_FROM_JACOBIANS == 1
    assert "atomicAdd" not in src  # every output element has one writer


def test_block_size_budget_and_masks():
    assert lowrank.block_size(10, 43_000) == 18 and lowrank.block_size(32, 195) == 40 and lowrank.block_size(64, 10_000) == 80
    assert lowrank.block_size(10, 12) == 12 and lowrank.block_size(1, 5) == 5
    with pytest.raises(ValueError):
        lowrank.block_size(0, 5)
    assert lowrank.default_max_iters(10) == 100
    theta = torch.tensor([5.0, 1.0, 2e-6, 1e-6, 1e-9, -1e-12], dtype=torch.float64)
    assert lowrank.mask_pairs(theta, 5).tolist() == [0, 1, 2]  # strictly above EPS, among the K leading pairs
    assert lowrank.mask_pairs(theta, 1).tolist() == [0]
    res = torch.tensor([4e-4, 6e-4, 1.0], dtype=torch.float64)
    assert lowrank.stop_rule(theta, res, 2, 1.2e-4) and not lowrank.stop_rule(theta, res, 2, 1e-4)
    assert not lowrank.stop_rule(theta, res, 3, 1.2e-4)  # the K leading pairs, not fewer
    a, b = lowrank.start_block(4, 9, 0, "cpu"), lowrank.start_block(4, 9, 0, "cpu")
    state = torch.random.get_rng_state()
    assert torch.equal(a, b) and not torch.equal(a, lowrank.start_block(4, 9, 1, "cpu"))
    assert torch.equal(state, torch.random.get_rng_state())  # the global generator is not touched


def _dense(eigs, seed=3):
    P = len(eigs)
    Qm, _ = torch.linalg.qr(torch.randn(P, P, dtype=torch.float64, generator=torch.Generator().manual_seed(seed)))
    return (Qm * torch.tensor(eigs, dtype=torch.float64)) @ Qm.T


def _solve(H, K, **kw):
    calls = []

    def matmat(Q):
        calls.append(Q.shape)
        return Q @ H

    r = lowrank.subspace_eig(matmat, H.shape[0], K, "cpu", dtype=torch.float64, **kw)
    assert r.n_sweeps == len(calls) and all(s == (lowrank.block_size(K, H.shape[0]), H.shape[0]) for s in calls)
    return r


def test_solver_on_a_matrix_with_a_repeated_eigenvalue():
    eigs = [9.0, 4.0, 4.0, 4.0, 2.5, 1.0] + [0.5 * 0.9 ** i for i in range(54)]
    H = _dense(eigs)
    r = _solve(H, 5, tol=1e-9)
    assert r.converged and r.n_sweeps < 50 and r.eigenvectors.shape == (60, 5)
    assert torch.allclose(r.eigenvalues, torch.tensor(eigs[:5], dtype=torch.float64), atol=1e-12 * 9 + 1e-14, rtol=0) or \
        float((r.eigenvalues - torch.tensor(eigs[:5], dtype=torch.float64)).abs().max()) <= 1e-12
    U = r.eigenvectors
    assert float((U.T @ U - torch.eye(5, dtype=torch.float64)).abs().max()) <= 1e-12
    res = torch.linalg.vector_norm(H @ U - U * r.eigenvalues, dim=0)
    assert float(res.max()) <= 1e-9 * 9.0 and torch.allclose(res, r.residuals, atol=1e-12)
    again = _solve(H, 5, tol=1e-9)
    assert torch.equal(again.eigenvectors, U) and again.n_sweeps == r.n_sweeps
    other = _solve(H, 5, tol=1e-9, seed=7)
    assert float((other.eigenvalues - r.eigenvalues).abs().max()) <= 1e-12


def test_solver_on_a_matrix_of_rank_below_K():
    H = _dense([3.0, 2.0, 0.7] + [0.0] * 37)
    r = _solve(H, 8)  # default tolerance
    assert r.converged and r.n_sweeps <= 2
    assert r.eigenvectors.shape == (40, 3)  # the pairs below EPS are masked out
    assert float((r.eigenvalues - torch.tensor([3.0, 2.0, 0.7], dtype=torch.float64)).abs().max()) <= 1e-12
    U = r.eigenvectors
    assert float((U @ torch.diag(r.eigenvalues) @ U.T - H).abs().max()) <= 1e-12


def test_solver_stops_at_the_sweep_budget():
    H = _dense([1.0 + 1e-3 * i for i in range(50)][::-1])  # no gap: no convergence in three sweeps
    r = _solve(H, 4, tol=1e-12, max_iters=3)
    assert not r.converged and r.n_sweeps == 3 and r.eigenvectors.shape == (50, 4)
