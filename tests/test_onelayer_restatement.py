"""Pins tests/onelayer_restatement.py, the fp64 autograd yardstick of the one-layer adjacency gradient, to the reference: under
each log determinant ("diag", "kron", "full") it must reproduce the reference's own ``model.adj.grad`` goldens of a one-layer
STE-GCN (tests/golden/onelayer/one1_*.npz: value, stored entries, the 200 non-edges) and the fitted curvature (the full GGN
``H``, its diagonal, the Kronecker factors).  The goldens are what the reference computes in fp32; measured on the CPU over
the four cases: value <= 1.5e-7, curvature <= 1.8e-7, gradients of the diagonal and Kronecker posteriors <= 2.5e-7 -- held at
1e-6, the bar of tests/test_adjgrad_restatement.py.  The full posterior's gradient (the reference inverts H + delta in fp32
in its backward pass) measures <= 6.3e-7 on the stored entries and 1.05e-6 on the non-edges of one1_f2c2_dir_1batch
(<= 2.8e-7 on the other three cases): the fp32 goldens cannot support 1e-6 there, so the full posterior's two gradient
comparisons are held at 2.1e-6, twice the measured worst case."""
import glob
import os

import numpy as np
import pytest
import torch

import onelayer_restatement as R
from conftest import GOLDEN

CASES = sorted(glob.glob(os.path.join(GOLDEN, "onelayer", "one1_*.npz")))
TOL = 1e-6
TOL_FULL_GRAD = 2.1e-6  # 2 x the measured worst case (module docstring)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def spec(g):
    return dict(num_nodes=int(g["num_nodes"]), X=g["X"], W=g["W0"], b=g["b0"], symmetric=bool(g["symmetric"]),
                batch_size=int(g["batch_size"]))


def test_the_four_gradient_cases_are_present():
    assert len(CASES) == 4


@pytest.mark.parametrize("logdet", ["diag", "kron", "full"])
@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[:-4] for p in CASES])
def test_restatement_reproduces_the_reference_goldens(path, logdet):
    g = np.load(path)
    val, gA, H = R.neg_marglik_adj_grad(g["adj_nz_row"], g["adj_nz_col"], g["train_idx"], g["train_y"], float(g["prior"]), logdet,
                                        **spec(g))
    ref = float(g[f"{logdet}_neg_marglik"])
    e_val = abs(val - ref) / abs(ref)
    e_st = rel(gA[g["adj_nz_row"], g["adj_nz_col"]], g[f"{logdet}_vals"])
    e_ne = rel(gA[g["ne_row"], g["ne_col"]], g[f"{logdet}_ne_val"])
    if logdet == "kron":
        assert int(g["kron_n_blocks"]) == 2  # one weight block (B, A), one bias block (B)
        e_h = max(rel(H[0], g["kron_0_0"]), rel(H[1], g["kron_0_1"]), rel(H[0], g["kron_1_0"]))
    elif logdet == "diag":
        e_h = rel(np.diagonal(H), g["diag_H"])
    else:
        e_h = rel(H, g["full_H"])
    print(f"{logdet}: value {e_val:.2e}  stored {e_st:.2e}  non-edges {e_ne:.2e}  curvature {e_h:.2e}")
    tol_g = TOL_FULL_GRAD if logdet == "full" else TOL
    assert e_val <= TOL and e_st < tol_g and e_ne < tol_g and e_h < TOL
    assert np.count_nonzero(g[f"{logdet}_ne_val"]) > 100  # the reference's adj.grad is dense


def test_closed_form_jacobian_is_the_autograd_jacobian():
    g = np.load(CASES[0])
    N = int(g["num_nodes"])
    A = torch.zeros(N, N, dtype=torch.float64)
    A[torch.from_numpy(g["adj_nz_row"]), torch.from_numpy(g["adj_nz_col"])] = 1.0
    P = R.propagation(A, bool(g["symmetric"]))
    X, W, b = R._t(g["X"]), R._t(g["W0"]), R._t(g["b0"])
    idx = torch.from_numpy(g["train_idx"])
    JW, Jb = torch.autograd.functional.jacobian(lambda w, bb: R.forward(P, X, w, bb)[idx], (W, b))
    J = torch.cat([JW.reshape(idx.shape[0], W.shape[0], -1), Jb], 2)
    assert torch.allclose(J, R.closed_form_jacobians(P, X, idx, W.shape[0]), rtol=0, atol=1e-14)
    assert torch.allclose(R.forward(P, X, W, b), R._t(g["logits"]), atol=1e-5)


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[:-4] for p in CASES])
def test_diagonal_formulas_are_the_full_formulas_with_a_diagonal_gamma(path):
    """G_ck = delta_ck diag(Gamma_c): the full posterior's per-sample pbar / ebar collapse to the diagonal posterior's."""
    g = np.load(path)
    N = int(g["num_nodes"])
    A = torch.zeros(N, N, dtype=torch.float64)
    A[torch.from_numpy(g["adj_nz_row"]), torch.from_numpy(g["adj_nz_col"])] = 1.0
    P = R.propagation(A, bool(g["symmetric"])).numpy()
    gamma = 0.5 / (g["diag_H"].astype(np.float64) + float(g["prior"]))
    pd, ed = R.diag_formulas(P, g["X"], g["train_idx"], g["W0"], g["b0"], gamma)
    pf, ef = R.full_from_blocks(P, g["X"], g["train_idx"], g["W0"], g["b0"], np.diag(gamma))
    assert rel(pd, pf) < 1e-13 and rel(ed, ef) < 1e-13
    assert np.abs(ed).max() > 0
