"""CPU tests of ``predictive_samples`` (laplace/baselaplace.py:1074-1120) and of ``_nn_predictive_samples`` (:1160-1181) on
the fronts, with the injected oracle backend: no device route exists there, so the per-sample loop runs."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle_backend import OracleBackend
from test_host_logic import _cpu_model

import laplace_gnn_amd as lg

NAMES = ["gcn_small_1batch_s0", "sage_small_3batch_s1"]


def _setup(name, likelihood="classification", y_key="train_y"):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    model = _cpu_model(g)
    loader = lg.TensorBatchLoader(torch.from_numpy(g["train_idx"]), torch.from_numpy(g[y_key]), int(g["batch_size"]))
    return g, model, loader


def test_every_parametric_front_has_predictive_samples():
    for cls in (lg.KronLaplace, lg.DiagLaplace, lg.FullLaplace, lg.FullLLLaplace, lg.KronLLLaplace, lg.DiagLLLaplace):
        assert callable(getattr(cls, "predictive_samples")), cls
        assert callable(getattr(cls, "_nn_predictive_samples")), cls


@pytest.mark.parametrize("name", NAMES)
def test_nn_samples_are_what_the_call_averages(name):
    g, model, loader = _setup(name)
    eps, idx = torch.from_numpy(g["pred_eps"]), torch.from_numpy(g["pred_idx"])
    before = [p.detach().clone() for p in model.parameters()]
    for structure in ("kron", "diag"):
        la = lg.Laplace(model, "classification", "all", structure, backend=OracleBackend)
        la.fit(loader)
        assert not la._nn_device_route()
        ps = la.predictive_samples(idx, pred_type="nn", n_samples=len(eps), eps=eps)
        assert ps.shape == (len(eps), len(idx), la.n_outputs)
        assert torch.allclose(ps.sum(-1), torch.ones(len(eps), len(idx)), atol=1e-5)
        py = la(idx, pred_type="nn", link_approx="mc", n_samples=len(eps), eps=eps)
        assert (ps.mean(0) - py).abs().max() < 1e-6
        assert np.abs(ps.mean(0).numpy() - g[structure + "_nn_py"]).max() < 2e-5
        for p, b in zip(model.parameters(), before):
            assert torch.equal(p.detach(), b) and p.data_ptr() != la.mean.data_ptr()
        # the reduction over chunks of samples gives the same mean
        la._NN_CHUNK_FLOATS = 3 * len(idx) * la.n_outputs
        py_chunked = la(idx, pred_type="nn", link_approx="mc", n_samples=len(eps), eps=eps)
        assert (py_chunked - py).abs().max() < 1e-6
        # generator path: reproducible
        a = la.predictive_samples(idx, "nn", n_samples=5, generator=torch.Generator().manual_seed(1))
        b = la.predictive_samples(idx, "nn", n_samples=5, generator=torch.Generator().manual_seed(1))
        assert a.shape[0] == 5 and torch.equal(a, b)


def test_full_posterior_nn_samples():
    g, model, loader = _setup("gcn_small_1batch_s0")
    eps, idx = torch.from_numpy(g["pred_eps"]), torch.from_numpy(g["pred_idx"])
    la = lg.Laplace(model, "classification", "all", "full", backend=OracleBackend)
    la.fit(loader)
    ps = la.predictive_samples(idx, "nn", n_samples=len(eps), eps=eps)
    assert ps.shape == (len(eps), len(idx), la.n_outputs)
    assert (ps.mean(0) - la(idx, pred_type="nn", link_approx="mc", eps=eps)).abs().max() < 1e-6


@pytest.mark.parametrize("name", NAMES)
def test_glm_samples_come_from_the_glm_predictive_distribution(name):
    g, model, loader = _setup(name)
    idx, eps = torch.from_numpy(g["pred_idx"]), torch.from_numpy(g["glm_eps"])
    for structure in ("kron", "diag"):
        la = lg.Laplace(model, "classification", "all", structure, backend=OracleBackend)
        la.fit(loader)
        f_mu, f_var = la._glm_predictive_distribution(idx)
        n = eps.shape[1]
        got = la.predictive_samples(idx, n_samples=n, eps=eps)  # pred_type defaults to "glm"
        assert got.shape == (n, len(idx), la.n_outputs)
        assert torch.allclose(got, la._glm_predictive_samples(f_mu, f_var, n, False, None, eps), atol=1e-6)
        got_d = la.predictive_samples(idx, "glm", n_samples=n, diagonal_output=True, eps=eps)
        want_d = la._glm_predictive_samples(f_mu, torch.diagonal(f_var, dim1=1, dim2=2), n, False, None, eps)
        assert torch.allclose(got_d, want_d, atol=1e-6)
        assert not torch.allclose(got_d, got, atol=1e-4)  # the off-diagonal entries are not read
        # the mean of the samples is the mc link of the GLM predictive
        assert (got.mean(0) - la(idx, pred_type="glm", link_approx="mc", n_samples=n, eps=eps)).abs().max() < 1e-6
        with pytest.raises(ValueError):
            la.predictive_samples(idx, pred_type="gp")


def test_regression_samples_and_chunked_moments():
    g, model, loader = _setup("gcn_small_1batch_s0", "regression", "reg_y")
    idx = torch.from_numpy(g["pred_idx"])
    la = lg.Laplace(model, "regression", "all", "diag", backend=OracleBackend, sigma_noise=0.7)
    la.fit(loader)
    C = la.n_outputs
    eps = torch.randn(9, la.n_params, generator=torch.Generator().manual_seed(0))
    fs = la.predictive_samples(idx, "nn", n_samples=9, eps=eps)
    assert fs.shape == (9, len(idx), C)
    assert (fs.sum(-1) - 1).abs().max() > 1e-3  # the outputs themselves, no softmax
    mean, var = la(idx, pred_type="nn", link_approx="mc", n_samples=9, eps=eps)
    assert torch.allclose(mean, fs.mean(0), atol=1e-6) and torch.allclose(var, fs.var(0), rtol=1e-5, atol=1e-8)
    la._NN_CHUNK_FLOATS = 2 * len(idx) * C  # chunks of two samples, the last of one
    mean_c, var_c = la(idx, pred_type="nn", link_approx="mc", n_samples=9, eps=eps)
    assert torch.allclose(mean_c, fs.mean(0), atol=1e-6)
    assert torch.allclose(var_c, fs.double().var(0).float(), rtol=1e-4, atol=1e-8)
    # "glm": samples of N(f_mu, f_var), no link
    f_mu, f_var = la._glm_predictive_distribution(idx)
    geps = torch.randn(C, 6, generator=torch.Generator().manual_seed(1))
    gs = la.predictive_samples(idx, "glm", n_samples=6, eps=geps)
    assert gs.shape == (6, len(idx), C)
    want = f_mu.unsqueeze(0) + torch.einsum("mck,ks->smc", torch.linalg.cholesky(f_var), geps)
    assert torch.allclose(gs, want, atol=1e-5)
