"""``lg.FunctionalLaplace`` on the CPU: the front over backends without ``gp_kernel`` (the einsum route from
``backend.jacobians``) against the reference's own FunctionalLaplace (tests/golden/gp, tools/make_gp_golden.py), the subset
order, the layout of K_MM, the factory key, the refusals, the prior-change flag and the marginal likelihood's gradient."""
import warnings

import numpy as np
import pytest
import torch

from gp_utils import GP_CASES, PREFIXES, ActBackend, gp_golden, gp_loader, gp_model, rel
from oracle_backend import CpuForwardGCN, OracleBackend

import laplace_gnn_amd as lg

RTOL = 1e-4      # fp32 parity with the reference
MARGLIK_RTOL = 3e-4  # as the other posteriors' marginal-likelihood tests


def _front(case, prefix, **kw):
    g = gp_golden(case)
    model = gp_model(g)
    # the CPU oracle behind OracleBackend is ReLU only: the tanh case takes the fp64 autograd helper
    if str(g["act"]) == "relu":
        model, backend = CpuForwardGCN(model), OracleBackend
    else:
        backend = ActBackend
    la = lg.Laplace(model, str(g["likelihood"]), "all", "gp", n_subset=int(g["n_subset"]), backend=backend,
                    independent_outputs=prefix == "indep", prior_precision=float(g["prior"]), **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        la.fit(gp_loader(g))
    return g, la


@pytest.mark.parametrize("prefix", PREFIXES)
@pytest.mark.parametrize("case", GP_CASES)
def test_front_matches_the_reference(case, prefix):
    g, la = _front(case, prefix)
    k = prefix + "_"
    M, C = int(g["n_subset"]), la.n_outputs
    assert isinstance(la, lg.FunctionalLaplace) and not la._on_device
    assert np.array_equal(la.subset_order, g[k + "order"])
    assert la.n_data == len(g["train_idx"]) and la._prior_factor_sod == M / len(g["train_idx"])
    if prefix == "indep":
        K, L = torch.stack(la.K_MM).numpy(), torch.stack(la.L).numpy()
        assert K.shape == (C, M, M)
    else:
        K, L = la.K_MM.numpy(), la.L.numpy()
        assert K.shape == (M * C, M * C)
    errs = {"K_MM": rel(K, g[k + "K_MM"]), "L": rel(L, g[k + "L"]), "mu": rel(la.mu.numpy(), g[k + "mu"]),
            "loss": abs(float(la.loss) - float(g[k + "loss"])) / abs(float(g[k + "loss"])),
            "log_det_ratio": abs(float(la.log_det_ratio) - float(g[k + "log_det_ratio"])) / abs(float(g[k + "log_det_ratio"])),
            "scatter": abs(float(la.scatter) - float(g[k + "scatter"])) / abs(float(g[k + "scatter"]))}
    m07 = float(la.log_marginal_likelihood())
    m3 = float(la.log_marginal_likelihood(prior_precision=torch.tensor(float(g["prior2"]))))
    e07 = abs(m07 - float(g[k + "marglik_pp07"])) / abs(float(g[k + "marglik_pp07"]))
    e3 = abs(m3 - float(g[k + "marglik_pp3"])) / abs(float(g[k + "marglik_pp3"]))
    assert la._recompute_Sigma
    la.prior_precision = float(g["prior"])
    la._build_Sigma_inv()
    pred = torch.from_numpy(g["pred_idx"])
    f_mu, f_var = la._glm_predictive_distribution(pred)
    errs["f_mu"], errs["f_var"] = rel(f_mu.numpy(), g[k + "f_mu"]), rel(f_var.numpy(), g[k + "f_var"])
    if prefix == "full":
        mu_j, cov = la._glm_predictive_distribution(pred, joint=True)
        assert tuple(cov.shape) == (9 * C, 9 * C) and tuple(mu_j.shape) == (9 * C,)
        errs["joint_cov"] = rel(cov.numpy(), g[k + "joint_cov"])
    else:
        with pytest.raises(NotImplementedError, match="joint"):
            la._glm_predictive_distribution(pred, joint=True)
    if str(g["likelihood"]) == "classification":
        errs["probit"] = float(np.abs(la(pred).numpy() - g[k + "probit"]).max())
        mc = la(pred, link_approx="mc", n_samples=32, eps=torch.from_numpy(g[k + "eps"]).to(f_mu.dtype))
        errs["mc"] = float(np.abs(mc.numpy() - g[k + "mc"]).max())
        for link in ("bridge", "bridge_norm"):
            probs = la(pred, link_approx=link)
            assert torch.allclose(probs.sum(-1), torch.ones(9, dtype=probs.dtype), atol=1e-5)
    else:
        mu_r, var_r = la(pred)
        assert rel(mu_r.numpy(), g[k + "f_mu"]) < RTOL and rel(var_r.numpy(), g[k + "f_var"]) < RTOL
        assert tuple(la(pred, diagonal_output=True)[1].shape) == (9, C)
    print(f"{case} {prefix}: " + " ".join(f"{n} {v:.1e}" for n, v in errs.items()) + f" marglik {e07:.1e} {e3:.1e}")
    for n, v in errs.items():
        assert v < RTOL, (n, v)
    assert e07 < MARGLIK_RTOL and e3 < MARGLIK_RTOL


def test_subset_order_is_the_numpy_generator_draw():
    # np.random.default_rng(0).choice(list(range(40)), 17, replace=False), worked out once with numpy alone
    want = [15, 13, 2, 1, 25, 31, 18, 8, 0, 36, 20, 28, 22, 7, 37, 5, 26]
    from laplace_gnn_amd.gp import sod_order

    assert sod_order(40, 17, 0).tolist() == want
    g, la = _front("gcn_small", "full")
    assert la.subset_order.tolist() == want
    batches = list(la.train_loader)
    assert [len(b[0]) for b in batches] == [7, 7, 3]
    assert torch.equal(torch.cat([b[0] for b in batches]), torch.from_numpy(g["train_idx"])[want])
    assert torch.equal(torch.cat([b[1] for b in batches]), torch.from_numpy(g["train_y"])[want])
    assert sod_order(40, 17, 1).tolist() != want


@pytest.mark.parametrize("independent", [False, True])
def test_store_K_batch_layout_with_a_ragged_last_batch(independent):
    g = gp_golden("gcn_small")
    la = lg.FunctionalLaplace(gp_model(g), "classification", n_subset=5, backend=ActBackend, independent_outputs=independent)
    la.n_outputs, la.batch_size, C = 2, 2, 2
    sizes = [2, 2, 1]
    la._init_K_MM(torch.zeros(1))
    gen = torch.Generator().manual_seed(0)
    blocks = {}
    for i in range(3):
        for j in range(i, 3):
            shape = (sizes[i], sizes[j], C) if independent else (sizes[i] * C, sizes[j] * C)
            blocks[i, j] = torch.randn(shape, generator=gen)
            la._store_K_batch(blocks[i, j], i, j)
    off = [0, 2, 4, 5]
    for (i, j), B in blocks.items():
        if independent:
            for c in range(C):
                assert torch.equal(la.K_MM[c][off[i]:off[i + 1], off[j]:off[j + 1]], B[:, :, c])
                assert torch.equal(la.K_MM[c][off[j]:off[j + 1], off[i]:off[i + 1]], B[:, :, c].T) or i == j
        else:
            assert torch.equal(la.K_MM[off[i] * C:off[i + 1] * C, off[j] * C:off[j + 1] * C], B)
            assert torch.equal(la.K_MM[off[j] * C:off[j + 1] * C, off[i] * C:off[i + 1] * C], B.T) or i == j


def test_factory_key_and_refusals():
    g = gp_golden("gcn_small")
    model = gp_model(g)
    la = lg.Laplace(model, "classification", "all", "gp", n_subset=17)
    assert type(la) is lg.FunctionalLaplace and lg.FunctionalLaplace._key == ("all", "gp")
    assert la._backend_cls is lg.HipGGN and la.n_subset == 17 and la.independent_outputs is False
    with pytest.raises(NotImplementedError, match="FunctionalLLLaplace"):
        lg.Laplace(model, "classification", "last_layer", "gp", n_subset=17)
    with pytest.raises(ValueError, match="isotropic"):
        lg.FunctionalLaplace(model, "classification", n_subset=17, prior_precision=torch.ones(3))
    with pytest.raises(NotImplementedError, match="enable_backprop"):
        lg.FunctionalLaplace(model, "classification", n_subset=17, enable_backprop=True)
    with pytest.raises(NotImplementedError, match="process_group"):
        la.fit(gp_loader(g), process_group=object())
    with pytest.raises(ValueError, match="n_subset"):
        lg.FunctionalLaplace(model, "classification", n_subset=41, backend=ActBackend).fit(gp_loader(g))
    with pytest.raises(RuntimeError, match="not been fitted"):
        la(torch.arange(3))
    _, fitted = _front("gcn_small", "full")
    pred = torch.from_numpy(g["pred_idx"])
    with pytest.raises(ValueError, match="Only gp"):
        fitted(pred, pred_type="glm")
    with pytest.raises(ValueError, match="link approximation"):
        fitted(pred, link_approx="softmax")
    with pytest.raises(ValueError, match="isotropic"):
        fitted.prior_precision = torch.ones(fitted.n_params)
    with pytest.raises(NotImplementedError, match="neg_marglik_adj_grad"):
        fitted.neg_marglik_adj_grad(gp_loader(g))
    with pytest.raises(NotImplementedError, match="state_dict"):
        fitted.state_dict()
    with pytest.raises(NotImplementedError, match="state_dict"):
        fitted.load_state_dict({})
    with pytest.raises(NotImplementedError, match="gridsearch"):
        fitted.optimize_prior_precision(method="gridsearch")
    with pytest.raises(ValueError, match="isotropic"):
        fitted.optimize_prior_precision(prior_structure="diag")
    with pytest.raises(ValueError, match="sigma_noise"):
        fitted.log_marginal_likelihood(sigma_noise=torch.tensor(0.5))


def test_hip_backend_refuses_what_it_cannot_serve_by_name():
    model = CpuForwardGCN(gp_model(gp_golden("gcn_small")))
    x = torch.arange(3)
    for kw, name in ((dict(subnetwork_indices=torch.arange(4)), "subnetwork_indices"), (dict(last_layer=True), "last_layer"),
                     (dict(stochastic=True), "stochastic")):
        be = lg.HipGGN(model, "classification", **kw)
        with pytest.raises(NotImplementedError, match=name):
            be.gp_kernel(x, x)
        with pytest.raises(NotImplementedError, match=name):
            be.gp_jvp(x, torch.zeros(1))


def test_prior_change_asks_for_a_new_cholesky_factor():
    g, la = _front("gcn_small", "full")
    assert la._fitted and not la._recompute_Sigma
    S07 = la.Sigma_inv.clone()
    pred = torch.from_numpy(g["pred_idx"])
    p07 = la(pred)
    la.prior_precision = 3.0
    assert la._recompute_Sigma and torch.equal(la.Sigma_inv, S07)
    with pytest.warns(UserWarning, match="prior precision has been changed"):
        p3 = la(pred)
    assert not la._recompute_Sigma and not torch.allclose(la.Sigma_inv, S07)
    want = torch.linalg.cholesky(la.gp_kernel_prior_variance * la.K_MM + torch.diag(1.0 / la.L))
    assert torch.allclose(la.Sigma_inv, want, rtol=1e-10, atol=0)
    assert float((p3 - p07).abs().max()) > 1e-4


@pytest.mark.parametrize("case,prefix", [("gcn_small", "full"), ("sage_small", "indep"), ("gcn_regression", "full")])
def test_marginal_likelihood_gradient_against_a_central_difference(case, prefix):
    _, la = _front(case, prefix)
    regression = la.likelihood == "regression"
    # the fitted quantities in fp64 (the oracle backend's Jacobians are fp32): the difference quotient's own error is then its
    # truncation term, ~h^2 = 1e-8, and the bound 1e-6 checks the derivative, not the rounding of the value
    f64 = lambda t: [x.double() for x in t] if isinstance(t, list) else t.double()  # noqa: E731
    la.K_MM, la.L, la.mu, la.loss = f64(la.K_MM), f64(la.L), f64(la.mu), la.loss.double()

    def value(log_pp, log_sn=None):
        kw = dict(sigma_noise=log_sn.exp()) if log_sn is not None else {}
        return la.log_marginal_likelihood(prior_precision=log_pp.exp(), **kw)

    lp = torch.tensor([0.3], dtype=torch.float64, requires_grad=True)
    ls = torch.tensor(-0.2, dtype=torch.float64, requires_grad=True) if regression else None
    value(lp, ls).backward()
    h = 1e-4
    with torch.no_grad():
        fd = (value(lp + h, ls) - value(lp - h, ls)) / (2 * h)
    assert abs(float(lp.grad) - float(fd)) < 1e-6 * max(1.0, abs(float(fd))), (float(lp.grad), float(fd))
    if regression:
        with torch.no_grad():
            fd_s = (value(lp, ls + h) - value(lp, ls - h)) / (2 * h)
        assert abs(float(ls.grad) - float(fd_s)) < 1e-6 * max(1.0, abs(float(fd_s))), (float(ls.grad), float(fd_s))


def test_optimize_prior_precision_lowers_the_negative_marginal_likelihood():
    _, la = _front("gcn_small", "full")
    before = -float(la.log_marginal_likelihood(prior_precision=torch.tensor(1.0)))
    la.optimize_prior_precision(method="marglik", n_steps=30, lr=0.1, init_prior_prec=1.0)
    assert not la._recompute_Sigma  # the factor was rebuilt for the value found
    after = -float(la.log_marginal_likelihood())
    pp = la.prior_precision
    assert pp.numel() == 1 and not pp.requires_grad and after < before
    want = torch.linalg.cholesky(la.gp_kernel_prior_variance * la.K_MM + torch.diag(1.0 / la.L))
    assert torch.allclose(la.Sigma_inv, want, rtol=1e-10, atol=0)
