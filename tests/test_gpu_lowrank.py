"""``HipGGN.eig_lowrank`` and ``lg.LowRankLaplace`` on the GPU against the dense fp64 GGN of tests/lowrank_utils.py.

Models: the 2-layer relu GCN at (N, F, H, C) = (96, 13, 10, 5), P = 195, and (300, 37, 64, 7), P = 2 887; train set: 60 ids in two
batches (37 + 23) with the hub, both isolated nodes and a repeated id.

fp32 floor of the residual, measured WITHOUT the solver (exact fp64 eigenvectors of H64 rounded to fp32, then
``max_i ||J32^T Lambda32 (J32 v_i) - l_i v_i|| / l_1`` over the ten leading pairs with torch fp32 on ``engine.jacobians``):
    P = 195:   2.40e-7   (l_1 = 27.5, l_10 = 0.885, l_19 = 0.386)
    P = 2 887: 7.98e-8   (l_1 = 28.4, l_10 = 2.70,  l_19 = 0.984)
``lowrank.DEFAULT_TOL`` is 8 x the larger value, 1.92e-6.  The tests below pass ``tol = 1e-4`` (the project's RTOL), 2.6 orders
above the floor."""
import functools

import pytest
import torch

from lowrank_utils import H64, SHAPES, case_id, edge_model, train_batches, train_loader, train_set

pytestmark = pytest.mark.gpu

TOL = 1e-4
CASES = [("gcn", 2, "relu", s, False) for s in SHAPES]
RTOL, MARGLIK_RTOL = 1e-4, 3e-4  # tests/test_gpu_gp.py


def backend(case, **kw):
    import laplace_gnn_amd as lg

    return lg.HipGGN(edge_model(*case), "classification", **kw)


@functools.lru_cache(maxsize=None)
def solved(case, seed=0):
    """(U, l, loss, info) of ``eig_lowrank`` with K = 10, tol = 1e-4: solved once per (case, seed) and left unchanged."""
    be = backend(case, low_rank=10, lowrank_seed=seed)
    U, l, loss = be.eig_lowrank(train_loader(case[3][0], case[3][3]), tol=TOL)
    be.check_async_errors()
    return U, l, loss, be.lowrank_info


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_eig_lowrank_against_the_dense_spectrum(case):
    H = H64(case)
    U, l, loss, info = solved(case)
    top = torch.linalg.eigvalsh(H).flip(0)[:10]
    lam1 = float(top[0])
    assert U.shape == (H.shape[0], 10) and l.shape == (10,) and U.dtype == torch.float32
    e_val = float((l.double() - top).abs().max()) / lam1
    U64 = U.double()
    res64 = torch.linalg.vector_norm(H @ U64 - U64 * l.double(), dim=0)
    e_res = float(res64.max()) / lam1
    e_orth = float((U64.T @ U64 - torch.eye(10, dtype=torch.float64, device="cuda")).abs().max())
    print(f"{case_id(case)}: sweeps {info.n_sweeps} converged {info.converged} eigenvalues {e_val:.2e} fp64 residual {e_res:.2e} "
          f"(solver's own {float(info.residuals.max()) / lam1:.2e}) orthonormality {e_orth:.2e} l_1 {lam1:.4e} l_10 {float(top[9]):.4e}")
    assert info.converged and 1 <= info.n_sweeps <= 100
    assert e_val <= 1e-5
    assert e_res <= 2 * TOL
    assert e_orth <= 1e-5
    want_loss = torch.zeros(1, device="cuda")
    eng = edge_model(*case).engine
    for idx, y in train_batches(case[3][0], case[3][3]):
        eng.full_accumulate(idx, y, torch.zeros(H.shape[0], H.shape[0], device="cuda"), want_loss)
    assert abs(float(loss) - float(want_loss)) <= 1e-6 * abs(float(want_loss))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_same_call_same_bits_and_another_seed_the_same_spectrum(case):
    U, l, _, info = solved(case)
    be = backend(case, low_rank=10)
    U2, l2, _ = be.eig_lowrank(train_loader(case[3][0], case[3][3]), tol=TOL)
    assert torch.equal(U, U2) and torch.equal(l, l2) and be.lowrank_info.n_sweeps == info.n_sweeps
    _, l3, _, info3 = solved(case, seed=7)
    top = torch.linalg.eigvalsh(H64(case)).flip(0)[:10]
    e = float((l3.double() - top).abs().max()) / float(top[0])
    print(f"{case_id(case)}: seed 7: sweeps {info3.n_sweeps}, eigenvalues within {e:.2e} of the dense spectrum")
    assert info3.converged and e <= 1e-5


def fitted(case, prior, **backend_kwargs):
    import laplace_gnn_amd as lg

    la = lg.Laplace(edge_model(*case), "classification", "all", "lowrank", prior_precision=prior,
                    backend_kwargs=dict(low_rank=10, lowrank_tol=TOL, **backend_kwargs))
    la.fit(train_loader(case[3][0], case[3][3]))
    return la


@pytest.mark.parametrize("prior", ["scalar", "layerwise"])
def test_class_algebra_against_the_dense_definition(prior):
    import laplace_gnn_amd as lg

    case = CASES[0]
    m = edge_model(*case)
    n_layers = len([p for p in m.parameters() if p.requires_grad])
    pp = 0.7 if prior == "scalar" else torch.linspace(0.4, 2.5, n_layers).cuda()
    la = fitted(case, pp)
    assert isinstance(la, lg.LowRankLaplace) and la.n_sweeps >= 1 and la.converged
    U, l = la.H
    Pn = U.shape[0]
    d = la.prior_precision_diag.double()
    P64 = U.double() @ torch.diag(l.double()) @ U.double().T + torch.diag(d)
    Pinv = torch.linalg.inv(P64)
    errs = {"logdet": abs(float(la.log_det_posterior_precision) - float(torch.logdet(P64))) / abs(float(torch.logdet(P64)))}
    idx = train_set(case[3][0], case[3][3])[0][:9].contiguous()
    Js = m.engine.jacobians(idx)[0]
    want_var = torch.einsum("ncp,pq,nkq->nck", Js.double(), Pinv, Js.double())
    errs["functional_variance"] = float((la.functional_variance(Js).double() - want_var).abs().max()) / float(want_var.abs().max())
    J2 = Js.double().reshape(-1, Pn)
    want_cov = J2 @ Pinv @ J2.T
    errs["functional_covariance"] = float((la.functional_covariance(Js).double() - want_cov).abs().max()) / float(want_cov.abs().max())
    T = la._sample_transform(torch.eye(Pn, device="cuda")).double()
    errs["sample_transform"] = float((T @ T.T - Pinv).abs().max()) / float(Pinv.abs().max())
    eps = torch.randn(3, Pn, generator=torch.Generator().manual_seed(5)).cuda()
    want_s = la.mean.double() + eps.double() @ T.T
    errs["sample"] = float((la.sample(eps=eps).double() - want_s).abs().max()) / float(want_s.abs().max())
    print(f"{prior}: " + " ".join(f"{n} {v:.2e}" for n, v in errs.items()))
    for n, v in errs.items():
        assert v <= 1e-4, (n, v)


def test_rank_at_or_above_K_matches_full_laplace():
    """6 train ids at C = 5: rank <= 24 < low_rank = 32; the low-rank posterior is the full one."""
    import laplace_gnn_amd as lg

    case = CASES[0]
    m = edge_model(*case)
    N, C = case[3][0], case[3][3]
    idx, y = train_set(N, C)
    loader = lg.TensorBatchLoader(idx[:6].contiguous(), y[:6].contiguous(), batch_size=4)
    lr = lg.Laplace(m, "classification", "all", "lowrank", prior_precision=0.7, backend_kwargs=dict(low_rank=32))
    lr.fit(loader)
    full = lg.Laplace(m, "classification", "all", "full", prior_precision=0.7)
    full.fit(loader)
    assert lr.H[0].shape[1] <= 24 and lr.converged and lr.n_sweeps <= 2, (lr.H[0].shape, lr.n_sweeps)
    m_lr, m_full = float(lr.log_marginal_likelihood()), float(full.log_marginal_likelihood())
    pred = torch.arange(0, N, 7, device="cuda")
    e_probit = float((lr(pred) - full(pred)).abs().max())
    lr.optimize_prior_precision(method="marglik", n_steps=25, lr=0.1, init_prior_prec=1.0)
    full.optimize_prior_precision(method="marglik", n_steps=25, lr=0.1, init_prior_prec=1.0)
    pp_lr, pp_full = float(lr.prior_precision), float(full.prior_precision)
    print(f"rank {lr.H[0].shape[1]} sweeps {lr.n_sweeps}: marglik {m_lr:.5f} vs {m_full:.5f}; probit {e_probit:.2e}; "
          f"optimised prior {pp_lr:.5f} vs {pp_full:.5f}")
    assert abs(m_lr - m_full) <= MARGLIK_RTOL * abs(m_full)
    assert e_probit <= RTOL
    assert abs(pp_lr - pp_full) <= MARGLIK_RTOL * abs(pp_full)


@pytest.mark.parametrize("case", CASES + [("sage", 2, "tanh", SHAPES[0], False)], ids=case_id)
def test_matrix_free_glm_predictive_against_the_chunked_jacobian_one(case):
    import laplace_gnn_amd as lg

    la = fitted(case, 0.7)
    pred = torch.arange(0, case[3][0], 5, device="cuda")
    assert la._lowrank_matrix_free()
    mu, var = la._glm_predictive_distribution(pred)
    mu_d, var_d = la._glm_predictive_distribution(pred, diagonal_output=True)
    mu_j, var_j = lg.ParametricLaplace._glm_predictive_distribution(la, pred)
    scale = float(var_j.abs().max())
    e = float((var - var_j).abs().max()) / scale
    e_d = float((var_d - torch.diagonal(var_j, dim1=1, dim2=2)).abs().max()) / scale
    print(f"{case_id(case)}: f_var {e:.2e} diagonal {e_d:.2e}")
    assert torch.allclose(mu, mu_j, atol=1e-6) and torch.allclose(mu_d, mu_j, atol=1e-6)
    assert e <= 1e-5 and e_d <= 1e-5
    la.prior_precision = torch.linspace(0.4, 2.5, la.n_layers).cuda()
    assert not la._lowrank_matrix_free()  # a per-layer prior takes the chunked-Jacobian path
    assert torch.equal(la._glm_predictive_distribution(pred)[1], lg.ParametricLaplace._glm_predictive_distribution(la, pred)[1])


def test_state_dict_round_trip():
    import laplace_gnn_amd as lg

    case = CASES[0]
    la = fitted(case, 0.7)
    sd = la.state_dict()
    assert isinstance(sd["H"], tuple) and sd["cls_name"] == "LowRankLaplace"
    lb = lg.Laplace(edge_model(*case), "classification", "all", "lowrank", prior_precision=1.0)
    lb.load_state_dict(sd)
    assert torch.equal(lb.H[0], la.H[0]) and torch.equal(lb.H[1], la.H[1])
    assert float(lb.log_marginal_likelihood()) == float(la.log_marginal_likelihood())
    pred = torch.arange(0, case[3][0], 9, device="cuda")
    assert torch.equal(lb(pred), la(pred))
    assert lb.predictive_samples(pred, n_samples=4, generator=torch.Generator(device="cuda").manual_seed(1)).shape == (4, pred.shape[0], 5)
    assert lb(pred, pred_type="nn", link_approx="mc", n_samples=8).shape == (pred.shape[0], 5)


def test_refusals():
    import laplace_gnn_amd as lg

    case = CASES[0]
    m = edge_model(*case)
    loader = train_loader(case[3][0], case[3][3])
    la = lg.Laplace(m, "classification", "all", "lowrank")
    with pytest.raises(ValueError, match="LowRank LA does not support updating."):
        la.fit(loader, override=False)
    with pytest.raises(NotImplementedError, match="process_group"):
        la.fit(loader, process_group=object())
    with pytest.raises(NotImplementedError, match="neg_marglik_adj_grad"):
        la.neg_marglik_adj_grad(loader)
    with pytest.raises(NotImplementedError, match="fit_graph"):
        la.fit_graph = True
    ef = lg.Laplace(m, "classification", "all", "lowrank", backend=lg.HipEF)
    with pytest.raises(NotImplementedError, match="eig_lowrank"):
        ef.fit(loader)
    with pytest.raises(NotImplementedError, match="ggn_matmat"):
        lg.HipEF(m, "classification").ggn_matmat(loader, torch.zeros(1, m.engine.n_params))
