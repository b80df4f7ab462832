"""Last-layer Kronecker / diagonal Laplace on the CPU: the fp64 restatement of the definitions (tests/lastlayer_reference.py)
against the reference's own numbers (tests/golden/lastlayer, tools/make_lastlayer_golden.py) and against the existing
goldens' full GGN; the factory; and the host logic of ``KronLLLaplace`` / ``DiagLLLaplace`` (marginal likelihood,
``override=False``, ``state_dict``, closed-form predictive variance, data-parallel fit) behind a stand-in backend."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import GOLDEN, ROOT

import laplace_gnn_amd as lg
import lastlayer_reference as R
from oracle_backend import oracle_model_of
from test_host_logic import _cpu_model

RTOL = 1e-4  # the project's bar for fitted blocks
LL_GOLDENS = ["ll_gcn_dir_3batch", "ll_gcn_sym_1batch", "ll_sage_dir_1batch", "ll_sage_sym_3batch"]


def _ll_golden(name):
    return np.load(os.path.join(GOLDEN, "lastlayer", name + ".npz"))


def _loader(g):
    return lg.TensorBatchLoader(torch.from_numpy(g["train_idx"]), torch.from_numpy(g["train_y"]), int(g["batch_size"]))


def _restated(g, fork_exact=True):
    om = oracle_model_of(_cpu_model(g).inner)
    return om, R.fit_from_model(om, g["train_idx"], g["train_y"], int(g["batch_size"]), fork_exact)


# ---- 1. the restatement against the reference's own numbers -----------------------------------------------------------------
@pytest.mark.parametrize("name", LL_GOLDENS)
def test_restatement_matches_the_reference_on_the_head(name):
    import gnn_laplace_oracle as O

    g = _ll_golden(name)
    om, fit = _restated(g, fork_exact=True)
    phi, s, f = O.lastlayer_features(om, g["train_idx"])
    assert R.rel(phi, g["Phi"]) < RTOL and R.rel(s, g["s"]) < RTOL and R.rel(f, g["logits"]) < RTOL
    assert R.rel(fit["A"], g["A"]) < RTOL
    assert R.rel(fit["B"], g["B"]) < RTOL
    assert R.rel(fit["diag"], g["diag"]) < RTOL
    assert abs(fit["loss"] - float(g["loss"])) < RTOL * abs(float(g["loss"]))
    up = R.fit_from_model(om, g["train_idx"], g["train_y"], int(g["batch_size"]), fork_exact=False)
    assert R.rel(up["Bb"], g["Bb_lambda"]) < RTOL  # upstream seeds: V V^T = Lambda, the bias-bias block of the full GGN
    if str(g["kind"]) == "sage":
        assert R.rel(fit["Bb"], g["Bb"]) < RTOL          # the reference's own bias block
        assert np.array_equal(fit["Bb"], fit["B"])       # s = 1
        assert R.rel(up["B"], g["Bb_lambda"]) < RTOL
    else:
        assert float(np.abs(g["s"] - 1).max()) > 0.1     # the GCN cases do exercise s_n != 1


def test_fp64_seeds_restate_the_oracle_seeds():
    import gnn_laplace_oracle as O

    f = np.random.default_rng(0).normal(size=(17, 5)).astype(np.float32) * 2
    for fe in (True, False):
        assert R.rel(R.seeds64(f, fe), O.kfac_seeds(f, fe)) < 1e-6
        V = R.seeds64(f, fe)
        if not fe:  # V V^T = diag(p) - p p^T
            p = R.softmax64(f)
            lam = np.einsum("nk,kj->nkj", p, np.eye(5)) - p[:, :, None] * p[:, None, :]
            assert R.rel(np.einsum("nkc,njc->nkj", V, V), lam) < 1e-12


# ---- 2. ... and against the full GGN over all weights of the existing goldens ------------------------------------------------
@pytest.mark.parametrize("name", ["gcn_small_1batch_s0", "sage_small_1batch_s0", "gcn3_small_1batch_s0", "sage3_small_1batch_s0"])
def test_restatement_is_the_tail_of_the_full_ggn(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    om, up = _restated(g, fork_exact=False)
    L = int(g["num_layers"])
    C, D = g[f"W{L - 1}"].shape
    p_ll = C * D + C
    full = g["full_H"].astype(np.float64)
    assert R.rel(up["diag"], np.diag(full)[-p_ll:]) < RTOL  # convs.{L-1}.lin.{weight, bias} are the last parameters
    assert abs(up["loss"] - float(g["full_loss"])) < RTOL * abs(float(g["full_loss"]))
    if str(g["kind"]) == "sage":
        assert R.rel(up["B"], full[-C:, -C:]) < RTOL
    else:  # GCN: the bias sees s_n
        assert R.rel(up["Bb"], full[-C:, -C:]) < RTOL


# ---- 3. the factory ----------------------------------------------------------------------------------------------------------
def test_factory_defaults_are_the_last_layer_kronecker_posterior():
    model = _cpu_model(_ll_golden("ll_sage_sym_3batch"))
    la = lg.Laplace(model, "classification", backend=R.LastLayerOracleBackend)
    assert type(la) is lg.KronLLLaplace and isinstance(la, lg.KronLaplace)
    ld = lg.Laplace(model, "classification", "last_layer", "diag", backend=R.LastLayerOracleBackend)
    assert type(ld) is lg.DiagLLLaplace and isinstance(ld, lg.DiagLaplace)
    head = model.convs[-1].lin
    for l in (la, ld):
        assert l.params[0] is head.weight and l.params[1] is head.bias and l.n_layers == 2
        assert l.n_params == head.weight.numel() + head.bias.numel()
        assert l.backend.last_layer
    with pytest.raises(NotImplementedError, match="classification"):
        lg.Laplace(model, "regression", backend=R.LastLayerOracleBackend)


def test_head_is_the_last_convolution_not_the_last_linear_in_module_order():
    g = np.load(os.path.join(GOLDEN, "gcn_resln_small_1batch_s0.npz"))
    model = _cpu_model(g)
    la = lg.Laplace(model, "classification", backend=R.LastLayerOracleBackend)
    assert la.params[0] is model.convs[-1].lin.weight
    assert la.params[0] is not [m for m in model.modules() if isinstance(m, torch.nn.Linear)][-1].weight


# ---- 4. host logic behind the stand-in backend ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ll_gcn_dir_3batch", "ll_sage_sym_3batch"])
def test_fit_marglik_override_and_state_dict(name):
    g = _ll_golden(name)
    model = _cpu_model(g)
    _, fit = _restated(g)
    loader = _loader(g)
    N = len(loader.dataset)
    la = lg.Laplace(model, "classification", backend=R.LastLayerOracleBackend, prior_precision=0.7)
    la.fit(loader)
    (B, A), (Bb,) = la.H_facs.kfacs
    assert R.rel(A, fit["A"]) < 1e-6 and R.rel(B, fit["B"]) < 1e-6 and R.rel(Bb, fit["Bb"]) < 1e-6
    assert R.rel(A, g["A"]) < RTOL and R.rel(B, g["B"]) < RTOL
    assert abs(float(la.loss) - fit["loss"]) < 1e-6 * fit["loss"] and la.n_data == N
    ld = lg.Laplace(model, "classification", "last_layer", "diag", backend=R.LastLayerOracleBackend, prior_precision=0.7)
    ld.fit(loader)
    assert R.rel(ld.H, fit["diag"]) < 1e-6 and R.rel(ld.H, g["diag"]) < RTOL
    assert abs(float(ld.loss) - fit["loss"]) < 1e-6 * fit["loss"]

    # the marginal likelihood by hand: log lik - 1/2 (logdet P - logdet P_0 + scatter), P = blockdiag(B (x) A, B_b) + delta I
    mean = np.concatenate([g["W1"].reshape(-1), g["b1"]]).astype(np.float64)
    for pp in (0.7, np.array([0.3, 2.0])):
        dw, db = (pp, pp) if np.isscalar(pp) else pp
        Pw = np.kron(fit["B"], fit["A"]) + dw * np.eye(fit["B"].shape[0] * fit["A"].shape[0])
        Pb = fit["Bb"] + db * np.eye(len(fit["Bb"]))
        prior = np.concatenate([np.full(len(Pw), dw), np.full(len(Pb), db)])
        hand = -fit["loss"] - 0.5 * (np.linalg.slogdet(Pw)[1] + np.linalg.slogdet(Pb)[1] - np.log(prior).sum()
                                     + (prior * mean * mean).sum())
        got = float(la.log_marginal_likelihood(prior_precision=torch.as_tensor(pp, dtype=torch.float32)))
        assert abs(got - hand) < 1e-4 * abs(hand), (got, hand)
        Pd = fit["diag"] + prior
        hand_d = -fit["loss"] - 0.5 * (np.log(Pd).sum() - np.log(prior).sum() + (prior * mean * mean).sum())
        got_d = float(ld.log_marginal_likelihood(prior_precision=torch.as_tensor(pp, dtype=torch.float32)))
        assert abs(got_d - hand_d) < 1e-4 * abs(hand_d)
    la.prior_precision = ld.prior_precision = 0.7

    # state_dict round trip
    lb = lg.Laplace(model, "classification", backend=R.LastLayerOracleBackend)
    lb.load_state_dict(la.state_dict())
    assert float(lb.log_marginal_likelihood()) == pytest.approx(float(la.log_marginal_likelihood()), rel=1e-6)
    assert torch.equal(lb.mean, la.mean) and lb.n_data == N
    with pytest.raises(ValueError, match="wrong Laplace type"):
        lg.Laplace(model, "classification", "all", "kron", backend=R.LastLayerOracleBackend).load_state_dict(la.state_dict())
    le = lg.Laplace(model, "classification", "last_layer", "diag", backend=R.LastLayerOracleBackend)
    le.load_state_dict(ld.state_dict())
    assert torch.equal(le.H, ld.H)

    # override=False twice: KronLaplace's discounting (A weighted by the data counts, B summed), the diagonal summed
    A1, B1, Bb1, loss1, H1 = A.clone(), B.clone(), Bb.clone(), float(la.loss), ld.H.clone()
    for _ in range(2):
        la.fit(loader, override=False)
        ld.fit(loader, override=False)
    (B3, A3), (Bb3,) = la.H_facs.kfacs
    assert R.rel(A3, A1) < 1e-6 and R.rel(B3, 3 * B1) < 1e-6 and R.rel(Bb3, 3 * Bb1) < 1e-6
    assert float(la.loss) == pytest.approx(3 * loss1, rel=1e-6) and la.n_data == 3 * N
    assert R.rel(ld.H, 3 * H1) < 1e-6 and float(ld.loss) == pytest.approx(3 * loss1, rel=1e-6) and ld.n_data == 3 * N


# ---- 5. the closed-form predictive variance -----------------------------------------------------------------------------------
@pytest.mark.parametrize("damping", [False, True])
@pytest.mark.parametrize("name", ["ll_gcn_dir_3batch", "ll_sage_dir_1batch"])
def test_closed_form_variance_is_the_inverse_square_form_of_the_jacobians(name, damping):
    g = _ll_golden(name)
    model = _cpu_model(g)
    la = lg.Laplace(model, "classification", backend=R.LastLayerOracleBackend, prior_precision=torch.tensor([0.625, 1.75]),
                    damping=damping, temperature=0.8)
    la.fit(_loader(g))
    x = torch.arange(int(g["num_nodes"]))
    phi, s, f = la.backend.lastlayer_features(x)
    Js = torch.from_numpy(R.jacobians_from_features(phi.numpy(), s.numpy(), f.shape[1]))
    # the posterior precision from the SAME fp64 eigenpairs, everything in fp64
    pairs = [[la._eigh64(0, 0), la._eigh64(0, 1)], [la._eigh64(1, 0)]]
    P = lg.KronDecomposed([[Q for _, Q in ps] for ps in pairs], [[lam for lam, _ in ps] for ps in pairs],
                          deltas=torch.zeros(2, dtype=torch.float64), damping=damping) * la._H_factor
    P = P + torch.tensor([0.625, 1.75], dtype=torch.float64)  # (exact in fp32: the front holds the prior in fp32)
    want = P.inv_square_form(Js)
    got = la._ll_variance(phi.double(), s.double(), False)
    assert R.rel(got.numpy(), want.numpy()) < 1e-12
    assert R.rel(la._ll_variance(phi.double(), s.double(), True).numpy(), torch.diagonal(want, dim1=1, dim2=2).numpy()) < 1e-12
    # the front's fp32 route against its own Jacobian route
    f_mu, f_var = la._glm_predictive_distribution(x)
    assert R.rel(f_var.numpy(), la.functional_variance(Js.float()).numpy()) < RTOL
    assert torch.allclose(f_mu, f)
    # the diagonal posterior
    ld = lg.Laplace(model, "classification", "last_layer", "diag", backend=R.LastLayerOracleBackend, prior_precision=0.6)
    ld.fit(_loader(g))
    want_d = torch.einsum("ncp,p,nkp->nck", Js, 1.0 / ld.posterior_precision.double(), Js)
    assert R.rel(ld._glm_predictive_distribution(x)[1].numpy(), want_d.numpy()) < 1e-5
    assert R.rel(ld._glm_predictive_distribution(x, diagonal_output=True)[1].numpy(),
                 torch.diagonal(want_d, dim1=1, dim2=2).numpy()) < 1e-5


def test_predictive_links_and_head_samples_on_the_cpu():
    g = _ll_golden("ll_sage_sym_3batch")
    model = _cpu_model(g)
    x = torch.arange(int(g["num_nodes"]))
    for sub in ("kron", "diag"):
        la = lg.Laplace(model, "classification", "last_layer", sub, backend=R.LastLayerOracleBackend)
        la.fit(_loader(g))
        for link in ("probit", "bridge", "bridge_norm", "mc"):
            p = la(x, link_approx=link, n_samples=20, generator=torch.Generator().manual_seed(0))
            assert p.shape == (len(x), 3) and torch.allclose(p.sum(-1), torch.ones(len(x)), atol=1e-5)
        before = [q.detach().clone() for q in model.parameters()]
        eps = torch.randn(7, la.n_params, generator=torch.Generator().manual_seed(1))
        p = la(x, pred_type="nn", link_approx="mc", eps=eps)
        assert all(torch.equal(a, b) for a, b in zip(before, model.parameters()))
        # by hand: every sampled head on the features
        phi, s, _ = la.backend.lastlayer_features(x)
        C, D = model.convs[-1].lin.weight.shape
        want = torch.stack([torch.softmax(phi @ th[:C * D].view(C, D).T + s[:, None] * th[C * D:], -1)
                            for th in la.sample(7, eps=eps)]).mean(0)
        assert torch.allclose(p, want, atol=1e-6)


# ---- 6. data-parallel fit ----------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _fit_both(name):
    g = _ll_golden(name)
    model = _cpu_model(g)
    out = {}
    for sub in ("kron", "diag"):
        la = lg.Laplace(model, "classification", "last_layer", sub, backend=R.LastLayerOracleBackend)
        la.fit(_loader(g))
        blocks = [h for F in la.H_facs.kfacs for h in F] if sub == "kron" else [la.H]
        out.update({f"{sub}{i}": b.numpy() for i, b in enumerate(blocks)})
        out[sub + "_loss"], out[sub + "_n"] = float(la.loss), la.n_data
        out[sub + "_marglik"] = float(la.log_marginal_likelihood())
        out[sub + "_calls"] = np.array([len(c[1]) for c in la.backend.calls])
    return out


def _worker(rank, world, port, name, out_dir):
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **_fit_both(name))
    dist.barrier()
    dist.destroy_process_group()


def test_world_2_fit_equals_the_single_process_fit(tmp_path):
    name = "ll_gcn_dir_3batch"
    mp.spawn(_worker, args=(2, _free_port(), name, str(tmp_path)), nprocs=2, join=True)
    ref = _fit_both(name)
    for r in range(2):
        out = np.load(os.path.join(tmp_path, f"rank{r}.npz"))
        for k, v in ref.items():
            if k.endswith("_calls"):  # every rank took a slice of every batch
                assert len(out[k]) == len(v) and out[k].sum() < v.sum()
            elif np.ndim(v):
                assert R.rel(out[k], v) < 1e-5, (r, k)
            else:
                assert float(out[k]) == pytest.approx(float(v), rel=1e-5), (r, k)
