"""CPU tests of subnetwork Laplace: the masks of ``laplace_gnn_amd.subnetmask`` on the Laplace parameter vector, and the front
(``SubnetLaplace`` / ``FullSubnetLaplace`` / ``DiagSubnetLaplace``) with an injected oracle backend against the reference's own
``laplace/subnetlaplace.py`` (goldens of tools/make_subnet_golden.py: default backend, prior precision 0.7)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle_backend import CpuForwardGCN, OracleBackend
from subnet_utils import SETS, SUBNET_CASES, model_from_golden, param_ranges, rel, subnet_golden

import laplace_gnn_amd as lg

RTOL = 1e-4


class SubnetOracleBackend(OracleBackend):
    """The CPU oracle sliced by ``subnetwork_indices`` the way GGNInterface slices its Jacobians
    (laplace/curvature/curvature.py:127-128)."""
    subnetwork_indices = None

    def full(self, x, y, **kw):
        loss, H = super().full(x, y, **kw)
        s = self.subnetwork_indices
        return loss, H[s][:, s]

    def diag(self, x, y, **kw):
        loss, H = super().diag(x, y, **kw)
        return loss, H[self.subnetwork_indices]

    def jacobians(self, x, enable_backprop=False):
        Js, f = super().jacobians(x, enable_backprop)
        return Js[:, :, self.subnetwork_indices], f


def _small_gcn(res=False, seed=0, layers=2):
    g = torch.Generator().manual_seed(seed)
    N, F, H, C = 40, 6, 5, 3
    X = torch.randn(N, F, generator=g)
    ei = torch.randint(0, N, (2, 90), generator=g)
    torch.manual_seed(seed)
    kw = dict(res=True, norm="layer") if res else {}
    return lg.GCN(F, H, C, layers, X, ei, **kw).eval(), (N, F, H, C)


def _theta(model):
    return torch.cat([p.detach().reshape(-1) for k, p in model.named_parameters() if "norms" not in k and "adj" not in k])


# ---- masks ------------------------------------------------------------------------------------------------------
def test_largest_magnitude_mask_is_the_top_k_of_the_laplace_vector():
    model, (N, F, H, C) = _small_gcn()
    theta = _theta(model)
    P = F * H + H + H * C + C
    assert theta.numel() == P
    mask = lg.LargestMagnitudeSubnetMask(model, n_params_subnet=11)
    with pytest.raises(AttributeError):
        mask.indices
    idx = mask.select()
    want = torch.sort(torch.argsort(theta.abs(), descending=True, stable=True)[:11]).values
    assert idx.dtype == torch.int64 and torch.equal(idx, want) and torch.equal(mask.indices, want)
    assert mask.n_params_subnet == 11
    assert float(theta.abs()[idx].min()) >= float(np.sort(theta.abs().numpy())[-11])
    with pytest.raises(ValueError):
        mask.select()  # already selected
    full = lg.LargestMagnitudeSubnetMask(model, n_params_subnet=P).select()
    assert torch.equal(full, torch.arange(P))
    with pytest.raises(ValueError):
        lg.LargestMagnitudeSubnetMask(model, n_params_subnet=P + 1)
    with pytest.raises(ValueError):
        lg.LargestMagnitudeSubnetMask(model, n_params_subnet=None)


def test_masks_index_the_laplace_vector_not_model_parameters():
    """A structure-learning model registers its dense adjacency as a parameter; it is no part of the Laplace vector."""
    g = torch.Generator().manual_seed(1)
    N, F, H, C = 30, 4, 5, 3
    X = torch.randn(N, F, generator=g)
    adj = (torch.rand(N, N, generator=g) < 0.1).float()
    torch.manual_seed(1)
    model = lg.STEGCN(F, H, C, 2, X, adj).eval()
    assert any("adj" in k for k, _ in model.named_parameters())
    P = F * H + H + H * C + C
    mask = lg.LargestMagnitudeSubnetMask(model, n_params_subnet=P)
    assert torch.equal(mask.select(), torch.arange(P))
    with pytest.raises(ValueError):
        lg.LargestMagnitudeSubnetMask(model, n_params_subnet=P + 1)
    with pytest.raises(ValueError):
        lg.ParamNameSubnetMask(model, [next(k for k, _ in model.named_parameters() if "adj" in k)]).select()


def test_name_masks_give_the_parameters_ranges():
    model, (N, F, H, C) = _small_gcn(res=True)
    r = param_ranges(model)
    assert list(r) == ["convs.0.lin.weight", "convs.0.lin.bias", "convs.1.lin.weight", "convs.1.lin.bias", "res.0.weight",
                       "res.0.bias"]

    def span(*names):
        return torch.cat([torch.arange(r[k][0], r[k][0] + r[k][1]) for k in names])

    idx = lg.ParamNameSubnetMask(model, ["convs.1.lin.bias", "convs.0.lin.bias"]).select()
    assert torch.equal(idx, span("convs.0.lin.bias", "convs.1.lin.bias"))  # sorted, whatever the order of the names
    idx = lg.ModuleNameSubnetMask(model, ["convs.0.lin"]).select()
    assert torch.equal(idx, torch.arange(0, F * H + H))
    idx = lg.ModuleNameSubnetMask(model, ["res.0", "convs.1.lin"]).select()
    assert torch.equal(idx, span("convs.1.lin.weight", "convs.1.lin.bias", "res.0.weight", "res.0.bias"))
    # the head is convs[-1].lin, not the last nn.Linear in module order (res.0)
    last = lg.LastLayerSubnetMask(model)
    assert torch.equal(last.select(), span("convs.1.lin.weight", "convs.1.lin.bias"))
    assert torch.equal(lg.LastLayerSubnetMask(model, "res.0").select(), span("res.0.weight", "res.0.bias"))
    for bad in (lambda: lg.ParamNameSubnetMask(model, ["convs.7.lin.weight"]).select(),
                lambda: lg.ParamNameSubnetMask(model, []).select(),
                lambda: lg.ParamNameSubnetMask(model, ["norms.0.weight"]).select(),  # a parameter, but no Laplace parameter
                lambda: lg.ModuleNameSubnetMask(model, ["convs.0"]).select(),        # has children
                lambda: lg.ModuleNameSubnetMask(model, ["nope"]).select(),
                lambda: lg.ModuleNameSubnetMask(model, []).select()):
        with pytest.raises(ValueError):
            bad()


def test_random_mask_is_reproducible_and_mask_conversion_validates():
    model, (N, F, H, C) = _small_gcn()
    P = F * H + H + H * C + C
    a = lg.RandomSubnetMask(model, 9, generator=torch.Generator().manual_seed(5)).select()
    b = lg.RandomSubnetMask(model, 9, generator=torch.Generator().manual_seed(5)).select()
    c = lg.RandomSubnetMask(model, 9, generator=torch.Generator().manual_seed(6)).select()
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert a.numel() == 9 and a.unique().numel() == 9 and int(a.min()) >= 0 and int(a.max()) < P
    assert bool((a[1:] > a[:-1]).all())
    m = lg.SubnetMask(model)
    bits = torch.zeros(P, dtype=torch.bool)
    bits[[3, 17]] = True
    assert m.convert_subnet_mask_to_indices(bits).tolist() == [3, 17]
    for bad in (bits.float(), bits[:-1], bits.reshape(1, -1), bits.long() * 2, [0, 1]):
        with pytest.raises(ValueError):
            m.convert_subnet_mask_to_indices(bad)
    with pytest.raises(NotImplementedError):
        m.select()


def test_largest_variance_mask_keeps_the_largest_marginal_variances():
    g = np.load(os.path.join(GOLDEN, "gcn_small_3batch_s1.npz"))
    model = CpuForwardGCN(model_from_golden(g))
    loader = lg.TensorBatchLoader(torch.from_numpy(g["train_idx"]), torch.from_numpy(g["train_y"]), int(g["batch_size"]))
    diag = lg.Laplace(model, "classification", "all", "diag", backend=OracleBackend, prior_precision=0.5)
    mask = lg.LargestVarianceDiagLaplaceSubnetMask(model, 13, diag)
    with pytest.raises(ValueError):
        mask.select()  # needs the loader
    idx = mask.select(loader)
    var = 1.0 / (diag.H + 0.5)
    assert rel(diag.H.numpy(), g["diag_H"]) < RTOL  # select() fitted the diagonal posterior it was given
    assert torch.equal(idx, torch.sort(torch.argsort(var, descending=True, stable=True)[:13]).values)


# ---- front --------------------------------------------------------------------------------------------------------
def _fit(case, prefix, structure, **kw):
    g = np.load(os.path.join(GOLDEN, case + ".npz"))
    sg = subnet_golden(case)
    model = CpuForwardGCN(model_from_golden(g))
    loader = lg.TensorBatchLoader(torch.from_numpy(g["train_idx"]), torch.from_numpy(g["train_y"]), int(g["batch_size"]))
    idx = torch.from_numpy(sg[prefix + "_indices"])
    la = lg.Laplace(model, "classification", "subnetwork", structure, subnetwork_indices=idx, backend=SubnetOracleBackend,
                    prior_precision=float(sg[prefix + "_prior"]), **kw)
    la.fit(loader)
    return g, sg, la, idx, loader


@pytest.mark.parametrize("prefix", SETS)
@pytest.mark.parametrize("case", SUBNET_CASES)
def test_full_subnet_laplace_matches_reference(case, prefix):
    g, sg, la, idx, _ = _fit(case, prefix, "full")
    k = prefix + "_"
    S, P = idx.numel(), int(g["n_params"])
    assert isinstance(la, lg.FullSubnetLaplace) and isinstance(la, lg.SubnetLaplace) and isinstance(la, lg.FullLaplace)
    assert la.n_params == P and la.n_params_subnet == S and tuple(la.H.shape) == (S, S)
    assert torch.equal(la.backend.subnetwork_indices, idx)
    assert np.linalg.norm(sg[k + "H"]) > 0
    assert rel(la.H.numpy(), sg[k + "H"]) < RTOL
    assert rel(la.H.numpy(), g["fullla_H"][idx.numpy()][:, idx.numpy()]) < RTOL  # the sub-block of the full posterior's H
    assert abs(float(la.loss) - float(sg[k + "loss"])) < RTOL * abs(float(sg[k + "loss"]))
    assert torch.equal(la.mean_subnet, la.mean[idx])
    got07 = float(la.log_marginal_likelihood())
    assert abs(got07 - float(sg[k + "marglik_pp07"])) < 3e-4 * abs(float(sg[k + "marglik_pp07"]))
    got1 = float(la.log_marginal_likelihood(prior_precision=torch.tensor(1.0)))
    assert abs(got1 - float(sg[k + "marglik_pp1"])) < 3e-4 * abs(float(sg[k + "marglik_pp1"]))
    la.prior_precision = float(sg[k + "prior"])
    eps, pidx = torch.from_numpy(sg[k + "eps"]), torch.from_numpy(g["pred_idx"])
    samples = la.sample(eps=eps)
    assert tuple(samples.shape) == (eps.shape[0], P)
    assert rel(samples.numpy(), sg[k + "samples"]) < 5e-4
    # non-subnet entries stay at the MAP exactly
    rest = np.setdiff1d(np.arange(P), idx.numpy())
    assert torch.equal(samples[:, rest], la.mean[rest].expand(eps.shape[0], -1))
    sub = torch.randn(3, S, generator=torch.Generator().manual_seed(0))
    full = la.assemble_full_samples(sub)
    assert torch.equal(full[:, idx], sub) and torch.equal(full[:, rest], la.mean[rest].expand(3, -1))
    _, f_var = la._glm_predictive_distribution(pidx)
    assert rel(f_var.numpy(), sg[k + "glm_fvar"]) < 5e-4
    assert np.abs(la(pidx).numpy() - sg[k + "glm_probit"]).max() < 5e-5
    # the other links and the sampling predictive run on the S-sized objects
    for link in ("mc", "bridge", "bridge_norm"):
        probs = la(pidx, link_approx=link, n_samples=5, generator=torch.Generator().manual_seed(0))
        assert torch.allclose(probs.sum(-1), torch.ones(len(pidx)), atol=1e-5)
    probs = la(pidx, pred_type="nn", link_approx="mc", eps=eps)
    assert torch.allclose(probs.sum(-1), torch.ones(len(pidx)), atol=1e-5)
    assert torch.equal(torch.cat([p.detach().reshape(-1) for p in la.params]), la.mean)  # the MAP is put back


@pytest.mark.parametrize("prefix", SETS)
@pytest.mark.parametrize("case", SUBNET_CASES)
def test_diag_subnet_laplace_matches_reference(case, prefix):
    g, sg, la, idx, _ = _fit(case, prefix, "diag")
    k = prefix + "_"
    S, P = idx.numel(), int(g["n_params"])
    assert isinstance(la, lg.DiagSubnetLaplace) and isinstance(la, lg.DiagLaplace) and tuple(la.H.shape) == (S,)
    assert np.linalg.norm(sg[k + "diag_H"]) > 0
    assert rel(la.H.numpy(), sg[k + "diag_H"]) < RTOL
    assert rel(la.H.numpy(), g["diag_H"][idx.numpy()]) < RTOL
    assert abs(float(la.loss) - float(sg[k + "loss"])) < RTOL * abs(float(sg[k + "loss"]))
    for pp, key in ((None, "diag_marglik_pp07"), (torch.tensor(1.0), "diag_marglik_pp1")):
        got = float(la.log_marginal_likelihood(prior_precision=pp))
        assert abs(got - float(sg[k + key])) < 3e-4 * abs(float(sg[k + key]))
    la.prior_precision = float(sg[k + "prior"])
    eps, pidx = torch.from_numpy(sg[k + "eps"]), torch.from_numpy(g["pred_idx"])
    assert rel(la.sample(eps=eps).numpy(), sg[k + "diag_samples"]) < 5e-4
    assert np.abs(la(pidx).numpy() - sg[k + "diag_glm_probit"]).max() < 5e-5


def test_prior_structures_tuning_and_state_dict(tmp_path):
    g, sg, la, idx, loader = _fit("gcn_small_1batch_s0", "struct", "full")
    S = idx.numel()
    # a length-S diagonal prior enters scatter, log det and the precision in the order of the indices
    pp = torch.linspace(0.5, 2.0, S)
    ml = float(la.log_marginal_likelihood(prior_precision=pp))
    Pm = la.H.double() + torch.diag(pp.double())
    delta = la.mean[idx].double()
    want = -float(la.loss) - 0.5 * (float(torch.logdet(Pm)) - float(pp.double().log().sum()) + float((delta * pp.double()) @ delta))
    assert abs(ml - want) < 3e-4 * abs(want)
    for bad in (torch.ones(S + 1), torch.ones(la.n_layers), torch.ones(la.n_params)):
        la.prior_precision = bad
        with pytest.raises(ValueError):
            la.prior_precision_diag
    la.prior_precision = 0.7
    before = float(la.log_marginal_likelihood())
    la.optimize_prior_precision(method="marglik", n_steps=20, lr=0.1, prior_structure="scalar")
    assert la.prior_precision.numel() == 1 and float(la.log_marginal_likelihood()) > before
    la.optimize_prior_precision(method="marglik", n_steps=20, lr=0.1, prior_structure="diag")
    assert la.prior_precision.numel() == S and float(la.log_marginal_likelihood()) > before
    la.prior_precision = 0.7

    path = os.path.join(tmp_path, "la.pt")
    torch.save(la.state_dict(), path)
    model2 = CpuForwardGCN(model_from_golden(g))
    la2 = lg.Laplace(model2, "classification", "subnetwork", "full", subnetwork_indices=idx, backend=SubnetOracleBackend)
    la2.load_state_dict(torch.load(path))
    pidx = torch.from_numpy(g["pred_idx"])
    assert float(la2.log_marginal_likelihood()) == float(la.log_marginal_likelihood())
    assert torch.equal(la2(pidx), la(pidx))
    # a state fitted on another subnetwork: another H shape, or the same shape over other indices
    other = lg.Laplace(model2, "classification", "subnetwork", "full", subnetwork_indices=idx[:-1], backend=SubnetOracleBackend)
    with pytest.raises(ValueError):
        other.load_state_dict(torch.load(path))
    moved = lg.Laplace(model2, "classification", "subnetwork", "full", subnetwork_indices=idx.flip(0),
                       backend=SubnetOracleBackend)
    with pytest.raises(ValueError):
        moved.load_state_dict(torch.load(path))
    wrong = lg.Laplace(model2, "classification", "subnetwork", "diag", subnetwork_indices=idx, backend=SubnetOracleBackend)
    with pytest.raises(ValueError):
        wrong.load_state_dict(torch.load(path))


def test_refusals():
    g = np.load(os.path.join(GOLDEN, "gcn_small_1batch_s0.npz"))
    model = CpuForwardGCN(model_from_golden(g))
    P = int(g["n_params"])

    def make(idx, structure="full", **kw):
        return lg.Laplace(model, "classification", "subnetwork", structure, subnetwork_indices=idx, backend=SubnetOracleBackend,
                          **kw)

    for bad in (torch.tensor([1, 5, 1]), torch.tensor([-1, 3]), torch.tensor([0, P]), torch.tensor([], dtype=torch.int64),
                torch.tensor([1.0, 2.0]), torch.tensor([[1, 2], [3, 4]]), torch.tensor([1, 2], dtype=torch.int32), None, [1, 2]):
        for structure in ("full", "diag"):
            with pytest.raises(ValueError):
                make(bad, structure)
    with pytest.raises(ValueError):
        make(torch.tensor([1, 2]), "kron")
    with pytest.raises(ValueError):
        make(torch.tensor([1, 2]), asdl_fisher_kwargs={"a": 1})
    with pytest.raises(TypeError):
        lg.Laplace(model, "classification", "subnetwork", "full", backend=SubnetOracleBackend)  # no indices
    ok = make(torch.tensor([P - 1, 0, 7]))
    assert ok.n_params_subnet == 3 and tuple(ok.H.shape) == (3, 3)  # H exists before the first fit, as in the reference
    with pytest.raises(NotImplementedError):
        ok.neg_marglik_adj_grad(None)
    with pytest.raises(NotImplementedError):
        make(torch.tensor([1, 2]), "diag").neg_marglik_adj_grad(None)
    ok.prior_precision = torch.ones(2)
    with pytest.raises(ValueError):
        ok.prior_precision_diag


def test_hip_backend_refuses_what_it_cannot_serve_by_name():
    """HipGGN takes the indices at construction or afterwards; HipEF, last_layer and stochastic refuse them by name."""
    g = np.load(os.path.join(GOLDEN, "gcn_small_1batch_s0.npz"))
    model = CpuForwardGCN(model_from_golden(g))  # (its ``engine`` is the CPU stand-in: the real backend classes run here)
    idx = torch.tensor([4, 0, 9])
    be = lg.HipGGN(model, "classification")
    assert be.subnetwork_indices is None
    be.subnetwork_indices = idx
    assert torch.equal(be.subnetwork_indices.cpu(), idx)
    assert torch.equal(lg.HipGGN(model, "classification", subnetwork_indices=idx).subnetwork_indices.cpu(), idx)
    with pytest.raises(NotImplementedError, match="HipEF"):
        lg.HipEF(model, "classification", subnetwork_indices=idx)
    ef = lg.HipEF(model, "classification")
    with pytest.raises(NotImplementedError, match="HipEF"):
        ef.subnetwork_indices = idx
    with pytest.raises(NotImplementedError, match="last_layer"):
        lg.HipGGN(model, "classification", last_layer=True, subnetwork_indices=idx)
    with pytest.raises(NotImplementedError, match="stochastic"):
        lg.HipGGN(model, "classification", stochastic=True, subnetwork_indices=idx)
    st = lg.HipGGN(model, "classification", stochastic=True)
    with pytest.raises(NotImplementedError, match="stochastic"):
        st.subnetwork_indices = idx
    with pytest.raises(ValueError):
        be.subnetwork_indices = torch.tensor([1.5])
