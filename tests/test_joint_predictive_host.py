"""CPU tests of the joint GLM predictive on the fronts (``functional_covariance``, ``_glm_predictive_distribution(joint=True)``,
``la(x, joint=True)``, ``la.glm_covariance``) with the injected oracle backend -- no engine there, so the chunked Jacobian route
in torch runs -- against the reference's goldens of tools/make_joint_golden.py, and of the C ABI of ``lgnn_glm_covariance``.
Bounds: 1e-4 relative (Frobenius) for covariances, the project's bar for predictive variances; 1e-5 for means."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gp_utils import gp_model, rel
from oracle_backend import CpuForwardGCN, OracleBackend
from test_host_logic import _cpu_model

import gnn_laplace_oracle as O
import laplace_gnn_amd as lg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOINT = os.path.join(GOLDEN, "joint")
NAMES = ["gcn_small_1batch_s0", "sage_small_1batch_s0", "gcn_resln_small_1batch_s0", "gcn_regression"]
STRUCTURES = ("kron", "diag", "full")
RTOL, MU_RTOL = 1e-4, 1e-5


class LikelihoodOracleBackend(OracleBackend):
    """``OracleBackend`` whose all-weights ``full`` follows the likelihood (the base class leaves it at classification)."""

    def full(self, x, y, **kw):
        loss, H = O.full_batch(self.model.oracle_model(), x.numpy(), y.numpy(), self.likelihood)
        return torch.tensor(float(loss)), torch.from_numpy(H)


@functools.lru_cache(maxsize=None)
def fitted(name, structure):
    j = np.load(os.path.join(JOINT, name + ".npz"))
    g = np.load(os.path.join(GOLDEN, str(j["source"]) + ".npz"))
    lik = str(j["likelihood"])
    model = CpuForwardGCN(gp_model(g)) if "act" in g.files else _cpu_model(g)
    loader = lg.TensorBatchLoader(torch.from_numpy(g["train_idx"]), torch.from_numpy(g["train_y"]), int(g["batch_size"]))
    la = lg.Laplace(model, lik, "all", structure, backend=LikelihoodOracleBackend, prior_precision=float(j["prior"]),
                    sigma_noise=float(j["sigma_noise"]))
    la.fit(loader)
    return j, la


@pytest.mark.parametrize("structure", STRUCTURES)
@pytest.mark.parametrize("name", NAMES)
def test_joint_predictive_matches_the_reference(name, structure):
    j, la = fitted(name, structure)
    pred = torch.from_numpy(j["pred"])
    C = la.n_outputs
    f_mu, f_cov = la._glm_predictive_distribution(pred, joint=True)
    assert f_mu.shape == (6 * C,) and f_cov.shape == (6 * C, 6 * C)
    e_mu, e_cov = rel(f_mu.numpy(), j[f"{structure}_f_mu_joint"]), rel(f_cov.numpy(), j[f"{structure}_f_cov"])
    print(f"{name} {structure}: f_mu {e_mu:.2e} f_cov {e_cov:.2e}")
    assert e_mu <= MU_RTOL and e_cov <= RTOL
    if str(j["likelihood"]) == "regression":
        mu, cov = la(pred, joint=True)
        assert rel(mu.numpy(), j[f"{structure}_call_mu"]) <= MU_RTOL and rel(cov.numpy(), j[f"{structure}_call_cov"]) <= RTOL


def precision64(la, structure):
    """The posterior precision materialised in fp64 from what the fit accumulated (no eigensolver)."""
    if structure == "diag":
        return torch.diag(la.posterior_precision.double())
    if structure == "full":
        return la.posterior_precision.double()
    f = float(la._H_factor)
    d = la._block_prior_precision(len(la.H_facs.kfacs), torch.float64)
    blocks = []
    for facs, delta in zip(la.H_facs.kfacs, d):
        m = facs[0].double() if len(facs) == 1 else torch.kron(facs[0].double(), facs[1].double())
        blocks.append(f * m + delta * torch.eye(m.shape[0], dtype=torch.float64))
    return torch.block_diag(*blocks)


@pytest.mark.parametrize("structure", STRUCTURES)
@pytest.mark.parametrize("name", ["gcn_small_1batch_s0", "gcn_resln_small_1batch_s0", "gcn_regression"])
def test_functional_covariance_identities(name, structure):
    _, la = fitted(name, structure)
    M, C, P = 5, la.n_outputs, la.n_params
    Js = torch.randn(M, C, P, generator=torch.Generator().manual_seed(3))
    K = la.functional_covariance(Js)
    assert K.shape == (M * C, M * C)
    J64 = Js.double().reshape(M * C, P)
    want = J64 @ torch.linalg.solve(precision64(la, structure), J64.T)
    e = rel(K.numpy(), want.numpy())
    blocks = torch.stack([K[n * C:(n + 1) * C, n * C:(n + 1) * C] for n in range(M)])
    e_var = rel(blocks.numpy(), la.functional_variance(Js).numpy())
    ev = torch.linalg.eigvalsh(K.double())
    print(f"{name} {structure}: vs fp64 {e:.2e}, blocks vs functional_variance {e_var:.2e}, eig min/max {float(ev[0] / ev[-1]):.2e}")
    assert e <= RTOL and e_var <= 1e-5
    assert torch.equal(K, K.T)
    assert float(ev[0]) >= -1e-5 * float(ev[-1])
    with pytest.raises(ValueError):
        la.functional_covariance(Js[:, :, :-1])


def test_every_parametric_front_has_a_functional_covariance():
    for cls in (lg.KronLaplace, lg.DiagLaplace, lg.FullLaplace, lg.FullLLLaplace, lg.KronLLLaplace, lg.DiagLLLaplace,
                lg.LowRankLaplace):
        assert callable(getattr(cls, "functional_covariance")) and callable(getattr(cls, "glm_covariance")), cls


def test_regression_call_returns_the_joint_predictive():
    j, la = fitted("gcn_regression", "kron")
    pred = torch.from_numpy(j["pred"])
    C = la.n_outputs
    mu, cov = la(pred, joint=True)
    assert mu.shape == (6 * C,) and cov.shape == (6 * C, 6 * C)
    mu_d, cov_d = la(pred, joint=True, diagonal_output=True)  # joint wins (laplace/baselaplace.py:622-625)
    assert torch.equal(cov_d, cov) and torch.equal(mu_d, mu)
    f_mu, f_var = la(pred)  # the marginal call is what it was
    assert f_mu.shape == (6, C) and f_var.shape == (6, C, C)
    blocks = torch.stack([cov[n * C:(n + 1) * C, n * C:(n + 1) * C] for n in range(6)])
    assert rel(blocks.numpy(), f_var.numpy()) <= 1e-5 and torch.equal(mu, f_mu.flatten())
    # the repeated node (positions 1 and 3): perfectly correlated outputs
    assert rel(cov[C:2 * C, 3 * C:4 * C].numpy(), cov[C:2 * C, C:2 * C].numpy()) <= 1e-5


@pytest.mark.parametrize("structure", ("kron", "diag"))
def test_classification_does_not_read_joint(structure):
    j, la = fitted("gcn_small_1batch_s0", structure)
    pred = torch.from_numpy(j["pred"])
    for link in ("probit", "bridge"):
        assert torch.equal(la(pred, link_approx=link, joint=True), la(pred, link_approx=link))
    assert torch.equal(la(pred, joint=True, some_unknown_keyword=1), la(pred))


@pytest.mark.parametrize("structure", STRUCTURES)
@pytest.mark.parametrize("name", ["sage_small_1batch_s0", "gcn_regression"])
def test_cross_block_is_the_off_diagonal_block_of_the_square(name, structure):
    j, la = fitted(name, structure)
    x, x2 = torch.from_numpy(j["pred"]), torch.tensor([9, 11, 12, 9])
    C = la.n_outputs
    cross = la.glm_covariance(x, x2)
    assert cross.shape == (6 * C, 4 * C)
    square = la.glm_covariance(torch.cat([x, x2]))
    assert torch.equal(square, square.T)
    assert rel(cross.numpy(), square[:6 * C, 6 * C:].numpy()) <= 1e-5
    assert rel(la.glm_covariance(x).numpy(), la._glm_predictive_distribution(x, joint=True)[1].numpy()) <= 1e-6
    # chunk pairs of Jacobians give the same block: two nodes per chunk
    la._JACOBIAN_BYTES_MAX = 3 * 2 * C * la.n_params * 4
    try:
        assert rel(la.glm_covariance(x, x2).numpy(), cross.numpy()) <= 1e-6
        sq2 = la.glm_covariance(torch.cat([x, x2]))
        assert torch.equal(sq2, sq2.T) and rel(sq2.numpy(), square.numpy()) <= 1e-6
    finally:
        del la._JACOBIAN_BYTES_MAX


def test_lgnn_glm_covariance_is_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "laplace_gnn_hip.h")).read()
    decl = re.search(r"LGNN_API int lgnn_glm_covariance\(([^;]*)\);", text)
    assert decl, "lgnn_glm_covariance is not declared in the header"
    assert len(decl.group(1).split(",")) == len(lg._lib.SIGNATURES["lgnn_glm_covariance"][1]) == 13
    assert re.search(r"#define LGNN_COV_FROM_JACOBIANS 1\b", text) and lg._lib.COV_FROM_JACOBIANS == 1
    for needle in ("laplace/baselaplace.py:1123-1158", ":1223-1242", ":1491-1494", ":1638-1644", ":1905-1910",
                   "laplace/utils/matrix.py (inv_square_form)"):
        assert needle in text, needle
    src = open(os.path.join(ROOT, "laplace-gnn_amd", "csrc", "glmcov.hip")).read()
    for needle in ("1223-1242", "1491-1494", "1638-1644", "1905-1910", "laplace/utils/matrix.py (inv_square_form)"):
        assert needle in src, needle
    lib = lg._lib.load()
    assert hasattr(lib, "lgnn_glm_covariance") and hasattr(lib, "lgnn_glm_covariance_chunk_pairs")
    out = subprocess.run(["nm", "-D", "--defined-only", lg._lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T lgnn_glm_covariance$", out, re.M) and re.search(r" T lgnn_glm_covariance_chunk_pairs$", out, re.M)
    for cls in (lg.HipGGN, lg.HipEF):
        assert callable(getattr(cls, "glm_covariance"))
    assert callable(lg.engine.GraphEngine.glm_covariance)


@pytest.mark.parametrize("structure", ("kron", "diag"))
@pytest.mark.parametrize("name", NAMES)
def test_device_operands_describe_the_same_posterior(name, structure):
    """``_covariance_operands`` -- what ``lgnn_glm_covariance`` is handed -- evaluated in fp64 on the host: per block rotate by
    ``Q_B^T . Q_A``, scale one side by ``S``; against ``functional_covariance`` of the same Jacobians."""
    _, la = fitted(name, structure)
    ops = la._covariance_operands()
    assert ops is not None and len(ops["S"]) == len(la.params) // 2
    M, C, P = 4, la.n_outputs, la.n_params
    Js = torch.randn(M, C, P, generator=torch.Generator().manual_seed(5))
    J, off, cols, scale = Js.double().reshape(M * C, P), 0, [], []
    for QA, QB, S in zip(ops["QA"], ops["QB"], ops["S"]):
        dout, din = S.shape[0], S.shape[1] - 1
        Jw, Jb = J[:, off:off + dout * din].reshape(-1, dout, din), J[:, off + dout * din:off + dout * din + dout]
        off += dout * din + dout
        assert (QA is None) == (QB is None) == (structure == "diag")
        if QA is not None:
            assert QA.shape == (din, din) and QB.shape == (dout, dout)
            Jw, Jb = torch.einsum("ok,roi,ij->rkj", QB.double(), Jw, QA.double()), Jb @ QB.double()
        cols += [Jw.reshape(M * C, -1), Jb]
        scale += [S[:, :din].double().reshape(-1), S[:, din].double()]
    assert off == P
    Jr = torch.cat(cols, 1)
    e = rel(((Jr * torch.cat(scale)) @ Jr.T).numpy(), la.functional_covariance(Js).numpy())
    print(f"{name} {structure}: operands vs functional_covariance {e:.2e}")
    assert e <= RTOL


def test_operands_are_refused_where_the_device_route_does_not_apply():
    _, la = fitted("gcn_small_1batch_s0", "full")
    assert la._covariance_operands() is None and la._glm_covariance_device(torch.arange(3), None) is None
    g = np.load(os.path.join(GOLDEN, "gcn_small_1batch_s0.npz"))
    loader = lg.TensorBatchLoader(torch.from_numpy(g["train_idx"]), torch.from_numpy(g["train_y"]), int(g["batch_size"]))
    damped = lg.KronLaplace(_cpu_model(g), "classification", backend=OracleBackend, damping=True)
    damped.fit(loader)
    assert damped._covariance_operands() is None
    x = torch.from_numpy(g["pred_idx"][:4])
    K = damped.glm_covariance(x)  # the Jacobian route serves it
    Js = damped.backend.jacobians(x)[0]
    assert rel(K.numpy(), damped.functional_covariance(Js).numpy()) <= 1e-6


def _check_joint_against_fp64(la, x, P64):
    """``joint=True`` and ``glm_covariance`` of a fitted posterior against fp64 ``J P^-1 J^T`` from its backend's Jacobians and
    the materialised precision ``P64``; the diagonal blocks against the marginal predictive."""
    C = la.n_outputs
    Js, f = la.backend.jacobians(x)
    J64 = Js.double().reshape(-1, Js.shape[-1])
    want = J64 @ torch.linalg.solve(P64, J64.T)
    f_mu, f_cov = la._glm_predictive_distribution(x, joint=True)
    assert f_cov.shape == (len(x) * C, len(x) * C) and torch.equal(f_cov, f_cov.T) and torch.equal(f_mu, f.flatten())
    blocks = torch.stack([f_cov[n * C:(n + 1) * C, n * C:(n + 1) * C] for n in range(len(x))])
    e, e_var = rel(f_cov.numpy(), want.numpy()), rel(blocks.numpy(), la._glm_predictive_distribution(x)[1].numpy())
    cross = la.glm_covariance(x[:3], x[2:])
    e_cross = rel(cross.numpy(), want[:3 * C, 2 * C:].numpy())
    assert e <= RTOL and e_var <= 1e-5 and e_cross <= RTOL, (e, e_var, e_cross)
    return e, e_var, e_cross


@pytest.mark.parametrize("structure", STRUCTURES)
def test_last_layer_posteriors_joint_predictive(structure):
    from lastlayer_reference import LastLayerOracleBackend

    g = np.load(os.path.join(GOLDEN, "gcn_small_1batch_s0.npz"))
    loader = lg.TensorBatchLoader(torch.from_numpy(g["train_idx"]), torch.from_numpy(g["train_y"]), int(g["batch_size"]))
    la = lg.Laplace(_cpu_model(g), "classification", "last_layer", structure, backend=LastLayerOracleBackend, prior_precision=0.7)
    la.fit(loader)
    assert la._covariance_operands() is None
    errs = _check_joint_against_fp64(la, torch.tensor([1, 2, 3, 2, 7]), precision64(la, structure))
    print(f"last layer {structure}: vs fp64 {errs[0]:.2e}, blocks vs marginal {errs[1]:.2e}, cross {errs[2]:.2e}")


@pytest.mark.parametrize("structure", ("full", "diag"))
def test_subnetwork_posteriors_joint_predictive(structure):
    from test_subnet_host import _fit

    _, _, la, idx, _ = _fit("sage_small_1batch_s0", "rand", structure)
    assert la._covariance_operands() is None
    errs = _check_joint_against_fp64(la, torch.tensor([1, 2, 3, 2, 7]), precision64(la, structure))
    print(f"subnetwork {structure} (S = {idx.numel()}): vs fp64 {errs[0]:.2e}, blocks vs marginal {errs[1]:.2e}, cross {errs[2]:.2e}")
