"""Drop-in proof: the backend class of this package, ``laplace_gnn_amd.HipGGN``, UNMODIFIED,
handed as ``backend=`` to a ``Laplace`` front -- constructor kwargs (baselaplace.py:175-190), return types (``self.H +=
H_batch`` at :852 goes through the host's ``Kron.__add__``, laplace/utils/matrix.py:85-86), conventions (A rescaled by M/N,
factor, fresh tensors) and results against the goldens the reference produced with its own CurvlinopsGGN backend.

Self-contained: the front is this package's own (the reference's class layout, string-keyed factory and ``backend=`` /
``backend_kwargs=`` arguments), and the host application's container module ``laplace.utils.matrix`` is a stand-in written
here (``host_matrix``) whose ``Kron.__add__`` accepts only its own class -- the contract ``curvature._kron_class`` bridges.

There is no GPU here: the engine behind the backend is the CPU oracle stand-in (tests/oracle_engine.py, same Python
surface as ``GraphEngine``); on a GPU box the engine is the HIP library and these same code lines of ``HipGGN`` run
(tests/test_gpu_frontend.py)."""
import os
import sys
import types

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from conftest import GOLDEN

import laplace_gnn_amd as lg
from laplace_gnn_amd import laplace as front
from laplace_gnn_amd import matrix as front_matrix
from test_host_logic import _cpu_model, rel

RTOL = 1e-4


@pytest.fixture(scope="module")
def ref():
    """The front the backend class is handed to: classes, factory and containers under the names the tests use."""
    return types.SimpleNamespace(laplace_factory=lg.Laplace, baselaplace=front, matrix=front_matrix)


@pytest.fixture
def host_matrix(monkeypatch):
    """A host application's ``laplace.utils.matrix`` loaded in this process: its own ``Kron`` (a weight [out, in] has the
    factors [out x out, in x in], a bias one [out x out]) whose ``__add__`` refuses any other class.  Removed again after
    the test."""

    class HostKron:
        def __init__(self, kfacs):
            self.kfacs = kfacs

        @classmethod
        def init_from_model(cls, params, device):
            kfacs = []
            for p in params:
                dims = [p.shape[0]] if p.ndim == 1 else [p.shape[0], p.shape[1]]
                kfacs.append([torch.zeros(d, d, device=device) for d in dims])
            return cls(kfacs)

        def __add__(self, other):
            if not isinstance(other, HostKron):
                raise ValueError("Can only add Kron to Kron.")
            return HostKron([[a.add(b) for a, b in zip(F, G)] for F, G in zip(self.kfacs, other.kfacs)])

    mod = types.ModuleType("laplace.utils.matrix")
    mod.Kron = HostKron
    monkeypatch.setitem(sys.modules, "laplace.utils.matrix", mod)
    return mod


def _loader(g, y_key="train_y"):
    return DataLoader(TensorDataset(torch.from_numpy(g["train_idx"]), torch.from_numpy(g[y_key])),
                      batch_size=int(g["batch_size"]), shuffle=False)  # gnn/marglik_training.py:125-127


@pytest.mark.parametrize("name", ["gcn_small_3batch_s1", "sage_small_3batch_s1", "gcn_small_isolated_s0",
                                  "gcn3_small_3batch_sym_s1", "sage3_small_3batch_s1",
                                  "gcn_resln_small_3batch_s1", "sage_resln_small_3batch_s1", "sage_resbn_small_1batch_s4"])
def test_reference_kron_and_diag_laplace_run_on_the_hip_backend_class(ref, name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    model = _cpu_model(g)
    la = ref.laplace_factory(model, "classification", subset_of_weights="all", hessian_structure="kron",
                             backend=lg.HipGGN)
    assert type(la) is ref.baselaplace.KronLaplace
    la.fit(_loader(g))
    be = la.backend
    # constructor contract (baselaplace.py:175-190): class(model, likelihood, dict_key_x=, dict_key_y=, **backend_kwargs)
    assert type(be) is lg.HipGGN and be.model is model and be.likelihood == "classification"
    assert (be.dict_key_x, be.dict_key_y, be.last_layer, be.stochastic) == ("input_ids", "labels", False, False)
    assert be.factor == 1.0 and isinstance(be.lossfunc, torch.nn.CrossEntropyLoss)
    assert [tuple(p.shape) for p in be.params] == [tuple(p.shape) for p in la.params]
    # the accumulated factors are the REFERENCE's container (its own __add__ accepted every batch of ours)
    assert type(la.H_facs) is ref.matrix.Kron and type(la.H) is ref.matrix.KronDecomposed
    assert len(la.H_facs.kfacs) == int(g["kron_n_blocks"])
    for i, Fs in enumerate(la.H_facs.kfacs):
        for j, Hm in enumerate(Fs):
            assert rel(Hm.numpy(), g[f"kron_{i}_{j}"]) < RTOL, (i, j)
    assert abs(float(la.loss) - float(g["kron_loss"])) < RTOL * float(g["kron_loss"])
    assert (la.n_data, la.n_outputs, la.n_params) == (int(g["n_data"]), int(g["n_outputs"]), int(g["n_params"]))
    assert [c[0] for c in model.engine.calls] == ["kfac"] * len(_loader(g))
    # downstream of the path everything is the reference's own code on our factors
    assert abs(float(la.log_marginal_likelihood()) - float(g["kron_marglik_pp1"])) < 2e-4 * abs(float(g["kron_marglik_pp1"]))
    pp = torch.from_numpy(g["kron_prior_layerwise"])
    assert abs(float(la.log_marginal_likelihood(prior_precision=pp)) - float(g["kron_marglik_layerwise"])) \
        < 2e-4 * abs(float(g["kron_marglik_layerwise"]))

    ld = ref.laplace_factory(model, "classification", subset_of_weights="all", hessian_structure="diag",
                             backend=lg.HipGGN)
    assert type(ld) is ref.baselaplace.DiagLaplace
    ld.fit(_loader(g))
    assert rel(ld.H.numpy(), g["diag_H"]) < RTOL
    assert abs(float(ld.loss) - float(g["diag_loss"])) < RTOL * float(g["diag_loss"])
    assert abs(float(ld.log_marginal_likelihood()) - float(g["diag_marglik_pp1"])) < 2e-4 * abs(float(g["diag_marglik_pp1"]))


def test_backend_returns_fresh_tensors_of_both_container_types(host_matrix):
    """With a host application's container module loaded, ``kron()`` hands out an object that the host's ``Kron.__add__``
    accepts (isinstance of ITS class) and that this package's front accepts too; callers mutate the result (``self.H += ``,
    ``F[1] *= ``), so every call returns fresh tensors."""
    g = np.load(os.path.join(GOLDEN, "gcn_small_1batch_s0.npz"))
    model = _cpu_model(g)
    be = lg.HipGGN(model, "classification")
    x, y = torch.from_numpy(g["train_idx"]), torch.from_numpy(g["train_y"])
    l1, k1 = be.kron(x, y, N=len(x))
    l2, k2 = be.kron(x, y, N=len(x))
    assert isinstance(k1, host_matrix.Kron) and isinstance(k1, lg.Kron)
    assert [[t.shape for t in F] for F in k1.kfacs] == [[t.shape for t in F] for F in
                                                         host_matrix.Kron.init_from_model(be.params, "cpu").kfacs]
    for Fa, Fb in zip(k1.kfacs, k2.kfacs):
        for a, b in zip(Fa, Fb):
            assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)
    k1.kfacs[0][0].mul_(0)  # mutating one result leaves the other (and the next call) intact
    assert float(k2.kfacs[0][0].abs().sum()) > 0
    zero = host_matrix.Kron.init_from_model(be.params, "cpu")
    acc = zero + k2  # the host's __add__
    assert type(acc) is host_matrix.Kron
    acc2 = lg.Kron.init_from_model(be.params, "cpu") + k2  # this package's __add__
    assert type(acc2) is lg.Kron and torch.equal(acc2.kfacs[0][0], acc.kfacs[0][0])
    assert torch.is_tensor(l1) and l1.ndim == 0


def test_reference_override_false_and_predictive_on_the_hip_backend_class(ref):
    """KronLaplace.fit(override=False) discounting (baselaplace.py:1589-1607) and the GLM predictive
    (``backend.jacobians``, :1123-1158) of the REFERENCE front with our backend, against the reference's goldens."""
    g = np.load(os.path.join(GOLDEN, "gcn_small_1batch_s0.npz"))
    model = _cpu_model(g)
    la = ref.baselaplace.KronLaplace(model, "classification", backend=lg.HipGGN)
    la.fit(_loader(g))
    facs1 = [[h.clone() for h in F] for F in la.H_facs.kfacs]
    la.fit(_loader(g), override=False)
    for F1, F2 in zip(facs1, la.H_facs.kfacs):  # B doubles, A = 0.5 A + 0.5 A
        assert rel(F2[0].numpy(), 2 * F1[0].numpy()) < 1e-5
        if len(F1) == 2:
            assert rel(F2[1].numpy(), F1[1].numpy()) < 1e-5
    la.fit(_loader(g))
    eval_idx = torch.from_numpy(g["pred_idx"])
    f_mu, f_var = la._glm_predictive_distribution(eval_idx)
    assert rel(f_mu.numpy(), g["kron_glm_fmu"]) < RTOL and rel(f_var.numpy(), g["kron_glm_fvar"]) < 1e-3
    assert rel(la(eval_idx, pred_type="glm", link_approx="probit").numpy(), g["kron_glm_probit"]) < 1e-3


def test_reference_regression_and_full_laplace_on_the_hip_backend_class(ref):
    g = np.load(os.path.join(GOLDEN, "sage_small_1batch_s0.npz"))
    model = _cpu_model(g)
    lr = ref.baselaplace.KronLaplace(model, "regression", sigma_noise=0.7, backend=lg.HipGGN)
    lr.fit(_loader(g, "reg_y"))
    assert lr.backend.factor == 0.5 and isinstance(lr.backend.lossfunc, torch.nn.MSELoss)
    for i, Fs in enumerate(lr.H_facs.kfacs):
        for j, Hm in enumerate(Fs):
            assert rel(Hm.numpy(), g[f"reg_kron_{i}_{j}"]) < RTOL, (i, j)
    assert abs(float(lr.loss) - float(g["reg_kron_loss"])) < RTOL * abs(float(g["reg_kron_loss"]))
    ldr = ref.baselaplace.DiagLaplace(model, "regression", sigma_noise=0.7, backend=lg.HipGGN)
    ldr.fit(_loader(g, "reg_y"))
    assert rel(ldr.H.numpy(), g["reg_diag_H"]) < RTOL
    assert abs(float(ldr.loss) - float(g["reg_diag_loss"])) < RTOL * abs(float(g["reg_diag_loss"]))
    lf = ref.baselaplace.FullLaplace(model, "classification", backend=lg.HipGGN)
    lf.fit(_loader(g))
    assert rel(lf.H.numpy(), g["fullla_H"]) < RTOL
    assert abs(float(lf.log_marginal_likelihood()) - float(g["fullla_marglik_pp1"])) < 2e-4 * abs(float(g["fullla_marglik_pp1"]))


def test_reference_rejects_nothing_about_the_class_name(ref):
    """baselaplace.py:142-149 refuses backends whose class name contains 'backpack' / 'asdfghjkl' once a parameter is
    excluded; ours must not trip that."""
    assert "backpack" not in lg.HipGGN.__name__.lower() and "asdfghjkl" not in lg.HipGGN.__name__.lower()


def test_reference_fronts_run_on_the_empirical_and_mc_fisher_backends(ref):
    """``backend=HipEF`` (the CurvlinopsEF counterpart) and ``backend=HipGGN, backend_kwargs=dict(stochastic=True)`` inside
    the reference's own KronLaplace / DiagLaplace, against the goldens of the reference's own EF / MC backends."""
    g = np.load(os.path.join(GOLDEN, "gcn_small_1batch_s0.npz"))
    model = _cpu_model(g)
    le = ref.baselaplace.KronLaplace(model, "classification", backend=lg.HipEF)
    le.fit(_loader(g))
    for i, Fs in enumerate(le.H_facs.kfacs):
        for j, Hm in enumerate(Fs):
            assert rel(Hm.numpy(), g[f"ef_kron_{i}_{j}"]) < RTOL, (i, j)
    ld = ref.baselaplace.DiagLaplace(model, "classification", backend=lg.HipEF)
    ld.fit(_loader(g))
    assert rel(ld.H.numpy(), g["ef_diag_fit"]) < RTOL
    S = int(g["mc_samples"])
    draws = [torch.from_numpy(g[f"mc_labels_0_{s}"]) for s in range(S)]
    lm = ref.baselaplace.KronLaplace(model, "classification", backend=lg.HipGGN, backend_kwargs=dict(stochastic=True),
                                     asdl_fisher_kwargs=dict(mc_labels=draws))
    lm.fit(_loader(g))
    assert lm.backend.stochastic
    for i, Fs in enumerate(lm.H_facs.kfacs):
        for j, Hm in enumerate(Fs):
            assert rel(Hm.numpy(), g[f"mc_kron_{i}_{j}"]) < RTOL, (i, j)
