"""The fp64 Hessian helper (tests/hessian_reference.py) pinned to the reference's goldens, and the host side of ``lg.HipHessian``
on a stand-in engine: refusals by name, the header declaration and the binding's signature.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import laplace_gnn_amd as lg
from hessian_reference import F64, HessianReference, propagation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
RTOL = 1e-4  # the goldens' tolerance (tests/test_oracle_golden.py, tests/test_gpu_frontend.py)
FIXTURES = ["gcn_small_1batch_s0", "sage_small_1batch_s0"]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def from_golden(name, likelihood="classification", layers=2):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    kind, N = str(g["kind"]), int(g["num_nodes"])
    P = propagation(kind, g["edge_index"], N)
    Ws, bs = [torch.from_numpy(g[f"W{l}"]) for l in range(2)], [torch.from_numpy(g[f"b{l}"]) for l in range(2)]
    dims = [g["X"].shape[1], Ws[0].shape[0], Ws[1].shape[0]]
    if layers == 1:  # the fixture's first layer alone, its hidden units as classes
        Ws, bs, dims = Ws[:1], bs[:1], dims[:2]
    ref = HessianReference(kind, P, g["X"], dims, "relu", likelihood)
    return g, ref, ref.flatten(Ws, bs)


@pytest.mark.parametrize("name", FIXTURES)
def test_propagation_and_logits_are_the_goldens(name):
    g, ref, theta = from_golden(name)
    want = torch.zeros_like(ref.P)
    want[torch.from_numpy(g["prop_row"]), torch.from_numpy(g["prop_col"])] = torch.from_numpy(g["prop_val"]).to(F64)
    assert float((ref.P - want).abs().max()) <= 1e-6
    assert ref.n_params == int(g["n_params"])
    f = ref.logits(theta)
    assert rel(f[torch.from_numpy(g["train_idx"])], g["f_first_batch"]) < RTOL and rel(f, g["logits"]) < RTOL


@pytest.mark.parametrize("name", FIXTURES)
def test_ggn_part_is_the_goldens_full_ggn_and_the_split_adds_up(name):
    g, ref, theta = from_golden(name)
    idx, y = g["train_idx"], g["train_y"]
    assert rel(ref.jacobians(theta, idx), g["jac_first_batch"]) < RTOL
    ggn, R = ref.split(theta, idx, y)
    assert rel(ggn, g["full_H"]) < RTOL
    H = ref.dense(theta, idx, y)
    scale = float(H.abs().max())
    assert float((R - (H - ggn)).abs().max()) <= 1e-12 * scale
    assert float((H - H.T).abs().max()) <= 1e-12 * scale
    assert float(R.abs().max()) >= 1e-2 * float(ggn.abs().max())  # not a small term away from the MAP
    C = ref.dims[-1]
    assert float(R[-C:].abs().max()) == 0.0  # (RV)_b1 = 0
    V = torch.randn(3, ref.n_params, dtype=F64, generator=torch.Generator().manual_seed(0))
    assert float((ref.hvp(theta, idx, y, V) - V @ H).abs().max()) <= 1e-12 * scale
    assert float((ref.resid_vp(theta, idx, y, V) - V @ R).abs().max()) <= 1e-12 * scale
    assert ref.min_abs_preactivation(theta) > 0.0


@pytest.mark.parametrize("name", FIXTURES)
def test_regression_split(name):
    g, ref, theta = from_golden(name, "regression")
    idx, y = g["train_idx"], g["reg_y"]
    ggn, R = ref.split(theta, idx, y)
    H = ref.dense(theta, idx, y)  # of 0.5 * MSE_sum: factor times the Hessian of the loss function
    assert rel(np.diagonal(ggn.numpy()), g["reg_diag_H"]) < RTOL  # sum J^T J, no factor
    assert float((R - (H - ggn)).abs().max()) <= 1e-12 * float(H.abs().max())
    assert abs(float(ref.loss(theta, idx, y)) - float(g["reg_diag_loss"])) <= RTOL * float(g["reg_diag_loss"])


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("likelihood", ["classification", "regression"])
def test_one_layer_has_no_residual_term(name, likelihood):
    g, ref, theta = from_golden(name, likelihood, layers=1)
    idx = g["train_idx"]
    C = ref.dims[-1]
    gen = torch.Generator().manual_seed(1)
    y = torch.randn(len(idx), C, generator=gen) if likelihood == "regression" else torch.randint(0, C, (len(idx),), generator=gen)
    ggn, R = ref.split(theta, idx, y)
    assert float(R.abs().max()) == 0.0
    assert float((ref.dense(theta, idx, y) - ggn).abs().max()) <= 1e-12 * float(ggn.abs().max())


# ---- host side -------------------------------------------------------------------------------------------------------------
class _Engine:  # a stand-in engine: enough for the constructor
    device = torch.device("cpu")


class _Model(torch.nn.Module):
    n_outputs = 2

    def forward(self, idx):
        return torch.zeros(idx.shape[0], 2)

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(3, 2)
        self.engine = _Engine()


def test_hiphessian_refusals_by_name():
    assert issubclass(lg.HipHessian, lg.HipCurvatureInterface) and "HipHessian" in lg.__all__
    m = _Model()
    with pytest.raises(NotImplementedError, match="last_layer=True.*HipGGN"):
        lg.HipHessian(m, "classification", last_layer=True)
    with pytest.raises(NotImplementedError, match="stochastic=True"):
        lg.HipHessian(m, "classification", stochastic=True)
    with pytest.raises(NotImplementedError, match="subnetwork_indices.*HipHessian"):
        lg.HipHessian(m, "classification", subnetwork_indices=torch.tensor([0, 1]))
    be = lg.HipHessian(m, "regression")
    assert be.factor == 0.5 and not be.last_layer and not be.stochastic
    with pytest.raises(NotImplementedError, match="subnetwork_indices.*HipHessian"):
        be.subnetwork_indices = torch.tensor([0])
    with pytest.raises(NotImplementedError, match="no kron.*CurvlinopsHessian has none"):
        be.kron(None, None, 1)
    with pytest.raises(NotImplementedError, match="no diag.*CurvlinopsHessian has none"):
        be.diag(None, None)
    with pytest.raises(NotImplementedError, match="ggn_matmat.*HipGGN only"):
        be.ggn_matmat([], None)
    with pytest.raises(NotImplementedError, match="eig_lowrank.*positive semi-definite.*indefinite"):
        be.eig_lowrank([])
    with pytest.raises(NotImplementedError, match="HipHessian has no kron"):
        be._kron_fisher_type
    for entry in ("kron_accumulate_", "diag_accumulate_", "full_accumulate_"):  # the GGN's in-place entries
        with pytest.raises(NotImplementedError, match="HipHessian has no " + entry):
            getattr(be, entry)(None, None, None, None)
    for name in ("jacobians", "gradients", "glm_covariance", "sampled_forward"):  # inherited unchanged
        assert getattr(lg.HipHessian, name) is getattr(lg.HipCurvatureInterface, name)
    assert lg.HipHessian.full is not lg.HipCurvatureInterface.full and callable(lg.HipHessian.hessian_matmat)


def test_the_front_routes_hiphessian_and_refuses_the_adjacency_gradient():
    X = torch.randn(12, 4, generator=torch.Generator().manual_seed(0))
    ei = torch.randint(0, 12, (2, 30), generator=torch.Generator().manual_seed(1))
    m = lg.GCN(4, 3, 2, 2, X, ei)
    la = lg.Laplace(m, "classification", "all", "full", backend=lg.HipHessian)
    assert type(la) is lg.FullLaplace and la._backend_cls is lg.HipHessian
    with pytest.raises(NotImplementedError, match="HipHessian"):
        la.neg_marglik_adj_grad([])
    with pytest.raises(NotImplementedError, match="HipHessian"):
        lg.FullLaplace(m, "classification", backend=lg.HipHessian).neg_marglik_adj_grad([])


class _Loader(list):
    dataset = range(4)


@pytest.mark.parametrize("structure", ["kron", "diag"])
def test_the_front_does_not_reach_a_ggn_through_the_in_place_routes(structure):
    """``kron`` is the factory's default structure, and its fit adds in place where the backend offers that: a HipHessian fit
    must refuse there as well, not come back as a GGN posterior."""
    m = _Model()
    batches = _Loader([(torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int64))])
    las = [lg.Laplace(m, "classification", "all", structure, backend=lg.HipHessian)]
    if structure == "kron":
        las += [lg.Laplace(m, "classification", "all", backend=lg.HipHessian),
                lg.KronLaplace(m, "classification", backend=lg.HipHessian)]
    for la in las:
        with pytest.raises(NotImplementedError, match="HipHessian has no " + structure):
            la.fit(batches)
    # (no such posterior can be fitted, so its ``neg_marglik_adj_grad`` stops at "not fitted")


def _c_args(decl):
    inner = decl[decl.index("(") + 1:decl.rindex(")")]
    return [a for a in re.sub(r"/\*.*?\*/", "", inner, flags=re.S).split(",") if a.strip()]


def test_header_declares_the_entry_and_the_binding_matches():
    name = "lgnn_hessian_resid_matmat"
    text = open(os.path.join(ROOT, "include", "laplace_gnn_hip.h")).read()
    m = re.search(r"LGNN_API int " + name + r"\s*\([^;]*\);", text)
    assert m, f"{name} is not declared in the header"
    res, args = lg._lib.SIGNATURES[name]
    assert res is lg._lib._i32 and len(args) == len(_c_args(m.group(0))) == 8
    assert lg._lib.HESSIAN_RESID_MATMAT == name
    assert "curvlinops.py:182-187" in text and "curvlinops/hessian.py" in text
    src = open(os.path.join(ROOT, "laplace-gnn_amd", "csrc", "hessmat.hip")).read()
    d = re.search(r'extern "C" int ' + name + r"\s*\([^{]*\)\s*\{", src)
    assert d and len(_c_args(d.group(0))) == len(args)
    assert "exact Hessian: closed-form models only" in src and "exact Hessian: closed-form models only" in text
    assert "atomicAdd" not in src  # every output element has one writer
    assert "hessmat.hip" in open(os.path.join(ROOT, "laplace-gnn_amd", "csrc", "Makefile")).read()
