"""CPU test (no GPU): the operands ``_matrix_free_operands()`` packs for ``GraphEngine.glm_variance_ext`` on 2-layer models
with res / norm -- block order convs.0.{W,b}, convs.1.{W,b}, res.0.{W,b}, the ``Sr`` packing, per-block priors, ``out_map`` --
contracted here in fp64 numpy with the closed-form tiles of csrc/predictive.hip (built from the oracle's ``forward_ext``),
against this package's Jacobian route and the reference's golden f_var.  Fit and Jacobians come from the oracle stand-in
backend (tests/oracle_backend.py), as in tests/test_reference_dropin.py."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle_backend import OracleBackend

import gnn_laplace_oracle as O
import laplace_gnn_amd as lg
from test_host_logic import _cpu_model, rel

RTOL = 1e-4
NAMES = ["gcn_resln_small_3batch_s1", "gcn_ln_small_3batch_sym_s7", "sage_resln_small_3batch_s1"]


def closed_form_variance(om, idx, ops, W1m=None):
    """diag(J P^-1 J^T) [M, C] of the operands ``ops`` from the closed-form first-layer tiles
    M_c = sum_u P[a,u] q_{u,c} (x) [z_u | bias_u] per block (conv: z = e, bias = rho; res: z = x, bias = 1), fp64."""
    f64 = np.float64
    fw = O.forward_ext(om)
    sage = om.kind == "sage"
    P = om.P.tocsr()
    X = om.X.astype(f64)
    n0 = fw["pre"][0].astype(f64)
    d = (n0 > 0).astype(f64)
    h1 = np.maximum(n0, 0.0)
    N, H = n0.shape
    if sage:
        E, rho = fw["lin_in"][0].astype(f64), np.ones(N)
        phi_all, s_all = fw["lin_in"][1].astype(f64), np.ones(N)
    else:
        rho = np.asarray(P.sum(axis=1)).reshape(-1).astype(f64)
        E = np.asarray(P @ X)
        phi_all, s_all = np.asarray(P @ h1), rho
    W1 = (om.weights[1] if W1m is None else W1m).astype(f64)
    wn, ws = (W1[:, H:], W1[:, :H]) if sage else (W1, None)
    C = W1.shape[0]
    gamma = om.norm_weight[0].astype(f64) if om.norm else None
    xh = fw["xhat"][0].astype(f64) if om.norm else None
    rstd = fw["rstd"][0].astype(f64) if om.norm else None

    def q(u, w):  # [C, H]: norm_u^T (d_u * w_c)
        g = d[u][None, :] * w
        if om.norm == "layer":
            g = g * gamma
            return rstd[u] * (g - g.mean(1, keepdims=True) - xh[u] * (g * xh[u]).mean(1, keepdims=True))
        if om.norm == "batch":
            return g * gamma * rstd.reshape(-1)
        return g

    np64 = lambda t: None if t is None else t.detach().cpu().numpy().astype(f64)  # noqa: E731
    o = {k: np64(v) for k, v in ops.items()}
    kron = o.get("QA0") is not None
    blocks = [(E, rho, o["S0"], o.get("QA0"), o.get("QB0"))]
    if "Sr" in o:
        blocks.append((X, np.ones(N), o["Sr"], o.get("QAr"), o.get("QBr")))
    out = np.zeros((len(idx), C))
    for m, a in enumerate(idx):
        a = int(a)
        entries = [(int(u), float(p), wn) for u, p in zip(P.indices[P.indptr[a]:P.indptr[a + 1]], P.data[P.indptr[a]:P.indptr[a + 1]])]
        if sage:
            entries.append((a, 1.0, ws))
        var = np.zeros(C)
        for Z, bias, S, QA, QB in blocks:
            Mt = np.zeros((C, H, Z.shape[1] + 1))
            for u, p, w in entries:
                qq, z = q(u, w), Z[u]
                if kron:
                    qq, z = qq @ QB, z @ QA
                Mt += p * qq[:, :, None] * np.concatenate([z, [bias[u]]])[None, None, :]
            var += (Mt * Mt * S[None]).sum((1, 2))
        phi = phi_all[a]
        if kron:
            pt = phi @ o["QA1"]
            var += o["QB1sq"] @ (o["S1"] @ (pt * pt))
        else:
            var += o["S1"] @ (phi * phi)
        out[m] = var + s_all[a] ** 2 * o["kappa"]
    return out


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("structure", ["kron", "diag"])
def test_operands_of_res_norm_models_contract_to_the_jacobian_route(name, structure):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    model = _cpu_model(g)
    om = model.oracle_model()
    res = bool(g["res"])
    loader = lg.TensorBatchLoader(torch.from_numpy(g["train_idx"]), torch.from_numpy(g["train_y"]), int(g["batch_size"]))
    la = lg.Laplace(model, "classification", subset_of_weights="all", hessian_structure=structure, backend=OracleBackend)
    la.fit(loader)
    x = torch.from_numpy(g["pred_idx"])
    Js, _ = la.backend.jacobians(x)
    nb = 6 if res else 4

    def jac_route(E=None):
        S = la.functional_variance(Js).double()
        if E is not None:
            S = E.double() @ S @ E.double().T
        return torch.diagonal(S, dim1=1, dim2=2).numpy()

    # prior 1: the Jacobian route and the reference's golden
    ops = la._matrix_free_operands()
    assert ops is not None, "the matrix-free route must take 2-layer res / norm models"
    assert ("Sr" in ops) == res
    if res:
        Hd, F = g["Wr0"].shape
        assert tuple(ops["Sr"].shape) == (Hd, F + 1)
        assert (structure == "kron") == ("QAr" in ops and "QBr" in ops)
    got = closed_form_variance(om, g["pred_idx"], ops)
    assert rel(got, jac_route()) < RTOL
    assert rel(got, np.diagonal(g[structure + "_glm_fvar"], axis1=1, axis2=2)) < RTOL
    # per-block prior (one entry per block: pins the block order) resp. a scalar != 1
    if structure == "kron":
        la.prior_precision = torch.tensor([0.5, 2.0, 1.5, 0.25, 3.0, 0.125][:nb])
    else:
        la.prior_precision = 0.7
    ops = la._matrix_free_operands()
    assert ops is not None
    assert rel(closed_form_variance(om, g["pred_idx"], ops), jac_route()) < RTOL
    # a linear map of the logits
    C = int(g["n_outputs"])
    E = torch.from_numpy(np.random.default_rng(3).standard_normal((C + 2, C)).astype(np.float32))
    ops = la._matrix_free_operands(E)
    W1m = E.numpy() @ g["W1"]
    assert rel(closed_form_variance(om, g["pred_idx"], ops, W1m=W1m), jac_route(E)) < RTOL
