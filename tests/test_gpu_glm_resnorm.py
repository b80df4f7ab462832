"""Matrix-free GLM predictive of 2-layer models built with res / norm (csrc/predictive.hip, lgnn_glm_variance_ext): the
per-class table route against this package's Jacobian route, the reference's goldens and, on plain models, the entry point
plain models always had.  Tolerance: rel < 1e-4 (the bar tests/test_gpu_frontend.py holds for the same comparison on plain
models), f_mu 1e-6."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_utils import rel

pytestmark = pytest.mark.gpu
RTOL = 1e-4
FIXTURES = ["gcn_bn_small_3batch_s3", "gcn_ln_small_3batch_sym_s7", "gcn_res_small_3batch_s2", "gcn_resln_mid_2batch_s0",
            "gcn_resln_small_1batch_s0", "gcn_resln_small_3batch_s1", "sage_ln_mid_2batch_s1", "sage_resbn_small_1batch_s4",
            "sage_resln_small_1batch_s0", "sage_resln_small_3batch_s1"]
KRON_PRIOR = [0.5, 2.0, 1.5, 0.25, 3.0, 0.125]  # one entry per block: convs.0.{W,b}, convs.1.{W,b}, res.0.{W,b}


def _golden_setup(name):
    import laplace_gnn_amd as lg
    from test_gpu_frontend import model_from_golden

    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    model = model_from_golden(g)
    loader = lg.TensorBatchLoader(torch.from_numpy(g["train_idx"]).cuda(), torch.from_numpy(g["train_y"]).cuda(),
                                  batch_size=int(g["batch_size"]))
    return g, model, loader, torch.from_numpy(g["pred_idx"]).cuda()


def _jacobian_route(la, x, E=None):
    Js, f = la.backend.jacobians(x)
    S = la.functional_variance(Js)
    if E is not None:
        S = E @ S @ E.T
    return f, torch.diagonal(S, dim1=1, dim2=2)


# ---- 1. golden fixtures ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_res_norm_fixtures_match_the_jacobian_route_and_the_reference(name):
    import laplace_gnn_amd as lg

    g, model, loader, x = _golden_setup(name)
    nb = 6 if bool(g["res"]) else 4
    for cls, key in ((lg.KronLaplace, "kron"), (lg.DiagLaplace, "diag")):
        la = cls(model, "classification")
        la.fit(loader)
        for pp in (1.0, torch.tensor(KRON_PRIOR[:nb]) if cls is lg.KronLaplace else 0.7):
            la.prior_precision = pp
            fast = la._glm_variance_matrix_free(x)
            assert fast is not None, "2-layer res / norm models take the matrix-free route"
            f_mu, f_vd = fast
            f_j, ref = _jacobian_route(la, x)
            assert rel(f_mu.cpu().numpy(), f_j.cpu().numpy()) < 1e-6
            assert rel(f_vd.cpu().numpy(), ref.cpu().numpy()) < RTOL, (key, pp)
        la.prior_precision = 1.0
        f_mu, f_vd = la._glm_variance_matrix_free(x)
        assert rel(f_vd.cpu().numpy(), np.diagonal(g[key + "_glm_fvar"], axis1=1, axis2=2)) < RTOL, key
        assert rel(la(x, link_approx="probit").cpu().numpy(), g[key + "_glm_probit"]) < RTOL, key
    model.engine.check_async_errors()


# ---- 2. mapped outputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gcn_resln_mid_2batch_s0", "sage_ln_mid_2batch_s1"])
def test_mapped_outputs_and_the_bridge_links_of_res_norm_models(name):
    import laplace_gnn_amd as lg

    g, model, loader, x = _golden_setup(name)
    C = int(g["n_outputs"])
    for cls, key in ((lg.KronLaplace, "kron"), (lg.DiagLaplace, "diag")):
        la = cls(model, "classification")
        la.fit(loader)
        for rows in (3, 11):  # fewer and more rows than classes
            E = torch.from_numpy(np.random.default_rng(rows).standard_normal((rows, C)).astype(np.float32)).cuda()
            fast = la._glm_variance_matrix_free(x, out_map=E)
            assert fast is not None
            f_j, ref = _jacobian_route(la, x, E)
            assert fast[1].shape == (x.shape[0], rows)
            assert rel(fast[0].cpu().numpy(), f_j.cpu().numpy()) < 1e-6
            assert rel(fast[1].cpu().numpy(), ref.cpu().numpy()) < RTOL, (key, rows)
        moments = la._bridge_moments_matrix_free(x)
        assert moments is not None
        f_mu, diag, rsum, total = (t.cpu().numpy() for t in moments)
        gold = g[key + "_glm_fvar"]
        assert rel(diag, np.diagonal(gold, axis1=1, axis2=2)) < RTOL, key
        assert rel(rsum, gold.sum(-1)) < RTOL and rel(total, gold.sum((1, 2))) < RTOL, key
        for link in ("bridge", "bridge_norm"):
            assert rel(la(x, link_approx=link).cpu().numpy(), g[f"{key}_glm_{link}"]) < RTOL, (key, link)
    model.engine.check_async_errors()


# ---- 3. kernel edges -----------------------------------------------------------------------------------------------------
N_SYN = 300


def _edge_graph(seed):
    """Node 0: 60 neighbours (61 staged entries: two staging passes of 48); node 1: 47 (48 staged); node 2: 48 (49 staged, on
    GraphSAGE the 49th is the node itself); node 3: no edges.  staged = neighbours + 1 for both families (the GCN's self loop
    resp. GraphSAGE's self entry).  Random edges among the remaining nodes only; the graph is symmetrised."""
    src = [0] * 60 + [1] * 47 + [2] * 48
    dst = list(range(10, 70)) + list(range(70, 117)) + list(range(117, 165))
    rng = np.random.default_rng(seed)
    rest = rng.integers(165, N_SYN, size=(2, 500))
    ei = np.concatenate([np.array([src, dst]), rest], axis=1).astype(np.int64)
    idx = np.concatenate([[0, 1, 2, 3, 0, 10, 70, 117, 164], rng.choice(np.arange(165, N_SYN), 7, replace=False)])
    return torch.from_numpy(ei), torch.from_numpy(idx.astype(np.int64))


def _synthetic(kind, F, H, C, norm, res, seed):
    import laplace_gnn_amd as lg

    ei, idx = _edge_graph(seed)
    gen = torch.Generator().manual_seed(seed)
    X = torch.randn(N_SYN, F, generator=gen)
    torch.manual_seed(seed)
    model = (lg.GCN if kind == "gcn" else lg.GraphSAGE)(F, H, C, 2, X, ei, symmetric=True, norm=norm, res=res)
    with torch.no_grad():
        for nm in (model.norms if norm else []):  # away from the defaults (1, 0, running mean 0 / var 1)
            nm.weight.copy_(1.0 + 0.3 * torch.randn(H, generator=gen))
            nm.bias.copy_(0.2 * torch.randn(H, generator=gen))
            if norm == "batch":
                nm.running_mean.copy_(0.3 * torch.randn(H, generator=gen))
                nm.running_var.copy_(0.5 + torch.rand(H, generator=gen))
    model.eval()
    model = model.to("cuda")
    tr = torch.randperm(N_SYN, generator=gen)[:100]
    y = torch.randint(0, C, (100,), generator=gen)
    return model, lg.TensorBatchLoader(tr.cuda(), y.cuda(), batch_size=50), idx.cuda()


def test_the_edge_graph_has_the_rows_the_kernel_cases_need():
    import laplace_gnn_amd as lg

    ei, idx = _edge_graph(0)
    eng = lg.GraphEngine(ei.cuda(), N_SYN, kind="gcn", symmetric=True)
    r, _, _ = eng.export_propagation()
    staged = torch.bincount(r.cpu(), minlength=N_SYN)  # the GCN's rows hold the self loop
    assert [int(staged[i]) for i in range(4)] == [61, 48, 49, 1]
    assert (idx == 0).sum() == 2 and int(idx.max()) < N_SYN
    eng.close()


@pytest.mark.parametrize("shape", [(150, 136, 5), (20, 20, 3)], ids=["F150_H136_C5", "F20_H20_C3"])
@pytest.mark.parametrize("norm,res", [("layer", True), ("layer", False), ("batch", True), (None, True), (None, False)],
                         ids=["ln_res", "ln", "bn_res", "res", "plain"])
@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_kernel_edges_against_the_jacobian_route(kind, norm, res, shape):
    """Hp = 256 with two (GCN) / three (GraphSAGE) ragged column chunks and a padded X (F % 4 = 2) resp. Hp = 64 with 44 idle
    rows and LayerNorm reductions over 20 channels; rows with two staging passes, exactly 48 and 49 staged entries, a node
    without edges and a repeated id.  Both posteriors, prior precision 2.0.  ``plain``: the same graph through the plain entries
    (lgnn_glm_variance): table rows under the Kronecker posterior, in-loop rows and E read in place (row stride of the
    forward, not a multiple of 4 at F = 150) under the diagonal one."""
    import laplace_gnn_amd as lg

    F, H, C = shape
    model, loader, idx = _synthetic(kind, F, H, C, norm, res, seed=11)
    for cls in (lg.KronLaplace, lg.DiagLaplace):
        la = cls(model, "classification", prior_precision=2.0)
        la.fit(loader)
        fast = la._glm_variance_matrix_free(idx)
        assert fast is not None
        f_j, ref = _jacobian_route(la, idx)
        assert rel(fast[0].cpu().numpy(), f_j.cpu().numpy()) < 1e-6
        err = rel(fast[1].cpu().numpy(), ref.cpu().numpy())
        print(kind, norm, res, shape, cls.__name__, "rel", err)
        assert err < RTOL, cls.__name__
        assert rel(fast[1][4].cpu().numpy(), fast[1][0].cpu().numpy()) < 1e-6  # the repeated id (LDS sums: last bits)
    model.engine.check_async_errors()
    model.engine.close()


# ---- 4. the ext entry on a plain model -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gcn_mid_1batch_s0", "sage_mid_2batch_s2"])
def test_ext_entry_on_a_plain_model_equals_the_plain_entry(name):
    """The table route of the new kernel instantiations without any norm arithmetic: q = d * w."""
    import laplace_gnn_amd as lg

    g, model, loader, x = _golden_setup(name)
    C = int(g["n_outputs"])
    E = torch.from_numpy(np.random.default_rng(5).standard_normal((C + 3, C)).astype(np.float32)).cuda()
    for cls in (lg.KronLaplace, lg.DiagLaplace):
        la = cls(model, "classification", prior_precision=2.0)
        la.fit(loader)
        for out_map in (None, E):
            ops = la._matrix_free_operands(out_map)
            mu_a, var_a = model.engine.glm_variance(x, out_map=out_map, **ops)
            mu_b, var_b = model.engine.glm_variance_ext(x, out_map=out_map, **ops)
            assert torch.equal(mu_a, mu_b)
            assert rel(var_b.cpu().numpy(), var_a.cpu().numpy()) < 1e-5, (cls.__name__, out_map is not None)
    model.engine.check_async_errors()


# ---- 5. no Jacobians -----------------------------------------------------------------------------------------------------
def test_every_link_of_a_res_layernorm_model_runs_without_jacobians():
    import laplace_gnn_amd as lg

    g, model, loader, x = _golden_setup("gcn_resln_small_3batch_s1")

    def no_jacobians(*a, **k):
        raise AssertionError("the GLM predictive of a 2-layer res / norm model must not form Jacobians")

    for cls in (lg.KronLaplace, lg.DiagLaplace):
        la = cls(model, "classification")
        la.fit(loader)
        la.backend.jacobians = no_jacobians
        for kw in ({}, {"link_approx": "bridge"}, {"link_approx": "bridge_norm"},
                   {"link_approx": "mc", "diagonal_output": True}):
            out = la(x, **kw)
            assert out.shape == (x.shape[0], la.n_outputs)
            assert torch.allclose(out.sum(dim=1), torch.ones_like(out[:, 0]), atol=1e-5), kw
    model.engine.check_async_errors()


# ---- 6. flagged id -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gcn_resln_small_3batch_s1", "sage_resln_small_3batch_s1", "gcn_mid_1batch_s0",
                                  "sage_mid_2batch_s2"])
def test_an_id_out_of_range_is_flagged_and_leaves_the_other_rows_alone(name):
    import laplace_gnn_amd as lg
    from laplace_gnn_amd._lib import HipLibraryError

    g, model, loader, x = _golden_setup(name)
    for cls in (lg.KronLaplace, lg.DiagLaplace):
        la = cls(model, "classification")
        la.fit(loader)
        _, good = la._glm_variance_matrix_free(x)
        model.engine.check_async_errors()
        bad = torch.cat([x[:3], torch.tensor([int(g["num_nodes"])], device="cuda"), x[3:]])
        _, var = la._glm_variance_matrix_free(bad)
        with pytest.raises(HipLibraryError, match="node index"):
            model.engine.check_async_errors()
        assert torch.count_nonzero(var[3]) == 0
        assert rel(torch.cat([var[:3], var[4:]]).cpu().numpy(), good.cpu().numpy()) < 1e-6
        model.engine.check_async_errors()  # the flag was reported once; the context stays usable
