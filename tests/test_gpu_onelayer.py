"""One-layer models on the GPU: the adjacency gradient of the marginal likelihood of a one-layer GCN under
the diagonal, Kronecker and full posterior (csrc/adjgrad_onelayer.hip: the ``onelayer_*`` route) against (a) the reference's own
``model.adj.grad`` goldens (tests/golden/onelayer/, tools/make_onelayer_golden.py) and (b) the fp64 restatement
(tests/onelayer_restatement.py, pinned to the same goldens on the CPU), the structure-learning loop of ``lg.STEGCN(..., 1, ...)``
against goldens of the reference's loop, the matrix-free GLM predictive of one-layer GCN / GraphSAGE models
(csrc/predictive.hip) against the Jacobian route of the same fit, and the refusals that stay.

Tolerances are those of the two-layer tests: fixtures value 5e-6 / gradients 1e-5 (tests/test_gpu_adjgrad.py), mid size 1e-4,
the loop 2e-5 / 1e-4 / 1e-4 / exact edge sets (tests/test_gpu_structure.py), predictive variance 1e-4 and f_mu 1e-6
(tests/test_gpu_glm_resnorm.py)."""
import glob
import os

import numpy as np
import pytest
import torch

import onelayer_restatement as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
ONE = os.path.join(GOLDEN, "onelayer")
CASES = sorted(glob.glob(os.path.join(ONE, "one1_*.npz")))
POSTERIORS = ["diag", "kron", "full"]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def laplace_cls(lg, structure):
    return {"diag": lg.DiagLaplace, "kron": lg.KronLaplace, "full": lg.FullLaplace}[structure]


def one_layer_gcn(lg, X, ei, W, b, sym, cls=None, **kw):
    C, F = W.shape
    model = (cls or lg.GCN)(F, 8, C, 1, torch.as_tensor(X), torch.as_tensor(ei), symmetric=sym, **kw)
    with torch.no_grad():
        model.convs[0].lin.weight.copy_(torch.as_tensor(W))
        model.convs[0].lin.bias.copy_(torch.as_tensor(b))
    return model.cuda().eval()


# ---- 1. the reference's goldens -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("structure", POSTERIORS)
@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[:-4] for p in CASES])
def test_adjacency_gradient_matches_reference_autograd(path, structure):
    import laplace_gnn_amd as lg

    g = np.load(path)
    model = one_layer_gcn(lg, g["X"], g["edge_index"], g["W0"], g["b0"], bool(g["symmetric"]))
    loader = lg.TensorBatchLoader(torch.from_numpy(g["train_idx"]).cuda(), torch.from_numpy(g["train_y"]).cuda(),
                                  batch_size=int(g["batch_size"]))
    la = laplace_cls(lg, structure)(model, "classification", prior_precision=float(g["prior"]))
    la.fit(loader)
    val, ei, grad = la.neg_marglik_adj_grad(loader)
    assert np.array_equal(ei[0].cpu().numpy(), g["adj_nz_row"]) and np.array_equal(ei[1].cpu().numpy(), g["adj_nz_col"])
    ref = float(g[f"{structure}_neg_marglik"])
    cand = torch.from_numpy(np.stack([g["ne_row"], g["ne_col"]])).cuda()  # (a symmetric model adds the mirrored orientation)
    val2, _, grad2, gc = la.neg_marglik_adj_grad(loader, candidates=cand)
    e = (abs(float(val) - ref) / abs(ref), rel(grad.cpu().numpy(), g[f"{structure}_vals"]),
         rel(gc.cpu().numpy(), g[f"{structure}_ne_val"]))
    print(f"{structure}: value {e[0]:.2e}  stored {e[1]:.2e}  candidates {e[2]:.2e}")
    assert e[0] <= 5e-6
    assert e[1] < 1e-5
    assert e[2] < 1e-5
    assert gc.shape[0] == 200
    diag = g["adj_nz_row"] == g["adj_nz_col"]
    assert float(np.abs(grad.cpu().numpy()[diag]).max()) == 0.0  # overwritten by fill_diagonal_(1) in the reference
    # a second call gives the same result: the accumulators are the caller's, nothing is left in the context
    assert float(val2) == float(val) and rel(grad2.cpu().numpy(), grad.cpu().numpy()) < 1e-5
    model.engine.check_async_errors()


# ---- 2. / 3. against the fp64 restatement --------------------------------------------------------------------------------------
def _restatement_case(structure, sym, N, F, C, E, batch_sizes, hub, n_cand, ws_limit, seed):
    import laplace_gnn_amd as lg

    gen = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, N - 1, (2, E), generator=gen)  # node N - 1 stays isolated
    if hub:  # node 0: a propagation row with 70 stored entries (69 neighbours + the self loop), above the 64-entry split
        k = torch.arange(1, 70)
        ei = ei[:, (ei[0] != 0) & (ei[1] != 0)]
        ei = torch.cat([ei, torch.stack([torch.zeros_like(k), k]), torch.stack([k, torch.zeros_like(k)])], 1)
    X = torch.randn(N, F, generator=gen)
    W, b = 0.5 * torch.randn(C, F, generator=gen), 0.3 * torch.randn(C, generator=gen)
    model = one_layer_gcn(lg, X, ei, W, b, sym)
    eng = model.engine
    M = sum(batch_sizes)
    idx = torch.randint(0, N - 1, (M,), generator=gen)  # with replacement: repeated ids inside and across batches
    idx[0], idx[1], idx[2] = 0, N - 1, 0  # the hub row (twice) and the isolated node
    y = torch.randint(0, C, (M,), generator=gen)
    loader = lg.TensorBatchLoader(idx.cuda(), y.cuda(), batch_size=batch_sizes[0])
    assert [int(bx.shape[0]) for bx, _ in loader] == list(batch_sizes)
    if ws_limit:
        eng.set_workspace_limit(ws_limit)
    rows, cols = (t.cpu() for t in eng.export_adj())
    if hub:
        pr, _, _ = eng.export_propagation()
        assert int((pr == 0).sum()) == 70
    assert int((rows == N - 1).sum()) == 1  # the isolated node keeps its self loop only
    stored = torch.zeros(N, N, dtype=torch.bool)
    stored[rows, cols] = True
    c = torch.randint(0, N, (2, 4 * n_cand), generator=gen)
    ok = (c[0] != c[1]) & ~stored[c[0], c[1]] & ~stored[c[1], c[0]]
    if sym:
        ok &= c[0] < c[1]
    c = c[:, ok]
    c = c[:, torch.from_numpy(np.unique((c[0] * N + c[1]).numpy(), return_index=True)[1])][:, :n_cand]
    assert c.shape[1] == n_cand and not bool(stored[c[0], c[1]].any())
    prior = 0.7
    la = laplace_cls(lg, structure)(model, "classification", prior_precision=prior)
    la.fit(loader)
    val, e2, grad, gc = la.neg_marglik_adj_grad(loader, candidates=c.cuda())
    eng.check_async_errors()
    rval, gA, _ = R.neg_marglik_adj_grad(rows.numpy(), cols.numpy(), idx.numpy(), y.numpy(), prior, structure, num_nodes=N,
                                         X=X.numpy(), W=W.numpy(), b=b.numpy(), symmetric=sym, batch_size=batch_sizes[0])
    e = (abs(float(val) - rval) / abs(rval), rel(grad.cpu().numpy(), gA[rows.numpy(), cols.numpy()]),
         rel(gc.cpu().numpy(), gA[c[0].numpy(), c[1].numpy()]))
    print(f"{structure} sym={sym}: value {e[0]:.2e}  stored {e[1]:.2e}  candidates {e[2]:.2e}")
    assert np.linalg.norm(gA[c[0].numpy(), c[1].numpy()]) > 0
    return e


@pytest.mark.parametrize("sym", [True, False])
@pytest.mark.parametrize("structure", POSTERIORS)
def test_adjacency_gradient_midsize_vs_restatement(structure, sym):
    """N = 400, F = 33 (odd width), C = 7, a hub row of 70 entries, an isolated batch node, three batches (350 / 350 / 200
    samples drawn with replacement) and a 4 MiB workspace cap: the full posterior takes the 350-sample batches in two
    chunks (2 C P floats per sample, P = 238: 314 samples per chunk)."""
    e = _restatement_case(structure, sym, N=400, F=33, C=7, E=1500, batch_sizes=(350, 350, 200), hub=True, n_cand=300,
                          ws_limit=4 << 20, seed=21)
    assert e[0] <= 5e-6 and e[1] < 1e-4 and e[2] < 1e-4


@pytest.mark.parametrize("structure", POSTERIORS)
def test_banana_shape_in_miniature(structure):
    """F = 2, C = 2, N = 64: the padded copy of X (F < 4) and E rows of width round_up(F + 1, 4)."""
    e = _restatement_case(structure, True, N=64, F=2, C=2, E=150, batch_sizes=(33,), hub=False, n_cand=100, ws_limit=0, seed=22)
    assert e[0] <= 5e-6 and e[1] < 1e-4 and e[2] < 1e-4


# ---- 4. the loop ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["steloop1_diag_sym", "steloop1_kron_dir"])
def test_structure_learning_loop_matches_the_reference(name):
    """Three hyper-steps of the fork's loop on a one-layer STE-GCN with every non-edge tracked: value and ``adj.grad`` of every
    step, the continuous adjacency after every optimizer step and the binarised edge set (bit exact)."""
    import laplace_gnn_amd as lg

    g = np.load(os.path.join(ONE, name + ".npz"))
    N, sym = int(g["num_nodes"]), bool(g["symmetric"])
    init = torch.from_numpy(g["adj_init"]) > 0.5
    cand = (~init).nonzero().t().contiguous()
    train_idx, train_y = torch.from_numpy(g["train_idx"]), torch.from_numpy(g["train_y"])
    model = one_layer_gcn(lg, g["X"], g["edge_index"], g["W0"], g["b0"], sym, cls=lg.STEGCN, threshold=float(g["threshold"]),
                          train_masked_update=bool(g["masked"]), train_nodes=train_idx, candidates=cand)
    assert model.num_layers == 1 and model.adj.numel() == N * N - N
    assert torch.equal(model.dense_adj().cpu(), torch.from_numpy(g["adj_init"]))
    loader = lg.TensorBatchLoader(train_idx.cuda(), train_y.cuda(), batch_size=int(g["batch_size"]))
    la = laplace_cls(lg, str(g["structure"]))(model, "classification", prior_precision=float(g["prior"]))
    opt = torch.optim.SGD([model.adj], lr=float(g["lr_adj"]), weight_decay=float(g["weight_decay"]), momentum=float(g["momentum"]))
    la.fit(loader)
    flips = 0
    for k in range(g["adj_steps"].shape[0]):
        opt.zero_grad()
        value = model.adj_backward(la, loader)
        assert abs(float(value) - float(g["neg_marglik"][k])) <= 2e-5 * abs(float(g["neg_marglik"][k])), k
        grad = torch.zeros(N, N)
        grad[model.adj_index[0].cpu(), model.adj_index[1].cpu()] = model.adj.grad.cpu()
        ref = g["grad_steps"][k]
        assert np.linalg.norm(grad.numpy() - ref) <= 1e-4 * np.linalg.norm(ref), (k, "adj.grad")
        if bool(g["grad_norm"]):
            torch.nn.utils.clip_grad_norm_(model.adj, max_norm=1.0)
        opt.step()
        flips += model.apply_adj()
        la.fit(loader)
        want = torch.from_numpy(g["adj_steps"][k])
        got = model.dense_adj().cpu()
        off = ~torch.eye(N, dtype=torch.bool)
        assert float((got - want)[off].abs().max()) <= 1e-4, (k, "adjacency values")
        eff = 0.5 * (want + want.T) if sym else want
        on = eff > float(g["threshold"])
        on.fill_diagonal_(True)
        er, ec = on.nonzero(as_tuple=True)
        sr, sc = model.engine.export_adj()
        assert torch.equal(sr.cpu(), er) and torch.equal(sc.cpu(), ec), (k, "binarised edge set")
    assert flips > 0  # the fixture's loop changes the graph
    last = float(-la.log_marginal_likelihood())
    assert abs(last - float(g["neg_marglik"][-1])) <= 2e-5 * abs(float(g["neg_marglik"][-1]))
    model.engine.check_async_errors()


# ---- 5. the matrix-free predictive ---------------------------------------------------------------------------------------------
def _jacobian_route(la, x, E=None):
    Js, f = la.backend.jacobians(x)
    S = la.functional_variance(Js)
    if E is not None:
        S = E @ S @ E.T
    return f, S


def _predictive_setup(kind, seed=31):
    import laplace_gnn_amd as lg

    N, F, C = 300, 10, 5
    gen = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, N - 1, (2, 900), generator=gen)  # node N - 1 has no edges
    X = torch.randn(N, F, generator=gen)
    torch.manual_seed(seed)
    model = (lg.GCN if kind == "gcn" else lg.GraphSAGE)(F, 8, C, 1, X, ei, symmetric=True).cuda().eval()
    tr = torch.randperm(N, generator=gen)[:100]
    y = torch.randint(0, C, (100,), generator=gen)
    x = torch.cat([torch.tensor([N - 1, 0, 0]), torch.randperm(N, generator=gen)[:37]]).cuda()  # isolated node, a repeated id
    return model, lg.TensorBatchLoader(tr.cuda(), y.cuda(), batch_size=40), x, N, C


@pytest.mark.parametrize("structure", ["kron", "diag"])
@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_matrix_free_predictive_of_one_layer_models(kind, structure):
    """N = 300, F = 10, C = 5: variance, mapped outputs and every link approximation against the Jacobian route of the same
    fit; then the same calls with ``backend.jacobians`` counted -- the matrix-free path must not touch it."""
    import laplace_gnn_amd as lg
    from laplace_gnn_amd._lib import HipLibraryError

    model, loader, x, N, C = _predictive_setup(kind)
    la = laplace_cls(lg, structure)(model, "classification", prior_precision=2.0)
    la.fit(loader)
    links = ({}, {"link_approx": "bridge"}, {"link_approx": "bridge_norm"}, {"link_approx": "mc", "diagonal_output": True})
    # the Jacobian route of the same fit: the links with the matrix-free route switched off
    f_j, S = _jacobian_route(la, x)
    eps = torch.randn(C, 50, generator=torch.Generator().manual_seed(1)).cuda()
    fast_fn = la._glm_variance_matrix_free
    la._glm_variance_matrix_free = lambda *a, **k: None
    slow = [la(x, eps=eps, n_samples=50, **kw) for kw in links]
    la._glm_variance_matrix_free = fast_fn
    calls = []
    real_jac = la.backend.jacobians

    def counted(*a, **k):
        calls.append(1)
        return real_jac(*a, **k)

    la.backend.jacobians = counted
    fast = la._glm_variance_matrix_free(x)
    assert fast is not None, "1-layer models take the matrix-free route"
    assert rel(fast[0].cpu().numpy(), f_j.cpu().numpy()) < 1e-6
    err = rel(fast[1].cpu().numpy(), torch.diagonal(S, dim1=1, dim2=2).cpu().numpy())
    print(kind, structure, "variance rel", err)
    assert err < 1e-4
    assert rel(fast[1][2].cpu().numpy(), fast[1][1].cpu().numpy()) < 1e-6  # the repeated id
    for rows in (3, 11):  # fewer and more rows than classes
        E = torch.from_numpy(np.random.default_rng(rows).standard_normal((rows, C)).astype(np.float32)).cuda()
        mapped = la._glm_variance_matrix_free(x, out_map=E)
        assert mapped is not None and mapped[1].shape == (x.shape[0], rows)
        ref = torch.diagonal(E @ S @ E.T, dim1=1, dim2=2)
        assert rel(mapped[1].cpu().numpy(), ref.cpu().numpy()) < 1e-4, rows
    for kw, want in zip(links, slow):
        out = la(x, eps=eps, n_samples=50, **kw)
        assert rel(out.cpu().numpy(), want.cpu().numpy()) < 1e-4, kw
        assert torch.allclose(out.sum(dim=1), torch.ones_like(out[:, 0]), atol=1e-5), kw
    assert not calls, "the matrix-free path of a 1-layer model must not form Jacobians"
    # an id out of range: sticky flag, zero row, the other rows untouched
    model.engine.check_async_errors()
    bad = torch.cat([x[:3], torch.tensor([N], device="cuda"), x[3:]])
    _, var = la._glm_variance_matrix_free(bad)
    with pytest.raises(HipLibraryError, match="node index"):
        model.engine.check_async_errors()
    assert torch.count_nonzero(var[3]) == 0
    assert rel(torch.cat([var[:3], var[4:]]).cpu().numpy(), fast[1].cpu().numpy()) < 1e-6
    model.engine.close()


# ---- 6. refusals that stay -----------------------------------------------------------------------------------------------------
def test_refusals_that_stay():
    import laplace_gnn_amd as lg

    gen = torch.Generator().manual_seed(3)
    N, F, C = 50, 6, 3
    ei = torch.randint(0, N, (2, 120), generator=gen)
    X = torch.randn(N, F, generator=gen)
    idx, y = torch.randperm(N, generator=gen)[:20].cuda(), torch.randint(0, C, (20,), generator=gen).cuda()
    loader = lg.TensorBatchLoader(idx, y, batch_size=20)
    torch.manual_seed(0)
    # a 3-layer model: the device entry points keep their words
    deep = lg.GCN(F, 8, C, 3, X, ei).cuda().eval()
    for cls in (lg.KronLaplace, lg.DiagLaplace):
        la = cls(deep, "classification")
        la.fit(loader)
        with pytest.raises(lg._lib.HipLibraryError, match="2-layer models"):
            la.neg_marglik_adj_grad(loader)
    la = lg.FullLaplace(deep, "classification")
    la.fit(loader)
    with pytest.raises(NotImplementedError, match="2-layer"):
        la.neg_marglik_adj_grad(loader)
    # one-layer GraphSAGE: the front ends and the device entry point
    sage = lg.GraphSAGE(F, 8, C, 1, X, ei).cuda().eval()
    for cls in (lg.KronLaplace, lg.DiagLaplace, lg.FullLaplace):
        la = cls(sage, "classification")
        la.fit(loader)
        with pytest.raises(NotImplementedError, match="1-layer GraphSAGE"):
            la.neg_marglik_adj_grad(loader)
    eng = sage.engine
    out_bar = torch.zeros(N, C, device="cuda")
    e_bar = torch.zeros(N, F + 1, device="cuda")
    grad_P = torch.zeros(eng.nnz, device="cuda")
    with pytest.raises(lg._lib.HipLibraryError, match="1-layer"):
        eng.diag_adjgrad_batch(idx, y, torch.ones(eng.n_params, device="cuda"), grad_P, out_bar, None, e_bar)
    with pytest.raises(lg._lib.HipLibraryError, match="1-layer"):
        eng.adjgrad_batch(idx, y, [torch.eye(C, device="cuda")], grad_P, out_bar)
    # dense=True on a one-layer GCN
    gcn1 = lg.GCN(F, 8, C, 1, X, ei).cuda().eval()
    for cls in (lg.KronLaplace, lg.DiagLaplace):
        la = cls(gcn1, "classification")
        la.fit(loader)
        with pytest.raises(NotImplementedError, match=r"dense=True\): plain 2-layer GCN"):
            la.neg_marglik_adj_grad(loader, dense=True)
    with pytest.raises(lg._lib.HipLibraryError, match="dense adjacency gradient covers plain 2-layer GCN"):
        gcn1.engine.diag_adjgrad_batch_dense(idx, y, torch.ones(gcn1.engine.n_params, device="cuda"), out_bar,
                                             torch.zeros(N, 8, device="cuda"), e_bar, torch.zeros(N, N, device="cuda"))
    with pytest.raises(NotImplementedError, match="LoRASTEGCN: num_layers must be 2"):
        lg.LoRASTEGCN(F, 8, C, 1, X, ei, r=4, lora_alpha=16.0)
    for m in (deep, sage, gcn1):
        m.engine.check_async_errors()
