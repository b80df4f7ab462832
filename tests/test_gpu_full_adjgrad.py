"""The adjacency gradient of the marginal likelihood under the FULL posterior (``FullLaplace.neg_marglik_adj_grad``;
lgnn_full_adjgrad_batch / lgnn_full_directions, csrc/fulladj.hip + the shared tangent / reverse chains of csrc/adjgrad_{ext,sage,onelayer}.hip):

1. the new entry point with a diagonal Gamma against the reference's own ``model.adj.grad`` goldens of DiagLaplace (1e-5, the bar
   of the diagonal tests for the same chain);
2. the product kernel alone against fp64 einsums, with rocBLAS' fp32 ``J Gamma`` as the error bar (at most 2x its error, never
   above 1e-4);
3. end to end against the fp64 autograd restatement (tests/adjgrad_restatement.py, pinned to the reference by
   tests/test_adjgrad_restatement.py): value 5e-6, gradients 1e-5 on the fixtures / 1e-4 at the seeded mid-size shapes;
4. the per-rank shares of every batch add up;
5. the front end: refusals and one structure-learning step;
and Gamma itself where the fp64 precision exceeds 2 GiB (built in column blocks), to its fp32 rounding bound.

Measured on the device (worst over the cases): 1. 5.6e-7 stored entries / 2.0e-7 non-edges;  2. rocBLAS 0.8e-7 .. 2.6e-7,
R 1.1e-7 .. 2.8e-7, K 0.5e-7 .. 1.0e-7 (per shape in DESIGN 12.17);  3. fixtures 5.5e-7 stored / 1.0e-6 non-edges (value
1.5e-7), mid-size 4.6e-7 / 3.4e-7 (value 2.1e-7);  4. 1.8e-7 / 3.5e-8."""
import functools
import glob
import os

import numpy as np
import pytest
import torch

from adjgrad_restatement import neg_marglik_adj_grad, spec_from_golden
from conftest import GOLDEN
from gpu_utils import rel
from test_gpu_frontend import model_from_golden

pytestmark = pytest.mark.gpu
CASES = sorted(p for p in glob.glob(os.path.join(GOLDEN, "*.npz")) if "adjgrad_diag_vals" in np.load(p))
IDS = [os.path.basename(p)[:-4] for p in CASES]


def _loader(g):
    import laplace_gnn_amd as lg

    return lg.TensorBatchLoader(torch.from_numpy(g["train_idx"]).cuda(), torch.from_numpy(g["train_y"]).cuda(),
                                batch_size=int(g["batch_size"]))


def _buffers(eng):
    N, Hd, F, C = eng.num_nodes, eng.dims[1], eng.dims[0], eng.dims[-1]
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=eng.device)  # noqa: E731
    return z(eng.nnz), z(N, C), z(N, Hd), z(N, F + 1)


def _full_gamma(la):
    """d(1/2 logdet(f H + Delta)) / dH of a fitted FullLaplace, as the front end builds it."""
    f = float(la._H_factor)
    G = torch.cholesky_inverse(torch.linalg.cholesky(la.posterior_precision.double())) * (0.5 * f)
    return (0.5 * (G + G.T)).float().contiguous()


@functools.lru_cache(maxsize=None)
def _restated_fixture(path):
    g = np.load(path)
    return neg_marglik_adj_grad(g["adj_nz_row"], g["adj_nz_col"], g["train_idx"], g["train_y"], float(g["adjgrad_prior"]), "full",
                                **spec_from_golden(g))[:2]


# ---- 1. the reference chain with a diagonal Gamma -------------------------------------------------------------------------
@pytest.mark.parametrize("path", CASES, ids=IDS)
def test_full_entry_point_with_a_diagonal_gamma_matches_reference_autograd(path):
    import laplace_gnn_amd as lg
    from laplace_gnn_amd.laplace import _adjacency_candidates

    g = np.load(path)
    model = model_from_golden(g)
    eng = model.engine
    loader = _loader(g)
    la = lg.DiagLaplace(model, "classification", prior_precision=float(g["adjgrad_prior"]))
    la.fit(loader)
    f = float(la._H_factor)
    Gamma = torch.diag(0.5 * f / la.posterior_precision).float().contiguous()
    sym = bool(g["symmetric"])
    cand = _adjacency_candidates(eng, torch.from_numpy(np.stack([g["adjgrad_ne_row"], g["adjgrad_ne_col"]])).cuda(), sym)
    grad_P, out_bar, h1_bar, e_bar = _buffers(eng)
    eng.set_likelihood("classification")
    for X, y in loader:
        eng.full_adjgrad_batch(X, y, Gamma, grad_P, out_bar, h1_bar, e_bar, loss_scale=f, cand=cand)
    grad, gc = eng.diag_adjgrad_finish(out_bar, h1_bar, e_bar, grad_P, cand=cand)
    if sym:
        gc = 0.5 * (gc[:200] + gc[200:])
    e_st, e_ne = rel(grad.cpu().numpy(), g["adjgrad_diag_vals"]), rel(gc.cpu().numpy(), g["adjgrad_diag_ne_val"])
    print(f"stored {e_st:.2e}  non-edges {e_ne:.2e}")
    assert e_st < 1e-5 and e_ne < 1e-5
    eng.check_async_errors()


# ---- 2. the product alone --------------------------------------------------------------------------------------------------
def _seeded_gcn(N, F, H, C, seed, **kw):
    import laplace_gnn_amd as lg

    gen = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, N, (2, 4 * N), generator=gen)
    X = torch.randn(N, F, generator=gen)
    torch.manual_seed(seed)
    model = lg.GCN(F, H, C, 2, X, ei, **kw)
    if kw.get("norm"):
        with torch.no_grad():
            model.norms[0].weight.copy_(0.5 + torch.rand(H, generator=gen))
            model.norms[0].bias.copy_(0.3 * torch.randn(H, generator=gen))
    return model.to("cuda").eval(), gen


def _product_case(name):
    """(model, idx, workspace limit or None, expected P).  The small goldens have C = 3 and P = 131 (GCN) / 251 (GraphSAGE):
    no multiple of 4, the scalar loads; P = 1 492 and 3 944 take the float4 loads."""
    if name in ("gcn_golden", "sage_golden"):
        g = np.load(os.path.join(GOLDEN, ("gcn" if name == "gcn_golden" else "sage") + "_small_3batch_s1.npz"))
        return model_from_golden(g), torch.from_numpy(g["train_idx"]).cuda(), None, None
    if name == "ragged_chunks":  # per sample of a chunk: C (2 P + N (3 H + C) + 2 N max(H, C)) floats = 1.53 MB -> 20 / 20 / 5
        model, gen = _seeded_gcn(300, 37, 33, 7, 31)
        idx = torch.randperm(300, generator=gen)[:45]
        idx[40:] = idx[:5]
        per_sample = 7 * (2 * 1492 + 300 * (3 * 33 + 7) + 2 * 300 * 33) * 4
        limit = 20 * per_sample + 1024
        # the case is about chunking: 45 samples in 20 / 20 / 5.  If the library's per-sample formula changes,
        # change the limit with it -- these lines keep the case from quietly becoming one chunk
        assert limit // per_sample == 20 and 2 * 20 < len(idx) and len(idx) % 20 != 0
        return model, idx.cuda(), limit, 1492
    if name == "wide_classes":  # C = 40: a sample's rows exceed one 32-row MFMA block, 3 samples per 128-row tile
        model, gen = _seeded_gcn(120, 20, 64, 40, 32)
        return model, torch.randperm(120, generator=gen)[:10].cuda(), None, 3944
    model, gen = _seeded_gcn(90, 12, 8, 3, 33, norm="layer", res=True)
    return model, torch.randperm(90, generator=gen)[:30].cuda(), None, 8 * 12 + 8 + 3 * 8 + 3 + 8 * 12 + 8


@pytest.mark.parametrize("name", ["gcn_golden", "sage_golden", "ragged_chunks", "wide_classes", "res_ln"])
def test_full_directions_match_fp64_einsum_within_twice_the_rocblas_error(name):
    model, idx, limit, P_expected = _product_case(name)
    eng = model.engine
    if limit is not None:
        eng.set_workspace_limit(limit)
    P = eng.n_params
    assert P_expected is None or P == P_expected
    gen = torch.Generator().manual_seed(7)
    B = torch.randn(P, P, generator=gen, dtype=torch.float64)
    Gamma64 = B @ B.T / P + torch.diag(0.5 + torch.rand(P, generator=gen, dtype=torch.float64))
    Gamma64 = 0.5 * (Gamma64 + Gamma64.T)
    Gamma = Gamma64.float().cuda().contiguous()
    Kn, R = eng.full_directions(idx, Gamma)
    J, _ = eng.jacobians(idx)
    p = torch.softmax(eng.forward(idx).double(), 1)
    Lam = torch.diag_embed(p) - p[:, :, None] * p[:, None, :]
    G64 = Gamma.double()  # (the fp32 matrix the device reads, in fp64)
    Z64 = torch.einsum("mcp,pq->mcq", J.double(), G64)
    K64 = torch.einsum("mcq,mkq->mck", Z64, J.double())
    R64 = 2.0 * torch.einsum("mck,mkq->mcq", Lam, Z64)
    e_blas = rel(torch.matmul(J.reshape(-1, P), Gamma).cpu().numpy(), Z64.reshape(-1, P).cpu().numpy())
    e_R, e_K = rel(R.cpu().numpy(), R64.cpu().numpy()), rel(Kn.cpu().numpy(), K64.cpu().numpy())
    print(f"{name}: P {P}  rocBLAS J Gamma {e_blas:.2e}  R {e_R:.2e}  K {e_K:.2e}")
    bar = min(2.0 * e_blas, 1e-4)
    assert e_R <= bar and e_K <= bar
    eng.check_async_errors()


def test_gamma_of_a_posterior_above_two_gib_is_its_scaled_inverse():
    """P = 16 455: the fp64 precision takes 2.2 GB, where the solver's one-call inverse is no longer used (it fails on the
    device at P = 23 063) and the identity is solved in column blocks.  Checked in fp64 on 8 seeded probes V, with U = A V and
    A = f H + Delta:  Gamma U = (f / 2) V.  Gamma is the fp32 rounding of an fp64 inverse, |dGamma_ij| <= 2^-24 |Gamma_ij|, so
    the residual is at most 2^-24 |Gamma| |U| entry by entry (the fp64 inverse's own error is 1e-9 of that); held at twice
    its norm.  A misplaced column block leaves a residual of the size of V, some 1e6 times the bar."""
    import laplace_gnn_amd as lg

    model, gen = _seeded_gcn(64, 1020, 16, 7, 35)
    idx = torch.randperm(64, generator=gen)[:8].cuda()
    y = torch.randint(0, 7, (8,), generator=gen).cuda()
    la = lg.FullLaplace(model, "classification", prior_precision=1.0)
    la.fit(lg.TensorBatchLoader(idx, y, batch_size=8))
    P = model.engine.n_params
    assert P == 16455 and P * P * 8 >= 2 ** 31
    Gamma = la._adj_gamma()
    assert Gamma.dtype == torch.float32 and Gamma.is_contiguous() and torch.equal(Gamma, Gamma.T)
    V = torch.randn(P, 8, generator=gen, dtype=torch.float64).cuda()
    U = la.posterior_precision.double() @ V
    G64 = Gamma.double()
    res = float((G64 @ U - 0.5 * float(la._H_factor) * V).norm())
    bar = 2.0 * 2.0 ** -24 * float((G64.abs() @ U.abs()).norm())
    print(f"P {P}  residual {res:.3e}  bar {bar:.3e}  |V| {float(V.norm()):.3e}")
    assert res <= bar
    model.engine.check_async_errors()


# ---- 3. end to end against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("path", CASES, ids=IDS)
def test_full_adjacency_gradient_matches_restatement_on_the_fixtures(path):
    import laplace_gnn_amd as lg

    g = np.load(path)
    model = model_from_golden(g)
    loader = _loader(g)
    la = lg.FullLaplace(model, "classification", prior_precision=float(g["adjgrad_prior"]))
    la.fit(loader)
    cand = torch.from_numpy(np.stack([g["adjgrad_ne_row"], g["adjgrad_ne_col"]])).cuda()
    val0, ei0, grad0 = la.neg_marglik_adj_grad(loader)
    val, ei, grad, gc = la.neg_marglik_adj_grad(loader, candidates=cand)
    assert np.array_equal(ei[0].cpu().numpy(), g["adj_nz_row"]) and np.array_equal(ei[1].cpu().numpy(), g["adj_nz_col"])
    assert rel(grad0.cpu().numpy(), grad.cpu().numpy()) < 1e-5 and abs(float(val0) - float(val)) <= 1e-6 * abs(float(val))
    rval, rG = _restated_fixture(path)
    e_v = abs(float(val) - rval) / abs(rval)
    e_st = rel(grad.cpu().numpy(), rG[g["adj_nz_row"], g["adj_nz_col"]])
    e_ne = rel(gc.cpu().numpy(), rG[g["adjgrad_ne_row"], g["adjgrad_ne_col"]])
    print(f"value {e_v:.2e}  stored {e_st:.2e}  non-edges {e_ne:.2e}")
    assert e_v <= 5e-6
    assert e_st < 1e-5 and e_ne < 1e-5
    diag = g["adj_nz_row"] == g["adj_nz_col"]
    if str(g["kind"]) == "gcn":
        assert float(np.abs(grad.cpu().numpy()[diag]).max()) == 0.0  # overwritten by fill_diagonal_(1) in the reference
    else:
        assert not diag.any()
    if path.endswith("gcn_small_3batch_s0.npz"):  # not the diagonal posterior's gradient
        ld = lg.DiagLaplace(model, "classification", prior_precision=float(g["adjgrad_prior"]))
        ld.fit(loader)
        assert rel(grad.cpu().numpy(), ld.neg_marglik_adj_grad(loader)[2].cpu().numpy()) > 0.1
    model.engine.check_async_errors()


MID = {"gcn": dict(kind="gcn", H=33), "gcn_sym": dict(kind="gcn", H=33, symmetric=True), "sage": dict(kind="sage", H=36),
       "res_ln": dict(kind="gcn", H=32, norm="layer", res=True), "block_prior": dict(kind="gcn", H=33, block_prior=True)}


@pytest.mark.parametrize("name", sorted(MID))
def test_full_adjacency_gradient_midsize_vs_restatement(name):
    """Seeded graphs of 300 nodes: widths that fill no tile, three batches with a ragged last one, repeated node ids, several
    sample chunks under a 4 MiB workspace, candidates that start at batch nodes."""
    import laplace_gnn_amd as lg

    cfg = dict(MID[name])
    kind, H, block_prior = cfg.pop("kind"), cfg.pop("H"), cfg.pop("block_prior", False)
    N, F, C, M = 300, 37, 7, 150
    gen = torch.Generator().manual_seed(29)
    ei = torch.randint(0, N - 10, (2, 1000), generator=gen)  # the last 10 nodes have no edges
    X = torch.randn(N, F, generator=gen)
    torch.manual_seed(5)
    model = (lg.GCN if kind == "gcn" else lg.GraphSAGE)(F, H, C, 2, X, ei, **cfg)
    norm = None
    if cfg.get("norm"):
        with torch.no_grad():
            nm = model.norms[0]
            nm.weight.copy_(0.5 + torch.rand(H, generator=gen))
            nm.bias.copy_(0.3 * torch.randn(H, generator=gen))
        norm = dict(kind="layer", eps=float(nm.eps), weight=nm.weight.detach().numpy().copy(),
                    bias=nm.bias.detach().numpy().copy())
    theta = [q.detach().numpy().copy() for c in model.convs for q in (c.lin.weight, c.lin.bias)]
    theta += [q.detach().numpy().copy() for r in model.res for q in (r.weight, r.bias)]
    model = model.to("cuda").eval()
    eng = model.engine
    idx = torch.randperm(N, generator=gen)[:M]
    idx[M // 2:M // 2 + 15] = idx[:15]  # repeated node ids (with their own labels) inside and across batches
    idx[-2:] = torch.tensor([N - 1, N - 2])  # isolated nodes in the batch
    y = torch.randint(0, C, (M,), generator=gen)
    loader = lg.TensorBatchLoader(idx.cuda(), y.cuda(), batch_size=64)  # 64 / 64 / 22
    eng.set_workspace_limit(4 << 20)
    prior = torch.tensor([0.3, 2.0, 0.8, 5.0]) if block_prior else 0.5
    la = lg.FullLaplace(model, "classification", prior_precision=prior.cuda() if block_prior else prior)
    la.fit(loader)
    rows_s, cols_s = (t.cpu() for t in eng.export_adj())
    stored = set(zip(rows_s.tolist(), cols_s.tolist()))
    cand = torch.randint(0, N, (2, 150), generator=torch.Generator().manual_seed(5))
    cand = torch.cat([cand, torch.stack([idx[:40], (idx[:40] + 7) % N])], dim=1)
    cand = cand[:, torch.tensor([(int(i), int(j)) not in stored and int(i) != int(j) for i, j in cand.t().tolist()])]
    val0, _, grad0 = la.neg_marglik_adj_grad(loader)
    val, e2, grad, gc = la.neg_marglik_adj_grad(loader, candidates=cand.cuda())
    assert rel(grad0.cpu().numpy(), grad.cpu().numpy()) < 1e-5 and abs(float(val0) - float(val)) <= 1e-6 * abs(float(val))
    assert np.array_equal(e2[0].cpu().numpy(), rows_s.numpy()) and np.array_equal(e2[1].cpu().numpy(), cols_s.numpy())
    delta = np.repeat(prior.double().numpy(), [q.size for q in theta]) if block_prior else prior
    rval, rG, _ = neg_marglik_adj_grad(rows_s.numpy(), cols_s.numpy(), idx.numpy(), y.numpy(), delta, "full", kind=kind,
                                       num_nodes=N, X=X.numpy(), theta=theta, symmetric=bool(cfg.get("symmetric", False)),
                                       norm=norm)
    e_v = abs(float(val) - rval) / abs(rval)
    e_st = rel(grad.cpu().numpy(), rG[rows_s.numpy(), cols_s.numpy()])
    e_ne = rel(gc.cpu().numpy(), rG[cand[0].numpy(), cand[1].numpy()])
    print(f"{name}: value {e_v:.2e}  stored {e_st:.2e}  candidates {e_ne:.2e}")
    assert e_v <= 5e-6
    assert e_st < 1e-4 and e_ne < 1e-4
    if kind == "gcn":
        assert float(grad.cpu().numpy()[(rows_s == cols_s).numpy()].__abs__().max()) == 0.0
    eng.check_async_errors()


# ---- 4. the ranks' shares add up ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gcn_small_3batch_s1", "sage_small_3batch_s1", "gcn_resln_small_3batch_s1"])
def test_half_slices_of_every_batch_add_up_to_the_single_call(name):
    """What the ranks of a job do (every rank takes its slice of every batch, then one all-reduce of the accumulators), without
    starting processes: two sets of buffers, summed before the finish."""
    import laplace_gnn_amd as lg
    from laplace_gnn_amd.laplace import _adjacency_candidates

    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    model = model_from_golden(g)
    eng = model.engine
    loader = _loader(g)
    la = lg.FullLaplace(model, "classification", prior_precision=float(g["adjgrad_prior"]))
    la.fit(loader)
    cand_ij = torch.from_numpy(np.stack([g["adjgrad_ne_row"], g["adjgrad_ne_col"]])).cuda()
    _, _, grad, gc = la.neg_marglik_adj_grad(loader, candidates=cand_ij)
    Gamma, f, sym = _full_gamma(la), float(la._H_factor), bool(g["symmetric"])
    parts = []
    for rank in range(2):
        cand = _adjacency_candidates(eng, cand_ij, sym)
        bufs = _buffers(eng)
        for X, y in loader:
            M = X.shape[0]
            lo, hi = M * rank // 2, M * (rank + 1) // 2
            eng.full_adjgrad_batch(X[lo:hi], y[lo:hi], Gamma, *bufs, loss_scale=f, cand=cand)
        parts.append((bufs, cand))
    (b0, c0), (b1, c1) = parts
    grad_P, out_bar, h1_bar, e_bar = (a + b for a, b in zip(b0, b1))
    cand = (c0[0], c0[1], c0[2] + c1[2])
    grad2, gc2 = eng.diag_adjgrad_finish(out_bar, h1_bar, e_bar, grad_P, cand=cand)
    if sym:
        gc2 = 0.5 * (gc2[:200] + gc2[200:])
    e_st, e_ne = rel(grad2.cpu().numpy(), grad.cpu().numpy()), rel(gc2.cpu().numpy(), gc.cpu().numpy())
    print(f"stored {e_st:.2e}  non-edges {e_ne:.2e}")
    assert e_st < 1e-5 and e_ne < 1e-5
    eng.check_async_errors()


# ---- 5. the front end --------------------------------------------------------------------------------------------------------
def test_full_adjacency_gradient_refusals():
    import laplace_gnn_amd as lg

    g = np.load(os.path.join(GOLDEN, "gcn_small_1batch_s0.npz"))
    model = model_from_golden(g)
    loader = _loader(g)
    la = lg.FullLaplace(model, "classification")
    with pytest.raises(AttributeError):
        la.neg_marglik_adj_grad(loader)
    la.fit(loader)
    with pytest.raises(NotImplementedError, match="dense"):
        la.neg_marglik_adj_grad(loader, dense=True)
    assert len(la.neg_marglik_adj_grad(loader)) == 3
    reg_loader = lg.TensorBatchLoader(torch.from_numpy(g["train_idx"]).cuda(), torch.from_numpy(g["reg_y"]).cuda(), 10000)
    lr = lg.FullLaplace(model, "regression")
    lr.fit(reg_loader)
    with pytest.raises(NotImplementedError, match="classification"):
        lr.neg_marglik_adj_grad(reg_loader)
    model.engine.check_async_errors()
    g3 = np.load(os.path.join(GOLDEN, "sage3_small_1batch_s0.npz"))
    model3 = model_from_golden(g3)
    loader3 = _loader(g3)
    l3 = lg.FullLaplace(model3, "classification")
    l3.fit(loader3)
    with pytest.raises(NotImplementedError, match="2-layer"):
        l3.neg_marglik_adj_grad(loader3)
    # the C entry point refuses the model too (not only the front end)
    P = model3.engine.n_params
    with pytest.raises(lg._lib.HipLibraryError, match="2-layer"):
        model3.engine.full_directions(torch.from_numpy(g3["train_idx"]).cuda()[:4], torch.eye(P, device="cuda"))
    model3.engine.check_async_errors()


def test_one_structure_learning_step_runs_with_a_full_posterior():
    """``STEGCN.adj_backward(la, loader)`` only calls ``la.neg_marglik_adj_grad``: with a FullLaplace it leaves the direct call's
    gradient on the tracked entries, and ``apply_adj()`` runs afterwards."""
    import laplace_gnn_amd as lg

    N, F, H, C, M = 80, 10, 8, 3, 30
    gen = torch.Generator().manual_seed(41)
    X = torch.randn(N, F, generator=gen)
    ei = torch.randint(0, N, (2, 200), generator=gen)
    ci = torch.randint(0, N, (2, 60), generator=gen)
    torch.manual_seed(6)
    model = lg.STEGCN(F, H, C, 2, X, ei, candidates=ci[:, ci[0] != ci[1]]).to("cuda").eval()
    idx = torch.randperm(N, generator=gen)[:M].cuda()
    y = torch.randint(0, C, (M,), generator=gen).cuda()
    loader = lg.TensorBatchLoader(idx, y, batch_size=16)
    la = lg.FullLaplace(model, "classification", prior_precision=0.7)
    la.fit(loader)
    eng = model.engine
    sr, sc = eng.export_adj()
    value = model.adj_backward(la, loader)
    tracked = model.adj_index
    keys, skeys = tracked[0] * N + tracked[1], sr * N + sc
    is_stored = torch.isin(keys, skeys)
    ne = tracked[:, ~is_stored]
    val, _, gs, gc = la.neg_marglik_adj_grad(loader, candidates=ne)
    assert abs(float(val) - float(value)) <= 1e-6 * abs(float(val))
    got = model.adj.grad
    assert rel(got[~is_stored].cpu().numpy(), gc.cpu().numpy()) < 1e-5
    hit = torch.isin(skeys, keys)
    pos = torch.searchsorted(keys, skeys[hit])
    assert rel(got[pos].cpu().numpy(), gs[hit].cpu().numpy()) < 1e-5
    assert float(got.abs().max()) > 0
    torch.optim.SGD([model.adj], lr=0.6 / float(got.abs().max())).step()  # the largest entries cross the threshold
    assert model.apply_adj() > 0
    la.fit(loader)
    assert torch.isfinite(la.neg_marglik_adj_grad(loader)[2]).all()
    model.engine.check_async_errors()
