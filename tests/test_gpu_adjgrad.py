"""SURVEY.md 8(f)-4 on the GPU: ``KronLaplace.neg_marglik_adj_grad`` (csrc/adjgrad*.hip through the C ABI) against
(a) the reference's ``model.adj.grad`` after ``(-log_marginal_likelihood()).backward()`` on its STEGCN / STEGraphSAGE (goldens generated
by oracle/make_golden.py from the reference's own autograd) and (b) the CPU oracle's hand-written reverse chain on
seeded mid-size inputs (class chunks under a small workspace cap, repeated node ids, upstream vs fork-exact seeds).
fp32 end to end (eigendecomposition, three chained sparse products per class plane).  Measured on the device
(tools/adjgrad_attribution.py, profiles/r03_adjgrad_attribution.log): gradient <= 1.3e-6 on the fixtures and <= 1.1e-5 at
the mid-size shapes (most of it the fp32 eigenpairs: 4e-7 .. 2e-6 with the factor gradients formed in fp64), value <= 3e-7,
candidate pairs <= 7e-7 -- so the tolerances are 1e-5 (fixtures) and 1e-4 (mid size; BASELINE.json north_star's bar)."""
import glob
import os

import numpy as np
import pytest
import torch

import gnn_laplace_oracle as O
from conftest import GOLDEN
from gpu_utils import oracle_from_arrays, rel
from test_gpu_frontend import model_from_golden

pytestmark = pytest.mark.gpu
CASES = sorted(p for p in glob.glob(os.path.join(GOLDEN, "*.npz")) if "adjgrad_vals" in np.load(p))


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[:-4] for p in CASES])
def test_adjacency_gradient_matches_reference_autograd(path):
    import laplace_gnn_amd as lg

    g = np.load(path)
    model = model_from_golden(g)
    loader = lg.TensorBatchLoader(torch.from_numpy(g["train_idx"]).cuda(), torch.from_numpy(g["train_y"]).cuda(),
                                  batch_size=int(g["batch_size"]))
    la = lg.KronLaplace(model, "classification", prior_precision=float(g["adjgrad_prior"]))
    la.fit(loader)
    val, ei, grad = la.neg_marglik_adj_grad(loader)
    assert np.array_equal(ei[0].cpu().numpy(), g["adj_nz_row"]) and np.array_equal(ei[1].cpu().numpy(), g["adj_nz_col"])
    assert abs(float(val) - float(g["adjgrad_neg_marglik"])) <= 5e-6 * abs(float(g["adjgrad_neg_marglik"]))
    assert rel(grad.cpu().numpy(), g["adjgrad_vals"]) < 1e-5
    diag = g["adj_nz_row"] == g["adj_nz_col"]
    if str(g["kind"]) == "gcn":
        assert float(grad.cpu().numpy()[diag].__abs__().max()) == 0.0  # overwritten by fill_diagonal_(1) in the reference
    else:
        assert not diag.any()  # GraphSAGE stores no self loops (fill_diagonal_(0))
    # a second call gives the same result (accumulators are the caller's, nothing is left in the context); this one also
    # asks for candidate pairs that are NOT edges: the reference's dense adj.grad has them (that is how its structure
    # learning proposes new edges), 200 of them are in the fixture
    cand = torch.from_numpy(np.stack([g["adjgrad_ne_row"], g["adjgrad_ne_col"]])).cuda()
    _, _, grad2, gc = la.neg_marglik_adj_grad(loader, candidates=cand)
    assert rel(grad2.cpu().numpy(), grad.cpu().numpy()) < 1e-5
    assert rel(gc.cpu().numpy(), g["adjgrad_ne_val"]) < 1e-5
    model.engine.check_async_errors()


@pytest.mark.parametrize("kind", ["gcn", "sage"])
@pytest.mark.parametrize("fork_exact,sym,H,C", [(True, True, 64, 10), (False, False, 32, 7), (True, False, 256, 12)])
def test_adjacency_gradient_midsize_vs_oracle(fork_exact, sym, H, C, kind):
    import laplace_gnn_amd as lg

    N, F, E, M = 2500, 24, 9000, 500
    gen = torch.Generator().manual_seed(13)
    ei = torch.randint(0, N, (2, E), generator=gen)
    X = torch.randn(N, F, generator=gen)
    torch.manual_seed(1)
    model = (lg.GCN if kind == "gcn" else lg.GraphSAGE)(F, H, C, 2, X, ei, symmetric=sym).to("cuda").eval()
    idx = torch.randperm(N, generator=gen)[:M]
    idx[M // 2:M // 2 + 20] = idx[:20]  # repeated node ids inside and across batches
    y = torch.randint(0, C, (M,), generator=gen)
    loader = lg.TensorBatchLoader(idx.cuda(), y.cuda(), batch_size=200)  # 200 / 200 / 100
    model.engine.set_workspace_limit(16 << 20)  # several class chunks
    la = lg.KronLaplace(model, "classification", prior_precision=0.5, backend_kwargs=dict(fork_exact_seed=fork_exact))
    la.fit(loader)
    cand = torch.randint(0, N, (2, 300), generator=torch.Generator().manual_seed(5))
    cand = cand[:, cand[0] != cand[1]]
    # without candidate pairs first: at H = 256 that is the path that defines the planes on the active rows only (the fit's
    # top-layer kernel and compacted backward GEMM); with candidates everything is defined on all rows
    val0, _, grad0 = la.neg_marglik_adj_grad(loader)
    val, e2, grad, gc = la.neg_marglik_adj_grad(loader, candidates=cand.cuda())
    assert abs(float(val0) - float(val)) <= 1e-6 * abs(float(val)) and rel(grad0.cpu().numpy(), grad.cpu().numpy()) < 1e-5
    Ws = [c.lin.weight.detach().cpu().numpy() for c in model.convs]
    bs = [c.lin.bias.detach().cpu().numpy() for c in model.convs]
    om = oracle_from_arrays(kind, N, ei.numpy(), X.numpy(), Ws, bs, sym)
    oval, rows, cols, og = O.kron_marglik_adj_grad(om, idx.numpy(), y.numpy(), 200, 0.5, fork_exact, sym)
    assert np.array_equal(e2[0].cpu().numpy(), rows) and np.array_equal(e2[1].cpu().numpy(), cols)
    assert abs(float(val) - oval) <= 5e-6 * abs(oval)
    assert rel(grad.cpu().numpy(), og) < 1e-4 and rel(grad0.cpu().numpy(), og) < 1e-4
    # candidate pairs against the oracle's dense N x N gradient; pairs that are stored edges are not candidates
    _, gd = O.kron_marglik_adj_grad(om, idx.numpy(), y.numpy(), 200, 0.5, fork_exact, sym, dense=True)
    stored = set(zip(rows.tolist(), cols.tolist()))
    keep = np.array([(int(i), int(j)) not in stored for i, j in cand.t().tolist()])
    assert keep.sum() > 250
    assert rel(gc.cpu().numpy()[keep], gd[cand[0].numpy()[keep], cand[1].numpy()[keep]]) < 1e-4
    model.engine.check_async_errors()


def test_adjacency_gradient_is_refused_outside_the_first_slice():
    import laplace_gnn_amd as lg

    g = np.load(os.path.join(GOLDEN, "sage3_small_1batch_s0.npz"))
    model = model_from_golden(g)
    loader = lg.TensorBatchLoader(torch.from_numpy(g["train_idx"]).cuda(), torch.from_numpy(g["train_y"]).cuda(), 10000)
    la = lg.KronLaplace(model, "classification")
    with pytest.raises(AttributeError):
        la.neg_marglik_adj_grad(loader)
    la.fit(loader)
    with pytest.raises(lg._lib.HipLibraryError, match="2-layer models"):
        la.neg_marglik_adj_grad(loader)


def test_candidate_pairs_are_validated_before_they_reach_the_device():
    """candidate pairs index rows in the device kernels; out-of-range ids, diagonal pairs and pairs that are
    stored entries must be refused on the host."""
    import laplace_gnn_amd as lg

    g = torch.Generator().manual_seed(0)
    N, F, H, C = 120, 10, 8, 3
    X = torch.randn(N, F, generator=g)
    ei = torch.randint(0, N, (2, 400), generator=g)
    torch.manual_seed(0)
    model = lg.GCN(F, H, C, 2, X, ei).cuda().eval()
    idx = torch.randperm(N, generator=g)[:40].cuda()
    y = torch.randint(0, C, (40,), generator=g).cuda()
    loader = lg.TensorBatchLoader(idx, y, batch_size=40)
    la = lg.KronLaplace(model, "classification")
    la.fit(loader)
    rows, cols = model.engine.export_adj()
    stored = torch.stack([rows[rows != cols][:1], cols[rows != cols][:1]])
    for bad in (torch.tensor([[0], [N]]), torch.tensor([[-1], [3]]), torch.tensor([[5], [5]]), stored.cpu(),
                torch.tensor([[2 ** 33], [1]])):
        with pytest.raises(ValueError, match="candidate"):
            la.neg_marglik_adj_grad(loader, candidates=bad)
    dense = torch.zeros(N, N, dtype=torch.bool)
    dense[rows.cpu(), cols.cpu()] = True
    ne = (~dense).nonzero()[:50].t().contiguous()
    ne = ne[:, ne[0] != ne[1]]
    out = la.neg_marglik_adj_grad(loader, candidates=ne)
    assert len(out) == 4 and out[3].shape[0] == ne.shape[1] and torch.isfinite(out[3]).all()
    model.engine.check_async_errors()



# ---- diagonal posterior: what the shipped STE-GCN configuration differentiates (gnn/configs/original/stegcn_config.yaml:7) ----
DIAG_CASES = sorted(p for p in glob.glob(os.path.join(GOLDEN, "*.npz")) if "adjgrad_diag_vals" in np.load(p))


@pytest.mark.parametrize("path", DIAG_CASES, ids=[os.path.basename(p)[:-4] for p in DIAG_CASES])
def test_diag_adjacency_gradient_matches_reference_autograd(path):
    """``DiagLaplace.neg_marglik_adj_grad`` (lgnn_diag_adjgrad_batch / _finish) against ``model.adj.grad`` of the reference's
    STEGCN after ``(-DiagLaplace.log_marginal_likelihood()).backward()``: stored entries and the fixture's 200 non-edges.
    fp32 with float atomics; the oracle's fp64 chain is at 3e-7 of the same goldens."""
    import laplace_gnn_amd as lg

    g = np.load(path)
    model = model_from_golden(g)
    loader = lg.TensorBatchLoader(torch.from_numpy(g["train_idx"]).cuda(), torch.from_numpy(g["train_y"]).cuda(),
                                  batch_size=int(g["batch_size"]))
    la = lg.DiagLaplace(model, "classification", prior_precision=float(g["adjgrad_prior"]))
    with pytest.raises(AttributeError):
        la.neg_marglik_adj_grad(loader)
    la.fit(loader)
    val, ei, grad = la.neg_marglik_adj_grad(loader)
    assert np.array_equal(ei[0].cpu().numpy(), g["adj_nz_row"]) and np.array_equal(ei[1].cpu().numpy(), g["adj_nz_col"])
    assert abs(float(val) - float(g["adjgrad_diag_neg_marglik"])) <= 5e-6 * abs(float(g["adjgrad_diag_neg_marglik"]))
    assert rel(grad.cpu().numpy(), g["adjgrad_diag_vals"]) < 1e-5
    diag = g["adj_nz_row"] == g["adj_nz_col"]
    if str(g["kind"]) == "gcn":
        assert float(np.abs(grad.cpu().numpy()[diag]).max()) == 0.0  # overwritten by fill_diagonal_(1) in the reference
    else:
        assert not diag.any()  # GraphSAGE stores no self loops
    cand = torch.from_numpy(np.stack([g["adjgrad_ne_row"], g["adjgrad_ne_col"]])).cuda()
    _, _, grad2, gc = la.neg_marglik_adj_grad(loader, candidates=cand)
    assert rel(grad2.cpu().numpy(), grad.cpu().numpy()) < 1e-5
    assert rel(gc.cpu().numpy(), g["adjgrad_diag_ne_val"]) < 1e-5
    model.engine.check_async_errors()


@pytest.mark.parametrize("sym,F,H,C,limit", [(True, 24, 64, 10, None), (False, 37, 33, 7, 1 << 20), (False, 130, 256, 12, 8 << 20)])
def test_diag_adjacency_gradient_midsize_vs_oracle(sym, F, H, C, limit):
    """Mid-size graphs against the oracle's reverse chain: widths that fill no tile, repeated node ids, sample chunks under a
    small workspace cap (the first-layer tiles of a chunk of samples live in the workspace), candidates vs the dense gradient."""
    import laplace_gnn_amd as lg

    N, E, M = 1500, 6000, 300
    gen = torch.Generator().manual_seed(17)
    ei = torch.randint(0, N, (2, E), generator=gen)
    X = torch.randn(N, F, generator=gen)
    torch.manual_seed(2)
    model = lg.GCN(F, H, C, 2, X, ei, symmetric=sym).to("cuda").eval()
    idx = torch.randperm(N, generator=gen)[:M]
    idx[M // 2:M // 2 + 15] = idx[:15]  # repeated node ids (with their own labels) inside and across batches
    y = torch.randint(0, C, (M,), generator=gen)
    loader = lg.TensorBatchLoader(idx.cuda(), y.cuda(), batch_size=128)
    if limit is not None:
        model.engine.set_workspace_limit(limit)
    la = lg.DiagLaplace(model, "classification", prior_precision=0.5)
    la.fit(loader)
    cand = torch.randint(0, N, (2, 300), generator=torch.Generator().manual_seed(5))
    cand = cand[:, cand[0] != cand[1]]
    rows_s, cols_s = model.engine.export_adj()
    stored = set(zip(rows_s.cpu().tolist(), cols_s.cpu().tolist()))
    cand = cand[:, torch.tensor([(int(i), int(j)) not in stored for i, j in cand.t().tolist()])]
    # make sure some candidates start at batch nodes (only those see the first-layer tiles), one of them a repeated id
    extra = torch.stack([idx[:40], (idx[:40] + 7) % N])
    extra = extra[:, torch.tensor([(int(i), int(j)) not in stored and int(i) != int(j) for i, j in extra.t().tolist()])]
    cand = torch.cat([cand, extra, extra.flip(0)], dim=1)
    cand = cand[:, torch.tensor([(int(i), int(j)) not in stored for i, j in cand.t().tolist()])]
    val0, _, grad0 = la.neg_marglik_adj_grad(loader)
    val, e2, grad, gc = la.neg_marglik_adj_grad(loader, candidates=cand.cuda())
    assert abs(float(val0) - float(val)) <= 1e-6 * abs(float(val)) and rel(grad0.cpu().numpy(), grad.cpu().numpy()) < 1e-5
    Ws = [c.lin.weight.detach().cpu().numpy() for c in model.convs]
    bs = [c.lin.bias.detach().cpu().numpy() for c in model.convs]
    om = oracle_from_arrays("gcn", N, ei.numpy(), X.numpy(), Ws, bs, sym)
    oval, rows, cols, og = O.diag_marglik_adj_grad(om, idx.numpy(), y.numpy(), 128, 0.5, sym)
    assert np.array_equal(e2[0].cpu().numpy(), rows) and np.array_equal(e2[1].cpu().numpy(), cols)
    assert abs(float(val) - oval) <= 5e-6 * abs(oval)
    assert rel(grad.cpu().numpy(), og) < 1e-4
    _, gd = O.diag_marglik_adj_grad(om, idx.numpy(), y.numpy(), 128, 0.5, sym, dense=True)
    assert rel(gc.cpu().numpy(), gd[cand[0].numpy(), cand[1].numpy()]) < 1e-4
    # a prior precision per layer (weight, bias, weight, bias): gamma_p = 1 / (2 (H_p + delta_p)) with the block's own delta
    pp = torch.tensor([0.3, 2.0, 0.8, 5.0])
    sizes = [H * F, H, C * H, C]
    val_l, _, grad_l = la.neg_marglik_adj_grad(loader, prior_precision=pp.cuda())
    oval_l, _, _, og_l = O.diag_marglik_adj_grad(om, idx.numpy(), y.numpy(), 128, np.repeat(pp.numpy().astype(np.float64), sizes), sym)
    assert abs(float(val_l) - oval_l) <= 5e-6 * abs(oval_l) and rel(grad_l.cpu().numpy(), og_l) < 1e-4
    assert rel(grad_l.cpu().numpy(), og) > 1e-2  # (a different gradient than under the scalar prior)
    model.engine.check_async_errors()


def test_diag_adjacency_gradient_is_refused_for_deeper_models():
    import laplace_gnn_amd as lg

    g = np.load(os.path.join(GOLDEN, "sage3_small_1batch_s0.npz"))
    model = model_from_golden(g)
    loader = lg.TensorBatchLoader(torch.from_numpy(g["train_idx"]).cuda(), torch.from_numpy(g["train_y"]).cuda(), 10000)
    la = lg.DiagLaplace(model, "classification")
    la.fit(loader)
    with pytest.raises(lg._lib.HipLibraryError, match="2-layer"):
        la.neg_marglik_adj_grad(loader)


@pytest.mark.parametrize("sym,F,H,C", [(True, 24, 64, 10), (False, 37, 36, 7)])  # (GraphSAGE: hidden width % 4 == 0)
def test_diag_adjacency_gradient_of_graphsage_midsize_vs_oracle(sym, F, H, C):
    """STEGraphSAGE + DiagLaplace (round 4; the driver offers the pair, gnn/utils.py:55-59, 81): the local (sample, class)
    kernel against the oracle's reverse chain -- repeated node ids, rows without neighbours, several sample chunks under a small
    workspace cap, candidates vs the oracle's dense gradient."""
    import laplace_gnn_amd as lg

    N, E, M = 900, 3000, 150
    gen = torch.Generator().manual_seed(19)
    ei = torch.randint(0, N - 20, (2, E), generator=gen)  # the last 20 nodes have no edges
    X = torch.randn(N, F, generator=gen)
    torch.manual_seed(3)
    model = lg.GraphSAGE(F, H, C, 2, X, ei, symmetric=sym).to("cuda").eval()
    idx = torch.randperm(N, generator=gen)[:M]
    idx[M // 2:M // 2 + 10] = idx[:10]
    idx[-3:] = torch.tensor([N - 1, N - 2, N - 3])  # isolated nodes in the batch
    y = torch.randint(0, C, (M,), generator=gen)
    loader = lg.TensorBatchLoader(idx.cuda(), y.cuda(), batch_size=64)
    model.engine.set_workspace_limit(8 << 20)
    la = lg.DiagLaplace(model, "classification", prior_precision=0.5)
    la.fit(loader)
    rows_s, cols_s = model.engine.export_adj()
    stored = set(zip(rows_s.cpu().tolist(), cols_s.cpu().tolist()))
    cand = torch.randint(0, N, (2, 200), generator=torch.Generator().manual_seed(5))
    cand = torch.cat([cand, torch.stack([idx[:40], (idx[:40] + 7) % N])], dim=1)
    cand = cand[:, torch.tensor([(int(i), int(j)) not in stored and int(i) != int(j) for i, j in cand.t().tolist()])]
    val0, _, grad0 = la.neg_marglik_adj_grad(loader)
    val, e2, grad, gc = la.neg_marglik_adj_grad(loader, candidates=cand.cuda())
    assert abs(float(val0) - float(val)) <= 1e-6 * abs(float(val)) and rel(grad0.cpu().numpy(), grad.cpu().numpy()) < 1e-5
    Ws = [c.lin.weight.detach().cpu().numpy() for c in model.convs]
    bs = [c.lin.bias.detach().cpu().numpy() for c in model.convs]
    om = oracle_from_arrays("sage", N, ei.numpy(), X.numpy(), Ws, bs, sym)
    oval, rows, cols, og = O.diag_marglik_adj_grad(om, idx.numpy(), y.numpy(), 64, 0.5, sym)
    assert np.array_equal(e2[0].cpu().numpy(), rows) and np.array_equal(e2[1].cpu().numpy(), cols)
    assert abs(float(val) - oval) <= 5e-6 * abs(oval)
    assert rel(grad.cpu().numpy(), og) < 1e-4
    _, gd = O.diag_marglik_adj_grad(om, idx.numpy(), y.numpy(), 64, 0.5, sym, dense=True)
    assert rel(gc.cpu().numpy(), gd[cand[0].numpy(), cand[1].numpy()]) < 1e-4
    model.engine.check_async_errors()


@pytest.mark.parametrize("structure", ["kron", "diag"])
@pytest.mark.parametrize("norm,res,sym,H", [("layer", True, True, 64), ("layer", False, False, 33), ("batch", True, False, 32),
                                            (None, True, True, 16)])
def test_adjacency_gradient_of_res_norm_models_midsize_vs_oracle(norm, res, sym, H, structure):
    """``res=True`` / ``norm="layer"|"batch"`` (gnn/models/base_gnn.py:141-149; the STE-GCN configurations of the WebKB graphs
    and Circle, gnn/configs/original/stegcn_config.yaml:54-105, 129-145) at a WebKB-like size: several plane chunks under a
    small workspace cap, repeated node ids, non-trivial norm state, candidates against the oracle's dense gradient."""
    import laplace_gnn_amd as lg

    N, F, C, E, M = 400, 48, 5, 1500, 90
    gen = torch.Generator().manual_seed(23)
    ei = torch.randint(0, N, (2, E), generator=gen)
    X = torch.randn(N, F, generator=gen)
    torch.manual_seed(4)
    model = lg.GCN(F, H, C, 2, X, ei, symmetric=sym, norm=norm, res=res)
    extras = {}
    with torch.no_grad():
        if norm is not None:
            nm = model.norms[0]
            nm.weight.copy_(0.5 + torch.rand(H, generator=gen))
            nm.bias.copy_(0.3 * torch.randn(H, generator=gen))
            extras.update(norm=norm, norm_weight=[nm.weight.numpy().copy()], norm_bias=[nm.bias.numpy().copy()],
                          norm_eps=float(nm.eps))
            if norm == "batch":
                nm.running_mean.copy_(0.2 * torch.randn(H, generator=gen))
                nm.running_var.copy_(0.5 + torch.rand(H, generator=gen))
                extras.update(norm_mean=[nm.running_mean.numpy().copy()], norm_var=[nm.running_var.numpy().copy()])
        if res:
            extras.update(res_weights=[model.res[0].weight.detach().numpy().copy()],
                          res_biases=[model.res[0].bias.detach().numpy().copy()])
    model = model.to("cuda").eval()
    idx = torch.randperm(N, generator=gen)[:M]
    idx[M // 2:M // 2 + 10] = idx[:10]
    y = torch.randint(0, C, (M,), generator=gen)
    loader = lg.TensorBatchLoader(idx.cuda(), y.cuda(), batch_size=40)  # 40 / 40 / 10
    model.engine.set_workspace_limit(4 << 20)
    la = lg.Laplace(model, "classification", "all", structure, prior_precision=0.5)
    la.fit(loader)
    rows_s, cols_s = model.engine.export_adj()
    stored = set(zip(rows_s.cpu().tolist(), cols_s.cpu().tolist()))
    cand = torch.randint(0, N, (2, 200), generator=torch.Generator().manual_seed(5))
    cand = torch.cat([cand, torch.stack([idx[:30], (idx[:30] + 11) % N])], dim=1)
    cand = cand[:, torch.tensor([(int(i), int(j)) not in stored and int(i) != int(j) for i, j in cand.t().tolist()])]
    val0, _, grad0 = la.neg_marglik_adj_grad(loader)
    val, e2, grad, gc = la.neg_marglik_adj_grad(loader, candidates=cand.cuda())
    assert abs(float(val0) - float(val)) <= 1e-6 * abs(float(val)) and rel(grad0.cpu().numpy(), grad.cpu().numpy()) < 1e-5
    Ws = [c.lin.weight.detach().cpu().numpy() for c in model.convs]
    bs = [c.lin.bias.detach().cpu().numpy() for c in model.convs]
    om = oracle_from_arrays("gcn", N, ei.numpy(), X.numpy(), Ws, bs, sym, **extras)
    if structure == "kron":
        oval, rows, cols, og = O.kron_marglik_adj_grad(om, idx.numpy(), y.numpy(), 40, 0.5, True, sym)
        _, gd = O.kron_marglik_adj_grad(om, idx.numpy(), y.numpy(), 40, 0.5, True, sym, dense=True)
    else:
        oval, rows, cols, og = O.diag_marglik_adj_grad(om, idx.numpy(), y.numpy(), 40, 0.5, sym)
        _, gd = O.diag_marglik_adj_grad(om, idx.numpy(), y.numpy(), 40, 0.5, sym, dense=True)
    assert np.array_equal(e2[0].cpu().numpy(), rows) and np.array_equal(e2[1].cpu().numpy(), cols)
    assert abs(float(val) - oval) <= 5e-6 * abs(oval)
    assert rel(grad.cpu().numpy(), og) < 1e-4
    assert rel(gc.cpu().numpy(), gd[cand[0].numpy(), cand[1].numpy()]) < 1e-4
    model.engine.check_async_errors()
