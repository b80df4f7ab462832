"""``DiagLaplace.propose_edges`` on the GPU (csrc/adjband.hip, laplace_gnn_amd/adjgrad.py: ``_propose_edges_drive``): the k
non-edges with the smallest entry of d(-marglik)/d adj, formed in row bands of the all-pairs gradient -- against the reference's
own ``model.adj.grad`` (the fixtures' 200 non-edges), the ``dense=True`` gradient, the candidates route, under a workspace limit
that refuses ``dense=True``, through ``STEGCN.add_candidates`` and one structure step, and the refusals.

The bound between routes is ``tol = 1e-5 * max|D|`` (D the ``dense=True`` gradient): the band's bilinear terms are the dense
route's tile GEMMs on the same operands, the per-sample term is the same kernel, and normalize_adj backward is the same fused
multiply-add -- what differs is the order of the sums in the sparse pass behind each (fixed here, float atomics there), a few
ulp of entries whose terms cancel to a small fraction of max|D|.  Criteria tolerate ties: every j whose row of d/dP is zero
shares rt_i within adjacency row i, so pair sets are never compared across routes."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_utils import rel
from test_gpu_frontend import model_from_golden

pytestmark = pytest.mark.gpu


def _eligible(eng):
    """bool [N, N]: off the diagonal and not stored."""
    N = eng.num_nodes
    r, c = eng.export_adj()
    ok = torch.ones(N, N, dtype=torch.bool, device=r.device)
    ok[r, c] = False
    ok.fill_diagonal_(False)
    return ok


def _check_selection(pairs, grad, D, ok, tol, k):
    """The contract of ``propose_edges`` against a dense gradient ``D`` [N, N]; prints and returns the worst |grad - D|."""
    N = D.shape[0]
    i, j = pairs
    assert pairs.dtype == torch.int64 and grad.dtype == torch.float32 and pairs.shape == (2, grad.shape[0])
    assert grad.shape[0] == min(k, int(ok.sum()))
    assert torch.unique(i * N + j).numel() == grad.shape[0]  # distinct
    assert bool(ok[i, j].all())  # off-diagonal, not stored
    worst = float((grad - D[i, j]).abs().max())
    print(f"propose_edges: k={k} worst |grad - D| = {worst:.3e} = {worst / float(D.abs().max()):.3e} max|D|")
    assert worst <= tol
    assert bool((grad[1:] >= grad[:-1]).all())  # ascending
    rest = torch.where(ok, D, torch.full_like(D, float("inf")))
    rest[i, j] = float("inf")
    assert float(rest.min()) >= float(grad.max()) - tol  # nothing eligible outside beats the largest returned value
    return worst


# ---- 1. the reference's own model.adj.grad -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rows,eligible", [("gcn_small_3batch_s0", 128, 3887), ("gcn_small_isolated_s0", 128, 3891),
                                                ("gcn_mid_1batch_s0", 128, None)])
def test_every_non_edge_matches_the_reference_autograd(name, rows, eligible):
    """k = all non-edges, so every value comes back: the fixture's 200 non-edge values of ``model.adj.grad`` after
    ``(-DiagLaplace.log_marginal_likelihood()).backward()`` (rel < 1e-5, the bar of test_gpu_adjgrad.py for this chain) and
    exactly the eligible set.  N = 64: one ragged band of a 128-row height; N = 512: four bands of 128."""
    import laplace_gnn_amd as lg

    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    model = model_from_golden(g)
    N = int(g["num_nodes"])
    loader = lg.TensorBatchLoader(torch.from_numpy(g["train_idx"]).cuda(), torch.from_numpy(g["train_y"]).cuda(),
                                  batch_size=int(g["batch_size"]))
    la = lg.DiagLaplace(model, "classification", prior_precision=float(g["adjgrad_prior"]))
    la.fit(loader)
    ok = _eligible(model.engine)
    n_el = int(ok.sum())
    assert n_el == N * N - model.engine.nnz and (eligible is None or n_el == eligible)
    val, pairs, grad = la.propose_edges(loader, n_el, band_bytes=rows * 4 * N)
    assert abs(float(val) - float(g["adjgrad_diag_neg_marglik"])) <= 5e-6 * abs(float(g["adjgrad_diag_neg_marglik"]))
    assert grad.shape[0] == n_el and bool((grad[1:] >= grad[:-1]).all())
    got = torch.full((N, N), float("nan"), device="cuda")
    got[pairs[0], pairs[1]] = grad
    assert torch.equal(~torch.isnan(got), ok)  # exactly the eligible set
    ne = got[torch.from_numpy(g["adjgrad_ne_row"]).cuda(), torch.from_numpy(g["adjgrad_ne_col"]).cuda()].cpu().numpy()
    err = rel(ne, g["adjgrad_diag_ne_val"])
    print(f"propose_edges {name}: rel error at the 200 non-edges {err:.3e}")
    assert err < 1e-5
    model.engine.check_async_errors()


# ---- 2. / 3. top-k against dense=True and the candidates route -----------------------------------------------------------
N2, F2, H2, C2 = 300, 37, 36, 7  # none a tile multiple


@pytest.fixture(scope="module")
def seeded():
    """A seeded plain directed GCN, 4 N random edges, 45 training ids whose last five repeat the first five, two batches; the
    fitted posterior and the ``dense=True`` gradient D, computed once and left unchanged."""
    import laplace_gnn_amd as lg

    gen = torch.Generator().manual_seed(31)
    ei = torch.randint(0, N2, (2, 4 * N2), generator=gen)
    X = torch.randn(N2, F2, generator=gen)
    torch.manual_seed(3)
    model = lg.GCN(F2, H2, C2, 2, X, ei).cuda().eval()
    idx = torch.randperm(N2, generator=gen)[:45]
    idx[40:] = idx[:5]
    y = torch.randint(0, C2, (45,), generator=gen)
    loader = lg.TensorBatchLoader(idx.cuda(), y.cuda(), batch_size=23)
    la = lg.DiagLaplace(model, "classification", prior_precision=0.5)
    la.fit(loader)
    value, D = la.neg_marglik_adj_grad(loader, dense=True)
    return dict(model=model, loader=loader, la=la, value=value, D=D, ok=_eligible(model.engine), tol=1e-5 * float(D.abs().max()))


@pytest.mark.parametrize("k", [50, 1])
def test_top_k_against_the_dense_gradient(seeded, k):
    """128 / 128 / 44-row bands and one band, k = 50 and k = 1, against ``dense=True``: distinct eligible pairs, values within
    tol, ascending, nothing eligible outside below max(grad) - tol, both bandings equal within tol.
    Measured on an MI355X: worst |grad - D| / max|D| = 0 (k = 50 and k = 1, both bandings: the dense route's bits); 7.2e-8 in the
    N = 600 case below."""
    la, loader, D, ok, tol = (seeded[n] for n in ("la", "loader", "D", "ok", "tol"))
    _, p3, g3 = la.propose_edges(loader, k, band_bytes=128 * 4 * N2)
    _, p1, g1 = la.propose_edges(loader, k, band_bytes=320 * 4 * N2)
    _check_selection(p3, g3, D, ok, tol, k)
    _check_selection(p1, g1, D, ok, tol, k)
    assert float((g3 - g1).abs().max()) <= tol
    seeded["model"].engine.check_async_errors()


@pytest.mark.parametrize("k", [50, 1])
def test_two_identical_calls_return_identical_bits(seeded, k):
    """Two identical calls of ``propose_edges``, compared bit for bit: no sum behind the result has an order that varies
    between runs -- the sparse pass is ``lgnn_diag_adjgrad_band_sparse`` (fixed-order sums in place of the float atomics of
    ``lgnn_diag_adjgrad_batch``), the operands and rs / cs come from ``_band_prepare`` (no split-K atomics, no rocBLAS), a band
    element has one writer, the merge has a fixed order.  Earlier versions that took the ordinary sparse pass, or
    gp_rowcol_kernel's atomic column sums, differed in the last bit on some runs (9.5e-7 at -7.264)."""
    la, loader = seeded["la"], seeded["loader"]
    _, pa, ga = la.propose_edges(loader, k, band_bytes=128 * 4 * N2)
    _, pb, gb = la.propose_edges(loader, k, band_bytes=128 * 4 * N2)
    print(f"propose_edges twice: k={k} worst difference {float((ga - gb).abs().max()):.3e}")
    assert torch.equal(ga, gb)


def test_every_stage_is_bit_reproducible(seeded):
    """The engine's four calls twice from zeroed buffers -- ``diag_adjgrad_band_sparse`` per batch (training ids that repeat,
    nodes that collect many samples' contributions), ``_band_prepare``, ``_band_batch`` / ``_band_finish`` per band: the
    adjoints, the completed stored-entry gradient, the prepared operands and the bands agree bit for bit (no float atomic
    decides a bit; one writer per band element).  The bands against ``dense=True`` within tol."""
    la, loader, model = seeded["la"], seeded["loader"], seeded["model"]
    eng, dev = model.engine, "cuda"
    gamma = (0.5 * la._H_factor / la.posterior_precision).to(torch.float32).contiguous()
    idx, y = loader.indices, loader.labels
    runs = []
    for _ in range(2):
        grad_P = torch.zeros(eng.nnz, device=dev)
        out_bar, h1_bar, e_bar = (torch.zeros(N2, w, device=dev) for w in (C2, H2, F2 + 1))
        eng.forward(idx[:1])
        for X, yb in loader:
            eng.diag_adjgrad_band_sparse(X, yb, gamma, grad_P, out_bar, h1_bar, e_bar, loss_scale=la._H_factor)
        prepared = eng.diag_adjgrad_band_prepare(out_bar, h1_bar, e_bar, grad_P)
        bands = []
        for a0, a1 in [(0, 128), (128, 256), (256, 300)]:
            band = torch.zeros(a1 - a0, N2, device=dev)
            mine = (idx >= a0) & (idx < a1)
            eng.diag_adjgrad_band_batch(idx[mine], y[mine], gamma, a0, a1, band)
            bands.append(eng.diag_adjgrad_band_finish(out_bar, prepared, e_bar, a0, a1, band))
        runs.append([grad_P, out_bar, h1_bar, e_bar, *prepared, torch.cat(bands)])
    for name, t0, t1 in zip(("grad_P", "out_bar", "h1_bar", "e_bar", "Hb", "Z0", "Z1", "rs", "cs", "bands"), *runs):
        assert torch.equal(t0, t1), name
    # the fixed-order pass computes what the ordinary pass computes
    ref_P = torch.zeros(eng.nnz, device=dev)
    ref = [torch.zeros(N2, w, device=dev) for w in (C2, H2, F2 + 1)]
    for X, yb in loader:
        eng.diag_adjgrad_batch(X, yb, gamma, ref_P, *ref, loss_scale=la._H_factor)
    eng.diag_adjgrad_finish(*ref, ref_P)
    for name, got, want in zip(("grad_P", "out_bar", "h1_bar", "e_bar"), runs[0][:4], (ref_P, *ref)):
        assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()), name
    G = runs[0][-1].t()  # band[j, i] = d / d adj[i, j]
    ok = seeded["ok"]
    assert bool(torch.isinf(G[~ok]).all()) and bool(torch.isfinite(G[ok]).all())  # the diagonal and the stored pairs, only
    assert float((G[ok] - seeded["D"][ok]).abs().max()) <= seeded["tol"]
    eng.check_async_errors()


def test_against_the_candidates_route(seeded):
    la, loader, tol = seeded["la"], seeded["loader"], seeded["tol"]
    val, pairs, grad = la.propose_edges(loader, 50, band_bytes=128 * 4 * N2)
    res = la.neg_marglik_adj_grad(loader, candidates=pairs)
    print(f"propose_edges vs candidates: worst {float((res[3] - grad).abs().max()):.3e}, tol {tol:.3e}")
    assert float((res[3] - grad).abs().max()) <= tol
    assert float(val) == float(la.neg_marglik_adj_grad(loader)[0]) == float(res[0])
    seeded["model"].engine.check_async_errors()


# ---- 4. where dense=True is refused ------------------------------------------------------------------------------------
def test_under_a_workspace_limit_that_refuses_the_dense_gradient():
    """N = 600 under the smallest workspace limit the library accepts (1 MiB < 4 N^2): ``dense=True`` is refused,
    ``propose_edges(k = 20)`` runs in the default bands (384 / 216 rows) and agrees with the candidates route.  The scale of
    tol and the selection rule come from a dense gradient formed before the limit is set."""
    import laplace_gnn_amd as lg

    gen = torch.Generator().manual_seed(2)
    N = 600
    model = lg.GCN(6, 8, 3, 2, torch.randn(N, 6, generator=gen), torch.randint(0, N, (2, 1500), generator=gen)).cuda().eval()
    idx, y = torch.randperm(N, generator=gen)[:30], torch.randint(0, 3, (30,), generator=gen)
    loader = lg.TensorBatchLoader(idx.cuda(), y.cuda(), batch_size=30)
    la = lg.DiagLaplace(model, "classification")
    la.fit(loader)
    D = la.neg_marglik_adj_grad(loader, dense=True)[1]
    tol = 1e-5 * float(D.abs().max())
    model.engine.set_workspace_limit(1 << 20)
    with pytest.raises(NotImplementedError):
        la.neg_marglik_adj_grad(loader, dense=True)
    val, pairs, grad = la.propose_edges(loader, 20)
    _check_selection(pairs, grad, D, _eligible(model.engine), tol, 20)
    res = la.neg_marglik_adj_grad(loader, candidates=pairs)
    assert float((res[3] - grad).abs().max()) <= tol and float(val) == float(res[0])
    model.engine.check_async_errors()


# ---- 5. the structure step ---------------------------------------------------------------------------------------------
def test_proposals_enter_the_tracked_adjacency_and_flip():
    """fit -> propose_edges -> add_candidates -> adj_backward -> step -> apply_adj on an STEGCN built without candidates."""
    import laplace_gnn_amd as lg

    gen = torch.Generator().manual_seed(7)
    N, F, H, C = 150, 9, 10, 4
    X, ei = torch.randn(N, F, generator=gen), torch.randint(0, N, (2, 500), generator=gen)
    torch.manual_seed(4)
    model = lg.STEGCN(F, H, C, 2, X, ei).cuda().eval()
    idx, y = torch.randperm(N, generator=gen)[:40], torch.randint(0, C, (40,), generator=gen)
    loader = lg.TensorBatchLoader(idx.cuda(), y.cuda(), batch_size=25)
    la = lg.DiagLaplace(model, "classification", prior_precision=0.5)
    la.fit(loader)
    tol = 1e-5 * float(la.neg_marglik_adj_grad(loader, dense=True)[1].abs().max())
    n0 = model.adj.numel()
    _, pairs, grad = la.propose_edges(loader, 10)
    assert model.add_candidates(pairs) == 10 and model.adj.numel() == n0 + 10 and model.adj.grad is None
    keys = model.adj_index[0] * N + model.adj_index[1]
    assert bool((keys[1:] > keys[:-1]).all())
    pos = torch.searchsorted(keys, pairs[0] * N + pairs[1])
    assert bool((model.adj[pos] == 0).all()) and int((model.adj == 1).sum()) == n0
    model.adj_backward(la, loader)
    assert float((model.adj.grad[pos] - grad).abs().max()) <= tol
    opt = torch.optim.SGD([model.adj], lr=1.0 / float(grad.abs().min()))
    opt.step()
    assert model.apply_adj() >= 1
    sr, sc = model.engine.export_adj()
    assert bool(torch.isin(pairs[0, 0] * N + pairs[1, 0], sr * N + sc))  # the most negative proposal is an edge now
    assert model.add_candidates(pairs) == 0
    model.engine.check_async_errors()


# ---- 6. refusals and the edges of the contract -------------------------------------------------------------------------
def test_refusals_and_contract_edges(seeded):
    import laplace_gnn_amd as lg

    la, loader, ok = seeded["la"], seeded["loader"], seeded["ok"]
    with pytest.raises(ValueError, match="k must be"):
        la.propose_edges(loader, 0)
    with pytest.raises(ValueError, match="band_bytes"):
        la.propose_edges(loader, 5, band_bytes=63 * 4 * N2)
    _, pairs, grad = la.propose_edges(loader, N2 * N2, band_bytes=128 * 4 * N2)  # k above the eligible count: all of them
    assert grad.shape[0] == int(ok.sum()) and bool(ok[pairs[0], pairs[1]].all()) and bool(torch.isfinite(grad).all())
    assert torch.unique(pairs[0] * N2 + pairs[1]).numel() == grad.shape[0]

    gen = torch.Generator().manual_seed(5)
    N, F = 90, 6
    X, ei = torch.randn(N, F, generator=gen), torch.randint(0, N, (2, 250), generator=gen)
    small = lg.TensorBatchLoader(torch.arange(20).cuda(), torch.randint(0, 3, (20,), generator=gen).cuda(), batch_size=20)
    for model, likelihood, cause in [(lg.GCN(F, 8, 3, 2, X, ei, symmetric=True), "classification", "symmetric"),
                                     (lg.GraphSAGE(F, 8, 3, 2, X, ei), "classification", "GraphSAGE"),
                                     (lg.GCN(F, 8, 3, 2, X, ei, res=True), "classification", "res / norm"),
                                     (lg.GCN(F, 8, 3, 2, X, ei, norm="layer"), "classification", "res / norm"),
                                     (lg.GCN(F, 8, 3, 1, X, ei), "classification", "1-layer"),
                                     (lg.GCN(F, 8, 3, 3, X, ei), "classification", "3-layer"),
                                     (lg.GCN(F, 8, 3, 2, X, ei), "regression", "regression")]:
        refused = lg.DiagLaplace(model.cuda().eval(), likelihood)
        with pytest.raises(NotImplementedError, match=cause):
            refused.propose_edges(small, 5)
    for cls in (lg.KronLaplace, lg.FullLaplace):
        assert not hasattr(cls, "propose_edges")

    # an invalid node id surfaces through check_async_errors, as in the ordinary route
    model = lg.GCN(F, 8, 3, 2, X, ei).cuda().eval()
    good = lg.DiagLaplace(model, "classification")
    good.fit(small)
    bad = small.indices.clone()
    bad[3] = 10_000
    good.propose_edges(lg.TensorBatchLoader(bad, small.labels, batch_size=20), 5)
    with pytest.raises(lg._lib.HipLibraryError, match="node index"):
        model.engine.check_async_errors()
    _, pairs, grad = good.propose_edges(small, 5)  # the context stays usable
    assert grad.shape[0] == 5 and bool(torch.isfinite(grad).all())
    model.engine.check_async_errors()
