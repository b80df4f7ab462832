"""``lg.STEGraphSAGE`` on the device: the reference's GraphSAGE structure-learning loop (gnn/models/models.py:121-183 under
gnn/marglik_training.py:197-224) against goldens of the reference's own run (tests/golden/sageloop/steloop_sage_*.npz,
tools/make_sage_loop_golden.py), and the engine capability it needs -- a GraphSAGE graph that keeps and edits its diagonal
(``GraphEngine(self_loops=True)``): edits against a fresh ingest, the curvature and training kernels on graphs with self
loops against fp64, and the per-row candidate slices of the per-sample gradient (csrc/adjgrad_sage.hip)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F_

from adjgrad_restatement import neg_marglik_adj_grad
from conftest import GOLDEN
from gpu_utils import rel

pytestmark = pytest.mark.gpu
SAGELOOP = os.path.join(GOLDEN, "sageloop")


def _switch_on(model, pairs):
    """Tracked pairs -> value 1, then ``apply_adj``: the way a self loop enters the engine's graph."""
    N = model.num_nodes
    with torch.no_grad():
        pos = torch.searchsorted(model._keys(), (pairs[0] * N + pairs[1]).to(model.adj.device))
        model.adj[pos] = 1.0
    return model.apply_adj()


@pytest.mark.parametrize("name", ["steloop_sage_kron_sym", "steloop_sage_diag_sym", "steloop_sage_kron_dir_masked"])
def test_structure_learning_loop_matches_the_reference(name):
    """Three hyper-steps of the fork's loop with EVERY pair tracked, the diagonal included: the negative log marginal
    likelihood and ``adj.grad`` (whole N x N grid) of every step, the continuous values after every optimizer step (<= 1e-4)
    and the binarised edge set with its learned self loops (bit exact).  Tolerances: tests/test_gpu_structure.py's."""
    import laplace_gnn_amd as lg

    g = np.load(os.path.join(SAGELOOP, name + ".npz"))
    N, sym, thr = int(g["num_nodes"]), bool(g["symmetric"]), float(g["threshold"])
    X = torch.from_numpy(g["X"])
    ei = torch.from_numpy(g["edge_index"])
    init = torch.from_numpy(g["adj_init"]) > 0.5
    assert not bool(init.diagonal().any())
    cand = (~init).nonzero().t().contiguous()  # every non-edge AND the diagonal: the reference's dense parameter
    train_idx, train_y = torch.from_numpy(g["train_idx"]), torch.from_numpy(g["train_y"])
    model = lg.STEGraphSAGE(X.shape[1], int(g["W0"].shape[0]), int(g["W1"].shape[0]), 2, X, ei, None, threshold=thr,
                            symmetric=sym, train_masked_update=bool(g["masked"]), train_nodes=train_idx, candidates=cand)
    with torch.no_grad():
        for l, conv in enumerate(model.convs):
            conv.lin.weight.copy_(torch.from_numpy(g[f"W{l}"]))
            conv.lin.bias.copy_(torch.from_numpy(g[f"b{l}"]))
    model = model.cuda().eval()
    assert model.adj.numel() == N * N
    assert torch.equal(model.dense_adj().cpu(), torch.from_numpy(g["adj_init"]))
    assert model.engine.self_loops
    loader = lg.TensorBatchLoader(train_idx.cuda(), train_y.cuda(), batch_size=int(g["batch_size"]))
    cls = lg.KronLaplace if str(g["structure"]) == "kron" else lg.DiagLaplace
    la = cls(model, "classification", prior_precision=float(g["prior"]))
    opt = torch.optim.SGD([model.adj], lr=float(g["lr_adj"]), weight_decay=float(g["weight_decay"]), momentum=float(g["momentum"]))
    la.fit(loader)
    loops_seen = 0
    for k in range(g["adj_steps"].shape[0]):
        opt.zero_grad()
        value = model.adj_backward(la, loader)
        ref_v = float(g["neg_marglik"][k])
        print(f"{name} step {k}: value rel {abs(float(value) - ref_v) / abs(ref_v):.2e}")
        assert abs(float(value) - ref_v) <= 2e-5 * abs(ref_v), k
        grad = torch.zeros(N, N)
        grad[model.adj_index[0].cpu(), model.adj_index[1].cpu()] = model.adj.grad.cpu()
        ref = g["grad_steps"][k]
        print(f"{name} step {k}: adj.grad rel {np.linalg.norm(grad.numpy() - ref) / np.linalg.norm(ref):.2e}")
        assert np.linalg.norm(grad.numpy() - ref) <= 1e-4 * np.linalg.norm(ref), (k, "adj.grad")
        if bool(g["grad_norm"]):
            torch.nn.utils.clip_grad_norm_(model.adj, max_norm=1.0)  # gnn/marglik_training.py:217-219
        opt.step()
        model.apply_adj()
        la.fit(loader)
        want = torch.from_numpy(g["adj_steps"][k])
        got = model.dense_adj().cpu()
        print(f"{name} step {k}: values max abs {float((got - want).abs().max()):.2e}")
        assert float((got - want).abs().max()) <= 1e-4, (k, "adjacency values")  # the diagonal included
        eff = 0.5 * (want + want.T) if sym else want
        on = eff > thr  # (no overwritten diagonal: gnn/models/models.py:160-180)
        er, ec = on.nonzero(as_tuple=True)
        sr, sc = model.engine.export_adj()
        assert torch.equal(sr.cpu(), er) and torch.equal(sc.cpu(), ec), (k, "binarised edge set")
        assert torch.equal(model.full_adj().cpu(), on.float())
        loops_seen += int(on.diagonal().sum())
    assert loops_seen > 0  # a gradient or a refit ran on a graph with a self loop
    last = float(-la.log_marginal_likelihood())
    assert abs(last - float(g["neg_marglik"][-1])) <= 2e-5 * abs(float(g["neg_marglik"][-1]))
    # the graph survives a rebuild of the engine (``.to()`` / ``_apply``), self loops included
    sr, sc = model.engine.export_adj()
    model = model.to("cuda")
    r2, c2 = model.engine.export_adj()
    assert torch.equal(sr, r2) and torch.equal(sc, c2)
    model.engine.check_async_errors()


@pytest.mark.parametrize("sym", [False, True])
def test_self_loop_edits_are_bit_exact_against_a_fresh_ingest(sym):
    """The flip recipe of tests/test_gpu_structure.py (random insertions, removals, no-ops, diagonal pairs; mirrored flips on
    the symmetric graph, one-sided ones in its last round) on engines with ``self_loops=True``: diagonal pairs take effect, and
    the edited engine equals an engine freshly built from the edited list -- integers and propagation values identical, a
    forward pass to 1e-6."""
    import laplace_gnn_amd as lg

    g = torch.Generator().manual_seed(7 + sym)
    N, F, H, C, E = 700, 24, 32, 5, 2600
    ei = torch.randint(0, N, (2, E), generator=g)
    ei[1, :6] = ei[0, :6]  # pairs (i, i) in the edge list
    X = torch.randn(N, F, generator=g).cuda()
    Ws = [(0.2 * torch.randn(H, 2 * F, generator=g)).cuda(), (0.2 * torch.randn(C, 2 * H, generator=g)).cuda()]
    bs = [(0.1 * torch.randn(H, generator=g)).cuda(), (0.1 * torch.randn(C, generator=g)).cuda()]
    eng = lg.GraphEngine(ei.cuda(), N, kind="sage", symmetric=sym, self_loops=True)
    eng.bind(X, Ws, bs)
    with pytest.raises(ValueError, match="self_loops"):
        lg.GraphEngine(ei.cuda(), N, kind="gcn", self_loops=True)
    idx = torch.arange(N).cuda()
    sr, sc = eng.export_adj()
    A = torch.zeros(N, N, dtype=torch.bool)
    A[ei[0], ei[1]] = True
    if sym:
        A |= A.T.clone()
    assert int(A.diagonal().sum()) >= 6 and torch.equal(torch.stack([sr.cpu(), sc.cpu()]), A.nonzero().t())  # ingest keeps (i, i)
    assert torch.equal(eng.adj_to_edge_index().cpu(), (A & ~torch.eye(N, dtype=torch.bool)).nonzero().t())
    diag_flips = 0
    for round_ in range(3):
        K = 400
        fi, fj = torch.randint(0, N, (K,), generator=g), torch.randint(0, N, (K,), generator=g)
        fj[:40] = fi[:40]  # diagonal pairs
        st = torch.randint(0, 2, (K,), generator=g).bool()
        st[:8] = True
        _, first = np.unique((fi * N + fj).numpy(), return_index=True)  # a pair may be listed once
        fi, fj, st = fi[first], fj[first], st[first]
        if sym and round_ < 2:  # mirrored flips keep the aliasing; the last round breaks it with one-sided ones
            off = fi != fj
            fi, fj, st = torch.cat([fi, fj[off]]), torch.cat([fj, fi[off]]), torch.cat([st, st[off]])
            _, first = np.unique((fi * N + fj).numpy(), return_index=True)
            fi, fj, st = fi[first], fj[first], st[first]
            state = {}
            for a, b, s in zip(fi.tolist(), fj.tolist(), st.tolist()):
                state.setdefault((min(a, b), max(a, b)), s)
            st = torch.tensor([state[(min(a, b), max(a, b))] for a, b in zip(fi.tolist(), fj.tolist())])
        d = fi == fj
        diag_flips += int((A[fi[d], fj[d]] != st[d]).sum())
        eng.update_adjacency(fi.cuda(), fj.cuda(), st.cuda())
        A[fi, fj] = st  # diagonal pairs included
        want_r, want_c = A.nonzero(as_tuple=True)
        got_r, got_c = eng.export_adj()
        assert torch.equal(got_r.cpu(), want_r) and torch.equal(got_c.cpu(), want_c), round_
        assert eng.nnz == int(A.sum())
        fresh = lg.GraphEngine(A.nonzero().t().contiguous().cuda(), N, kind="sage", symmetric=False, self_loops=True)
        fresh.bind(X, Ws, bs)
        r1, c1, v1 = eng.export_propagation()
        r2, c2, v2 = fresh.export_propagation()
        assert torch.equal(r1, r2) and torch.equal(c1, c2) and torch.equal(v1, v2)
        deg = A.sum(1).clamp(min=1).float()
        assert torch.allclose(v1.cpu(), (1.0 / deg)[r1.cpu()], rtol=1e-6, atol=0)  # a stored (i, i) counts in its row's sum
        assert eng.is_symmetric == fresh.is_symmetric == bool(torch.equal(A, A.T))
        assert torch.allclose(eng.forward(idx), fresh.forward(idx), rtol=1e-6, atol=1e-6)
        fresh.close()
    assert diag_flips > 20
    eng.check_async_errors()
    eng.close()


def _loop_graph(N, n_edges, loops, lonely, isolated, gen):
    """Random off-diagonal edges that avoid ``lonely`` and ``isolated``; ``lonely`` is among ``loops``."""
    ei = torch.randint(0, N, (2, n_edges), generator=gen)
    keep = (ei[0] != ei[1])
    for v in (lonely, isolated):
        keep &= (ei[0] != v) & (ei[1] != v)
    assert lonely in loops.tolist() and isolated not in loops.tolist()
    return ei[:, keep]


@pytest.mark.parametrize("sym", [False, True])
def test_diag_curvature_on_a_graph_with_self_loops_against_fp64(sym):
    """``DiagLaplace`` on a GraphSAGE graph with six self loops -- one node whose only entry is its self loop, one isolated
    node, a repeated sample id -- against the fp64 restatement (tests/adjgrad_restatement.py takes the diagonal as given):
    value, gradient on the stored entries (self loops included) and on 60 candidates, diagonal ones among them.  Tolerances:
    tests/test_gpu_adjgrad.py's for this call on the GraphSAGE fixtures (value 5e-6, gradients 1e-5)."""
    import laplace_gnn_amd as lg

    N, F, H, C, M = 40, 6, 8, 3, 25
    gen = torch.Generator().manual_seed(31 + sym)
    loops = torch.tensor([2, 5, 11, 17, 23, 38])
    lonely, isolated = 17, 29
    ei = _loop_graph(N, 90, loops, lonely, isolated, gen)
    X = torch.randn(N, F, generator=gen)
    torch.manual_seed(5)
    model = lg.STEGraphSAGE(F, H, C, 2, X, ei, None, dropout_p=0.0, symmetric=sym, candidates=torch.stack([loops, loops]))
    model = model.cuda().eval()
    assert _switch_on(model, torch.stack([loops, loops])) == loops.numel()
    idx = torch.randperm(N, generator=gen)[:M]
    idx[0], idx[1], idx[2], idx[9] = lonely, isolated, 5, 5  # the special rows are samples; node 5 (a self loop) twice
    y = torch.randint(0, C, (M,), generator=gen)
    loader = lg.TensorBatchLoader(idx.cuda(), y.cuda(), batch_size=10)
    la = lg.DiagLaplace(model, "classification", prior_precision=0.5)
    la.fit(loader)
    sr, sc = model.engine.export_adj()
    stored = torch.zeros(N, N, dtype=torch.bool)
    stored[sr.cpu(), sc.cpu()] = True
    assert int(stored.diagonal().sum()) == 6 and int(stored[lonely].sum()) == 1 and int(stored[isolated].sum()) == 0
    # 60 candidates: diagonal pairs (of a sample, of the isolated node, of a node outside the batch), pairs from samples to the
    # isolated node, random non-edges; a symmetric model takes one orientation per unordered pair
    in_batch = torch.zeros(N, dtype=torch.bool)
    in_batch[idx] = True
    outside = int((~in_batch & ~stored.diagonal()).nonzero()[0])
    sample = int(idx[[int(v) not in loops.tolist() for v in idx]][3])
    chosen = [(sample, sample), (isolated, isolated), (outside, outside)]
    chosen += [(int(a), isolated) for a in idx[3:8].tolist() if int(a) != isolated and not stored[int(a), isolated]]
    taken = set(chosen) | {(b, a) for a, b in chosen}
    free = (~stored).nonzero()
    for k in torch.randperm(free.shape[0], generator=gen).tolist():
        a, b = int(free[k, 0]), int(free[k, 1])
        if len(chosen) < 60 and a != b and (a, b) not in taken:
            chosen.append((a, b))
            taken |= {(a, b), (b, a)}
    assert len(chosen) == 60
    cand = torch.tensor(chosen)[torch.randperm(60, generator=gen)].t().contiguous()
    assert int((cand[0] == cand[1]).sum()) == 3
    val, e2, grad, gc = la.neg_marglik_adj_grad(loader, candidates=cand.cuda())
    theta = [p.detach().cpu().numpy() for p in (model.convs[0].lin.weight, model.convs[0].lin.bias,
                                                 model.convs[1].lin.weight, model.convs[1].lin.bias)]
    oval, gA, _ = neg_marglik_adj_grad(sr.cpu().numpy(), sc.cpu().numpy(), idx.numpy(), y.numpy(), 0.5, "diag", kind="sage",
                                       num_nodes=N, X=X.numpy(), theta=theta, symmetric=sym)
    assert torch.equal(e2[0], sr) and torch.equal(e2[1], sc)
    e_val = abs(float(val) - oval) / abs(oval)
    e_grad = rel(grad.cpu().numpy(), gA[sr.cpu().numpy(), sc.cpu().numpy()])
    e_cand = rel(gc.cpu().numpy(), gA[cand[0].numpy(), cand[1].numpy()])
    dg = (sr == sc).cpu().numpy()
    e_loops = rel(grad.cpu().numpy()[dg], gA[sr.cpu().numpy(), sc.cpu().numpy()][dg])
    print(f"sym={sym}: value {e_val:.2e}, stored {e_grad:.2e}, self loops {e_loops:.2e}, candidates {e_cand:.2e}")
    assert e_val <= 5e-6
    assert e_grad < 1e-5 and e_loops < 1e-5
    assert e_cand < 1e-5
    model.engine.check_async_errors()


@pytest.mark.parametrize("sym", [False, True])
def test_kfac_routes_agree_on_a_graph_with_self_loops(sym):
    """The one-hop path route against the class-plane route (``paths=False``) on a GraphSAGE graph with ten self loops, two
    batches with a repeated id: B factors at the tolerance of tests/test_gpu_paths.py for that comparison (2e-5), A factors
    and the loss equal.  (The Kronecker fit on a self-loop graph is pinned to the reference by the loop fixtures at H = 8.)"""
    import laplace_gnn_amd as lg

    N, F, H, C, E, M = 300, 20, 136, 5, 1200, 160
    gen = torch.Generator().manual_seed(41 + sym)
    ei = torch.randint(0, N, (2, E), generator=gen)
    ei = ei[:, ei[0] != ei[1]]
    loops = torch.randperm(N, generator=gen)[:10]
    ei = torch.cat([ei, torch.stack([loops, loops])], 1)
    X = torch.randn(N, F, generator=gen).cuda()
    Ws = [(0.2 * torch.randn(H, 2 * F, generator=gen)).cuda(), (0.2 * torch.randn(C, 2 * H, generator=gen)).cuda()]
    bs = [(0.1 * torch.randn(H, generator=gen)).cuda(), (0.1 * torch.randn(C, generator=gen)).cuda()]
    idx = torch.randperm(N, generator=gen)[:M]
    idx[:5] = loops[:5]  # nodes with a self loop among the samples, one of them twice
    idx[100] = loops[0]
    y = torch.randint(0, C, (M,), generator=gen)
    eng = lg.GraphEngine(ei.cuda(), N, kind="sage", symmetric=sym, self_loops=True)
    eng.bind(X, Ws, bs)
    sr, sc = eng.export_adj()
    assert int((sr == sc).sum()) == 10
    assert eng.kfac_plan(paths=True)["paths"] and not eng.kfac_plan(paths=False)["paths"]
    flat, views, loss = eng.new_kfac_buffers()
    flat2, views2, loss2 = eng.new_kfac_buffers()
    for s in range(0, M, 80):
        eng.kfac_accumulate(idx[s:s + 80].cuda(), y[s:s + 80].cuda(), M, views, loss, paths=True)
        assert eng.last_kfac_used_paths
        eng.kfac_accumulate(idx[s:s + 80].cuda(), y[s:s + 80].cuda(), M, views2, loss2, paths=False)
        assert not eng.last_kfac_used_paths
    torch.cuda.synchronize()
    for l, ((A, B), (A2, B2)) in enumerate(zip(views, views2)):
        e = rel(B.cpu().numpy(), B2.cpu().numpy())
        print(f"sym={sym} B_{l}: path vs plane {e:.2e}")
        assert e < 2e-5, f"B_{l} vs the plane route"
        assert rel(A.cpu().numpy(), A2.cpu().numpy()) < 2e-5
        assert float(B.abs().sum()) > 0
    assert abs(float(loss) - float(loss2)) <= 1e-6 * abs(float(loss2))
    eng.check_async_errors()
    eng.close()


def test_candidate_slices_of_the_per_sample_gradient_against_fp64():
    """``sage_diag_pair_kernel`` reads each row's slice of the candidates ordered by row: K = 300 candidates in shuffled order on
    an ``lg.GraphSAGE`` model -- several per row, rows with none, rows outside the batch, a batch with a repeated id -- against
    the fp64 restatement, in the caller's order (gradients 1e-5, value 5e-6: tests/test_gpu_adjgrad.py's fixture tolerances)."""
    import laplace_gnn_amd as lg

    N, F, H, C, M, K = 60, 5, 8, 3, 20, 300
    gen = torch.Generator().manual_seed(53)
    ei = torch.randint(0, N, (2, 150), generator=gen)
    X = torch.randn(N, F, generator=gen)
    torch.manual_seed(6)
    model = lg.GraphSAGE(F, H, C, 2, X, ei, symmetric=False).cuda().eval()
    idx = torch.randperm(N, generator=gen)[:M]
    idx[7] = idx[2]  # a repeated id inside the first batch
    y = torch.randint(0, C, (M,), generator=gen)
    loader = lg.TensorBatchLoader(idx.cuda(), y.cuda(), batch_size=12)
    la = lg.DiagLaplace(model, "classification", prior_precision=0.5)
    la.fit(loader)
    sr, sc = model.engine.export_adj()
    stored = torch.zeros(N, N, dtype=torch.bool)
    stored[sr.cpu(), sc.cpu()] = True
    in_batch = torch.zeros(N, dtype=torch.bool)
    in_batch[idx] = True
    no_cand = torch.cat([idx[:3], (~in_batch).nonzero()[:5, 0]])  # rows without a candidate, inside and outside the batch
    free = (~stored).nonzero()
    free = free[~torch.isin(free[:, 0], no_cand) & (free[:, 0] != free[:, 1])]
    other = (~in_batch & ~torch.isin(torch.arange(N), no_cand)).nonzero()[0, 0]
    diag_c = torch.stack([torch.stack([idx[5], idx[5]]), torch.stack([idx[15], idx[15]]), torch.stack([other, other])])
    assert idx[5] != idx[15] and not bool(stored[diag_c[:, 0], diag_c[:, 1]].any())  # (lg.GraphSAGE stores no diagonal)
    cand = torch.cat([free[torch.randperm(free.shape[0], generator=gen)[:K - 3]], diag_c])
    cand = cand[torch.randperm(K, generator=gen)].t().contiguous()  # shuffled: the caller's order is arbitrary
    assert cand.shape[1] == K
    per_row = torch.bincount(cand[0], minlength=N)
    assert int(per_row.max()) >= 4 and int((per_row[idx[3:]] >= 2).sum()) > 5  # several per row, at batch rows too
    assert int((per_row[~in_batch] > 0).sum()) > 10 and int(per_row[no_cand].sum()) == 0
    assert int((cand[0] == cand[1]).sum()) == 3  # GraphSAGE's diagonal pairs are genuine non-edges
    val, _, grad, gc = la.neg_marglik_adj_grad(loader, candidates=cand.cuda())
    theta = [p.detach().cpu().numpy() for p in (model.convs[0].lin.weight, model.convs[0].lin.bias,
                                                 model.convs[1].lin.weight, model.convs[1].lin.bias)]
    oval, gA, _ = neg_marglik_adj_grad(sr.cpu().numpy(), sc.cpu().numpy(), idx.numpy(), y.numpy(), 0.5, "diag", kind="sage",
                                       num_nodes=N, X=X.numpy(), theta=theta, symmetric=False)
    e_cand = rel(gc.cpu().numpy(), gA[cand[0].numpy(), cand[1].numpy()])
    e_grad = rel(grad.cpu().numpy(), gA[sr.cpu().numpy(), sc.cpu().numpy()])
    print(f"candidates {e_cand:.2e}, stored {e_grad:.2e}, value {abs(float(val) - oval) / abs(oval):.2e}")
    assert abs(float(val) - oval) <= 5e-6 * abs(oval)
    assert e_cand < 1e-5 and e_grad < 1e-5
    # the same candidates in another order: the same numbers at the permuted places (summation order aside)
    perm = torch.randperm(K, generator=gen)
    _, _, _, gc2 = la.neg_marglik_adj_grad(loader, candidates=cand[:, perm].cuda())
    assert rel(gc2.cpu().numpy(), gc.cpu().numpy()[perm.numpy()]) < 1e-5
    model.engine.check_async_errors()


@pytest.mark.parametrize("sym", [False, True])
def test_one_training_step_with_self_loops_against_fp64(sym):
    """One training step (``dropout_p = 0``) of ``STEGraphSAGE`` on a graph with two learned self loops: logits and weight
    gradients against a dense fp64 autograd restatement of the model (mean aggregation over the stored row, the self loop
    included).  Tolerance: tests/test_gpu_train.py's (1e-4 relative per tensor)."""
    import laplace_gnn_amd as lg

    N, F, H, C, M = 90, 10, 16, 4, 40
    gen = torch.Generator().manual_seed(61 + sym)
    ei = torch.randint(0, N, (2, 260), generator=gen)
    X = torch.randn(N, F, generator=gen)
    loops = torch.tensor([4, 57])
    torch.manual_seed(7)
    model = lg.STEGraphSAGE(F, H, C, 2, X, ei, None, dropout_p=0.0, symmetric=sym, candidates=torch.stack([loops, loops])).cuda()
    assert _switch_on(model, torch.stack([loops, loops])) == 2
    idx = torch.randperm(N, generator=gen)[:M]
    idx[0], idx[1], idx[6] = 4, 57, 4
    y = torch.randint(0, C, (M,), generator=gen)
    model.train()
    f = model(idx.cuda())
    loss = F_.cross_entropy(f, y.cuda())
    loss.backward()
    assert model.adj.grad is None  # the training forward differentiates the weights only
    A = model.full_adj().cpu().double()
    assert float(A.diagonal().sum()) == 2.0 and float(A[4, 4]) == 1.0
    rs = A.sum(1, keepdim=True)
    P = A / torch.where(rs == 0, torch.ones_like(rs), rs)
    prm = {k: t.detach().cpu().double().requires_grad_(True) for k, t in model.named_parameters() if "adj" not in k}
    x = X.double()
    h = torch.relu(torch.cat([x, P @ x], 1) @ prm["convs.0.lin.weight"].T + prm["convs.0.lin.bias"])
    out = torch.cat([h, P @ h], 1) @ prm["convs.1.lin.weight"].T + prm["convs.1.lin.bias"]
    rf = out[idx]
    F_.cross_entropy(rf, y).backward()
    e = rel(f.detach().cpu().numpy(), rf.detach().numpy())
    print(f"sym={sym} logits: {e:.2e}")
    assert e <= 1e-4
    for k, t in model.named_parameters():
        if "adj" in k:
            continue
        e = rel(t.grad.cpu().numpy(), prm[k].grad.numpy())
        print(f"sym={sym} {k}: {e:.2e}")
        assert e <= 1e-4, k
    model.engine.check_async_errors()
