"""The product wave's pair loop of paths_fused_kernel (csrc/paths_fused.hip): a node's first step starts the
accumulators (C = 0, nothing clears them between nodes), a chunk's last pair leaves out an empty second step, the node
ranges come from a register window refilled every 32 nodes, the hand-off counters are LDS stores.  Random graphs hit the step
(4 paths), pair (8) and chunk (64) boundaries only by chance, so the graphs here are built to hit them: "spokes" -- a
destination node joined to one middle node that is joined to exactly k batch nodes -- on top of a random background.  Every
node's path count is recomputed on the CPU and the wanted counts are asserted to occur.  The defect this loop once had was
intermittent: every comparison of the prescribed-count cases is made on five consecutive accumulates into fresh buffers.

Bounds as in test_gpu_paths.py: rel < 1e-4 per factor block and loss against the CPU oracle, rel < 2e-5 for B_0 against the
class-plane route of the same library."""
import functools

import numpy as np
import pytest
import torch

import gnn_laplace_oracle as O
from gpu_utils import oracle_from_arrays, rel
from test_gpu_scale import _engine, _make

pytestmark = pytest.mark.gpu
RTOL = 1e-4
# step and pair boundaries; chunk boundaries, and a second chunk that is a half pair
KS = [0, 1, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17, 63, 64, 65, 68, 69, 72, 73, 128, 129]
N_NODES, M_BATCH = 3000, 170
N_LEAF_HOSTS, LEAVES = 39, 10  # batch nodes no spoke uses, each joined to ten nodes that have no other edge (2 paths each)
RESERVED = 2 * len(KS) + N_LEAF_HOSTS * LEAVES
REPEATS = 5


@functools.lru_cache(maxsize=None)
def _spoke_graph(bg_edges, seed=0):
    """edge_index [2, E] and the batch's ids [M_BATCH] (one id listed twice).  The last RESERVED nodes are the spokes'
    destination and middle nodes, then the leaves: no background edge touches them and none is in the batch."""
    g = torch.Generator().manual_seed(seed)
    free = N_NODES - RESERVED
    batch = torch.randperm(free, generator=g)[:M_BATCH - 1]
    idx = torch.cat([batch[:60], batch[3:4], batch[60:]])  # a node id listed twice accumulates
    edges = [torch.randint(0, free, (2, bg_edges), generator=g)]
    spoke_batch = batch[:len(batch) - N_LEAF_HOSTS]
    for j, k in enumerate(KS):
        d, c = free + 2 * j, free + 2 * j + 1
        edges.append(torch.tensor([[d], [c]]))
        if k:
            nb = spoke_batch[torch.randperm(len(spoke_batch), generator=g)[:k]]
            edges.append(torch.stack([torch.full((k,), c, dtype=torch.int64), nb]))
    leaves = free + 2 * len(KS) + torch.arange(N_LEAF_HOSTS * LEAVES)
    edges.append(torch.stack([leaves, batch[len(batch) - N_LEAF_HOSTS:].repeat_interleave(LEAVES)]))
    return torch.cat(edges, 1), idx


def _path_counts(ei, idx, kind="gcn"):
    """Per destination node the number of paths the fused kernel runs for this batch, and the graph's expected paths per
    node as kfac_paths_first_layer evaluates it.  A path is (n <- v <- u) with v in row n and u in row v of the symmetrised
    adjacency (GCN: with self loops) for every DISTINCT batch node u: an id listed twice is one path of doubled weight."""
    rp, col = O.edge_index_to_adj_csr(ei.numpy(), N_NODES, kind, True)
    rows = np.repeat(np.arange(N_NODES), np.diff(rp))
    in_batch = np.zeros(N_NODES)
    in_batch[np.unique(idx.numpy())] = 1
    one_hop = np.bincount(rows, weights=in_batch[col], minlength=N_NODES)
    two_hop = np.bincount(rows, weights=one_hop[col], minlength=N_NODES)
    deg = np.diff(rp).astype(np.float64)
    ppn = float((deg * deg).sum()) / N_NODES * len(idx) / N_NODES
    return one_hop.astype(np.int64), two_hop.astype(np.int64), ppn


def _steps(k):  # 4-path steps of a node with k paths: chunks of 64, at least one step
    return max(sum(-(-min(64, k - s) // 4) for s in range(0, k, 64)), 1)


def _assert_counts(ei, idx, list_instance):
    _, cnt, ppn = _path_counts(ei, idx)
    free = N_NODES - RESERVED
    for j, k in enumerate(KS):
        assert cnt[free + 2 * j] == k, (k, cnt[free + 2 * j])
    steps = np.array([_steps(int(k)) for k in cnt])
    assert (steps % 2 == 1).any() and (steps % 2 == 0).any()
    assert (ppn < 2.5) == list_instance, ppn  # (the node-list instance runs below 2.5 expected paths per node)
    return cnt


def test_the_two_graphs_fall_on_either_side_of_the_node_list_threshold():
    dense = _assert_counts(*_spoke_graph(9000), list_instance=False)
    sparse = _assert_counts(*_spoke_graph(150), list_instance=True)
    # the sparse graph is the half pair's main case: most of its nodes with paths need exactly one step
    with_paths = sparse[sparse > 0]
    assert (with_paths <= 4).mean() > 0.5 and (dense > 8).any()


@functools.lru_cache(maxsize=None)
def _case(H, C, bg_edges, fork_exact, regression):
    """The model, the batch and the oracle's factors of one case (computed once, shared by the repeats)."""
    ei, idx = _spoke_graph(bg_edges)
    _, X, Ws, bs = _make("gcn", N_NODES, 24, H, C, 10, L=2, seed=H + C)
    g = torch.Generator().manual_seed(7)
    y = torch.randn(len(idx), C, generator=g) if regression else torch.randint(0, C, (len(idx),), generator=g)
    om = oracle_from_arrays("gcn", N_NODES, ei.numpy(), X.numpy(), [w.numpy() for w in Ws], [b.numpy() for b in bs], True)
    oloss, okf = O.kfac_batch(om, idx.numpy(), y.numpy(), len(idx), fork_exact,
                              likelihood="regression" if regression else "classification")
    return ei, idx, X, Ws, bs, y, oloss, okf


def _run_case(H, C, bg_edges, fork_exact=True, regression=False):
    import laplace_gnn_amd as lg

    ei, idx, X, Ws, bs, y, oloss, okf = _case(H, C, bg_edges, fork_exact, regression)
    M = len(idx)
    if regression:
        eng = lg.GraphEngine(ei.cuda(), N_NODES, kind="gcn", symmetric=True)
        eng.bind(X.cuda(), [w.cuda() for w in Ws], [b.cuda() for b in bs], likelihood="regression")
    else:
        eng = _engine("gcn", N_NODES, ei, X, Ws, bs)
    idx_d, y_d = idx.cuda(), y.cuda()
    _, plane, _ = eng.new_kfac_buffers()
    eng.kfac_accumulate(idx_d, y_d, M, plane, eng.new_kfac_buffers()[2], fork_exact=fork_exact, paths=False)
    assert not eng.last_kfac_used_paths
    torch.cuda.synchronize()
    plane_B0 = plane[0][1].cpu().numpy()
    scale = np.sqrt(0.5) if regression else 1.0  # (the oracle applied the interface's factor; the engine returns raw factors)
    for r in range(REPEATS):
        _, views, loss = eng.new_kfac_buffers()
        eng.kfac_accumulate(idx_d, y_d, M, views, loss, fork_exact=fork_exact, paths=True)
        assert eng.last_kfac_used_paths  # (otherwise the plane route would be compared with itself)
        torch.cuda.synchronize()
        for l, (A, B) in enumerate(views):
            e = rel(B.cpu().numpy() * scale, okf[2 * l][0])
            print(f"H={H} C={C} bg={bg_edges} repeat {r}: B_{l} vs oracle {e:.2e}")
            assert e < RTOL, f"B_{l} vs oracle, repeat {r}"
            if not regression:
                assert rel(A.cpu().numpy(), okf[2 * l][1]) < RTOL, f"A_{l} vs oracle, repeat {r}"
        e = rel(views[0][1].cpu().numpy(), plane_B0)
        print(f"H={H} C={C} bg={bg_edges} repeat {r}: B_0 vs the plane route {e:.2e}")
        assert e < 2e-5, f"B_0 vs the plane route, repeat {r}"
        assert torch.equal(views[0][1], views[0][1].T)
        if not regression:
            assert abs(float(loss) - float(oloss)) <= RTOL * abs(float(oloss)), f"loss, repeat {r}"
    eng.check_async_errors()
    eng.close()


@pytest.mark.parametrize("H,C", [(256, 40), (192, 7), (132, 33), (256, 50)])  # (50 classes: a second, HI launch)
@pytest.mark.parametrize("bg_edges", [9000, 150])  # the plain and the node-list instance
def test_prescribed_path_counts_vs_oracle_and_plane_route(H, C, bg_edges):
    _run_case(H, C, bg_edges)


def test_prescribed_path_counts_without_the_exact_fork():
    _run_case(256, 40, 9000, fork_exact=False)


@pytest.mark.parametrize("bg_edges", [9000, 150])
def test_prescribed_path_counts_regression_likelihood(bg_edges):
    """V = sqrt(2) I: only the alpha products run (the NOBG bodies of the pair loop)."""
    _run_case(256, 40, bg_edges, regression=True)


def test_prescribed_path_counts_fp32_gram_role(monkeypatch):
    """LGNN_GRAM_F32=1 (read per call): the fp32 tile write shares the pair loop."""
    monkeypatch.setenv("LGNN_GRAM_F32", "1")
    _run_case(256, 40, 9000)


def test_graphsage_one_hop_route_prescribed_neighbour_counts():
    """The same product role over one-hop paths: isolated nodes and nodes with exactly 1, 4, 5, 8 and 9 batch neighbours
    (a step, a step and a half pair, a pair, a pair and a half)."""
    import laplace_gnn_amd as lg

    H, C = 256, 40
    ks = [1, 4, 5, 8, 9] * 4
    g = torch.Generator().manual_seed(3)
    free = N_NODES - len(ks) - 200  # the last 200 nodes are isolated, the len(ks) before them the prescribed ones
    batch = torch.randperm(free, generator=g)[:M_BATCH - 3]
    idx = torch.cat([batch, batch[5:6], torch.tensor([N_NODES - 1, N_NODES - 2])])  # a duplicate and two isolated nodes
    edges = [torch.randint(0, free, (2, 4000), generator=g)]
    for j, k in enumerate(ks):
        nb = batch[torch.randperm(len(batch), generator=g)[:k]]
        edges.append(torch.stack([torch.full((k,), free + j, dtype=torch.int64), nb]))
    ei = torch.cat(edges, 1)
    one_hop, _, _ = _path_counts(ei, idx, "sage")
    assert [int(one_hop[free + j]) for j in range(len(ks))] == ks
    assert (one_hop[N_NODES - 200:] == 0).all()
    _, X, Ws, bs = _make("sage", N_NODES, 24, H, C, 10, L=2, seed=11)
    y = torch.randint(0, C, (len(idx),), generator=g)
    eng = lg.GraphEngine(ei.cuda(), N_NODES, kind="sage", symmetric=True)
    eng.bind(X.cuda(), [w.cuda() for w in Ws], [b.cuda() for b in bs])
    om = oracle_from_arrays("sage", N_NODES, ei.numpy(), X.numpy(), [w.numpy() for w in Ws], [b.numpy() for b in bs], True)
    oloss, okf = O.kfac_batch(om, idx.numpy(), y.numpy(), len(idx))
    _, plane, _ = eng.new_kfac_buffers()
    eng.kfac_accumulate(idx.cuda(), y.cuda(), len(idx), plane, eng.new_kfac_buffers()[2], paths=False)
    assert not eng.last_kfac_used_paths
    for r in range(2):
        _, views, loss = eng.new_kfac_buffers()
        eng.kfac_accumulate(idx.cuda(), y.cuda(), len(idx), views, loss)
        assert eng.last_kfac_used_paths
        torch.cuda.synchronize()
        for l, (A, B) in enumerate(views):
            assert rel(B.cpu().numpy(), okf[2 * l][0]) < RTOL, f"B_{l} vs oracle, repeat {r}"
            assert rel(A.cpu().numpy(), okf[2 * l][1]) < RTOL, f"A_{l} vs oracle, repeat {r}"
        assert rel(views[0][1].cpu().numpy(), plane[0][1].cpu().numpy()) < 2e-5, f"B_0 vs the plane route, repeat {r}"
        assert abs(float(loss) - float(oloss)) <= RTOL * abs(float(oloss))
    eng.check_async_errors()
    eng.close()
