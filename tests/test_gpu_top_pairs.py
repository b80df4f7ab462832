"""The GCN top layer of the two-hop path route from sample pairs (csrc/toppairs.hip): ``B_1`` as one MFMA K step
per sample and per pair of samples that share a node, against

* the CPU oracle at the bar of ``test_gpu_paths.py`` (``B_0`` and ``B_1``), 1e-4,
* the plane route (``paths=False``: ``seed_spmm_gram_kernel``) on the same inputs, 2e-5,
* the fp64 restatement of ``B_1`` of ``test_gpu_top_tiles.py`` at that file's bound, 4.886e-7.

Every case asserts the route and the top-layer kernel of every call (``last_kfac_used_paths``, ``last_kfac_top_kernel``) and
makes every comparison on three consecutive fits of the same device tensors: the batch-structure cache sees the batch for the
first time, builds its entry (R, the path list, the pair lists), and hits it.  ``LGNN_PAIR_LIST_CAP=1`` sends three of the class
counts to ``top_tiles_kernel`` at the same bounds.

Shapes: N = 300, F = 8, H = 132 (the path route's smallest width), M <= 64 -- except the prescribed graph, whose row of 66 batch
neighbours needs a batch of 70.
"""
import numpy as np
import pytest
import torch

import gnn_laplace_oracle as O
from gpu_utils import oracle_from_arrays, rel
from test_gpu_scale import _make
from test_gpu_top_tiles import BOUND, RTOL, _b1_fp64, _dense_p, _labels

pytestmark = pytest.mark.gpu

F, H, N = 8, 132, 300
SEED_SPMM_GRAM, TILES, PAIRS = 0, 1, 2


def _engine(ei, X, Ws, bs, mode, symmetric=True):
    import laplace_gnn_amd as lg

    eng = lg.GraphEngine(ei.cuda(), N, kind="gcn", symmetric=symmetric)
    eng.bind(X.cuda(), [w.cuda() for w in Ws], [b.cuda() for b in bs],
             likelihood="regression" if mode == "regression" else "classification")
    return eng


def _fit(eng, batches, ys, n_train, mode, paths, kernel, cuts=None):
    """one fit; asserts the route and the top-layer kernel of every call.  Returns [B_0, B_1] (fp64 numpy)."""
    _, views, loss = eng.new_kfac_buffers()
    C = eng.dims[-1]
    for idx, y in zip(batches, ys):
        for a, b in (zip(cuts[:-1], cuts[1:]) if cuts else [(0, C)]):
            eng.kfac_accumulate(idx, y, n_train, views, loss, fork_exact=mode == "fork", paths=paths, classes=(a, b))
            assert eng.last_kfac_used_paths == bool(paths)
            assert eng.last_kfac_top_kernel == kernel
            assert eng.last_kfac_top_on_tiles == (kernel != SEED_SPMM_GRAM)
    torch.cuda.synchronize()
    return [B.cpu().numpy().astype(np.float64) for _, B in views]


def _references(eng, ei, X, Ws, bs, batches, ys, mode, symmetric):
    """(the plane route's [B_0, B_1], the fp64 restatement of B_1, the oracle's [B_0, B_1]): computed once per case"""
    n_train = sum(len(b) for b in batches)
    old = _fit(eng, [b.cuda() for b in batches], [y.cuda() for y in ys], n_train, mode, False, SEED_SPMM_GRAM)
    P = _dense_p(eng, N)
    logits = eng.forward_all().cpu().double()
    ref = sum(_b1_fp64(P, logits, b, mode) for b in batches)
    om = oracle_from_arrays("gcn", N, ei.numpy(), X.numpy(), [w.numpy() for w in Ws], [b.numpy() for b in bs], symmetric)
    oB = [0.0, 0.0]
    for b, y in zip(batches, ys):
        _, kf = O.kfac_batch(om, b.numpy(), y.numpy(), n_train, fork_exact=mode == "fork",
                             likelihood="regression" if mode == "regression" else "classification")
        scale = np.sqrt(2.0) if mode == "regression" else 1.0  # (the oracle applied the interface's sqrt(.5) per factor)
        oB = [oB[l] + scale * kf[2 * l][0].astype(np.float64) for l in range(2)]
    return old, ref, oB


def _compare(what, new, old, ref, oB, C, mode):
    assert np.isfinite(new[0]).all() and np.isfinite(new[1]).all()
    if C == 1 and mode != "regression":  # one class: the seed is exactly zero (p = 1); every kernel leaves cancellation residue
        assert max(np.abs(new[1]).max(), np.abs(old[1]).max(), np.abs(ref).max()) < 1e-10
        # ... and with it B_0: zero in the oracle; on either route a row of Y is a cancellation residue of a few fp32 ulps of
        # |w| |W_1| (<= 1e-6 here) and B_0 sums the squares of a few thousand of them: the same bound holds with room
        print(f"{what}: one class, max |B_0| {np.abs(new[0]).max():.3e} (plane route {np.abs(old[0]).max():.3e}), "
              f"max |B_1| {np.abs(new[1]).max():.3e}")
        assert max(np.abs(new[0]).max(), np.abs(old[0]).max(), np.abs(oB[0]).max()) < 1e-10
        return
    e = rel(new[1], ref)
    print(f"{what}: B_1 vs fp64 {e:.3e} (bound {BOUND:.3e}; seed_spmm_gram {rel(old[1], ref):.3e}), vs oracle "
          f"{rel(new[1], oB[1]):.3e}, vs plane route {rel(new[1], old[1]):.3e}; B_0 vs oracle {rel(new[0], oB[0]):.3e}, "
          f"vs plane route {rel(new[0], old[0]):.3e}")
    assert rel(new[1], oB[1]) < RTOL and rel(new[0], oB[0]) < RTOL, what
    assert rel(new[1], old[1]) < 2e-5 and rel(new[0], old[0]) < 2e-5, what
    assert np.array_equal(new[1], new[1].T)
    assert e <= BOUND, (what, e, BOUND)


def _check(what, ei, C, batches, mode="fork", cuts=None, kernel=PAIRS, seed=0, ws_limit=None, symmetric=True):
    _, X, Ws, bs = _make("gcn", N, F, H, C, 1, L=2, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    ys = [_labels(mode, len(b), C, g) for b in batches]
    n_train = sum(len(b) for b in batches)
    eng = _engine(ei, X, Ws, bs, mode, symmetric)
    if ws_limit:
        eng.set_workspace_limit(ws_limit)
    old, ref, oB = _references(eng, ei, X, Ws, bs, batches, ys, mode, symmetric)
    dev, ydev = [b.cuda() for b in batches], [y.cuda() for y in ys]
    for rep in range(3):
        new = _fit(eng, dev, ydev, n_train, mode, True, kernel, cuts)
        _compare(f"{what} fit {rep}", new, old, ref, oB, C, mode)
    eng.check_async_errors()
    eng.close()


def _random_graph(E, seed):
    return torch.randint(0, N, (2, E), generator=torch.Generator().manual_seed(seed))


def _random_batches(M, parts, seed):
    idx = torch.randperm(N, generator=torch.Generator().manual_seed(seed))[:M]
    return list(idx.chunk(parts))


# class count -> class cuts under the smallest workspace limit, or None
CLASS_CASES = {1: None, 7: None, 16: None, 17: None, 33: [0, 1, 20, 33], 40: None, 48: None, 49: None, 64: [0, 5, 37, 64]}


@pytest.mark.parametrize("C", sorted(CLASS_CASES))
def test_class_counts_and_class_ranges(C):
    cuts = CLASS_CASES[C]
    _check(f"C={C}", _random_graph(900, C), C, _random_batches(64, 2, C + 1), cuts=cuts, seed=C,
           ws_limit=(1 << 20) if cuts else None)


@pytest.mark.parametrize("C", [7, 40, 64])
def test_a_pair_list_that_cannot_hold_the_bound_keeps_the_tile_kernel(C, monkeypatch):
    monkeypatch.setenv("LGNN_PAIR_LIST_CAP", "1")
    _check(f"tiles C={C}", _random_graph(900, C), C, _random_batches(64, 2, C + 1), cuts=CLASS_CASES[C], kernel=TILES, seed=C,
           ws_limit=(1 << 20) if CLASS_CASES[C] else None)


def _adjacency(ei, symmetric=True):
    A = torch.zeros(N, N)
    A[ei[0], ei[1]] = 1.0
    if symmetric:
        A = A + A.T
    return ((A + torch.eye(N)) > 0).float()  # what the GCN's propagation matrix connects: self loops


def test_prescribed_neighbour_counts():
    """Batch = nodes 0 .. 69.  Node 200 + t is joined to exactly the batch nodes 0 .. k_t - 1; nodes 206 .. 299 have no edge."""
    M, ks = 70, [1, 2, 3, 8, 9, 66]
    src, dst = [], []
    for t, k in enumerate(ks):
        src += [200 + t] * k
        dst += list(range(k))
    ei = torch.tensor([src, dst])
    inb = torch.zeros(N)
    inb[:M] = 1.0
    cnt = (_adjacency(ei) @ inb).long()  # d_n: the entries of row n of R
    assert [int(cnt[200 + t]) for t in range(len(ks))] == ks
    assert int(cnt[206:].sum()) == 0  # no batch neighbour: no entry
    assert all(int(cnt[n]) == 1 for n in range(M))  # a batch node's only batch neighbour is itself (self loop)
    assert sorted(set(cnt.tolist())) == [0, 1, 2, 3, 8, 9, 66]
    assert int((cnt * (cnt - 1) // 2).sum()) == sum(k * (k - 1) // 2 for k in ks) == 2213  # the pair terms; M sample terms
    for C in (40, 7):
        _check(f"prescribed C={C}", ei, C, [torch.arange(M)], seed=C)


def _shared_graph():
    """batch nodes 0 and 1 share the three nodes 100, 101, 102 (outside the batch); batch node 5 has no edge: its only batch
    neighbour is its self loop; random edges among the nodes 10 .. 99"""
    shared = torch.tensor([[0, 1, 0, 1, 0, 1], [100, 100, 101, 101, 102, 102]])
    rest = 10 + torch.randint(0, 90, (2, 300), generator=torch.Generator().manual_seed(21))
    return torch.cat([shared, rest], 1)


def test_a_pair_that_shares_three_nodes_a_lone_self_loop_and_repeated_ids():
    ei = _shared_graph()
    A = _adjacency(ei)
    assert int((A[0] * A[1]).sum()) == 3 and int(A[5].sum()) == 1
    base = torch.cat([torch.tensor([0, 1, 5]), 10 + torch.randperm(90, generator=torch.Generator().manual_seed(22))[:40]])
    _check("shared pair", ei, 17, [base], seed=23)
    r = int(base[10])
    idx = torch.cat([base, torch.tensor([0, r, r])])  # node 0 (of the shared pair) twice, another batch node three times
    assert int((idx == 0).sum()) == 2 and int((idx == r).sum()) == 3 and len(idx) <= 64
    _check("repeated ids", ei, 17, [idx], seed=24)


def test_directed_graph():
    ei = _random_graph(900, 31)
    A = _adjacency(ei, symmetric=False)
    assert not torch.equal(A, A.T)
    _check("directed", ei, 40, _random_batches(64, 2, 32), seed=33, symmetric=False)


@pytest.mark.parametrize("mode", ["fork", "upstream", "regression"])
def test_seed_modes(mode):
    _check(f"mode={mode}", _random_graph(900, 6), 17, _random_batches(64, 2, 7), mode=mode, seed=8)


def test_cache_paths(monkeypatch):
    """a tagged batch three times (first sight, build, hit), an untagged batch, and the cache switched off: the pair lists are
    the entry's on a hit and the workspace's otherwise"""
    C, M = 40, 64
    ei = _random_graph(900, 9)
    _, X, Ws, bs = _make("gcn", N, F, H, C, 1, L=2, seed=10)
    g = torch.Generator().manual_seed(11)
    idx = torch.randperm(N, generator=g)[:M]
    y = torch.randint(0, C, (M,), generator=g)
    monkeypatch.delenv("LGNN_BATCH_CACHE_MB", raising=False)
    eng = _engine(ei, X, Ws, bs, "fork")
    old, ref, oB = _references(eng, ei, X, Ws, bs, [idx], [y], "fork", True)
    idx_d, y_d = idx.cuda(), y.cuda()
    untagged = torch.stack([idx_d, idx_d], 1)[:, 0]  # not contiguous: handed over as a copy, never tagged
    assert not untagged.is_contiguous()

    def fit(what, i, expect, kernel=PAIRS):
        s0 = eng.batch_cache_stats()
        for rep in range(3 if expect is None else 1):
            new = _fit(eng, [i], [y_d], M, "fork", True, kernel)
            _compare(f"cache {what} {rep}", new, old, ref, oB, C, "fork")
        s1 = eng.batch_cache_stats()
        want = expect or {"hits": 0, "misses": 0, "builds": 0}
        assert {k: s1[k] - s0[k] for k in ("hits", "misses", "builds")} == want, (what, s0, s1)
        return s1

    none = {"hits": 0, "misses": 0, "builds": 0}
    s0 = fit("first sight", idx_d, {**none, "misses": 1})
    s1 = fit("build", idx_d, {**none, "builds": 1})
    assert s1["entries"] == 1 and s1["bytes"] > s0["bytes"]
    s2 = fit("hit", idx_d, {**none, "hits": 1})
    assert s2["bytes"] == s1["bytes"]
    # the pair lists are counted in the entry's bytes: the same batch under another tag, its entry built while the tile kernel
    # runs (no pair lists), then hit by the pair kernel, which builds them from the entry's R and adds them
    inb = torch.zeros(N)
    inb[idx] = 1.0
    d = (_adjacency(ei) @ inb).long()
    n_pairs = int((d * (d - 1) // 2).sum())
    assert n_pairs > 0
    idx_2 = idx_d.clone()
    monkeypatch.setenv("LGNN_PAIR_LIST_CAP", "1")
    fit("first sight, tiles", idx_2, {**none, "misses": 1}, TILES)
    t1 = fit("build, tiles", idx_2, {**none, "builds": 1}, TILES)
    assert t1["entries"] == 2 and t1["bytes"] - s2["bytes"] == s1["bytes"] - 4 * M - 12 * n_pairs - 4
    monkeypatch.delenv("LGNN_PAIR_LIST_CAP")
    t2 = fit("hit, pairs added", idx_2, {**none, "hits": 1})
    assert t2["entries"] == 2 and t2["bytes"] - t1["bytes"] == 4 * M + 12 * n_pairs + 4
    t3 = fit("hit", idx_2, {**none, "hits": 1})
    assert t3["bytes"] == t2["bytes"] == 2 * s1["bytes"]
    fit("untagged", untagged, None)
    monkeypatch.setenv("LGNN_BATCH_CACHE_MB", "0")
    fit("cache off", idx_d, None)
    assert eng.batch_cache_stats()["entries"] == 0
    eng.check_async_errors()
    eng.close()
