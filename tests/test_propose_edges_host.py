"""CPU tests of the host side of ``DiagLaplace.propose_edges`` (laplace_gnn_amd/adjgrad.py: ``_band_plan``, ``_deal_to_bands``,
``_propose_edges_drive``) with a stand-in engine that records its calls and fills each band from a known [N, N] matrix (plain
tensors, no library, no GPU, as tests/test_adjgrad_front_host.py), and of ``STEGCN.add_candidates``."""
import types

import pytest
import torch

import laplace_gnn_amd as lg
from laplace_gnn_amd import adjgrad as ag

N, F, H, C = 200, 4, 5, 3


class BandEngine:
    """``band_finish`` writes ``band[t, i] = G[i, a0 + t]`` (+inf on the diagonal and the stored pairs), what the device leaves."""
    device = torch.device("cpu")
    kind, num_nodes, num_layers, has_extras, is_symmetric, act = "gcn", N, 2, False, False, "relu"
    dims = (F, H, C)

    def __init__(self, G, stored, workspace_limit=32 << 30):
        self.G, self.stored, self.nnz, self.workspace_limit = G, stored, stored.shape[1], workspace_limit
        self.sparse, self.band_batches, self.band_finishes, self.order = [], [], [], []

    def set_likelihood(self, likelihood):
        self.order.append("likelihood")

    def forward(self, idx):
        self.order.append("forward")  # (synchronises the parameter versions)

    def diag_adjgrad_band_sparse(self, X, y, gamma, grad_P, out_bar, h1_bar, e_bar, loss_scale=1.0):
        self.sparse.append((X.clone(), y.clone()))
        self.order.append("batch")

    def diag_adjgrad_band_prepare(self, out_bar, h1_bar, e_bar, grad_P):
        assert tuple(e_bar.shape) == (N, F + 1) and tuple(grad_P.shape) == (self.nnz,)
        self.order.append("prepare")
        return ("Hb", "Z0", "Z1", "rs", "cs")

    def diag_adjgrad_band_batch(self, idx, y, gamma, a0, a1, band):
        assert tuple(band.shape) == (a1 - a0, N) and bool((band == 0).all())
        self.band_batches.append((idx.clone(), y.clone(), a0, a1))
        self.order.append("band_batch")

    def diag_adjgrad_band_finish(self, out_bar, prepared, e_bar, a0, a1, band):
        assert prepared == ("Hb", "Z0", "Z1", "rs", "cs") and tuple(band.shape) == (a1 - a0, N) and band.is_contiguous()
        masked = self.G.clone()
        masked[self.stored[0], self.stored[1]] = float("inf")
        masked.fill_diagonal_(float("inf"))
        band.copy_(masked[:, a0:a1].t())
        self.band_finishes.append((a0, a1))
        self.order.append("band_finish")
        return band


def _setup(seed=0, ties=False):
    gen = torch.Generator().manual_seed(seed)
    G = torch.randn(N, N, generator=gen)
    if ties:
        G = torch.round(G * 2) / 2  # a few dozen distinct values: large tie groups
    stored = torch.unique(torch.randint(0, N, (2, 600), generator=gen), dim=1)
    idx = torch.randint(0, N, (70,), generator=gen)
    y = torch.randint(0, C, (70,), generator=gen)
    return G, stored, idx, y


# ---- band boundaries --------------------------------------------------------------------------------------------------
def test_band_plan_boundaries_ragged_last_band_and_defaults():
    assert ag._band_plan(300, 128 * 4 * 300, None) == (128, [(0, 128), (128, 256), (256, 300)])
    assert ag._band_plan(300, 128 * 4 * 300 + 4 * 300 * 63, None)[0] == 128  # rounded DOWN to whole 64-row tiles
    assert ag._band_plan(512, 128 * 4 * 512, None) == (128, [(0, 128), (128, 256), (256, 384), (384, 512)])
    assert ag._band_plan(64, 128 * 4 * 64, None) == (128, [(0, 64)])  # one ragged band
    assert ag._band_plan(64, 64 * 4 * 64, None) == (64, [(0, 64)])  # exactly one tile
    with pytest.raises(ValueError, match="band_bytes"):
        ag._band_plan(64, 64 * 4 * 64 - 1, None)
    with pytest.raises(ValueError, match="band_bytes"):
        ag._band_plan(300, 0, None)
    # default: the smaller of the workspace limit and 1 GiB
    assert ag._band_plan(600, None, 1 << 20) == (384, [(0, 384), (384, 600)])
    assert ag._band_plan(600, None, 32 << 30) == ag._band_plan(600, 1 << 30, None) == ag._band_plan(600, None, None)
    h, bands = ag._band_plan(169_343, None, 32 << 30)
    assert h == (1 << 30) // (4 * 169_343) // 64 * 64 == 1536 and len(bands) == 111 and bands[-1] == (110 * 1536, 169_343)
    for n, bb in [(300, 128 * 4 * 300), (169_343, 1 << 30), (65, 64 * 4 * 65)]:
        h, bands = ag._band_plan(n, bb, None)
        assert bands[0][0] == 0 and bands[-1][1] == n and all(a[1] == b[0] for a, b in zip(bands, bands[1:]))
        assert all(a1 - a0 == h for a0, a1 in bands[:-1]) and 0 < bands[-1][1] - bands[-1][0] <= h and h * 4 * n <= bb


def test_every_sample_is_dealt_to_exactly_one_band():
    idx = torch.tensor([5, 299, 128, 127, 5, 256, 0, 255, 1000, -3])
    order, counts = ag._deal_to_bands(idx, 128, 3)
    assert counts == [5, 2, 3] and sorted(order.tolist()) == list(range(10))
    assert idx[order].tolist() == [5, 127, 5, 0, -3, 128, 255, 299, 256, 1000]  # the loader's order within a band
    order, counts = ag._deal_to_bands(idx, 320, 1)
    assert counts == [10] and order.tolist() == list(range(10))


# ---- the driver ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("rows", [64, 128, 256])
@pytest.mark.parametrize("k", [1, 50, N * N])
def test_driver_returns_the_smallest_eligible_entries(rows, k, ties):
    G, stored, idx, y = _setup(ties=ties)
    eng = BandEngine(G, stored)
    loader = lg.TensorBatchLoader(idx, y, batch_size=32)  # 32 / 32 / 6
    pairs, grad = ag._propose_edges_drive(eng, loader, k, rows * 4 * N, weight=torch.ones(3), loss_scale=1.0)
    height, bands = ag._band_plan(N, rows * 4 * N, None)
    # one sparse pass over the loader's batches, then prepare, then per band: its samples, then its finish
    assert [x.tolist() for x, _ in eng.sparse] == [idx[:32].tolist(), idx[32:64].tolist(), idx[64:].tolist()]
    assert eng.order[:6] == ["likelihood", "forward", "batch", "batch", "batch", "prepare"]
    assert eng.band_finishes == bands
    seen = torch.cat([b[0] for b in eng.band_batches])
    assert sorted(seen.tolist()) == sorted(idx.tolist())  # every sample once over all bands
    for bi, by, a0, a1 in eng.band_batches:
        assert (a0, a1) in bands and bool(((bi >= a0) & (bi < a1)).all()) and bi.numel() <= 32
        for n, lab in zip(bi.tolist(), by.tolist()):  # the labels travel with their samples
            assert lab in y[idx == n].tolist()
    last = {}
    for pos, what in enumerate(eng.order):
        last[what] = pos
    assert eng.order.index("band_batch") > eng.order.index("prepare") and last["band_finish"] == len(eng.order) - 1
    # the result: the k smallest eligible entries, ascending, pairs (i, j) with grad = G[i, j]
    ok = torch.ones(N, N, dtype=torch.bool)
    ok[stored[0], stored[1]] = False
    ok.fill_diagonal_(False)
    kk = min(k, int(ok.sum()))
    assert pairs.dtype == torch.int64 and tuple(pairs.shape) == (2, kk) and grad.dtype == torch.float32
    assert torch.equal(grad, G[pairs[0], pairs[1]]) and bool(ok[pairs[0], pairs[1]].all())
    assert torch.unique(pairs[0] * N + pairs[1]).numel() == kk
    assert torch.equal(grad, torch.sort(G[ok]).values[:kk])  # (ties: any member of a group -- the VALUES are determined)


def test_driver_caps_a_bands_pieces_by_the_loaders_batch():
    G, stored, _, _ = _setup()
    idx = torch.cat([torch.full((50,), 3), torch.full((20,), 150)])
    eng = BandEngine(G, stored)
    ag._propose_edges_drive(eng, lg.TensorBatchLoader(idx, torch.zeros(70, dtype=torch.int64), batch_size=16), 5, 128 * 4 * N,
                            weight=torch.ones(3), loss_scale=1.0)
    assert [(b[0].numel(), b[2], b[3]) for b in eng.band_batches] == [(16, 0, 128)] * 3 + [(2, 0, 128), (16, 128, 200), (4, 128, 200)]


def test_front_checks_k_scope_and_fit_in_that_order():
    model = torch.nn.Linear(2, 2)
    model.symmetric = False
    G, stored, idx, y = _setup()
    la = lg.DiagLaplace(model, "classification")
    la._backend = types.SimpleNamespace(engine=BandEngine(G, stored))
    loader = lg.TensorBatchLoader(idx, y, batch_size=32)
    with pytest.raises(ValueError, match="k must be"):
        la.propose_edges(loader, 0)
    with pytest.raises(AttributeError, match="not fitted"):
        la.propose_edges(loader, 3)
    for attr, value, cause in [("kind", "sage", "GraphSAGE"), ("num_layers", 1, "1-layer"), ("num_layers", 3, "3-layer"),
                               ("has_extras", True, "res / norm"), ("is_symmetric", True, "symmetric")]:
        eng = BandEngine(G, stored)
        setattr(eng, attr, value)
        la._backend = types.SimpleNamespace(engine=eng)
        with pytest.raises(NotImplementedError, match=cause):
            la.propose_edges(loader, 3)
    model.symmetric = True
    la._backend = types.SimpleNamespace(engine=BandEngine(G, stored))
    with pytest.raises(NotImplementedError, match="symmetric"):
        la.propose_edges(loader, 3)
    for cls in (lg.KronLaplace, lg.FullLaplace, lg.FunctionalLaplace, lg.LowRankLaplace):
        assert not hasattr(cls, "propose_edges")
    for cls in (lg.DiagLLLaplace, lg.DiagSubnetLaplace):  # they inherit from DiagLaplace: refused by name
        with pytest.raises(NotImplementedError, match="propose_edges"):
            cls.propose_edges(object(), loader, 3)


def test_front_refuses_a_distributed_world(monkeypatch):
    from laplace_gnn_amd import laplace as lp

    model = torch.nn.Linear(2, 2)
    G, stored, idx, y = _setup()
    la = lg.DiagLaplace(model, "classification")
    la._backend = types.SimpleNamespace(engine=BandEngine(G, stored))
    monkeypatch.setattr(lp, "_dist_info", lambda process_group: (0, 2))
    with pytest.raises(NotImplementedError, match="world larger than 1"):
        la.propose_edges(lg.TensorBatchLoader(idx, y, batch_size=32), 3)


# ---- add_candidates -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("cls", ["STEGCN", "STEGraphSAGE"])
def test_add_candidates_keeps_order_and_values(cls, masked):
    n = 8
    X = torch.randn(n, 3)
    ei = torch.tensor([[0, 1, 2, 3, 5], [1, 2, 3, 4, 0]])
    train = [0, 1, 5]
    model = getattr(lg, cls)(3, 4, 2, 2, X, ei, train_masked_update=masked, train_nodes=train if masked else None,
                             candidates=torch.tensor([[0], [7]]))
    with torch.no_grad():
        model.adj[2] = 0.7  # a learned value
    before = dict(zip((model.adj_index[0] * n + model.adj_index[1]).tolist(), model.adj.tolist()))
    old_param = model.adj
    added = model.add_candidates(torch.tensor([[5, 0, 3, 0, 1, 5], [1, 1, 3, 7, 0, 1]]))  # (0, 1), (0, 7) tracked; (5, 1) twice
    diag = cls == "STEGraphSAGE"  # GraphSAGE tracks (3, 3); a GCN drops its diagonal
    assert added == (3 if diag else 2)
    keys = (model.adj_index[0] * n + model.adj_index[1])
    assert bool((keys[1:] > keys[:-1]).all()) and model.adj.numel() == len(before) + added  # row-major sorted, no duplicates
    after = dict(zip(keys.tolist(), model.adj.tolist()))
    assert all(after[k] == v for k, v in before.items())  # old values in place
    new = {5 * n + 1, 1 * n + 0} | ({3 * n + 3} if diag else set())
    assert set(after) - set(before) == new and all(after[k] == 0.0 for k in new)
    assert isinstance(model.adj, torch.nn.Parameter) and model.adj is not old_param and model.adj.grad is None
    assert "adj" in dict(model.named_parameters()) and "adj_index" in dict(model.named_buffers())
    if masked:
        is_train = torch.zeros(n, dtype=torch.bool)
        is_train[train] = True
        both = is_train[model.adj_index[0]] & is_train[model.adj_index[1]]
        want = torch.where(both, torch.tensor(0.0 if diag else 0.1), torch.tensor(1.0))
        assert torch.equal(model.grad_adj_mask, want) and "grad_adj_mask" in dict(model.named_buffers())
    else:
        assert not hasattr(model, "grad_adj_mask")
    assert model.add_candidates(torch.tensor([[5, 0], [1, 1]])) == 0 and model.adj.numel() == len(after)
    with pytest.raises(ValueError, match="candidate"):
        model.add_candidates(torch.tensor([[0], [n]]))


def test_add_candidates_tracks_both_orientations_of_a_symmetric_model():
    n = 6
    model = lg.STEGCN(3, 4, 2, 2, torch.randn(n, 3), torch.tensor([[0, 1, 3], [1, 2, 0]]), symmetric=True)
    assert model.add_candidates(torch.tensor([[4], [2]])) == 2
    keys = (model.adj_index[0] * n + model.adj_index[1]).tolist()
    assert 4 * n + 2 in keys and 2 * n + 4 in keys and keys == sorted(keys)
