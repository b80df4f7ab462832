"""CPU tests of the host driver behind ``neg_marglik_adj_grad`` (laplace_gnn_amd/adjgrad.py: ``_adjgrad_drive``): which samples
each rank hands to the engine, what is all-reduced and in which order, the symmetric candidates' tail and the ``dense=True``
refusals -- with a stub engine that records its calls (plain tensors, no library, no GPU).  7 nodes, 3 classes, a loader with two
batches of 5 and 2 samples; ``_dist_info`` is patched to simulate the ranks of a job."""
import types

import pytest
import torch

import laplace_gnn_amd as lg
from laplace_gnn_amd import laplace as lp

N, F, H, C = 7, 4, 5, 3
IDX = torch.tensor([3, 0, 6, 1, 5, 2, 4])
Y = torch.tensor([0, 2, 1, 1, 0, 2, 1])
STORED = torch.tensor([[0, 0, 1, 2, 3, 4, 5, 6], [0, 1, 1, 2, 3, 4, 5, 6]])  # row-major sorted
CAND = torch.tensor([[0, 2, 5], [3, 6, 1]])  # K = 3 pairs (i, j), none stored
RANKS = [(0, 1), (0, 2), (1, 2)]


class StubEngine:
    """Records every call the driver makes; the finish returns recognisable tensors."""
    device = torch.device("cpu")
    num_nodes, num_layers, has_extras = N, 2, False

    def __init__(self, kind="gcn", dims=(F, H, C)):
        self.kind, self.dims, self.nnz = kind, dims, STORED.shape[1]
        self.num_layers = len(dims) - 1
        self.batches, self.finishes, self.likelihoods = [], [], []

    def export_adj(self):
        return STORED[0].clone(), STORED[1].clone()

    def set_likelihood(self, likelihood):
        self.likelihoods.append(likelihood)

    def _batch(self, name, X, y, weight, buffers, kw):
        self.batches.append(types.SimpleNamespace(name=name, X=X.clone(), y=y.clone(), weight=weight, buffers=buffers, kw=kw))

    def _finish(self, name, buffers, target, cand):
        self.finishes.append(types.SimpleNamespace(name=name, buffers=buffers, target=target, cand=cand))
        grad = torch.arange(target.numel(), dtype=torch.float32).reshape(target.shape) + 100.0
        return grad if cand is None else (grad, torch.arange(cand[0].numel(), dtype=torch.float32) ** 2)

    def adjgrad_batch(self, X, y, gB, grad_P, out_bar, fork_exact=True, loss_scale=1.0, cand=None):
        self._batch("adjgrad_batch", X, y, gB, [grad_P, out_bar], dict(fork_exact=fork_exact, loss_scale=loss_scale, cand=cand))

    def adjgrad_finish(self, out_bar, gA, a_scale, grad_P, cand=None):
        return self._finish("adjgrad_finish", [out_bar, gA, a_scale], grad_P, cand)

    def adjgrad_batch_dense(self, X, y, gB, out_bar, G, fork_exact=True, loss_scale=1.0):
        self._batch("adjgrad_batch_dense", X, y, gB, [G, out_bar], dict(fork_exact=fork_exact, loss_scale=loss_scale))

    def adjgrad_finish_dense(self, out_bar, gA, a_scale, G):
        return self._finish("adjgrad_finish_dense", [out_bar, gA, a_scale], G, None)

    def diag_adjgrad_batch(self, X, y, gamma, grad_P, out_bar, h1_bar, e_bar, loss_scale=1.0, cand=None):
        self._batch("diag_adjgrad_batch", X, y, gamma, [grad_P, out_bar, h1_bar, e_bar], dict(loss_scale=loss_scale, cand=cand))

    def full_adjgrad_batch(self, X, y, Gamma, grad_P, out_bar, h1_bar, e_bar, loss_scale=1.0, cand=None):
        self._batch("full_adjgrad_batch", X, y, Gamma, [grad_P, out_bar, h1_bar, e_bar], dict(loss_scale=loss_scale, cand=cand))

    def diag_adjgrad_finish(self, out_bar, h1_bar, e_bar, grad_P, cand=None):
        return self._finish("diag_adjgrad_finish", [out_bar, h1_bar, e_bar], grad_P, cand)

    def diag_adjgrad_batch_dense(self, X, y, gamma, out_bar, h1_bar, e_bar, G, loss_scale=1.0):
        self._batch("diag_adjgrad_batch_dense", X, y, gamma, [G, out_bar, h1_bar, e_bar], dict(loss_scale=loss_scale))

    def diag_adjgrad_finish_dense(self, out_bar, h1_bar, e_bar, G):
        return self._finish("diag_adjgrad_finish_dense", [out_bar, h1_bar, e_bar], G, None)


GB, GA = [torch.full((2, 2), 4.0), torch.full((3, 3), 8.0)], [torch.full((2, 2), 6.0), torch.full((3, 3), 10.0)]
BIG_GAMMA = torch.eye(9)


def _front(monkeypatch, structure, eng, symmetric=False):
    """A fitted-looking posterior of the given structure over the stub engine; its value and weighting are stubbed out (they
    are the class's own business, not the driver's)."""
    model = torch.nn.Linear(2, 2)
    model.symmetric = symmetric
    cls = {"kron": lg.KronLaplace, "diag": lg.DiagLaplace, "full": lg.FullLaplace}[structure]
    la = cls(model, "classification")
    la._backend = types.SimpleNamespace(engine=eng, fork_exact_seed=True)
    la.H_facs = la.H = object()
    la.n_data = 7
    monkeypatch.setattr(cls, "_log_marginal_likelihood64", lambda self: torch.tensor(-1.5), raising=False)
    monkeypatch.setattr(cls, "log_marginal_likelihood", lambda self, *a, **k: torch.tensor(-1.5))
    monkeypatch.setattr(cls, "_logdet_factor_gradients", lambda self: (list(GB), list(GA)), raising=False)
    monkeypatch.setattr(cls, "posterior_precision", property(lambda self: torch.full((9,), 2.0)))
    monkeypatch.setattr(cls, "_adj_gamma", lambda self: BIG_GAMMA, raising=False)
    return la


@pytest.fixture
def job(monkeypatch):
    """Patch the process-group queries: ``job(rank, world)`` sets the simulated rank and returns the list that records what
    ``all_reduce_flat_`` is handed."""
    state = {"rw": (0, 1), "reduced": []}
    monkeypatch.setattr(lp, "_dist_info", lambda process_group: state["rw"])
    monkeypatch.setattr(lp, "all_reduce_flat_", lambda tensors, process_group=None: state["reduced"].append(list(tensors)))

    def set_rank(rank, world):
        state["rw"] = (rank, world)
        return state["reduced"]
    return set_rank


def _loader():
    return lg.TensorBatchLoader(IDX, Y, batch_size=5)


def _same(tensors, want):
    return len(tensors) == len(want) and all(a is b for a, b in zip(tensors, want))


@pytest.mark.parametrize("rank,world", RANKS)
@pytest.mark.parametrize("dense", [False, True])
def test_kronecker_deals_whole_batches_round_robin(monkeypatch, job, rank, world, dense):
    reduced = job(rank, world)
    eng = StubEngine()
    out = _front(monkeypatch, "kron", eng).neg_marglik_adj_grad(_loader(), dense=dense)
    batches = [(IDX[:5], Y[:5]), (IDX[5:], Y[5:])]
    mine = [b for t, b in enumerate(batches) if t % world == rank]
    assert len(eng.batches) == len(mine)
    for call, (X, y) in zip(eng.batches, mine):  # the rank's batches, whole
        assert call.name == ("adjgrad_batch_dense" if dense else "adjgrad_batch")
        assert torch.equal(call.X, X) and torch.equal(call.y, y)
        assert all(torch.equal(g, 0.5 * g0) for g, g0 in zip(call.weight, GB))  # 1/2 d logdet / dB_l
        assert call.kw["fork_exact"] is True and call.kw["loss_scale"] == 1.0
    target, out_bar = eng.finishes[0].target, eng.finishes[0].buffers[0]
    assert target.shape == ((N, N) if dense else (STORED.shape[1],)) and out_bar.shape == (N, C)
    assert all(_same(c.buffers, [target, out_bar]) for c in eng.batches)
    assert all(torch.equal(g, 0.5 * g0) for g, g0 in zip(eng.finishes[0].buffers[1], GA))
    assert eng.finishes[0].buffers[2] == 2 / 7 and len(eng.finishes) == 1  # a_scale = batches / samples
    assert eng.likelihoods == []
    if world == 1:
        assert reduced == []
    else:
        assert len(reduced) == 1 and _same(reduced[0], [target, out_bar])  # [grad_P, out_bar] / [G, out_bar]
    assert float(out[0]) == 1.5 and len(out) == (2 if dense else 3)
    if not dense:
        assert torch.equal(out[1], STORED)


@pytest.mark.parametrize("rank,world", RANKS + [(0, 3), (1, 3), (2, 3)])
@pytest.mark.parametrize("structure,dense", [("diag", False), ("diag", True), ("full", False)])
def test_diagonal_and_full_slice_every_batch_by_samples(monkeypatch, job, rank, world, structure, dense):
    reduced = job(rank, world)
    eng = StubEngine()
    out = _front(monkeypatch, structure, eng).neg_marglik_adj_grad(_loader(), dense=dense)
    want = []
    for X, y in [(IDX[:5], Y[:5]), (IDX[5:], Y[5:])]:
        M = X.shape[0]
        lo, hi = M * rank // world, M * (rank + 1) // world
        if hi > lo:  # an empty slice (rank 0 of 3 in the batch of 2) is no engine call
            want.append((X[lo:hi], y[lo:hi]))
    assert len(eng.batches) == len(want) and all(c.X.numel() > 0 for c in eng.batches)
    name = {"diag": "diag_adjgrad_batch", "full": "full_adjgrad_batch"}[structure] + ("_dense" if dense else "")
    for call, (X, y) in zip(eng.batches, want):
        assert call.name == name and torch.equal(call.X, X) and torch.equal(call.y, y)
        if structure == "full":
            assert call.weight is BIG_GAMMA
        else:  # 1/2 f / posterior_precision, f = 1
            assert torch.equal(call.weight, torch.full((9,), 0.25)) and call.weight.dtype == torch.float32
        assert call.kw["loss_scale"] == 1.0
    fin = eng.finishes[0]
    assert fin.name == "diag_adjgrad_finish" + ("_dense" if dense else "") and len(eng.finishes) == 1
    out_bar, h1_bar, e_bar = fin.buffers
    assert out_bar.shape == (N, C) and h1_bar.shape == (N, H) and e_bar.shape == (N, F + 1)
    assert all(_same(c.buffers, [fin.target, out_bar, h1_bar, e_bar]) for c in eng.batches)
    assert eng.likelihoods == ["classification"]
    if world == 1:
        assert reduced == []
    else:
        assert len(reduced) == 1 and _same(reduced[0], [fin.target, out_bar, h1_bar, e_bar])
    assert float(out[0]) == 1.5 and len(out) == (2 if dense else 3)


@pytest.mark.parametrize("structure", ["diag", "full"])
def test_slices_of_two_ranks_tile_every_batch(monkeypatch, job, structure):
    seen = []
    for rank in (0, 1):
        job(rank, 2)
        eng = StubEngine()
        _front(monkeypatch, structure, eng).neg_marglik_adj_grad(_loader())
        assert len(eng.batches) == 2  # every rank sees every batch
        seen.append([c.X for c in eng.batches])
    for t, X in enumerate([IDX[:5], IDX[5:]]):
        assert torch.equal(torch.cat([seen[0][t], seen[1][t]]), X)


@pytest.mark.parametrize("structure", ["kron", "diag", "full"])
def test_one_layer_model_has_no_h1_bar_in_the_reduce_list(monkeypatch, job, structure):
    reduced = job(1, 2)
    eng = StubEngine(dims=(F, C))
    _front(monkeypatch, structure, eng).neg_marglik_adj_grad(_loader(), candidates=CAND)
    fin = eng.finishes[0]
    if structure == "kron":
        assert _same(reduced[0], [fin.target, fin.buffers[0], fin.cand[2]])
    else:
        out_bar, h1_bar, e_bar = fin.buffers
        assert h1_bar is None and _same(reduced[0], [fin.target, out_bar, e_bar, fin.cand[2]])


@pytest.mark.parametrize("structure", ["kron", "diag", "full"])
@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_symmetric_candidates_go_in_both_orientations_and_come_back_averaged(monkeypatch, job, structure, kind):
    reduced = job(0, 2)
    eng = StubEngine(kind=kind)
    out = _front(monkeypatch, structure, eng, symmetric=True).neg_marglik_adj_grad(_loader(), candidates=CAND)
    K = CAND.shape[1]
    ci, cj = torch.cat([CAND[0], CAND[1]]), torch.cat([CAND[1], CAND[0]])  # 2K pairs (i, j): both orientations
    ca, cb = (cj, ci) if kind == "gcn" else (ci, cj)  # entry (i, j) of the adjacency = entry (j, i) of a GCN's D A^T D
    cand = eng.finishes[0].cand
    assert cand[0].dtype == torch.int32 and torch.equal(cand[0], ca.to(torch.int32)) and torch.equal(cand[1], cb.to(torch.int32))
    assert cand[2].shape == (2 * K,) and cand[2].dtype == torch.float32
    assert all(c.kw["cand"] is cand for c in eng.batches)
    fin = eng.finishes[0]
    buffers = [fin.buffers[0]] if structure == "kron" else list(fin.buffers)
    assert _same(reduced[0], [fin.target] + buffers + [cand[2]])  # the candidates' accumulator goes last
    gc = torch.arange(2 * K, dtype=torch.float32) ** 2  # what the stub's finish returned
    assert len(out) == 4 and torch.equal(out[3], 0.5 * (gc[:K] + gc[K:]))
    assert torch.equal(out[1], STORED) and torch.equal(out[2], torch.arange(STORED.shape[1], dtype=torch.float32) + 100.0)


def test_asymmetric_candidates_come_back_as_the_finish_returned_them(monkeypatch, job):
    job(0, 1)
    eng = StubEngine()
    out = _front(monkeypatch, "diag", eng).neg_marglik_adj_grad(_loader(), candidates=CAND)
    assert eng.finishes[0].cand[0].numel() == 3 and torch.equal(out[3], torch.arange(3, dtype=torch.float32) ** 2)


@pytest.mark.parametrize("structure", ["kron", "diag"])
def test_dense_with_candidates_is_refused(monkeypatch, job, structure):
    job(0, 1)
    eng = StubEngine()
    with pytest.raises(ValueError, match="^dense=True covers every pair: no candidates$"):
        _front(monkeypatch, structure, eng).neg_marglik_adj_grad(_loader(), candidates=CAND, dense=True)
    assert eng.batches == [] and eng.finishes == []


def test_dense_under_the_full_posterior_is_refused(monkeypatch, job):
    job(0, 1)
    eng = StubEngine()
    with pytest.raises(NotImplementedError) as err:
        _front(monkeypatch, "full", eng).neg_marglik_adj_grad(_loader(), dense=True)
    assert str(err.value) == ("adjacency gradient under the full posterior: stored entries and candidates only "
                              "(dense=True is offered by KronLaplace and DiagLaplace)")
    assert eng.batches == [] and eng.finishes == []
