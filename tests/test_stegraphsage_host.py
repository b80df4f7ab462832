"""Host side of ``lg.STEGraphSAGE`` (no GPU): the tracked pairs with diagonal candidates, the hard gradient mask, the effective
values, the reduction of a dense reference checkpoint, the refusals, and the conditions the loop fixtures
(tests/golden/sageloop/steloop_sage_*.npz, tools/make_sage_loop_golden.py) were kept under."""
import os

import numpy as np
import pytest
import torch

import laplace_gnn_amd as lg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sageloop")
FIXTURES = ["steloop_sage_kron_sym", "steloop_sage_diag_sym", "steloop_sage_kron_dir_masked"]


def _model(symmetric, **kw):
    X = torch.randn(6, 3, generator=torch.Generator().manual_seed(0))
    ei = torch.tensor([[0, 1, 2, 2, 1], [1, 2, 3, 2, 2]])  # (2, 2) is dropped once (gnn/models/models.py:135); (1, 2) twice
    cand = torch.tensor([[0, 4, 5, 3], [0, 4, 1, 3]])
    return lg.STEGraphSAGE(3, 4, 2, 2, X, ei, None, symmetric=symmetric, candidates=cand, **kw)


def test_is_exported():
    assert "STEGraphSAGE" in lg.__all__ and lg.STEGraphSAGE.kind == "sage"
    assert issubclass(lg.STEGraphSAGE, lg.GraphSAGE) and not issubclass(lg.STEGraphSAGE, lg.STEGCN)


def test_tracked_pairs_directed():
    m = _model(False)
    assert m.adj_index.tolist() == [[0, 0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 3, 4, 1]]  # row-major sorted, diagonal candidates kept
    assert m.adj.tolist() == [0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0]
    assert m.edge_index.tolist() == [[0, 1, 2, 1], [1, 2, 3, 2]]  # the initial graph has no self loop
    dense = m.dense_adj()
    assert float(dense.sum()) == 3.0 and float(dense.diagonal().sum()) == 0.0  # the diagonal as tracked, not filled


def test_tracked_pairs_symmetric_hold_both_orientations():
    m = _model(True)
    assert m.adj_index.tolist() == [[0, 0, 1, 1, 1, 2, 2, 3, 3, 4, 5], [0, 1, 0, 2, 5, 1, 3, 2, 3, 4, 1]]
    assert m.adj.tolist() == [0.0, 1.0, 1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0]
    keys = (m.adj_index[0] * 6 + m.adj_index[1]).tolist()
    assert keys == sorted(keys) and all((j * 6 + i) in keys for i, j in zip(*m.adj_index.tolist()))


def test_stegcn_keeps_dropping_the_diagonal():
    X = torch.randn(6, 3)
    m = lg.STEGCN(3, 4, 2, 2, X, torch.tensor([[0, 1, 2], [1, 2, 2]]), candidates=torch.tensor([[0, 4], [0, 1]]))
    assert m.adj_index.tolist() == [[0, 1, 4], [1, 2, 1]]


def test_hard_mask():
    """``train_adj_mask`` (gnn/models/utils.py:19-22, models.py:152-154): 0 between two training nodes, (t, t) included, 1
    elsewhere -- not STEGCN's 0.1."""
    m = _model(False, train_masked_update=True, train_nodes=torch.tensor([0, 1, 3, 3]))
    is_train = torch.zeros(6, dtype=torch.bool)
    is_train[[0, 1, 3]] = True
    want = (~(is_train[m.adj_index[0]] & is_train[m.adj_index[1]])).float()
    assert torch.equal(m.grad_adj_mask, want)
    assert m.grad_adj_mask.tolist() == [0.0, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0]  # (0, 0), (0, 1) and (3, 3) are train-train
    g = lg.STEGCN(3, 4, 2, 2, torch.randn(6, 3), torch.tensor([[0, 1, 4], [1, 2, 5]]), train_masked_update=True,
                  train_nodes=torch.tensor([0, 1]))
    assert g.grad_adj_mask.tolist() == pytest.approx([0.1, 1.0, 1.0])
    with pytest.raises(ValueError, match="train_nodes"):
        _model(False, train_masked_update=True)


def test_effective_values():
    m = _model(False)
    with torch.no_grad():
        m.adj.copy_(torch.arange(7.0))
    assert torch.equal(m._effective(), torch.arange(7.0))
    s = _model(True)
    with torch.no_grad():
        s.adj.copy_(torch.arange(11.0))
    dense = s.dense_adj()
    eff = 0.5 * (dense + dense.T)
    assert torch.equal(s._effective(), eff[s.adj_index[0], s.adj_index[1]])
    assert float(s._effective()[0]) == 0.0 and float(s._effective()[8]) == 8.0  # (i, i) is its own mirror


@pytest.mark.parametrize("symmetric", [False, True])
def test_dense_reference_checkpoint_is_reduced_to_the_tracked_pairs(symmetric):
    m = _model(symmetric)
    gen = torch.Generator().manual_seed(3)
    dense = torch.rand(6, 6, generator=gen)
    dense[0, 0], dense[4, 4], dense[3, 3] = 0.9, 0.2, 0.7
    state = {k: v.clone() for k, v in m.state_dict().items()}
    state["adj"] = dense
    m.load_state_dict(state)
    assert torch.equal(m.adj.detach(), dense[m.adj_index[0], m.adj_index[1]])
    eff = 0.5 * (dense + dense.T) if symmetric else dense
    on = eff > 0.5
    assert bool(on[0, 0]) and bool(on[3, 3]) and not bool(on[4, 4])
    assert torch.equal(m.edge_index, on.nonzero().t())  # the binarised graph WITH its diagonal
    assert m._engine is None
    # the module's own checkpoint holds the tracked values as they are
    own = m.state_dict()
    assert own["adj"].dim() == 1
    m2 = _model(symmetric)
    m2.load_state_dict(own)
    assert torch.equal(m2.adj.detach(), m.adj.detach())
    bad = dict(state, adj=torch.zeros(5, 5))
    with pytest.raises(RuntimeError, match="expected"):
        m.load_state_dict(bad)


def test_refusals_name_what_they_refuse():
    X, ei = torch.randn(6, 3), torch.tensor([[0, 1, 4], [1, 2, 5]])
    with pytest.raises(NotImplementedError, match="sign_grad"):
        lg.STEGraphSAGE(3, 4, 2, 2, X, ei, None, sign_grad=True)
    with pytest.raises(NotImplementedError, match="res=True"):
        lg.STEGraphSAGE(3, 4, 2, 2, X, ei, None, res=True)
    for norm in ("layer", "batch"):
        with pytest.raises(NotImplementedError, match=f"norm='{norm}'"):
            lg.STEGraphSAGE(3, 4, 2, 2, X, ei, None, norm=norm)
    for layers in (1, 3):
        with pytest.raises(NotImplementedError, match=f"num_layers={layers}"):
            lg.STEGraphSAGE(3, 4, 2, layers, X, ei, None)
    lg.STEGraphSAGE(3, 4, 2, 2, X, ei, None, res=False, norm=None)  # the plain model's spelled-out defaults pass


def test_num_sampled_nodes_per_hop_is_accepted_and_ignored():
    """The reference's sampling line is commented out (gnn/models/models.py:174-177): no sampler, no ``sample_seed`` needed."""
    X, ei = torch.randn(6, 3), torch.tensor([[0, 1, 1, 1], [1, 2, 3, 4]])
    a = lg.STEGraphSAGE(3, 4, 2, 2, X, ei, 1)
    b = lg.STEGraphSAGE(3, 4, 2, 2, X, ei)
    assert a.num_sampled_nodes_per_hop is None and torch.equal(a.edge_index, b.edge_index)  # GraphSAGE's sampler stays off
    assert torch.equal(a.adj_index, b.adj_index)
    with pytest.raises(RuntimeError, match="GPU"):
        a.engine  # (the full graph's engine, not sampled_edge_index's: that one would build a second engine first)


def test_engine_takes_the_flag_after_the_existing_arguments():
    """``GraphEngine(edge_index, num_nodes, kind, symmetric, self_loops=False)``; the flag crosses the C ABI as a bit of
    ``kind`` (the GCN refusal needs a device: tests/test_gpu_stegraphsage.py)."""
    import inspect
    sig = inspect.signature(lg.GraphEngine.__init__)
    assert sig.parameters["self_loops"].default is False and list(sig.parameters)[1:5] == ["edge_index", "num_nodes", "kind", "symmetric"]
    assert lg._lib.KIND_SELF_LOOPS == 0x100 and not (lg._lib.KIND_SELF_LOOPS & (lg._lib.KIND_GCN | lg._lib.KIND_SAGE))


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_conditions(name):
    """What tools/make_sage_loop_golden.py asserts when it keeps a seed, on the committed files."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert str(g["kind"]) == "sage" and int(g["seed"]) >= {"steloop_sage_kron_dir_masked": 51}.get(name, 62)
    N, thr, sym = int(g["num_nodes"]), float(g["threshold"]), bool(g["symmetric"])
    assert (N, g["X"].shape[1], g["W0"].shape[0], g["W1"].shape[0]) == (64, 12, 8, 3)
    assert g["edge_index"].shape == (2, 150) and g["train_idx"].shape == (33,) and int(g["batch_size"]) == 12
    assert len(np.unique(g["train_idx"])) == 32 and g["adj_steps"].shape == (3, N, N) and float(g["prior"]) == 1.0
    assert float(np.abs(np.diag(g["adj_init"])).max()) == 0.0
    eye = np.eye(N, dtype=bool)
    eff = [0.5 * (a + a.T) if sym else a for a in [g["adj_init"]] + list(g["adj_steps"])]
    # every effective value at least 4e-4 from the threshold after every step: a comparison to 1e-4 decides every edge alike
    assert min(float(np.abs(e - thr).min()) for e in eff[1:]) >= 4e-4
    diag_on = [int((np.diag(e) > thr).sum()) for e in eff[1:]]
    if sym:  # a later gradient and refit run on a graph with a self loop
        assert diag_on[0] > 0 or diag_on[1] > 0
    flips = sum(int((((a > thr) != (b > thr)) & ~eye).sum()) for a, b in zip(eff[:-1], eff[1:]))
    assert flips >= 50
    if bool(g["masked"]):
        t = np.unique(g["train_idx"])
        for a in g["adj_steps"]:
            assert np.array_equal(a[np.ix_(t, t)], g["adj_init"][np.ix_(t, t)])  # no train-train value moves
    expect = {"steloop_sage_kron_sym": ("kron", True, True, 8.0, 0.9, 5e-4, False),
              "steloop_sage_diag_sym": ("diag", True, True, 8.0, 0.9, 5e-4, False),
              "steloop_sage_kron_dir_masked": ("kron", False, False, 0.05, 0.5, 0.0, True)}[name]
    got = (str(g["structure"]), sym, bool(g["grad_norm"]), float(g["lr_adj"]), float(g["momentum"]), float(g["weight_decay"]),
           bool(g["masked"]))
    assert got == expect
