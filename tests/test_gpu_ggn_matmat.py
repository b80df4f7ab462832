"""GGN-times-block products on the GPU (csrc/ggnmat.hip behind ``lgnn_ggn_matmat`` / ``lgnn_jvp_block``) against the dense fp64
GGN ``H64 = sum_n J_n^T Lambda_n J_n`` built from ``engine.jacobians`` (tests/lowrank_utils.py).

Graphs and models are those of tests/test_gpu_gp.py; the train set is 60 ids in two batches (37 + 23) with the hub, both
isolated nodes and a repeated id.  Bound: 1e-5 of max|G|, the project's bound for fp32 against fp64.  1- and 2-layer models
without res / norm take the structured route (no Jacobians), the 3-layer GCN and the res + LayerNorm model the route over chunks
of ``lgnn_jacobians`` rows, which ``from_jacobians=True`` forces on any model."""
import pytest
import torch

from lowrank_utils import (BOUND, H64, ODD_SHAPE, SHAPES, WS_DEFAULT, case_id, directions, edge_model, ggn64, train_batches,
                           train_set)

pytestmark = pytest.mark.gpu

STRUCTURED = [(k, L, a, s, False) for k in ("gcn", "sage") for L in (1, 2) for a in ("relu", "tanh") for s in SHAPES]
GENERAL = [("gcn", 3, "relu", s, False) for s in SHAPES] + [("sage", 2, "relu", s, True) for s in SHAPES]
ODD = [("gcn", 2, "relu", ODD_SHAPE, False), ("sage", 2, "tanh", ODD_SHAPE, False)]  # F = 12; k H = 10, 50, 330: no multiple of 64
# more than 64 (and, GraphSAGE, more than 128) columns of q: a second class window in the forward product and several class
# chunks in the transpose's prologue; H = F = 70: two ragged tiles of the hidden width, of K and of the output columns
WIDE = [("sage", 2, "relu", (96, 13, 10, 70), False), ("gcn", 2, "tanh", (96, 70, 70, 5), False),
        ("gcn", 1, "relu", (96, 70, 10, 70), False)]
KS = (1, 5, 33)


def product(case, V, **kw):
    """V @ H over the two train batches through ``engine.ggn_matmat_``: (G, loss)."""
    eng = edge_model(*case).engine
    G = torch.zeros_like(V)
    loss = torch.zeros(1, device="cuda")
    for idx, y in train_batches(case[3][0], case[3][3]):
        eng.ggn_matmat_(G, loss, idx, y, V, **kw)
    return G, loss


def rel_err(got, want):
    scale = float(want.abs().max())
    assert scale > 0 and got.shape == want.shape
    return float((got.double() - want.double()).abs().max()) / scale


@pytest.mark.parametrize("case", STRUCTURED + GENERAL + ODD + WIDE, ids=case_id)
def test_block_product_against_the_dense_fp64_ggn(case):
    H = H64(case)
    errs = {}
    for k in KS:
        V = directions(k, H.shape[0])
        errs[k] = rel_err(product(case, V)[0], V.double() @ H)
    print(f"{case_id(case)}: " + " ".join(f"k={k} {e:.2e}" for k, e in errs.items()))
    edge_model(*case).engine.check_async_errors()
    assert max(errs.values()) <= BOUND, errs


@pytest.mark.parametrize("case", STRUCTURED + ODD[:1] + WIDE, ids=case_id)
def test_structured_route_agrees_with_the_route_over_jacobians(case):
    H = H64(case)
    V = directions(5, H.shape[0])
    got, base = product(case, V)[0], product(case, V, from_jacobians=True)[0]
    e_routes, e64 = rel_err(got, base), rel_err(base, V.double() @ H)
    print(f"{case_id(case)}: routes {e_routes:.2e}; from_jacobians vs fp64 {e64:.2e}")
    assert e_routes <= BOUND and e64 <= BOUND


@pytest.mark.parametrize("case", STRUCTURED[::3] + GENERAL[:1] + GENERAL[2:3] + ODD[:1] + WIDE, ids=case_id)
def test_jvp_block_against_fp64_and_gp_jvp(case):
    eng = edge_model(*case).engine
    idx = train_set(case[3][0], case[3][3])[0][:37].contiguous()
    J = eng.jacobians(idx)[0].double()
    worst = 0.0
    for k in KS:
        V = directions(k, eng.n_params)
        got = eng.jvp_block(idx, V)
        assert got.shape == (37, case[3][3], k)
        worst = max(worst, rel_err(got, torch.einsum("bcp,kp->bck", J, V.double())))
        e0 = rel_err(got[:, :, 0], eng.gp_jvp(idx, V[0].contiguous()))
        worst = max(worst, e0)
    print(f"{case_id(case)}: jvp_block vs fp64 / gp_jvp {worst:.2e}")
    assert worst <= BOUND


DET_CASES = [("gcn", 2, "relu", SHAPES[1], False), ("sage", 2, "tanh", SHAPES[0], False), ("gcn", 1, "relu", SHAPES[0], False),
             ("gcn", 3, "relu", SHAPES[0], False), ("sage", 2, "relu", SHAPES[0], True)]


@pytest.mark.parametrize("case", DET_CASES, ids=case_id)
def test_two_calls_return_the_same_bits_and_G_accumulates(case):
    eng = edge_model(*case).engine
    V = directions(33, eng.n_params)
    for kw in ({}, {"from_jacobians": True}):
        G1, G2 = product(case, V, **kw)[0], product(case, V, **kw)[0]
        assert torch.equal(G1, G2), kw
    idx, y = train_batches(case[3][0], case[3][3])[0]
    G = torch.zeros_like(V)
    loss = torch.zeros(1, device="cuda")
    eng.ggn_matmat_(G, loss, idx, y, V)
    once, loss_once = G.clone(), float(loss)
    eng.ggn_matmat_(G, loss, idx, y, V)
    assert torch.equal(G, once + once)  # x + x is exact in fp32
    assert abs(float(loss) - 2 * loss_once) <= 1e-6 * abs(loss_once)
    assert torch.equal(eng.jvp_block(idx, V), eng.jvp_block(idx, V))
    eng.check_async_errors()


@pytest.mark.parametrize("case", [("gcn", 2, "relu", SHAPES[1], False), ("sage", 2, "relu", SHAPES[1], False),
                                  ("gcn", 3, "relu", SHAPES[0], False)], ids=case_id)
def test_a_small_workspace_limit_gives_the_same_product(case):
    eng = edge_model(*case).engine
    V = directions(33, eng.n_params)  # the structured route chunks the directions, the general one the samples
    idx = train_set(case[3][0], case[3][3])[0][:37].contiguous()
    one, j_one = product(case, V)[0], eng.jvp_block(idx, V)
    try:
        eng.set_workspace_limit(1 << 20)
        many, j_many = product(case, V)[0], eng.jvp_block(idx, V)
    finally:
        eng.set_workspace_limit(WS_DEFAULT)
    e, ej = rel_err(many, one), rel_err(j_many, j_one)
    e64 = rel_err(many, V.double() @ H64(case))
    print(f"{case_id(case)}: chunked vs one chunk {e:.2e}, jvp_block {ej:.2e}; chunked vs fp64 {e64:.2e}")
    assert e <= BOUND and ej <= BOUND and e64 <= BOUND


def test_regression_likelihood():
    import laplace_gnn_amd as lg

    case = ("gcn", 2, "tanh", SHAPES[0], False)
    m = edge_model(*case)
    N, C = case[3][0], case[3][3]
    idx = train_set(N, C)[0]
    y = torch.randn(60, C, generator=torch.Generator().manual_seed(12)).cuda()
    V = directions(5, m.engine.n_params)
    try:
        be = lg.HipGGN(m, "regression")
        G, loss = be.ggn_matmat([(idx[:37].contiguous(), y[:37].contiguous()), (idx[37:].contiguous(), y[37:].contiguous())], V)
        want = V.double() @ ggn64(m.engine, idx, regression=True)
        f = m.engine.forward(idx).double()
        want_loss = 0.5 * float(((f - y.double()) ** 2).sum())
    finally:
        m.engine.set_likelihood("classification")
    e = rel_err(G, want)
    print(f"regression: {e:.2e}, loss {float(loss):.6f} vs {want_loss:.6f}")
    assert e <= BOUND and abs(float(loss) - want_loss) <= 1e-5 * abs(want_loss)


@pytest.mark.parametrize("case", [("gcn", 2, "relu", SHAPES[0], False), ("sage", 1, "relu", SHAPES[0], False),
                                  ("gcn", 3, "relu", SHAPES[0], False)], ids=case_id)
def test_an_out_of_range_id_contributes_nothing_and_sets_the_sticky_flag(case):
    import laplace_gnn_amd as lg

    eng = edge_model(*case).engine
    N, C = case[3][0], case[3][3]
    idx, y = train_batches(N, C)[0]
    V = directions(5, eng.n_params)
    keep = torch.ones(37, dtype=torch.bool, device="cuda")
    keep[4] = False
    want = torch.zeros_like(V)
    eng.ggn_matmat_(want, torch.zeros(1, device="cuda"), idx[keep].contiguous(), y[keep].contiguous(), V)
    eng.check_async_errors()
    for bad_id in (N, -1):
        bad = idx.clone()
        bad[4] = bad_id
        G = torch.zeros_like(V)
        eng.ggn_matmat_(G, torch.zeros(1, device="cuda"), bad, y, V)
        with pytest.raises(lg._lib.HipLibraryError, match="node index"):
            eng.check_async_errors()
        eng.check_async_errors()  # cleared
        assert rel_err(G, want) <= BOUND
        out = eng.jvp_block(bad, V)
        assert float(out[4].abs().max()) == 0.0 and torch.equal(out[keep], eng.jvp_block(idx, V)[keep])
        with pytest.raises(lg._lib.HipLibraryError, match="node index"):
            eng.check_async_errors()
        eng.check_async_errors()


@pytest.mark.parametrize("case", [("gcn", 2, "relu", SHAPES[1], False), ("sage", 2, "relu", SHAPES[0], True)], ids=case_id)
def test_loss_equals_the_full_accumulate_loss(case):
    eng = edge_model(*case).engine
    P = eng.n_params
    loss_full = torch.zeros(1, device="cuda")
    H = torch.zeros(P, P, device="cuda")
    for idx, y in train_batches(case[3][0], case[3][3]):
        eng.full_accumulate(idx, y, H, loss_full)
    V = directions(5, P)
    G, loss = product(case, V)
    print(f"{case_id(case)}: loss {float(loss):.6f} vs full_accumulate {float(loss_full):.6f}; V H vs full_accumulate's H "
          f"{rel_err(G, V @ H):.2e}")
    assert abs(float(loss) - float(loss_full)) <= 1e-6 * abs(float(loss_full))
