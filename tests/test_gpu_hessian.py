"""The exact loss Hessian on the GPU (csrc/hessmat.hip behind ``lgnn_hessian_resid_matmat``, ``lg.HipHessian``) against the fp64
double-backward reference of tests/hessian_reference.py (pinned to the goldens by tests/test_hessian_reference.py).

Graphs, models, train set (60 ids in two batches with the hub, both isolated nodes and a repeated id) and directions are those of
tests/lowrank_utils.py; the reference is built from the same seeds on the CPU and checked to hold the same numbers.  Shapes: the
structured cases of tests/test_gpu_ggn_matmat.py, F = 12, more than 128 columns of G (GraphSAGE, C = 70) and ragged tiles of H, K
and the output (H = F = 70).  Bound: 1e-5 of the largest entry, the project's bound for fp32 against fp64.  Before a comparison
the fp64 side asserts that it is no vacuous one: ``max|V R| >= 1e-2 max|V GGN|``, and for ReLU ``min|s| >= 1e-5`` over all nodes
(the fp32 and fp64 masks agree).  Every case prints what it measured."""
import functools

import pytest
import torch

from hessian_reference import F64, HessianReference, propagation
from lowrank_utils import BOUND, ODD_SHAPE, SHAPES, WS_DEFAULT, directions, edge_model, train_batches, train_set
from test_gpu_gp import edge_graph

pytestmark = pytest.mark.gpu

# A sixth entry is the model's seed (tests/test_gpu_gp.edge_model).  With seed 0 the two ReLU models at (300, 37, 64, 7) have a
# pre-activation within 1e-5 of the kink (min|s| = 7.2e-6 and 8.1e-6 in fp64); seeds 3 and 2 are the first that have none.
SEEDS = {("gcn", 2, "relu", SHAPES[1]): 3, ("sage", 2, "relu", SHAPES[1]): 2}
GCN_RELU_BIG = ("gcn", 2, "relu", SHAPES[1], False, 3)
SAGE_RELU_BIG = ("sage", 2, "relu", SHAPES[1], False, 2)
STRUCTURED = [(k, L, a, s, False) + ((SEEDS[(k, L, a, s)],) if (k, L, a, s) in SEEDS else ())
              for k in ("gcn", "sage") for L in (1, 2) for a in ("relu", "tanh") for s in SHAPES]
ODD = [("gcn", 2, "relu", ODD_SHAPE, False), ("sage", 2, "tanh", ODD_SHAPE, False)]
WIDE = [("sage", 2, "relu", (96, 13, 10, 70), False), ("gcn", 2, "tanh", (96, 70, 70, 5), False)]
TWO = [c for c in STRUCTURED + ODD + WIDE if c[1] == 2]
ONE = [c for c in STRUCTURED if c[1] == 1]
KS = (1, 5, 33)
MARGLIK_RTOL = 3e-4  # tests/test_gpu_frontend.py, the full posterior
SMALL = [("gcn", 2, "relu", SHAPES[0], False), ("sage", 2, "tanh", SHAPES[0], False)]


def case_id(c):
    k, L, a, s = c[:4]
    return f"{k}{L}-{a}-N{s[0]}F{s[1]}H{s[2]}C{s[3]}" + ("-resln" if c[4] else "") + (f"-s{c[5]}" if len(c) > 5 else "")


def cpu_train_set(N, C):
    """tests/lowrank_utils.train_set without a device."""
    a = torch.randperm(N - 2, generator=torch.Generator().manual_seed(2))[:37].clone()
    a[0], a[1], a[2] = 3, N - 1, N - 2
    a[7] = a[9]
    b = torch.randperm(N, generator=torch.Generator().manual_seed(3))[:50].clone()
    return torch.cat([a, b[:23]]), torch.randint(0, C, (60,), generator=torch.Generator().manual_seed(11))


@functools.lru_cache(maxsize=None)
def reference(case, likelihood="classification"):
    """(HessianReference, theta) of the case's model from tests/test_gpu_gp.edge_model's seeds, on the CPU."""
    import laplace_gnn_amd as lg

    kind, L, act, (N, F, H, C), _ = case[:5]
    seed = case[5] if len(case) > 5 else 0
    X = torch.randn(N, F, generator=torch.Generator().manual_seed(seed + 1))
    ei = edge_graph(N, seed)
    torch.manual_seed(seed)
    m = (lg.GCN if kind == "gcn" else lg.GraphSAGE)(F, H, C, L, X, ei, act=act).eval()
    ref = HessianReference(kind, propagation(kind, ei, N), X, [F, H, C] if L == 2 else [F, C], act, likelihood)
    theta = ref.flatten([c.lin.weight for c in m.convs], [c.lin.bias for c in m.convs])
    return ref, theta


@functools.lru_cache(maxsize=None)
def expected(case, k):
    """fp64 (V @ R, V @ H) over the 60-id train set, preconditions asserted."""
    ref, theta = reference(case)
    idx, y = cpu_train_set(case[3][0], case[3][3])
    V = directions(k, ref.n_params).cpu().to(F64)
    VR, VH = ref.resid_vp(theta, idx, y, V), ref.hvp(theta, idx, y, V)
    if case[1] == 2:
        assert float(VR.abs().max()) >= 1e-2 * float((VH - VR).abs().max()), "the residual term is negligible here"
        if case[2] == "relu":
            assert ref.min_abs_preactivation(theta) >= 1e-5, "a pre-activation too close to the kink"
    return VR, VH


def check_same_inputs(case):
    """The CPU reference holds the engine's numbers: parameters, train set, propagation matrix."""
    ref, theta = reference(case)
    m = edge_model(*case)
    got = ref.flatten([c.lin.weight for c in m.convs], [c.lin.bias for c in m.convs])
    assert torch.equal(got, theta)
    N, C = case[3][0], case[3][3]
    idx, y = train_set(N, C)
    ci, cy = cpu_train_set(N, C)
    assert torch.equal(idx.cpu(), ci) and torch.equal(y.cpu(), cy)
    r, c, v = (t.cpu() for t in m.engine.export_propagation())
    P = torch.zeros(N, N, dtype=F64).index_put_((r.long(), c.long()), v.to(F64), accumulate=True)
    assert float((P - ref.P).abs().max()) <= 1e-6


def rel_err(got, want):
    scale = float(want.abs().max())
    assert scale > 0 and got.shape == want.shape
    return float((got.double().cpu() - want.double().cpu()).abs().max()) / scale


def resid_product(case, V, batches=None):
    """V @ R over the train batches: per batch ``ggn_matmat_`` (into a scratch block) and then the residual product."""
    eng = edge_model(*case).engine
    G, scratch, loss = torch.zeros_like(V), torch.zeros_like(V), torch.zeros(1, device="cuda")
    for idx, y in batches or train_batches(case[3][0], case[3][3]):
        eng.ggn_matmat_(scratch, loss, idx, y, V)
        eng.hessian_resid_matmat_(G, idx, y, V)
    return G


def hessian_product(case, V, likelihood="classification", batches=None):
    import laplace_gnn_amd as lg

    m = edge_model(*case)
    try:
        return lg.HipHessian(m, likelihood).hessian_matmat(batches or train_batches(case[3][0], case[3][3]), V)
    finally:
        m.engine.set_likelihood("classification")


@pytest.mark.parametrize("case", TWO, ids=case_id)
def test_residual_and_hessian_products_against_fp64_double_backward(case):
    check_same_inputs(case)
    errs = {}
    for k in KS:
        VR, VH = expected(case, k)
        V = directions(k, VR.shape[1])
        errs[k] = (rel_err(resid_product(case, V), VR), rel_err(hessian_product(case, V)[0], VH))
    print(f"{case_id(case)}: " + " ".join(f"k={k} R {a:.2e} H {b:.2e}" for k, (a, b) in errs.items()))
    edge_model(*case).engine.check_async_errors()
    assert max(max(e) for e in errs.values()) <= BOUND, errs


@pytest.mark.parametrize("case", ONE, ids=case_id)
def test_one_layer_models_leave_G_untouched(case):
    check_same_inputs(case)
    eng = edge_model(*case).engine
    VR, VH = expected(case, 5)
    assert float(VR.abs().max()) == 0.0
    V = directions(5, eng.n_params)
    G = torch.randn(5, eng.n_params, generator=torch.Generator().manual_seed(6)).cuda()
    before = G.clone()
    for idx, y in train_batches(case[3][0], case[3][3]):
        eng.hessian_resid_matmat_(G, idx, y, V)
    assert torch.equal(G, before)
    e = rel_err(hessian_product(case, V)[0], VH)
    print(f"{case_id(case)}: H = GGN {e:.2e}")
    eng.check_async_errors()
    assert e <= BOUND


@pytest.mark.parametrize("case", [("gcn", 2, "tanh", SHAPES[0], False), ("sage", 2, "relu", SHAPES[0], False)], ids=case_id)
def test_regression_likelihood(case):
    ref, theta = reference(case, "regression")
    N, C = case[3][0], case[3][3]
    idx = cpu_train_set(N, C)[0]
    y = torch.randn(60, C, generator=torch.Generator().manual_seed(12))
    V = directions(5, ref.n_params)
    VR, VH = ref.resid_vp(theta, idx, y, V.cpu().to(F64)), ref.hvp(theta, idx, y, V.cpu().to(F64))
    assert float(VR.abs().max()) >= 1e-2 * float((VH - VR).abs().max())
    if case[2] == "relu":
        assert ref.min_abs_preactivation(theta) >= 1e-5
    gi, gy = idx.cuda(), y.cuda()
    bs = [(gi[:37].contiguous(), gy[:37].contiguous()), (gi[37:].contiguous(), gy[37:].contiguous())]
    m = edge_model(*case)
    try:
        m.engine.set_likelihood("regression")
        e_r = rel_err(resid_product(case, V, bs), VR)
    finally:
        m.engine.set_likelihood("classification")
    G, loss = hessian_product(case, V, "regression", bs)
    e_h, want_loss = rel_err(G, VH), float(ref.loss(theta, idx, y))
    print(f"{case_id(case)} regression: R {e_r:.2e} H {e_h:.2e}, loss {float(loss):.6f} vs {want_loss:.6f}")
    assert e_r <= BOUND and e_h <= BOUND and abs(float(loss) - want_loss) <= 1e-5 * abs(want_loss)


@pytest.mark.parametrize("case", [GCN_RELU_BIG, ("sage", 2, "tanh", SHAPES[0], False)], ids=case_id)
def test_two_calls_return_the_same_bits_and_G_accumulates(case):
    eng = edge_model(*case).engine
    V = directions(33, eng.n_params)
    assert torch.equal(resid_product(case, V), resid_product(case, V))
    assert torch.equal(hessian_product(case, V)[0], hessian_product(case, V)[0])
    idx, y = train_batches(case[3][0], case[3][3])[0]
    G = torch.zeros_like(V)
    eng.hessian_resid_matmat_(G, idx, y, V)
    once = G.clone()
    eng.hessian_resid_matmat_(G, idx, y, V)
    assert float(once.abs().max()) > 0 and torch.equal(G, once + once)  # x + x is exact in fp32
    eng.check_async_errors()


@pytest.mark.parametrize("case", [("gcn", 2, "tanh", SHAPES[1], False), SAGE_RELU_BIG], ids=case_id)
def test_a_small_workspace_limit_gives_the_same_product(case):
    eng = edge_model(*case).engine
    VR, _ = expected(case, 33)
    V = directions(33, eng.n_params)
    one = resid_product(case, V)
    try:
        eng.set_workspace_limit(1 << 20)  # E and T of one direction: 300 x 64 floats each -- several chunks of directions
        many = resid_product(case, V)
    finally:
        eng.set_workspace_limit(WS_DEFAULT)
    e, e64 = rel_err(many, one), rel_err(many, VR)
    print(f"{case_id(case)}: chunked vs one chunk {e:.2e}; chunked vs fp64 {e64:.2e}")
    assert e <= BOUND and e64 <= BOUND


@pytest.mark.parametrize("case", SMALL, ids=case_id)
def test_full_matches_the_dense_fp64_hessian(case):
    import laplace_gnn_amd as lg

    check_same_inputs(case)
    ref, theta = reference(case)
    N, C = case[3][0], case[3][3]
    ci, cy = cpu_train_set(N, C)
    H64 = ref.dense(theta, ci, cy)
    idx, y = train_set(N, C)
    be = lg.HipHessian(edge_model(*case), "classification")
    loss, H = be.full(idx, y)
    eye = torch.eye(ref.n_params, device="cuda")
    G, loss2 = be.hessian_matmat([(idx, y)], eye)
    e, e_sym, e_mm = rel_err(H, H64), float((H - H.T).abs().max()) / float(H.abs().max()), rel_err(G, H.double())
    want_loss = float(ref.loss(theta, ci, cy))
    print(f"{case_id(case)}: full vs fp64 {e:.2e}, asymmetry {e_sym:.2e}, hessian_matmat(I) vs full {e_mm:.2e}, "
          f"loss {float(loss):.6f} vs {want_loss:.6f}")
    assert e <= BOUND and e_sym <= BOUND and e_mm <= BOUND
    assert abs(float(loss) - want_loss) <= 1e-5 * want_loss and abs(float(loss2) - want_loss) <= 1e-5 * want_loss
    try:  # several identity blocks, each in several chunks of the library's
        be.RESID_BLOCK = 64
        be.engine.set_workspace_limit(1 << 20)
        e_blocks = rel_err(be.full(idx, y)[1], H64)
    finally:
        be.engine.set_workspace_limit(WS_DEFAULT)
    assert e_blocks <= BOUND
    ry = torch.randn(60, C, generator=torch.Generator().manual_seed(12))
    rref, _ = reference(case, "regression")
    try:  # regression: sum J^T J + R, factor on the loss alone
        rloss, rH = lg.HipHessian(edge_model(*case), "regression").full(idx, ry.cuda())
    finally:
        be.engine.set_likelihood("classification")
    e_reg = rel_err(rH, rref.dense(theta, ci, ry))
    print(f"{case_id(case)}: blocks of 64 under 1 MiB {e_blocks:.2e}, regression full {e_reg:.2e}")
    assert e_reg <= BOUND and abs(float(rloss) - float(rref.loss(theta, ci, ry))) <= 1e-5 * float(rref.loss(theta, ci, ry))


@pytest.mark.parametrize("case", SMALL, ids=case_id)
def test_full_laplace_on_the_exact_hessian(case):
    import laplace_gnn_amd as lg

    ref, theta = reference(case)
    N, C = case[3][0], case[3][3]
    ci, cy = cpu_train_set(N, C)
    H64 = ref.dense(theta, ci, cy)
    delta = 64.0  # min eig(H) is -7.4 and -20.2 in fp64 here; the five optimiser steps below move delta by less than a factor 2
    prec = H64 + delta * torch.eye(ref.n_params, dtype=F64)
    lo = float(torch.linalg.eigvalsh(0.5 * (prec + prec.T)).min())
    assert lo > 0.1 and float(torch.linalg.eigvalsh(H64).min()) < 0, "the prior makes an indefinite Hessian positive definite"
    want_loss = float(ref.loss(theta, ci, cy))
    want = -want_loss - 0.5 * (float(torch.logdet(prec)) - ref.n_params * float(torch.log(torch.tensor(delta, dtype=F64)))
                               + delta * float(theta @ theta))
    m = edge_model(*case)
    for la in (lg.Laplace(m, "classification", "all", "full", backend=lg.HipHessian, prior_precision=delta),
               lg.FullLaplace(m, "classification", backend=lg.HipHessian, prior_precision=delta)):
        assert type(la) is lg.FullLaplace
        la.fit(lg.TensorBatchLoader(*train_set(N, C), batch_size=37))
        got = float(la.log_marginal_likelihood())
        e_h = rel_err(la.H, H64)
        print(f"{case_id(case)}: la.H {e_h:.2e}, loss {float(la.loss):.6f} vs {want_loss:.6f}, marglik {got:.5f} vs {want:.5f}")
        assert e_h <= BOUND and abs(float(la.loss) - want_loss) <= 1e-5 * want_loss
        assert abs(got - want) <= MARGLIK_RTOL * abs(want)
    idx = train_set(N, C)[0][:8].contiguous()
    probs = la(idx)
    assert probs.shape == (8, C) and bool(torch.isfinite(probs).all()) and float((probs.sum(1) - 1).abs().max()) < 1e-4
    assert la.sample(3, generator=torch.Generator(device="cuda").manual_seed(0)).shape == (3, ref.n_params)
    assert set(la.state_dict()) >= {"H", "mean", "loss"}
    la.optimize_prior_precision(method="marglik", n_steps=5, lr=0.1, init_prior_prec=delta)
    assert bool(torch.isfinite(la.log_marginal_likelihood()))
    with pytest.raises(NotImplementedError, match="HipHessian"):
        la.neg_marglik_adj_grad([])
    m.engine.check_async_errors()


@pytest.mark.parametrize("case", [("gcn", 3, "relu", SHAPES[0], False), ("sage", 2, "relu", SHAPES[0], True)], ids=case_id)
def test_models_without_a_closed_form_are_refused(case):
    import laplace_gnn_amd as lg

    m = edge_model(*case)
    eng = m.engine
    idx, y = train_batches(case[3][0], case[3][3])[0]
    V = directions(2, eng.n_params)
    G = torch.zeros_like(V)
    eng.ggn_matmat_(torch.zeros_like(V), torch.zeros(1, device="cuda"), idx, y, V)
    with pytest.raises(lg._lib.HipLibraryError, match="exact Hessian: closed-form models only"):
        eng.hessian_resid_matmat_(G, idx, y, V)
    with pytest.raises(lg._lib.HipLibraryError, match="exact Hessian: closed-form models only"):
        lg.HipHessian(m, "classification").full(idx, y)
    assert float(G.abs().max()) == 0.0
    eng.check_async_errors()


@pytest.mark.parametrize("case", [("gcn", 2, "relu", SHAPES[0], False), ("sage", 2, "tanh", SHAPES[0], False)], ids=case_id)
def test_an_out_of_range_id_or_label_contributes_nothing_and_sets_the_sticky_flag(case):
    import laplace_gnn_amd as lg

    eng = edge_model(*case).engine
    N, C = case[3][0], case[3][3]
    idx, y = train_batches(N, C)[0]
    V = directions(5, eng.n_params)
    keep = torch.ones(37, dtype=torch.bool, device="cuda")
    keep[4] = False
    want = torch.zeros_like(V)
    eng.ggn_matmat_(torch.zeros_like(V), torch.zeros(1, device="cuda"), idx, y, V)
    eng.hessian_resid_matmat_(want, idx[keep].contiguous(), y[keep].contiguous(), V)
    eng.check_async_errors()
    assert float(want.abs().max()) > 0
    for bad_id in (N, -1):
        bad = idx.clone()
        bad[4] = bad_id
        G = torch.zeros_like(V)
        eng.hessian_resid_matmat_(G, bad, y, V)
        with pytest.raises(lg._lib.HipLibraryError, match="node index"):
            eng.check_async_errors()
        eng.check_async_errors()  # cleared
        assert rel_err(G, want) <= BOUND
    bad_y = y.clone()
    bad_y[4] = C
    G = torch.zeros_like(V)
    eng.hessian_resid_matmat_(G, idx, bad_y, V)
    with pytest.raises(lg._lib.HipLibraryError, match="label"):
        eng.check_async_errors()
    eng.check_async_errors()
    assert rel_err(G, want) <= BOUND
    with pytest.raises(ValueError, match="G must be contiguous"):
        eng.hessian_resid_matmat_(torch.zeros(4, eng.n_params, device="cuda"), idx, y, V)
