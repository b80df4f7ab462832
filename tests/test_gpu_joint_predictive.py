"""The joint GLM predictive on the GPU (csrc/glmcov.hip behind ``lgnn_glm_covariance``, ``GraphEngine.glm_covariance``,
``la.glm_covariance`` / ``la(x, joint=True)``): K = J(a) P^-1 J(b)^T for block-diagonal Kronecker and diagonal posteriors.

At the C-ABI level the operands are synthetic and seeded -- Q_A, Q_B from ``torch.linalg.qr`` of Gaussians, S uniform in
[0.05, 2] -- and the yardstick is fp64 from the same operands and ``eng.jacobians(...)[0].double()``: independent of the
eigensolver and of the routes of the code under test.  Error: max |got - want| / max |want|; bound 1e-4, the project's bar for
predictive variances.  Models and id lists are those of tests/test_gpu_gp.py, restated: ``edge_graph`` has a hub row (more than
64 stored entries), two isolated nodes and duplicate edges; idx_a (37 ids) holds the hub, the isolated nodes and a repeated id,
idx_b has 50 ids.  (N, F, H, C) = (96, 13, 10, 5) and (300, 37, 64, 7): a 32-wide k-tile is crossed, the output tiles of 128
rows are ragged (185, 350) and K is odd.

1. structured route and ``from_jacobians=True`` against fp64: {gcn, sage} x {1, 2 layers} x {relu, tanh} x {diag, kron} x shapes;
2. general route against fp64: a 3-layer GCN and a GraphSAGE with res + LayerNorm (three blocks), both posteriors;
3. ``idx_b=None``: exactly symmetric; two calls: identical bits; under the default workspace and under 1 MiB;
4. a 1 MiB workspace: several chunk pairs (asserted from the engine's count), within the bound of fp64;
5. the diagonal of K(a, a) against ``lgnn_glm_variance``'s variances for the same operands;
6. ids N and -1: zero rows and columns, the sticky flag, the other entries unchanged;
7. the front: the reference's goldens through ``lg.KronLaplace`` / ``lg.DiagLaplace`` / ``lg.FullLaplace``, and
   ``la.glm_covariance`` against ``functional_covariance`` of device Jacobians.
Every case prints what it measured."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BOUND = 1e-4
WS_DEFAULT = 32 << 30
SHAPES = [(96, 13, 10, 5), (300, 37, 64, 7)]
POSTERIORS = ("diag", "kron")
STRUCTURED = [(k, L, a, s, False) for k in ("gcn", "sage") for L in (1, 2) for a in ("relu", "tanh") for s in SHAPES]
GENERAL = [("gcn", 3, "relu", SHAPES[0], False), ("sage", 2, "relu", SHAPES[0], True)]


def _id(c):
    k, L, a, s, ext = c
    return f"{k}{L}-{a}-N{s[0]}F{s[1]}" + ("-resln" if ext else "")


def edge_graph(N, seed):
    """Random edges with duplicates, node 3 with more than 64 stored entries, nodes N-1 and N-2 isolated."""
    g = torch.Generator().manual_seed(seed)
    hi = N - 2
    ei = torch.randint(0, hi, (2, 3 * N), generator=g)
    hub = torch.randperm(hi, generator=g)[:70]
    return torch.cat([ei, ei[:, :N // 3], torch.stack([torch.full((70,), 3), hub]), torch.stack([hub, torch.full((70,), 3)])], 1)


@functools.lru_cache(maxsize=None)
def edge_model(kind, L, act, shape, extras=False, seed=0):
    import laplace_gnn_amd as lg

    N, F, H, C = shape
    X = torch.randn(N, F, generator=torch.Generator().manual_seed(seed + 1))
    torch.manual_seed(seed)
    kw = dict(res=True, norm="layer") if extras else {}
    m = (lg.GCN if kind == "gcn" else lg.GraphSAGE)(F, H, C, L, X, edge_graph(N, seed), act=act, **kw).eval().cuda()
    if extras:
        gn = torch.Generator().manual_seed(seed + 5)
        with torch.no_grad():
            for nm in m.norms:
                nm.weight.copy_((0.5 + torch.rand(H, generator=gn)).cuda())
                nm.bias.copy_((0.3 * torch.randn(H, generator=gn)).cuda())
    return m


def batches(N):
    a = torch.randperm(N - 2, generator=torch.Generator().manual_seed(2))[:37].clone()
    a[0], a[1], a[2] = 3, N - 1, N - 2  # the hub, the isolated nodes
    a[7] = a[9]                         # a repeated id
    b = torch.randperm(N, generator=torch.Generator().manual_seed(3))[:50].clone()
    return a.cuda(), b.cuda()


@functools.lru_cache(maxsize=None)
def operands(case, post):
    """Seeded synthetic operands of the model's blocks: dict(QA=[..], QB=[..], S=[..]) on the device."""
    eng = edge_model(*case).engine
    g = torch.Generator().manual_seed(11)
    QA, QB, S = [], [], []
    for din, dout in eng.block_dims:
        if post == "kron":
            QA.append(torch.linalg.qr(torch.randn(din, din, generator=g, dtype=torch.float64))[0].float().cuda())
            QB.append(torch.linalg.qr(torch.randn(dout, dout, generator=g, dtype=torch.float64))[0].float().cuda())
        else:
            QA.append(None)
            QB.append(None)
        S.append((0.05 + 1.95 * torch.rand(dout, din + 1, generator=g)).cuda())
    return dict(QA=QA, QB=QB, S=S)


def rotated64(eng, J, ops):
    """fp64 rows J [R, P] with every Kronecker block in its eigenbasis, and the flat scale: K = (Ja~ * s) Jb~^T."""
    R, off, cols, scale = J.shape[0], 0, [], []
    for (din, dout), QA, QB, S in zip(eng.block_dims, ops["QA"], ops["QB"], ops["S"]):
        Jw = J[:, off:off + dout * din].reshape(R, dout, din)
        off += dout * din
        Jb = J[:, off:off + dout]
        off += dout
        if QA is not None:
            Jw = torch.einsum("ok,roi,ij->rkj", QB.double(), Jw, QA.double())
            Jb = Jb @ QB.double()
        cols += [Jw.reshape(R, -1), Jb]
        scale += [S[:, :din].double().reshape(-1), S[:, din].double()]
    assert off == J.shape[1]
    return torch.cat(cols, 1), torch.cat(scale)


def fp64_cov(eng, a, b, ops):
    P = eng.n_params
    Ja, s = rotated64(eng, eng.jacobians(a)[0].double().reshape(-1, P), ops)
    Jb, _ = rotated64(eng, eng.jacobians(b)[0].double().reshape(-1, P), ops)
    return (Ja * s) @ Jb.T


@functools.lru_cache(maxsize=None)
def want_ab(case, post):
    a, b = batches(case[3][0])
    return fp64_cov(edge_model(*case).engine, a, b, operands(case, post))


def err(got, want):
    scale = float(want.abs().max())
    assert scale > 0 and got.shape == want.shape
    return float((got.double() - want).abs().max()) / scale


@pytest.mark.parametrize("post", POSTERIORS)
@pytest.mark.parametrize("case", STRUCTURED, ids=_id)
def test_structured_route_and_the_route_over_jacobians_against_fp64(case, post):
    eng = edge_model(*case).engine
    a, b = batches(case[3][0])
    ops, want = operands(case, post), want_ab(case, post)
    e_s = err(eng.glm_covariance(a, b, **ops), want)
    e_j = err(eng.glm_covariance(a, b, from_jacobians=True, **ops), want)
    eng.check_async_errors()
    print(f"{_id(case)} {post}: structured {e_s:.2e} from_jacobians {e_j:.2e} ratio {e_s / max(e_j, 1e-30):.2f}")
    assert e_s <= BOUND and e_j <= BOUND


@pytest.mark.parametrize("post", POSTERIORS)
@pytest.mark.parametrize("case", GENERAL, ids=_id)
def test_general_route_against_fp64(case, post):
    eng = edge_model(*case).engine
    assert len(eng.block_dims) == 3
    a, b = batches(case[3][0])
    e = err(eng.glm_covariance(a, b, **operands(case, post)), want_ab(case, post))
    eng.check_async_errors()
    print(f"{_id(case)} {post}: general {e:.2e}")
    assert e <= BOUND


SYM_CASES = [("gcn", 2, "relu", SHAPES[1], False), ("sage", 2, "tanh", SHAPES[0], False), ("gcn", 1, "relu", SHAPES[0], False),
             ("gcn", 3, "relu", SHAPES[0], False), ("sage", 2, "relu", SHAPES[0], True)]


@pytest.mark.parametrize("post", POSTERIORS)
@pytest.mark.parametrize("case", SYM_CASES, ids=_id)
def test_same_ids_give_an_exactly_symmetric_covariance_and_calls_repeat_bit_for_bit(case, post):
    eng = edge_model(*case).engine
    a, b = batches(case[3][0])
    ops = operands(case, post)
    try:
        for limit in (WS_DEFAULT, 1 << 20):
            eng.set_workspace_limit(limit)
            for kw in ({}, {"from_jacobians": True}):
                K = eng.glm_covariance(a, None, **kw, **ops)
                assert torch.equal(K, K.T), (limit, kw)
                assert torch.equal(K, eng.glm_covariance(a, **kw, **ops)), (limit, kw)
                assert torch.equal(eng.glm_covariance(a, b, **kw, **ops), eng.glm_covariance(a, b, **kw, **ops)), (limit, kw)
    finally:
        eng.set_workspace_limit(WS_DEFAULT)
    eng.check_async_errors()


CHUNK_CASES = [("gcn", 2, "relu", SHAPES[1], False), ("sage", 2, "relu", SHAPES[1], False), ("gcn", 3, "relu", SHAPES[0], False)]


@pytest.mark.parametrize("post", POSTERIORS)
@pytest.mark.parametrize("case", CHUNK_CASES, ids=_id)
def test_a_small_workspace_limit_runs_several_chunks_within_the_bound(case, post):
    eng = edge_model(*case).engine
    a, b = batches(case[3][0])
    try:
        eng.set_workspace_limit(1 << 20)
        K = eng.glm_covariance(a, b, **operands(case, post))
        chunks = eng.glm_covariance_chunk_pairs()
    finally:
        eng.set_workspace_limit(WS_DEFAULT)
    eng.glm_covariance(a, b, **operands(case, post))
    one = eng.glm_covariance_chunk_pairs()
    e = err(K, want_ab(case, post))
    print(f"{_id(case)} {post}: {chunks} chunk pairs under 1 MiB ({one} by default), vs fp64 {e:.2e}")
    assert chunks > 1 and one == 1 and e <= BOUND


VAR_CASES = [("gcn", 2, "relu", SHAPES[0], False), ("sage", 2, "relu", SHAPES[1], False), ("gcn", 1, "relu", SHAPES[0], False),
             ("sage", 1, "tanh", SHAPES[1], False)]


@pytest.mark.parametrize("post", POSTERIORS)
@pytest.mark.parametrize("case", VAR_CASES, ids=_id)
def test_the_diagonal_matches_the_matrix_free_variances(case, post):
    """An independent kernel: ``lgnn_glm_variance`` (csrc/predictive.hip) from the same operands in its own conventions."""
    eng = edge_model(*case).engine
    a, _ = batches(case[3][0])
    ops = operands(case, post)
    S, QA, QB = ops["S"], ops["QA"], ops["QB"]
    S1 = S[-1][:, :-1].contiguous()
    if post == "kron":
        var_ops = dict(S1=S1, kappa=(QB[-1] * QB[-1]) @ S[-1][:, -1], QA1=QA[-1], QB1sq=QB[-1] * QB[-1])
        if len(S) == 2:
            var_ops.update(S0=S[0], QA0=QA[0], QB0=QB[0])
    else:
        var_ops = dict(S1=S1, kappa=S[-1][:, -1].contiguous())
        if len(S) == 2:
            var_ops.update(S0=S[0])
    if len(S) == 1:
        var_ops["S0"] = None
    eng.set_likelihood("classification")
    _, f_var = eng.glm_variance(a, **var_ops)
    K = eng.glm_covariance(a, **ops)
    eng.check_async_errors()
    e = err(torch.diagonal(K).reshape(f_var.shape), f_var.double())
    print(f"{_id(case)} {post}: diag K(a, a) vs lgnn_glm_variance {e:.2e}")
    assert e <= BOUND


@pytest.mark.parametrize("post", POSTERIORS)
@pytest.mark.parametrize("case", [("gcn", 2, "relu", SHAPES[0], False), ("sage", 1, "relu", SHAPES[0], False),
                                  ("gcn", 3, "relu", SHAPES[0], False)], ids=_id)
def test_out_of_range_ids_give_zero_rows_and_columns_and_the_sticky_flag(case, post):
    import laplace_gnn_amd as lg

    eng = edge_model(*case).engine
    N, C = case[3][0], case[3][3]
    a, b = batches(N)
    ops = operands(case, post)
    good = eng.glm_covariance(a, b, **ops).view(37, C, 50, C)
    eng.check_async_errors()
    bad_a, bad_b = a.clone(), b.clone()
    bad_a[4], bad_b[11] = N, -1
    K = eng.glm_covariance(bad_a, bad_b, **ops).view(37, C, 50, C)
    with pytest.raises(lg._lib.HipLibraryError, match="node index"):
        eng.check_async_errors()
    eng.check_async_errors()  # cleared
    ka, kb = torch.ones(37, dtype=torch.bool, device="cuda"), torch.ones(50, dtype=torch.bool, device="cuda")
    ka[4], kb[11] = False, False
    assert float(K[4].abs().max()) == 0.0 and float(K[:, :, 11].abs().max()) == 0.0
    e = err(K[ka][:, :, kb], good[ka][:, :, kb].double())
    print(f"{_id(case)} {post}: entries beside the bad ids differ by {e:.2e}")
    assert e <= BOUND


def test_a_wrong_number_of_blocks_is_a_named_error():
    import ctypes

    import laplace_gnn_amd as lg

    case = ("gcn", 2, "relu", SHAPES[0], False)
    eng = edge_model(*case).engine
    a, _ = batches(case[3][0])
    ops = operands(case, "diag")
    with pytest.raises(ValueError, match="one entry per Linear layer"):
        eng.glm_covariance(a, QA=ops["QA"][:1], QB=ops["QB"][:1], S=ops["S"][:1])
    K = torch.empty(37 * 5, 37 * 5, device="cuda")
    arr = lg._lib.ptr_array([None])
    sv = lg._lib.ptr_array([ops["S"][0].data_ptr()])
    rc = eng.lib.lgnn_glm_covariance(eng._h, a.data_ptr(), 37, a.data_ptr(), 37, 1, arr, arr, sv, 0, K.data_ptr(), 37 * 5,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc != 0 and b"n_blocks" in eng.lib.lgnn_last_error()


# ---- the front on the device ---------------------------------------------------------------------------------------------
JOINT_NAMES = ["gcn_small_1batch_s0", "sage_small_1batch_s0", "gcn_resln_small_1batch_s0", "gcn_regression"]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@functools.lru_cache(maxsize=None)
def fitted(name, structure):
    """The fixture's model on the device and its fitted posterior (prior and noise as tools/make_joint_golden.py)."""
    import laplace_gnn_amd as lg
    from conftest import GOLDEN
    from golden_utils import constructor_extras

    j = np.load(os.path.join(GOLDEN, "joint", name + ".npz"))
    g = np.load(os.path.join(GOLDEN, str(j["source"]) + ".npz"))
    kind, L = str(g["kind"]), int(g["num_layers"])
    X, ei = torch.from_numpy(g["X"]), torch.from_numpy(g["edge_index"])
    m = (lg.GCN if kind == "gcn" else lg.GraphSAGE)(X.shape[1], g["W0"].shape[0], g[f"W{L - 1}"].shape[0], L, X, ei,
                                                    symmetric=bool(g["symmetric"]), **constructor_extras(g),
                                                    **({"act": str(g["act"])} if "act" in g.files else {}))
    with torch.no_grad():
        for l, conv in enumerate(m.convs):
            conv.lin.weight.copy_(torch.from_numpy(g[f"W{l}"]))
            conv.lin.bias.copy_(torch.from_numpy(g[f"b{l}"]))
        for l, lin in enumerate(m.res):
            lin.weight.copy_(torch.from_numpy(g[f"Wr{l}"]))
            lin.bias.copy_(torch.from_numpy(g[f"br{l}"]))
        if m.norm_kind is not None:
            for l, nm in enumerate(m.norms):
                nm.weight.copy_(torch.from_numpy(g[f"norm_w{l}"]))
                nm.bias.copy_(torch.from_numpy(g[f"norm_b{l}"]))
    m = m.eval().cuda()
    loader = lg.TensorBatchLoader(torch.from_numpy(g["train_idx"]).cuda(), torch.from_numpy(g["train_y"]).cuda(),
                                  batch_size=int(g["batch_size"]))
    la = lg.Laplace(m, str(j["likelihood"]), "all", structure, prior_precision=float(j["prior"]), sigma_noise=float(j["sigma_noise"]))
    la.fit(loader)
    return j, la


@pytest.mark.parametrize("structure", ("kron", "diag", "full"))
@pytest.mark.parametrize("name", JOINT_NAMES)
def test_front_matches_the_reference_goldens(name, structure):
    j, la = fitted(name, structure)
    pred = torch.from_numpy(j["pred"]).cuda()
    C = la.n_outputs
    on_device = la._glm_covariance_device(pred, None) is not None
    assert on_device == (structure != "full")  # Kronecker and diagonal posteriors: lgnn_glm_covariance; full: Jacobian chunks
    f_mu, f_cov = la._glm_predictive_distribution(pred, joint=True)
    assert f_mu.shape == (6 * C,) and f_cov.shape == (6 * C, 6 * C) and torch.equal(f_cov, f_cov.T)
    e_mu, e_cov = rel(f_mu.cpu().numpy(), j[f"{structure}_f_mu_joint"]), rel(f_cov.cpu().numpy(), j[f"{structure}_f_cov"])
    print(f"{name} {structure}: f_mu {e_mu:.2e} f_cov {e_cov:.2e} ({'lgnn_glm_covariance' if on_device else 'Jacobian chunks'})")
    assert e_mu <= 1e-5 and e_cov <= BOUND
    if str(j["likelihood"]) == "regression":
        mu, cov = la(pred, joint=True)
        assert rel(mu.cpu().numpy(), j[f"{structure}_call_mu"]) <= 1e-5 and rel(cov.cpu().numpy(), j[f"{structure}_call_cov"]) <= BOUND
    else:
        assert torch.equal(la(pred, joint=True), la(pred))
    la.backend.engine.check_async_errors()


@pytest.mark.parametrize("name", JOINT_NAMES)
def test_glm_covariance_matches_functional_covariance_of_device_jacobians(name):
    j, la = fitted(name, "kron")
    x, x2 = torch.from_numpy(j["pred"]).cuda(), torch.tensor([9, 11, 12, 9]).cuda()
    C = la.n_outputs
    Js = la.backend.jacobians(torch.cat([x, x2]))[0]
    want = la.functional_covariance(Js).double()
    square = la.glm_covariance(torch.cat([x, x2]))
    cross = la.glm_covariance(x, x2)
    e_sq, e_cr = err(square, want), err(cross, want[:6 * C, 6 * C:])
    print(f"{name}: la.glm_covariance vs functional_covariance(Js): square {e_sq:.2e} cross {e_cr:.2e}")
    assert cross.shape == (6 * C, 4 * C) and torch.equal(square, square.T)
    assert e_sq <= BOUND and e_cr <= BOUND
    la.backend.engine.check_async_errors()


def test_a_workspace_limit_below_one_samples_buffers_is_a_named_error():
    """V is not slabbed over k: at (F, H, C) = (200, 64, 7) one sample's V pair is 731 KB, above half of a 1 MiB limit."""
    import laplace_gnn_amd as lg

    case = ("gcn", 2, "relu", (96, 200, 64, 7), False)
    eng = edge_model(*case).engine
    a, b = batches(96)
    try:
        eng.set_workspace_limit(1 << 20)
        for post, kw in (("kron", {}), ("kron", {"from_jacobians": True}), ("diag", {"from_jacobians": True})):
            with pytest.raises(lg._lib.HipLibraryError, match="workspace limit is below one sample"):
                eng.glm_covariance(a, b, **kw, **operands(case, post))
        K = eng.glm_covariance(a, b, **operands(case, "diag"))  # the diagonal posterior's tables fit: several chunk pairs
        assert eng.glm_covariance_chunk_pairs() > 1
    finally:
        eng.set_workspace_limit(WS_DEFAULT)
    e = err(K, want_ab(case, "diag"))
    print(f"{_id(case)} diag under 1 MiB: {e:.2e}")
    eng.check_async_errors()
    assert e <= BOUND


def test_low_rank_joint_predictive_agrees_with_its_own_functional_covariance():
    """``LowRankLaplace`` keeps its ``functional_covariance`` (laplace/baselaplace.py:1802-1810); ``joint=True`` and
    ``glm_covariance`` go through ``_covariance_rows``: the two hold the same formula and must agree."""
    import laplace_gnn_amd as lg

    case = ("gcn", 2, "relu", SHAPES[0], False)
    N, C = case[3][0], case[3][3]
    a, b = batches(N)
    idx = torch.cat([a, b[:23]]).contiguous()
    y = torch.randint(0, C, (60,), generator=torch.Generator().manual_seed(11)).cuda()
    la = lg.Laplace(edge_model(*case), "classification", "all", "lowrank", prior_precision=0.7, backend_kwargs=dict(low_rank=8))
    la.fit(lg.TensorBatchLoader(idx, y, batch_size=37))
    x = b[30:36].contiguous()
    Js, f = la.backend.jacobians(x)
    own = la.functional_covariance(Js).double()
    f_mu, f_cov = la._glm_predictive_distribution(x, joint=True)
    e_joint = err(f_cov, own)
    e_cross = err(la.glm_covariance(x[:2], x[2:]), own[:2 * C, 2 * C:])
    blocks = torch.stack([f_cov[n * C:(n + 1) * C, n * C:(n + 1) * C] for n in range(6)])
    e_var = err(blocks, la._glm_predictive_distribution(x)[1].double())
    print(f"low rank: joint vs functional_covariance {e_joint:.2e}, cross {e_cross:.2e}, blocks vs marginal {e_var:.2e}")
    assert torch.equal(f_cov, f_cov.T) and torch.equal(f_mu, f.flatten())
    assert e_joint <= BOUND and e_cross <= BOUND and e_var <= BOUND
