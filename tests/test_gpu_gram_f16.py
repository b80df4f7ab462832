"""The Gram role of paths_fused_kernel on v_mfma_f32_16x16x32_f16 over TWO scaled fp16 pieces per tile value (csrc/paths_fused.hip,
gram_f16_role; the scales: PathScale in csrc/paths.h, GramScale in paths_fused.hip).

Without a GPU: numpy restatements of the split (h0 = fp16(y), h1 = fp16(y - h0), both round to nearest), of the operand
identity U x U + U x T = T x T + T x U = (h0 + h1)^T (h0 + h1), and of the bound the launch's scale is taken from, checked against the tile
values Y the oracle's backward pass gives for one small batch of a GCN and of a GraphSAGE.

With a GPU: B_0 of the path route against the fp32 role of the same library (LGNN_GRAM_F32=1, read per call), the CPU oracle
and an fp64 restatement, at the bounds of tests/test_gpu_split_gram.py:

* against the fp32 role, same inputs: 2e-6,
* against the CPU oracle: 1e-4,
* against the fp64 restatement: e_new <= max(1e-6, 2 e_f32 + 1e-7).

Shapes, graphs and the runner of tests/test_gpu_gram16.py (N = 300, F = 8, batches of 60, the route asserted on every
accumulate, five consecutive accumulates per comparison).  No test looks at which tile form a launch ran."""
import numpy as np
import pytest
import torch

import gnn_laplace_oracle as O
from gpu_utils import oracle_from_arrays, rel
from test_gpu_gram16 import DENSE, M, N, F, REPEATS, SPARSE, _engine, _graph, _run
from test_gpu_scale import _fp64_kfac_classes, _make
from test_gpu_split_gram import _accumulate

gpu = pytest.mark.gpu


# ---- without a GPU --------------------------------------------------------------------------------------------------------
def _split(y):
    """the kernel's split_pair: both conversions round to nearest even and keep fp16 subnormals (numpy's astype does)"""
    y = np.asarray(y, np.float32)
    h0 = y.astype(np.float16)
    h1 = (y - h0.astype(np.float32)).astype(np.float16)
    return h0, h1


def test_the_two_pieces_reproduce_a_scaled_value():
    """Over the scaled range |y| <= 2^15: y - h0 is exact in fp32, h0 + h1 is y to 2^-22 |y| wherever h1 is a normal fp16
    (|y| >= 2^-3 is enough: |y - h0| is then either zero or at least 2^-14) and to 2^-25 -- half a subnormal step -- below."""
    rng = np.random.default_rng(0)
    mant = rng.uniform(1.0, 2.0, 400000).astype(np.float32) * rng.choice([-1.0, 1.0], 400000).astype(np.float32)
    expo = rng.integers(-40, 15, 400000)
    y = np.ldexp(mant, expo).astype(np.float32)
    y = np.concatenate([y, np.float32([0.0, 2.0 ** 15, -2.0 ** 15, 2.0 ** -3, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 1 + 2.0 ** -11])])
    assert np.abs(y).max() <= 2.0 ** 15
    h0, h1 = _split(y)
    assert np.isfinite(h0).all() and np.isfinite(h1).all()
    r = y.astype(np.float64) - h0.astype(np.float64)
    assert np.array_equal(r.astype(np.float32).astype(np.float64), r), "y - h0 is exact in fp32"
    err = np.abs(r - h1.astype(np.float64))
    big = np.abs(y) >= 2.0 ** -3
    assert (err[big] <= 2.0 ** -22 * np.abs(y[big])).all()
    assert (err <= np.maximum(2.0 ** -22 * np.abs(y), 2.0 ** -25)).all()


def test_the_two_operand_forms_give_the_complete_product():
    """U = (h0 | h1) and T = (h1 | h0) along K: U^T U + U^T T = (h0 + h1)^T (h0 + h1), all four piece products (fp64: exact up
    to the sums' rounding)."""
    rng = np.random.default_rng(1)
    y = (rng.standard_normal((40, 24)) * np.exp(rng.uniform(-3, 3, (40, 1)))).astype(np.float32) * np.float32(64.0)
    h0, h1 = (p.astype(np.float64) for p in _split(y))
    U, T = np.concatenate([h0, h1]), np.concatenate([h1, h0])
    want = (h0 + h1).T @ (h0 + h1)
    for got in (U.T @ U + U.T @ T, T.T @ T + T.T @ U):  # (the kernel runs the second pair)
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    assert rel(got, y.astype(np.float64).T @ y.astype(np.float64)) <= 2.0 ** -21


def _tiles_and_bound(kind, m, idx):
    """Y [N, C, H] of one batch from the oracle's backward pass (the gradient at the first Linear's output, class column by
    class column) and the restatement of PathScale: the column factors cn and the launch's bound on |Y[n][c, j]| cn_j."""
    fw = O.forward_ext(m)
    f = fw["out"][idx]
    Nn, C = fw["out"].shape
    V = O.kfac_seeds(f, True)
    Y = []
    for c in range(C):
        G = np.zeros((Nn, C), np.float32)
        np.add.at(G, idx, V[:, :, c])
        Y.append(O.backward_general(m, fw, G)[0][0])
    Y = np.stack(Y, 1).astype(np.float64)
    al, be, ga, u, p = (a.astype(np.float64) for a in O.seed_factors(f, True))
    W1 = m.weights[1].astype(np.float64)
    PT = abs(m.PT).astype(np.float64)
    sel = np.zeros((Nn, len(idx)))
    sel[idx, np.arange(len(idx))] = 1.0  # (a node listed twice owns two columns; GraphSAGE below: distinct ids)
    H = W1.shape[1] // (2 if kind == "sage" else 1)
    halves = [W1[:, :H], W1[:, H:]] if kind == "sage" else [W1]
    cn = 2.0 ** -np.floor(np.log2(np.max([np.abs(h).max(0) for h in halves], 0)))

    def rows(coef_b, coef_g, Wh):  # max over the samples of  max_c |beta| max_j |b cn| + max_c |gamma| max_j |g cn|
        b, g = (u @ Wh) * cn, (p @ Wh) * cn
        return float((np.abs(coef_b).max(1) * np.abs(b).max(1) + np.abs(coef_g).max(1) * np.abs(g).max(1)).max())

    if kind == "gcn":
        wsum = float((PT @ (PT @ sel).sum(1)).max())  # sum over the paths n <- v <- m of |P^T[n, v] P^T[v, m]|
        w1max, bgmax = np.abs(halves[0] * cn).max(), rows(be, ga, halves[0])
    else:  # neighbour paths m -> n; a batch node's own beta / gamma path (weight 1) and its C one-hot alpha paths (|alpha_c|)
        own = np.zeros(Nn)
        own[idx] = 1.0 + np.abs(al).sum(1)
        wsum = float(((PT @ sel).sum(1) + own).max())
        w1max = max(np.abs(h * cn).max() for h in halves)
        bgmax = max(rows(be, ga, halves[1]), rows(be, ga, halves[0]), float(np.abs(halves[0] * cn).max()))
    # the two triangle inequalities: over a path's three terms, and over the rows k of the sample's seed block V[k, c]
    tri = np.abs(al).max() * w1max + bgmax
    vmax = float(np.abs(V.astype(np.float64)).sum(1).max())
    return Y, cn, wsum * (min(tri, vmax * w1max) + 2.0 ** -12 * tri)


@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_the_bound_is_a_bound(kind):
    """max_n sum_paths |w| * (min(tri, max_m max_c sum_k |V_m[k, c]| max |W1n|) + 2^-12 tri), tri = max |alpha| max |W1n| + max_m
    (max |beta| max |b_m| + max |gamma| max |g_m|), bounds every column-normalised tile value of the batch."""
    ei, idx = _graph(DENSE)
    idx = np.unique(idx.numpy())
    _, X, Ws, bs = _make(kind, N, F, 132, 7, 1, L=2, seed=5)
    Ws[1] = Ws[1] * (2.0 ** torch.randint(-12, 13, (Ws[1].shape[1],), generator=torch.Generator().manual_seed(3)))[None, :]
    m = oracle_from_arrays(kind, N, ei.numpy(), X.numpy(), [w.numpy() for w in Ws], [b.numpy() for b in bs], True)
    Y, cn, bound = _tiles_and_bound(kind, m, idx)
    top = np.abs(Y * cn[None, None, :]).max()
    print(f"{kind}: bound {bound:.4g}, largest normalised |Y| {top:.4g}, slack {bound / top:.3g}")
    assert top > 0 and np.isfinite(bound)
    assert top <= bound * (1 + 1e-6)


# ---- with a GPU -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("C", [7, 8, 9, 16, 17, 24, 25, 32, 33, 40, 48, 49, 64])
def test_class_counts(C):
    """one to three 16-row chunks, either side of every boundary; 49 and 64: a second launch of 1 / 16 classes"""
    _run(f"C={C}", "gcn", 256, C, DENSE)


@gpu
def test_one_class():
    """C = 1: the seed of a one-class softmax is exactly zero, B_0 a cancellation residue under both roles (see
    tests/test_gpu_gram16.py); a launch of one class with data in it is the class range (3, 4) below."""
    ei, idx = _graph(DENSE)
    _, X, Ws, bs = _make("gcn", N, F, 256, 1, 1, L=2, seed=257)
    y = torch.zeros(M, dtype=torch.int64)
    eng = _engine("gcn", ei, X, Ws, bs)
    calls = [(idx.cuda(), y.cuda(), M, {"paths": True})]
    f0, _, _ = _accumulate(eng, True, calls)
    for r in range(REPEATS):
        s0, _, _ = _accumulate(eng, False, calls)
        assert eng.last_kfac_used_paths
        print(f"C=1 repeat {r}: max |B_0| {np.abs(s0).max():.3e} (fp32 role {np.abs(f0).max():.3e})")
        assert np.isfinite(s0).all() and max(np.abs(s0).max(), np.abs(f0).max()) < 1e-10
    eng.check_async_errors()
    eng.close()


@gpu
@pytest.mark.parametrize("classes", [(3, 4), (0, 7), (16, 33), (8, 48)])
def test_class_ranges_of_one_call(classes):
    """launches of 1, 7, 17 and 40 classes that do not start at class 0"""
    _run(f"classes={classes}", "gcn", 256, 7 if classes[1] <= 7 else 48, DENSE, classes=classes)


@gpu
@pytest.mark.parametrize("H", [132, 192, 256])
@pytest.mark.parametrize("bg_edges", [DENSE, SPARSE])
@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_widths_instances_and_families(kind, bg_edges, H):
    _run(f"{kind} H={H} bg={bg_edges}", kind, H, 40, bg_edges)


@gpu
@pytest.mark.parametrize("C", [40, 48])
def test_regression_likelihood(C):
    _run(f"regression C={C}", "gcn", 256, C, DENSE, regression=True)


def _compare(what, kind, ei, idx, X, Ws, bs, C, expect_data=True):
    """the fp32 role and the fp64 restatement once, then REPEATS accumulates under the default role.  Returns the last B_0.
    Two accumulates come first and are thrown away: a GCN batch's path list is built with atomics, in an order that differs
    from build to build, until the batch-structure cache holds it (from the third accumulate of a batch on).  Where a tile is
    what cancellation leaves, another order of a node's paths is another tile, under either role; the roles are compared on
    ONE list."""
    g = torch.Generator().manual_seed(7)
    y = torch.randint(0, C, (len(idx),), generator=g)
    eng = _engine(kind, ei, X, Ws, bs)
    calls = [(idx.cuda(), y.cuda(), len(idx), {"paths": True})]
    for _ in range(2):
        _accumulate(eng, True, calls)
    f0, _, _ = _accumulate(eng, True, calls)
    assert eng.last_kfac_used_paths
    assert np.isfinite(f0).all(), what
    if expect_data:
        assert np.abs(f0).max() > 0, what
    ref64, _, _ = _fp64_kfac_classes(kind, eng, idx.cuda(), y.cuda(), range(C), X, [w.cuda() for w in Ws], [b.cuda() for b in bs])
    ref64 = ref64.cpu().numpy()
    e_f32 = rel(f0, ref64)
    for r in range(REPEATS):
        s0, _, _ = _accumulate(eng, False, calls)
        assert eng.last_kfac_used_paths
        e_role, e_new = rel(s0, f0), rel(s0, ref64)
        print(f"{what} repeat {r}: |B_0| {np.linalg.norm(f0):.3e}, vs fp32 role {e_role:.3e}, vs fp64 {e_new:.3e} (fp32 role {e_f32:.3e})")
        assert np.isfinite(s0).all(), what
        assert e_role <= 2e-6, (what, r)
        if np.linalg.norm(ref64) > 0:
            assert e_new <= max(1e-6, 2 * e_f32 + 1e-7), (what, r)
    eng.check_async_errors()
    eng.close()
    return s0


@gpu
@pytest.mark.parametrize("kind", ["gcn", "sage"])
@pytest.mark.parametrize("log2_scale", [20, -20, 5])
def test_w1_and_the_logits_scaled(kind, log2_scale):
    """W_1 and b_1 times 2^20, 2^-20 and 32: the logits, and every tile value's W_1 factor, scale with them (at 32 the samples'
    seeds spread over many binades).

    At 2^20 the softmax is one-hot in fp32, every sample's seed block is zero and a tile value is what the cancellation
    alpha W_1 - beta b_m leaves of terms of size 2^20: rounding noise.  The launch's bound follows the seed block
    (PathScale's vmax) down to 2^-12 of the terms' size, so the noise still gets fp16 pieces that resolve it."""
    ei, idx = _graph(DENSE)
    _, X, Ws, bs = _make(kind, N, F, 256, 40, 1, L=2, seed=21)
    Ws[1], bs[1] = Ws[1] * 2.0 ** log2_scale, bs[1] * 2.0 ** log2_scale
    _compare(f"{kind} W_1, b_1 x 2^{log2_scale}", kind, ei, idx, X, Ws, bs, 40, expect_data=log2_scale != 20)


@gpu
@pytest.mark.parametrize("log2_scale", [20, -20])
def test_w1_scaled_at_the_same_logits(log2_scale):
    """W_1 times 2^k and the first layer times 2^-k (ReLU is positively homogeneous): the logits, the seeds and the mask stay,
    every tile value scales by 2^k and B_0 by 4^k, exactly -- the relative errors are those of the unscaled model."""
    ei, idx = _graph(DENSE)
    _, X, Ws, bs = _make("gcn", N, F, 256, 40, 1, L=2, seed=22)
    base = _compare("unscaled", "gcn", ei, idx, X, Ws, bs, 40)
    k = 2.0 ** log2_scale
    Ws[0], bs[0], Ws[1] = Ws[0] / k, bs[0] / k, Ws[1] * k
    got = _compare(f"W_1 x 2^{log2_scale}, first layer / 2^{log2_scale}", "gcn", ei, idx, X, Ws, bs, 40)
    assert rel(got / k ** 2, base) <= 2e-6


@gpu
def test_a_few_nodes_far_below_the_launch_s_largest():
    """Ten leaves (242 .. 251) hang on a hub of degree 209 whose only neighbour in the batch is a second hub: each has ONE
    path, of weight 2^-12; four isolated batch nodes, listed four times each, have a path of weight 4.  The leaves' tiles lie
    2^12 and more below the launch's largest (checked on the oracle's tiles) and the Frobenius bounds hold all the same."""
    g = torch.Generator().manual_seed(31)
    B, hub1, hub2 = 240, 240, 241
    leaves, lone = torch.arange(242, 252), torch.arange(252, 256)
    perm = torch.randperm(B, generator=g)
    inb, outb = perm[:43], perm[43:]
    ei = torch.cat([torch.randint(0, B, (2, 1200), generator=g), torch.stack([torch.full((len(outb),), hub1), outb]),
                    torch.stack([torch.full((B,), hub2), torch.arange(B)]), torch.stack([torch.full((10,), hub1), leaves]),
                    torch.tensor([[hub1], [hub2]])], 1)
    idx = torch.cat([inb, torch.tensor([hub2]), lone.repeat(4)])
    _, X, Ws, bs = _make("gcn", N, F, 256, 40, 1, L=2, seed=23)
    m = oracle_from_arrays("gcn", N, ei.numpy(), X.numpy(), [w.numpy() for w in Ws], [b.numpy() for b in bs], True)
    Y, _, _ = _tiles_and_bound("gcn", m, idx.numpy())
    per_node = np.abs(Y).max((1, 2))
    small = per_node[242:252]
    print(f"largest tile value {per_node.max():.3e}; the leaves': {small.max():.3e}")
    assert small.min() > 0 and small.max() <= per_node.max() * 2.0 ** -12
    _compare("small tiles", "gcn", ei, idx, X, Ws, bs, 40)


@gpu
def test_a_zero_scale_gives_zero_factors():
    """W_1 = 0: every tile value, the bound and B_0 are zero (the launch has no scale to run the pieces with)."""
    ei, idx = _graph(DENSE)
    _, X, Ws, bs = _make("gcn", N, F, 256, 40, 1, L=2, seed=24)
    Ws[1] = Ws[1] * 0.0
    eng = _engine("gcn", ei, X, Ws, bs)
    y = torch.randint(0, 40, (M,), generator=torch.Generator().manual_seed(7))
    for f32 in (True, False):
        s0, _, _ = _accumulate(eng, f32, [(idx.cuda(), y.cuda(), M, {"paths": True})])
        assert eng.last_kfac_used_paths
        assert np.array_equal(s0, np.zeros_like(s0))
    eng.check_async_errors()
    eng.close()


@gpu
@pytest.mark.parametrize("kind", ["gcn", "sage"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_non_finite_input_gives_a_non_finite_factor(kind, bad):
    ei, idx = _graph(DENSE)
    _, X, Ws, bs = _make(kind, N, F, 256, 10, 1, L=2, seed=25)
    Ws[1][3, 17] = bad
    eng = _engine(kind, ei, X, Ws, bs)
    y = torch.randint(0, 10, (M,), generator=torch.Generator().manual_seed(7))
    for f32 in (False, True):
        s0, _, _ = _accumulate(eng, f32, [(idx.cuda(), y.cuda(), M, {"paths": True})])
        assert eng.last_kfac_used_paths
        assert not np.isfinite(s0).all(), f"fp32 role: {f32}"
    eng.close()


@gpu
def test_two_identical_calls_agree():
    """the flush is atomic adds in whatever order the workgroups finish: 1e-6 between two runs, as elsewhere in the suite"""
    ei, idx = _graph(DENSE)
    _, X, Ws, bs = _make("gcn", N, F, 256, 40, 1, L=2, seed=26)
    eng = _engine("gcn", ei, X, Ws, bs)
    y = torch.randint(0, 40, (M,), generator=torch.Generator().manual_seed(7))
    calls = [(idx.cuda(), y.cuda(), M, {"paths": True})]
    a, _, _ = _accumulate(eng, False, calls)
    b, _, _ = _accumulate(eng, False, calls)
    assert eng.last_kfac_used_paths
    assert rel(a, b) <= 1e-6
    eng.close()
