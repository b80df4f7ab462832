"""``lgnn_knn`` (csrc/knn.hip) and its fronts ``lg.knn`` / ``knn_graph`` / ``get_knn_graph`` / ``knn_candidates``: the kNN
initial graph of the reference's ``--init_graph knng`` configurations (gnn/utils.py:355-369, gnn/marglik_training.py:407-408).

The yardstick is an fp64 brute force in the difference form, written here.  With u = 2^-24 and tau = 4 (F + 2) u -- the
worst-case rounding of the fp32 difference form, not a measured number:

* tolerant criterion, every row: each returned neighbour j has d64(i, j) <= d64_(k)(i) (1 + tau); ``dist`` ascends and matches
  d64(i, nbr) to relative tau (absolute tau max d64 where d64 is zero); no self index, no repeated index;
* exact criterion, rows in general position (every relative gap between successive fp64 distances up to rank k + 1 exceeds tau):
  the returned indices equal the fp64 order;
* the share of general-position rows is asserted to be at least 0.85 -- a condition on the inputs.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def tau_of(F):
    return 4.0 * (F + 2) * U


def d64_matrix(X32: np.ndarray) -> np.ndarray:
    """fp64 difference form sum_f (x_f - y_f)^2 of the fp32 inputs, all pairs, diagonal +inf."""
    X = torch.tensor(X32, dtype=torch.float64)
    N, F = X.shape
    out = torch.empty(N, N, dtype=torch.float64)
    step = max(1, (1 << 22) // (N * F))  # rows per block: a few MB of differences at a time
    buf = torch.empty(step, N, F, dtype=torch.float64)
    for r in range(0, N, step):
        n = min(step, N - r)
        d = torch.sub(X[r:r + n, None, :], X[None, :, :], out=buf[:n])
        d.mul_(d)
        torch.sum(d, -1, out=out[r:r + n])
    out.fill_diagonal_(float("inf"))
    return out.numpy()


def reference(X32: np.ndarray, k: int, exact_ties: bool = False):
    """(D, order [N, k + 1] by (d64, index), general-position mask [N]).  ``exact_ties``: inputs whose equal fp64 distances
    are equal in fp32 as well (duplicated points, integer coordinates) -- a gap of exactly zero is then decided by the index
    on both sides and does not take a row out of general position."""
    D = d64_matrix(X32)
    N, F = X32.shape
    kk = min(k + 1, N - 1)
    order = np.argsort(D, axis=1, kind="stable")[:, :kk]  # stable: equal d64 keeps the smaller index first
    ds = np.take_along_axis(D, order, axis=1)
    gaps = ds[:, 1:] - ds[:, :-1]
    clear = gaps > tau_of(F) * ds[:, 1:]
    if exact_ties:
        clear |= gaps == 0
    gp = clear.all(axis=1)
    return D, order, gp


def check(X32: np.ndarray, k: int, nbr: np.ndarray, dist: np.ndarray, ref=None, min_share=0.85, rows=None):
    D, order, gp = ref if ref is not None else reference(X32, k)
    N, F = X32.shape
    tau = tau_of(F)
    share = float(gp.mean())
    print(f"N={N} F={F} k={k}: general-position share {share:.4f}")
    assert share >= min_share, share
    assert nbr.shape == (N, k) and dist.shape == (N, k) and nbr.dtype == np.int64 and dist.dtype == np.float32
    sel = np.arange(N) if rows is None else rows
    nb, ds = nbr[sel], dist[sel].astype(np.float64)
    assert ((nb >= 0) & (nb < N)).all()
    assert (nb != sel[:, None]).all(), "self index returned"
    srt = np.sort(nb, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "repeated index"
    d_true = D[sel[:, None], nb]
    dk = np.take_along_axis(D[sel], order[sel][:, k - 1:k], axis=1)
    assert (d_true <= dk * (1 + tau)).all(), "a returned neighbour is farther than the k-th nearest allows"
    assert (ds[:, 1:] >= ds[:, :-1]).all(), "dist is not ascending"
    finite = D[np.isfinite(D)]
    tol = tau * np.where(d_true > 0, d_true, finite.max())
    err = np.abs(ds - d_true)
    print(f"  max |dist - d64| / tol = {float((err / tol).max()):.3f}")
    assert (err <= tol).all()
    g = gp[sel]
    assert np.array_equal(nb[g], order[sel][g][:, :k]), "general-position rows must equal the fp64 order"


def run(X32: np.ndarray, k: int):
    import laplace_gnn_amd as lg

    nbr, dist = lg.knn(torch.tensor(X32).cuda(), k)
    return nbr.cpu().numpy(), dist.cpu().numpy(), lg.knn.last_fallback_rows


def normal(N, F, seed):
    return np.random.default_rng(seed).standard_normal((N, F)).astype(np.float32)


def far_cluster(n, F, seed, sign=1.0):
    return (sign * 100.0 + 1e-2 * np.random.default_rng(seed).standard_normal((n, F))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case1(N, F, k):
    X = normal(N, F, 1000 + N + F)
    X.setflags(write=False)
    return X, reference(X, k)


SHAPES = [(1000, 33, 10), (2500, 128, 10), (1500, 2, 10), (300, 1433, 3)]


# ---- 1. the fast path -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,F,k", SHAPES)
def test_knn_matches_fp64_brute_force_on_the_fast_path(N, F, k):
    """F not a multiple of 4, F = 2, a long K loop (F = 1433), N not a multiple of the 64-row tile (N = 300: a ragged last
    tile), the column-split merge (every shape here has fewer than 1024 row tiles).  The certificate passes on every row.
    The running threshold and the per-tile select act at N >= 1000 (several column tiles per split); at N = 300 every split
    is one tile, and what rejects there is the final cut to the 16 candidates a split hands on."""
    X, ref = case1(N, F, k)
    nbr, dist, nfb = run(X, k)
    print(f"fallback rows: {nfb}")
    check(X, k, nbr, dist, ref)
    assert nfb == 0


# ---- 2. the certificate -----------------------------------------------------------------------------------------------------
def test_knn_gram_cancellation_is_caught_by_the_certificate():
    """Two clusters at +-100 per coordinate with spread 1e-2: n_i ~ 1.6e5 against distances ~ 3e-3 -- the fp32 Gram form
    carries no information about the neighbours, no row can be certified, every row is recomputed by brute force."""
    F, k = 16, 5
    X = np.concatenate([far_cluster(300, F, 21, 1.0), far_cluster(300, F, 22, -1.0)])
    nbr, dist, nfb = run(X, k)
    check(X, k, nbr, dist)
    assert nfb == 600


# ---- 3. fast path and fallback in one call ----------------------------------------------------------------------------------
def test_knn_mixes_certified_rows_and_fallback_rows():
    """The tight cluster's rows are contiguous, so one column split holds all 99 other cluster points of a cluster row, more
    than the 64 it keeps: those rows cannot be certified (n_i ~ 1.6e5), the standard-normal rows can."""
    F, k = 16, 5
    X = np.concatenate([normal(900, F, 31), far_cluster(100, F, 32)])
    nbr, dist, nfb = run(X, k)
    print(f"fallback rows: {nfb}")
    check(X, k, nbr, dist)
    assert 0 < nfb < 1000


# ---- 4. ties ------------------------------------------------------------------------------------------------------------------
def test_knn_orders_exact_ties_by_index():
    """200 points, each duplicated once: the first neighbour is the duplicate at distance exactly 0.  27 points of an integer
    grid (coordinates exact in fp32, so are all their distances): the order there is (d, index), compared for equality.
    Every other point is duplicated too, so ranks come in exactly tied pairs on every row: general position here means that
    each gap is either exactly zero (equal in fp32 as well: identical bits resp. exact integers) or exceeds tau."""
    F, k = 8, 4
    base = normal(200, F, 41)
    grid = np.zeros((27, F), np.float32)
    grid[:, :3] = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(27, 3)
    grid += 50.0
    X = np.concatenate([base, base, grid])
    perm = np.random.default_rng(42).permutation(X.shape[0])
    X = X[perm]
    nbr, dist, nfb = run(X, k)
    ref = reference(X, k, exact_ties=True)
    check(X, k, nbr, dist, ref)
    D, order, _ = ref
    where = np.empty_like(perm)
    where[perm] = np.arange(perm.size)  # where[j]: the row that input point j landed in
    dup = where[(np.arange(400) + 200) % 400]
    rows = where[:400]
    assert np.array_equal(nbr[rows, 0], dup) and (dist[rows, 0] == 0).all()
    g = where[400:]
    assert np.array_equal(nbr[g], order[g][:, :k]), "ties must come out smaller index first"
    assert np.array_equal(dist[g].astype(np.float64), np.take_along_axis(D[g], order[g][:, :k], axis=1))


# ---- 5. small and edge shapes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,F,k", [(5, 3, 4), (65, 1, 32)])
def test_knn_small_shapes(N, F, k):
    """Fewer points than the filter keeps (trivially certified); a single tile resp. one more than a tile."""
    X = normal(N, F, 50 + N)
    nbr, dist, nfb = run(X, k)
    check(X, k, nbr, dist)
    assert nfb == 0


def test_knn_refuses_bad_arguments():
    import ctypes as C

    import laplace_gnn_amd as lg

    X = torch.from_numpy(normal(20, 4, 60)).cuda()
    for k in (0, 33, 20, 25):
        with pytest.raises(lg._lib.HipLibraryError, match="knn: "):
            lg.knn(X, k)
    lib = lg._lib.load()
    nbr = torch.empty(20, 3, dtype=torch.int32, device="cuda")
    dist = torch.empty(20, 3, dtype=torch.float32, device="cuda")
    nfb = C.c_int64(0)
    rc = lib.lgnn_knn(X.data_ptr(), 20, 4, 3, 3, nbr.data_ptr(), dist.data_ptr(), C.byref(nfb),
                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    with pytest.raises(lg._lib.HipLibraryError, match="ld >= F"):
        lg._lib.check(rc, "lgnn_knn")


# ---- 6. determinism and strides -----------------------------------------------------------------------------------------------
def test_knn_is_deterministic_and_takes_strided_rows():
    import laplace_gnn_amd as lg

    X, _ = case1(2500, 128, 10)
    Xd = torch.from_numpy(np.array(X)).cuda()
    a_n, a_d = lg.knn(Xd, 10)
    b_n, b_d = lg.knn(Xd, 10)
    assert torch.equal(a_n, b_n) and torch.equal(a_d.view(torch.int32), b_d.view(torch.int32))
    wide = torch.randn(2500, 135, device="cuda")
    wide[:, 3:131] = Xd
    view = wide[:, 3:131]  # ld = 135 > F, rows not 16-byte aligned
    assert view.stride(0) == 135 and not view.is_contiguous()
    c_n, c_d = lg.knn(view, 10)
    assert torch.equal(a_n, c_n) and torch.equal(a_d.view(torch.int32), c_d.view(torch.int32))


# ---- 7. the fronts ------------------------------------------------------------------------------------------------------------
def _knn_fixture():
    N, F = 60, 8
    X = normal(N, F, 70)
    _, order, gp = reference(X, 6)
    assert gp.all(), "the fixture must be in general position on every row"
    return X, order


def _restated_get_knn_graph(order, k):
    """gnn/utils.py:355-369 on the fp64 neighbours: knn_graph's (neighbour, centre) pairs -> dense adj, (adj + adj^T).bool(),
    diagonal dropped, nonzero() order."""
    N = order.shape[0]
    adj = np.zeros((N, N), bool)
    adj[order[:, :k].reshape(-1), np.repeat(np.arange(N), k)] = True
    adj = adj | adj.T
    np.fill_diagonal(adj, False)
    return np.stack(np.nonzero(adj))


def test_knn_graph_fronts_feed_the_models():
    import laplace_gnn_amd as lg

    X, order = _knn_fixture()
    N, F = X.shape
    Xd = torch.from_numpy(X).cuda()
    pyg = lg.knn_graph(Xd, 3)
    assert np.array_equal(pyg.cpu().numpy(), np.stack([order[:, :3].reshape(-1), np.repeat(np.arange(N), 3)]))
    ei = lg.get_knn_graph(Xd, 3)
    want = _restated_get_knn_graph(order, 3)
    assert ei.dtype == torch.int64 and np.array_equal(ei.cpu().numpy(), want)
    torch.manual_seed(0)
    for sym in (False, True):
        model = lg.GCN(F, 16, 4, 2, torch.from_numpy(X), ei, symmetric=sym).cuda().eval()
        sr, sc = model.engine.export_adj()
        stored = np.unique(np.concatenate([want[0] * N + want[1], np.arange(N) * (N + 1)]))
        assert np.array_equal((sr * N + sc).cpu().numpy(), stored)  # exactly those pairs plus the diagonal
        cand = lg.knn_candidates(model, Xd, 6)
        ci, cj = cand.cpu().numpy()
        assert cand.dtype == torch.int64 and cand.shape[0] == 2 and ci.size > 0
        assert (ci != cj).all() and not np.isin(ci * N + cj, stored).any()
        assert np.unique(ci * N + cj).size == ci.size
        pairs = np.stack([order[:, :6].reshape(-1), np.repeat(np.arange(N), 6)])  # every kNN pair (neighbour, centre)
        if sym:
            assert (ci < cj).all() and not np.isin(cj * N + ci, stored).any()
            lo, hi = np.minimum(*pairs), np.maximum(*pairs)
            covered = np.isin(lo * N + hi, stored) | np.isin(lo * N + hi, ci * N + cj)
        else:
            covered = np.isin(pairs[0] * N + pairs[1], stored) | np.isin(pairs[0] * N + pairs[1], ci * N + cj)
        assert covered.all()
        ste = lg.STEGCN(F, 16, 4, 2, torch.from_numpy(X), ei, symmetric=sym, candidates=cand).cuda().eval()
        tracked = (ste.adj_index[0] * N + ste.adj_index[1]).cpu().numpy()
        assert np.isin(ci * N + cj, tracked).all()
        # plumbing only (the gradient's parity is pinned elsewhere): one value per candidate, finite
        idx = torch.arange(0, N, 2)
        y = torch.randint(0, 4, (idx.numel(),), generator=torch.Generator().manual_seed(1))
        loader = lg.TensorBatchLoader(idx.cuda(), y.cuda(), batch_size=16)
        la = lg.Laplace(model, "classification", subset_of_weights="all", hessian_structure="diag")
        la.fit(loader)
        res = la.neg_marglik_adj_grad(loader, candidates=cand)
        assert res[3].shape == (ci.size,) and bool(torch.isfinite(res[3]).all())
