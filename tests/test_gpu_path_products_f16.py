"""The beta / gamma products of paths_fused_kernel on v_mfma_f32_16x16x32_f16 over two fp16 pieces per operand (csrc/paths_fused.hip,
PCurH; the piece table and the rule that picks the launches: path_bound_kernel in csrc/paths.hip, PathScale in csrc/paths.h).

Without a GPU: numpy restatements of both splits, of the four-slot sum, of the table's row normalisation, and the sweep the
rule's constant comes from (W_1, b_1 x 2^k, k = 0 .. 20, on the GCN model of tests/test_gpu_gram_f16.py's scaled-logits test).

With a GPU: B_0 of the path route against the fp32 role of the same library (LGNN_GRAM_F32=1) and an fp64 restatement, at
the two bounds of tests/test_gpu_gram_f16.py (its ``_compare``: a cached path list, e_role <= 2e-6, e_new <= max(1e-6,
2 e_f32 + 1e-7)), with the product role of every launch asserted.  Shapes, graphs and the runner's parts of
tests/test_gpu_gram16.py (N = 300, F = 8, batches of 60)."""
import functools

import numpy as np
import pytest
import torch

import gnn_laplace_oracle as O
from gpu_utils import oracle_from_arrays, rel
from test_gpu_gram16 import DENSE, SPARSE, M, N, F, REPEATS, _engine, _graph
from test_gpu_gram_f16 import _split
from test_gpu_scale import _fp64_kfac_classes, _make
from test_gpu_split_gram import _accumulate

gpu = pytest.mark.gpu
F32 = np.float32
ROLE_F32, ROLE_GRAM_F16, ROLE_PRODUCTS_F16 = 0, 1, 2  # kRole* of csrc/paths.h
SHARE = {"gcn": 2.0 ** -1, "sage": 2.0 ** -3}  # kPieceShareLog2Gcn / Sage of csrc/paths.h: pieces where min(tri, vmax w1max) >= SHARE tri


# ---- without a GPU --------------------------------------------------------------------------------------------------------
def _pieces(x):
    h0, h1 = _split(x)
    return h0.astype(np.float64), h1.astype(np.float64)


ROW_LOG2 = 6  # kPieceRowLog2 of csrc/paths.h


def _row_scale(t):
    """path_bound_kernel's piece_row: per table row the power of two 2^k with 2^k max_j |t[m, j]| in [2^6, 2^7), k kept in
    [-126, 126]; its inverse, zero for a row of zeros."""
    mx = np.abs(t).max(1).astype(F32)
    eb = (mx.view(np.uint32) >> 23).astype(np.int64)
    k = np.clip(127 + ROW_LOG2 - eb, -126, 126)
    return np.ldexp(F32(1), k).astype(F32), np.where(mx > 0, np.ldexp(F32(1), -k), 0).astype(F32)


def test_both_splits_are_split_pair_s():
    """a' (below 2^10) and b' (a row below 2^7): x - x0 is exact in fp32 and x0 + x1 is x to 2^-22 |x| wherever
    x1 is a normal fp16 (|x| >= 2^-3 is enough), to 2^-25 below."""
    rng = np.random.default_rng(0)
    n = 200000
    mant = rng.uniform(1.0, 2.0, n).astype(F32) * rng.choice([-1.0, 1.0], n).astype(F32)
    a = np.ldexp(mant, rng.integers(-30, 9, n)).astype(F32)
    b = np.ldexp(mant, rng.integers(-30, 6, n)).astype(F32)
    for x in (a, b, F32([0.0, 2.0 ** 10, 2.0 ** 7 - 2.0 ** -17, 2.0 ** -3, 2.0 ** -24])):
        x0, x1 = _pieces(x)
        assert np.isfinite(x0).all() and np.isfinite(x1).all()
        r = x.astype(np.float64) - x0
        assert np.array_equal(r.astype(F32).astype(np.float64), r), "x - x0 is exact in fp32"
        err = np.abs(r - x1)
        big = np.abs(x) >= 2.0 ** -3
        assert (err[big] <= 2.0 ** -22 * np.abs(x[big])).all()
        assert (err <= np.maximum(2.0 ** -22 * np.abs(x), 2.0 ** -25)).all()


def test_the_four_slots_are_the_complete_product():
    """A lane's slots  a0 a0 a1 a1  against  b0 b1 b0 b1  (and likewise gamma): the sum is (a0 + a1)(b0 + b1), every product
    exact in fp32 (11 x 11 bits)."""
    rng = np.random.default_rng(1)
    a = (rng.standard_normal(4096) * 4).astype(F32)
    b = (rng.standard_normal(4096) * 2.0 ** 5).astype(F32)
    a0, a1 = _pieces(a)
    b0, b1 = _pieces(b)
    A, B = np.stack([a0, a0, a1, a1]), np.stack([b0, b1, b0, b1])
    prods = A * B
    assert np.array_equal(prods.astype(F32).astype(np.float64), prods)
    assert np.array_equal(prods.sum(0), (a0 + a1) * (b0 + b1))
    a, b = a.astype(np.float64), b.astype(np.float64)
    da, db = (np.maximum(2.0 ** -22 * np.abs(x), 2.0 ** -25) for x in (a, b))  # (what each split may lose, see above)
    assert (np.abs(prods.sum(0) - a * b) <= np.abs(a) * db + np.abs(b) * da + da * db).all()


# ---- the path sum of one batch, restated: fp64, fp32 products, piece products ---------------------------------------------
def _gcn_paths(m, idx):
    """per destination node the paths (sample, middle node, fp32 weight) of a GCN batch; idx without repeats"""
    PT = m.PT.tocsr()
    pos = {int(n): i for i, n in enumerate(idx)}
    out = []
    for n in range(PT.shape[0]):
        lst = []
        for kk in range(PT.indptr[n], PT.indptr[n + 1]):
            v = PT.indices[kk]
            for k2 in range(PT.indptr[v], PT.indptr[v + 1]):
                if int(PT.indices[k2]) in pos:
                    lst.append((pos[int(PT.indices[k2])], v, F32(F32(PT.data[kk]) * F32(PT.data[k2]))))
        out.append(lst)
    return out


def _tables(kind, m, idx):
    """What the fused kernel reads for one batch, as csrc/paths.hip builds it: per table row t the coefficient rows (alpha,
    -beta, -gamma) [C] and the table rows b_t, g_t [H] (column-normalised), the W_1 operand, the mask rows, and per destination
    node its paths (t, mask row, weight).  GCN: t is the sample.  GraphSAGE (sage_path_tables_kernel): t = 2 m + 1 the neighbour
    path m -> n, t = 2 m the node's own beta / gamma terms on the self half of W_1, t = 2 M + c the own alpha term as a "beta"
    product with a one-hot coefficient row, table row W_1s[c] and path weight alpha_c^m; the mask row is the destination's."""
    out, _, pre = O.forward_all(m)
    C = out.shape[1]
    W1 = m.weights[1].astype(F32)
    al, be, ga, u, p = O.seed_factors(out[idx], True)
    vmax = float(np.abs(O.kfac_seeds(out[idx], True).astype(np.float64)).sum(1).max())
    mask = pre[0] > 0
    Mb = len(idx)
    if kind == "gcn":
        cn = (2.0 ** -np.floor(np.log2(np.abs(W1).max(0)))).astype(F32)
        paths = [[(t, v, w) for t, v, w in lst] for lst in _gcn_paths(m, idx)]
        return dict(cA=al, cB=-be, cG=-ga, b=(u @ W1).astype(F32) * cn, g=(p @ W1).astype(F32) * cn, W1n=W1 * cn,
                    w1max=float(np.abs(W1 * cn).max()), mask=mask, paths=paths, vmax=vmax)
    H = W1.shape[1] // 2
    Ws_, Wn_ = W1[:, :H], W1[:, H:]
    cn = (2.0 ** -np.floor(np.log2(np.maximum(np.abs(Ws_).max(0), np.abs(Wn_).max(0))))).astype(F32)
    T = 2 * Mb + C
    cA, cB, cG = (np.zeros((T, C), F32) for _ in range(3))
    b, g = np.zeros((T, H), F32), np.zeros((T, H), F32)
    cA[1:2 * Mb:2], cB[1:2 * Mb:2], cG[1:2 * Mb:2] = al, -be, -ga
    cB[0:2 * Mb:2], cG[0:2 * Mb:2] = -be, -ga
    b[1:2 * Mb:2], g[1:2 * Mb:2] = (u @ Wn_).astype(F32) * cn, (p @ Wn_).astype(F32) * cn
    b[0:2 * Mb:2], g[0:2 * Mb:2] = (u @ Ws_).astype(F32) * cn, (p @ Ws_).astype(F32) * cn
    cB[2 * Mb:] = np.eye(C, dtype=F32)
    b[2 * Mb:] = Ws_ * cn
    PT = m.PT.tocsr()
    pos = {int(n): i for i, n in enumerate(idx)}
    paths = []
    for n in range(PT.shape[0]):
        lst = [(2 * pos[int(v)] + 1, n, F32(PT.data[k])) for k, v in zip(range(PT.indptr[n], PT.indptr[n + 1]),
                                                                          PT.indices[PT.indptr[n]:PT.indptr[n + 1]]) if int(v) in pos]
        if n in pos:
            mi = pos[n]
            lst.append((2 * mi, n, F32(1)))
            lst += [(2 * Mb + c, n, F32(al[mi, c])) for c in range(C)]
        paths.append(lst)
    return dict(cA=cA, cB=cB, cG=cG, b=b, g=g, W1n=Wn_ * cn, w1max=float(max(np.abs(Ws_ * cn).max(), np.abs(Wn_ * cn).max())),
                mask=mask, paths=paths, vmax=vmax)


def _restate(m, idx, cols=slice(None), kind="gcn"):
    """B_0 (the columns `cols`) of a batch from its path list, the fused kernel's arithmetic restated three ways: fp64
    throughout; the fp32 MFMAs (one rounding per path and term into an fp32 accumulator); the piece products (a step of four
    paths: 32 exact products, one rounding into the accumulator).  The alpha product (exact pieces) and the tile write's FMA
    are the same in the last two; the Gram is taken in fp64 in all three: what differs is the products alone.  Returns the
    launch's scalars, the rule's ratio, the three distances and the fp64 B_0."""
    tb = _tables(kind, m, idx)
    cA, cB, cG, b, g, paths = tb["cA"], tb["cB"], tb["cG"], tb["b"], tb["g"], tb["paths"]
    C = cA.shape[1]
    W1n, mask = tb["W1n"][:, cols], tb["mask"][:, cols]
    amax, w1max, vmax = float(np.abs(cA).max()), tb["w1max"], tb["vmax"]
    bgmax = float((np.abs(cB).max(1) * np.abs(b).max(1) + np.abs(cG).max(1) * np.abs(g).max(1)).max())
    wsum = max(sum(abs(float(w)) for _, _, w in lst) for lst in paths)
    tri, seedb = amax * w1max + bgmax, vmax * w1max
    low = min(tri, seedb)
    res = {"tri": tri, "seedb": seedb, "ratio": low / tri if tri else 0.0, "pieces": low >= SHARE[kind] * tri}
    bound = wsum * (low + 2.0 ** -9 * tri)  # (the sweep restates the pieces whatever the rule says)
    if not (np.isfinite(bound) and 2.0 ** -49 <= bound < 2.0 ** 78):
        return res
    s = F32(2.0 ** (14 - int(np.floor(np.log2(bound)))))
    (ub, db), (ug, dg) = _row_scale(b), _row_scale(g)
    bp, gp = b * ub[:, None], g * ug[:, None]
    assert np.array_equal(bp / ub[:, None], b) and np.array_equal(gp / ug[:, None], g), "the row normalisation is exact"
    assert max(np.abs(bp).max(), np.abs(gp).max()) < 2.0 ** (ROW_LOG2 + 1)
    cbp, cgp = cB * db[:, None], cG * dg[:, None]
    b, g, bp, gp = b[:, cols], g[:, cols], bp[:, cols], gp[:, cols]
    Hc = W1n.shape[1]
    B64, B32, B16 = (np.zeros((Hc, Hc)) for _ in range(3))
    a_top = 0.0
    f8 = lambda x: x.astype(np.float64)
    for lst in paths:
        if not lst:
            continue
        t1, y32, y16, Y64 = np.zeros((C, Hc), F32), np.zeros((C, Hc), F32), np.zeros((C, Hc), F32), np.zeros((C, Hc))
        for s0 in range(0, len(lst), 4):
            acc16 = np.zeros((C, Hc))
            terms = []
            for t, v, w in lst[s0:s0 + 4]:
                ws_, mk = F32(w * s), mask[v].astype(F32)
                t1 = (f8(t1) + f8((ws_ * cA[t]).astype(F32))[:, None] * mk[None, :]).astype(F32)
                terms.append(((ws_ * cB[t]).astype(F32), b[t] * mk, (ws_ * cG[t]).astype(F32), g[t] * mk))
                Y64 += float(ws_) * (f8(cA[t])[:, None] * f8(W1n) + np.outer(f8(cB[t]), f8(b[t])) + np.outer(f8(cG[t]), f8(g[t]))) * mk[None, :]
                for ap, tp in (((ws_ * cbp[t]).astype(F32), bp[t] * mk), ((ws_ * cgp[t]).astype(F32), gp[t] * mk)):
                    a_top = max(a_top, float(np.abs(ap).max()))
                    (x0, x1), (z0, z1) = _pieces(ap), _pieces(tp)
                    acc16 += np.outer(x0, z0) + np.outer(x0, z1) + np.outer(x1, z0) + np.outer(x1, z1)
            for k in (0, 2):  # (a step's four beta MFMA terms, then its four gamma terms)
                for t in terms:
                    y32 = (f8(y32) + np.outer(f8(t[k]), f8(t[k + 1]))).astype(F32)
            y16 = (f8(y16) + acc16).astype(F32)
        Y32 = f8((f8(W1n) * f8(t1) + f8(y32)).astype(F32))
        Y16 = f8((f8(W1n) * f8(t1) + f8(y16)).astype(F32))
        B64 += Y64.T @ Y64
        B32 += Y32.T @ Y32
        B16 += Y16.T @ Y16
    res.update(a_top=a_top, norm=float(np.linalg.norm(B64)), e_role=rel(B16, B32), e_new=rel(B16, B64), e_f32=rel(B32, B64),
               B64=B64 / float(s) ** 2)  # (the fp64 B_0, still with the columns' normalisation)
    return res


def _scaled_model(kind, log2_scale, H=256, C=40, seed=21, col_spread=0):
    """the model of tests/test_gpu_gram_f16.py's scaled-logits test: W_1 and b_1 times 2^k"""
    ei, idx = _graph(DENSE)
    _, X, Ws, bs = _make(kind, N, F, H, C, 1, L=2, seed=seed)
    Ws[1], bs[1] = Ws[1] * 2.0 ** log2_scale, bs[1] * 2.0 ** log2_scale
    if col_spread:
        g = torch.Generator().manual_seed(3)
        Ws[1] = Ws[1] * (2.0 ** torch.randint(-col_spread, col_spread + 1, (Ws[1].shape[1],), generator=g))[None, :]
    return ei, idx, X, Ws, bs


def _oracle(kind, ei, X, Ws, bs):
    return oracle_from_arrays(kind, N, ei.numpy(), X.numpy(), [w.numpy() for w in Ws], [b.numpy() for b in bs], True)


def test_the_row_normalisation_is_exact_and_keeps_the_coefficients_in_range():
    """W_1's columns span 2^24: every table row times its power of two is exact (asserted inside the restatement) and below
    2^7, and the largest weighted, scaled coefficient |a'| = |w s beta 2^-k| stays below 2^9 tri / (min(tri, vmax w1max) +
    2^-9 tri) -- PathScale's argument: 2^10 where the rule lets pieces run -- far from 65504."""
    ei, idx, X, Ws, bs = _scaled_model("gcn", 0, H=132, C=7, seed=5, col_spread=12)
    r = _restate(_oracle("gcn", ei, X, Ws, bs), np.unique(idx.numpy()), cols=slice(0, 32))
    print(f"ratio {r['ratio']:.3g}, largest |a'| {r['a_top']:.3g}, e_role {r['e_role']:.3e}, e_new {r['e_new']:.3e} (fp32 {r['e_f32']:.3e})")
    assert 0 < r["a_top"] <= 2.0 ** (15 - ROW_LOG2) / (r["ratio"] + 2.0 ** -9)
    assert r["ratio"] < SHARE["gcn"] or r["a_top"] < 2.0 ** 10


@functools.lru_cache(maxsize=None)
def _sweep(kind):
    rows = []
    for k in range(21):
        ei, idx, X, Ws, bs = _scaled_model(kind, k)
        r = _restate(_oracle(kind, ei, X, Ws, bs), np.unique(idx.numpy()), cols=slice(0, 32), kind=kind)
        r.pop("B64", None)
        rows.append(r)
    return rows


@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_the_rule_s_constant_is_what_the_sweep_gives(kind):
    """W_1, b_1 x 2^k, k = 0 .. 20, on both models of tests/test_gpu_gram_f16.py's scaled-logits test: the restated B_0 (32 of
    its columns) on pieces against fp64 and against the fp32 restatement, held to a QUARTER of that file's two bounds (the
    margin is for the device's other summation order).  The rule min(tri, vmax w1max) >= 2^-K tri must let pieces run at no k
    that misses them: K is the largest power of two's exponent with 2^-K above every ratio that missed.  GCN: K = 1 (k = 4 ..
    9 sit at ratios 0.39 .. 0.28 while the error -- under either role -- grows, and k = 9 misses: vmax is a maximum over
    samples and does not see how many of them cancel).  GraphSAGE, whose `tri` carries the self half of W_1: the first miss is
    at ratio 0.10, K = 3.  Under the rule |a'| stays below 2^(9 + K)."""
    ok, ratios = [], []
    for k, r in enumerate(_sweep(kind)):
        if "e_role" not in r:
            print(f"{kind} k = {k:2d}: ratio {r['ratio']:.3e} (no usable bound: the fp32 role)")
            ok.append(False), ratios.append(r["ratio"])
            continue
        good = r["e_role"] <= 2e-6 / 4 and r["e_new"] <= max(1e-6, 2 * r["e_f32"] + 1e-7) / 4
        print(f"{kind} k = {k:2d}: ratio {r['ratio']:.3e}, |B_0| {r['norm']:.3e}, e_role {r['e_role']:.3e}, e_new {r['e_new']:.3e}, "
              f"e_f32 {r['e_f32']:.3e}, largest |a'| {r['a_top']:.3g}: {'within' if good else 'OUTSIDE'} a quarter of the bounds")
        ok.append(good), ratios.append(r["ratio"])
        if r["ratio"] >= SHARE[kind]:
            assert r["a_top"] < 2.0 ** 9 / SHARE[kind]
    worst_bad = max(q for q, g in zip(ratios, ok) if not g)
    K = int(np.floor(-np.log2(worst_bad) - 1e-12))  # the largest K with 2^-K above every ratio that missed
    print(f"{kind}: largest ratio outside: {worst_bad:.3f} -> K = {K}")
    assert SHARE[kind] == 2.0 ** -K and K == {"gcn": 1, "sage": 3}[kind]
    assert all(g for q, g in zip(ratios, ok) if q >= SHARE[kind])
    assert sum(q >= SHARE[kind] for q in ratios) >= 3 and sum(q < SHARE[kind] for q in ratios) >= 3  # (both sides are populated)


def test_the_graphsage_restatement_is_the_oracle_s_b0():
    """the path tables of _tables restate what the oracle's backward pass gives (fp64 against the oracle's fp32: 1e-6)"""
    for kind in ("gcn", "sage"):
        ei, idx, X, Ws, bs = _scaled_model(kind, 0, H=132, C=7, seed=5)
        m, ids = _oracle(kind, ei, X, Ws, bs), np.unique(idx.numpy())
        r, tb = _restate(m, ids, kind=kind), _tables(kind, m, ids)
        H = tb["W1n"].shape[1]
        cn = tb["W1n"][0] / (m.weights[1][0, :H] if kind == "gcn" else m.weights[1][0, H:])
        _, okf = O.kfac_batch(m, ids, np.zeros(len(ids), np.int64), len(ids), True)
        assert rel(r["B64"] / np.outer(cn, cn), okf[0][0].astype(np.float64)) <= 1e-6


# ---- with a GPU -----------------------------------------------------------------------------------------------------------
def _role(eng):
    from laplace_gnn_amd import _lib

    return _lib.last_paths_product_role(eng._h)


def _compare(what, kind, ei, idx, X, Ws, bs, C, want_role=ROLE_PRODUCTS_F16, classes=None):
    """tests/test_gpu_gram_f16.py's _compare (two accumulates thrown away: the roles are compared on ONE cached path list) with
    the product role of every launch asserted.  Returns the last B_0."""
    g = torch.Generator().manual_seed(7)
    y = torch.randint(0, C, (len(idx),), generator=g)
    eng = _engine(kind, ei, X, Ws, bs)
    kw = {"paths": True}
    if classes is not None:
        kw["classes"] = classes
    calls = [(idx.cuda(), y.cuda(), len(idx), kw)]
    for _ in range(2):
        _accumulate(eng, True, calls)
    f0, _, _ = _accumulate(eng, True, calls)
    assert eng.last_kfac_used_paths and _role(eng)[0] == ROLE_F32
    assert np.isfinite(f0).all() and np.abs(f0).max() > 0, what
    cls = range(C) if classes is None else range(*classes)
    ref64, _, _ = _fp64_kfac_classes(kind, eng, idx.cuda(), y.cuda(), cls, X, [w.cuda() for w in Ws], [b.cuda() for b in bs])
    ref64 = ref64.cpu().numpy()
    e_f32 = rel(f0, ref64)
    for r in range(REPEATS):
        s0, _, _ = _accumulate(eng, False, calls)
        role, sc = _role(eng)
        e_role, e_new = rel(s0, f0), rel(s0, ref64)
        print(f"{what} repeat {r}: role {role}, vs fp32 role {e_role:.3e}, vs fp64 {e_new:.3e} (fp32 role {e_f32:.3e})")
        assert eng.last_kfac_used_paths and role == want_role, (what, r, role, sc)
        assert np.isfinite(s0).all(), what
        assert e_role <= 2e-6, (what, r)
        assert e_new <= max(1e-6, 2 * e_f32 + 1e-7), (what, r)
    eng.check_async_errors()
    eng.close()
    return s0


@gpu
@pytest.mark.parametrize("C", [7, 16, 17, 40, 48, 49])
def test_class_counts(C):
    """one to three class tiles, either side of a tile boundary; 49: the second launch runs the HI form on one class"""
    ei, idx = _graph(DENSE)
    _, X, Ws, bs = _make("gcn", N, F, 256, C, 1, L=2, seed=256 + C)
    _compare(f"C={C}", "gcn", ei, idx, X, Ws, bs, C)


@gpu
@pytest.mark.parametrize("H", [132, 192, 256])
@pytest.mark.parametrize("bg_edges", [DENSE, SPARSE])
@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_widths_instances_and_families(kind, bg_edges, H):
    """Every case runs the pieces, GraphSAGE's (the self half of W_1 as table rows, the one-hot alpha paths) included; the role
    the rule names, restated here from the launch's scalars, is the one that ran."""
    ei, idx = _graph(bg_edges)
    _, X, Ws, bs = _make(kind, N, F, H, 40, 1, L=2, seed=H + 40)
    eng = _engine(kind, ei, X, Ws, bs)
    y = torch.randint(0, 40, (M,), generator=torch.Generator().manual_seed(7))
    _accumulate(eng, False, [(idx.cuda(), y.cuda(), M, {"paths": True})])
    role, sc = _role(eng)
    eng.close()
    tri = sc["amax"] * sc["w1max"] + sc["bgmax"]
    assert min(tri, sc["vmax"] * sc["w1max"]) >= SHARE[kind] * tri, sc
    assert role == ROLE_PRODUCTS_F16, sc
    _compare(f"{kind} H={H} bg={bg_edges}", kind, ei, idx, X, Ws, bs, 40)


PATH_COUNTS = [1, 4, 5, 8, 9, 65]
BATCH = 70


def _relay_graph():
    """Destination node 100 + i hangs on a relay node 200 + i of its own, and the relay on PATH_COUNTS[i] of the BATCH batch
    nodes 0 .. 69: with self loops the two-hop paths n <- v <- m of the destination node are those through its relay, one per
    batch neighbour of the relay -- exactly PATH_COUNTS[i]."""
    src, dst = [], []
    for i, c in enumerate(PATH_COUNTS):
        src.append(100 + i), dst.append(200 + i)
        for j in range(c):
            src.append(200 + i), dst.append((7 * i + j) % BATCH)
    return torch.tensor([src, dst]), torch.arange(BATCH)


def test_the_relay_graph_has_nodes_with_the_path_counts():
    ei, idx = _relay_graph()
    _, X, Ws, bs = _make("gcn", N, F, 256, 40, 1, L=2, seed=77)
    paths = _gcn_paths(_oracle("gcn", ei, X, Ws, bs), idx.numpy())
    assert [len(paths[100 + i]) for i in range(len(PATH_COUNTS))] == PATH_COUNTS


@gpu
def test_nodes_with_1_4_5_8_9_and_65_paths():
    """the `half` pair (1 and 4 paths), a second step (5), a pair boundary (8 | 9), a second chunk (65)"""
    ei, idx = _relay_graph()
    _, X, Ws, bs = _make("gcn", N, F, 256, 40, 1, L=2, seed=77)
    _compare("path counts", "gcn", ei, idx, X, Ws, bs, 40)


@gpu
@pytest.mark.parametrize("kind,k_pieces,k_fp32", [("gcn", 3, 4), ("sage", 10, 11)])
def test_the_role_flips_across_the_rule_s_threshold(kind, k_pieces, k_fp32):
    """either side of the family's share in the sweep: GCN k = 3 (ratio 0.79) | k = 4 (0.39), GraphSAGE k = 10 (0.24) | k = 11 (0.07)"""
    for k, want in ((k_pieces, ROLE_PRODUCTS_F16), (k_fp32, ROLE_GRAM_F16)):
        ei, idx, X, Ws, bs = _scaled_model(kind, k)
        _compare(f"{kind} W_1, b_1 x 2^{k}", kind, ei, idx, X, Ws, bs, 40, want_role=want)


@gpu
def test_a_zero_w1_gives_exact_zeros_and_a_nan_a_non_finite_factor():
    ei, idx = _graph(DENSE)
    y = torch.randint(0, 40, (M,), generator=torch.Generator().manual_seed(7))
    for bad in (0.0, float("nan")):
        _, X, Ws, bs = _make("gcn", N, F, 256, 40, 1, L=2, seed=24)
        if bad == 0.0:
            Ws[1] = Ws[1] * 0.0
        else:
            Ws[1][3, 17] = bad
        eng = _engine("gcn", ei, X, Ws, bs)
        s0, _, _ = _accumulate(eng, False, [(idx.cuda(), y.cuda(), M, {"paths": True})])
        assert eng.last_kfac_used_paths and _role(eng)[0] == ROLE_F32  # (no usable bound: fp32 throughout)
        if bad == 0.0:
            assert np.array_equal(s0, np.zeros_like(s0))
        else:
            assert not np.isfinite(s0).all()
        eng.close()
