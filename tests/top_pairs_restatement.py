"""fp64 numpy restatement of the GCN top layer of the two-hop path route, twice: per node, as ``top_tiles_kernel`` sums it
(csrc/toptiles.hip), and from sample pairs, as ``top_pairs_kernel`` does (csrc/toppairs.hip).

    V_m[k, c] = a_c d_kc - b_c u_k - c_c p_k          G_n[c, k] = sum_m w_nm V_m[k, c]
    B_1 = sum_n G_n^T G_n = sum_m s_m V_m V_m^T + sum_{m < m'} q_mm' (V_m V_m'^T + V_m' V_m^T)

with ``s_m = sum_n w_nm^2`` and one pair term ``w_nm w_nm'`` per node the two samples share.  The pair form never builds a
``V``: a term is a diagonal plus four outer products, whose vectors need four dot products over the classes.
"""
import numpy as np

MODES = ("upstream", "fork", "regression")


def sample_tables(mode, idx, logits, cb, ce):
    """the rows (a, b, c) and (u, p) of every batch position as ``path_tables_kernel`` writes them: zero for a repeated id,
    (a, b, c) zero outside the class range [cb, ce).  ``logits`` [N, C] fp64."""
    idx = np.asarray(idx)
    M, C = len(idx), logits.shape[1]
    first = {}
    for m, n in enumerate(idx):
        first.setdefault(int(n), m)
    own = np.array([first[int(n)] == m for m, n in enumerate(idx)])
    f = logits[idx]
    a, b, c, u, p = (np.zeros((M, C)) for _ in range(5))
    if mode == "regression":
        a[:] = np.sqrt(2.0)
    else:
        e = np.exp(f - f.max(1, keepdims=True))
        p = e / e.sum(1, keepdims=True)
        sp = np.sqrt(p)
        if mode == "fork":
            t = f - (p * f).sum(1, keepdims=True)
            a, b, c, u = sp * (1 + 0.5 * t), sp, 0.5 * sp * t, p * (1 + t)
        else:
            a, b, u = sp, sp, p
    keep = np.zeros(C)
    keep[cb:ce] = 1.0
    o = own[:, None].astype(np.float64)
    return {"a": a * keep * o, "b": b * keep * o, "c": c * keep * o, "u": u * o, "p": p * o, "own": own}


def r_rows(P, idx):
    """row n of R = P^T[:, batch]: the pairs (m, w) with m the first position of a batch node and w = P[idx[m], n] times the
    number of times the node is listed (``path_r_kernel``).  ``P`` dense [N, N]."""
    idx = np.asarray(idx)
    N = P.shape[0]
    first, mult = {}, {}
    for m, n in enumerate(idx):
        first.setdefault(int(n), m)
        mult[int(n)] = mult.get(int(n), 0) + 1
    rows = [[] for _ in range(N)]
    for node, m in first.items():
        for n in np.nonzero(P[node])[0]:
            rows[int(n)].append((m, float(P[node, n]) * mult[node]))
    return rows


def _v(tab, m):
    return np.diag(tab["a"][m]) - np.outer(tab["u"][m], tab["b"][m]) - np.outer(tab["p"][m], tab["c"][m])  # [k, c]


def b1_per_node(rows, tab):
    """sum_n G_n^T G_n with G_n formed densely"""
    C = tab["a"].shape[1]
    B = np.zeros((C, C))
    for row in rows:
        if not row:
            continue
        G = sum(w * _v(tab, m).T for m, w in row)  # [c, k]
        B += G.T @ G
    return B


def pair_terms(rows, M):
    """(s [M], the pair triples (m, m', w w')): one triple per node and unordered pair of its entries"""
    s = np.zeros(M)
    pairs = []
    for row in rows:
        for x, (m, w) in enumerate(row):
            s[m] += w * w
            for m2, w2 in row[x + 1:]:
                pairs.append((m, m2, w * w2))
    return s, pairs


def _term(tab, m, m2):
    """V_m V_m'^T as the kernel forms it: the diagonal, then the four K slots (u | X) (p | Y) (a b' | u') (a c' | p')"""
    a, b, c, u, p = (tab[k][m] for k in "abcup")
    a2, b2, c2, u2, p2 = (tab[k][m2] for k in "abcup")
    X = (b @ b2) * u2 + (b @ c2) * p2 - b * a2
    Y = (c @ b2) * u2 + (c @ c2) * p2 - c * a2
    return np.diag(a * a2) + np.outer(u, X) + np.outer(p, Y) - np.outer(a * b2, u2) - np.outer(a * c2, p2)


def b1_pairs(rows, tab):
    """T = sum of weight V V'^T over the sample terms (s_m / 2) and the pair terms; returns T + T^T and the term counts"""
    M, C = tab["a"].shape
    s, pairs = pair_terms(rows, M)
    T = np.zeros((C, C))
    for m in range(M):
        if s[m] != 0.0:
            T += 0.5 * s[m] * _term(tab, m, m)
    for m, m2, w in pairs:
        T += w * _term(tab, m, m2)
    return T + T.T, (int((s != 0).sum()), len(pairs))
