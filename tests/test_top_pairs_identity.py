"""The expansion behind ``top_pairs_kernel`` (csrc/toppairs.hip) against ``sum_n G_n^T G_n`` formed directly, in
fp64 numpy (tests/top_pairs_restatement.py): random tables for C in {1, 7, 40}, the three seed modes, a class sub-range,
repeated ids, and nodes with 0 / 1 / 2 / 5 entries of R.  Agreement to 1e-12."""
import numpy as np
import pytest

from top_pairs_restatement import MODES, b1_pairs, b1_per_node, pair_terms, r_rows, sample_tables

TOL = 1e-12


def _graph(N, M, rng):
    """dense P [N, N] with random weights.  Batch = nodes 0 .. M - 1; node N - 4 + t is joined to exactly (0, 1, 2, 5)[t] batch
    nodes; the batch nodes are joined among themselves at random (and to themselves: self loops)."""
    P = np.zeros((N, N))
    for t, d in enumerate((0, 1, 2, 5)):
        P[rng.permutation(M)[:d], N - 4 + t] = rng.uniform(0.1, 1.0, d)
    for m in range(M):
        P[m, m] = rng.uniform(0.1, 1.0)
        nb = rng.integers(0, N - 4, 3)
        P[m, nb] = rng.uniform(0.1, 1.0, 3)
    return P


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.mark.parametrize("C", [1, 7, 40])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sub", [False, True])
def test_pair_expansion_equals_the_per_node_sum(C, mode, sub):
    rng = np.random.default_rng(100 * C + 10 * MODES.index(mode) + sub)
    N, M = 40, 12
    P = _graph(N, M, rng)
    idx = np.concatenate([np.arange(M), [3, 3, 7]])  # node 3 three times, node 7 twice
    logits = rng.normal(size=(N, C)) * 2.0
    cb, ce = (C // 3, max(C // 3 + 1, (2 * C) // 3)) if sub else (0, C)
    tab = sample_tables(mode, idx, logits, cb, ce)
    rows = r_rows(P, idx)
    counts = [len(rows[N - 4 + t]) for t in range(4)]
    assert counts == [0, 1, 2, 5]
    assert not tab["own"][M:].any() and not any(m >= M for row in rows for m, _ in row)
    direct = b1_per_node(rows, tab)
    got, (n_samples, n_pairs) = b1_pairs(rows, tab)
    assert n_samples == M and n_pairs == sum(len(r) * (len(r) - 1) // 2 for r in rows) and n_pairs >= 11
    if C == 1 and mode != "regression":  # one class: V = 0 up to rounding (p = 1)
        assert np.abs(direct).max() < 1e-20 and np.abs(got).max() < 1e-20
        return
    assert np.abs(direct).max() > 0
    assert _rel(got, direct) < TOL, (C, mode, sub, _rel(got, direct))
    assert np.array_equal(got, got.T)


def test_repeated_ids_live_in_the_weights():
    """a node listed three times: one sample term with nine times the weight, and its pair terms with three times"""
    rng = np.random.default_rng(5)
    N, M = 40, 6
    P = _graph(N, M, rng)
    once, thrice = np.arange(M), np.concatenate([np.arange(M), [2, 2]])
    s1, p1 = pair_terms(r_rows(P, once), M)
    s3, p3 = pair_terms(r_rows(P, thrice), M + 2)
    assert np.allclose(s3[:M], s1 * np.where(np.arange(M) == 2, 9.0, 1.0), rtol=1e-15) and not s3[M:].any()
    assert len(p1) == len(p3)
    for (a, b, w), (a3, b3, w3) in zip(p1, p3):
        assert (a, b) == (a3, b3) and np.isclose(w3, w * (3.0 if 2 in (a, b) else 1.0), rtol=1e-15)
