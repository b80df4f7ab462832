"""CPU tests of the kNN-graph front (laplace-gnn_amd/knn.py): the new entry point is exported and declared consistently, a CPU
tensor is refused, and the index helpers -- PyG's edge order, the reference's symmetrisation (gnn/utils.py:355-369), the
candidate filter -- are exercised on a hand-made neighbour table without the library."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import laplace_gnn_amd as lg

K = importlib.import_module("laplace_gnn_amd.knn")  # (the package attribute `knn` is the function)

# centre -> its two neighbours, in order
NBR = torch.tensor([[1, 2], [0, 2], [1, 3], [2, 4], [3, 2]])


def test_lgnn_knn_is_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "laplace_gnn_hip.h")).read()
    decl = re.search(r"LGNN_API int lgnn_knn\(([^;]*)\);", text)
    assert decl, "lgnn_knn is not declared in the header"
    assert len(decl.group(1).split(",")) == len(lg._lib.SIGNATURES["lgnn_knn"][1]) == 9
    for needle in ("gnn/utils.py:355-369", "marglik_training.py:407-408", "smaller index first", "synchronises"):
        assert needle in text, needle
    lib = lg._lib.load()
    assert hasattr(lib, "lgnn_knn")
    out = subprocess.run(["nm", "-D", "--defined-only", lg._lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T lgnn_knn$", out, re.M)
    for name in ("knn", "knn_graph", "get_knn_graph", "knn_candidates"):
        assert name in lg.__all__ and callable(getattr(lg, name))


def test_knn_refuses_cpu_tensors_and_wrong_dtypes():
    with pytest.raises(lg._lib.HipLibraryError, match="no CPU path"):
        lg.knn(torch.randn(10, 3), 2)
    with pytest.raises(lg._lib.HipLibraryError, match="no CPU path"):
        lg.get_knn_graph(torch.randn(10, 3), 2)
    with pytest.raises(ValueError):
        lg.knn(torch.randn(10), 2)


def test_edge_index_from_nbr_is_pygs_source_to_target_order():
    ei = K.edge_index_from_nbr(NBR)
    assert ei.dtype == torch.int64
    assert ei.tolist() == [[1, 2, 0, 2, 1, 3, 2, 4, 3, 2], [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]]


def test_symmetrize_matches_the_dense_restatement():
    N = 5
    ei = K.edge_index_from_nbr(NBR)
    adj = torch.zeros(N, N)
    adj[ei[0], ei[1]] = 1                      # edge_index_to_adj (gnn/utils.py:325-330)
    adj = (adj + adj.t()).bool().float()       # gnn/utils.py:364
    adj.fill_diagonal_(0)                      # adj_to_edge_index (gnn/utils.py:333-336)
    want = adj.nonzero().t()
    got = K.symmetrize_edge_index(ei, N)
    assert torch.equal(got, want)
    # duplicates and self pairs in the input change nothing
    noisy = torch.cat([ei, ei[:, :3], torch.tensor([[2, 4], [2, 4]])], dim=1)
    assert torch.equal(K.symmetrize_edge_index(noisy, N), want)


@pytest.mark.parametrize("symmetric", [False, True])
def test_pairs_not_stored(symmetric):
    N = 5
    # stored pattern: the path 0-1-2 in both orientations plus the diagonal, row-major sorted
    st = sorted({(0, 1), (1, 0), (1, 2), (2, 1)} | {(i, i) for i in range(N)})
    sr, sc = torch.tensor([a for a, _ in st]), torch.tensor([b for _, b in st])
    pairs = K.edge_index_from_nbr(NBR)  # (neighbour, centre)
    got = K.pairs_not_stored(pairs, sr, sc, N, symmetric)
    listed = set(zip(*pairs.tolist()))
    if symmetric:
        want = sorted({(min(a, b), max(a, b)) for a, b in listed} - set(st))
        assert all(a < b for a, b in zip(*got.tolist()))
    else:
        want = sorted(listed - set(st))
    assert list(zip(*got.tolist())) == want and len(want) > 0
    assert all(a != b for a, b in want)
    # nothing stored at all; an empty pair list
    none = torch.zeros(0, dtype=torch.int64)
    assert K.pairs_not_stored(pairs, none, none, N, symmetric).shape[1] == (6 if symmetric else 10)
    assert K.pairs_not_stored(torch.zeros(2, 0, dtype=torch.int64), sr, sc, N, symmetric).shape == (2, 0)
