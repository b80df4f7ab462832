"""Helpers shared by the low-rank Laplace tests: the graphs and models of tests/test_gpu_gp.py (a hub row of more than 64
entries, two isolated nodes, duplicate edges), the 60-id train set in two batches and the fp64 reference GGN."""
import functools

import torch

from test_gpu_gp import ODD_SHAPE, SHAPES, batches, edge_model  # noqa: F401

BOUND = 1e-5  # the project's bound for fp32 against fp64, relative to the largest entry
WS_DEFAULT = 32 << 30


def case_id(c):
    k, L, a, s, ext = c
    return f"{k}{L}-{a}-N{s[0]}F{s[1]}H{s[2]}C{s[3]}" + ("-resln" if ext else "")


@functools.lru_cache(maxsize=None)
def train_set(N, C):
    """60 ids in two batches (37 + 23): the hub, both isolated nodes and one repeated id; labels in [0, C)."""
    a, b = batches(N)
    idx = torch.cat([a, b[:23]]).contiguous()
    y = torch.randint(0, C, (60,), generator=torch.Generator().manual_seed(11)).cuda()
    return idx, y


def train_batches(N, C):
    idx, y = train_set(N, C)
    return [(idx[:37].contiguous(), y[:37].contiguous()), (idx[37:].contiguous(), y[37:].contiguous())]


def train_loader(N, C):
    import laplace_gnn_amd as lg

    idx, y = train_set(N, C)
    return lg.TensorBatchLoader(idx, y, batch_size=37)


def ggn64(eng, idx, regression=False):
    """``sum_n J_n^T Lambda_n J_n`` in fp64 from ``engine.jacobians`` (pinned to fp64 by tests/test_gpu_tanh.py), Lambda from
    the fp64 softmax of the logits (regression: the identity)."""
    J, f = eng.jacobians(idx)
    J = J.double()
    if regression:
        return torch.einsum("ncp,ncq->pq", J, J)
    p = torch.softmax(f.double(), dim=-1)
    Lam = torch.diag_embed(p) - p.unsqueeze(2) * p.unsqueeze(1)
    return torch.einsum("ncp,nck,nkq->pq", J, Lam, J)


@functools.lru_cache(maxsize=None)
def H64(case):
    """The fp64 GGN of the case's model over the 60-id train set."""
    eng = edge_model(*case).engine
    N, C = case[3][0], case[3][3]
    return ggn64(eng, train_set(N, C)[0])


def directions(k, P, seed=4):
    return torch.randn(k, P, generator=torch.Generator().manual_seed(seed)).cuda()
