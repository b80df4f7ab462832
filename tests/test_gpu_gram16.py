"""The Gram role of paths_fused_kernel on v_mfma_f32_16x16x32_bf16 (csrc/paths_fused.hip, gram_split16_role): B_0
of the path route against the fp32 role of the same library (LGNN_GRAM_F32=1, read per call), the CPU oracle and an fp64
restatement, at the bounds tests/test_gpu_split_gram.py holds the bf16 role to:

* against the fp32 role, same inputs: 2e-6,
* against the CPU oracle: 1e-4,
* against the fp64 restatement: e_new <= max(1e-6, 2 e_f32 + 1e-7).

What the role can get wrong is its chunk schedule -- a launch's classes are cut into chunks of 16 tile rows and, where the
number of 8-row chunks is odd, one last chunk of 8 rows that runs on two MFMAs per tile instead of three -- and the one operand
set it refills while the chunk's MFMAs still run.  So: every class count on either side of a chunk boundary, both launches of
a call with more than 48 classes, the three kinds of width, one 8-row group of W_1 at a time, both kernel instances and both
model families.  The Gram waves run up to a node behind the product waves: every comparison is made on five consecutive
accumulates into fresh buffers.  Every accumulate asserts that the path route ran.

Shapes as in tests/test_gpu_top_pairs.py: N = 300, F = 8, batches of 60."""
import functools

import numpy as np
import pytest
import torch

import gnn_laplace_oracle as O
from gpu_utils import oracle_from_arrays, rel
from test_gpu_scale import _fp64_kfac_classes, _make
from test_gpu_split_gram import _accumulate

pytestmark = pytest.mark.gpu

N, F, M = 300, 8, 60
REPEATS = 5
DENSE, SPARSE = 1500, 90  # background edges: the instance without a node list / with one
LEAVES = 40               # (sparse graph) nodes whose only edge goes to a batch node


@functools.lru_cache(maxsize=None)
def _graph(bg_edges):
    """edge_index and the batch (one id listed twice).  The sparse graph's last LEAVES nodes are leaves of batch nodes."""
    g = torch.Generator().manual_seed(bg_edges)
    free = N - LEAVES
    batch = torch.randperm(free, generator=g)[:M - 1]
    idx = torch.cat([batch[:20], batch[3:4], batch[20:]])
    edges = [torch.randint(0, free, (2, bg_edges), generator=g)]
    if bg_edges == SPARSE:
        edges.append(torch.stack([free + torch.arange(LEAVES), batch[:LEAVES]]))
    return torch.cat(edges, 1), idx


def _expected_paths_per_node(ei):
    """what the library's choice of kernel instance goes by (GCN): two-hop paths of the graph / N * M / N"""
    rp, _ = O.edge_index_to_adj_csr(ei.numpy(), N, "gcn", True)
    deg = np.diff(rp).astype(np.float64)
    return float((deg * deg).sum()) / N * M / N


def test_the_two_graphs_fall_on_either_side_of_the_node_list_threshold():
    assert _expected_paths_per_node(_graph(DENSE)[0]) > 2.5
    assert _expected_paths_per_node(_graph(SPARSE)[0]) < 2.5


def _engine(kind, ei, X, Ws, bs, regression=False):
    import laplace_gnn_amd as lg

    eng = lg.GraphEngine(ei.cuda(), N, kind=kind, symmetric=True)
    eng.bind(X.cuda(), [w.cuda() for w in Ws], [b.cuda() for b in bs],
             likelihood="regression" if regression else "classification")
    return eng


def _run(what, kind, H, C, bg_edges, regression=False, w1_rows=None, classes=None, fp64=True):
    """One case: the references once (fp32 role, oracle, fp64 restatement), then REPEATS accumulates under the default role."""
    ei, idx = _graph(bg_edges)
    _, X, Ws, bs = _make(kind, N, F, H, C, 1, L=2, seed=H + C)
    if w1_rows is not None:  # W_1 zero except the rows [w1_rows)
        keep = torch.zeros(C, 1)
        keep[w1_rows[0]:w1_rows[1]] = 1.0
        Ws[1] = Ws[1] * keep
    g = torch.Generator().manual_seed(7)
    y = torch.randn(M, C, generator=g) if regression else torch.randint(0, C, (M,), generator=g)
    eng = _engine(kind, ei, X, Ws, bs, regression)
    kw = {"paths": True}
    if classes is not None:
        kw["classes"] = classes
    calls = [(idx.cuda(), y.cuda(), M, kw)]
    f0, _, _ = _accumulate(eng, True, calls)
    assert eng.last_kfac_used_paths
    assert np.isfinite(f0).all() and np.abs(f0).max() > 0, what
    oracle = ref64 = None
    if classes is None:
        om = oracle_from_arrays(kind, N, ei.numpy(), X.numpy(), [w.numpy() for w in Ws], [b.numpy() for b in bs], True)
        _, okf = O.kfac_batch(om, idx.numpy(), y.numpy(), M, True, likelihood="regression" if regression else "classification")
        # (regression: the oracle applied the interface's sqrt(.5) per factor, the engine returns raw factors)
        oracle = okf[0][0].astype(np.float64) * (np.sqrt(2.0) if regression else 1.0)
        assert rel(f0, oracle) <= 1e-4, what
    if fp64 and not regression:
        cls = range(C) if classes is None else range(*classes)
        ref64, _, _ = _fp64_kfac_classes(kind, eng, idx.cuda(), y.cuda(), cls, X, [w.cuda() for w in Ws], [b.cuda() for b in bs])
        ref64 = ref64.cpu().numpy()
    for r in range(REPEATS):
        s0, _, _ = _accumulate(eng, False, calls)
        assert eng.last_kfac_used_paths
        e_role = rel(s0, f0)
        line = f"{what} repeat {r}: vs fp32 role {e_role:.3e}"
        if oracle is not None:
            line += f", vs oracle {rel(s0, oracle):.3e}"
        if ref64 is not None:
            e_new, e_f32 = rel(s0, ref64), rel(f0, ref64)
            line += f", vs fp64 {e_new:.3e} (fp32 role {e_f32:.3e})"
        print(line)
        assert np.isfinite(s0).all() and np.abs(s0).max() > 0, what
        assert e_role <= 2e-6, (what, r)
        if oracle is not None:
            assert rel(s0, oracle) <= 1e-4, (what, r)
        if ref64 is not None:
            assert e_new <= max(1e-6, 2 * e_f32 + 1e-7), (what, r)
    eng.check_async_errors()
    eng.close()


# ceil(C / 8) = 1 .. 6 chunks of 8 rows, either parity, either side of every boundary; 50 and 64: a second launch of 2 / 16 classes
CLASS_COUNTS = [7, 8, 9, 15, 16, 17, 24, 25, 32, 33, 40, 41, 48, 50, 64]


@pytest.mark.parametrize("C", CLASS_COUNTS)
def test_chunk_schedule_over_class_counts(C):
    _run(f"C={C}", "gcn", 256, C, DENSE)


def test_one_class():
    """C = 1: the seed of a one-class softmax is exactly zero (p = 1), B_0 is zero in exact arithmetic and a cancellation residue
    of a few fp32 ulps squared on every route (tests/test_gpu_top_pairs.py holds both routes to 1e-10 there): the same here,
    under both roles.  The launch of ONE class with data in it is the class range (3, 4) of a 7-class model below."""
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


@pytest.mark.parametrize("classes", [(3, 4), (0, 7), (16, 33), (8, 48)])
def test_class_ranges_of_one_call(classes):
    """launches of 1, 7, 17 and 40 classes that do not start at class 0 (fp32 role and fp64 restatement of the same range)"""
    _run(f"classes={classes}", "gcn", 256, 7 if classes[1] <= 7 else 48, DENSE, classes=classes)


# a partial column block (132), a product wave without columns (192), the headline width
@pytest.mark.parametrize("H", [132, 192, 256])
@pytest.mark.parametrize("bg_edges", [DENSE, SPARSE])
@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_widths_instances_and_families(kind, bg_edges, H):
    _run(f"{kind} H={H} bg={bg_edges}", kind, H, 40, bg_edges)


@pytest.mark.parametrize("C,group", [(48, g) for g in range(6)] + [(40, g) for g in range(5)])
def test_one_row_group_at_a_time(C, group):
    """Regression likelihood: Y = sqrt(2) W_1 (.) T1, so with W_1 zero except the rows of ONE group of 8 classes the tile has that
    8-row chunk alone: a chunk that is dropped, counted twice or taken with the wrong operand form shows in its own case.
    C = 48: six groups in three 16-row chunks; C = 40: the fifth group is the odd last chunk."""
    _run(f"C={C} group {group}", "gcn", 256, C, DENSE, regression=True, w1_rows=(8 * group, 8 * group + 8))
