"""The alpha product of paths_fused_kernel's product waves on v_mfma_f32_16x16x32_bf16 (csrc/paths_fused.hip, PAlpha and
p_mfma_alpha): T1 += (w alpha) Mk of a PAIR of steps as one set of 12 bf16 MFMAs, the fp32 value w alpha cut into
three bf16 pieces by truncation and laid along K beside the 0 / 1 mask.  The product is exact, so the bounds are the ones
tests/test_gpu_split_gram.py holds B_0 of the path route to:

* against the CPU oracle: 1e-4,
* against the fp64 restatement: e <= max(1e-6, 2 e_f32 + 1e-7), e_f32 the fp32 Gram role's distance (LGNN_GRAM_F32=1).

What the change can get wrong is the packing of the K slots, the order of a pair and its two flags (`first`: the pair starts
the node's accumulators; `half`: the pair's second step has no path and its slots must be zero).  So: graphs with prescribed
path counts per node -- "spokes" as in tests/test_gpu_product_chain.py, a destination node joined to middle nodes that are
joined to exactly k batch nodes between them -- for k = 0 .. 17, 63 .. 73, 128, 129 (every combination of the flags, both sides
of the 64-path chunk boundary), recomputed on the CPU and asserted to occur; class counts on either side of every class tile
and both launches of a call with more than 48 classes; the three kinds of width; both kernel instances; GCN and GraphSAGE;
the regression likelihood (the alpha product alone); the seeds without the exact fork; coefficients that span more than 20
binades; the fp32 Gram role.  Shapes of tests/test_gpu_gram16.py: N = 300, F = 8, batches of 60; every comparison is made on
five consecutive accumulates into fresh buffers, and every accumulate asserts that the path route ran.

The fp64 restatement covers the classification likelihood with the exact fork; the regression and fork_exact=False cases
are held to the oracle alone, as in tests/test_gpu_gram16.py."""
import functools

import numpy as np
import pytest
import torch

import gnn_laplace_oracle as O
from gpu_utils import oracle_from_arrays, rel
from test_gpu_gram16 import F, M, N, REPEATS, _engine, _expected_paths_per_node
from test_gpu_product_chain import _path_counts, _steps
from test_gpu_scale import _fp64_kfac_classes, _make
from test_gpu_split_gram import _accumulate

gpu = pytest.mark.gpu

KS_ALL = list(range(18)) + list(range(63, 74)) + [128, 129]  # the kernel instance without a node list
KS_LIST = list(range(18))                                     # the node-list instance: the graph has to stay sparse
PER_MIDDLE = 45  # batch nodes joined to one middle node (the batch has 59 distinct ones)


@functools.lru_cache(maxsize=None)
def _spokes(ks):
    """edge_index, the batch (one id listed twice) and the destination node of every prescribed count.  The batch is the
    first 59 nodes; a destination d with k paths has ceil(k / 45) middle nodes c (edges d - c), and the middle nodes are
    joined to k batch nodes between them, dealt round robin so that the batch nodes' degrees stay even."""
    g = torch.Generator().manual_seed(len(ks))
    batch = torch.arange(M - 1)
    idx = torch.cat([batch[:20], batch[3:4], batch[20:]])
    src, dst, dest = [], [], {}
    nxt, deal = M - 1, 0
    for k in ks:
        d = nxt
        nxt += 1
        dest[k] = d
        left = k
        for _ in range(max(-(-k // PER_MIDDLE), 1)):
            c = nxt
            nxt += 1
            src.append(d)
            dst.append(c)
            take = min(left, PER_MIDDLE)
            for j in range(take):
                src.append(c)
                dst.append(int(batch[(deal + j) % len(batch)]))
            deal += take
            left -= take
    assert nxt <= N
    if ks == tuple(KS_ALL):  # a random background among the batch nodes and the unused ones (none touches a spoke)
        free = torch.cat([batch, torch.arange(nxt, N)])
        bg = free[torch.randint(0, len(free), (2, 200), generator=g)]
        src += bg[0].tolist()
        dst += bg[1].tolist()
    return torch.tensor([src, dst]), idx, dest


def _graph(list_instance):
    return _spokes(tuple(KS_LIST if list_instance else KS_ALL))


@pytest.mark.parametrize("list_instance", [False, True])
def test_the_graphs_hold_the_prescribed_path_counts_and_choose_the_instance(list_instance):
    ei, idx, dest = _graph(list_instance)
    _, cnt, _ = _path_counts(ei, idx)  # (counts of a 3000-node graph whose nodes past N are isolated)
    for k, d in dest.items():
        assert cnt[d] == k, (k, cnt[d])
    assert (cnt[N:] == 0).all()
    # (first, half) of a node's pairs: one step = a first half pair, two = a first full pair, then the later pairs
    steps = {k: _steps(k) for k in dest}
    assert {1, 2, 3, 4}.issubset(set(steps.values()))
    assert any(k > 64 and -(-(k - 64) // 4) % 2 == 1 for k in dest) or list_instance  # a later chunk that ends in a half pair
    assert (_expected_paths_per_node(ei) < 2.5) == list_instance


def test_truncated_pieces_are_exact():
    """The split the kernel uses, restated in numpy: r1 = a - hi(a), r2 = r1 - hi(r1) are exact in fp32, r2 has no low
    half, and the three high halves sum to a -- for every a whose r2 is zero or a normal number."""
    g = np.random.default_rng(0)
    a = (g.standard_normal(1 << 20) * np.exp2(g.integers(-30, 30, 1 << 20))).astype(np.float32)
    hi = lambda x: (x.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    r1 = a - hi(a)
    r2 = r1 - hi(r1)
    assert (r2.view(np.uint32) & np.uint32(0xffff) == 0).all()
    assert (hi(a).astype(np.float64) + hi(r1).astype(np.float64) + r2.astype(np.float64) == a.astype(np.float64)).all()
    assert (r1.astype(np.float64) == a.astype(np.float64) - hi(a).astype(np.float64)).all()


def _run(what, kind, H, C, list_instance, regression=False, fork_exact=True, gram_f32=False, logit_scale=None):
    """One case: the references once (oracle; fp64 restatement and the fp32 Gram role's distance from it), then REPEATS
    accumulates."""
    ei, idx, _ = _graph(list_instance)
    _, X, Ws, bs = _make(kind, N, F, H, C, 1, L=2, seed=H + C)
    if logit_scale is not None:
        Ws[1] = Ws[1] * logit_scale
        bs[1] = bs[1] * logit_scale
    g = torch.Generator().manual_seed(7)
    y = torch.randn(M, C, generator=g) if regression else torch.randint(0, C, (M,), generator=g)
    eng = _engine(kind, ei, X, Ws, bs, regression)
    if logit_scale is not None:
        # the alpha coefficients are products of the samples' class probabilities: their spread within a sample
        p = torch.softmax(eng.forward_all()[idx.cuda()].double(), 1)
        spread = torch.log2(p.max(1).values / p.min(1).values)
        print(f"{what}: log2(p_max / p_min) per sample: median {float(spread.median()):.1f}, max {float(spread.max()):.1f}")
        assert float(spread.median()) > 20
    kw = {"paths": True}
    if not fork_exact:
        kw["fork_exact"] = False
    calls = [(idx.cuda(), y.cuda(), M, kw)]
    lik = "regression" if regression else "classification"
    om = oracle_from_arrays(kind, N, ei.numpy(), X.numpy(), [w.numpy() for w in Ws], [b.numpy() for b in bs], True)
    _, okf = O.kfac_batch(om, idx.numpy(), y.numpy(), M, fork_exact, likelihood=lik)
    # (regression: the oracle applied the interface's sqrt(.5) per factor, the engine returns raw factors)
    oracle = okf[0][0].astype(np.float64) * (np.sqrt(2.0) if regression else 1.0)
    ref64 = e_f32 = None
    if fork_exact and not regression:
        ref64, _, _ = _fp64_kfac_classes(kind, eng, idx.cuda(), y.cuda(), range(C), X, [w.cuda() for w in Ws], [b.cuda() for b in bs])
        ref64 = ref64.cpu().numpy()
        f0, _, _ = _accumulate(eng, True, calls)
        assert eng.last_kfac_used_paths
        e_f32 = rel(f0, ref64)
    for r in range(REPEATS):
        s0, _, _ = _accumulate(eng, gram_f32, calls)
        assert eng.last_kfac_used_paths
        e_or = rel(s0, oracle)
        line = f"{what} repeat {r}: vs oracle {e_or:.3e}"
        if ref64 is not None:
            e_new = rel(s0, ref64)
            line += f", vs fp64 {e_new:.3e} (fp32 Gram role {e_f32:.3e})"
        print(line)
        assert np.isfinite(s0).all() and np.abs(s0).max() > 0, what
        assert e_or <= 1e-4, (what, r)
        if ref64 is not None:
            assert e_new <= max(1e-6, 2 * e_f32 + 1e-7), (what, r)
    eng.check_async_errors()
    eng.close()


# either side of every 16-class tile of the A operand; 49 and 64: a second launch (HI) of 1 / 16 classes
@gpu
@pytest.mark.parametrize("C", [7, 16, 17, 32, 33, 40, 48, 49, 64])
def test_class_counts_over_the_prescribed_path_counts(C):
    _run(f"C={C}", "gcn", 256, C, False)


@gpu
def test_one_class():
    """C = 1: the seed of a one-class softmax is exactly zero, B_0 is a cancellation residue of a few fp32 ulps squared on every
    route (tests/test_gpu_gram16.py holds it to 1e-10): the same here -- an A operand of zeros in 15 of 16 rows."""
    ei, idx, _ = _graph(False)
    _, X, Ws, bs = _make("gcn", N, F, 256, 1, 1, L=2, seed=257)
    y = torch.zeros(M, dtype=torch.int64)
    eng = _engine("gcn", ei, X, Ws, bs)
    calls = [(idx.cuda(), y.cuda(), M, {"paths": True})]
    for r in range(REPEATS):
        s0, _, _ = _accumulate(eng, False, calls)
        assert eng.last_kfac_used_paths
        print(f"C=1 repeat {r}: max |B_0| {np.abs(s0).max():.3e}")
        assert np.isfinite(s0).all() and np.abs(s0).max() < 1e-10
    eng.check_async_errors()
    eng.close()


# a partial column block (132), a product wave without columns (192), the headline width
@gpu
@pytest.mark.parametrize("H", [132, 192, 256])
@pytest.mark.parametrize("list_instance", [False, True])
@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_widths_instances_and_families(kind, list_instance, H):
    _run(f"{kind} H={H} list={list_instance}", kind, H, 40, list_instance)


@gpu
@pytest.mark.parametrize("list_instance", [False, True])
@pytest.mark.parametrize("C", [40, 64])
def test_regression_likelihood_runs_the_alpha_product_alone(C, list_instance):
    """V = sqrt(2) I: no beta / gamma product, a pair is its 12 bf16 MFMAs (C = 64: also in the second launch)."""
    _run(f"regression C={C} list={list_instance}", "gcn", 256, C, list_instance, regression=True)


@gpu
def test_without_the_exact_fork():
    _run("fork_exact=False", "gcn", 256, 40, False, fork_exact=False)


@gpu
def test_coefficients_over_more_than_twenty_binades():
    """Logits scaled by 32: a sample's class probabilities, and with them the coefficients that meet in one K group of the
    alpha MFMAs, span more than 20 binades (asserted on the median sample; a scale of 16 gave a median of 15)."""
    _run("logits x 32", "gcn", 256, 40, False, logit_scale=32.0)


@gpu
def test_under_the_fp32_gram_role():
    """LGNN_GRAM_F32=1 (read per call): the products apart from the bf16 Gram role, at the same bounds."""
    _run("fp32 Gram role", "gcn", 256, 40, False, gram_f32=True)
