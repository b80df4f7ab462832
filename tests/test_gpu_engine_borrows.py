"""The engine's borrow rule (``GraphEngine._call``): a copy the engine makes for one enqueue-only call -- a dtype, device or
contiguity copy of an argument -- lives in a local variable until the call has returned and no longer; torch's allocator
hands its block out again in stream order, so work enqueued later may overwrite it and the call's result does not change.

Every entry runs twice on one tiny model (2-layer GCN and 2-layer GraphSAGE, N = 64, F = 8, H = 16, C = 3, M = 20 with a repeated
id): once on arguments already in the library's dtype and layout, held alive by the test, and once on arguments that force
the engine's own copy, with tensors of the copies' sizes allocated and filled with 1e30 right after the call returns and before
any synchronisation.  The two results agree to the suite's 1e-4 relative bar: accumulation-order noise is seven orders below
it, a copy read after its block was overwritten thirty orders above.  A broken rule gives wrong numbers, never a bad address."""
import pytest
import torch

import laplace_gnn_amd as lg
from laplace_gnn_amd._lib import HipLibraryError

pytestmark = pytest.mark.gpu
N, F, H, C, M = 64, 8, 16, 3, 20
BAR = 1e-4


def _engine(kind, widths=(F, H, C)):
    g = torch.Generator().manual_seed(7)
    ei = torch.randint(0, N, (2, 200), generator=g)
    mult = 2 if kind == "sage" else 1
    X = torch.randn(N, F, generator=g).cuda()
    Ws = [(torch.randn(o, mult * i, generator=g) / (mult * i) ** 0.5).cuda() for i, o in zip(widths[:-1], widths[1:])]
    bs = [(0.1 * torch.randn(o, generator=g)).cuda() for o in widths[1:]]
    eng = lg.GraphEngine(ei.cuda(), N, kind=kind, symmetric=True)
    eng.bind(X, Ws, bs)
    return eng


@pytest.fixture(scope="module")
def engines():
    made = {kind: _engine(kind) for kind in ("gcn", "sage")}
    keys = {kind: set(vars(eng)) for kind, eng in made.items()}  # right after ``bind``
    yield made, keys
    for eng in made.values():
        eng.close()


@pytest.fixture(params=["gcn", "sage"])
def eng(request, engines):
    made, keys = engines
    yield made[request.param]
    # after every call of this file: no entry parks a tensor (or anything else) in a new attribute of the engine
    assert set(vars(made[request.param])) == keys[request.param]


@pytest.fixture(scope="module")
def batch():
    g = torch.Generator().manual_seed(11)
    idx = torch.randperm(N, generator=g)[:M]
    idx[-1] = idx[0]  # a repeated id
    return idx.cuda(), torch.randint(0, C, (M,), generator=g).cuda(), torch.randn(M, C, generator=g, dtype=torch.float64).cuda()


def _poison(*shapes):
    """What the next enqueue of a caller may do: take blocks of the copies' sizes and overwrite them."""
    return [torch.full(tuple(s), 1e30, dtype=torch.float32, device="cuda") for s in shapes]


def _close(outs, refs):
    torch.cuda.synchronize()
    assert len(outs) == len(refs)
    for a, b in zip(outs, refs):
        assert bool(torch.isfinite(a).all())
        assert float((a.double() - b.double()).norm()) <= BAR * float(b.double().norm()), (a.shape, a.flatten()[:4], b.flatten()[:4])


def test_regression_diag_accumulate_with_fp64_targets(eng, batch):
    idx, _, t64 = batch
    eng.set_likelihood("regression")
    t32, outs = t64.float(), []
    for t in (t32, t64):
        diag, loss = torch.zeros(eng.n_params, device="cuda"), torch.zeros(1, device="cuda")
        eng.diag_accumulate(idx, t, diag, loss)
        junk = _poison((M, C)) if t is t64 else None
        outs.append((diag, loss))
    _close(*outs[::-1])
    del junk


def test_regression_ef_accumulate_with_fp64_targets(eng, batch):
    idx, _, t64 = batch
    eng.set_likelihood("regression")
    s64 = t64.flip(0).contiguous()  # seed and loss targets differ: two copies in one call
    outs = []
    for seed, t in ((s64.float(), t64.float()), (s64, t64)):
        diag, loss = torch.zeros(eng.n_params, device="cuda"), torch.zeros(1, device="cuda")
        G = eng.ef_accumulate(idx, seed, t, diag=diag, grads=True, loss=loss)
        junk = _poison((M, C), (M, C)) if t is t64 else None
        outs.append((diag, loss, G))
    _close(*outs[::-1])
    del junk


def test_regression_kfac_accumulate_fisher_with_fp64_targets(eng, batch):
    idx, _, t64 = batch
    eng.set_likelihood("regression")
    s64 = t64.flip(0).contiguous()
    outs = []
    for seed, t in ((s64.float(), t64.float()), (s64, t64)):
        flat, views, loss = eng.new_kfac_buffers()
        eng.kfac_accumulate_fisher(idx, seed, t, M, views, loss)
        junk = _poison((M, C), (M, C)) if t is t64 else None
        outs.append((flat,))
    _close(*outs[::-1])
    del junk


def test_adjgrad_batch_with_transposed_gammas(eng, batch):
    idx, y, _ = batch
    eng.set_likelihood("classification")
    g = torch.Generator().manual_seed(3)
    base = [torch.randn(o, o, generator=g).cuda() for _, o in eng.block_dims]
    outs = []
    for gammas in ([b.t().contiguous() for b in base], [b.t() for b in base]):
        grad_P, out_bar = torch.zeros(eng.nnz, device="cuda"), torch.zeros(N, C, device="cuda")
        eng.adjgrad_batch(idx, y, gammas, grad_P, out_bar)
        junk = _poison(*(b.shape for b in base)) if not gammas[0].is_contiguous() else None
        outs.append((grad_P, out_bar))
    _close(*outs[::-1])
    del junk


def test_glm_variance_with_fp64_operands(eng, batch):
    idx = batch[0]
    eng.set_likelihood("classification")
    g = torch.Generator().manual_seed(5)
    (i0, o0), (i1, o1) = eng.block_dims  # diagonal posterior: inverse precisions of (W_0 | b_0), of W_1 and of b_1
    ops64 = {k: (0.5 + torch.rand(*s, generator=g, dtype=torch.float64)).cuda()
             for k, s in (("S0", (o0, i0 + 1)), ("S1", (o1, i1)), ("kappa", (o1,)))}
    outs = []
    for ops in ({k: v.float() for k, v in ops64.items()}, ops64):
        f_mu, f_var = eng.glm_variance(idx, **ops)
        junk = _poison(*(v.shape for v in ops64.values())) if ops is ops64 else None
        outs.append((f_mu, f_var))
    _close(*outs[::-1])
    del junk


def test_sampled_forward_with_fp64_theta(eng, batch):
    idx = batch[0]
    eng.set_likelihood("classification")
    th64 = 0.3 * torch.randn(4, eng.n_params, generator=torch.Generator().manual_seed(9), dtype=torch.float64).cuda()
    outs = []
    for th in (th64.float(), th64):
        out = eng.sampled_forward(idx, th)
        junk = _poison(th64.shape) if th is th64 else None
        outs.append((out,))
    _close(*outs[::-1])
    del junk


def test_no_call_adds_an_attribute_to_the_engine(eng, batch, engines):
    """The fixture's check, spelled out for the calls that used to park their copies in ``_keep``."""
    idx, y, t64 = batch
    eng.set_likelihood("regression")
    eng.diag_accumulate(idx, t64, torch.zeros(eng.n_params, device="cuda"), torch.zeros(1, device="cuda"))
    eng.set_likelihood("classification")
    eng.adjgrad_batch(idx, y, [torch.eye(o, device="cuda") for _, o in eng.block_dims], torch.zeros(eng.nnz, device="cuda"),
                      torch.zeros(N, C, device="cuda"))
    torch.cuda.synchronize()
    assert set(vars(eng)) == engines[1][eng.kind] and not hasattr(eng, "_keep")


def test_a_refused_call_raises_under_the_c_entrys_name(batch):
    deep = _engine("gcn", widths=(F, H, H, C))
    try:
        with pytest.raises(HipLibraryError) as err:
            deep.sampled_forward(batch[0], torch.zeros(2, deep.n_params, device="cuda"))
        assert str(err.value).startswith("lgnn_sampled_forward")
    finally:
        deep.close()
