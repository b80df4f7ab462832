"""The Gram role of paths_fused_kernel on bf16 MFMAs over a three-piece split of every fp32 tile value (csrc/paths_fused.hip,
gram_split_role) against the fp32 role (LGNN_GRAM_F32=1, read per call), fp64 restatements and the CPU oracle: the headline
shape, a sweep over classes per launch (R), widths, model families and both kernel instances (node list or not), inputs that
span many binades, and non-finite inputs."""
import os

import numpy as np
import pytest
import torch

import gnn_laplace_oracle as O
from gpu_utils import oracle_from_arrays, rel
from test_gpu_scale import _engine, _fp64_kfac_classes, _make

pytestmark = pytest.mark.gpu


def _accumulate(eng, f32, calls):
    """B_0, B_1 and the loss of a run of kfac_accumulate calls (idx, y, n_train, kwargs) under one Gram role"""
    old = os.environ.pop("LGNN_GRAM_F32", None)
    if f32:
        os.environ["LGNN_GRAM_F32"] = "1"
    try:
        _, views, loss = eng.new_kfac_buffers()
        for idx, y, n_train, kw in calls:
            eng.kfac_accumulate(idx, y, n_train, views, loss, **kw)
        torch.cuda.synchronize()
    finally:
        os.environ.pop("LGNN_GRAM_F32", None)
        if old is not None:
            os.environ["LGNN_GRAM_F32"] = old
    return views[0][1].cpu().numpy().astype(np.float64), views[1][1].cpu().numpy().astype(np.float64), float(loss)


def test_headline_batch_split_gram_against_fp64_and_the_fp32_role():
    """One full arxiv-shaped batch of 10 000 (all 40 classes: one launch of the no-list instance at R = 40): the split Gram is no
    further from an fp64 restatement than twice the fp32 role's distance, and within 2e-6 of the fp32 role."""
    import bench
    import laplace_gnn_amd as lg

    w, ei, X, train_idx, train_y = bench.make_workload("arxiv", "cuda")
    torch.manual_seed(0)
    model = lg.GCN(w["F"], w["H"], w["C"], 2, X, ei, symmetric=True).to("cuda").eval()
    eng = model.engine
    M = w["batch"]
    idx, y = train_idx.cuda()[:M].clone(), train_y.cuda()[:M]
    Ws = [c.lin.weight.detach() for c in model.convs]
    bs = [c.lin.bias.detach() for c in model.convs]
    B0, _, _ = _fp64_kfac_classes("gcn", eng, idx, y, range(w["C"]), X, Ws, bs)
    B0 = B0.cpu().numpy()
    calls = [(idx, y, w["n_train"], {})]
    s0, s1, sl = _accumulate(eng, False, calls)
    f0, f1, fl = _accumulate(eng, True, calls)
    assert eng.last_kfac_used_paths
    e_split, e_f32 = rel(s0, B0), rel(f0, B0)
    print(f"headline B_0 vs fp64: split {e_split:.3e}, fp32 role {e_f32:.3e}; split vs fp32 role {rel(s0, f0):.3e}")
    assert e_split <= 2 * e_f32 + 1e-7
    assert rel(s0, f0) <= 2e-6
    assert rel(s1, f1) <= 1e-6 and abs(sl - fl) <= 1e-6 * abs(fl)  # (B_1 and the loss come from other kernels)
    eng.check_async_errors()
    eng.close()


# classes C (a launch takes at most 48: C = 64 is two launches, 48 + 16), width H, model family
SWEEP = [("gcn", 256, 40), ("gcn", 132, 7), ("gcn", 192, 33), ("gcn", 256, 48), ("gcn", 132, 64),
         ("sage", 256, 40), ("sage", 192, 7), ("sage", 132, 48), ("sage", 256, 64), ("sage", 192, 33)]


@pytest.mark.parametrize("kind,H,C", SWEEP)
def test_split_gram_sweep_vs_fp32_role_and_oracle(kind, H, C):
    """Batches of 300 (GCN: the instance without a node list) and of 60 (the node-list instance), and one class range of a
    single class (R = 1): split vs the fp32 role <= 2e-6, vs the CPU oracle <= 1e-4."""
    N, F, E = 3000, 48, 12000
    ei, X, Ws, bs = _make(kind, N, F, H, C, E, L=2, seed=H + C)
    g = torch.Generator().manual_seed(7)
    idx = torch.randperm(N, generator=g)[:360]
    y = torch.randint(0, C, (360,), generator=g)
    eng = _engine(kind, N, ei, X, Ws, bs)
    assert eng.kfac_plan()["paths"]
    calls = [(idx[:300].cuda(), y[:300].cuda(), 360, {}), (idx[300:].cuda(), y[300:].cuda(), 360, {})]
    s0, _, _ = _accumulate(eng, False, calls)
    f0, _, _ = _accumulate(eng, True, calls)
    om = oracle_from_arrays(kind, N, ei.numpy(), X.numpy(), [w.numpy() for w in Ws], [b.numpy() for b in bs], True)
    _, oH = O.fit_kron(om, idx.numpy(), y.numpy(), 300, True)
    print(f"{kind} H={H} C={C}: split vs fp32 role {rel(s0, f0):.3e}, vs oracle {rel(s0, oH[0][0]):.3e}")
    assert rel(s0, f0) <= 2e-6
    assert rel(s0, oH[0][0]) <= 1e-4
    one = [(idx[:300].cuda(), y[:300].cuda(), 360, {"classes": (C // 2, C // 2 + 1)})]
    s0, _, _ = _accumulate(eng, False, one)
    f0, _, _ = _accumulate(eng, True, one)
    assert np.abs(f0).max() > 0
    assert rel(s0, f0) <= 2e-6, "R = 1"
    eng.check_async_errors()
    eng.close()


@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_split_gram_over_thirty_binades_against_fp64(kind):
    """Hidden unit h of the first layer scaled by 2^-15 or 2^15 in turn and W_1's columns of it by the inverse (ReLU is
    positively homogeneous: the logits, the seeds and the ReLU mask stay as they were): column h of every tile is scaled by
    2^15 or 2^-15, so a tile row spans more than 30 binades.  B_0 against an fp64 restatement, in the Frobenius norm and
    entry by entry on the diagonal (sums of squares: no cancellation)."""
    N, F, H, C, E = 3000, 48, 256, 40, 12000
    ei, X, Ws, bs = _make(kind, N, F, H, C, E, L=2, seed=11)
    s = torch.tensor([2.0 ** (15 if h % 2 else -15) for h in range(H)])
    Ws[0] = Ws[0] / s[:, None]
    bs[0] = bs[0] / s
    Ws[1] = Ws[1] * (s.repeat(2) if kind == "sage" else s)[None, :]
    eng = _engine(kind, N, ei, X, Ws, bs)
    g = torch.Generator().manual_seed(8)
    idx = torch.randperm(N, generator=g)[:300].cuda()
    y = torch.randint(0, C, (300,), generator=g).cuda()
    B0, _, _ = _fp64_kfac_classes(kind, eng, idx, y, range(C), X, [w.cuda() for w in Ws], [b.cuda() for b in bs])
    B0 = B0.cpu().numpy()
    calls = [(idx, y, 300, {})]
    s0, _, _ = _accumulate(eng, False, calls)
    f0, _, _ = _accumulate(eng, True, calls)
    d = np.diag(B0)
    ds, df = np.abs(np.diag(s0) - d) / d, np.abs(np.diag(f0) - d) / d
    print(f"{kind} 2^+-15: B_0 vs fp64 split {rel(s0, B0):.3e} (diag max {ds.max():.3e}), "
          f"fp32 role {rel(f0, B0):.3e} (diag max {df.max():.3e})")
    assert rel(s0, B0) <= max(1e-6, 2 * rel(f0, B0) + 1e-7)
    assert ds.max() <= max(1e-6, 2 * df.max() + 1e-7)
    eng.check_async_errors()
    eng.close()


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_input_gives_a_non_finite_factor_under_both_roles(bad):
    N, F, H, C, E = 2000, 32, 256, 10, 8000
    ei, X, Ws, bs = _make("gcn", N, F, H, C, E, L=2, seed=4)
    Ws[1][3, 17] = bad
    eng = _engine("gcn", N, ei, X, Ws, bs)
    g = torch.Generator().manual_seed(9)
    idx = torch.randperm(N, generator=g)[:200].cuda()
    y = torch.randint(0, C, (200,), generator=g).cuda()
    for f32 in (False, True):
        s0, _, _ = _accumulate(eng, f32, [(idx, y, 200, {})])
        assert not np.isfinite(s0).all(), f"fp32 role: {f32}"
    eng.close()
