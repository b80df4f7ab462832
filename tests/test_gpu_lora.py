"""LoRASTEGCN on the device (gnn/models/models.py:186-235): the all-pairs adjacency gradient (``neg_marglik_adj_grad(...,
dense=True)``, lgnn_*_dense, csrc/lora.hip) against the sparse route's fixtures and the CPU oracle's ``dense=True``, the LoRA
re-threshold (lgnn_lora_threshold) against an fp64 restatement at the Cora shape, lgnn_lora_grad against fp64 torch, and the
model's loop (fit, adj_backward, SGD step, apply_adj) against the oracle's dense gradient step by step."""
import glob
import os

import numpy as np
import pytest
import torch

import gnn_laplace_oracle as O
from conftest import GOLDEN
from gpu_utils import oracle_from_arrays, rel
from test_gpu_frontend import model_from_golden

pytestmark = pytest.mark.gpu
PLAIN_GCN = sorted(p for p in glob.glob(os.path.join(GOLDEN, "*.npz"))
                   if "adjgrad_vals" in np.load(p) and str(np.load(p)["kind"]) == "gcn" and int(np.load(p)["num_layers"]) == 2
                   and not any(k in np.load(p).files and str(np.load(p)[k]) not in ("None", "False", "none") for k in ("res", "norm")))


@pytest.mark.parametrize("structure", ["kron", "diag"])
@pytest.mark.parametrize("path", PLAIN_GCN, ids=[os.path.basename(p)[:-4] for p in PLAIN_GCN])
def test_dense_gradient_equals_the_sparse_route_on_the_fixtures(path, structure):
    """The dense gradient at the stored entries and at the fixture's non-edge pairs equals the reference's adj.grad there
    (the COO route's own fixtures, <= 1e-5), its diagonal is 0 and a symmetric model's is symmetric."""
    import laplace_gnn_amd as lg

    g = np.load(path)
    model = model_from_golden(g)
    loader = lg.TensorBatchLoader(torch.from_numpy(g["train_idx"]).cuda(), torch.from_numpy(g["train_y"]).cuda(),
                                  batch_size=int(g["batch_size"]))
    cls = lg.KronLaplace if structure == "kron" else lg.DiagLaplace
    la = cls(model, "classification", prior_precision=float(g["adjgrad_prior"]))
    la.fit(loader)
    val, G = la.neg_marglik_adj_grad(loader, dense=True)
    G = G.cpu().numpy()
    pre = "adjgrad_" if structure == "kron" else "adjgrad_diag_"
    assert abs(float(val) - float(g[pre + "neg_marglik"])) <= 5e-6 * abs(float(g[pre + "neg_marglik"]))
    assert rel(G[g["adj_nz_row"], g["adj_nz_col"]], g[pre + "vals"]) < 1e-5
    assert rel(G[g["adjgrad_ne_row"], g["adjgrad_ne_col"]], g[pre + "ne_val"]) < 1e-5
    assert float(np.abs(np.diag(G)).max()) == 0.0
    if bool(g["symmetric"]):
        assert np.array_equal(G, G.T)
    # the sparse route is unchanged next to it
    _, _, grad = la.neg_marglik_adj_grad(loader)
    assert rel(grad.cpu().numpy(), g[pre + "vals"]) < 1e-5
    model.engine.check_async_errors()


@pytest.mark.parametrize("structure,sym", [("kron", True), ("kron", False), ("diag", True), ("diag", False)])
def test_dense_gradient_midsize_vs_oracle(structure, sym):
    """N = 1000, two batches, repeated node ids: the device's dense gradient against the oracle's ``dense=True`` (<= 1e-4).
    ``device_bytes()`` counts the dense route's scratch accumulator of the stored entries (fp32 [nnz]), which the engine owns:
    before every buffer was enumerated from its struct, ``lgnn_device_bytes`` left it out (and ``close()`` leaked it).  (The
    route's other buffers grow in the same call -- 3.3 MB at this shape -- so this bound alone held before as well; measured once
    for kron / symmetric: 3 350 276 B against 3 313 256 B with the old lists, the difference nnz * 4 + (2 M + 1) * 4 = 37 020.)"""
    import laplace_gnn_amd as lg

    N, F, H, C, E, M = 1000, 40, 64, 6, 4000, 300
    gen = torch.Generator().manual_seed(21 + sym)
    ei = torch.randint(0, N, (2, E), generator=gen)
    X = torch.randn(N, F, generator=gen)
    torch.manual_seed(3)
    model = lg.GCN(F, H, C, 2, X, ei, symmetric=sym).cuda().eval()
    idx = torch.randint(0, N, (M,), generator=gen)  # (repeats on purpose)
    y = torch.randint(0, C, (M,), generator=gen)
    loader = lg.TensorBatchLoader(idx.cuda(), y.cuda(), batch_size=M // 2)
    cls = lg.KronLaplace if structure == "kron" else lg.DiagLaplace
    la = cls(model, "classification", prior_precision=0.7)
    la.fit(loader)
    before = model.engine.device_bytes()
    val, G = la.neg_marglik_adj_grad(loader, dense=True)
    grown = model.engine.device_bytes() - before
    print(f"dense adjacency gradient: device_bytes grew by {grown} B, nnz * 4 = {model.engine.nnz * 4} B")
    assert grown >= model.engine.nnz * 4
    Ws = [c.lin.weight.detach().cpu().numpy() for c in model.convs]
    bs = [c.lin.bias.detach().cpu().numpy() for c in model.convs]
    om = oracle_from_arrays("gcn", N, ei.numpy(), X.numpy(), Ws, bs, sym)
    if structure == "kron":
        ov, oG = O.kron_marglik_adj_grad(om, idx.numpy(), y.numpy(), M // 2, 0.7, symmetric_param=sym, dense=True)
    else:
        ov, oG = O.diag_marglik_adj_grad(om, idx.numpy(), y.numpy(), M // 2, 0.7, symmetric_param=sym, dense=True)
    assert abs(float(val) - ov) <= 2e-5 * abs(ov)
    assert rel(G.cpu().numpy(), oG) < 1e-4
    model.engine.check_async_errors()


def _effective64(model):
    """fp64 restatement of models.py:226-230 before the threshold (diagonal excluded by the caller)."""
    A = model.adj_lora_A.detach().double().cpu()
    B = model.adj_lora_B.detach().double().cpu()
    M = model.full_adj().double().cpu() + (B @ A) * model.scaling
    return 0.5 * (M + M.T) if model.symmetric else M


@pytest.mark.parametrize("r,alpha,sym", [(1, 1.0, False), (16, 16.0, True), (17, 8.0, False), (64, 64.0, True),
                                         (16, 4000.0, False)])
def test_lora_threshold_at_the_cora_shape(r, alpha, sym):
    """lgnn_lora_threshold on a Cora-shaped graph: the engine's pattern equals the fp64 binarisation except for pairs within
    1e-5 of the threshold; a second apply_adj flips nothing; the large-scaling case flips more than nnz entries."""
    import laplace_gnn_amd as lg

    N, E, F, H, C = 2708, 5278, 32, 16, 7
    gen = torch.Generator().manual_seed(r)
    ei = torch.randint(0, N, (2, E), generator=gen)
    X = torch.randn(N, F, generator=gen)
    torch.manual_seed(r)
    model = lg.LoRASTEGCN(F, H, C, 2, X, ei, r=r, lora_alpha=alpha, symmetric=sym).cuda().eval()
    eng = model.engine
    nnz0 = eng.nnz

    def check():
        eff = _effective64(model)
        want = eff > model.threshold
        want.fill_diagonal_(True)
        near = (eff - model.threshold).abs() < 1e-5
        got = torch.zeros(N, N, dtype=torch.bool)
        sr, sc = eng.export_adj()
        got[sr.cpu(), sc.cpu()] = True
        assert bool(((got != want) & ~near).sum() == 0)

    check()
    assert model.apply_adj() == 0
    with torch.no_grad():  # any state: a new A, B copied in
        model.adj_lora_A.copy_(0.5 * torch.randn(r, N, generator=gen) / r ** 0.5)
        model.adj_lora_B.copy_(torch.randn(N, r, generator=gen))
    n = model.apply_adj()
    assert n > 0
    check()
    assert model.apply_adj() == 0
    if alpha > 1000:
        assert n > nnz0
    eng.check_async_errors()


@pytest.mark.parametrize("N,r", [(300, 1), (1000, 16), (777, 33), (2708, 64)])
def test_lora_grad_against_fp64(N, r):
    """lgnn_lora_grad against fp64 torch, bit-identical on a second call.  Its per-row-tile partials of grad_A belong to the
    engine, so ``device_bytes()`` grows by at least one tile [r, N] fp32 on the first call -- an assertion that fails before
    every buffer was enumerated from its struct: ``lgnn_device_bytes`` left the LoRA scratch out (and ``close()`` leaked it)."""
    import laplace_gnn_amd as lg

    gen = torch.Generator().manual_seed(N + r)
    X = torch.randn(N, 4, generator=gen)
    model = lg.LoRASTEGCN(4, 8, 3, 2, X, torch.randint(0, N, (2, 3 * N), generator=gen), r=r, lora_alpha=2.0 * r).cuda()
    eng = model.engine
    G = torch.randn(N, N, generator=gen)
    A = torch.randn(r, N, generator=gen)
    B = torch.randn(N, r, generator=gen)
    s = 0.37
    before = eng.device_bytes()
    gA, gB = eng.lora_grad(G.cuda(), A.cuda(), B.cuda(), s)
    grown = eng.device_bytes() - before
    print(f"lora_grad: device_bytes grew by {grown} B, r * N * 4 = {r * N * 4} B")
    assert grown >= r * N * 4
    rA = s * (B.double().T @ G.double())
    rB = s * (G.double() @ A.double().T)
    assert rel(gA.cpu().numpy(), rA.numpy()) < 1e-5
    assert rel(gB.cpu().numpy(), rB.numpy()) < 1e-5
    gA2, _ = eng.lora_grad(G.cuda(), A.cuda(), B.cuda(), s)
    assert torch.equal(gA, gA2)  # deterministic reduction


@pytest.mark.parametrize("structure,sym,r", [("kron", True, 4), ("kron", False, 16), ("diag", True, 16), ("diag", False, 4)])
def test_lora_loop_against_the_oracle(structure, sym, r):
    """Three steps of the loop (fit, adj_backward, SGD step, apply_adj): neg_marglik, the A / B gradients (scaling B^T G,
    scaling G A^T with the oracle's dense G on the model's current graph), the SGD update and the binarised edge set."""
    import laplace_gnn_amd as lg

    N, F, H, C, E, M = 64, 12, 16, 4, 160, 40
    gen = torch.Generator().manual_seed(5 + r + sym)
    ei = torch.randint(0, N, (2, E), generator=gen)
    X = torch.randn(N, F, generator=gen)
    torch.manual_seed(11)
    model = lg.LoRASTEGCN(F, H, C, 2, X, ei, r=r, lora_alpha=16.0, symmetric=sym).cuda().eval()
    names = [k for k, _ in model.named_parameters()]
    assert "adj" in names and "adj_lora_A" in names and "adj_lora_B" in names
    idx = torch.randperm(N, generator=gen)[:M]
    y = torch.randint(0, C, (M,), generator=gen)
    loader = lg.TensorBatchLoader(idx.cuda(), y.cuda(), batch_size=20)
    cls = lg.KronLaplace if structure == "kron" else lg.DiagLaplace
    la = cls(model, "classification", prior_precision=1.0)
    plain = lg.GCN(F, H, C, 2, X, ei, symmetric=sym).cuda()
    assert la.n_params == cls(plain, "classification").n_params
    opt = torch.optim.SGD([model.adj_lora_A, model.adj_lora_B], lr=0.05, weight_decay=1e-3)
    Ws = [c.lin.weight.detach().cpu().numpy() for c in model.convs]
    bs = [c.lin.bias.detach().cpu().numpy() for c in model.convs]
    la.fit(loader)
    for k in range(3):
        sr, sc = model.engine.export_adj()
        off = (sr != sc).cpu()
        om = oracle_from_arrays("gcn", N, torch.stack([sr.cpu()[off], sc.cpu()[off]]).numpy(), X.numpy(), Ws, bs, False)
        if structure == "kron":
            ov, oG = O.kron_marglik_adj_grad(om, idx.numpy(), y.numpy(), 20, 1.0, symmetric_param=sym, dense=True)
        else:
            ov, oG = O.diag_marglik_adj_grad(om, idx.numpy(), y.numpy(), 20, 1.0, symmetric_param=sym, dense=True)
        A0 = model.adj_lora_A.detach().double().cpu()
        B0 = model.adj_lora_B.detach().double().cpu()
        opt.zero_grad()
        value = model.adj_backward(la, loader)
        assert abs(float(value) - ov) <= 2e-5 * abs(ov), k
        s = model.scaling
        oGt = torch.from_numpy(oG)
        assert rel(model.adj_lora_A.grad.cpu().numpy(), (s * B0.T @ oGt).numpy()) < 1e-4, k
        assert rel(model.adj_lora_B.grad.cpu().numpy(), (s * oGt @ A0.T).numpy()) < 1e-4, k
        gA = model.adj_lora_A.grad.detach().double().cpu()
        opt.step()
        assert float((model.adj_lora_A.detach().double().cpu() - (A0 - 0.05 * (gA + 1e-3 * A0))).abs().max()) <= 1e-5
        model.apply_adj()
        eff = _effective64(model)
        want = eff > model.threshold
        want.fill_diagonal_(True)
        near = (eff - model.threshold).abs() < 1e-5
        got = model.binarized_adj().cpu() > 0.5
        assert bool(((got != want) & ~near).sum() == 0), k
        assert model.apply_adj() == 0
        la.fit(loader)
    model.engine.check_async_errors()


def test_dense_refusals():
    import laplace_gnn_amd as lg

    gen = torch.Generator().manual_seed(2)
    N = 80
    X = torch.randn(N, 6, generator=gen)
    ei = torch.randint(0, N, (2, 200), generator=gen)
    idx, y = torch.arange(30), torch.randint(0, 3, (30,), generator=gen)
    loader = lg.TensorBatchLoader(idx.cuda(), y.cuda(), batch_size=30)
    sage = lg.GraphSAGE(6, 8, 3, 2, X, ei).cuda().eval()
    la = lg.KronLaplace(sage, "classification")
    la.fit(loader)
    with pytest.raises(NotImplementedError):
        la.neg_marglik_adj_grad(loader, dense=True)
    res = lg.GCN(6, 8, 3, 2, X, ei, res=True).cuda().eval()
    la = lg.DiagLaplace(res, "classification")
    la.fit(loader)
    with pytest.raises(NotImplementedError):
        la.neg_marglik_adj_grad(loader, dense=True)
    N2 = 600  # 4 N^2 bytes above the smallest workspace limit the library accepts (1 MiB)
    gcn = lg.GCN(6, 8, 3, 2, torch.randn(N2, 6, generator=gen), torch.randint(0, N2, (2, 1500), generator=gen)).cuda().eval()
    la = lg.KronLaplace(gcn, "classification")
    la.fit(loader)
    gcn.engine.set_workspace_limit(1 << 20)
    with pytest.raises(NotImplementedError):
        la.neg_marglik_adj_grad(loader, dense=True)
    with pytest.raises(ValueError):
        la.neg_marglik_adj_grad(loader, dense=True, candidates=torch.tensor([[0], [1]]))


LORA_GOLDEN = sorted(glob.glob(os.path.join(GOLDEN, "lora", "*.npz")))


@pytest.mark.parametrize("path", LORA_GOLDEN, ids=[os.path.basename(p)[:-4] for p in LORA_GOLDEN])
def test_lora_loop_matches_the_reference(path):
    """Three steps of the reference's own LoRASTEGCN loop (tests/golden/lora, tools/make_lora_golden.py) on the device: value
    <= 2e-5, adj_lora_A / adj_lora_B grads <= 1e-4, A and B after the SGD step <= 1e-5, the engine's edge set after every
    apply_adj equal to the reference's binarisation."""
    import laplace_gnn_amd as lg

    g = np.load(path)
    N, r, sym = int(g["num_nodes"]), int(g["r"]), bool(g["symmetric"])
    X = torch.from_numpy(g["X"])
    base = torch.from_numpy(g["adj0"]).nonzero().t().contiguous()
    model = lg.LoRASTEGCN(X.shape[1], g["W0"].shape[0], g["W1"].shape[0], 2, X, base, r=r, lora_alpha=float(g["lora_alpha"]),
                          threshold=float(g["threshold"]), symmetric=sym)
    with torch.no_grad():
        for l, conv in enumerate(model.convs):
            conv.lin.weight.copy_(torch.from_numpy(g[f"W{l}"]))
            conv.lin.bias.copy_(torch.from_numpy(g[f"b{l}"]))
        model.adj_lora_A.copy_(torch.from_numpy(g["A0"]))
        model.adj_lora_B.copy_(torch.from_numpy(g["B0"]))
    model = model.cuda().eval()
    assert torch.equal(model.full_adj().cpu(), torch.from_numpy(g["adj0"]).float())

    def edge_set():
        sr, sc = model.engine.export_adj()
        got = torch.zeros(N, N, dtype=torch.uint8)
        got[sr.cpu(), sc.cpu()] = 1
        return got.numpy()

    assert np.array_equal(edge_set(), g["edges0"])
    loader = lg.TensorBatchLoader(torch.from_numpy(g["train_idx"]).cuda(), torch.from_numpy(g["train_y"]).cuda(),
                                  batch_size=int(g["batch_size"]))
    cls = lg.KronLaplace if str(g["structure"]) == "kron" else lg.DiagLaplace
    la = cls(model, "classification", prior_precision=float(g["prior"]))
    opt = torch.optim.SGD([model.adj_lora_A, model.adj_lora_B], lr=float(g["lr"]), weight_decay=float(g["weight_decay"]))
    la.fit(loader)
    for k in range(g["neg_marglik"].shape[0]):
        opt.zero_grad()
        value = model.adj_backward(la, loader)
        ref = float(g["neg_marglik"][k])
        assert abs(float(value) - ref) <= 2e-5 * abs(ref), k
        assert rel(model.adj_lora_A.grad.cpu().numpy(), g["grad_A"][k]) <= 1e-4, k
        assert rel(model.adj_lora_B.grad.cpu().numpy(), g["grad_B"][k]) <= 1e-4, k
        lr, wd = float(g["lr"]), float(g["weight_decay"])
        A0, B0 = model.adj_lora_A.detach().clone(), model.adj_lora_B.detach().clone()
        gA, gB = model.adj_lora_A.grad.detach().clone(), model.adj_lora_B.grad.detach().clone()
        opt.step()
        # the driver's step (no momentum, weight decay) on the device's gradient, and the reference's A, B after it (the
        # gradient's fp32 error times lr is what separates the two: relative <= 1e-5)
        assert float((model.adj_lora_A.detach() - (A0 - lr * (gA + wd * A0))).abs().max()) <= 1e-5, k
        assert float((model.adj_lora_B.detach() - (B0 - lr * (gB + wd * B0))).abs().max()) <= 1e-5, k
        assert rel(model.adj_lora_A.detach().cpu().numpy(), g["A_steps"][k]) <= 1e-5, k
        assert rel(model.adj_lora_B.detach().cpu().numpy(), g["B_steps"][k]) <= 1e-5, k
        with torch.no_grad():  # continue from the reference's A, B (the edge set then compares exactly)
            model.adj_lora_A.copy_(torch.from_numpy(g["A_steps"][k]))
            model.adj_lora_B.copy_(torch.from_numpy(g["B_steps"][k]))
        model.apply_adj()
        assert np.array_equal(edge_set(), g["edges_steps"][k]), k
        assert model.apply_adj() == 0
        la.fit(loader)
    model.engine.check_async_errors()
