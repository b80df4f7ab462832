"""LoRASTEGCN without a GPU (gnn/models/models.py:186-235): the maths the device route is pinned to -- the oracle's dense
adjacency gradient (``dense=True``) against its own sparse route and candidate pairs, the LoRA chain rule grad_A = scaling B^T G,
grad_B = scaling G A^T against fp64 autograd -- and the host side: parameter names and shapes, the
Laplace parameter filter, the refusals and the ABI tables of the new entry points."""
import glob
import os
import re

import numpy as np
import pytest
import torch

import gnn_laplace_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LORA_GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "lora", "*.npz")))
NEW_ENTRY_POINTS = ["lgnn_kfac_adjgrad_batch_dense", "lgnn_adjgrad_finish_dense", "lgnn_diag_adjgrad_batch_dense",
                    "lgnn_diag_adjgrad_finish_dense", "lgnn_lora_threshold", "lgnn_lora_grad"]


def _small_oracle(sym, seed=0):
    rng = np.random.default_rng(seed)
    N, F, H, C, E = 48, 7, 9, 4, 120
    ei = rng.integers(0, N, (2, E))
    X = rng.standard_normal((N, F)).astype(np.float32)
    Ws = [0.5 * rng.standard_normal((H, F)).astype(np.float32), 0.5 * rng.standard_normal((C, H)).astype(np.float32)]
    bs = [0.1 * rng.standard_normal(H).astype(np.float32), 0.1 * rng.standard_normal(C).astype(np.float32)]
    rp, col = O.edge_index_to_adj_csr(ei, N, "gcn", sym)
    m = O.GnnModel("gcn", rp, col, X, Ws, bs)
    idx = rng.choice(N, 20, replace=False)
    y = rng.integers(0, C, 20)
    return m, idx, y


def binarise64(g, A, B):
    """The reference's binarisation (models.py:226-230) in fp64: adj0 + (B @ A) * scaling, symmetric average, > threshold,
    diagonal on."""
    s = float(g["lora_alpha"]) / int(g["r"])
    M = g["adj0"].astype(np.float64) + (B.astype(np.float64) @ A.astype(np.float64)) * s
    if bool(g["symmetric"]):
        M = 0.5 * (M + M.T)
    on = M > float(g["threshold"])
    np.fill_diagonal(on, True)
    return on


def oracle_dense_step(g, on):
    """The oracle's dense d(-marglik)/d adj on the graph ``on`` (dense 0/1 with the self loops)."""
    N = int(g["num_nodes"])
    off = on.copy()
    np.fill_diagonal(off, False)
    rp, col = O.edge_index_to_adj_csr(np.stack(off.nonzero()), N, "gcn", False)
    m = O.GnnModel("gcn", rp, col, g["X"], [g["W0"], g["W1"]], [g["b0"], g["b1"]])
    fn = O.kron_marglik_adj_grad if str(g["structure"]) == "kron" else O.diag_marglik_adj_grad
    return fn(m, g["train_idx"], g["train_y"], int(g["batch_size"]), float(g["prior"]), symmetric_param=bool(g["symmetric"]),
              dense=True)


def relerr(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("path", LORA_GOLDEN, ids=[os.path.basename(p)[:-4] for p in LORA_GOLDEN])
def test_lora_loop_goldens_replay_on_the_oracle(path):
    """Three steps of the reference's own LoRASTEGCN loop (tools/make_lora_golden.py): the value, scaling B^T G and
    scaling G A^T with the oracle's dense G on the current graph, the SGD update (no momentum, weight decay) and the edge set."""
    g = np.load(path)
    s = float(g["lora_alpha"]) / int(g["r"])
    lr, wd = float(g["lr"]), float(g["weight_decay"])
    A, B = g["A0"].astype(np.float64), g["B0"].astype(np.float64)
    on = binarise64(g, A, B)
    assert np.array_equal(on, g["edges0"].astype(bool))
    for k in range(g["neg_marglik"].shape[0]):
        val, G = oracle_dense_step(g, on)
        ref = float(g["neg_marglik"][k])
        assert abs(val - ref) <= 2e-5 * abs(ref), k
        gA, gB = s * B.T @ G, s * G @ A.T
        assert relerr(gA, g["grad_A"][k]) <= 1e-4, k
        assert relerr(gB, g["grad_B"][k]) <= 1e-4, k
        A2 = A - lr * (g["grad_A"][k] + wd * A)
        B2 = B - lr * (g["grad_B"][k] + wd * B)
        assert float(np.abs(A2 - g["A_steps"][k]).max()) <= 1e-5, k
        assert float(np.abs(B2 - g["B_steps"][k]).max()) <= 1e-5, k
        A, B = g["A_steps"][k].astype(np.float64), g["B_steps"][k].astype(np.float64)
        on = binarise64(g, A, B)
        assert np.array_equal(on, g["edges_steps"][k].astype(bool)), k


@pytest.mark.parametrize("structure", ["kron", "diag"])
@pytest.mark.parametrize("sym", [True, False])
def test_oracle_dense_gradient_is_the_sparse_one_on_every_pair(structure, sym):
    """The all-pairs gradient that lgnn_*_finish_dense must produce: on the stored entries it is the sparse route's, on
    non-edges the candidate route's (via the sparse form's own formulas), its diagonal is 0 and a symmetric model's is
    symmetric."""
    m, idx, y = _small_oracle(sym)
    fn = O.kron_marglik_adj_grad if structure == "kron" else O.diag_marglik_adj_grad
    v1, rows, cols, g = fn(m, idx, y, 10, 1.0, symmetric_param=sym)
    v2, G = fn(m, idx, y, 10, 1.0, symmetric_param=sym, dense=True)
    assert abs(v1 - v2) <= 1e-12 * abs(v1)
    assert np.allclose(G[rows, cols], g, rtol=1e-9, atol=1e-12)
    assert np.all(np.diag(G) == 0.0)
    if sym:
        assert np.allclose(G, G.T, rtol=0, atol=1e-14)
    N = G.shape[0]
    stored = np.zeros((N, N), dtype=bool)
    stored[rows, cols] = True
    assert np.abs(G[~stored]).max() > 0  # non-edges carry gradient: what LoRA's A, B see


def test_lora_chain_rule():
    """grad_A = scaling B^T G and grad_B = scaling G A^T for M = adj0 + scaling B A (symmetric: (M + M^T) / 2), the STE passing
    G through: autograd of <G, sym(M)> in fp64."""
    rng = np.random.default_rng(3)
    N, r, s = 30, 5, 16.0 / 5
    G = torch.from_numpy(rng.standard_normal((N, N)))
    G = 0.5 * (G + G.T)
    G.fill_diagonal_(0.0)
    A = torch.from_numpy(rng.standard_normal((r, N))).requires_grad_()
    B = torch.from_numpy(rng.standard_normal((N, r))).requires_grad_()
    adj0 = torch.from_numpy((rng.random((N, N)) < 0.1).astype(np.float64))
    M = adj0 + (B @ A) * s
    M = 0.5 * (M + M.T)
    (G * M).sum().backward()
    assert torch.allclose(A.grad, s * B.detach().T @ G, rtol=1e-12, atol=1e-12)
    assert torch.allclose(B.grad, s * G @ A.detach().T, rtol=1e-12, atol=1e-12)


def test_lora_model_host_side():
    import laplace_gnn_amd as lg

    g = torch.Generator().manual_seed(0)
    N, F, H, C = 64, 6, 8, 3
    X = torch.randn(N, F, generator=g)
    ei = torch.randint(0, N, (2, 150), generator=g)
    torch.manual_seed(0)
    m = lg.LoRASTEGCN(F, H, C, 2, X, ei, r=4, lora_alpha=16.0, symmetric=True)
    shapes = {k: (tuple(v.shape), v.requires_grad) for k, v in m.named_parameters()}
    assert shapes["adj_lora_A"] == ((4, N), True) and shapes["adj_lora_B"] == ((N, 4), True)
    assert shapes["adj"][1] is False
    assert m.scaling == 4.0
    plain = lg.GCN(F, H, C, 2, X, ei, symmetric=True)
    n_lora = sum(v.numel() for k, v in m.named_parameters() if v.requires_grad and "adj" not in k and "norms" not in k)
    n_plain = sum(v.numel() for k, v in plain.named_parameters() if v.requires_grad and "adj" not in k)
    assert n_lora == n_plain
    # the driver's weight optimizer (gnn/marglik_training.py:87-92) sees the convs only
    assert all(k.startswith("convs.") for k, _ in m.named_parameters() if "adj" not in k)
    # the base pattern: the given edges as they are (the reference's adj after reset_parameters), CSR consistent with adj_index
    dense = m.full_adj()
    want = torch.zeros(N, N)
    want[ei[0], ei[1]] = 1.0
    assert torch.equal(dense, want)
    rp, col = m.base_rowptr.long(), m.base_col.long()
    assert int(rp[-1]) == m.adj.numel() == m.adj_index.shape[1]
    assert torch.equal(col, m.adj_index[1])
    # A: kaiming_uniform(a=sqrt 5) bound 1/sqrt(N); B: standard normal
    assert float(m.adj_lora_A.detach().abs().max()) <= 1.0 / np.sqrt(N) + 1e-6
    # a reference checkpoint: dense 0/1 adj [N, N] + A + B
    ref = {k: v.clone() for k, v in m.state_dict().items() if k not in ("adj", "adj_index")}
    base = torch.zeros(N, N)
    base[0, 1] = base[1, 0] = base[5, 9] = base[9, 5] = 1.0
    ref["adj"] = base
    ref["adj_lora_A"] = torch.randn(4, N, generator=g)
    m2 = lg.LoRASTEGCN(F, H, C, 2, X, ei, r=4, lora_alpha=16.0, symmetric=True)
    m2.load_state_dict(ref)
    assert torch.equal(m2.full_adj(), base)
    assert torch.equal(m2.adj_lora_A, ref["adj_lora_A"])
    # this module's own checkpoint: the base pattern (and its CSR) come back from adj_index
    m3 = lg.LoRASTEGCN(F, H, C, 2, X, torch.randint(0, N, (2, 40), generator=g), r=4, lora_alpha=16.0, symmetric=True)
    m3.load_state_dict(m2.state_dict())
    assert torch.equal(m3.full_adj(), base)
    assert torch.equal(m3.base_col, m2.base_col) and torch.equal(m3.base_rowptr, m2.base_rowptr)


def test_lora_model_refusals():
    import laplace_gnn_amd as lg

    X = torch.randn(20, 3)
    ei = torch.randint(0, 20, (2, 30))
    with pytest.raises(NotImplementedError):
        lg.LoRASTEGCN(3, 4, 2, 2, X, ei, r=2, lora_alpha=1.0, res=True)
    with pytest.raises(NotImplementedError):
        lg.LoRASTEGCN(3, 4, 2, 2, X, ei, r=2, lora_alpha=1.0, norm="layer")
    with pytest.raises(NotImplementedError):
        lg.LoRASTEGCN(3, 4, 2, 3, X, ei, r=2, lora_alpha=1.0)
    with pytest.raises(ValueError):
        lg.LoRASTEGCN(3, 4, 2, 2, X, ei, r=0, lora_alpha=1.0)


def test_new_entry_points_in_the_abi_tables():
    import laplace_gnn_amd as lg

    with open(os.path.join(ROOT, "include", "laplace_gnn_hip.h")) as f:
        header = set(re.findall(r"LGNN_API\s+[\w\s\*]+?\b(lgnn_[a-z_]+)\s*\(", f.read()))
    for name in NEW_ENTRY_POINTS:
        assert name in header, name
        assert name in lg._lib.SIGNATURES, name
    with open(os.path.join(ROOT, "laplace-gnn_amd", "csrc", "Makefile")) as f:
        assert "lora.hip" in f.read()
