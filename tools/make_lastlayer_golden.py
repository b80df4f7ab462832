"""Goldens of the last-layer Kronecker and diagonal GGN -> tests/golden/lastlayer/*.npz.

Runs only where the reference tree exists (oracle/ref_loader.py loads its files by path; nothing of it is copied, only data
is stored).  The reference has no runnable last-layer path for its GNNs, so the numbers come from its own
curvature code applied to the head alone, on the features its own models produce:

* the input of ``convs[-1].lin`` is taken from the reference's ``GCN`` / ``GraphSAGE`` with a forward hook; per batch sample
  ``Phi = [h | A_bar h]`` rows, ``s = 1`` (GraphSAGE) resp. ``Phi = (A_hat h)`` rows, ``s = rowsum(A_hat)`` with the model's own
  ``forward_adj()`` (GCN), so that the logits are ``Phi W^T + s b``;
* GraphSAGE: ``CurvlinopsGGN.kron`` (laplace/curvature/curvlinops.py:77-108) and ``GGNInterface.diag`` / ``.full``
  (laplace/curvature/curvature.py:374-432) on ``nn.Linear(D, C)`` carrying the head's weights;
* GCN: the same on ``nn.Linear(D + 1, C, bias=False)`` with weight ``[W | b]`` and input ``[Phi | s]`` -- identical logits; ``B``
  comes out directly, ``A`` is the top-left ``D x D`` of its input factor, the diagonal comes out in full, and
  ``sum_n s_n^2 Lambda_n`` is the bias-bias block of ``.full``.

Stored per case: the inputs (``edge_index``, ``X``, weights, ``train_idx``, ``train_y``, ``batch_size``), ``Phi``, ``s``, and per
fit (sums over the loader's batches, ``N = n_train``): ``A``, ``B`` (the fork's seeds), ``Bb`` (GraphSAGE only: the reference's
bias block, equal to ``B``), ``Bb_lambda = sum s^2 Lambda`` (the bias-bias block of ``.full``: what upstream seeds give),
``diag`` (weight row major, then bias) and ``loss``.  An isolated node is a batch sample and one node id is repeated.

    python tools/make_lastlayer_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
OUT = os.path.join(ROOT, "tests", "golden", "lastlayer")

CASES = {
    # name: kind, n, f, n_edges, n_train, batch_size, symmetric, seed   (H = 8, C = 3)
    "ll_gcn_dir_3batch": dict(kind="gcn", n=56, f=5, n_edges=140, n_train=23, batch_size=9, symmetric=False, seed=11),
    "ll_gcn_sym_1batch": dict(kind="gcn", n=48, f=12, n_edges=110, n_train=20, batch_size=10000, symmetric=True, seed=12),
    "ll_sage_dir_1batch": dict(kind="sage", n=52, f=7, n_edges=120, n_train=21, batch_size=10000, symmetric=False, seed=13),
    "ll_sage_sym_3batch": dict(kind="sage", n=64, f=9, n_edges=160, n_train=26, batch_size=10, symmetric=True, seed=14),
}


def make_case(ns, torch, kind, n, f, n_edges, n_train, batch_size, symmetric, seed, h=8, c=3):
    from torch import nn

    from make_golden import reference_dense_adj

    g = torch.Generator().manual_seed(seed)
    hi = n - 1  # the last node is isolated
    ei = torch.randint(0, hi, (2, n_edges), generator=g)
    ei = torch.cat([ei, ei[:, : n_edges // 10], torch.arange(0, hi, 7).repeat(2, 1)], 1)  # duplicates, explicit self loops
    X = torch.randn(n, f, generator=g)
    adj0 = reference_dense_adj(torch, ei, n)
    torch.manual_seed(seed)
    if kind == "gcn":
        model = ns.gnn_models.GCN(f, h, c, 2, X, adj0.clone(), dropout_p=0.5, symmetric=symmetric)
    else:
        model = ns.gnn_models.GraphSAGE(f, h, c, 2, X, adj0.clone(), num_sampled_nodes_per_hop=None, dropout_p=0.5,
                                        symmetric=symmetric)
    model.eval()
    perm = torch.randperm(n - 1, generator=g)
    train_idx = perm[:n_train].clone()
    train_idx[3] = train_idx[5]  # a repeated node id inside one batch
    train_idx[-1] = n - 1        # the isolated node is a batch sample
    train_y = torch.randint(0, c, (n_train,), generator=g)

    head = model.convs[-1].lin
    seen = {}
    hook = head.register_forward_hook(lambda mod, inp, out: seen.__setitem__("in", inp[0].detach().clone()))
    with torch.no_grad():
        logits = model(torch.arange(n))
    hook.remove()
    W, b = head.weight.detach().clone(), head.bias.detach().clone()
    D = W.shape[1]
    with torch.no_grad():
        if kind == "gcn":
            P = model.forward_adj()
            Phi_all, s_all = P @ seen["in"], P.sum(dim=1)
        else:
            Phi_all, s_all = seen["in"], torch.ones(n)
        assert torch.allclose(Phi_all @ W.T + s_all[:, None] * b, logits, atol=1e-5), "f = W phi + s b"
    Phi, s = Phi_all[train_idx], s_all[train_idx]

    if kind == "gcn":  # [W | b] on [Phi | s]: the same logits without a bias
        lin = nn.Linear(D + 1, c, bias=False)
        with torch.no_grad():
            lin.weight.copy_(torch.cat([W, b[:, None]], dim=1))
        inp = torch.cat([Phi, s[:, None]], dim=1)
    else:
        lin = nn.Linear(D, c)
        with torch.no_grad():
            lin.weight.copy_(W)
            lin.bias.copy_(b)
        inp = Phi
    lin.eval()
    with torch.no_grad():
        assert torch.allclose(lin(inp), logits[train_idx], atol=1e-5)

    kron_be = ns.curvature_curvlinops.CurvlinopsGGN(lin, "classification")
    ggn_be = ns.curvature.GGNInterface(lin, "classification")
    A = torch.zeros(D, D)
    B, Bb, Bbl = torch.zeros(c, c), torch.zeros(c, c), torch.zeros(c, c)
    diag = torch.zeros(c * D + c)
    loss = 0.0
    for s0 in range(0, n_train, batch_size):
        xb, yb = inp[s0:s0 + batch_size], train_y[s0:s0 + batch_size]
        l_k, kron = kron_be.kron(xb, yb, N=n_train)
        l_d, dg = ggn_be.diag(xb, yb)
        l_f, full = ggn_be.full(xb, yb)
        assert abs(float(l_k) - float(l_d)) < 1e-4 * abs(float(l_k)) and abs(float(l_k) - float(l_f)) < 1e-4 * abs(float(l_k))
        loss += float(l_k)
        kf = [[t.detach() for t in F] for F in kron.kfacs]
        B += kf[0][0]
        if kind == "gcn":
            assert len(kf) == 1
            A += kf[0][1][:D, :D]
            dgm = dg.detach().view(c, D + 1)
            diag += torch.cat([dgm[:, :D].reshape(-1), dgm[:, D]])
            bias_pos = torch.arange(c) * (D + 1) + D
        else:
            assert len(kf) == 2
            A += kf[0][1]
            Bb += kf[1][0]
            diag += dg.detach()
            bias_pos = c * D + torch.arange(c)
        Bbl += full.detach()[bias_pos][:, bias_pos]
    out = {"kind": kind, "symmetric": symmetric, "num_nodes": n, "num_layers": 2, "batch_size": batch_size,
           "edge_index": ei.numpy(), "X": X.numpy(), "train_idx": train_idx.numpy(), "train_y": train_y.numpy(),
           "Phi": Phi.numpy().astype(np.float32), "s": s.numpy().astype(np.float32),
           "logits": logits[train_idx].numpy().astype(np.float32),
           "A": A.numpy().astype(np.float32), "B": B.numpy().astype(np.float32), "Bb_lambda": Bbl.numpy().astype(np.float32),
           "diag": diag.numpy().astype(np.float32), "loss": np.float64(loss)}
    if kind == "sage":
        out["Bb"] = Bb.numpy().astype(np.float32)
    for l, conv in enumerate(model.convs):
        out[f"W{l}"] = conv.lin.weight.detach().numpy().copy()
        out[f"b{l}"] = conv.lin.bias.detach().numpy().copy()
    return out


def main():
    import torch

    import ref_loader

    ns = ref_loader.load()
    os.makedirs(OUT, exist_ok=True)
    for name, kw in CASES.items():
        out = make_case(ns, torch, **kw)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB  loss={float(out['loss']):.4f}  |A|={np.linalg.norm(out['A']):.4f}  "
              f"|B|={np.linalg.norm(out['B']):.4f}  s in [{out['s'].min():.3f}, {out['s'].max():.3f}]")


if __name__ == "__main__":
    main()
