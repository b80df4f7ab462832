"""Goldens of the reference's own LoRASTEGCN structure-learning loop -> tests/golden/lora/*.npz.

Runs only where the reference tree exists (oracle/ref_loader.py loads its files by path; nothing of it is copied).  For every
case {kron, diag} x {symmetric, directed}, N = 64, r in {4, 16}: the reference's ``LoRASTEGCN`` (gnn/models/models.py:186-235)
and ``KronLaplace`` / ``DiagLaplace`` run the driver's loop (gnn/marglik_training.py:96-100, 197-224) for three steps --
fit, ``neg_marglik.backward()``, ``SGD([adj_lora_A, adj_lora_B], lr, weight_decay)`` step, refit -- the pattern of
``oracle/make_golden.py::make_structure_loop``.  Stored: the inputs, the weights, the initial A and B, and per step the negative
log marginal likelihood, the A / B gradients, A and B after the step and the binarised edge set (with the self loops).  A seed
is kept only when every effective value stays at least 1e-5 away from the threshold (fp32 summation order cannot flip an edge).

    python tools/make_lora_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
OUT = os.path.join(ROOT, "tests", "golden", "lora")
MIN_MARGIN = 1e-5


def effective(torch, model):
    """What the reference thresholds (models.py:226-229), off-diagonal pairs only."""
    with torch.no_grad():
        m = model.adj + (model.adj_lora_B @ model.adj_lora_A) * model.scaling
        if model.symmetric:
            m = (m + m.T) / 2
    return m


def edges(torch, model):
    on = effective(torch, model) > model.threshold
    on.fill_diagonal_(True)  # fill_diagonal_(1) after the STE (models.py:230)
    return on.numpy().astype(np.uint8)


def margin(torch, model):
    e = (effective(torch, model) - model.threshold).abs()
    e.fill_diagonal_(float("inf"))
    return float(e.min())


def run_case(ns, torch, structure, symmetric, r, seed, n=64, f=12, h=8, c=3, n_edges=150, n_train=33, batch_size=12,
             lora_alpha=16.0, lr=0.05, weight_decay=1e-3, prior=1.0, steps=3):
    from torch.utils.data import DataLoader, TensorDataset

    from make_golden import reference_dense_adj

    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, n_edges), generator=g)
    X = torch.randn(n, f, generator=g)
    adj0 = reference_dense_adj(torch, ei, n)
    perm = torch.randperm(n, generator=g)
    train_idx = perm[:n_train].clone()
    train_idx[3] = train_idx[5]  # a repeated node id
    train_y = torch.randint(0, c, (n_train,), generator=g)
    loader = DataLoader(TensorDataset(train_idx, train_y), batch_size=batch_size, shuffle=False)
    torch.manual_seed(seed)
    model = ns.gnn_models.LoRASTEGCN(f, h, c, 2, X, adj0.clone(), r=r, lora_alpha=lora_alpha, dropout_p=0.5, threshold=0.5,
                                     symmetric=symmetric)
    model.eval()
    out = {"kind": "gcn", "structure": structure, "symmetric": symmetric, "num_nodes": n, "num_layers": 2, "r": r,
           "lora_alpha": np.float64(lora_alpha), "threshold": np.float64(0.5), "lr": np.float64(lr),
           "weight_decay": np.float64(weight_decay), "prior": np.float64(prior), "batch_size": batch_size,
           "edge_index": ei.numpy(), "X": X.numpy(), "train_idx": train_idx.numpy(), "train_y": train_y.numpy(),
           "adj0": adj0.numpy().astype(np.uint8), "A0": model.adj_lora_A.detach().numpy().copy(),
           "B0": model.adj_lora_B.detach().numpy().copy(), "edges0": edges(torch, model)}
    for l, conv in enumerate(model.convs):
        out[f"W{l}"] = conv.lin.weight.detach().numpy().copy()
        out[f"b{l}"] = conv.lin.bias.detach().numpy().copy()
    margins = [margin(torch, model)]
    bl = ns.baselaplace
    cls = bl.KronLaplace if structure == "kron" else bl.DiagLaplace
    lap = cls(model, "classification", prior_precision=prior)
    lap.fit(loader)
    neg = -lap.log_marginal_likelihood()
    opt = torch.optim.SGD([model.adj_lora_A, model.adj_lora_B], lr=lr, weight_decay=weight_decay)  # marglik_training.py:96-100
    negs, gA, gB, As, Bs, Es = [], [], [], [], [], []
    for _ in range(steps):
        opt.zero_grad()
        negs.append(float(neg.detach()))
        neg.backward()
        gA.append(model.adj_lora_A.grad.detach().numpy().copy())
        gB.append(model.adj_lora_B.grad.detach().numpy().copy())
        opt.step()
        As.append(model.adj_lora_A.detach().numpy().copy())
        Bs.append(model.adj_lora_B.detach().numpy().copy())
        Es.append(edges(torch, model))
        margins.append(margin(torch, model))
        for p in model.parameters():  # (the weights are not stepped in this loop; drop what backward left there)
            p.grad = None
        lap.fit(loader)
        neg = -lap.log_marginal_likelihood()
    out.update(neg_marglik=np.array(negs, dtype=np.float64), grad_A=np.stack(gA), grad_B=np.stack(gB), A_steps=np.stack(As),
               B_steps=np.stack(Bs), edges_steps=np.stack(Es), neg_marglik_final=np.float64(float(neg)))
    flips = [int((a != b).sum()) for a, b in zip([out["edges0"]] + Es[:-1], Es)]
    return out, min(margins), flips


def main():
    import torch

    import ref_loader

    ns = ref_loader.load()
    os.makedirs(OUT, exist_ok=True)
    for structure in ("kron", "diag"):
        for symmetric in (True, False):
            for r in (4, 16):
                name = f"lora_{structure}_{'sym' if symmetric else 'dir'}_r{r}"
                for seed in range(100, 140):
                    out, m, flips = run_case(ns, torch, structure, symmetric, r, seed)
                    print(f"{name} seed {seed}: smallest distance from the threshold {m:.2e}")
                    if m >= MIN_MARGIN:
                        break
                else:
                    raise RuntimeError(f"{name}: no seed with margin >= {MIN_MARGIN}")
                out["seed"] = seed
                out["margin"] = np.float64(m)
                path = os.path.join(OUT, name + ".npz")
                np.savez_compressed(path, **out)
                print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB  neg_marglik={list(out['neg_marglik'])}  "
                      f"flips per step={flips}")


if __name__ == "__main__":
    main()
