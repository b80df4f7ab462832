"""Goldens of the reference's own one-layer STE-GCN (the Banana block of gnn/configs/original/stegcn_config.yaml:108-127:
``num_layers: 1``) -> tests/golden/onelayer/*.npz.

Runs only where the reference tree exists (oracle/ref_loader.py loads its files by path; nothing of it is copied, only data
is stored).  Two families:

* gradient cases ``one1_*``: the reference's ``STEGCN(f, h, c, 1, ...)`` (gnn/models/models.py:65-118) under ``DiagLaplace``,
  ``KronLaplace`` and ``FullLaplace`` (``GGNInterface`` backend), prior precision 0.7: ``-log_marginal_likelihood()``,
  ``adj.grad`` after ``neg_marglik.backward()`` on the stored entries of the 0/1 adjacency and on 200 non-edges, and the
  fitted ``H`` / Kronecker factors.  Graphs with duplicate edges, explicit self loops and an isolated node; one batch and
  three ragged batches with a repeated node id.
* loop cases ``steloop1_*``: three hyper-steps in the pattern of ``oracle/make_golden.py::make_structure_loop`` with
  ``num_layers=1``.  A seed is kept only when every effective adjacency value stays at least 1e-5 away from the threshold
  after each step (fp32 summation order cannot flip an edge).

    python tools/make_onelayer_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
OUT = os.path.join(ROOT, "tests", "golden", "onelayer")
MIN_MARGIN = 1e-5
PRIOR = 0.7

GRAD_CASES = {
    # name: n, f, c, n_edges, n_train, batch_size, symmetric, seed
    "one1_f5c3_dir_3batch": dict(n=56, f=5, c=3, n_edges=140, n_train=23, batch_size=9, symmetric=False, seed=3),
    "one1_f5c3_sym_1batch": dict(n=48, f=5, c=3, n_edges=110, n_train=20, batch_size=10000, symmetric=True, seed=4),
    "one1_f2c2_sym_3batch": dict(n=64, f=2, c=2, n_edges=160, n_train=26, batch_size=10, symmetric=True, seed=5),
    "one1_f2c2_dir_1batch": dict(n=52, f=2, c=2, n_edges=120, n_train=21, batch_size=10000, symmetric=False, seed=6),
}

LOOP_CASES = {
    # Banana's settings (stegcn_config.yaml:108-127): diag posterior, symmetric, momentum 0.9, weight decay 5e-4, clipping
    "steloop1_diag_sym": dict(structure="diag", symmetric=True, grad_norm=True, lr_adj=2.0, momentum=0.9, weight_decay=5e-4,
                              masked=False, f=2, c=2),
    "steloop1_kron_dir": dict(structure="kron", symmetric=False, grad_norm=False, lr_adj=0.05, momentum=0.5, weight_decay=0.0,
                              masked=True, f=5, c=3),
}


def laplace_of(ns, structure, model, prior):
    bl = ns.baselaplace
    if structure == "diag":
        return bl.DiagLaplace(model, "classification", prior_precision=prior)
    if structure == "kron":
        return bl.KronLaplace(model, "classification", prior_precision=prior)
    return bl.FullLaplace(model, "classification", prior_precision=prior, backend=ns.curvature.GGNInterface)


def grad_case(ns, torch, n, f, c, n_edges, n_train, batch_size, symmetric, seed, h=8):
    from torch.utils.data import DataLoader, TensorDataset

    from make_golden import reference_dense_adj

    g = torch.Generator().manual_seed(seed)
    hi = n - 1  # the last node is isolated
    ei = torch.randint(0, hi, (2, n_edges), generator=g)
    ei = torch.cat([ei, ei[:, : n_edges // 10], torch.arange(0, hi, 7).repeat(2, 1)], 1)  # duplicates, explicit self loops
    X = torch.randn(n, f, generator=g)
    adj0 = reference_dense_adj(torch, ei, n)
    perm = torch.randperm(n - 1, generator=g)
    train_idx = perm[:n_train].clone()
    train_idx[3] = train_idx[5]  # a repeated node id inside one batch
    train_idx[-1] = n - 1        # the isolated node is a batch sample
    train_y = torch.randint(0, c, (n_train,), generator=g)
    loader = DataLoader(TensorDataset(train_idx, train_y), batch_size=batch_size, shuffle=False)
    out = {"kind": "gcn", "symmetric": symmetric, "num_nodes": n, "num_layers": 1, "batch_size": batch_size,
           "edge_index": ei.numpy(), "X": X.numpy(), "train_idx": train_idx.numpy(), "train_y": train_y.numpy(),
           "prior": np.float64(PRIOR)}
    pick = None
    for structure in ("diag", "kron", "full"):
        torch.manual_seed(seed)  # the same weights for every posterior
        ste = ns.gnn_models.STEGCN(f, h, c, 1, X, adj0.clone(), dropout_p=0.5, threshold=0.5, symmetric=symmetric)
        ste.eval()
        if "W0" not in out:
            out["W0"] = ste.convs[0].lin.weight.detach().numpy().copy()
            out["b0"] = ste.convs[0].lin.bias.detach().numpy().copy()
            adj = ste.adj.detach()
            nzr, nzc = adj.nonzero(as_tuple=True)  # row-major order of the stored 0/1 matrix (with the self loops)
            out["adj_nz_row"], out["adj_nz_col"] = nzr.numpy(), nzc.numpy()
            with torch.no_grad():
                out["logits"] = ste(torch.arange(n)).numpy()
            dense01 = np.zeros((n, n), dtype=bool)
            dense01[out["adj_nz_row"], out["adj_nz_col"]] = True
            ner, nec = np.nonzero(~dense01)
            pick = np.random.default_rng(seed + 7).choice(len(ner), size=200, replace=False)
            out["ne_row"], out["ne_col"] = ner[pick], nec[pick]
        assert np.array_equal(out["W0"], ste.convs[0].lin.weight.detach().numpy())
        la = laplace_of(ns, structure, ste, PRIOR)
        la.fit(loader)
        neg = -la.log_marginal_likelihood()
        neg.backward()
        gr = ste.adj.grad.detach().numpy()
        assert np.count_nonzero(gr) > n, "the reference leaves a dense adj.grad"
        out[f"{structure}_neg_marglik"] = np.float64(float(neg))
        out[f"{structure}_vals"] = gr[out["adj_nz_row"], out["adj_nz_col"]].astype(np.float32)
        out[f"{structure}_ne_val"] = gr[out["ne_row"], out["ne_col"]].astype(np.float32)
        out[f"{structure}_loss"] = np.float64(float(la.loss))
        if structure == "kron":
            out["kron_n_blocks"] = len(la.H_facs.kfacs)
            for i, fs in enumerate(la.H_facs.kfacs):
                for j, hm in enumerate(fs):
                    out[f"kron_{i}_{j}"] = hm.detach().numpy().astype(np.float32)
        else:
            out[f"{structure}_H"] = la.H.detach().numpy().astype(np.float32)
    return out


def loop_case(ns, torch, structure, symmetric, grad_norm, lr_adj, momentum, weight_decay, masked, f, c, seed, n=64, h=8,
              n_edges=150, n_train=33, batch_size=12, prior=1.0, steps=3):
    from torch.utils.data import DataLoader, TensorDataset

    from make_golden import reference_dense_adj

    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, n_edges), generator=g)
    X = torch.randn(n, f, generator=g)
    adj0 = reference_dense_adj(torch, ei, n)
    perm = torch.randperm(n, generator=g)
    train_idx = perm[:n_train].clone()
    train_idx[3] = train_idx[5]
    train_y = torch.randint(0, c, (n_train,), generator=g)
    loader = DataLoader(TensorDataset(train_idx, train_y), batch_size=batch_size, shuffle=False)
    torch.manual_seed(seed)
    ste = ns.gnn_models.STEGCN(f, h, c, 1, X, adj0.clone(), dropout_p=0.5, threshold=0.5, symmetric=symmetric,
                               train_masked_update=masked, train_nodes=train_idx if masked else None)
    ste.eval()
    out = {"kind": "gcn", "symmetric": symmetric, "num_nodes": n, "batch_size": batch_size, "edge_index": ei.numpy(),
           "X": X.numpy(), "train_idx": train_idx.numpy(), "train_y": train_y.numpy(), "num_layers": 1, "structure": structure,
           "grad_norm": bool(grad_norm), "lr_adj": np.float64(lr_adj), "momentum": np.float64(momentum),
           "weight_decay": np.float64(weight_decay), "masked": bool(masked), "prior": np.float64(prior),
           "threshold": np.float64(0.5), "W0": ste.convs[0].lin.weight.detach().numpy().copy(),
           "b0": ste.convs[0].lin.bias.detach().numpy().copy(), "adj_init": ste.adj.detach().numpy().copy()}
    lap = laplace_of(ns, structure, ste, prior)
    lap.fit(loader)
    neg = -lap.log_marginal_likelihood()
    opt = torch.optim.SGD([ste.adj], lr=lr_adj, weight_decay=weight_decay, momentum=momentum)  # marglik_training.py:97-99
    negs, adjs, grads = [float(neg)], [], []
    for _ in range(steps):
        opt.zero_grad()
        neg.backward()
        grads.append(ste.adj.grad.detach().numpy().copy())  # (before clipping)
        if grad_norm:
            torch.nn.utils.clip_grad_norm_(ste.adj, max_norm=1.0)
        opt.step()
        lap.fit(loader)
        neg = -lap.log_marginal_likelihood()
        negs.append(float(neg))
        adjs.append(ste.adj.detach().numpy().copy())
    out["neg_marglik"] = np.array(negs, dtype=np.float64)
    out["adj_steps"] = np.stack(adjs).astype(np.float32)
    out["grad_steps"] = np.stack(grads).astype(np.float32)

    def eff(a):
        e = (a + a.T) / 2 if symmetric else a.copy()
        np.fill_diagonal(e, np.inf)  # the diagonal is overwritten on use
        return e

    margin = min(float(np.abs(eff(a) - 0.5).min()) for a in adjs)
    flips = [int(((eff(a) > 0.5) != (eff(b) > 0.5)).sum()) for a, b in zip([out["adj_init"]] + adjs[:-1], adjs)]
    return out, margin, flips


def main():
    import torch

    import ref_loader

    ns = ref_loader.load()
    os.makedirs(OUT, exist_ok=True)
    for name, kw in GRAD_CASES.items():
        out = grad_case(ns, torch, **kw)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB  "
              + "  ".join(f"{s}={float(out[s + '_neg_marglik']):.4f}" for s in ("diag", "kron", "full")))
    for name, kw in LOOP_CASES.items():
        for seed in range(200, 260):
            out, m, flips = loop_case(ns, torch, seed=seed, **kw)
            print(f"{name} seed {seed}: smallest distance from the threshold {m:.2e}, flips per step {flips}")
            if m >= MIN_MARGIN and sum(flips) > 0:
                break
        else:
            raise RuntimeError(f"{name}: no seed with margin >= {MIN_MARGIN} and at least one flipped entry")
        out["seed"] = seed
        out["margin"] = np.float64(m)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB  neg_marglik={list(out['neg_marglik'])}  flips per step={flips}")


if __name__ == "__main__":
    main()
