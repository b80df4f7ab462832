"""Goldens of the reference's own GraphSAGE structure-learning loop -> tests/golden/sageloop/steloop_sage_*.npz (a folder of
their own: tests/test_oracle_golden.py replays every tests/golden/steloop_*.npz as a GCN loop).

Runs only where the reference tree exists (oracle/ref_loader.py loads its files by path; nothing of it is copied, only data
is stored).  The loop is ``oracle/make_golden.py::make_structure_loop``'s -- fit, ``neg_marglik.backward()``, optional
``clip_grad_norm_``, ``adj_optimizer.step()`` (SGD with momentum and weight decay), refit, three times
(gnn/marglik_training.py:197-224) -- run by the reference's ``STEGraphSAGE`` (gnn/models/models.py:121-183) with its
``KronLaplace`` / ``DiagLaplace``; the same shapes (N = 64, F = 12, H = 8, C = 3, 150 edges, 33 training ids with one
repeated, batches of 12, prior 1.0) and the same keys, plus ``kind = "sage"`` and the ``seed`` that was kept.

``STEGraphSAGE`` zeroes the diagonal of its dense ``adj`` once (models.py:135) and never overwrites it again, so the stored
``adj_steps`` / ``grad_steps`` carry a LEARNED diagonal.  A seed is kept -- the first at or after the one listed -- when

* after every step every effective value (``(adj + adj^T) / 2`` of a symmetric run) is at least 4e-4 away from the
  threshold (the margin of make_golden.py's loop fixtures: a comparison to 1e-4 then decides every edge the same way),
* a symmetric run has a diagonal entry switched on after step 0 or 1, so a later gradient and refit see a self loop,
* at least 50 off-diagonal entries flip over the run,
* a masked run moves no value between two training nodes.

    python tools/make_sage_loop_golden.py [fixture names]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.dont_write_bytecode = True
OUT = os.environ.get("LGNN_GOLDEN_OUT", os.path.join(ROOT, "tests", "golden", "sageloop"))
MIN_MARGIN = 4e-4
MIN_FLIPS = 50
SEED_TRIES = 40

LOOPS = {
    "steloop_sage_kron_sym": dict(structure="kron", seed=62, symmetric=True, grad_norm=True, lr_adj=8.0, momentum=0.9,
                                  weight_decay=5e-4),
    "steloop_sage_diag_sym": dict(structure="diag", seed=62, symmetric=True, grad_norm=True, lr_adj=8.0, momentum=0.9,
                                  weight_decay=5e-4),
    "steloop_sage_kron_dir_masked": dict(structure="kron", seed=51, symmetric=False, grad_norm=False, lr_adj=0.05, momentum=0.5,
                                         weight_decay=0.0, masked=True),
}


def fixture_conditions(out):
    """What a kept fixture satisfies (also re-checked on the committed files by tests/test_stegraphsage_host.py): returns a
    dict of the measured quantities, raises AssertionError with the failing one."""
    thr, sym = float(out["threshold"]), bool(out["symmetric"])
    n = int(out["num_nodes"])
    eye = np.eye(n, dtype=bool)
    eff = [0.5 * (a + a.T) if sym else a for a in [out["adj_init"]] + list(out["adj_steps"])]
    margin = min(float(np.abs(e - thr).min()) for e in eff[1:])
    assert margin >= MIN_MARGIN, f"margin {margin:.2e}"
    diag_on = [int((np.diag(e) > thr).sum()) for e in eff[1:]]
    if sym:
        assert diag_on[0] > 0 or diag_on[1] > 0, f"no diagonal entry on after step 0 or 1: {diag_on}"
    flips = sum(int((((a > thr) != (b > thr)) & ~eye).sum()) for a, b in zip(eff[:-1], eff[1:]))
    assert flips >= MIN_FLIPS, f"{flips} off-diagonal flips"
    if bool(out["masked"]):
        t = np.unique(out["train_idx"])
        for a in out["adj_steps"]:
            assert np.array_equal(a[np.ix_(t, t)], out["adj_init"][np.ix_(t, t)]), "a train-train value moved"
    return dict(margin=margin, diag_on=diag_on, offdiag_flips=flips)


def run_loop(ns, torch, structure, seed, symmetric, grad_norm, lr_adj, momentum, weight_decay, masked=False, steps=3, n=64,
             f=12, h=8, c=3, n_edges=150, n_train=33, batch_size=12, prior=1.0):
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
    ste = ns.gnn_models.STEGraphSAGE(f, h, c, 2, X, adj0.clone(), None, dropout_p=0.5, threshold=0.5, symmetric=symmetric,
                                     sign_grad=False, train_masked_update=masked, train_nodes=train_idx if masked else None)
    ste.eval()
    out = {"kind": "sage", "seed": np.int64(seed), "symmetric": symmetric, "num_nodes": n, "batch_size": batch_size,
           "edge_index": ei.numpy(), "X": X.numpy(), "train_idx": train_idx.numpy(), "train_y": train_y.numpy(),
           "num_layers": 2, "structure": structure, "grad_norm": bool(grad_norm), "lr_adj": np.float64(lr_adj),
           "momentum": np.float64(momentum), "weight_decay": np.float64(weight_decay), "sign_grad": False,
           "masked": bool(masked), "prior": np.float64(prior), "threshold": np.float64(0.5)}
    for l, conv in enumerate(ste.convs):
        out[f"W{l}"] = conv.lin.weight.detach().numpy().copy()
        out[f"b{l}"] = conv.lin.bias.detach().numpy().copy()
    out["adj_init"] = ste.adj.detach().numpy().copy()  # (symmetrised 0/1, diagonal zeroed once: models.py:135)
    bl = ns.baselaplace
    cls = bl.KronLaplace if structure == "kron" else bl.DiagLaplace
    lap = cls(ste, "classification", prior_precision=prior)
    lap.fit(loader)
    neg = -lap.log_marginal_likelihood()
    opt = torch.optim.SGD([ste.adj], lr=lr_adj, weight_decay=weight_decay, momentum=momentum)
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
    return out


def main():
    import torch

    import ref_loader

    torch.set_num_threads(8)
    ns = ref_loader.load()
    only = set(sys.argv[1:])
    os.makedirs(OUT, exist_ok=True)
    for name, kw in LOOPS.items():
        if only and name not in only:
            continue
        kw = dict(kw)
        first = kw.pop("seed")
        for seed in range(first, first + SEED_TRIES):
            out = run_loop(ns, torch, seed=seed, **kw)
            try:
                got = fixture_conditions(out)
            except AssertionError as e:
                print(f"{name}: seed {seed} dropped ({e})")
                continue
            path = os.path.join(OUT, name + ".npz")
            np.savez_compressed(path, **out)
            print(f"{name}: seed {seed}, {os.path.getsize(path) / 1024:.0f} KiB, neg_marglik={out['neg_marglik'].tolist()}, {got}")
            break
        else:
            raise SystemExit(f"{name}: no seed in [{first}, {first + SEED_TRIES}) meets the conditions")


if __name__ == "__main__":
    main()
