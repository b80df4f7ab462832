"""Goldens of the reference's own subnetwork Laplace (laplace/subnetlaplace.py:15-233: ``FullSubnetLaplace`` /
``DiagSubnetLaplace``) -> tests/golden/subnet/*.npz.

Runs only where the reference tree exists (oracle/ref_loader.py loads its files by path; nothing of it is copied, only data
is stored).  Four of the existing small cases are rebuilt from their stored inputs (graph, features, weights, res / norm
state, batches) as the reference's dense-adjacency models; both posteriors are fitted with the reference's default backend
(``backend=None``: its constructor refuses every backend class passed explicitly, subnetlaplace.py:102-106) and prior
precision 0.7.

Subnetwork indices index the Laplace parameter vector (``la.mean``: ``named_parameters()`` without ``adj`` / ``norms``, each
parameter flattened row major).  Two index sets per case, stored under the prefixes ``rand_`` and ``struct_``:

* ``rand``: 24 indices drawn with a seeded generator, kept in the UNSORTED order of the draw;
* ``struct``: the whole first-layer bias, three rows of the first-layer weight, the last layer's bias.

Per set: ``indices``, ``H`` [S, S], ``diag_H`` [S], ``loss``, ``marglik_pp07`` / ``marglik_pp1`` (and ``diag_marglik_*``),
``eps`` [4, S] with the ``samples`` / ``diag_samples`` [4, P] they give at prior precision 0.7, ``glm_fvar`` and
``glm_probit`` on the case's ``pred_idx``.

    python tools/make_subnet_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "subnet")
PRIOR = 0.7
CASES = ("gcn_small_1batch_s0", "sage_small_1batch_s0", "gcn3_small_1batch_s0", "sage_resln_small_1batch_s0")


def reference_model(ns, torch, g):
    from make_golden import reference_dense_adj

    X, ei = torch.from_numpy(g["X"]), torch.from_numpy(g["edge_index"])
    L, n = int(g["num_layers"]), int(g["num_nodes"])
    f, h, c = X.shape[1], g["W0"].shape[0], g[f"W{L - 1}"].shape[0]
    extras = {}
    if "norm" in g.files:
        norm = str(g["norm"])
        extras = dict(norm=None if norm == "None" else norm, res=bool(g["res"]))
    adj0 = reference_dense_adj(torch, ei, n)
    if str(g["kind"]) == "gcn":
        model = ns.gnn_models.GCN(f, h, c, L, X, adj0, dropout_p=0.5, symmetric=bool(g["symmetric"]), **extras)
    else:
        model = ns.gnn_models.GraphSAGE(f, h, c, L, X, adj0, num_sampled_nodes_per_hop=None, dropout_p=0.5,
                                        symmetric=bool(g["symmetric"]), **extras)
    with torch.no_grad():
        for l, conv in enumerate(model.convs):
            conv.lin.weight.copy_(torch.from_numpy(g[f"W{l}"]))
            conv.lin.bias.copy_(torch.from_numpy(g[f"b{l}"]))
        for l, lin in enumerate(getattr(model, "res", [])):
            lin.weight.copy_(torch.from_numpy(g[f"Wr{l}"]))
            lin.bias.copy_(torch.from_numpy(g[f"br{l}"]))
        if extras.get("norm") is not None:
            for l, nm in enumerate(model.norms):
                nm.weight.copy_(torch.from_numpy(g[f"norm_w{l}"]))
                nm.bias.copy_(torch.from_numpy(g[f"norm_b{l}"]))
                if extras["norm"] == "batch":
                    nm.running_mean.copy_(torch.from_numpy(g[f"norm_rm{l}"]))
                    nm.running_var.copy_(torch.from_numpy(g[f"norm_rv{l}"]))
    model.eval()
    with torch.no_grad():  # the rebuilt model is the one the case was made from
        assert np.abs(model(torch.arange(n)).numpy() - g["logits"]).max() < 1e-5
    return model


def index_sets(torch, g, model, seed):
    """{prefix: int64 indices into the Laplace vector}."""
    names, off, P = {}, 0, 0
    for k, v in model.named_parameters():
        if v.requires_grad and "adj" not in k and "norms" not in k:
            names[k] = (P, tuple(v.shape))
            P += v.numel()
    assert P == int(g["n_params"])
    L = int(g["num_layers"])
    gen = torch.Generator().manual_seed(1000 + seed)
    rand = torch.randperm(P, generator=gen)[:24].clone()  # a permutation's head: distinct, unsorted
    assert not bool((rand[1:] > rand[:-1]).all())
    w0, (h, in0) = names["convs.0.lin.weight"]
    b0, _ = names["convs.0.lin.bias"]
    bl, (c,) = names[f"convs.{L - 1}.lin.bias"]
    rows = [5, 0, 2]  # three first-layer rows, not in increasing order
    struct = torch.cat([torch.arange(b0, b0 + h)] + [torch.arange(w0 + r * in0, w0 + (r + 1) * in0) for r in rows]
                       + [torch.arange(bl, bl + c)])
    return {"rand": rand, "struct": struct}


def subnet_case(ns, torch, sub, g, model, idx, seed):
    from torch.utils.data import DataLoader, TensorDataset

    loader = DataLoader(TensorDataset(torch.from_numpy(g["train_idx"]), torch.from_numpy(g["train_y"])),
                        batch_size=int(g["batch_size"]), shuffle=False)
    pred_idx = torch.from_numpy(g["pred_idx"])
    S = idx.numel()
    out = {"indices": idx.numpy().astype(np.int64), "prior": np.float64(PRIOR)}
    eps = torch.from_numpy(np.random.default_rng(seed + S).standard_normal((4, S)).astype(np.float32))
    out["eps"] = eps.numpy()

    lf = sub.FullSubnetLaplace(model, "classification", idx, prior_precision=PRIOR)
    lf.fit(loader)
    assert tuple(lf.H.shape) == (S, S)
    out["H"] = lf.H.detach().numpy().astype(np.float32)
    out["loss"] = np.float64(float(lf.loss))
    out["marglik_pp07"] = np.float64(float(lf.log_marginal_likelihood()))
    out["marglik_pp1"] = np.float64(float(lf.log_marginal_likelihood(prior_precision=torch.tensor(1.0))))
    lf.prior_precision = PRIOR
    out["samples"] = lf.assemble_full_samples(lf.mean_subnet[None, :] + eps @ lf.posterior_scale).detach().numpy().astype(
        np.float32)
    _, f_var = lf._glm_predictive_distribution(pred_idx)
    out["glm_fvar"] = f_var.detach().numpy().astype(np.float32)
    out["glm_probit"] = lf(pred_idx, pred_type="glm", link_approx="probit").detach().numpy().astype(np.float32)

    ld = sub.DiagSubnetLaplace(model, "classification", idx, prior_precision=PRIOR)
    ld.fit(loader)
    assert tuple(ld.H.shape) == (S,)
    out["diag_H"] = ld.H.detach().numpy().astype(np.float32)
    out["diag_marglik_pp07"] = np.float64(float(ld.log_marginal_likelihood()))
    out["diag_marglik_pp1"] = np.float64(float(ld.log_marginal_likelihood(prior_precision=torch.tensor(1.0))))
    ld.prior_precision = PRIOR
    out["diag_samples"] = ld.assemble_full_samples(
        ld.mean_subnet.reshape(1, S) + eps * ld.posterior_scale.reshape(1, S)).detach().numpy().astype(np.float32)
    out["diag_glm_probit"] = ld(pred_idx, pred_type="glm", link_approx="probit").detach().numpy().astype(np.float32)
    return out


def main():
    import importlib

    import torch

    import ref_loader

    ns = ref_loader.load()
    sub = importlib.import_module("laplace.subnetlaplace")
    os.makedirs(OUT, exist_ok=True)
    for seed, name in enumerate(CASES):
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        model = reference_model(ns, torch, g)
        out = {"case": name}
        for prefix, idx in index_sets(torch, g, model, seed).items():
            res = subnet_case(ns, torch, sub, g, model, idx, seed)
            if "fullla_H" in g.files:  # the reference's sub-block of its own full posterior
                sel = res["indices"]
                ref = g["fullla_H"][sel][:, sel]
                err = np.linalg.norm(res["H"] - ref) / np.linalg.norm(ref)
                assert err < 1e-5, (name, prefix, err)
            out.update({f"{prefix}_{k}": v for k, v in res.items()})
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB  "
              + "  ".join(f"{p}: S={len(out[p + '_indices'])} marglik={float(out[p + '_marglik_pp07']):.4f}"
                          for p in ("rand", "struct")))


if __name__ == "__main__":
    main()
