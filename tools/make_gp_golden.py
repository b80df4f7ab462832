"""Goldens of the reference's own ``FunctionalLaplace`` (laplace/baselaplace.py:1922-2960) -> tests/golden/gp/*.npz.

Runs only where the reference tree exists (oracle/ref_loader.py loads its files by path; nothing of it is copied, only data
is stored).  The reference's class is built as ``FunctionalLaplace(model, lik, n_subset=M, backend=CurvlinopsGGN,
independent_outputs=..., prior_precision=0.7)`` on the reference's dense-adjacency models.

One workaround: the reference's constructor sets ``la.mean = parameters_to_vector(model.parameters())``, which contains the
dense ``adj``; ``fit`` then fails in ``_mean_scatter_term_batch`` (the Jacobians have the Laplace vector's width).  The tool
sets ``la.mean = parameters_to_vector(la.params).detach()`` before ``fit``; the reference computes everything else.

Cases (training ids distinct, ``n_subset * C < P`` asserted: K_MM then has full rank and a condition number near 1e4; with
``n_subset * C > P`` the reference's own fp32 scatter term is 5e-5 off its fp64 value and proves nothing):

* 2-layer GCN and GraphSAGE, (N, F, H, C) = (64, 12, 8, 3), 40 training ids, batch 7, n_subset 17 (three ragged batches);
* a GCN at (300, 37, 64, 7), 120 ids, batch 16, n_subset 45;
* a regression GCN and a GraphSAGE with ``res=True, norm="layer"`` at the small shape; a tanh GCN and a 3-layer GCN (H = 16)
  with batch 4 and n_subset 11: at n_subset 17 their K_MM has a condition number above 1e6 on every seed tried.
The tool asserts cond(K_MM) < 1e5 for every case.

Per case the inputs, then under the prefixes ``full_`` and ``indep_`` (``independent_outputs``): ``order`` (the subset),
``K_MM``, ``L``, ``mu``, ``loss``, ``log_det_ratio``, ``scatter``, ``marglik_pp07``, ``marglik_pp3``; on the 9 held-out nodes
``pred_idx``: ``f_mu``, ``f_var``, ``joint_cov`` (``full_`` only: the reference's einsum for the joint independent kernel does
not run), and for classification ``probit`` and ``mc`` (the latter with the stored ``eps`` [C, 32]).

    python tools/make_gp_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
OUT = os.path.join(ROOT, "tests", "golden", "gp")
PRIOR, PRIOR2 = 0.7, 3.0

#        name             kind    N    F   H  C  L  edges  ids  batch  M   likelihood        act     res    norm
CASES = [
    ("gcn_small",        "gcn",   64, 12,  8, 3, 2,  200,  40,  7,  17, "classification", "relu", False, None),
    ("sage_small",       "sage",  64, 12,  8, 3, 2,  200,  40,  7,  17, "classification", "relu", False, None),
    ("gcn_mid",          "gcn",  300, 37, 64, 7, 2,  900, 120, 16,  45, "classification", "relu", False, None),
    ("gcn_regression",   "gcn",   64, 12,  8, 3, 2,  200,  40,  7,  17, "regression",     "relu", False, None),
    ("gcn_tanh",         "gcn",   64, 12,  8, 3, 2,  200,  40,  4,  11, "classification", "tanh", False, None),
    ("gcn3_small",       "gcn",   64, 12, 16, 3, 3,  200,  40,  4,  11, "classification", "relu", False, None),
    ("sage_resln_small", "sage",  64, 12,  8, 3, 2,  200,  40,  7,  17, "classification", "relu", True, "layer"),
]


def build_case(ns, torch, spec, seed):
    from make_golden import reference_dense_adj

    name, kind, n, f, h, c, L, n_edges, n_train, batch, M, lik, act, res, norm = spec
    g = torch.Generator().manual_seed(100 + seed)
    ei = torch.randint(0, n - 2, (2, n_edges), generator=g)  # the last two nodes stay isolated
    ei = torch.cat([ei, ei[:, : n_edges // 10], torch.arange(0, n - 2, 7).repeat(2, 1)], 1)  # duplicates, self loops
    X = torch.randn(n, f, generator=g)
    adj0 = reference_dense_adj(torch, ei, n)
    torch.manual_seed(100 + seed)
    extras = dict(norm=norm, res=res) if (norm is not None or res) else {}
    if kind == "gcn":
        model = ns.gnn_models.GCN(f, h, c, L, X, adj0.clone(), dropout_p=0.5, symmetric=True, act=act, **extras)
    else:
        model = ns.gnn_models.GraphSAGE(f, h, c, L, X, adj0.clone(), num_sampled_nodes_per_hop=None, dropout_p=0.5,
                                        symmetric=True, act=act, **extras)
    if norm is not None:
        gn = torch.Generator().manual_seed(1100 + seed)
        with torch.no_grad():
            for nm in model.norms:
                nm.weight.copy_(0.5 + torch.rand(h, generator=gn))
                nm.bias.copy_(0.3 * torch.randn(h, generator=gn))
    model.eval()
    perm = torch.randperm(n, generator=g)
    train_idx, pred_idx = perm[:n_train].clone(), perm[n_train:n_train + 9].clone()
    assert len(set(train_idx.tolist())) == n_train
    if lik == "regression":
        train_y = torch.randn(n_train, c, generator=g)
    else:
        train_y = torch.randint(0, c, (n_train,), generator=g)
    out = {"kind": kind, "symmetric": True, "num_nodes": n, "batch_size": batch, "n_subset": M, "likelihood": lik, "act": act,
           "edge_index": ei.numpy(), "X": X.numpy(), "train_idx": train_idx.numpy(), "train_y": train_y.numpy(),
           "pred_idx": pred_idx.numpy(), "num_layers": L, "prior": np.float64(PRIOR), "prior2": np.float64(PRIOR2)}
    for l, conv in enumerate(model.convs):
        out[f"W{l}"], out[f"b{l}"] = conv.lin.weight.detach().numpy().copy(), conv.lin.bias.detach().numpy().copy()
    if extras:
        out["norm"], out["res"] = str(norm), bool(res)
        for l, lin in enumerate(model.res):
            out[f"Wr{l}"], out[f"br{l}"] = lin.weight.detach().numpy().copy(), lin.bias.detach().numpy().copy()
        if norm is not None:
            out["norm_eps"] = np.float64(model.norms[0].eps)
            for l, nm in enumerate(model.norms):
                out[f"norm_w{l}"], out[f"norm_b{l}"] = nm.weight.detach().numpy().copy(), nm.bias.detach().numpy().copy()
    with torch.no_grad():
        out["logits"] = model(torch.arange(n)).numpy().copy()
    return model, out


def f32(t):
    return t.detach().numpy().astype(np.float32)


def gp_results(ns, torch, model, case, independent):
    from torch.nn.utils import parameters_to_vector
    from torch.utils.data import DataLoader, TensorDataset

    bl = ns.baselaplace
    lik, M, C = case["likelihood"], int(case["n_subset"]), case[f"W{int(case['num_layers']) - 1}"].shape[0]
    loader = DataLoader(TensorDataset(torch.from_numpy(case["train_idx"]), torch.from_numpy(case["train_y"])),
                        batch_size=int(case["batch_size"]), shuffle=False)
    la = bl.FunctionalLaplace(model, lik, n_subset=M, backend=ns.curvature_curvlinops.CurvlinopsGGN,
                              independent_outputs=independent, prior_precision=PRIOR)
    la.mean = parameters_to_vector(la.params).detach()  # (the one workaround, see the module docstring)
    P = la.mean.numel()
    assert M * C < P, (M, C, P)
    la.fit(loader)
    out = {"order": la.train_loader.sampler.indices.numpy().astype(np.int64), "n_params": np.int64(P)}
    if independent:
        out["K_MM"] = np.stack([f32(k) for k in la.K_MM])
        out["L"] = np.stack([f32(l) for l in la.L])
    else:
        out["K_MM"], out["L"] = f32(la.K_MM), f32(la.L)
        out["cond"] = np.float64(np.linalg.cond(la.K_MM.detach().numpy().astype(np.float64)))
        assert out["cond"] < 1e5, out["cond"]
    out["mu"], out["loss"] = f32(la.mu), np.float64(float(la.loss))
    out["log_det_ratio"], out["scatter"] = np.float64(float(la.log_det_ratio)), np.float64(float(la.scatter))
    out["marglik_pp07"] = np.float64(float(la.log_marginal_likelihood()))
    out["marglik_pp3"] = np.float64(float(la.log_marginal_likelihood(prior_precision=torch.tensor(PRIOR2))))
    la.prior_precision = PRIOR
    la._build_Sigma_inv()
    pred = torch.from_numpy(case["pred_idx"])
    f_mu, f_var = la._glm_predictive_distribution(pred)
    out["f_mu"], out["f_var"] = f32(f_mu), f32(f_var)
    if not independent:
        out["joint_cov"] = f32(la._glm_predictive_distribution(pred, joint=True)[1])
    if lik == "classification":
        out["probit"] = f32(la(pred, link_approx="probit"))
        eps = torch.randn((C, 32), generator=torch.Generator().manual_seed(7))
        out["eps"] = eps.numpy()
        samples = la._glm_predictive_samples(f_mu, f_var, 32, False, torch.Generator().manual_seed(7))
        out["mc"] = f32(samples.mean(dim=0))
    return out


def main():
    import warnings

    import torch

    import ref_loader

    warnings.simplefilter("ignore")
    ns = ref_loader.load()
    os.makedirs(OUT, exist_ok=True)
    for seed, spec in enumerate(CASES):
        model, case = build_case(ns, torch, spec, seed)
        out = dict(case)
        for prefix, independent in (("full", False), ("indep", True)):
            out.update({f"{prefix}_{k}": v for k, v in gp_results(ns, torch, model, case, independent).items()})
        path = os.path.join(OUT, spec[0] + ".npz")
        np.savez_compressed(path, **out)
        print(f"{spec[0]}: {os.path.getsize(path) / 1024:.0f} KiB  P={int(out['full_n_params'])}  cond(K_MM)={float(out['full_cond']):.2e}"
              f"  marglik {float(out['full_marglik_pp07']):.4f} / indep {float(out['indep_marglik_pp07']):.4f}")


if __name__ == "__main__":
    main()
