"""Goldens of the reference's joint GLM predictive (laplace/baselaplace.py:1123-1158 with ``joint=True``, i.e.
``functional_covariance``: KronLaplace :1638-1644, DiagLaplace :1905-1910, FullLaplace :1491-1494) -> tests/golden/joint/*.npz.

Runs only where the reference tree exists (oracle/ref_loader.py loads its files by path; nothing of it is copied, only data
is stored).  The graphs, features, weights and training sets are those of existing fixtures -- ``gcn_small_1batch_s0``,
``sage_small_1batch_s0``, ``gcn_resln_small_1batch_s0`` (classification) and ``gp/gcn_regression`` (regression) -- rebuilt as the
reference's dense-adjacency models.  Per fixture the reference's ``KronLaplace``, ``DiagLaplace`` (default backend) and
``FullLaplace`` (``GGNInterface``, as the existing full goldens) are fitted with ``prior_precision=0.7`` (regression:
``sigma_noise=0.7`` too) and, for six prediction nodes ``pred`` -- four held-out nodes, one of them twice, and an isolated
node (where the graph has none: its node of lowest degree, printed) -- the tool stores under the prefixes ``kron_`` / ``diag_`` /
``full_``:

* ``f_mu_joint`` [6 C] and ``f_cov`` [6 C, 6 C]: ``la._glm_predictive_distribution(pred, joint=True)``;
* regression: ``call_mu`` / ``call_cov``: what ``la(pred, joint=True)`` returns.

    python tools/make_joint_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "joint")
PRIOR, SIGMA = 0.7, 0.7
SOURCES = ["gcn_small_1batch_s0", "sage_small_1batch_s0", "gcn_resln_small_1batch_s0", os.path.join("gp", "gcn_regression")]


def reference_model(ns, torch, g):
    from make_golden import reference_dense_adj

    kind, L = str(g["kind"]), int(g["num_layers"])
    X, ei = torch.from_numpy(g["X"]), torch.from_numpy(g["edge_index"])
    n, f, h, c = X.shape[0], X.shape[1], g["W0"].shape[0], g[f"W{L - 1}"].shape[0]
    extras = {}
    if "res" in g.files or "norm" in g.files:
        norm = str(g["norm"]) if "norm" in g.files else "None"
        extras = dict(norm=None if norm == "None" else norm, res=bool(g["res"]) if "res" in g.files else False)
    if "act" in g.files:
        extras["act"] = str(g["act"])
    adj0 = reference_dense_adj(torch, ei, n)
    if kind == "gcn":
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
    model.eval()
    with torch.no_grad():  # the rebuilt model is the fixture's
        assert np.abs(model(torch.arange(n)).numpy() - g["logits"]).max() < 1e-5
    return model


def prediction_nodes(g):
    """Four nodes outside the training set, the second of them again, and an isolated node (or the one of lowest degree)."""
    n, ei = int(g["num_nodes"]), g["edge_index"]
    deg = np.zeros(n, np.int64)
    off = ei[0] != ei[1]
    np.add.at(deg, ei[0][off], 1)
    np.add.at(deg, ei[1][off], 1)
    lone = int(np.argmin(deg))  # (first of the minima)
    train = set(g["train_idx"].tolist())
    held = [v for v in range(n) if v not in train and v != lone][:4]
    return np.array([held[0], held[1], held[2], held[1], held[3], lone], np.int64), int(deg[lone])


def f32(t):
    return t.detach().numpy().astype(np.float32)


def main():
    import warnings

    import torch
    from torch.utils.data import DataLoader, TensorDataset

    import ref_loader

    warnings.simplefilter("ignore")
    ns = ref_loader.load()
    bl = ns.baselaplace
    os.makedirs(OUT, exist_ok=True)
    for src in SOURCES:
        g = np.load(os.path.join(GOLDEN, src + ".npz"))
        lik = str(g["likelihood"]) if "likelihood" in g.files else "classification"
        model = reference_model(ns, torch, g)
        pred_np, lone_deg = prediction_nodes(g)
        pred = torch.from_numpy(pred_np)
        loader = DataLoader(TensorDataset(torch.from_numpy(g["train_idx"]), torch.from_numpy(g["train_y"])),
                            batch_size=int(g["batch_size"]), shuffle=False)
        kw = dict(prior_precision=PRIOR)
        if lik == "regression":
            kw["sigma_noise"] = SIGMA
        out = {"source": src.replace(os.sep, "/"), "likelihood": lik, "pred": pred_np, "prior": np.float64(PRIOR),
               "sigma_noise": np.float64(SIGMA if lik == "regression" else 1.0)}
        for prefix, make in (("kron", lambda: bl.KronLaplace(model, lik, **kw)), ("diag", lambda: bl.DiagLaplace(model, lik, **kw)),
                             ("full", lambda: bl.FullLaplace(model, lik, backend=ns.curvature.GGNInterface, **kw))):
            la = make()
            la.fit(loader)
            f_mu, f_cov = la._glm_predictive_distribution(pred, joint=True)
            C = int(la.n_outputs)
            assert f_mu.shape == (6 * C,) and f_cov.shape == (6 * C, 6 * C)
            out[f"{prefix}_f_mu_joint"], out[f"{prefix}_f_cov"] = f32(f_mu), f32(f_cov)
            if lik == "regression":
                mu, cov = la(pred, joint=True)
                assert cov.shape == (6 * C, 6 * C)
                out[f"{prefix}_call_mu"], out[f"{prefix}_call_cov"] = f32(mu), f32(cov)
        name = os.path.basename(src)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB  {lik}  pred {pred_np.tolist()} (degree of the last: {lone_deg})  "
              f"|f_cov| kron {np.abs(out['kron_f_cov']).max():.3e} diag {np.abs(out['diag_f_cov']).max():.3e} "
              f"full {np.abs(out['full_f_cov']).max():.3e}")


if __name__ == "__main__":
    main()
