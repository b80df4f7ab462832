"""Per-call times of a ONE-layer STE-GCN structure-learning step: ``fit``, ``adj_backward`` under the
diagonal, Kronecker and full posterior, and ``apply_adj``, medians of device events after warm-up, at

* a Banana-like shape (gnn/configs/original/stegcn_config.yaml:108-127): N = 5300 points in the plane, F = 2, C = 2, a
  symmetric kNN graph (k = 10), all training nodes in one batch;
* a Cora-shaped one-layer model (bench.make_workload("cora"): N = 2708, F = 1433, C = 7), next to the TWO-layer model
  (H = 64) on the same graph and batches -- the one-layer chain is a subset of that work and must not take longer.

Writes one JSON document (default profiles/onelayer_step.json).

    python tools/time_onelayer_step.py [--reps 7] [--out profiles/onelayer_step.json] [--two-layer-full]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import laplace_gnn_amd as lg  # noqa: E402


def timed(fn, reps, warmup=2):
    ts = []
    for k in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if k >= warmup:
            ts.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "n": len(ts)}


def banana(dev, n=5300, k=10, seed=0):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, 2, (n,), generator=g)
    t = torch.rand(n, generator=g) * 3.14159
    X = torch.stack([torch.cos(t) + y * 1.0, torch.sin(t) * (1 - 2 * y) + y * 0.5], 1) + 0.15 * torch.randn(n, 2, generator=g)
    d = torch.cdist(X.to(dev), X.to(dev))
    d.fill_diagonal_(float("inf"))
    nb = d.topk(k, largest=False).indices.cpu()
    ei = torch.stack([torch.arange(n).repeat_interleave(k), nb.reshape(-1)])
    train_idx = torch.randperm(n, generator=g)[: n // 2]
    return ei, X, train_idx, y[train_idx]


def one_case(label, F, H, C, layers, X, ei, train_idx, train_y, batch, structures, reps, dev):
    out = {}
    loader = lg.TensorBatchLoader(train_idx.to(dev), train_y.to(dev), batch_size=batch)
    for structure in structures:
        torch.manual_seed(0)
        model = lg.STEGCN(F, H, C, layers, X, ei, symmetric=True).to(dev).eval()
        cls = {"diag": lg.DiagLaplace, "kron": lg.KronLaplace, "full": lg.FullLaplace}[structure]
        la = cls(model, "classification", prior_precision=1.0)
        r = {"fit": timed(lambda: la.fit(loader), reps)}

        def bwd():
            model.adj.grad = None
            model.adj_backward(la, loader)

        r["adj_backward"] = timed(bwd, reps)
        r["apply_adj"] = timed(model.apply_adj, reps)
        r["n_params"] = int(la.n_params)
        print(f"{label} {structure}: fit {r['fit']['median_ms']:.3f} ms  adj_backward {r['adj_backward']['median_ms']:.3f} ms  "
              f"apply_adj {r['apply_adj']['median_ms']:.3f} ms", flush=True)
        out[structure] = r
        model.engine.check_async_errors()
        model.engine.close()
        del la, model
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "onelayer_step.json"))
    ap.add_argument("--two-layer-full", action="store_true",
                    help="also time the two-layer full posterior at H = 64 (P = 92 231: a 34 GB Gamma)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0), "reps": args.reps}
    ei, X, tr, ty = banana(dev)
    doc["banana"] = {"shape": {"N": int(X.shape[0]), "F": 2, "C": 2, "knn": 10, "n_train": int(tr.numel()), "batches": 1},
                     "one_layer": one_case("banana 1-layer", 2, 64, 2, 1, X, ei, tr, ty, int(tr.numel()),
                                           ("diag", "kron", "full"), args.reps, dev)}
    w, ei, X, tr, ty = bench.make_workload("cora", dev)
    N, F, C = w["N"], w["F"], w["C"]
    doc["cora"] = {"shape": {"N": N, "E": w["E"], "F": F, "C": C, "n_train": int(tr.numel()), "batch": w["batch"]},
                   "one_layer": one_case("cora 1-layer", F, 64, C, 1, X, ei, tr, ty, w["batch"], ("diag", "kron", "full"),
                                         args.reps, dev),
                   "two_layer_H64": one_case("cora 2-layer H=64", F, 64, C, 2, X, ei, tr, ty, w["batch"],
                                             ("diag", "kron") + (("full",) if args.two_layer_full else ()), args.reps, dev)}
    one, two = doc["cora"]["one_layer"], doc["cora"]["two_layer_H64"]
    doc["cora"]["one_layer_not_slower"] = {s: one[s]["adj_backward"]["median_ms"] <= two[s]["adj_backward"]["median_ms"]
                                           for s in two}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(json.dumps(doc["cora"]["one_layer_not_slower"]))


if __name__ == "__main__":
    main()
