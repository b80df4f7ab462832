"""Time of the kNN initial graph: ``lg.knn`` (csrc/knn.hip: Gram-form filter on the fp32 matrix cores, rerank
in the difference form, certificate, brute-force fallback) against a row-chunked ``torch.cdist`` + ``topk`` on the same GPU
(chunks of 8 192 rows, so that the N x N distances the baseline materialises fit), medians of device events after warm-up, at

* Cora (N = 2 708, F = 1 433, k = 3),
* a Banana-like shape (gnn/configs/original/stegcn_config.yaml:108-127: N = 5 300 points in the plane, F = 2, k = 10),
* arxiv (N = 169 343, F = 128, k = 3).

Every shape also reports ``num_fallback`` (rows the filter could not certify) and whether the two neighbour tables agree.
Writes one JSON document (default profiles/knn_graph.json).

    python tools/time_knn_graph.py [--reps 5] [--out profiles/knn_graph.json] [--shapes cora banana arxiv]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import laplace_gnn_amd as lg  # noqa: E402

CHUNK = 8192


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


def cdist_topk(X, k):
    """The baseline: distances of 8 192 rows at a time against all points, self masked, ``topk``."""
    N = X.shape[0]
    nbr = torch.empty(N, k, dtype=torch.int64, device=X.device)
    for r in range(0, N, CHUNK):
        d = torch.cdist(X[r:r + CHUNK], X)
        n = d.shape[0]
        d[torch.arange(n, device=X.device), torch.arange(r, r + n, device=X.device)] = float("inf")
        nbr[r:r + n] = d.topk(k, largest=False).indices
    return nbr


def banana(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, 2, (n,), generator=g)
    t = torch.rand(n, generator=g) * 3.14159
    return torch.stack([torch.cos(t) + y * 1.0, torch.sin(t) * (1 - 2 * y) + y * 0.5], 1) + 0.15 * torch.randn(n, 2, generator=g)


def shape_input(name):
    g = torch.Generator().manual_seed(0)
    if name == "cora":
        return torch.randn(2708, 1433, generator=g), 3
    if name == "banana":
        return banana(5300), 10
    return torch.randn(169_343, 128, generator=g), 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_graph.json"))
    ap.add_argument("--shapes", nargs="+", default=["cora", "banana", "arxiv"], choices=["cora", "banana", "arxiv"])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "baseline_chunk_rows": CHUNK}
    for name in args.shapes:
        X, k = shape_input(name)
        X = X.to(dev).contiguous()
        r = {"shape": {"N": int(X.shape[0]), "F": int(X.shape[1]), "k": k}}
        r["knn"] = timed(lambda: lg.knn(X, k), args.reps)
        nbr, _ = lg.knn(X, k)
        r["num_fallback"] = int(lg.knn.last_fallback_rows)
        r["cdist_topk"] = timed(lambda: cdist_topk(X, k), args.reps)
        base = cdist_topk(X, k)
        # (cdist's matrix-multiply form may order near-ties differently: a share, not an assertion)
        r["rows_equal_to_baseline"] = float((nbr == base).all(dim=1).float().mean())
        r["speedup"] = r["cdist_topk"]["median_ms"] / r["knn"]["median_ms"]
        print(f"{name}: knn {r['knn']['median_ms']:.3f} ms  cdist+topk {r['cdist_topk']['median_ms']:.3f} ms  "
              f"fallback rows {r['num_fallback']}  rows equal {r['rows_equal_to_baseline']:.4f}", flush=True)
        doc[name] = r
        del X, nbr, base
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
