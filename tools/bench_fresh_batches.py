#!/usr/bin/env python3
"""la.fit() of bench.py's workload with a loader that hands out FRESH tensors on every pass (clones of its slices), the way
torch's DataLoader collates: no batch ever repeats its identity, so the batch-structure cache never gets
past remembering tags.  Such a caller must not pay for the cache: compare this figure between two builds
(LGNN_LIB_DIR) or with LGNN_BATCH_CACHE_MB=0.  Prints one JSON line.

    python tools/bench_fresh_batches.py [--workload arxiv] [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class FreshLoader:
    def __init__(self, inner):
        self.inner = inner
        self.dataset = inner.dataset

    def __len__(self):
        return len(self.inner)

    def __iter__(self):
        for X, y in self.inner:
            yield X.clone(), y.clone()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="arxiv")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch

    import bench
    import laplace_gnn_amd as lg

    dev = torch.device("cuda", 0)
    w, ei, X, train_idx, train_y = bench.make_workload(args.workload, dev)
    torch.manual_seed(0)
    cls = lg.GraphSAGE if w.get("kind") == "sage" else lg.GCN
    model = cls(w["F"], w["H"], w["C"], w.get("layers", 2), X, ei, symmetric=True).to(dev)
    loader = FreshLoader(lg.TensorBatchLoader(train_idx.to(dev), train_y.to(dev), batch_size=w["batch"]))
    la = lg.Laplace(model, "classification", subset_of_weights="all", hessian_structure="kron")
    ms = []
    for k in range(args.warmup + args.steps):
        model.engine.invalidate()
        model.__dict__.pop("_lgnn_eig_cache", None)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        la.fit(loader)
        e1.record()
        torch.cuda.synchronize()
        if k >= args.warmup:
            ms.append(e0.elapsed_time(e1))
    print(json.dumps({"workload": args.workload, "loader": "fresh clones per pass", "steps": args.steps,
                      "ms_per_step_median": statistics.median(ms), "ms_per_step_min": min(ms), "ms_per_step_max": max(ms),
                      "batch_cache": model.engine.batch_cache_stats()}))


if __name__ == "__main__":
    main()
