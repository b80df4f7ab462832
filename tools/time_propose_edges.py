"""Wall time of DiagLaplace.propose_edges(k = 1000) at the arxiv shape of bench.py (bench.make_workload("arxiv"): N = 169 343,
F = 128, H = 256, C = 40, 90 941 training nodes in batches of 10 000, a directed plain GCN) next to
DiagLaplace.neg_marglik_adj_grad(loader) -- the stored entries only -- on the same inputs; the band height and the number of
bands beside them.  Host clock around work that ends in a device synchronise; one warm-up call of each, then --reps timed calls
(the second timed call is skipped when the warm-up took longer than --budget seconds: the whole run shares a GPU visit).

    python tools/time_propose_edges.py [--workload arxiv] [--k 1000] [--reps 2] [--band-bytes B] [--out profiles/x.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import laplace_gnn_amd as lg  # noqa: E402
from laplace_gnn_amd.adjgrad import _band_plan  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="arxiv")
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--band-bytes", type=int, default=None)
    ap.add_argument("--budget", type=float, default=120.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    w, ei, X, train_idx, train_y = bench.make_workload(args.workload, dev)
    N, F, H, C = w["N"], w["F"], w["H"], w["C"]
    torch.manual_seed(0)
    model = lg.GCN(F, H, C, 2, X, ei, symmetric=False).to(dev).eval()
    loader = lg.TensorBatchLoader(train_idx.to(dev), train_y.to(dev), batch_size=w["batch"])
    la = lg.DiagLaplace(model, "classification", prior_precision=1.0)
    la.fit(loader)
    eng = model.engine
    height, bands = _band_plan(N, args.band_bytes, eng.workspace_limit)
    res = dict(workload=args.workload, N=N, F=F, H=H, C=C, n_train=int(train_idx.shape[0]), batch=w["batch"], nnz=eng.nnz, k=args.k,
               band_height=height, bands=len(bands), band_bytes=4 * N * min(height, N),
               gemm_flops=2 * N * N * (C + H + F + 1), device=torch.cuda.get_device_name(0))
    print(json.dumps(res), flush=True)
    sparse_ms, propose_ms = [], []
    _, warm = timed(lambda: la.neg_marglik_adj_grad(loader))
    print(f"neg_marglik_adj_grad warm-up {warm:.1f} ms", flush=True)
    for _ in range(args.reps):
        out, ms = timed(lambda: la.neg_marglik_adj_grad(loader))
        sparse_ms.append(ms)
        print(f"neg_marglik_adj_grad {ms:.1f} ms", flush=True)
    (_, pairs, grad), warm = timed(lambda: la.propose_edges(loader, args.k, band_bytes=args.band_bytes))
    print(f"propose_edges warm-up {warm:.1f} ms", flush=True)
    for _ in range(args.reps if warm <= 1e3 * args.budget else 1):
        (val, pairs, grad), ms = timed(lambda: la.propose_edges(loader, args.k, band_bytes=args.band_bytes))
        propose_ms.append(ms)
        print(f"propose_edges {ms:.1f} ms", flush=True)
    eng.check_async_errors()
    # the proposals against the candidates route on the same inputs
    gc = la.neg_marglik_adj_grad(loader, candidates=pairs)[3]
    res.update(neg_marglik_adj_grad_ms=sparse_ms, propose_edges_ms=propose_ms, propose_edges_warmup_ms=warm,
               returned=int(grad.shape[0]), grad_min=float(grad.min()), grad_max=float(grad.max()),
               worst_vs_candidates=float((gc - grad).abs().max()), neg_marglik=float(val))
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
