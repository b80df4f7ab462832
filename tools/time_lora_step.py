"""Wall time of one LoRASTEGCN structure-learning step at the Cora shape (bench.make_workload("cora"), r = 16,
lora_alpha = 16): fit, adj_backward (the all-pairs gradient + lgnn_lora_grad), the SGD step, apply_adj (lgnn_lora_threshold)
and the flips per step, under a Kronecker and a diagonal posterior; next to it the existing STEGCN adj_backward on the same
graph with every non-edge a candidate pair (the COO route).  The kernel-level split (dense_nt_kernel,
dense_diag_pair_kernel, ...) comes from a kernel-trace run of the same script (profiles/r05_lora_step.log).

    python tools/time_lora_step.py [--steps 3] [--no-stegcn]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import laplace_gnn_amd as lg  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--r", type=int, default=16)
    ap.add_argument("--no-stegcn", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    w, ei, X, train_idx, train_y = bench.make_workload("cora", dev)
    N, F, H, C = w["N"], w["F"], w["H"], w["C"]
    print(f"cora shape: N={N} E={w['E']} F={F} H={H} C={C} n_train={len(train_idx)} r={args.r}")
    loader = lg.TensorBatchLoader(train_idx.to(dev), train_y.to(dev), batch_size=w["batch"])
    for structure in ("kron", "diag"):
        torch.manual_seed(0)
        model = lg.LoRASTEGCN(F, H, C, 2, X, ei, r=args.r, lora_alpha=16.0, symmetric=True).to(dev).eval()
        cls = lg.KronLaplace if structure == "kron" else lg.DiagLaplace
        la = cls(model, "classification", prior_precision=1.0)
        opt = torch.optim.SGD([model.adj_lora_A, model.adj_lora_B], lr=1e-3, weight_decay=1e-4)
        _ = model.engine
        for k in range(args.steps + 1):  # step 0 warms up
            _, t_fit = timed(lambda: la.fit(loader))
            opt.zero_grad()
            _, t_bwd = timed(lambda: model.adj_backward(la, loader))
            _, t_step = timed(opt.step)
            flips, t_apply = timed(model.apply_adj)
            if k:
                print(f"{structure} step {k}: fit {t_fit:8.2f} ms  adj_backward {t_bwd:8.2f} ms  sgd {t_step:6.2f} ms  "
                      f"apply_adj {t_apply:6.2f} ms  flips {flips}  nnz {model.engine.nnz}")
    if not args.no_stegcn:
        torch.manual_seed(0)
        init = torch.zeros(N, N, dtype=torch.bool)
        init[ei[0], ei[1]] = True
        init = init | init.T
        init.fill_diagonal_(True)
        cand = (~init).nonzero().t().contiguous()
        model = lg.STEGCN(F, H, C, 2, X, ei, symmetric=True, candidates=cand).to(dev).eval()
        la = lg.KronLaplace(model, "classification", prior_precision=1.0)
        la.fit(loader)
        for k in range(2):
            model.adj.grad = None
            _, t = timed(lambda: model.adj_backward(la, loader))
            print(f"STEGCN kron adj_backward, all {cand.shape[1]} non-edges as candidates (call {k}): {t:9.2f} ms")


if __name__ == "__main__":
    main()
