"""dev: wall time of DiagLaplace.neg_marglik_adj_grad on an lg.GraphSAGE model with many candidate pairs -- the shape at which
sage_diag_pair_kernel's walk over the candidates shows (csrc/adjgrad_sage.hip): N = 2000, about 8 neighbours per node, F = 64,
H = 64, C = 7, one batch of 500 samples, K = 200000 candidates in shuffled order.
usage: python tools/time_sage_candidates.py [reps] [--save FILE.npy]   (one JSON line; FILE gets the candidates' gradient, for
comparing two builds on the same seeded inputs)"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import laplace_gnn_amd as lg

args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = int(args[0]) if args and args[0].isdigit() else 10
save = sys.argv[sys.argv.index("--save") + 1] if "--save" in sys.argv else None
N, F, H, C, M, K = 2000, 64, 64, 7, 500, 200_000
g = torch.Generator().manual_seed(3)
ei = torch.randint(0, N, (2, 8 * N), generator=g)
X = torch.randn(N, F, generator=g)
torch.manual_seed(0)
model = lg.GraphSAGE(F, H, C, 2, X, ei, symmetric=False).to("cuda").eval()
idx = torch.randperm(N, generator=g)[:M]
idx[7] = idx[3]
y = torch.randint(0, C, (M,), generator=g)
loader = lg.TensorBatchLoader(idx.cuda(), y.cuda(), batch_size=M)
la = lg.DiagLaplace(model, "classification", prior_precision=0.5)
la.fit(loader)
A = torch.zeros(N, N, dtype=torch.bool)
sr, sc = model.engine.export_adj()
A[sr.cpu(), sc.cpu()] = True
free = (~A).flatten().nonzero()[:, 0]
pick = free[torch.randperm(free.numel(), generator=g)[:K]]  # shuffled: the caller's order is arbitrary
cand = torch.stack([pick // N, pick % N]).cuda()
times = []
for rep in range(3 + reps):  # three warm-up calls
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = la.neg_marglik_adj_grad(loader, candidates=cand)
    torch.cuda.synchronize()
    if rep >= 3:
        times.append((time.perf_counter() - t0) * 1e3)
model.engine.check_async_errors()
gc = out[3].cpu().numpy()
if save:
    np.save(save, gc)
print(json.dumps({"shape": dict(N=N, F=F, H=H, C=C, M=M, K=int(cand.shape[1]), nnz=int(sr.numel())), "ms": [round(t, 3) for t in times],
                  "median_ms": round(sorted(times)[len(times) // 2], 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3),
                  "value": float(out[0]), "cand_abs_sum": float(np.abs(gc).sum()), "stored_abs_sum": float(out[2].abs().sum())}))
