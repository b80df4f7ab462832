"""One structure-learning step of lg.STEGraphSAGE (and, on the same inputs, lg.STEGCN) at a Cora-like shape: N = 2708,
F = 1433, H = 64, C = 7, 5278 edges, 140 training nodes, the 2-hop non-edges of the training nodes as candidates (for the
GraphSAGE model also the training nodes' diagonal pairs): fit, adj_backward (= neg_marglik.backward()), clip + SGD step,
re-binarise + lgnn_update_adjacency (gnn/marglik_training.py:211-224).
usage: python tools/time_sage_structure_step.py [diag|kron]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import laplace_gnn_amd as lg

structure = sys.argv[1] if len(sys.argv) > 1 else "diag"
N, F, H, C, E, T = 2708, 1433, 64, 7, 5278, 140
g = torch.Generator().manual_seed(1)
ei = torch.randint(0, N, (2, E), generator=g)
ei = ei[:, ei[0] != ei[1]]
X = (torch.rand(N, F, generator=g) < 0.01).float()
tri = torch.randperm(N, generator=g)[:T]
try_ = torch.randint(0, C, (T,), generator=g)
A = torch.zeros(N, N)
A[ei[0], ei[1]] = 1
A = ((A + A.T) > 0).float()
two = ((A[tri] @ A) > 0) & (A[tri] == 0)  # reachable in two hops from a training node, not adjacent to it
two[torch.arange(T), tri] = False
r, c = two.nonzero(as_tuple=True)
cand = torch.stack([tri[r], c])
for name in ("stegcn", "stegraphsage"):
    torch.manual_seed(0)
    if name == "stegcn":
        model = lg.STEGCN(F, H, C, 2, X, ei, symmetric=True, candidates=cand)
    else:
        model = lg.STEGraphSAGE(F, H, C, 2, X, ei, None, symmetric=True, candidates=torch.cat([cand, torch.stack([tri, tri])], 1))
    model = model.to("cuda").eval()
    loader = lg.TensorBatchLoader(tri.cuda(), try_.cuda(), batch_size=10_000)
    la = (lg.DiagLaplace if structure == "diag" else lg.KronLaplace)(model, "classification")
    opt = torch.optim.SGD([model.adj], lr=0.8, weight_decay=5e-4, momentum=0.9)
    ts = {k: [] for k in ("fit", "backward", "step", "apply", "flips")}
    for it in range(12):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        la.fit(loader)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        opt.zero_grad()
        model.adj_backward(la, loader)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        torch.nn.utils.clip_grad_norm_(model.adj, max_norm=1.0)
        opt.step()
        torch.cuda.synchronize(); t3 = time.perf_counter()
        n = model.apply_adj()
        torch.cuda.synchronize(); t4 = time.perf_counter()
        if it >= 2:
            for k, v in zip(("fit", "backward", "step", "apply", "flips"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3, n)):
                ts[k].append(v)
    med = lambda v: sorted(v)[len(v) // 2]
    sr, sc = model.engine.export_adj()
    print(f"{name}/{structure}: tracked pairs {model.adj.numel()}, per step (median of 10; min - max): "
          + ", ".join(f"{lab} {1e3 * med(ts[k]):.3f} ms ({1e3 * min(ts[k]):.3f} - {1e3 * max(ts[k]):.3f})"
                      for lab, k in (("fit", "fit"), ("adj_backward", "backward"), ("clip + SGD", "step"),
                                     ("re-binarise + update_adjacency", "apply")))
          + f", entries flipped per step {ts['flips']}, self loops stored at the end {int((sr == sc).sum())}", flush=True)
    model.engine.check_async_errors()
    model.engine.close()
