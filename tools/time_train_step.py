"""Time of one epoch of training steps (forward, cross entropy, backward, Adam step per batch) at the shapes bench.py defines:

  (a) the HIP path: ``lg.GCN`` / ``lg.GraphSAGE`` in train() mode (lgnn_train_forward / lgnn_train_backward, csrc/train.hip);
  (b) the only alternative on this stack: the same model restated with ``torch.sparse.mm`` on the propagation matrix from
      ``export_propagation()`` and torch autograd, same GPU, same process, same masks' distribution, alternating with (a).

Device events around synchronised work, ``--warmup`` epochs first, the median of ``--epochs`` (>= 20) epochs each; next to it one
``la.fit`` (KronLaplace) over the same loader, and the split-K weight-gradient kernel's bytes and flop from the shapes (its
time comes from a kernel-trace run of this script).  One JSON line per workload on stdout; ``--out`` also writes it to a file.

    python tools/time_train_step.py --workload arxiv [--epochs 20] [--warmup 3] [--out profiles/train_step_arxiv.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F_  # noqa: E402

import bench  # noqa: E402
import laplace_gnn_amd as lg  # noqa: E402


class TorchSparseGNN(torch.nn.Module):
    """(b): BaseGNN.forward (2-layer, plain) on a sparse propagation matrix, torch autograd."""

    def __init__(self, kind, P, X, model, p):
        super().__init__()
        self.kind, self.P, self.X, self.p = kind, P, X, p
        self.W = torch.nn.ParameterList(torch.nn.Parameter(c.lin.weight.detach().clone()) for c in model.convs)
        self.b = torch.nn.ParameterList(torch.nn.Parameter(c.lin.bias.detach().clone()) for c in model.convs)

    def forward(self, idx):
        x = self.X
        L = len(self.W)
        for l in range(L):
            if self.kind == "gcn":
                s = torch.sparse.mm(self.P, F_.linear(x, self.W[l], self.b[l]))
            else:
                s = F_.linear(torch.cat([x, torch.sparse.mm(self.P, x)], 1), self.W[l], self.b[l])
            if l < L - 1:
                x = F_.dropout(torch.relu(s), self.p, self.training)
        return s[idx]


def epoch(model, optimizer, loader):
    model.train()
    for idx, y in loader:
        f = model(idx)
        optimizer.zero_grad()
        loss = F_.cross_entropy(f, y)
        loss.backward()
        optimizer.step()
    return loss


def timed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="arxiv", choices=["arxiv", "arxiv_sage", "cora"])
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--p", type=float, default=0.5)
    ap.add_argument("--no-torch", action="store_true", help="only (a): for kernel-trace runs")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    w, ei, X, train_idx, train_y = bench.make_workload(args.workload, dev)
    kind = w.get("kind", "gcn")
    N, F, H, C = w["N"], w["F"], w["H"], w["C"]
    torch.manual_seed(0)
    cls = lg.GCN if kind == "gcn" else lg.GraphSAGE
    model = cls(F, H, C, 2, X, ei, dropout_p=args.p, symmetric=True).to(dev)
    loader = lg.TensorBatchLoader(train_idx.to(dev), train_y.to(dev), batch_size=w["batch"])
    r, c, v = model.engine.export_propagation()
    P = torch.sparse_coo_tensor(torch.stack([r, c]), v, (N, N)).coalesce().to_sparse_csr()
    ref = TorchSparseGNN(kind, P, model.X, model, args.p).to(dev)
    opt_a = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4)
    opt_b = torch.optim.Adam(ref.parameters(), lr=0.01, weight_decay=5e-4)
    runs = {"hip": lambda: epoch(model, opt_a, loader)}
    if not args.no_torch:
        runs["torch_sparse"] = lambda: epoch(ref, opt_b, loader)
    times = {k: [] for k in runs}
    for i in range(args.warmup + args.epochs):  # alternating (a) and (b)
        for k, fn in runs.items():
            t = timed_ms(fn)
            if i >= args.warmup:
                times[k].append(t)
    la = lg.KronLaplace(model, "classification", prior_precision=1.0)
    la.fit(loader)
    fit_ms = statistics.median(timed_ms(lambda: la.fit(loader)) for _ in range(5))
    mult = 2 if kind == "sage" else 1
    n_batches = len(list(loader))
    # split-K weight gradient per batch: D [N, out] and In [N, in (+ 1)] read once per 128 output columns resp. 128 rows
    wgrad = []
    for (k_in, w_out) in ((mult * F, H), (mult * H, C)):
        wgrad.append(dict(out_rows=w_out, in_cols=k_in, flop=2 * N * w_out * (k_in + 1),
                          min_bytes=4 * N * (w_out + k_in + 1)))
    res = dict(workload=args.workload, kind=kind, N=N, nnz=int(model.engine.nnz), F=F, H=H, C=C, n_train=int(len(train_idx)),
               batches=n_batches, p=args.p, epochs=args.epochs, warmup=args.warmup,
               hip_epoch_ms_median=statistics.median(times["hip"]), hip_epoch_ms_min=min(times["hip"]),
               hip_epoch_ms_max=max(times["hip"]), kron_fit_ms_median=fit_ms,
               epoch_share_of_fit=statistics.median(times["hip"]) / fit_ms, wgrad_per_batch=wgrad)
    if "torch_sparse" in times:
        tb = times["torch_sparse"]
        res.update(torch_sparse_epoch_ms_median=statistics.median(tb), torch_sparse_epoch_ms_min=min(tb),
                   torch_sparse_epoch_ms_max=max(tb), speedup_vs_torch_sparse=statistics.median(tb) / statistics.median(times["hip"]))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
