"""dev: wall time of the sampling predictive ``la(test_idx, pred_type="nn", link_approx="mc", n_samples=100)`` -- what mc_eval
reports with (gnn/marglik_training.py:341-353) -- on the arxiv-shaped and Cora-shaped workloads of bench.py, GCN and GraphSAGE,
KronLaplace and DiagLaplace.  Median of ``--reps`` calls after ``--warmup``, device-synchronised.

  --label NAME --json PATH    append one JSON line per measurement, tagged NAME.  Run it once from a checkout of the commit to
                              compare against and once from this one (the script measures the package beside it)
  --merge A.json B.json --out PATH
                              pair the lines of two such files (A: the earlier commit) and write one JSON document with the ratios

Where the engine has the one-pass route (csrc/sampled.hip) one more call runs with the library's event timing on: the time of
the first-layer tile kernel (first_layer_kernel) alone, and its rate against 2 |R| F' H S flop and the fp32 MFMA peak."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--label", default="this")
ap.add_argument("--json", default=None)
ap.add_argument("--workloads", default="arxiv,cora")
ap.add_argument("--kinds", default="gcn,sage")
ap.add_argument("--posteriors", default="kron,diag")
ap.add_argument("--samples", type=int, default=100)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--merge", nargs=2, default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()

KEY = ("workload", "kind", "posterior")

if args.merge:
    def lines(path):
        return {tuple(r[k] for k in KEY): r for r in map(json.loads, open(path)) if r.get("what") == "nn_predictive"}
    a, b = lines(args.merge[0]), lines(args.merge[1])
    rows = []
    for k in sorted(a.keys() & b.keys()):
        rows.append(dict(zip(KEY, k), parent_ms=a[k]["ms"], new_ms=b[k]["ms"], parent_over_new=a[k]["ms"] / b[k]["ms"],
                         **{f: b[k][f] for f in ("test_nodes", "needed_rows", "samples", "hidden_kernel_ms", "hidden_kernel_tflops",
                                                 "hidden_kernel_share_of_peak", "hidden_kernel_share_of_wall",
                                                 "max_abs_diff_of_two_calls") if f in b[k]}))
    doc = dict(what="la(test_idx, pred_type='nn', link_approx='mc', n_samples=S): median wall ms, parent commit vs this one",
               reps=args.reps, warmup=args.warmup, rows=rows)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))
    sys.exit(0)

import torch
import bench
import laplace_gnn_amd as lg

N_TEST = {"arxiv": 48_603, "cora": 1_000}  # the sizes of the datasets' public test splits


def emit(**rec):
    rec.update(label=args.label)
    print(json.dumps(rec), flush=True)
    if args.json:
        with open(args.json, "a") as f:
            f.write(json.dumps(rec) + "\n")


for name in args.workloads.split(","):
    w, ei, X, tri, try_ = bench.make_workload(name, "cuda")
    rest = torch.ones(w["N"], dtype=torch.bool)
    rest[tri] = False
    test_idx = rest.nonzero().squeeze(1)[:N_TEST[name]].cuda()
    for kind in args.kinds.split(","):
        torch.manual_seed(0)
        model = (lg.GCN if kind == "gcn" else lg.GraphSAGE)(w["F"], w["H"], w["C"], 2, X, ei, symmetric=True).to("cuda").eval()
        eng = model.engine
        loader = lg.TensorBatchLoader(tri.cuda(), try_.cuda(), batch_size=w["batch"])
        # |R|: the rows the evaluation nodes read (GCN: the columns of their rows of P; GraphSAGE: and themselves)
        r, c, _ = eng.export_propagation()
        mark = torch.zeros(w["N"], dtype=torch.bool, device="cuda")
        mark[test_idx] = True
        need = torch.zeros_like(mark)
        need[c[mark[r]]] = True
        if kind == "sage":
            need |= mark
        n_rows = int(need.sum())
        for post in args.posteriors.split(","):
            la = (lg.KronLaplace if post == "kron" else lg.DiagLaplace)(model, "classification", prior_precision=2.0)
            la.fit(loader)
            eps = torch.randn(args.samples, la.n_params, generator=torch.Generator().manual_seed(1)).cuda()

            def call():
                return la(test_idx, pred_type="nn", link_approx="mc", n_samples=args.samples, eps=eps)

            times, outs = [], []
            for rep in range(args.warmup + args.reps):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                out = call()
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
                outs.append(out)
                outs = outs[-2:]
            ms = statistics.median(times[args.warmup:])
            rec = dict(what="nn_predictive", workload=name, kind=kind, posterior=post, samples=args.samples,
                       test_nodes=int(test_idx.numel()), needed_rows=n_rows, ms=ms, min_ms=min(times[args.warmup:]),
                       max_abs_diff_of_two_calls=float((outs[0] - outs[1]).abs().max()),
                       rowsum_mean=float(out.sum(-1).mean()))
            if hasattr(eng, "sampled_forward") and la._nn_device_route():
                eng.enable_kernel_timing(True)
                call()
                torch.cuda.synchronize()
                k_ms = float(sum(eng.kernel_timing_launches()))
                eng.enable_kernel_timing(False)
                flop = 2.0 * n_rows * eng.in_dims[0] * w["H"] * args.samples
                rec.update(hidden_kernel_ms=k_ms, hidden_kernel_tflops=flop / (k_ms * 1e-3) / 1e12,
                           hidden_kernel_share_of_peak=flop / (k_ms * 1e-3) / 1e12 / bench.PEAK_MFMA_F32_TFLOPS,
                           hidden_kernel_share_of_wall=k_ms / ms)
            emit(**rec)
            del la, eps, outs, out
        eng.close()
        del model
        torch.cuda.empty_cache()
