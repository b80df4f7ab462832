"""dev: wall time of la(x) on every node of the arxiv shape, per link approximation (matrix-free routes of csrc/predictive.hip).

  --res / --norm {layer,batch}   build the models with res=True / that norm (the per-class table route, lgnn_glm_variance_ext)
  --baseline M                   also time the Jacobian-chunk route on an M-node subset (probit), alternating with the
                                 matrix-free route on the same subset, and report their agreement at that size
  --json PATH                    append one JSON line per measurement
  --train N                      fit on the first N training nodes only (the diagonal posterior of a res / norm model is fitted
                                 from plane-route Jacobians, 91 ms per sample: 90 941 of them take hours; what la(x) costs
                                 does not depend on N)
  --kinds / --posteriors / --links   restrict what is run (a profiler run wants one call)"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
import laplace_gnn_amd as lg

ap = argparse.ArgumentParser()
ap.add_argument("--res", action="store_true")
ap.add_argument("--norm", choices=["layer", "batch"], default=None)
ap.add_argument("--baseline", type=int, default=0)
ap.add_argument("--json", default=None)
ap.add_argument("--train", type=int, default=0)
ap.add_argument("--kinds", default="gcn,sage")
ap.add_argument("--posteriors", default="kron,diag")
ap.add_argument("--links", default="probit,bridge,bridge_norm,mc")
args = ap.parse_args()
LINKS = {"probit": {}, "bridge": {}, "bridge_norm": {}, "mc": {"diagonal_output": True, "n_samples": 100}}


def emit(**rec):
    rec.update(res=args.res, norm=args.norm, train=args.train or len(tri))
    print(json.dumps(rec), flush=True)
    if args.json:
        with open(args.json, "a") as f:
            f.write(json.dumps(rec) + "\n")


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


w, ei, X, tri, try_ = bench.make_workload("arxiv", "cuda")
if args.train:
    tri, try_ = tri[:args.train], try_[:args.train]
for kind in args.kinds.split(","):
    torch.manual_seed(0)
    model = (lg.GCN if kind == "gcn" else lg.GraphSAGE)(w["F"], w["H"], w["C"], 2, X, ei, symmetric=True, res=args.res,
                                                        norm=args.norm).to("cuda").eval()
    if args.norm:  # away from the defaults (weight 1, bias 0, running statistics 0 / 1)
        with torch.no_grad():
            for nm in model.norms:
                nm.weight.add_(0.3 * torch.randn_like(nm.weight)); nm.bias.add_(0.2 * torch.randn_like(nm.bias))
                if args.norm == "batch":
                    nm.running_mean.add_(0.3 * torch.randn_like(nm.running_mean)); nm.running_var.mul_(0.5 + torch.rand_like(nm.running_var))
    loader = lg.TensorBatchLoader(tri.cuda(), try_.cuda(), batch_size=w["batch"])
    for post in args.posteriors.split(","):
        cls = lg.KronLaplace if post == "kron" else lg.DiagLaplace
        la = cls(model, "classification", prior_precision=2.0)
        la.fit(loader)
        every = torch.arange(w["N"], device="cuda")
        for link in args.links.split(","):
            for rep in range(2):  # the second repetition is reported
                out, dt = timed(lambda: la(every, link_approx=link, **LINKS[link]))
            emit(what="all_nodes", kind=kind, posterior=post, link=link, nodes=w["N"], ms=dt * 1e3,
                 rowsum_mean=float(out.sum(-1).mean()))
        if args.baseline:
            sub = torch.randperm(w["N"], generator=torch.Generator().manual_seed(1))[:args.baseline].cuda()
            fast_route = la._glm_variance_matrix_free
            t_fast, t_jac = [], []
            for rep in range(2):  # alternating; the second pair is reported
                la._glm_variance_matrix_free = lambda x, out_map=None: None  # forces the Jacobian-chunk route
                (_, v_jac), dt = timed(lambda: la._glm_predictive_distribution(sub, diagonal_output=True)); t_jac.append(dt)
                la._glm_variance_matrix_free = fast_route
                (_, v_fast), dt = timed(lambda: la._glm_predictive_distribution(sub, diagonal_output=True)); t_fast.append(dt)
            emit(what="subset", kind=kind, posterior=post, nodes=args.baseline, jacobian_ms_per_node=t_jac[1] * 1e3 / args.baseline,
                 matrix_free_ms_per_node=t_fast[1] * 1e3 / args.baseline, rel=rel(v_fast, v_jac))
    model.engine.close()
